"""The yardsticks of the reward normaliser (csrc/wsmg_pg_rollout.hip, wsmgmap.rollout.RewardNormalizer) and their case table.

`reward_norm_ref` is the return path of baselines' `VecNormalize`, restated step by step in numpy float64 (baselines is not a
dependency and there is no golden).  state = {mean, var, count, ret[N]}; for s = first_row .. T-1:

    ret = ret * gamma + rewards[s]
    bmean = sum_n ret / N;  bM2 = sum_n (ret - bmean)^2         (two passes; both sums in index order)
    delta = bmean - mean;  tot = count + N
    mean = mean + delta * N / tot;  var = (var * count + bM2 + delta * delta * count * N / tot) / tot;  count = tot
    out[s] = float32(clip(rewards[s] / sqrt(var + eps), -clip, +clip))
    ret = ret * masks[s+1]

and with update=False only the `out` line with the stored var.  gamma, clip and eps are seen as the float32 numbers a launch is
handed (pg_util.f32_scalar), so that a kernel and this loop differ by arithmetic only: by the order of the two sums over n.

`reward_norm_welford` is an independent restatement for the CPU tests: Python floats, element by element, the running moments
advanced one value at a time by Welford's update (mathematically the same merge, rounded differently).

The bars of the GPU tests are derived here (`state_bars`, `assert_outputs`), not tuned: see their docstrings."""
import numpy as np
import torch

import rollout_util as ru
from pg_util import f32_scalar

PREFETCH = 8           # NORM_PF of csrc/wsmg_pg_rollout.hip: the steps the walk's row loads run ahead
GAMMA, CLIP, EPS, COUNT0 = 0.99, 10.0, 1e-8, 1e-4
STEPS = (1, 2, PREFETCH - 1, PREFETCH + 1, 40)
# every N of rollout_util.ENVS with two of the T (so each T meets small and large N; 1 x 1 is the first)
SHAPES = tuple((STEPS[i % len(STEPS)], n) for i, n in enumerate(ru.ENVS)) + tuple((STEPS[(i + 2) % len(STEPS)], n) for i, n in enumerate(ru.ENVS))
KINDS = ("randn", "scaled_100", "zeros", "nan_3_2")
# "scaled_100" starts from a normaliser built with this count0: the initial var = 1 then outweighs the first rows (N values each), and
# rewards of order 100 are clipped there.  (With the default count0 the first row's own variance takes over at once and an output
# is of order one whatever the scale of the rewards.)
SCALED_COUNT0 = 1e4


def fresh_state(N, count0=COUNT0):
    st = np.zeros(3 + N, dtype=np.float64)
    st[1], st[2] = 1.0, f32_scalar(count0)
    return st


def case_count0(kind):
    return SCALED_COUNT0 if kind == "scaled_100" else COUNT0


def inputs(T, N, mask_kind="random_20", kind="randn", seed=0):
    """(rewards [T, N, 1], masks [T+1, N, 1]) float32 on the CPU."""
    g = torch.Generator(); g.manual_seed(7919 * T + 31 * N + seed + 13 * ru.MASKS.index(mask_kind))
    rewards = torch.randn(T, N, 1, generator=g)
    masks = ru.make_masks(mask_kind, T, N, g)
    if kind == "scaled_100":
        rewards = rewards * 100.0
    elif kind == "zeros":
        rewards = torch.zeros(T, N, 1)
    elif kind == "nan_3_2":
        rewards[3, 2] = float("nan")
    else:
        assert kind == "randn"
    return rewards, masks


def _np2(t):
    return np.array(torch.as_tensor(t).detach().cpu().reshape(t.shape[0], -1).numpy())


def reward_norm_ref(rewards, masks, state, gamma=GAMMA, clip=CLIP, eps=EPS, first_row=0, update=True):
    """-> (out float32 [T, N] with rows < first_row zero, new state float64 [3 + N]); the arguments are not modified."""
    r, m = _np2(rewards).astype(np.float64), _np2(masks).astype(np.float64)
    T, N = r.shape
    st = np.array(torch.as_tensor(state).detach().cpu().numpy(), dtype=np.float64)
    gamma, clip, eps = f32_scalar(gamma), f32_scalar(clip), f32_scalar(eps)
    out = np.zeros((T, N), dtype=np.float32)
    with np.errstate(all="ignore"):
        if not update:
            out[first_row:] = np.clip(r[first_row:] / np.sqrt(st[1] + eps), -clip, clip).astype(np.float32)
            return out, st
        mean, var, count, ret = st[0], st[1], st[2], st[3:].copy()
        for s in range(first_row, T):
            ret = ret * gamma + r[s]
            bmean = np.cumsum(ret)[-1] / N
            d = ret - bmean
            bm2 = np.cumsum(d * d)[-1]
            delta, tot = bmean - mean, count + N
            mean = mean + delta * N / tot
            var = (var * count + bm2 + delta * delta * count * N / tot) / tot
            count = tot
            out[s] = np.clip(r[s] / np.sqrt(var + eps), -clip, clip).astype(np.float32)
            ret = ret * m[s + 1]
    new = np.empty_like(st)
    new[0], new[1], new[2], new[3:] = mean, var, count, ret
    return out, new


def reward_norm_welford(rewards, masks, state, gamma=GAMMA, clip=CLIP, eps=EPS, first_row=0):
    """(out float64 [T, N] NOT rounded to float32, new state): Python floats, one value at a time."""
    r, m = _np2(rewards).astype(np.float64).tolist(), _np2(masks).astype(np.float64).tolist()
    T, N = len(r), len(r[0])
    st = [float(v) for v in torch.as_tensor(state).detach().cpu().numpy()]
    gamma, clip, eps = f32_scalar(gamma), f32_scalar(clip), f32_scalar(eps)
    mean, count, ret = st[0], st[2], st[3:]
    m2 = st[1] * count
    out = [[0.0] * N for _ in range(T)]
    for s in range(first_row, T):
        for n in range(N):
            x = ret[n] = ret[n] * gamma + r[s][n]
            count += 1.0
            d = x - mean
            mean += d / count
            m2 += d * (x - mean)
        sd = (m2 / count + eps) ** 0.5
        for n in range(N):
            v = r[s][n] / sd
            out[s][n] = v if v != v else min(max(v, -clip), clip)
            ret[n] *= m[s + 1][n]
    return np.array(out), np.array([mean, m2 / count, count] + ret)


# ----------------------------------------------------------------------------- the bars
def state_bars(ref_state, N, steps):
    """Absolute bars {mean, var, ret [N]} for a state advanced by `steps` rows from a state both sides shared.  A kernel and the
    oracle perform the same float64 operations except for the ORDER of two sums of N terms per step; a sum of N terms taken in any
    order is within (N - 1) 2^-53 (relative to the sum of magnitudes) of any other, the handful of operations behind it add a few
    2^-53 more (16 is generous), and the differences of `steps` steps add up: (N + 16) steps 2^-53, relative to |mean| + sqrt(var)
    for the mean (the scale of the values `ret` whose sum moves it) and to their own magnitudes for var and ret.  Times 4 for slack.
    `count` has no bar: it is formed by the same additions and must be equal."""
    rel = 4.0 * (N + 16) * steps * 2.0 ** -53
    mean, var = float(ref_state[0]), float(ref_state[1])
    return dict(mean=rel * (abs(mean) + abs(var) ** 0.5), var=rel * abs(var), ret=rel * np.abs(ref_state[3:]))


def assert_state(tag, got, ref, N, steps, log=print):
    """got, ref: float64 [3 + N] (tensor or array).  NaNs must sit where the oracle's do.  Prints the figures, then asserts."""
    got = np.array(torch.as_tensor(got).detach().cpu().numpy(), dtype=np.float64)
    assert got.shape == ref.shape == (3 + N,), (tag, got.shape, ref.shape)
    assert np.array_equal(np.isnan(got), np.isnan(ref)), f"{tag}: NaN pattern of the state"
    assert got[2] == ref[2] or (np.isnan(got[2]) and np.isnan(ref[2])), f"{tag}: count {got[2]!r} is not the oracle's {ref[2]!r}"
    rel = 4.0 * (N + 16) * steps * 2.0 ** -53
    if np.isnan(ref[:2]).any():          # a NaN reward: the moments are NaN on both sides; the other columns' carries still compare
        ok = ~np.isnan(ref[3:])
        assert (np.abs(got[3:] - ref[3:])[ok] <= rel * np.abs(ref[3:])[ok]).all(), f"{tag}: ret beside a NaN"
        return
    bars = state_bars(ref, N, steps)
    e_mean, e_var = abs(got[0] - ref[0]), abs(got[1] - ref[1])
    ok = ~np.isnan(ref[3:])
    e_ret = np.abs(got[3:] - ref[3:])[ok]
    worst = float((e_ret - bars["ret"][ok]).max()) if ok.any() else 0.0
    log(f"{tag}: mean error {e_mean:.3e} bar {bars['mean']:.3e};  var error {e_var:.3e} bar {bars['var']:.3e};  "
        f"ret max error {float(e_ret.max()) if ok.any() else 0.0:.3e} (worst error - bar {worst:.3e})")
    assert e_mean <= bars["mean"] and e_var <= bars["var"] and (e_ret <= bars["ret"][ok]).all(), tag


def assert_outputs(tag, got, ref, clip=CLIP):
    """got: float32 tensor, ref: the oracle's float32 array (one element count).  Each output is formed in float64 and rounded
    once, from a var within ~1e-13 of the oracle's: it is the oracle's float32 or its neighbour (one ulp).  An element at the clip is
    a float32 constant on both sides: exact.  NaN stays NaN."""
    g = np.array(torch.as_tensor(got).detach().cpu().reshape(-1).numpy())
    r = ref.reshape(-1)
    assert g.dtype == r.dtype == np.float32 and g.shape == r.shape, (tag, g.dtype, g.shape, r.shape)
    assert np.array_equal(np.isnan(g), np.isnan(r)), f"{tag}: NaN pattern of the outputs"
    ok = ~np.isnan(r)
    at_clip = ok & (np.abs(r) == np.float32(f32_scalar(clip)))
    assert np.array_equal(g[at_clip], r[at_clip]), f"{tag}: an element at the clip is not exact"
    with np.errstate(all="ignore"):
        ulp = np.spacing(np.abs(r[ok]))
    assert (np.abs(g[ok].astype(np.float64) - r[ok].astype(np.float64)) <= ulp.astype(np.float64)).all(), f"{tag}: more than one ulp"
    return int(at_clip.sum())


def same_bits64(a, b):
    a = torch.as_tensor(a).detach().cpu().contiguous().reshape(-1)
    b = torch.as_tensor(b).detach().cpu().contiguous().reshape(-1)
    return a.dtype == b.dtype == torch.float64 and a.shape == b.shape and torch.equal(a.view(torch.int64), b.view(torch.int64))
