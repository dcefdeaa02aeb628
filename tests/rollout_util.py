"""The yardsticks of the rollout's returns and advantages (csrc/wsmg_pg_rollout.hip, wsmgmap/rollout.py) and their case table.

`gae_ref` is habitat-baselines' `RolloutStorage.compute_returns` followed by `PPO.get_advantages`, restated as the torch loop a user
writes today (habitat is not a dependency), on [T, N, 1] tensors with Python-float gamma and tau:

    use_gae:   value_preds[T] = next_value;  gae = 0
               for s = T-1 .. 0:  delta = rewards[s] + gamma * value_preds[s+1] * masks[s+1] - value_preds[s]
                                  gae = delta + gamma * tau * masks[s+1] * gae;   returns[s] = gae + value_preds[s]
    else:      returns[T] = next_value;  for s = T-1 .. 0:  returns[s] = returns[s+1] * gamma * masks[s+1] + rewards[s]
    adv = returns[:T] - value_preds[:T];   adv_norm = (adv - adv.mean()) / (adv.std() + eps)

In float32 on the CPU it is the BIT yardstick of `returns`, `adv` and `value_preds[T]`; in float64 it is the oracle of the normalised
advantages and their statistics, whose bar is tests/pg_util.py's rule (4 x the float32 loop's own error, floor 1e-6 x max |oracle|).
The float64 run sees gamma, gamma * tau and eps as the float32 numbers the kernel is handed (pg_util.f32_scalar), so that the two
differ by arithmetic only.  `gae_numpy` is an independent elementwise float32 restatement (no torch) for the CPU tests."""
import numpy as np
import torch

from pg_util import f32_scalar

EPS = 1e-5
PREFETCH = 16          # GAE_PF of csrc/wsmg_pg_rollout.hip: the steps its row loads run ahead of the chain
GAMMA_TAU = ((0.99, 0.95), (1.0, 1.0), (0.9, 0.0), (0.0, 0.95))
MASKS = ("ones", "zeros", "zero_row_1", "zero_row_T", "random_20", "one_env_masked")
ENVS = (1, 2, 8, 63, 64, 65, 255, 256, 257, 1024)
# (T, N): every T from 1 to two past the prefetch depth, each with the next N of ENVS (so every N meets a small T, 1024 included);
# then the long rollouts and the workgroup's column edges at a T that wraps the register ring more than once
SHAPES = tuple((T, ENVS[(T - 1) % len(ENVS)]) for T in range(1, PREFETCH + 3)) + (
    (64, 8), (200, 65), (200, 1), (64, 257), (33, 256), (35, 255), (3, 1024), (17, 1024), (2, 1))


def make_masks(kind, T, N, g):
    m = torch.ones(T + 1, N, 1)
    if kind == "zeros":
        m.zero_()
    elif kind == "zero_row_1":
        m[min(1, T)] = 0
    elif kind == "zero_row_T":
        m[T] = 0
    elif kind == "random_20":
        m = (torch.rand(T + 1, N, 1, generator=g) >= 0.2).float()
    elif kind == "one_env_masked":
        m[:, 0] = 0          # (with N = 1 the only environment; else beside live ones)
    else:
        assert kind == "ones"
    return m


def inputs(T, N, kind="random_20", seed=0):
    """(rewards [T,N,1], value_preds [T+1,N,1] with row T a sentinel, masks [T+1,N,1], next_value [N,1]) float32 on the CPU."""
    g = torch.Generator(); g.manual_seed(100003 * T + 101 * N + seed + 17 * MASKS.index(kind))
    rewards = torch.randn(T, N, 1, generator=g)
    value_preds = torch.randn(T + 1, N, 1, generator=g)
    value_preds[T] = 123.0
    next_value = torch.randn(N, 1, generator=g)
    return rewards, value_preds, make_masks(kind, T, N, g), next_value


def gae_ref(rewards, value_preds, masks, next_value, gamma, tau, use_gae, dtype=torch.float32, eps=EPS, returns=None):
    """-> dict(returns [T+1,N,1], value_preds [T+1,N,1], adv, adv_norm [T,N,1], stats [2] = {mean, std}) in `dtype`; the inputs are
    not modified.  returns: the tensor's earlier content (row T survives GAE), default NaN."""
    T = rewards.shape[0]
    if dtype == torch.float32:
        gt = gamma * tau
    else:
        gamma, gt, eps = f32_scalar(gamma), f32_scalar(gamma * tau), f32_scalar(eps)
    c = lambda t: t.detach().clone().to(dtype)      # noqa: E731
    rewards, value_preds, masks, next_value = c(rewards), c(value_preds), c(masks), c(next_value).reshape(value_preds[T].shape)
    returns = torch.full_like(value_preds, float("nan")) if returns is None else c(returns)
    if use_gae:
        value_preds[T] = next_value
        gae = 0
        for s in reversed(range(T)):
            delta = rewards[s] + gamma * value_preds[s + 1] * masks[s + 1] - value_preds[s]
            gae = delta + gt * masks[s + 1] * gae
            returns[s] = gae + value_preds[s]
    else:
        returns[T] = next_value
        for s in reversed(range(T)):
            returns[s] = returns[s + 1] * gamma * masks[s + 1] + rewards[s]
    adv = returns[:T] - value_preds[:T]
    mean, std = adv.mean(), adv.std()
    return dict(returns=returns, value_preds=value_preds, adv=adv, adv_norm=(adv - mean) / (std + eps), stats=torch.stack([mean, std]))


def gae_numpy(rewards, value_preds, masks, next_value, gamma, tau, use_gae):
    """(returns, value_preds, adv) as float32 numpy arrays: the specification element by element, every operation a float32
    operation on float32 scalars; gamma * tau is formed in double and rounded once."""
    f = np.float32
    r, v, m = (np.array(t.reshape(t.shape[0], -1).numpy(), dtype=f) for t in (rewards, value_preds, masks))
    nv = np.array(next_value.reshape(-1).numpy(), dtype=f)
    T, N = r.shape
    ret = np.full((T + 1, N), np.nan, dtype=f)
    ga, gt = f(gamma), f(float(gamma) * float(tau))
    for n in range(N):
        if use_gae:
            v[T, n] = nv[n]
            g = f(0)
            for s in range(T - 1, -1, -1):
                d = f(f(r[s, n] + f(f(ga * v[s + 1, n]) * m[s + 1, n])) - v[s, n])
                g = f(d + f(f(gt * m[s + 1, n]) * g))
                ret[s, n] = f(g + v[s, n])
        else:
            ret[T, n] = nv[n]
            for s in range(T - 1, -1, -1):
                ret[s, n] = f(f(f(ret[s + 1, n] * ga) * m[s + 1, n]) + r[s, n])
    return ret, v, (ret[:T] - v[:T]).astype(f)


def same_bits(a, b):
    """Equal as bit patterns (NaNs and the sign of zero included); a, b float32 tensors or arrays of one element count."""
    a = torch.as_tensor(a).detach().cpu().contiguous().reshape(-1)
    b = torch.as_tensor(b).detach().cpu().contiguous().reshape(-1)
    return a.dtype == b.dtype == torch.float32 and a.shape == b.shape and torch.equal(a.view(torch.int32), b.view(torch.int32))
