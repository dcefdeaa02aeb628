"""GPU: scoring the waypoint attention, the action mean and the progress head on the device — wsmg_nav_rows / wsmg_nav_accumulate
(csrc/wsmg_nav_eval.hip) through ops.nav_rows / ops.nav_accumulate and wsmgmap.metrics.NavigationMeter, against the float64 host
form NavigationMeter.rows_from (itself held to the brute-force yardstick in tests/test_nav_eval_cpu.py) on the cases of
tests/nav_eval_util.py.  Integer fields (states, cells, Chebyshev distance, stop codes, every count) are compared for equality; a
float field is held to (n + 8) * 2^-52 * sum|terms| (nav_eval_util's docstring names n and the terms per field), the accumulated
sums to the same bound with n the number of rows.  dis is integer-valued in the kernel-level cases, so every window sum is exact in
float32; the policy-level case has a fractional gt_path and so holds the kernel to the row-major order of the sum as well."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import nav_eval_util as nu
from oracle import cases
from util import T, state_dict_values

pytestmark = pytest.mark.gpu


def _dev(kw):
    return {k: (v.cuda() if torch.is_tensor(v) else v) for k, v in kw.items()}


def _check(what, B=None, **kw):
    """ops.nav_rows on the device against rows_from on the host -> the device's record (numpy)."""
    from wsmgmap import ops
    from wsmgmap.metrics import NavigationMeter
    d = _dev(kw)
    if "mask" in d:
        d["row_mask"] = d.pop("mask")
    got = ops.nav_rows(B=B, **d)
    torch.cuda.synchronize()
    want = NavigationMeter.rows_from(**kw).numpy()
    worst = nu.compare(got.cpu(), want, nu.bounds(want, **kw), what)
    print(f"nav_rows[{what}]: largest deviation {worst:.3f} of its bound")
    return got.cpu().numpy()


# ----------------------------------------------------------------------------- 1. window arithmetic
@pytest.mark.parametrize("B", [1, 5])
@pytest.mark.parametrize("shape", nu.SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_every_window_shape_matches_the_host_form(shape, B):
    H, W, S = shape
    if W > 10240 and B > 1:
        B = 2
    rows = _check(str(shape), **nu.group_args(nu.random_case(B, H, W, S)))
    assert nu.states(rows) == [(1, 1, 1)] * B


def test_an_unaligned_map_takes_the_scalar_head_and_tail():
    """Rows of 7 x 5 = 35 floats start at every residue of 16 bytes; a storage offset of one float moves them all once more."""
    c = nu.random_case(5, 7, 5, 4, seed=9)
    back = torch.zeros(5 * 35 + 1)
    back[1:] = c["dis"].reshape(-1)
    kw = nu.group_args(c)
    from wsmgmap import ops
    from wsmgmap.metrics import NavigationMeter
    d = _dev(kw)
    d["dis"] = back.cuda()[1:].view(5, 7, 5)
    assert d["dis"].data_ptr() % 16 == 4 and d["dis"].is_contiguous()
    got = ops.nav_rows(**d).cpu()
    want = NavigationMeter.rows_from(**kw).numpy()
    nu.compare(got, want, nu.bounds(want, **kw), "unaligned")


# ----------------------------------------------------------------------------- 2. ties, edges
def test_ties_resolve_to_the_lower_index():
    rows = _check("ties", **nu.group_args(nu.ties_case()))
    assert rows[1, nu.ATT_TARGET] == 50 and rows[3, nu.ATT_PEAK] == 77


def test_corner_and_edge_targets_clip_the_neighbourhood():
    c, targets, peaks = nu.edges_case()
    rows = _check("edges", **nu.group_args(c))
    assert rows[:, nu.ATT_TARGET].tolist() == targets and rows[:, nu.ATT_PEAK].tolist() == peaks
    assert rows[:, nu.ATT_CHEB].tolist() == [23.0] * 5                          # the largest distance a 24 x 24 map has


# ----------------------------------------------------------------------------- 3. invalid rows, the mask, absent groups
def test_an_invalid_row_is_counted_in_its_own_group_only():
    c, want = nu.invalid_case()
    rows = _check("invalid", **nu.group_args(c))
    assert nu.states(rows) == want


@pytest.mark.parametrize("dtype", [torch.bool, torch.uint8])
@pytest.mark.parametrize("mask", [[0, 0, 0, 0, 0], [0, 1, 1, 1, 0]], ids=["none", "inner"])
def test_masked_rows_are_not_counted(mask, dtype):
    rows = _check("mask", mask=torch.tensor(mask).to(dtype), **nu.group_args(nu.random_case(5, 7, 5, 4, seed=6)))
    assert nu.states(rows) == [(1, 1, 1) if v else (0, 0, 0) for v in mask]


@pytest.mark.parametrize("groups", [("act", "prog"), ("att", "prog"), ("att", "act"), ()], ids=lambda g: "+".join(g) or "none")
def test_absent_groups(groups):
    from wsmgmap import ops
    c = nu.random_case(5, 10, 10, 4, seed=7)
    if groups:
        rows = _check("absent", **nu.group_args(c, groups))
    else:          # all three NULL: legal, counts nothing
        rows = ops.nav_rows(B=5).cpu().numpy()
        assert np.isnan(np.delete(rows, [nu.ATT_STATE, nu.ACT_STATE, nu.PROG_STATE], axis=1)).all()
        counts, sums = ops.nav_accumulate(torch.from_numpy(rows).cuda())
        assert not counts.any() and not sums.any()
    assert nu.states(rows) == [tuple(int(g in groups) for g in ("att", "act", "prog"))] * 5


# ----------------------------------------------------------------------------- 4. the stop rule
def test_stop_codes_at_the_threshold_and_one_ulp_either_side():
    from wsmgmap import ops
    c, codes = nu.stop_case()
    rows = _check("stop", **c)
    assert rows[:, nu.PROG_STOP].tolist() == [float(v) for v in codes]
    counts, _ = ops.nav_accumulate(torch.from_numpy(rows).cuda())
    assert counts[9:13].tolist() == [codes.count(k) for k in range(4)] == [1, 2, 2, 4]


# ----------------------------------------------------------------------------- 5. accumulation through the meter
class _Net:
    def __init__(self, att):
        self.att_map_t_m = att


class _Pol:
    def __init__(self, c):
        self.net, self.prog = _Net(c["att"]), c["prog"]


def _obs(c):
    return {"gt_path": c["dis"], "waypoint": c["waypoint"], "progress": c["progress"]}


def _three_updates(batches):
    from wsmgmap.metrics import NavigationMeter
    meter = NavigationMeter()
    own = []
    for c in batches:
        d = _dev(c)
        meter.update(_Pol(d), _obs(d), d["pred"])
        own.append(meter.rows.cpu().numpy().copy())
    torch.cuda.synchronize()
    return meter, own


def test_three_updates_add_up_in_row_order_and_repeat_to_the_bit():
    from wsmgmap.metrics import NavigationMeter
    batches = [nu.invalid_case()[0], nu.random_case(1, 10, 10, 4, seed=8), nu.edges_case(4, 10, 10)[0]]          # B = 5, 1, 5
    meter, own = _three_updates(batches)
    host = [NavigationMeter.rows_from(**nu.group_args(c)).numpy() for c in batches]
    c_want, s_want = nu.brute_totals(host)
    assert meter.counts.cpu().tolist() == c_want and c_want[0] == 2 + 1 + 5 and c_want[1] == 3 and c_want[6] == 1 and c_want[8] == 1
    got = meter.sums.cpu().numpy()
    nrows = sum(len(r) for r in host)
    for k, f in enumerate(nu.SUM_FIELDS):
        terms = sum(float(np.abs(np.nan_to_num(r[:, f], nan=0.0)).sum()) for r in host)
        bound = (nrows + 8) * nu.EPS * terms
        print(f"nav_accumulate: sum of field {f}: device {got[k]!r} host {s_want[k]!r} bound {bound:.3e}")
        assert abs(got[k] - s_want[k]) <= bound, f"sum of field {f}"
    # against the device's own rows the fold is the same additions in the same order: the same bits
    c_own, s_own = nu.brute_totals(own)
    assert meter.counts.cpu().tolist() == c_own and got.tolist() == s_own
    again, own2 = _three_updates(batches)
    assert torch.equal(again._block, meter._block) and all(np.array_equal(a, b, equal_nan=True) for a, b in zip(own, own2))
    out = meter.compute()
    ref = NavigationMeter.scores_from(torch.tensor(c_own), torch.tensor(s_own, dtype=torch.float64), axes=2)
    assert out.keys() == ref.keys() and all(np.array_equal(out[k], ref[k], equal_nan=True) for k in out)
    assert out["attention_rows"] == 8 and out["progress_invalid"] == 1 and len(out["action_abs"]) == 2
    # state_dict round trip through the host, reset
    other = NavigationMeter()
    other.load_state_dict({k: (v.cpu() if torch.is_tensor(v) else v) for k, v in meter.state_dict().items()})
    assert torch.equal(other._block, meter._block)
    meter.reset()
    assert not meter._block.any() and np.isnan(meter.compute()["hit_at_0"]) and other.counts[0] == 8


def test_update_refuses_what_it_cannot_score_and_skips_what_is_absent():
    from wsmgmap import _abi
    from wsmgmap.metrics import NavigationMeter
    d = _dev(nu.random_case(4, 10, 10, 4, seed=10))
    meter = NavigationMeter()
    with pytest.raises(_abi.WsmgError, match="nothing to score"):
        meter.update(_Pol(dict(att=None, prog=None)), {})
    with pytest.raises(_abi.WsmgError, match=r"'gt_path'.*\(4, 10, 10\) on cpu"):
        meter.update(_Pol(d), dict(_obs(d), gt_path=d["dis"].cpu()), d["pred"])
    with pytest.raises(_abi.WsmgError, match=r"'gt_path'.*float64 \(4, 10, 10\)"):
        meter.update(_Pol(d), dict(_obs(d), gt_path=d["dis"].double()), d["pred"])
    with pytest.raises(_abi.WsmgError, match=r"'waypoint'.*4 rows.*\(3, 3\)"):
        meter.update(_Pol(d), dict(_obs(d), waypoint=d["waypoint"][:3]), d["pred"])
    with pytest.raises(_abi.WsmgError, match=r"'progress'.*\(5, 1\)"):
        meter.update(_Pol(d), dict(_obs(d), progress=torch.zeros(5, 1, device="cuda")), d["pred"])
    with pytest.raises(_abi.WsmgError, match=r"\(4, 15\)"):
        meter.update(_Pol(dict(d, att=d["att"][:, :15])), _obs(d), d["pred"])
    with pytest.raises(_abi.WsmgError, match=r"3 weights \(3,\) for 4 rows"):
        meter.update(_Pol(d), _obs(d), d["pred"], torch.ones(3, device="cuda"))
    assert not meter._block.any()
    # absent inputs: each group is skipped, the others are scored; 'waypoint_distribution' stands in for 'gt_path'
    obs = {"waypoint_distribution": d["dis"], "progress": d["progress"]}
    meter.update(_Pol(d), obs, d["pred"], torch.tensor([1.0, 0.0, 2.0, 0.5], device="cuda"))
    assert nu.states(meter.rows.cpu()) == [(1, 0, 1), (0, 0, 0), (1, 0, 1), (1, 0, 1)]
    meter.update(_Pol(d).net, _obs(d))                      # a bare network: the attention alone
    assert nu.states(meter.rows.cpu()) == [(1, 0, 0)] * 4 and meter.counts.cpu().tolist()[:2] == [7, 0]


# ----------------------------------------------------------------------------- 6. entry-point refusals leave the outputs alone
def test_refused_calls_return_einval_and_touch_nothing():
    from wsmgmap import _abi, ops
    L = _abi.lib()
    d = _dev(nu.random_case(4, 10, 10, 4, seed=11))
    rows = torch.full((4, ops.NAV_ROW), 7.0, device="cuda", dtype=torch.float64)
    p = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())          # noqa: E731

    def call(**over):
        a = dict(att=d["att"], dis=d["dis"], S=4, H=10, W=10, pred=d["pred"], waypoint=d["waypoint"], ld=3, A=2, prog=d["prog"],
                 progress=d["progress"], B=4, rows=rows)
        a.update(over)
        return L.wsmg_nav_rows(p(a["att"]), p(a["dis"]), a["S"], a["H"], a["W"], p(a["pred"]), p(a["waypoint"]), a["ld"], a["A"],
                               p(a["prog"]), p(a["progress"]), 0.8, None, a["B"], p(a["rows"]), None)
    for over in (dict(B=0), dict(S=0), dict(S=65), dict(H=0), dict(W=-1), dict(att=None), dict(dis=None), dict(A=0), dict(A=5),
                 dict(pred=None), dict(progress=None), dict(rows=None)):
        assert call(**over) == -1, over
    counts = torch.full((ops.NAV_COUNTS,), 3, device="cuda", dtype=torch.int64)
    sums = torch.full((ops.NAV_SUMS,), 0.5, device="cuda", dtype=torch.float64)
    for args in ((None, 4, p(counts), p(sums)), (p(rows), 0, p(counts), p(sums)), (p(rows), 4, None, p(sums)), (p(rows), 4, p(counts), None)):
        assert L.wsmg_nav_accumulate(*args, None) == -1
    torch.cuda.synchronize()
    assert bool((rows == 7.0).all()) and bool((counts == 3).all()) and bool((sums == 0.5).all())
    assert call() == 0                                       # the same arguments, none overridden: accepted
    torch.cuda.synchronize()
    assert nu.states(rows.cpu()) == [(1, 1, 1)] * 4
    with pytest.raises(_abi.WsmgError, match=r"\(4, 17\)"):
        ops.nav_rows(**{**nu.group_args(d), "att": torch.zeros(4, 17, device="cuda")})
    with pytest.raises(_abi.WsmgError, match="pairs"):
        ops.nav_rows(att=d["att"], S=4)
    with pytest.raises(_abi.WsmgError, match=r"float64 \[4, 18\]"):
        ops.nav_rows(**nu.group_args(d), out=torch.zeros(4, 17, device="cuda", dtype=torch.float64))
    with pytest.raises(_abi.WsmgError, match="float32"):
        ops.nav_rows(prog=d["prog"].double(), progress=d["progress"].double())


# ----------------------------------------------------------------------------- 7. capture
def test_update_replays_from_a_captured_graph():
    from wsmgmap.metrics import NavigationMeter
    d = _dev(nu.edges_case(4, 10, 10)[0])
    w = torch.tensor([1.0, 0.0, 0.5, 2.0, 1.0], device="cuda")
    eager = NavigationMeter()
    eager.update(_Pol(d), _obs(d), d["pred"], w)
    meter = NavigationMeter()
    meter.update(_Pol(d), _obs(d), d["pred"], w)             # the eager warm-up: the record and the mask exist from here on
    ptrs = (meter.rows.data_ptr(), meter._mask.data_ptr())
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):                            # one stream, no parallel branches
        meter.update(_Pol(d), _obs(d), d["pred"], w)
    assert (meter.rows.data_ptr(), meter._mask.data_ptr()) == ptrs
    meter.reset()
    graph.replay()
    graph.replay()
    torch.cuda.synchronize()
    assert meter.counts.cpu().tolist() == (2 * eager.counts).cpu().tolist() and eager.counts[0] == 4 and eager.counts[7] == 4
    nrows = 8
    for k, f in enumerate(nu.SUM_FIELDS):          # s + s is exact; the replayed fold adds the same rows a second time onto s
        want, got = 2 * float(eager.sums[k]), float(meter.sums[k])
        assert abs(got - want) <= (nrows + 8) * nu.EPS * abs(want), f"sum of field {f}"
    assert np.array_equal(meter.rows.cpu().numpy(), eager.rows.cpu().numpy(), equal_nan=True)


# ----------------------------------------------------------------------------- 8. the policy
class _Box:
    shape = (2,)


Tn, N = 4, 2


@functools.lru_cache(maxsize=None)
def _update():
    """One teacher-forcing update (forward, the meter, backward) of the deterministic-fill T = 4 x N = 2 policy with the monitors on
    -> (policy, observations, pred, weights, meter, copies of att / prog / pred taken in front of the meter)."""
    from wsmgmap.common.aux_losses import AuxLosses
    from wsmgmap.config import default_model_config
    from wsmgmap.metrics import NavigationMeter
    from wsmgmap.models.policy import BasePolicy
    pol = BasePolicy(None, _Box(), default_model_config(num_proc=2))
    pol.load_state_dict(state_dict_values(), strict=True)
    pol = pol.cuda()
    pol.train()
    pol.net.depth_encoder.eval()
    pol.net.rgb_encoder.eval()
    obs_np, prev, masks, weights = cases.update_inputs(Tn, N)
    og = {k: T(v).cuda() for k, v in obs_np.items()}
    w = T(weights).cuda()
    meter = NavigationMeter()
    AuxLosses.activate()
    AuxLosses.clear()
    try:
        pred, aux = pol(og, torch.zeros(2, N, 512, device="cuda"), T(prev).cuda(), T(masks).cuda(), w)
        before = [t.detach().clone() for t in (pol.net.att_map_t_m, pol.prog, pred)]
        meter.update(pol, og, pred, w)
        host = dict(att=pol.net.att_map_t_m.detach().cpu(), prog=pol.prog.detach().cpu(), pred=pred.detach().cpu())
        after = [t.detach().clone() for t in (pol.net.att_map_t_m, pol.prog, pred)]
        ((pred ** 2).mean() + aux).backward()
        torch.cuda.synchronize()
    finally:
        AuxLosses.deactivate()
        AuxLosses.clear()
    return og, w, meter, host, before, after


def test_policy_update_is_scored_as_the_host_form_scores_it():
    from wsmgmap.metrics import NavigationMeter
    og, w, meter, host, before, after = _update()
    B = Tn * N
    assert tuple(host["att"].shape) == (B, 576) and tuple(host["prog"].shape) == (B, 1) and tuple(host["pred"].shape) == (B, 2)
    assert tuple(og["waypoint"].shape) == (B, 3)
    kw = dict(att=host["att"], dis=og["gt_path"].cpu(), S=24, pred=host["pred"], waypoint=og["waypoint"].cpu(), prog=host["prog"],
              progress=og["progress"].cpu(), mask=(w > 0).view(-1).cpu())
    want = NavigationMeter.rows_from(**kw).numpy()
    worst = nu.compare(meter.rows.cpu(), want, nu.bounds(want, **kw), "policy")
    print(f"policy update: largest deviation {worst:.3f} of its bound")
    assert nu.states(want) == [(1, 1, 1)] * (B - 1) + [(0, 0, 0)]               # the padded step is left out
    c_want, _ = nu.brute_totals([want])
    assert meter.counts.cpu().tolist() == c_want
    out = meter.compute()
    assert out["attention_rows"] == out["action_rows"] == out["progress_rows"] == B - 1 and 0.0 <= out["hit_at_2"] <= 1.0
    assert 0.0 < out["mean_entropy"] <= float(np.log(576)) + 1e-6 and sum(sum(r) for r in out["stop_confusion"]) == B - 1
    assert all(torch.equal(a, b) for a, b in zip(before, after))                # the meter reads, nothing else
