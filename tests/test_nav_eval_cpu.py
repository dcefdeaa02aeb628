"""CPU: the host side of the attention / action / progress scoring — the two entry points of csrc/wsmg_nav_eval.hip in the header and
the binding, every refused argument (the checks precede the first launch, so no GPU is needed), the refusals of ops.nav_rows and
NavigationMeter, and NavigationMeter.rows_from, the documented host form of the row record, against the brute-force yardstick of
tests/nav_eval_util.py on every case the GPU tests use.  The kernels are tested in tests/test_gpu_nav_eval.py."""
import ctypes
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import nav_eval_util as nu

EINVAL = -1
NAMES = ("wsmg_nav_rows", "wsmg_nav_accumulate")

_buf = (ctypes.c_uint64 * 64)()
P = ctypes.cast(_buf, ctypes.c_void_p)      # a non-null host pointer: never dereferenced, every check precedes the launch


def _rows(L, **over):
    """(att, dis, S, H, W, pred, waypoint, ld_waypoint, A, prog, progress, stop_threshold, row_mask, B, rows, stream), valid unless
    overridden."""
    a = dict(att=P, dis=P, S=24, H=100, W=100, pred=P, waypoint=P, ld=3, A=2, prog=P, progress=P, thr=0.8, row_mask=None, B=8, rows=P)
    a.update(over)
    return L.wsmg_nav_rows(a["att"], a["dis"], a["S"], a["H"], a["W"], a["pred"], a["waypoint"], a["ld"], a["A"], a["prog"],
                           a["progress"], a["thr"], a["row_mask"], a["B"], a["rows"], None)


def test_entry_points_are_declared_bound_and_exported():
    """(Their declarations against the binding, and the header's named constants against the Python side's and the yardstick's:
    tests/test_abi_cpu.py.)"""
    from wsmgmap import _abi
    L = _abi.lib()
    for name in NAMES:
        assert name in _abi.exported_names() and hasattr(L, name)
        assert list(getattr(L, name).argtypes) == list(_abi._SIG[name]) and getattr(L, name).restype is ctypes.c_int
    assert len(_abi._SIG[NAMES[0]]) == 16 and len(_abi._SIG[NAMES[1]]) == 5


@pytest.mark.parametrize("over", [
    dict(rows=None), dict(B=0), dict(B=-3), dict(S=0), dict(S=-1), dict(S=65), dict(S=1 << 16), dict(S=46341),
    dict(H=0), dict(W=0), dict(H=-1), dict(W=-100), dict(H=1 << 16, W=1 << 15),
    dict(att=None), dict(dis=None), dict(pred=None), dict(waypoint=None), dict(prog=None), dict(progress=None),
    dict(A=0), dict(A=5), dict(A=-1), dict(A=3, ld=2),
], ids=lambda o: ",".join(f"{k}={v}" for k, v in o.items()))
def test_rows_refuses_bad_arguments_before_any_launch(over):
    from wsmgmap import _abi
    assert _rows(_abi.lib(), **over) == EINVAL


def test_accumulate_refuses_bad_arguments_before_any_launch():
    from wsmgmap import _abi
    L = _abi.lib()
    assert L.wsmg_nav_accumulate(None, 4, P, P, None) == EINVAL
    assert L.wsmg_nav_accumulate(P, 4, None, P, None) == EINVAL
    assert L.wsmg_nav_accumulate(P, 4, P, None, None) == EINVAL
    assert L.wsmg_nav_accumulate(P, 0, P, P, None) == EINVAL
    assert L.wsmg_nav_accumulate(P, -1, P, P, None) == EINVAL


def test_ops_and_meter_refuse_cpu_tensors():
    from wsmgmap import _abi, ops
    from wsmgmap.metrics import NavigationMeter
    c = nu.random_case(2, 10, 10, 4)
    with pytest.raises(_abi.WsmgError, match="no CPU fallback"):
        ops.nav_rows(**nu.group_args(c))
    with pytest.raises(_abi.WsmgError, match="no CPU fallback"):
        ops.nav_rows(prog=c["prog"], progress=c["progress"])
    with pytest.raises(_abi.WsmgError, match="no CPU fallback"):
        ops.nav_accumulate(torch.zeros(2, ops.NAV_ROW, dtype=torch.float64))
    with pytest.raises(_abi.WsmgError, match="no CPU fallback"):
        NavigationMeter(device="cpu")
    with pytest.raises(ValueError, match="finite"):
        NavigationMeter(stop_threshold=float("nan"), device="cpu")


def test_compute_of_an_empty_meter_has_nan_rates():
    from wsmgmap import ops
    from wsmgmap.metrics import NavigationMeter
    out = NavigationMeter.scores_from(torch.zeros(ops.NAV_COUNTS, dtype=torch.int64), torch.zeros(ops.NAV_SUMS, dtype=torch.float64), axes=2)
    for k in ("attention_rows", "attention_invalid", "action_rows", "action_invalid", "progress_rows", "progress_invalid"):
        assert out[k] == 0
    for k in ("hit_at_0", "hit_at_1", "hit_at_2", "mean_cell_distance", "mean_mass_near_target", "mean_entropy", "action_mse", "action_l2",
              "progress_mae", "progress_mse", "stop_precision", "stop_recall"):
        assert math.isnan(out[k]), k
    assert len(out["action_abs"]) == 2 and all(math.isnan(v) for v in out["action_abs"]) and out["stop_confusion"] == [[0, 0], [0, 0]]


def test_scores_by_hand():
    from wsmgmap.metrics import NavigationMeter
    #                        att inv h0 h1 h2 act inv prog inv  tn fp fn tp
    counts = torch.tensor([4, 1, 1, 2, 3, 2, 0, 10, 2, 4, 1, 2, 3])
    sums = torch.tensor([6.0, 5.0, 2.0, 8.0, 1.0, 1.5, 0.5, 0.25, 0.0, 0.0, 2.0, 0.5], dtype=torch.float64)
    s = NavigationMeter.scores_from(counts, sums, axes=2)
    assert (s["hit_at_0"], s["hit_at_1"], s["hit_at_2"]) == (0.25, 0.5, 0.75) and s["attention_invalid"] == 1
    assert s["mean_chebyshev_distance"] == 1.5 and s["mean_cell_distance"] == 1.25 and s["mean_mass_near_target"] == 0.5 and s["mean_entropy"] == 2.0
    assert s["action_mse"] == 0.5 and s["action_l2"] == 0.75 and s["action_abs"] == [0.25, 0.125]
    assert s["progress_mae"] == 0.2 and s["progress_mse"] == 0.05 and s["progress_invalid"] == 2
    assert s["stop_confusion"] == [[4, 1], [2, 3]] and s["stop_precision"] == 3 / 4 and s["stop_recall"] == 3 / 5


# ----------------------------------------------------------------------------- rows_from against the brute-force yardstick
def _both(what, B=None, **kw):
    from wsmgmap.metrics import NavigationMeter
    got = NavigationMeter.rows_from(**kw)
    want = nu.brute_rows(B=B, **kw)
    assert got.dtype == torch.float64 and tuple(got.shape) == want.shape
    nu.compare(got, want, nu.bounds(want, **kw), what)
    return got.numpy()


@pytest.mark.parametrize("B", [1, 5])
@pytest.mark.parametrize("shape", nu.SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_host_form_matches_the_yardstick_on_every_window_shape(shape, B):
    H, W, S = shape
    if W > 10240 and B > 1:
        B = 2
    c = nu.random_case(B, H, W, S)
    rows = _both(str(shape), **nu.group_args(c))
    assert nu.states(rows) == [(1, 1, 1)] * B
    # the yardstick's windows are torch's: the cell means are F.interpolate(mode="area") (exact here: integer-valued dis)
    area = F.interpolate(c["dis"].double().unsqueeze(1), size=(S, S), mode="area").reshape(B, -1).numpy()
    cells = np.array([[float(v) for v in nu.brute_cells(c["dis"][b].numpy(), S)] for b in range(B)])
    assert np.allclose(cells, area, rtol=1e-6, atol=0)
    if W <= 10240:          # (two means of 3 415-wide windows can differ by less than a float32 ulp: a tie there, none in float64)
        assert np.array_equal(rows[:, nu.ATT_TARGET], area.argmin(1))


def test_host_form_resolves_ties_to_the_lower_index():
    rows = _both("ties", **nu.group_args(nu.ties_case()))
    assert rows[1, nu.ATT_TARGET] == 50 and rows[3, nu.ATT_PEAK] == 77


def test_host_form_clips_the_neighbourhood_at_the_edges():
    c, targets, peaks = nu.edges_case()
    rows = _both("edges", **nu.group_args(c))
    assert rows[:, nu.ATT_TARGET].tolist() == targets and rows[:, nu.ATT_PEAK].tolist() == peaks
    assert rows[:, nu.ATT_CHEB].tolist() == [23.0] * 5 and rows[0, nu.ATT_EUCLID] == math.sqrt(2 * 23 * 23)
    a = c["att"].double()
    assert rows[0, nu.ATT_MASS] == float(((a[0, 0] + a[0, 1]) + a[0, 24]) + a[0, 25])          # four cells, row-major


def test_host_form_counts_an_invalid_row_in_its_own_group_only():
    c, want = nu.invalid_case()
    rows = _both("invalid", **nu.group_args(c))
    assert nu.states(rows) == want
    assert np.isnan(rows[0, 1:7]).all() and not np.isnan(rows[0, 8:18]).any()


@pytest.mark.parametrize("mask", [[0, 0, 0, 0, 0], [0, 1, 1, 1, 0]], ids=["none", "inner"])
def test_host_form_leaves_masked_rows_uncounted(mask):
    c = nu.random_case(5, 7, 5, 4, seed=6)
    for m in (torch.tensor(mask, dtype=torch.bool), torch.tensor(mask, dtype=torch.uint8)):
        rows = _both("mask", mask=m, **nu.group_args(c))
        assert nu.states(rows) == [(1, 1, 1) if v else (0, 0, 0) for v in mask]


def test_host_form_compares_the_stop_threshold_in_float32():
    c, codes = nu.stop_case()
    rows = _both("stop", **c)
    assert rows[:, nu.PROG_STOP].tolist() == [float(v) for v in codes] and sorted(set(codes)) == [0, 1, 2, 3]
    assert codes == [0, 2, 2, 1, 3, 3, 1, 3, 3]


@pytest.mark.parametrize("groups", [("act", "prog"), ("att", "prog"), ("att", "act"), ()], ids=lambda g: "+".join(g) or "none")
def test_host_form_with_absent_groups(groups):
    c = nu.random_case(5, 10, 10, 4, seed=7)
    kw = nu.group_args(c, groups)
    if not groups:
        kw["mask"] = torch.ones(5, dtype=torch.bool)
    rows = _both("absent", B=5, **kw)
    assert nu.states(rows) == [tuple(int(g in groups) for g in ("att", "act", "prog"))] * 5


def test_totals_from_matches_the_yardstick():
    from wsmgmap.metrics import NavigationMeter
    recs = [nu.brute_rows(**nu.group_args(nu.invalid_case()[0])), nu.brute_rows(**nu.group_args(nu.random_case(1, 10, 10, 4, seed=8))),
            nu.brute_rows(**nu.stop_case()[0]), nu.brute_rows(**nu.group_args(nu.edges_case(4, 10, 10)[0]))]
    counts = sums = None
    for r in recs:
        counts, sums = NavigationMeter.totals_from(torch.from_numpy(r), counts, sums)
    c, s = nu.brute_totals(recs)
    assert counts.tolist() == c and sums.tolist() == s                    # the same additions in the same order: the same bits
    assert c[0] == 2 + 1 + 5 and c[1] == 3 and c[6] == 1 and c[8] == 1 and sum(c[9:13]) == c[7] == 4 + 1 + 9 + 5
