"""GPU: the per-tensor gradient report (csrc/wsmg_optim.hip: grad_scan_multi_kernel, grad_report_fold_kernel,
grad_report_latch_kernel; wsmgmap.optim.grad_stats, wsmgmap.optim.Adam(grad_report=True).grad_report() / .last_skipped()) against
float64 numpy written here: counts by np.isnan / np.isinf, the maximum over np.abs(g[np.isfinite(g)]), the norm
np.sqrt((g.astype(np.float64) ** 2).sum()) cast to float32.

Tensors: tests/test_gpu_adam_guard.py's sizes around the 4-element vector and the 4 096-element chunk, once 16-byte aligned and once
as views one float into their storage (the scalar path), then 250-element tensors up to 50 (the table of 48 spills into a second
launch), then a parameter with zero elements and a parameter without a gradient: 52 report rows.

THE BARS: counts equal; max |g| bit-equal (a maximum of float32 values); the norm within 2 float32 ulps, relative 2^-22 — the sums are
float64 on both sides (relative 1e-16 apart at most per addition), so the only visible roundings are the square root and the cast."""
import functools

import numpy as np
import pytest
import torch

from adam_util import _bits, _ptr, _stream
from oracle import cases
from oracle import detfill as df
from util import T, state_dict_values

pytestmark = pytest.mark.gpu

SIZES = [1, 3, 4, 4095, 4096, 4097, 8193]
ALL_SIZES = SIZES + SIZES + [250] * (50 - 2 * len(SIZES))
N_REAL = len(ALL_SIZES)              # rows 0 .. 49 have gradients; row 50 has zero elements, row 51 has no gradient
ROW_EMPTY, ROW_NOGRAD, N_ROWS = N_REAL, N_REAL + 1, N_REAL + 2
CHUNK = 4096
TOTAL_BLOCKS = sum((n + CHUNK - 1) // CHUNK for n in ALL_SIZES)
LR = 2.5e-4
NORM_RTOL = 2.0 ** -22
FAR = CHUNK * 257 + 1                # one tensor of more than 256 chunks: the fold's threads take a second chunk each


def _off(i):
    return 1 if len(SIZES) <= i < 2 * len(SIZES) else 0


@functools.lru_cache(maxsize=None)
def _grads():
    """The 50 float32 gradients — computed once, never written."""
    out = []
    for i, n in enumerate(ALL_SIZES):
        g = df.uniform(f"report.{i}.g", (n,), 0.2)
        g.setflags(write=False)
        out.append(g)
    return out


def _yard(g):
    """(norm as float32, max |g| over the finite elements, NaNs, Infs) of one float32 array, in float64 numpy."""
    g = np.asarray(g, dtype=np.float32).reshape(-1)
    with np.errstate(over="ignore", invalid="ignore"):
        norm = np.float32(np.sqrt((g.astype(np.float64) ** 2).sum()))
    fin = g[np.isfinite(g)]
    return norm, (np.abs(fin).max() if fin.size else np.float32(0.0)), int(np.isnan(g).sum()), int(np.isinf(g).sum())


class DevSet:
    """The parameters on the device: .params (52), .grads[i] the gradient views of the first 50, .host[i] what they hold."""

    def __init__(self, scale=None, which=None):
        which = list(range(N_REAL)) if which is None else which
        self.host, self.grads, self.params = [], [], []
        for i in which:
            g = _grads()[i]
            if scale is not None:
                g = (g * np.float32(scale)).astype(np.float32)
            off, n = _off(i), g.size
            pbuf, gbuf = torch.zeros(n + 8, device="cuda"), torch.zeros(n + 8, device="cuda")
            assert gbuf.data_ptr() % 16 == 0
            p = torch.nn.Parameter(pbuf[off:off + n])
            p.grad = gbuf[off:off + n]
            p.grad.copy_(T(np.array(g)))
            assert p.grad.data_ptr() % 16 == 4 * off
            self.host.append(np.array(g))
            self.grads.append(p.grad)
            self.params.append(p)
        if len(which) == N_REAL:
            empty = torch.nn.Parameter(torch.zeros(0, device="cuda"))
            empty.grad = torch.zeros(0, device="cuda")
            self.params += [empty, torch.nn.Parameter(torch.zeros(7, device="cuda"))]

    def poison(self, row, at, value):
        self.grads[row][at] = value
        self.host[row][at] = value

    def heal(self, row):
        g = _grads()[row]
        self.grads[row].copy_(T(np.array(g)))
        self.host[row] = np.array(g)


def _check_table(name, table, host, tail=False):
    """An [n, 4] int32 table (device or host) against the yardstick of host[i], row by row; tail: the rows of the parameter without
    elements and of the one without a gradient follow, and are zero."""
    table = table.cpu().numpy()
    assert table.shape == (len(host) + (2 if tail else 0), 4), table.shape
    worst = 0.0
    for i, g in enumerate(host):
        norm, mx, nan, inf = _yard(g)
        got_norm, got_max = table[i, :2].view(np.float32)
        got_nan, got_inf = (int(x) & 0xffffffff for x in table[i, 2:])
        assert (got_nan, got_inf) == (nan, inf), f"{name}: row {i}: counts {(got_nan, got_inf)}, float64 {(nan, inf)}"
        assert got_max.view(np.uint32) == np.float32(mx).view(np.uint32), f"{name}: row {i}: max |g| {got_max!r}, float64 {mx!r}"
        if np.isfinite(norm):
            err = abs(float(got_norm) - float(norm)) / float(norm) if norm > 0 else abs(float(got_norm))
            worst = max(worst, err)
            assert err <= NORM_RTOL, f"{name}: row {i}: norm {got_norm!r}, float64 {norm!r}, relative error {err:.3e}"
        else:
            assert (np.isnan(norm) and np.isnan(got_norm)) or got_norm == norm, f"{name}: row {i}: norm {got_norm!r}, float64 {norm!r}"
    for i in ((ROW_EMPTY, ROW_NOGRAD) if tail else ()):
        assert not table[i].any(), f"{name}: row {i} of a parameter without elements / gradient is not zero: {table[i]}"
    print(f"{name}: worst relative norm error {worst:.3e} (bar {NORM_RTOL:.3e})")


def _stats_table(stats):
    """[GradStat] back into the [n, 4] int32 layout (what _check_table reads)."""
    f = np.array([[s.norm, s.max_abs] for s in stats], dtype=np.float32).view(np.int32)
    c = np.array([[s.nan, s.inf] for s in stats], dtype=np.uint32).view(np.int32)
    return torch.from_numpy(np.concatenate([f, c], axis=1))


def _adam(ds, **kw):
    from wsmgmap import optim
    kw.setdefault("skip_nonfinite", True)
    return optim.Adam(ds.params, lr=LR, **kw)


# ----------------------------------------------------------------------------- 1. the statistics
@pytest.mark.parametrize("scale", [1e-30, None, 1e30], ids=["1e-30", "unit", "1e30"])
def test_statistics_match_float64(scale):
    from wsmgmap import optim
    ds = DevSet(scale)
    table = optim.grad_stats(ds.params)
    assert table.shape == (N_ROWS, 4) and table.dtype == torch.int32 and table.is_cuda
    _check_table(f"grad_stats {scale}", table, ds.host, tail=True)
    f = optim.stats_as_float(table)
    assert f.shape == (N_ROWS, 2) and f.dtype == torch.float32 and torch.equal(_bits(f), table[:, :2])
    # a parameter whose gradient goes away: its row is zero, no other row moves
    keep = ds.params[5].grad
    ds.params[5].grad = None
    gone = optim.grad_stats(ds.params)
    ds.params[5].grad = keep
    same = [i for i in range(N_ROWS) if i != 5]
    assert torch.equal(gone[same], table[same]) and not bool(gone[5].any())
    # the optimizer's report after a guarded step (taken: every gradient is finite)
    opt = _adam(ds, grad_report=True)
    assert opt.last_skipped() is None and all(s == (s.index, s.name, 0.0, 0.0, 0, 0) for s in opt.grad_report())
    opt.step()
    stats = opt.grad_report()
    assert opt.skipped_steps == 0 and opt.last_skipped() is None
    assert [s.index for s in stats] == list(range(N_ROWS)) and stats[3].name == "group0.param3"
    assert torch.equal(_stats_table(stats), table.cpu()), "the optimizer's report differs from grad_stats on the same gradients"
    assert all(torch.equal(_bits(g), _bits(T(h).cuda())) for g, h in zip(ds.grads, ds.host)), "a gradient was written"


# ----------------------------------------------------------------------------- 2. determinism and order
def test_two_calls_give_the_same_bits():
    from wsmgmap import optim
    ds = DevSet()
    a, b = optim.grad_stats(ds.params), optim.grad_stats(ds.params)
    assert torch.equal(a, b)
    opt = _adam(ds, grad_report=True)
    opt.step()
    first = opt._report.clone()
    opt.step()
    assert torch.equal(opt._report, first) and torch.equal(first, a)


@pytest.mark.parametrize("n", SIZES + [FAR])
def test_one_tensor_norm_has_the_guard_records_bits(n):
    """guard_finalize's order: for a list of one tensor the report's word 0 IS the guard record's norm."""
    g = df.uniform(f"report.one.{n}", (n,), 0.2)
    p = torch.nn.Parameter(torch.zeros(n, device="cuda"))
    p.grad = T(g).cuda()
    from wsmgmap import optim
    opt = optim.Adam([p], lr=LR, skip_nonfinite=True, grad_report=True)
    opt.step()
    torch.cuda.synchronize()
    assert torch.equal(opt._report[0, 0], _bits(opt.grad_norm)), (opt.grad_report(), float(opt.grad_norm))
    _check_table(f"one tensor of {n}", opt._report, [g])


# ----------------------------------------------------------------------------- 3. where the poison sits
NAN, INF = float("nan"), float("inf")
UNALIGNED_8193 = 2 * len(SIZES) - 1
# (name, [(row, element, value)], row of the largest norm: a NaN norm counts as the largest, ties go to the lowest row)
POISON = [("nan-at-0", [(5, 0, NAN)], 5),
          ("nan-at-last", [(5, 4096, NAN)], 5),                            # the one element of the second chunk
          ("nan-both-sides-of-a-chunk-boundary", [(6, 4095, NAN), (6, 4096, NAN)], 6),
          ("nan-in-the-tail-of-an-unaligned-view", [(UNALIGNED_8193, 8192, NAN)], UNALIGNED_8193),
          ("nan-in-the-vector-tail", [(6, 8192, NAN)], 6),                 # aligned 8193: the last chunk's scalar tail
          ("plus-and-minus-inf", [(3, 10, INF), (3, 4094, -INF)], 3),
          ("nan-in-tensor-49", [(49, 123, NAN)], 49),                      # the second launch
          ("two-tensors", [(30, 7, NAN), (9, 1, INF)], 30),                # first non-finite: 9; its norm is Inf, 30's is NaN
          ("two-nan-tensors", [(30, 7, NAN), (9, 1, NAN)], 9)]


def test_where_the_poison_sits():
    assert ALL_SIZES[UNALIGNED_8193] == 8193 and _off(UNALIGNED_8193) == 1 and N_REAL > 48
    ds = DevSet()
    opt = _adam(ds, grad_report=True)
    for k, (name, spots, largest) in enumerate(POISON):
        for row, at, value in spots:
            ds.poison(row, at, value)
        opt.step()
        ls = opt.last_skipped()
        rows = sorted({row for row, _, _ in spots})
        assert ls is not None and ls.skipped == k + 1 == opt.skipped_steps and ls.attempt == k + 1, (name, ls and ls[:2])
        _check_table(name, _stats_table(ls.stats), ds.host, tail=True)       # nan, inf and the FINITE maximum of every row
        assert ls.first_nonfinite is ls.stats[rows[0]] and ls.first_nonfinite.index == rows[0], name
        assert ls.nonfinite_tensors == len(rows) and ls.largest.index == largest, (name, ls.nonfinite_tensors, ls.largest)
        assert ls.first_nonfinite.nan + ls.first_nonfinite.inf == sum(1 for r, _, _ in spots if r == rows[0]), name
        assert torch.equal(_stats_table(opt.grad_report()), _stats_table(ls.stats)), name
        for row in rows:
            ds.heal(row)


# ----------------------------------------------------------------------------- 4. overflow without a non-finite element
def test_float32_overflow_of_the_norm_over_finite_gradients():
    ds = DevSet()
    ds.grads[6].fill_(3e38)
    ds.host[6][:] = np.float32(3e38)
    s64 = (ds.host[6].astype(np.float64) ** 2).sum()
    assert np.isfinite(s64) and np.sqrt(s64) > float(np.finfo(np.float32).max)
    opt = _adam(ds, grad_report=True)
    opt.step()
    ls = opt.last_skipped()
    assert opt.skipped_steps == 1 and np.isinf(float(opt.grad_norm))
    assert ls is not None and ls.first_nonfinite is None and ls.nonfinite_tensors == 0
    assert ls.largest.index == 6 and np.isinf(ls.largest.norm) and (ls.largest.nan, ls.largest.inf) == (0, 0)
    assert np.float32(ls.largest.max_abs) == np.float32(3e38)
    _check_table("overflow", _stats_table(ls.stats), ds.host, tail=True)


# ----------------------------------------------------------------------------- 5. the latch holds
def test_latch_is_written_by_skipped_steps_only():
    ds = DevSet()
    opt = _adam(ds, grad_report=True)
    p0 = ds.params[0]
    sentinel = (torch.arange(opt._latch.numel(), device="cuda", dtype=torch.int32) * 7 + 0x5a5a0001)
    opt._latch.copy_(sentinel)
    opt.step()                                             # clean
    torch.cuda.synchronize()
    assert torch.equal(opt._latch, sentinel), "a step that was taken stored into the latch"
    opt._latch.zero_()
    assert opt.last_skipped() is None
    ds.poison(12, 4096, NAN)
    opt.step()                                             # skipped
    ls = opt.last_skipped()
    assert ls.attempt == opt.state[p0]["step"] == 2 and ls.skipped == 1 and ls.first_nonfinite.index == 12
    held = opt._latch.clone()
    ds.heal(12)
    for _ in range(3):
        opt.step()
    torch.cuda.synchronize()
    assert torch.equal(opt._latch, held), "clean steps changed the latch"
    again = opt.last_skipped()
    assert again[:2] == ls[:2] and again.first_nonfinite.index == 12 and again.first_nonfinite.nan == 1
    _check_table("report of the last clean step", _stats_table(opt.grad_report()), ds.host, tail=True)
    assert opt.skipped_steps == 1 and opt.state[p0]["step"] == 5
    ds.poison(40, 3, -INF)
    opt.step()
    ls2 = opt.last_skipped()
    assert ls2.skipped == 2 and ls2.attempt == opt.state[p0]["step"] == 6
    assert ls2.first_nonfinite.index == 40 and (ls2.first_nonfinite.nan, ls2.first_nonfinite.inf) == (0, 1)
    assert ls2.stats[12].nan == 0 and ls2.nonfinite_tensors == 1
    # load_state_dict re-creates the tables zeroed, where it re-creates the guard record
    opt.load_state_dict(opt.state_dict())
    assert opt.last_skipped() is None and not bool(opt._report.any()) and opt.skipped_steps == 0


# ----------------------------------------------------------------------------- 6. the report changes nothing
@pytest.mark.parametrize("hyper", [False, True], ids=["by-value", "hyper"])
@pytest.mark.parametrize("clip", [False, True], ids=["skip", "clip+skip"])
def test_the_report_changes_nothing(clip, hyper):
    norm = float(np.sqrt(sum((g.astype(np.float64) ** 2).sum() for g in _grads())))
    kw = dict(skip_nonfinite=True, hyper_on_device=hyper, **({"max_grad_norm": 0.5 * norm} if clip else {}))
    off, on = DevSet(), DevSet()
    a, b = _adam(off, **kw), _adam(on, grad_report=True, **kw)
    assert a._report is None and b._report is not None
    for what in ("clean", "skipped", "clean again"):
        for ds in (off, on):
            if what == "skipped":
                ds.poison(20, 100, NAN)
            elif what == "clean again":
                ds.heal(20)
        a.step(); b.step()
        torch.cuda.synchronize()
        assert torch.equal(_bits(a._guard), _bits(b._guard)), f"{what}: guard records {a._guard.tolist()} / {b._guard.tolist()}"
        assert torch.equal(_bits(a._guard_step), _bits(b._guard_step)), what
        for i, (p, q) in enumerate(zip(off.params, on.params)):
            assert torch.equal(_bits(p), _bits(q)), f"{what}: parameter {i}"
            if p.grad is not None:
                for key in ("exp_avg", "exp_avg_sq"):
                    assert torch.equal(_bits(a.state[p][key]), _bits(b.state[q][key])), f"{what}: {key} of parameter {i}"
    assert a.skipped_steps == b.skipped_steps == 1 and float(a._guard_step) == 2.0
    assert any(bool(p.detach().ne(0).any()) for p in on.params), "no step was taken at all"


# ----------------------------------------------------------------------------- 7. under a graph
def test_latch_names_the_poisoned_replay_of_a_graph():
    pick = [1, 2, 5, 6, len(SIZES) + 6, N_REAL - 1]            # 3, 4, 4097, 8193 elements, 8193 unaligned, 250
    ds = DevSet(which=pick)
    from wsmgmap import optim
    opt = optim.Adam(ds.params, lr=LR, max_grad_norm=1e3, skip_nonfinite=True, grad_report=True)
    opt.step()                                 # eager: the moments exist and every kernel has been launched before the capture
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        opt.step()
    opt.note_replayed_steps(-1)                # capture ran the host bookkeeping once without executing anything
    for k in range(4):
        if k == 1:
            ds.grads[3][4096] = NAN
        if k == 2:
            ds.grads[3].copy_(T(ds.host[3]))
        graph.replay()
        opt.note_replayed_steps(1)
    ls = opt.last_skipped(["a", "b", "c", "d", "e", "f"])
    assert ls is not None and ls.first_nonfinite.index == 3 and ls.first_nonfinite.name == "d"
    assert ls.attempt == 3 and ls.skipped == 1 and (ls.first_nonfinite.nan, ls.first_nonfinite.inf) == (1, 0)
    assert ls.nonfinite_tensors == 1 and ls.largest.index == 3
    _check_table("fourth replay", _stats_table(opt.grad_report()), ds.host)
    assert opt.skipped_steps == 1 and float(opt._guard_step) == 4.0 and opt.state[ds.params[0]]["step"] == 5


# ----------------------------------------------------------------------------- 8. the policy's update
class _Box:
    shape = (2,)


def test_policy_update_names_the_poisoned_parameter():
    """The T = 4 x N = 2 float32 update of test_policy_update_skips_a_poisoned_gradient_and_clips_a_clean_one."""
    from wsmgmap import optim
    from wsmgmap.common.aux_losses import AuxLosses
    from wsmgmap.config import default_model_config
    from wsmgmap.models.policy import BasePolicy
    obs_np, prev, masks, weights = cases.update_inputs(4, 2, n_tok=(80, 37), tag="adam")
    policy = BasePolicy(None, _Box(), default_model_config(num_proc=2, compute_dtype="f32"))
    policy.load_state_dict(state_dict_values(), strict=True)
    policy.net.instruction_encoder.embedding_layer.weight.requires_grad_(False)
    policy = policy.cuda()
    policy.train(); policy.net.depth_encoder.eval(); policy.net.rgb_encoder.eval()
    obs = {k: T(v).cuda() for k, v in obs_np.items()}
    prev, masks, weights = T(prev).cuda(), T(masks).cuda(), T(weights).cuda()
    AuxLosses.activate(); AuxLosses.clear()
    pred, aux = policy(dict(obs), torch.zeros(2, 2, 512, device="cuda"), prev, masks, weights)
    ((pred ** 2).mean() + aux).backward()
    AuxLosses.deactivate()
    named = list(policy.named_parameters())
    live = [p for _, p in named if p.grad is not None]
    assert len(live) > 96 and len(live) < len(named)
    norm = float(optim.global_grad_norm(policy.parameters()))
    opt = optim.Adam(policy.parameters(), lr=LR, max_grad_norm=0.5 * norm, skip_nonfinite=True, grad_report=True)
    victim = live[len(live) // 2]
    victim.grad.view(-1)[7 % victim.numel()] = NAN
    opt.step()
    ls = opt.last_skipped(policy)
    want = next(name for name, p in named if p is victim)
    assert opt.skipped_steps == 1 and ls is not None and ls.attempt == 1
    assert ls.first_nonfinite.name == want and ls.first_nonfinite.index == [id(p) for _, p in named].index(id(victim))
    assert (ls.first_nonfinite.nan, ls.first_nonfinite.inf, ls.nonfinite_tensors) == (1, 0, 1)
    assert [s.name for s in ls.stats] == [name for name, _ in named]
    for s, (name, p) in zip(ls.stats, named):
        if p.grad is None:
            assert (s.norm, s.max_abs, s.nan, s.inf) == (0.0, 0.0, 0, 0), f"{name}: a parameter without a gradient has a non-zero row"
        elif p is not victim:
            y = _yard(p.grad.cpu().numpy())
            assert (s.nan, s.inf) == (0, 0) and np.float32(s.max_abs) == y[1] and abs(s.norm - float(y[0])) <= NORM_RTOL * float(y[0]), name


# ----------------------------------------------------------------------------- 9. refusals launch nothing
def test_rejected_arguments_launch_nothing():
    from wsmgmap import _abi
    from wsmgmap.optim import _AdamDesc
    L = _abi.lib()
    ds = DevSet()
    n = N_REAL
    descs = (_AdamDesc * n)()
    for d, g in zip(descs, ds.grads):
        d.grad, d.n = g.data_ptr(), g.numel()
    partials = torch.full((TOTAL_BLOCKS + 4,), -7.0, device="cuda", dtype=torch.float64)
    scan = torch.full((4 * TOTAL_BLOCKS + 8,), -7, device="cuda", dtype=torch.int32)
    report = torch.full((4 * n + 4,), -7, device="cuda", dtype=torch.int32)
    latch = torch.full((8 + 4 * n + 4,), -7, device="cuda", dtype=torch.int32)
    guard = torch.tensor([1.0, 1.0, 1.0, 3.0], device="cuda")             # a record that says "skipped": a launched latch would write
    step = torch.full((2,), 5.0, device="cuda")
    torch.cuda.synchronize()
    args = dict(descs=descs, n=n, partials=_ptr(partials), pcap=TOTAL_BLOCKS, scan=_ptr(scan), scap=TOTAL_BLOCKS, guard=_ptr(guard),
                step=_ptr(step), report=_ptr(report), latch=_ptr(latch))

    def rep(**kw):
        a = {**args, **kw}
        return L.wsmg_grad_report_multi(a["descs"], a["n"], a["partials"], a["pcap"], a["scan"], a["scap"], a["guard"], a["step"],
                                        a["report"], a["latch"], _stream())

    def stats(**kw):
        a = {**args, **kw}
        return L.wsmg_grad_stats_multi(a["descs"], a["n"], a["partials"], a["pcap"], a["scan"], a["scap"], a["report"], _stream())
    huge, odd = (_AdamDesc * n)(), (_AdamDesc * n)()
    many = (_AdamDesc * 1025)()                # 1025 x 2^20 chunks: above 2^30 in all, each tensor below 2^32 elements
    for src, dst in ((descs, huge), (descs, odd)):
        for s, d in zip(src, dst):
            d.grad, d.n = s.grad, s.n
    huge[3].n = 1 << 32
    odd[4].grad = ds.grads[4].data_ptr() + 2
    for d in many:
        d.grad, d.n = ds.grads[0].data_ptr(), (1 << 32) - 1
    for f in (rep, stats):
        for key in ("descs", "partials", "scan", "report"):
            assert f(**{key: None}) == -1, (f.__name__, key)
        assert f(partials=_ptr(partials, 4)) == -1 and f(scan=_ptr(scan, 2)) == -1 and f(report=_ptr(report, 2)) == -1
        assert f(n=-1) == -1 and f(pcap=-1) == -1 and f(scap=-1) == -1
        assert f(descs=huge) == -1 and f(descs=odd) == -1
        assert f(descs=many, n=1025, pcap=1 << 40, scap=1 << 40) == -1
        assert f(pcap=TOTAL_BLOCKS - 1) == -2 and f(scap=TOTAL_BLOCKS - 1) == -2            # WSMG_ENOMEM
    assert rep(guard=None, step=None) == -1                   # latch without guard
    assert rep(step=None) == -1 and rep(guard=None, latch=None) == -1        # guard without step_dev, and the reverse
    assert rep(guard=_ptr(guard, 2)) == -1 and rep(step=_ptr(step, 2)) == -1 and rep(latch=_ptr(latch, 2)) == -1
    torch.cuda.synchronize()
    assert bool((partials == -7.0).all()) and bool((scan == -7).all()) and bool((report == -7).all()) and bool((latch == -7).all())
    assert guard.tolist() == [1.0, 1.0, 1.0, 3.0] and step.tolist() == [5.0, 5.0]
    # and the same arguments, complete, run: exactly the tables' used parts are written, the record and the count are only read
    assert stats() == 0 and rep() == 0
    torch.cuda.synchronize()
    assert bool((partials[TOTAL_BLOCKS:] == -7.0).all()) and bool((scan[4 * TOTAL_BLOCKS:] == -7).all())
    assert bool((report[4 * n:] == -7).all()) and bool((latch[8 + 4 * n:] == -7).all())
    assert guard.tolist() == [1.0, 1.0, 1.0, 3.0] and step.tolist() == [5.0, 5.0]
    _check_table("entry points", report[:4 * n].view(n, 4), ds.host)
    assert latch[:8].tolist() == [3, 8, -1, int(np.argmax([_yard(g)[0] for g in ds.host])), 0, 0, 0, 0]
    assert torch.equal(latch[8:8 + 4 * n], report[:4 * n])
    assert rep(guard=None, step=None, latch=None) == 0       # the report alone behind someone else's partials
