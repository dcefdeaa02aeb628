"""GPU: Adam's hyper-parameters read from a device record (csrc/wsmg_optim.hip: adam_multi_hyper_kernel,
adam_multi_guarded_hyper_kernel, grad_guard_finalize_hyper_kernel; wsmg_adam_step_multi_hyper, wsmg_grad_norm_multi_hyper;
wsmgmap.optim.Adam(hyper_on_device=True).sync_hyper(); wsmgmap.graph.GraphedUpdate), so that a step captured in a HIP graph follows
`param_groups` edits, `torch.optim.lr_scheduler` and a new `max_grad_norm`.

Three yardsticks.  (1) THE SAME BITS as the by-value kernels (adam_multi_kernel, adam_multi_guarded_kernel,
grad_guard_finalize_kernel: the same element step, adam1, behind another front end) for equal values — `torch.equal` on int32 views, no
tolerance.
(2) float64 `torch.optim.Adam` (+ `clip_grad_norm_`) on the same schedule at the project's Adam bar, rtol 2e-6 / atol 1e-7, not
widened: the record adds no rounding (the values reach the kernel as the float32 a by-value argument would be).  (3) What the flag is
for: a replayed graph steps with the values of NOW; without the flag it steps with the values of its capture (asserted too).

Tensors as tests/adam_util.py lays them out: sizes around the 4-element vector and the 4 096-element workgroup, once 16-byte
aligned and once one float off, then ragged small sizes up to 50 tensors (the table of 48 spills into a second launch); values from
oracle.detfill."""
import functools
import warnings

import numpy as np
import pytest
import torch

import adam_util
from adam_util import ALL_SIZES, SIZES, TOTAL_BLOCKS, _bits, _norm64, _ptr, _stream
from oracle import cases
from util import T, state_dict_values

pytestmark = pytest.mark.gpu

EPS = 1e-8
RTOL, ATOL = 2e-6, 1e-7
# (lr, weight_decay, betas) of four consecutive steps: each of the three changes at least once
SCHED = [(2.5e-4, 0.0, (0.9, 0.999)), (1.25e-4, 0.01, (0.9, 0.999)), (1.25e-4, 0.01, (0.8, 0.99)), (5e-5, 0.0, (0.85, 0.995))]
PICK = [1, 2, 5, 6, len(SIZES) + 6, len(ALL_SIZES) - 1]            # 3, 4, 4097, 8193 elements, 8193 unaligned, 250: the graph tests
_values = functools.partial(adam_util._values, "hyper")            # this file's numbers
DevSet = functools.partial(adam_util.DevSet, "hyper")


def _split(items, n_groups):
    """One group, or two: the 14 tensors around the vector / workgroup sizes and the ragged rest."""
    return [list(items)] if n_groups == 1 else [list(items[:2 * len(SIZES)]), list(items[2 * len(SIZES):])]


def _group_hyper(step, j):
    """Group j's (lr, weight_decay, betas) at schedule entry `step`: the second group differs in lr and weight_decay."""
    lr, wd, betas = SCHED[step]
    return lr * (1 + j), wd + 0.005 * j, betas


def _apply(opt, step):
    for j, group in enumerate(opt.param_groups):
        group["lr"], group["weight_decay"], group["betas"] = _group_hyper(step, j)


def _adam(ds, n_groups=1, **kw):
    """wsmgmap.optim.Adam over the set's parameters (in n_groups groups) with the set's moments at step 0 through load_state_dict, so
    that the first step already runs on non-zero moments; hyper-parameters of schedule entry 0."""
    from wsmgmap import optim
    params = ds.params()
    groups = [{"params": g} for g in _split(params, n_groups)]
    opt = optim.Adam(groups, lr=1e-3, eps=EPS, **kw)
    sd = opt.state_dict()
    sd["state"] = {i: {"step": torch.tensor(0.0), "exp_avg": row[2], "exp_avg_sq": row[3]} for i, row in enumerate(ds.views)}
    opt.load_state_dict(sd)
    _apply(opt, 0)
    return params, opt


def _state(params, opt):
    """[(p, exp_avg, exp_avg_sq)] per parameter."""
    return [(p, opt.state[p]["exp_avg"], opt.state[p]["exp_avg_sq"]) for p in params]


def _same_bits(name, params_a, opt_a, params_b, opt_b):
    for i, (a, b) in enumerate(zip(_state(params_a, opt_a), _state(params_b, opt_b))):
        for what, x, y in zip("pmv", a, b):
            assert torch.equal(_bits(x), _bits(y)), f"{name}: tensor {i} ({x.numel()} elements) {what} differs from the by-value step"
    if opt_a._guard is not None:
        assert torch.equal(_bits(opt_a._guard), _bits(opt_b._guard)), f"{name}: guard record {opt_a._guard.tolist()} != {opt_b._guard.tolist()}"
        assert float(opt_a._guard_step) == float(opt_b._guard_step), f"{name}: device step count"
    for ka, kb in zip(opt_a._step_dev.values(), opt_b._step_dev.values()):
        assert float(ka) == float(kb), f"{name}: device step count"


def _form(form, values):
    return dict(capturable=True) if form == "capturable" else dict(max_grad_norm=0.5 * _norm64(values), skip_nonfinite=True)


def _float64_adam(values, n_groups=1):
    """(parameters, torch.optim.Adam) in float64 over the values, with their moments at step 0."""
    qs = [torch.nn.Parameter(T(p).double()) for _, (p, _, _, _) in values]
    ref = torch.optim.Adam([{"params": g} for g in _split(qs, n_groups)], lr=1e-3, eps=EPS)
    for q, (_, (_, _, m, v)) in zip(qs, values):
        ref.state[q] = {"step": torch.tensor(0.0), "exp_avg": T(m).double().clone(), "exp_avg_sq": T(v).double().clone()}
    return qs, ref


def _float64_step(qs, ref, values, max_norm=None):
    for q, (_, (_, g, _, _)) in zip(qs, values):
        q.grad = T(g).double().clone()
    if max_norm is not None:
        torch.nn.utils.clip_grad_norm_(qs, max_norm)
    ref.step()


def _within_the_adam_bar(name, qs, ref, state):
    """Parameters and both moments ([(p, exp_avg, exp_avg_sq)]) against the float64 optimizer's at rtol 2e-6 / atol 1e-7."""
    worst = 0.0
    for i, (q, (p, m, v)) in enumerate(zip(qs, state)):
        s = ref.state[q]
        for what, got, want in (("p", p, q.detach()), ("m", m, s["exp_avg"]), ("v", v, s["exp_avg_sq"])):
            got = got.detach().double().cpu().reshape(want.shape)
            worst = max(worst, float(((got - want).abs() / (ATOL / RTOL + want.abs())).max()))
            torch.testing.assert_close(got, want, rtol=RTOL, atol=ATOL, msg=lambda t: f"tensor {i} {what}: {t}")
    print(f"{name}: worst |err| / (atol/rtol + |ref|) against float64 = {worst:.3e} (bar {RTOL:.1e})")


def _record_rows(opt):
    """What the record should hold, as float32 rows."""
    rows = [[g["lr"], g["betas"][0], g["betas"][1], g["eps"], g["weight_decay"], 0, 0, 0] for g in opt.param_groups]
    rows.append([opt.max_grad_norm or 0.0] + [0] * 7)
    return torch.tensor(rows, dtype=torch.float32)


# ----------------------------------------------------------------------------- 1 + 2. same bits as by value; float64 torch.optim.Adam
@pytest.mark.parametrize("n_groups", [1, 2])
@pytest.mark.parametrize("form", ["capturable", "guarded"])
def test_schedule_gives_the_by_value_bits_and_matches_float64_adam(form, n_groups):
    """Four eager steps, lr / weight_decay / betas changed in `param_groups` between them (two groups: different values per row of
    the record): parameters, both moments, the guard record and the device step count of the hyper_on_device optimizer are
    bit-identical to a twin without the flag after every step — the twin runs the parent commit's kernels — and both sit within the
    Adam bar of float64 clip_grad_norm_ + torch.optim.Adam on the same schedule.  One group: all 50 tensors in one call, so the Adam
    table spills into a second launch; guarded: max_grad_norm = half the norm, so every step is clipped."""
    values = _values()
    kw = _form(form, values)
    da, db = DevSet(), DevSet()
    pa, oa = _adam(da, n_groups, hyper_on_device=True, **kw)
    pb, ob = _adam(db, n_groups, **kw)
    assert oa.hyper_record.shape == (n_groups + 1, 8) and oa._hyper_stage.is_pinned()
    qs, ref = _float64_adam(values, n_groups)                       # the float64 oracle
    for k in range(len(SCHED)):
        for opt in (oa, ob, ref):
            _apply(opt, k)
        oa.step()
        ob.step()
        torch.cuda.synchronize()
        _same_bits(f"{form}, {n_groups} group(s), step {k + 1}", pa, oa, pb, ob)
        assert torch.equal(oa.hyper_record.cpu(), _record_rows(oa)), "the record is not param_groups' values as float32"
        _float64_step(qs, ref, values, kw.get("max_grad_norm"))
    assert oa.sync_hyper() is False                                   # nothing changed since the last step
    if form == "guarded":
        assert float(oa._guard[1]) < 0.51 and oa.skipped_steps == 0 and float(oa._guard_step) == len(SCHED)
    _within_the_adam_bar(f"{form}, {n_groups} group(s)", qs, ref, _state(pa, oa))
    assert da.slack_untouched() and db.slack_untouched()


# ----------------------------------------------------------------------------- 1b. the one element step where the three loops meet
MEET = [(1, 0), (3, 0), (4, 0), (7, 0), (4096, 0), (4097, 0), (4097, 1), (8195, 0)]     # (elements, floats off a 16-byte boundary)


@functools.lru_cache(maxsize=None)
def _meet_values():
    """One set in which the 16-byte body, its scalar tail and the misaligned scalar loop all run and a tensor crosses a chunk edge:
    4 097 elements once aligned (a body of 4 096, then a second workgroup's tail of one) and once one float off; 8 195 = two full
    chunks and a tail of three; 1, 3, 7: tails only or a body of one vector."""
    return [adam_util._fill(f"hyper.meet.{i}", off, n) for i, (n, off) in enumerate(MEET)]


def test_one_element_step_on_every_loop_gives_every_front_end_the_same_bits():
    """Three steps with weight_decay = 0.01 (schedule entry 1) through the capturable by-value form and its hyper_on_device twin,
    and through the guarded pair clipped at half the norm (coef < 1): within each pair parameters, both moments, the guard record
    and the device step count are equal bit for bit after every step, and all four sit inside the Adam bar of float64
    clip_grad_norm_ + torch.optim.Adam."""
    values = _meet_values()
    for form in ("capturable", "guarded"):
        kw = _form(form, values)
        da, db = DevSet(values=values), DevSet(values=values)
        pa, oa = _adam(da, hyper_on_device=True, **kw)
        pb, ob = _adam(db, **kw)
        qs, ref = _float64_adam(values)
        for opt in (oa, ob, ref):
            _apply(opt, 1)
        assert oa.param_groups[0]["weight_decay"] == 0.01
        for k in range(3):
            oa.step()
            ob.step()
            torch.cuda.synchronize()
            _same_bits(f"{form}, step {k + 1}", pa, oa, pb, ob)
            _float64_step(qs, ref, values, kw.get("max_grad_norm"))
        assert _device_step(oa) == _device_step(ob) == 3.0
        if form == "guarded":
            assert float(oa._guard[1]) < 0.51 and float(ob._guard[1]) < 0.51 and oa.skipped_steps == 0
        _within_the_adam_bar(f"{form}, hyper_on_device", qs, ref, _state(pa, oa))
        _within_the_adam_bar(f"{form}, by value", qs, ref, _state(pb, ob))
        assert da.slack_untouched() and db.slack_untouched()


# ----------------------------------------------------------------------------- 3 + 4. inside a HIP graph
def _captured(form, n_groups=2):
    """(graph, set, params, opt) with opt.step() captured after one eager step, and (set, params, opt) of the eager by-value twin after
    the same step.  Six small tensors with static gradient buffers, in two groups (the 4-tensor group and the 2-tensor group)."""
    values = [_values()[i] for i in PICK]
    kw = _form(form, values)
    ds, twin = DevSet(values=values), DevSet(values=values)
    from wsmgmap import optim

    def make(s, **more):
        params = s.params()
        opt = optim.Adam([{"params": params[:4]}, {"params": params[4:]}], lr=1e-3, eps=EPS, **kw, **more)
        sd = opt.state_dict()
        sd["state"] = {i: {"step": torch.tensor(0.0), "exp_avg": row[2], "exp_avg_sq": row[3]} for i, row in enumerate(s.views)}
        opt.load_state_dict(sd)
        _apply(opt, 0)
        return params, opt
    params, opt = make(ds, hyper_on_device=True)
    tparams, topt = make(twin)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        opt.step()                      # the kernels' first launches and the device step counters: outside the capture
        topt.step()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        opt.step()
    opt.note_replayed_steps(-1)         # capture ran the host bookkeeping once without executing anything
    torch.cuda.synchronize()
    _same_bits(f"{form}: after the eager step and the capture", params, opt, tparams, topt)
    return graph, ds, params, opt, twin, tparams, topt


def _device_step(opt):
    return float(opt._guard_step) if opt._guard_step is not None else float(next(iter(opt._step_dev.values())))


@pytest.mark.parametrize("form", ["capturable", "guarded"])
def test_graph_replay_follows_the_schedule(form):
    """THE test of the flag (it fails on the by-value kernels: a replay steps with the values of its capture).  One eager step,
    `step()` captured with torch.cuda.graph, a StepLR scheduler attached; before each of three replays the scheduler steps (and
    weight_decay / betas are edited by hand once) and sync_hyper() is called: bit-identical to the eager by-value twin stepped with
    the same values.  Then lr = 0: a replay leaves every parameter's bits alone while moments and the device step count advance.
    Guarded: a new max_grad_norm between replays puts the float32 value of clip_grad_norm_'s formula into guard[coef]."""
    graph, ds, params, opt, twin, tparams, topt = _captured(form)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")           # (no optimizer.step() call between scheduler steps: the graph steps)
        sched = torch.optim.lr_scheduler.StepLR(opt, step_size=1, gamma=0.5)
        tsched = torch.optim.lr_scheduler.StepLR(topt, step_size=1, gamma=0.5)
        for k in range(3):
            sched.step()
            tsched.step()
            if k == 1:
                for o in (opt, topt):
                    o.param_groups[0]["weight_decay"] = 0.02
                    o.param_groups[1]["betas"] = (0.8, 0.99)
            assert opt.param_groups[0]["lr"] == SCHED[0][0] * 0.5 ** (k + 1) and opt.param_groups[1]["lr"] == 2 * opt.param_groups[0]["lr"]
            assert opt.sync_hyper() is True and opt.sync_hyper() is False
            graph.replay()
            opt.note_replayed_steps(1)
            topt.step()
            torch.cuda.synchronize()
            _same_bits(f"{form}: replay {k + 1}", params, opt, tparams, topt)
    assert _device_step(opt) == 4.0 and float(opt.state_dict()["state"][0]["step"]) == 4.0
    # lr = 0
    for o in (opt, topt):
        for g in o.param_groups:
            g["lr"] = 0.0
    before = [(_bits(p).clone(), _bits(m).clone(), _bits(v).clone()) for p, m, v in _state(params, opt)]
    assert opt.sync_hyper() is True
    graph.replay()
    opt.note_replayed_steps(1)
    topt.step()
    torch.cuda.synchronize()
    for i, ((p, m, v), (bp, bm, bv)) in enumerate(zip(_state(params, opt), before)):
        assert torch.equal(_bits(p), bp), f"tensor {i}: a replay with lr = 0 moved the parameter"
        assert not torch.equal(_bits(m), bm) and not torch.equal(_bits(v), bv), f"tensor {i}: the moments did not advance"
    assert _device_step(opt) == 5.0
    _same_bits(f"{form}: lr = 0", params, opt, tparams, topt)
    if form == "guarded":
        norm = opt._guard[0].cpu()
        for factor, clipped in ((0.25, True), (3.0, False)):
            new = factor * float(norm)
            opt.max_grad_norm = new
            topt.max_grad_norm = new
            for o in (opt, topt):
                for g in o.param_groups:
                    g["lr"] = 1e-4
            assert opt.sync_hyper() is True
            graph.replay()
            opt.note_replayed_steps(1)
            topt.step()
            torch.cuda.synchronize()
            want = (torch.tensor(new, dtype=torch.float32) / (norm + 1e-6)).clamp(max=1.0)      # clip_grad_norm_'s formula, float32
            assert want.dtype == torch.float32 and (float(want) < 1.0) == clipped
            assert torch.equal(_bits(opt._guard[1].cpu()), _bits(want)), f"guard[coef] {float(opt._guard[1])!r}, formula {float(want)!r}"
            _same_bits(f"guarded: max_grad_norm = {factor} x norm", params, opt, tparams, topt)
    assert ds.slack_untouched()


def test_skip_under_replay_writes_nothing_and_the_next_replay_uses_the_new_lr():
    """The guard's skip with the record in use: a NaN gradient under replay (with a new lr already synced) writes nothing and does
    not advance the step count; the next replay, clean gradient and another lr, is the by-value twin's next step bit for bit."""
    graph, ds, params, opt, twin, tparams, topt = _captured("guarded")
    g0 = ds.views[3][1]
    good = g0.clone()
    g0[4096] = float("nan")
    for g in opt.param_groups:
        g["lr"] = 7e-5
    before = [(_bits(p).clone(), _bits(m).clone(), _bits(v).clone()) for p, m, v in _state(params, opt)]
    assert opt.sync_hyper() is True
    graph.replay()
    opt.note_replayed_steps(1)
    torch.cuda.synchronize()
    for i, ((p, m, v), (bp, bm, bv)) in enumerate(zip(_state(params, opt), before)):
        assert torch.equal(_bits(p), bp) and torch.equal(_bits(m), bm) and torch.equal(_bits(v), bv), f"tensor {i}: written by a skipped step"
    assert opt.skipped_steps == 1 and _device_step(opt) == 1.0 and not np.isfinite(float(opt.grad_norm))
    g0.copy_(good)
    for o in (opt, topt):
        for j, g in enumerate(o.param_groups):
            g["lr"] = 3e-5 * (1 + j)
    assert opt.sync_hyper() is True
    graph.replay()
    opt.note_replayed_steps(1)
    topt.step()
    torch.cuda.synchronize()
    assert _device_step(opt) == 2.0 and float(opt.state_dict()["state"][0]["step"]) == 2.0
    opt._guard[3] = 0.0                      # (the twin never saw the NaN: compare the rest of the record)
    _same_bits("the replay after the skipped one", params, opt, tparams, topt)


# ----------------------------------------------------------------------------- 5. stale under capture, invalid values
def test_stale_record_under_capture_raises_and_invalid_values_leave_the_record_alone():
    from wsmgmap import _abi, optim
    values = [_values()[i] for i in PICK]
    ds = DevSet(values=values)
    params, opt = _adam(ds, capturable=True, hyper_on_device=True)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        opt.step()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    record = opt.hyper_record.cpu().clone()
    before = [_bits(p).clone() for p in params]
    marker = torch.zeros((), device="cuda")
    opt.param_groups[0]["lr"] = 1e-5                 # ... and no sync_hyper()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        with pytest.raises(_abi.WsmgError, match=r"sync_hyper\(\)"):
            opt.step()
        with pytest.raises(_abi.WsmgError, match=r"sync_hyper\(\)"):
            opt.sync_hyper()
        marker.add_(1.0)                             # (so that the graph is not empty)
    assert {st["step"] for st in opt.state.values()} == {1}, "the refused step ran its host bookkeeping"
    graph.replay()
    torch.cuda.synchronize()
    assert float(marker) == 1.0 and _device_step(opt) == 1.0, "the refused step was captured"
    assert all(torch.equal(_bits(p), b) for p, b in zip(params, before))
    assert torch.equal(opt.hyper_record.cpu(), record)
    # invalid values: ValueError from sync_hyper() and from step(), the record keeps its contents
    for key, bad in (("lr", -1.0), ("eps", -1e-8), ("weight_decay", -0.1), ("betas", (1.0, 0.999)), ("betas", (0.9, -0.1))):
        keep = opt.param_groups[0][key]
        opt.param_groups[0][key] = bad
        with pytest.raises(ValueError):
            opt.sync_hyper()
        with pytest.raises(ValueError):
            opt.step()
        opt.param_groups[0][key] = keep
    torch.cuda.synchronize()
    assert torch.equal(opt.hyper_record.cpu(), record) and all(torch.equal(_bits(p), b) for p, b in zip(params, before))
    assert {st["step"] for st in opt.state.values()} == {1}
    opt.param_groups[0]["lr"] = torch.tensor(2e-5)   # a tensor-valued lr is read with float()
    assert opt.sync_hyper() is True
    torch.cuda.synchronize()
    assert float(opt.hyper_record[0, 0]) == float(np.float32(2e-5))
    guarded = optim.Adam(ds.params(), max_grad_norm=1.0, hyper_on_device=True)
    guarded.max_grad_norm = 2.5
    assert guarded.sync_hyper() is True and guarded.hyper_record[1].tolist() == [2.5] + [0.0] * 7
    with pytest.raises(ValueError):
        guarded.add_param_group({"params": [torch.nn.Parameter(torch.zeros(3, device="cuda"))]})


# ----------------------------------------------------------------------------- 6. argument checks, before any launch
def test_rejected_arguments_launch_nothing():
    from wsmgmap import _abi
    L = _abi.lib()
    ds = DevSet()
    descs, n = ds.descs(), len(ds.views)
    partials = torch.full((TOTAL_BLOCKS + 4,), -7.0, device="cuda", dtype=torch.float64)
    guard = torch.full((4,), -7.0, device="cuda")
    step = torch.full((2,), 5.0, device="cuda")
    record = torch.tensor([2.5e-4, 0.9, 0.999, EPS, 0.0, 0, 0, 0, 1.0, 0, 0, 0, 0, 0, 0, 0], device="cuda")
    snap = [buf.clone() for _, _, buf in ds.bufs]
    torch.cuda.synchronize()
    args = dict(descs=descs, n=n, partials=_ptr(partials), cap=TOTAL_BLOCKS, row=_ptr(record, 32), skip=1, guard=_ptr(guard), step=_ptr(step))

    def norm(**kw):
        a = {**args, **kw}
        return L.wsmg_grad_norm_multi_hyper(a["descs"], a["n"], a["partials"], a["cap"], a["row"], a["skip"], a["guard"], a["step"], _stream())

    def adam(**kw):
        a = {"row": _ptr(record), **{k: args[k] for k in ("descs", "n", "step", "guard")}, **kw}
        return L.wsmg_adam_step_multi_hyper(a["descs"], a["n"], a["row"], a["step"], a["guard"], _stream())
    assert norm(cap=TOTAL_BLOCKS - 1) == -2                                      # WSMG_ENOMEM: one partial short
    assert norm(row=None) == -1 and norm(row=_ptr(record, 34)) == -1             # WSMG_EINVAL: null row, misaligned row
    assert norm(guard=None) == -1 and norm(partials=None) == -1 and norm(n=-1) == -1 and norm(cap=-1) == -1 and norm(descs=None) == -1
    assert norm(guard=_ptr(guard, 2)) == -1 and norm(step=_ptr(step, 2)) == -1 and norm(partials=_ptr(partials, 4)) == -1
    assert adam(row=None) == -1 and adam(row=_ptr(record, 2)) == -1
    assert adam(step=None) == -1 and adam(step=_ptr(step, 2)) == -1 and adam(guard=_ptr(guard, 2)) == -1
    assert adam(n=-1) == -1 and adam(descs=None) == -1
    bad = ds.descs()
    bad[n - 1].exp_avg = None                        # the LAST descriptor (second launch of the table): nothing before it may run
    assert adam(descs=bad) == -1
    bad = ds.descs()
    bad[n - 1].grad = bad[n - 1].grad + 2
    assert adam(descs=bad) == -1
    torch.cuda.synchronize()
    assert bool((partials == -7.0).all()) and bool((guard == -7.0).all()) and step.tolist() == [5.0, 5.0]
    assert all(torch.equal(_bits(buf), _bits(s)) for (_, _, buf), s in zip(ds.bufs, snap))
    assert norm() == 0                                                           # and the same arguments, complete, run
    torch.cuda.synchronize()
    assert step.tolist() == [6.0, 5.0] and bool((partials[TOTAL_BLOCKS:] == -7.0).all()) and guard[2:].tolist() == [0.0, -7.0]
    norm64 = _norm64(_values())
    assert abs(float(guard[0]) - norm64) <= 2e-7 * norm64
    assert float(guard[1]) == float(np.float32(1.0) / (np.float32(guard[0].item()) + np.float32(1e-6)))
    assert adam() == 0
    torch.cuda.synchronize()
    assert any(not torch.equal(_bits(buf), _bits(s)) for (_, _, buf), s in zip(ds.bufs, snap)) and ds.slack_untouched()
    assert record.tolist()[8:] == [1.0] + [0.0] * 7 and record[5:8].tolist() == [0.0] * 3    # no kernel writes the record


# ----------------------------------------------------------------------------- 7. state_dict round trip
def test_state_dict_round_trip_rebuilds_the_record():
    """Two steps on a schedule, state_dict() -> a new optimizer constructed with other values -> load_state_dict(): the record holds
    the loaded groups' values and the next step is the uninterrupted twin's, bit for bit."""
    from wsmgmap import optim
    values = _values()
    kw = _form("guarded", values)
    da, db = DevSet(), DevSet()
    pa, oa = _adam(da, 2, hyper_on_device=True, **kw)
    pb, ob = _adam(db, 2, hyper_on_device=True, **kw)
    for k in range(2):
        for o in (oa, ob):
            _apply(o, k)
            o.step()
    sd = ob.state_dict()
    assert set(sd) == {"state", "param_groups"} and not any("hyper" in k for g in sd["param_groups"] for k in g)
    pc = db.params()
    oc = optim.Adam([{"params": g} for g in _split(pc, 2)], lr=0.5, betas=(0.5, 0.5), eps=1e-3, weight_decay=0.3, hyper_on_device=True, **kw)
    torch.cuda.synchronize()
    assert oc.hyper_record[0].tolist() == [0.5, 0.5, 0.5, float(np.float32(1e-3)), float(np.float32(0.3)), 0.0, 0.0, 0.0]
    oc.load_state_dict(sd)
    torch.cuda.synchronize()
    assert torch.equal(oc.hyper_record.cpu(), _record_rows(ob)) and torch.equal(oc.hyper_record.cpu(), _record_rows(oc))
    assert oc.sync_hyper() is False and float(oc._guard_step) == 2.0
    for o in (oa, oc):
        _apply(o, 2)
        o.step()
    torch.cuda.synchronize()
    _same_bits("the step after load_state_dict", pa, oa, pc, oc)
    assert float(oc.state_dict()["state"][0]["step"]) == 3.0


# ----------------------------------------------------------------------------- 8. the policy's update as a graph
class _Box:
    shape = (2,)


def _policy():
    from wsmgmap.config import default_model_config
    from wsmgmap.models.policy import BasePolicy
    pol = BasePolicy(None, _Box(), default_model_config(num_proc=2, compute_dtype="f32"))
    pol.load_state_dict(state_dict_values(), strict=True)
    pol.net.instruction_encoder.embedding_layer.weight.requires_grad_(False)
    pol = pol.cuda()
    pol.train(); pol.net.depth_encoder.eval(); pol.net.rgb_encoder.eval()
    return pol


def _loss_fn(pred, aux, o, w):
    return (pred ** 2).mean() + aux


LRS = [1e-5, 1e-5, 1e-5, 5e-6, 2.5e-6, 0.0]       # per call: two eager, the capture + first replay, two replays at new values, lr = 0


def _graphed_sequence(flag):
    """Six GraphedUpdate calls at T = 4 x N = 2 (float32 mode, eager_calls = 2, the inputs of test_graphed_update_matches_eager_updates)
    with lr set in param_groups before each: (policy, optimizer, graph owner, losses of the first five, did the sixth move a parameter)."""
    from wsmgmap import optim
    from wsmgmap.graph import GraphedUpdate
    obs_np, prev, masks, weights = cases.update_inputs(4, 2, n_tok=(80, 37), tag="graph")
    obs = {k: T(v).cuda() for k, v in obs_np.items()}
    prev, masks, weights = T(prev).cuda(), T(masks).cuda(), T(weights).cuda()
    pol = _policy()
    opt = optim.Adam(pol.parameters(), lr=LRS[0], capturable=True, hyper_on_device=flag)
    gu = GraphedUpdate(pol, opt, _loss_fn, eager_calls=2)
    losses, moved = [], None
    for k, lr in enumerate(LRS):
        opt.param_groups[0]["lr"] = lr
        if k == len(LRS) - 1:
            torch.cuda.synchronize()
            before = [_bits(p).clone() for p in pol.parameters()]
        loss = float(gu(obs, torch.zeros(2, 2, 512, device="cuda"), prev, masks, weights))
        if k < len(LRS) - 1:
            losses.append(loss)
    torch.cuda.synchronize()
    moved = [n for (n, p), b in zip(pol.named_parameters(), before) if not torch.equal(_bits(p), b)]
    return pol, opt, gu, losses, moved, (obs, prev, masks, weights)


def test_graphed_update_follows_param_groups_edits():
    """Five updates, lr halved twice after the capture, against an eager by-value twin on the same schedule at the bars of
    test_graphed_update_matches_eager_updates (rtol 3e-3 / atol 1e-5 on losses, 2e-4 max(1, |y|) on parameters; one graph).  Those
    bars are lr-limited and cannot see a stale lr, so a sixth call with lr = 0 must leave every parameter bit-identical."""
    from wsmgmap import ops, optim
    from wsmgmap.common.aux_losses import AuxLosses
    AuxLosses.activate()
    pa, oa, gu, la, moved, (obs, prev, masks, weights) = _graphed_sequence(True)
    assert len(gu._graphs) == 1 and gu.calls == 6
    assert not moved, f"a replay with lr = 0 moved {len(moved)} parameter tensors: {moved[:4]}"
    assert {int(v["step"]) for v in oa.state.values()} == {6} and float(next(iter(oa._step_dev.values()))) == 6.0
    pb = _policy()
    ob = optim.Adam(pb.parameters(), lr=LRS[0])
    lb = []
    for lr in LRS[:5]:
        ob.param_groups[0]["lr"] = lr
        ob.zero_grad(set_to_none=True)
        AuxLosses.clear()
        pred, aux = pb(dict(obs), torch.zeros(2, 2, 512, device="cuda"), prev, masks, weights)
        loss = _loss_fn(pred, aux, obs, weights)
        loss.backward()
        ob.step()
        lb.append(float(loss))
    print("losses graph", la, "eager", lb)
    np.testing.assert_allclose(la, lb, rtol=3e-3, atol=1e-5)
    for (n, x), y in zip(pa.named_parameters(), pb.parameters()):       # (the sixth call changed no parameter of pa)
        assert float((x - y).abs().max()) <= 2e-4 * max(1.0, float(y.abs().max())), n
    AuxLosses.deactivate()
    ops.check_rnn_status()


def test_graphed_update_without_the_flag_steps_with_the_captured_lr():
    """What the flag is for: the same six calls with hyper_on_device=False — the sixth, lr = 0 in param_groups, still moves the
    parameters, because the replayed kernel arguments hold the lr of the capture."""
    from wsmgmap import ops
    from wsmgmap.common.aux_losses import AuxLosses
    AuxLosses.activate()
    _, opt, gu, _, moved, _ = _graphed_sequence(False)
    assert len(gu._graphs) == 1 and opt.sync_hyper() is False
    assert len(moved) > 90, f"only {len(moved)} parameter tensors moved"
    AuxLosses.deactivate()
    ops.check_rnn_status()
