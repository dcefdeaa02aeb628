"""GPU: amsgrad, maximize and the decoupled weight decay of the Adam step (csrc/wsmg_optim.hip: adam_multi_ext_kernel<GUARD, HYPER,
AMSGRAD>; wsmg_adam_step_multi_ext, _dev_ext, _guarded_ext, _hyper_ext; wsmgmap.optim.Adam(amsgrad=..., maximize=...),
wsmgmap.optim.AdamW) against float64 `torch.optim.Adam` / `torch.optim.AdamW` on the CPU.

Tensors as tests/adam_util.py lays them out: sizes around the 4-element vector and the 4 096-element workgroup, once 16-byte aligned and
once one float off, then ragged small sizes up to 50 tensors (the table of 48 spills into a second launch); values from oracle.detfill.
max_exp_avg_sq is a fifth view per tensor, laid out the same way (8 floats of zeroed slack, the same offset from a 16-byte boundary).

THE BAR of every stepped comparison is the existing Adam bar, rtol 2e-6 / atol 1e-7 (tests/test_gpu_adam_guard.py), not widened.  What
the options add to a plain step: maximize — nothing (a sign); amsgrad — nothing (a selection; sqrt reads another exact float32);
decoupled decay — the float32 rounding of the factor 1 - lr wd (3e-8 relative: half an ulp below 1) and of the product p * factor
(6e-8), 9e-8 on p per step and under 3e-7 over the three steps taken here."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import adam_util
from adam_util import ALL_SIZES, SIZES, TOTAL_BLOCKS, _bits, _norm64, _ptr, _stream
from oracle import cases
from util import T, state_dict_values

pytestmark = pytest.mark.gpu

LR, B1, B2, EPS, WD = 2.5e-4, 0.9, 0.999, 1e-8, 0.01
RTOL, ATOL = 2e-6, 1e-7
AMSGRAD, MAXIMIZE, DECOUPLED = 1, 2, 4
PICK = [1, 2, 5, 6, len(SIZES) + 6, len(ALL_SIZES) - 1]            # 3, 4, 4097, 8193 elements, 8193 unaligned, 250: the graph test
_values = functools.partial(adam_util._values, "variants")         # this file's numbers
DevSet = functools.partial(adam_util.DevSet, "variants")


class VmaxSet:
    """max_exp_avg_sq beside a DevSet: one view per tensor into a zeroed buffer with 8 floats of slack, at the DevSet's offset from a
    16-byte boundary, preloaded with the set's exp_avg_sq (so that the first step meets both sides of the maximum)."""

    def __init__(self, ds):
        self.bufs, self.views = [], []
        for (off, _), row in zip(ds.values, ds.views):
            n = row[3].numel()
            buf = torch.zeros(n + 8, device="cuda")
            view = buf[off:off + n]
            view.copy_(row[3])
            assert view.data_ptr() % 16 == 4 * off
            self.bufs.append((off, n, buf))
            self.views.append(view)

    def ptrs(self):
        return (ctypes.c_void_p * len(self.views))(*[v.data_ptr() for v in self.views])

    def slack_untouched(self):
        return all(bool((buf[:off] == 0).all()) and bool((buf[off + n:] == 0).all()) for off, n, buf in self.bufs)


def _flag_kw(flags):
    """(optimizer class name, keyword arguments) of a flag combination; weight_decay = WD in either form."""
    return ("AdamW" if flags & DECOUPLED else "Adam"), dict(amsgrad=bool(flags & AMSGRAD), maximize=bool(flags & MAXIMIZE), weight_decay=WD)


def _opt(ds, vs, flags, start_step=0, groups=None, **kw):
    """wsmgmap.optim.Adam / AdamW of `flags` over the set's parameters, the set's moments (and vs, the VmaxSet, with amsgrad) and
    `start_step` loaded through load_state_dict: the first step already runs on non-zero moments."""
    from wsmgmap import optim
    name, fkw = _flag_kw(flags)
    params = ds.params()
    opt = getattr(optim, name)(params if groups is None else [{"params": [params[i] for i in g]} for g in groups],
                               lr=LR, betas=(B1, B2), eps=EPS, **fkw, **kw)
    sd = opt.state_dict()
    sd["state"] = {i: {"step": torch.tensor(float(start_step)), "exp_avg": row[2], "exp_avg_sq": row[3],
                       **({"max_exp_avg_sq": vs.views[i]} if flags & AMSGRAD else {})} for i, row in enumerate(ds.views)}
    opt.load_state_dict(sd)
    if flags & AMSGRAD:
        assert all(opt.state[p]["max_exp_avg_sq"].data_ptr() == v.data_ptr() for p, v in zip(params, vs.views))
    return params, opt


def _state(params, opt, flags):
    """[(p, exp_avg, exp_avg_sq[, max_exp_avg_sq])] per parameter."""
    keys = ("exp_avg", "exp_avg_sq") + (("max_exp_avg_sq",) if flags & AMSGRAD else ())
    return [(p,) + tuple(opt.state[p][k] for k in keys) for p in params]


def _same_bits(name, a, b):
    for i, (x, y) in enumerate(zip(a, b)):
        assert len(x) == len(y)
        for what, s, t in zip(("p", "m", "v", "vmax"), x, y):
            assert torch.equal(_bits(s), _bits(t)), f"{name}: tensor {i} ({s.numel()} elements) {what} differs"


def _snapshot(state):
    return [tuple(_bits(t).clone() for t in row) for row in state]


def _float64(values, flags, start_step, max_norm=None, nan_at=None):
    """(parameters, float64 torch.optim.Adam / AdamW of `flags` with the values' moments, max_exp_avg_sq = exp_avg_sq, at start_step,
    a function that takes one step with the values' gradients)."""
    name, fkw = _flag_kw(flags)
    qs = [torch.nn.Parameter(T(p).double()) for _, (p, _, _, _) in values]
    ref = getattr(torch.optim, name)(qs, lr=LR, betas=(B1, B2), eps=EPS, **fkw)
    for q, (_, (_, _, m, v)) in zip(qs, values):
        ref.state[q] = {"step": torch.tensor(float(start_step)), "exp_avg": T(m).double().clone(), "exp_avg_sq": T(v).double().clone(),
                        **({"max_exp_avg_sq": T(v).double().clone()} if flags & AMSGRAD else {})}

    def step():
        for q, (_, (_, g, _, _)) in zip(qs, values):
            q.grad = T(g).double().clone()
        if nan_at is not None:
            qs[nan_at[0]].grad[nan_at[1]] = float("nan")
        if max_norm is not None:
            torch.nn.utils.clip_grad_norm_(qs, max_norm)
        ref.step()
    return qs, ref, step


def _within_the_adam_bar(name, qs, ref, state, flags):
    keys = ("exp_avg", "exp_avg_sq") + (("max_exp_avg_sq",) if flags & AMSGRAD else ())
    worst = 0.0
    for i, (q, row) in enumerate(zip(qs, state)):
        wants = (q.detach(),) + tuple(ref.state[q][k] for k in keys)
        for what, got, want in zip(("p", "m", "v", "vmax"), row, wants):
            got = got.detach().double().cpu().reshape(want.shape)
            worst = max(worst, float(((got - want).abs() / (ATOL / RTOL + want.abs())).max()))
            torch.testing.assert_close(got, want, rtol=RTOL, atol=ATOL, msg=lambda t: f"{name}: tensor {i} {what}: {t}")
    print(f"{name}: worst |err| / (atol/rtol + |ref|) against float64 = {worst:.3e} (bar {RTOL:.1e})")


# ----------------------------------------------------------------------------- 0. amsgrad constructs on the device; state_dict both ways
@pytest.mark.parametrize("name", ["Adam", "AdamW"])
def test_amsgrad_constructs_over_cuda_parameters_and_its_state_dict_is_torchs(name):
    """Adam(amsgrad=True) / AdamW(amsgrad=True) over CUDA parameters (over CPU parameters the construction is refused:
    tests/test_adam_variants_cpu.py): the state is lazy, gains max_exp_avg_sq at the first step, and state_dict() goes to the torch
    optimizer of the same name and back — after one more step on each side both sit inside the Adam bar of each other."""
    from wsmgmap import optim
    values = [_values()[i] for i in PICK]
    ds = DevSet(values=values)
    params = ds.params()
    opt = getattr(optim, name)(params, lr=LR, betas=(B1, B2), eps=EPS, weight_decay=WD, amsgrad=True)
    assert len(opt.state) == 0 and opt.param_groups[0]["amsgrad"] is True and opt._flags(opt.param_groups[0]) & AMSGRAD
    opt.step()
    assert all(set(opt.state[p]) == {"step", "exp_avg", "exp_avg_sq", "max_exp_avg_sq"} for p in params)
    sd = opt.state_dict()
    twins = [torch.nn.Parameter(p.detach().clone()) for p in params]
    ref = getattr(torch.optim, name)(twins, lr=0.5)
    # torch takes ours (load_state_dict adopts the tensors it is given: clones, so that each side steps its own)
    ref.load_state_dict({"state": {k: {kk: vv.clone() for kk, vv in v.items()} for k, v in sd["state"].items()}, "param_groups": sd["param_groups"]})
    assert ref.param_groups[0]["amsgrad"] is True and ref.param_groups[0]["lr"] == LR
    back = getattr(optim, name)(ds.params(), lr=0.5)
    mid = ref.state_dict()
    assert set(mid["state"][0]) == set(sd["state"][0]) and float(mid["state"][0]["step"]) == 1.0
    for t, p in zip(twins, params):
        t.grad = p.grad.clone()
    ref.step()
    opt.step()
    torch.cuda.synchronize()
    for i, (t, p) in enumerate(zip(twins, params)):
        for key in ("exp_avg", "exp_avg_sq", "max_exp_avg_sq"):
            torch.testing.assert_close(opt.state[p][key], ref.state[t][key], rtol=RTOL, atol=ATOL, msg=lambda m: f"tensor {i} {key}: {m}")
        torch.testing.assert_close(p.detach(), t.detach(), rtol=RTOL, atol=ATOL, msg=lambda m: f"tensor {i} p: {m}")
    back.load_state_dict(ref.state_dict())               # and ours takes torch's
    assert back._flags(back.param_groups[0]) == opt._flags(opt.param_groups[0]) and back.param_groups[0]["lr"] == LR
    assert {st["step"] for st in back.state.values()} == {2}
    assert all("max_exp_avg_sq" in st for st in back.state.values())


# ----------------------------------------------------------------------------- 1. each option alone, and all three: float64 torch
MODES = {"amsgrad": AMSGRAD, "maximize-l2": MAXIMIZE, "adamw": DECOUPLED, "all": AMSGRAD | MAXIMIZE | DECOUPLED}


@pytest.mark.parametrize("step", [1, 1000])
@pytest.mark.parametrize("mode", sorted(MODES))
def test_three_steps_match_float64_torch(mode, step):
    """Three consecutive steps of the by-value form from preloaded moments, the first of them step 1 or step 1000, against float64
    torch.optim.Adam(amsgrad / maximize, weight_decay = 0.01: the L2 term behind the negation) or torch.optim.AdamW: p, m, v and vmax
    inside the Adam bar after every step.  max_exp_avg_sq starts as exp_avg_sq, so the first step raises it where
    b2 v + (1 - b2) g'^2 > v and keeps it elsewhere: asserted on the float64 reference, at least 5 % of all elements each."""
    flags = MODES[mode]
    values = _values()
    ds = DevSet()
    vs = VmaxSet(ds)
    params, opt = _opt(ds, vs, flags, start_step=step - 1)
    qs, ref, ref_step = _float64(values, flags, step - 1)
    for k in range(3):
        opt.step()
        ref_step()
        torch.cuda.synchronize()
        if k == 0 and flags & AMSGRAD:
            raised = sum(int((ref.state[q]["max_exp_avg_sq"] > T(v).double()).sum()) for q, (_, (_, _, _, v)) in zip(qs, values))
            total = sum(ALL_SIZES)
            print(f"{mode}: the first step raises vmax in {raised} of {total} elements ({100.0 * raised / total:.1f} %)")
            assert raised >= 0.05 * total and total - raised >= 0.05 * total
        _within_the_adam_bar(f"{mode}, step {step + k}", qs, ref, _state(params, opt, flags), flags)
    assert float(opt.state_dict()["state"][0]["step"]) == step + 2
    assert ds.slack_untouched() and vs.slack_untouched() and ds.grads_unchanged()
    if not flags & AMSGRAD:                                            # and a step without amsgrad never touches a fifth array
        assert all(torch.equal(_bits(x), _bits(T(v).cuda())) for x, (_, (_, _, _, v)) in zip(vs.views, values))
        assert all("max_exp_avg_sq" not in opt.state[p] for p in params)


# ----------------------------------------------------------------------------- 2. flags = 0 through _ext: the old entry points' bits
def _guard_record(ds, max_norm):
    """(guard record, step count) of wsmg_grad_norm_multi over the set at step count 6 -> 7."""
    from wsmgmap import _abi
    partials = torch.empty(TOTAL_BLOCKS, device="cuda", dtype=torch.float64)
    guard = torch.zeros(4, device="cuda")
    step = torch.full((), 6.0, device="cuda")
    _abi.call("wsmg_grad_norm_multi", ds.descs(), len(ds.views), _ptr(partials), TOTAL_BLOCKS, max_norm, 1, _ptr(guard), _ptr(step), _stream())
    return guard, step


@pytest.mark.parametrize("front", ["by-value", "dev", "guarded", "hyper", "guarded-hyper"])
def test_flags_zero_through_the_ext_entry_points_is_the_old_step_bit_for_bit(front):
    """The same inputs through wsmg_adam_step_multi[_dev|_guarded|_hyper] and through its `_ext` form with flags = 0 and no
    max_exp_avg_sq array: p, m, v of all 50 tensors (both alignments, every loop, two launches) equal bit for bit.  weight_decay =
    0.01 (the L2 fma), the guarded forms clipped at half the norm (coef < 1), step 7."""
    from wsmgmap import _abi
    values = _values()
    da, db = DevSet(), DevSet()
    n = len(da.views)
    hyper = torch.tensor([LR, B1, B2, EPS, WD, 0, 0, 0], device="cuda")
    by_value = (LR, B1, B2, EPS, WD)
    for ds, ext in ((da, ""), (db, "_ext")):
        more = (None, 0) if ext else ()
        guard, step = _guard_record(ds, 0.5 * _norm64(values))
        if front == "by-value":
            _abi.call("wsmg_adam_step_multi" + ext, ds.descs(), n, *more, *by_value, 1.0 - B1 ** 7, 1.0 - B2 ** 7, _stream())
        elif front == "dev":
            _abi.call("wsmg_adam_step_multi_dev" + ext, ds.descs(), n, *more, *by_value, _ptr(step), _stream())
        elif front == "guarded":
            _abi.call("wsmg_adam_step_multi_guarded" + ext, ds.descs(), n, *more, *by_value, _ptr(step), _ptr(guard), _stream())
        else:
            _abi.call("wsmg_adam_step_multi_hyper" + ext, ds.descs(), n, *more, _ptr(hyper), _ptr(step),
                      _ptr(guard) if front == "guarded-hyper" else None, _stream())
        torch.cuda.synchronize()
        assert float(step) == 7.0 and 0.49 < float(guard[1]) < 0.51
    for i, (ra, rb) in enumerate(zip(da.views, db.views)):
        for what, k in (("p", 0), ("m", 2), ("v", 3)):
            assert torch.equal(_bits(ra[k]), _bits(rb[k])), f"{front}: tensor {i} ({ra[k].numel()} elements) {what} differs from the old entry point"
        assert not torch.equal(_bits(ra[0]), _bits(T(values[i][1][0]).cuda())), f"{front}: tensor {i} was not stepped"
    assert da.slack_untouched() and db.slack_untouched() and db.grads_unchanged()


# ----------------------------------------------------------------------------- 3. the front ends agree, for every flag combination
FRONTS = {"dev": dict(capturable=True), "guarded": dict(skip_nonfinite=True), "hyper": dict(capturable=True, hyper_on_device=True),
          "guarded-hyper": dict(skip_nonfinite=True, hyper_on_device=True)}


@pytest.mark.parametrize("flags", range(1, 8))
def test_front_ends_agree_to_the_bit(flags):
    """Three steps from preloaded moments through the by-value entry point, the device step count, the guard (skip_nonfinite alone:
    coef == 1) and the hyper record, unguarded and guarded: p, m, v (and vmax) of the five are equal bit for bit after every step —
    the decay factor of the hyper forms is formed in the kernel from the record's row, that of the others on the host.  The by-value
    step is called at the ABI with the bias corrections the kernels form from a device step count, 1 - beta^step in double of the
    float32 beta ("equal values give equal bits": wsmgmap.optim.Adam's own by-value step, held to float64 above, raises the Python
    float beta, which is another value); the other four are the optimizer's paths."""
    from wsmgmap import _abi
    dv = DevSet()
    vv = VmaxSet(dv)
    n = len(dv.views)
    sets = {}
    for name, kw in FRONTS.items():
        ds = DevSet()
        vs = VmaxSet(ds)
        sets[name] = (ds, vs) + _opt(ds, vs, flags, **kw)
    b1, b2 = float(np.float32(B1)), float(np.float32(B2))
    for k in range(3):
        _abi.call("wsmg_adam_step_multi_ext", dv.descs(), n, vv.ptrs() if flags & AMSGRAD else None, flags, LR, B1, B2, EPS, WD,
                  1.0 - b1 ** (k + 1), 1.0 - b2 ** (k + 1), _stream())
        for ds, vs, params, opt in sets.values():
            opt.step()
        torch.cuda.synchronize()
        base = [(row[0], row[2], row[3]) + ((x,) if flags & AMSGRAD else ()) for row, x in zip(dv.views, vv.views)]
        for name in FRONTS:
            _same_bits(f"flags {flags}, step {k + 1}: {name} against by-value", _state(*sets[name][2:], flags), base)
    assert dv.slack_untouched() and vv.slack_untouched() and dv.grads_unchanged()
    for name, (ds, vs, params, opt) in sets.items():
        assert ds.slack_untouched() and vs.slack_untouched() and ds.grads_unchanged(), name
        if "guarded" in name:
            assert float(opt._guard[1]) == 1.0 and opt.skipped_steps == 0 and float(opt._guard_step) == 3.0


# ----------------------------------------------------------------------------- 4. a NaN gradient: skipped behind the guard, else in vmax
NAN_AT = (len(SIZES) + 5, 4096)            # the 4 097-element tensor one float off a 16-byte boundary: its second workgroup


@pytest.mark.parametrize("hyper", [False, True], ids=["by-value", "hyper"])
def test_guarded_nan_step_writes_nothing_and_an_unguarded_one_reaches_vmax(hyper):
    flags = AMSGRAD | DECOUPLED
    values = _values()
    ds = DevSet()
    vs = VmaxSet(ds)
    params, opt = _opt(ds, vs, flags, start_step=4, skip_nonfinite=True, hyper_on_device=hyper)
    ds.views[NAN_AT[0]][1][NAN_AT[1]] = float("nan")
    before = _snapshot(_state(params, opt, flags))
    opt.step()
    torch.cuda.synchronize()
    for i, (row, b) in enumerate(zip(_state(params, opt, flags), before)):
        assert all(torch.equal(_bits(t), x) for t, x in zip(row, b)), f"tensor {i} was written by a skipped step"
    assert opt.skipped_steps == 1 and float(opt._guard_step) == 4.0 and np.isnan(float(opt.grad_norm))
    assert float(opt.state_dict()["state"][0]["step"]) == 4.0
    assert ds.slack_untouched() and vs.slack_untouched()
    # unguarded: the NaN reaches m, v, vmax and p of that element, as torch.maximum lets it, and of no other
    du = DevSet()
    vu = VmaxSet(du)
    pu, ou = _opt(du, vu, flags, start_step=4, capturable=hyper, hyper_on_device=hyper)
    du.views[NAN_AT[0]][1][NAN_AT[1]] = float("nan")
    ou.step()
    torch.cuda.synchronize()
    qs, ref, ref_step = _float64(values, flags, 4, nan_at=NAN_AT)
    ref_step()
    assert bool(ref.state[qs[NAN_AT[0]]]["max_exp_avg_sq"][NAN_AT[1]].isnan())
    for i, (row, q) in enumerate(zip(_state(pu, ou, flags), qs)):
        wants = (q.detach(), ref.state[q]["exp_avg"], ref.state[q]["exp_avg_sq"], ref.state[q]["max_exp_avg_sq"])
        for what, got, want in zip(("p", "m", "v", "vmax"), row, wants):
            assert torch.equal(got.detach().isnan().cpu(), want.isnan()), f"tensor {i} {what}: NaN where torch has none, or the reverse"
            assert int(want.isnan().sum()) == (1 if i == NAN_AT[0] else 0)
    assert du.slack_untouched() and vu.slack_untouched()


# ----------------------------------------------------------------------------- 5. a clipped step with maximize
def test_clipped_step_with_maximize_uses_the_norm_and_coefficient_of_the_gradient():
    """max_grad_norm = half the norm with and without maximize: the guard record {norm, coef, skip, skipped} is the same, bit for
    bit; the step sits inside the Adam bar of float64 clip_grad_norm_ + torch.optim.Adam(maximize=True); and with weight_decay = 0
    and zero moments a maximized step's exp_avg is the plain step's negated and its exp_avg_sq the plain step's (the negation is exact)."""
    values = _values()
    norm = _norm64(values)
    da, db = DevSet(), DevSet()
    pa, oa = _opt(da, None, MAXIMIZE, max_grad_norm=0.5 * norm, skip_nonfinite=True)
    pb, ob = _opt(db, None, 0, max_grad_norm=0.5 * norm, skip_nonfinite=True)
    oa.step()
    ob.step()
    torch.cuda.synchronize()
    assert torch.equal(_bits(oa._guard), _bits(ob._guard)), f"{oa._guard.tolist()} != {ob._guard.tolist()}"
    assert abs(float(oa.grad_norm) - norm) <= 2e-7 * norm and 0.49 < float(oa._guard[1]) < 0.51 and oa.skipped_steps == 0
    qs, ref, ref_step = _float64(values, MAXIMIZE, 0, max_norm=0.5 * norm)
    ref_step()
    _within_the_adam_bar("maximize, clipped", qs, ref, _state(pa, oa, MAXIMIZE), MAXIMIZE)
    assert da.grads_unchanged() and da.slack_untouched()
    # the exact mirror: weight_decay = 0 and zero moments, so that m and the step change sign and nothing else
    dc, dd = DevSet(fresh=True), DevSet(fresh=True)
    from wsmgmap import optim
    pc, pd = dc.params(), dd.params()
    oc = optim.Adam(pc, lr=LR, eps=EPS, maximize=True, max_grad_norm=0.5 * norm)
    od = optim.Adam(pd, lr=LR, eps=EPS, max_grad_norm=0.5 * norm)
    oc.step()
    od.step()
    torch.cuda.synchronize()
    for i, (c, d) in enumerate(zip(pc, pd)):
        assert torch.equal(_bits(oc.state[c]["exp_avg"]), _bits(-od.state[d]["exp_avg"])), f"tensor {i}: m is not the plain step's negated"
        assert torch.equal(_bits(oc.state[c]["exp_avg_sq"]), _bits(od.state[d]["exp_avg_sq"])), f"tensor {i}: v"
    assert torch.equal(_bits(oc._guard), _bits(od._guard))


# ----------------------------------------------------------------------------- 6. the decoupled decay follows the hyper record in a graph
def test_decoupled_decay_under_replay_follows_lr_and_weight_decay():
    """AdamW(amsgrad=True, capturable=True, hyper_on_device=True) over six small tensors in two groups: one eager step, step() captured
    with torch.cuda.graph, then lr and weight_decay edited in `param_groups` (each group its own values), sync_hyper(), replay — the
    kernel forms 1 - lr wd from the record's row: bit-identical to an eager by-value twin stepped with the new values."""
    flags = AMSGRAD | DECOUPLED
    values = [_values()[i] for i in PICK]
    ds, twin = DevSet(values=values), DevSet(values=values)
    vs, vt = VmaxSet(ds), VmaxSet(twin)
    groups = [[0, 1, 2, 3], [4, 5]]
    params, opt = _opt(ds, vs, flags, groups=groups, capturable=True, hyper_on_device=True)
    tparams, topt = _opt(twin, vt, flags, groups=groups, capturable=True)
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
    _same_bits("after the eager step and the capture", _state(params, opt, flags), _state(tparams, topt, flags))
    for k, (lr, wd) in enumerate(((1e-3, 0.1), (5e-4, 0.0), (2e-3, 0.25))):
        for o in (opt, topt):
            for j, g in enumerate(o.param_groups):
                g["lr"], g["weight_decay"] = lr * (1 + j), wd + 0.05 * j
        before = _snapshot(_state(params, opt, flags))
        assert opt.sync_hyper() is True
        graph.replay()
        opt.note_replayed_steps(1)
        topt.step()
        torch.cuda.synchronize()
        now = _state(params, opt, flags)
        _same_bits(f"replay {k + 1} (lr {lr}, weight_decay {wd})", now, _state(tparams, topt, flags))
        assert all(not torch.equal(_bits(row[0]), b[0]) for row, b in zip(now, before)), "a replay left a parameter alone"
    assert float(next(iter(opt._step_dev.values()))) == 4.0 and float(opt.state_dict()["state"][0]["step"]) == 4.0
    assert ds.slack_untouched() and vs.slack_untouched() and ds.grads_unchanged()


# ----------------------------------------------------------------------------- 8. argument checks, before any launch
def test_rejected_arguments_launch_nothing():
    from wsmgmap import _abi
    L = _abi.lib()
    ds = DevSet()
    vs = VmaxSet(ds)
    descs, n = ds.descs(), len(ds.views)
    step = torch.full((2,), 5.0, device="cuda")
    guard = torch.tensor([1.0, 1.0, 0.0, 0.0], device="cuda")
    record = torch.tensor([LR, B1, B2, EPS, WD, 0, 0, 0], device="cuda")
    snap = [buf.clone() for _, _, buf in ds.bufs] + [buf.clone() for _, _, buf in vs.bufs]
    torch.cuda.synchronize()
    by_value = (LR, B1, B2, EPS, WD)

    def calls(vmax, flags, descs=descs):
        return [L.wsmg_adam_step_multi_ext(descs, n, vmax, flags, *by_value, 0.5, 0.5, _stream()),
                L.wsmg_adam_step_multi_dev_ext(descs, n, vmax, flags, *by_value, _ptr(step), _stream()),
                L.wsmg_adam_step_multi_guarded_ext(descs, n, vmax, flags, *by_value, _ptr(step), _ptr(guard), _stream()),
                L.wsmg_adam_step_multi_hyper_ext(descs, n, vmax, flags, _ptr(record), _ptr(step), None, _stream()),
                L.wsmg_adam_step_multi_hyper_ext(descs, n, vmax, flags, _ptr(record), _ptr(step), _ptr(guard), _stream())]
    assert calls(None, AMSGRAD) == [-1] * 5                                     # the flag without the array
    assert calls(None, AMSGRAD | MAXIMIZE | DECOUPLED) == [-1] * 5
    for bad_flags in (8, 16 | AMSGRAD, -1, 1 << 30):                             # a bit outside the three
        assert calls(vs.ptrs(), bad_flags) == [-1] * 5, bad_flags
    hole = vs.ptrs()
    hole[n - 1] = None                               # the LAST tensor (second launch of the table): nothing before it may run
    assert calls(hole, AMSGRAD) == [-1] * 5
    odd = vs.ptrs()
    odd[n - 1] = odd[n - 1] + 2                      # not a multiple of 4
    assert calls(odd, AMSGRAD) == [-1] * 5
    bad = ds.descs()
    bad[n - 1].exp_avg = None                        # and the checks of the entry points without `_ext` stay
    assert calls(vs.ptrs(), AMSGRAD, descs=bad) == [-1] * 5
    assert L.wsmg_adam_step_multi_ext(descs, n, vs.ptrs(), AMSGRAD, *by_value, 0.0, 0.5, _stream()) == -1
    assert L.wsmg_adam_step_multi_dev_ext(descs, n, vs.ptrs(), AMSGRAD, *by_value, None, _stream()) == -1
    assert L.wsmg_adam_step_multi_guarded_ext(descs, n, vs.ptrs(), AMSGRAD, *by_value, _ptr(step), None, _stream()) == -1
    assert L.wsmg_adam_step_multi_hyper_ext(descs, n, vs.ptrs(), AMSGRAD, None, _ptr(step), None, _stream()) == -1
    assert L.wsmg_adam_step_multi_hyper_ext(descs, n, vs.ptrs(), AMSGRAD, _ptr(record, 2), _ptr(step), None, _stream()) == -1
    assert L.wsmg_adam_step_multi_ext(descs, -1, vs.ptrs(), AMSGRAD, *by_value, 0.5, 0.5, _stream()) == -1
    torch.cuda.synchronize()
    assert all(torch.equal(_bits(buf), _bits(s)) for (_, _, buf), s in zip(ds.bufs + vs.bufs, snap)), "a rejected call wrote something"
    assert step.tolist() == [5.0, 5.0]
    # a hole beside an EMPTY descriptor is no error, and without the flag the array is not read at all
    empty = ds.descs()
    empty[n - 1].n = 0
    assert L.wsmg_adam_step_multi_dev_ext(empty, n, hole, AMSGRAD, *by_value, _ptr(step), _stream()) == 0
    torch.cuda.synchronize()
    for i in range(n - 1):                           # vmax is the maximum of what it was and the new v, exactly
        was = snap[4 * n + i][vs.bufs[i][0]:vs.bufs[i][0] + vs.bufs[i][1]]
        assert torch.equal(_bits(vs.views[i]), _bits(torch.maximum(was, ds.views[i][3]))), f"tensor {i}: vmax"
    assert L.wsmg_adam_step_multi_dev_ext(descs, n, None, MAXIMIZE | DECOUPLED, *by_value, _ptr(step), _stream()) == 0
    torch.cuda.synchronize()
    changed = [not torch.equal(_bits(buf), _bits(s)) for (_, _, buf), s in zip(ds.bufs + vs.bufs, snap)]
    assert all(changed[4 * i + k] for i in range(n) for k in (0, 2, 3)) and not any(changed[4 * i + 1] for i in range(n))
    assert any(changed[4 * n:-1]) and not changed[-1], "vmax of the emptied tensor was written"
    assert ds.slack_untouched() and vs.slack_untouched() and record.tolist()[5:] == [0.0] * 3


# ----------------------------------------------------------------------------- 9. the policy's update under GraphedUpdate
class _Box:
    shape = (2,)


def _loss_fn(pred, aux, o, w):
    return (pred ** 2).mean() + aux


def test_graphed_policy_updates_equal_the_eager_step_bit_for_bit():
    """T = 4 x N = 2, float32 mode: two updates under GraphedUpdate (eager_calls = 1: the second is the captured graph's replay)
    with AdamW(amsgrad=True, max_grad_norm=..., skip_nonfinite=True).  The eager run it is held to is an eager optimizer of the same
    construction over copies of the parameters, stepped with the gradients of the graphed update: parameters, exp_avg, exp_avg_sq,
    max_exp_avg_sq, the guard record and the device step count equal bit for bit after each update.  (A second POLICY run eagerly
    cannot be the yardstick of a bit-wise comparison: the backward pass accumulates weight gradients with float atomics, and two
    eager twins already differ by 2e-4 after four updates — tests/test_gpu_round2.py, test_graphed_update_matches_eager_updates.)
    The first update is not clipped (coef = 1); before the capture max_grad_norm is set to half the measured norm, so the replayed
    step is (coef < 1)."""
    from wsmgmap import ops, optim
    from wsmgmap.common.aux_losses import AuxLosses
    from wsmgmap.config import default_model_config
    from wsmgmap.graph import GraphedUpdate
    from wsmgmap.models.policy import BasePolicy
    obs_np, prev, masks, weights = cases.update_inputs(4, 2, n_tok=(80, 37), tag="graph")
    obs = {k: T(v).cuda() for k, v in obs_np.items()}
    prev, masks, weights = T(prev).cuda(), T(masks).cuda(), T(weights).cuda()
    pol = BasePolicy(None, _Box(), default_model_config(num_proc=2, compute_dtype="f32"))
    pol.load_state_dict(state_dict_values(), strict=True)
    pol.net.instruction_encoder.embedding_layer.weight.requires_grad_(False)
    pol = pol.cuda()
    pol.train(); pol.net.depth_encoder.eval(); pol.net.rgb_encoder.eval()
    AuxLosses.activate()
    kw = dict(lr=1e-5, weight_decay=0.05, amsgrad=True, max_grad_norm=1e30, skip_nonfinite=True)
    opt = optim.AdamW(pol.parameters(), **kw)
    every = list(pol.parameters())
    twins = [torch.nn.Parameter(p.detach().clone()) for p in every]
    topt = optim.AdamW(twins, **kw)
    gu = GraphedUpdate(pol, opt, _loss_fn, eager_calls=1)
    coefs = []
    for k in range(2):
        loss = float(gu(obs, torch.zeros(2, 2, 512, device="cuda"), prev, masks, weights))
        torch.cuda.synchronize()
        assert np.isfinite(loss)
        live = [i for i, p in enumerate(every) if p.grad is not None]
        assert len(live) > 96                                             # three launches of the table
        for i, t in enumerate(twins):
            t.grad = every[i].grad.clone() if i in live else None
        topt.step()
        torch.cuda.synchronize()
        for i in live:
            a, b = opt.state[every[i]], topt.state[twins[i]]
            assert torch.equal(_bits(every[i]), _bits(twins[i])), f"update {k + 1}: parameter {i} differs from the eager step"
            for key in ("exp_avg", "exp_avg_sq", "max_exp_avg_sq"):
                assert torch.equal(_bits(a[key]), _bits(b[key])), f"update {k + 1}: {key} of parameter {i} differs from the eager step"
        assert torch.equal(_bits(opt._guard), _bits(topt._guard)) and float(opt._guard_step) == float(topt._guard_step) == k + 1
        coefs.append(float(opt._guard[1]))
        if k == 0:
            norm = float(opt.grad_norm)
            assert np.isfinite(norm) and norm > 0
            opt.max_grad_norm = topt.max_grad_norm = 0.5 * norm
    print(f"clip coefficients of the two updates: {coefs}")
    assert len(gu._graphs) == 1 and gu.calls == 2 and coefs[0] == 1.0 and coefs[1] < 1.0 and opt.skipped_steps == 0
    assert {float(st["step"]) for st in opt.state_dict()["state"].values()} == {2.0}
    AuxLosses.deactivate()
    ops.check_rnn_status()
