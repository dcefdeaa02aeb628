"""GPU: the guarded Adam step (csrc/wsmg_optim.hip: grad_sumsq_multi_kernel, grad_guard_finalize_kernel,
adam_multi_guarded_kernel; wsmgmap.optim.Adam(max_grad_norm=..., skip_nonfinite=...), wsmgmap.optim.global_grad_norm) against
float64 torch: `torch.linalg.vector_norm`, `torch.nn.utils.clip_grad_norm_` + `torch.optim.Adam`.

Tensors as test_adam_kernel_paths_match_float64_torch_adam lays them out: the sizes around the 4-element vector and the 4 096-element
workgroup, once 16-byte aligned and once as views one float off, then ragged small sizes up to 50 tensors (the table of 48 spills
into a second launch, so the norm's partials span launches); values from oracle.detfill.

THE BAR of every stepped comparison is the existing Adam bar, rtol 2e-6 / atol 1e-7 (one float32 rounding of p is 6e-8 relative).
The guard adds to a plain step: the float32 rounding of the norm (6e-8), of norm + 1e-6 and of the quotient (6e-8 each), and of
g * coef (6e-8) — under 3e-7 relative on g, 6e-7 on its square, inside the bar; it was not widened."""
import functools

import numpy as np
import pytest
import torch

import adam_util
from adam_util import ALL_SIZES, SIZES, TOTAL_BLOCKS, _bits, _norm64, _ptr, _stream
from oracle import cases
from util import T, state_dict_values

pytestmark = pytest.mark.gpu

LR, B1, B2, EPS = 2.5e-4, 0.9, 0.999, 1e-8
RTOL, ATOL = 2e-6, 1e-7
_values = functools.partial(adam_util._values, "guard")            # this file's numbers
DevSet = functools.partial(adam_util.DevSet, "guard")


def _oracle(values, fresh, start_step, n_steps, wd=0.0, max_norm=None):
    """float64 clip_grad_norm_ + torch.optim.Adam, n_steps with the same gradients: (parameters, optimizer)."""
    ps = [torch.nn.Parameter(T(p).double()) for _, (p, _, _, _) in values]
    opt = torch.optim.Adam(ps, lr=LR, betas=(B1, B2), eps=EPS, weight_decay=wd)
    if not fresh:
        for q, (_, (_, _, m, v)) in zip(ps, values):
            opt.state[q] = {"step": torch.tensor(float(start_step)), "exp_avg": T(m).double().clone(), "exp_avg_sq": T(v).double().clone()}
    for _ in range(n_steps):
        for q, (_, (_, g, _, _)) in zip(ps, values):
            q.grad = T(g).double().clone()
        if max_norm is not None:
            torch.nn.utils.clip_grad_norm_(ps, max_norm)
        opt.step()
    return ps, opt


def _check(name, got_p, got_m, got_v, ps, opt):
    worst = 0.0
    for i, q in enumerate(ps):
        s = opt.state[q]
        for what, got, want in (("p", got_p[i], q.detach()), ("m", got_m[i], s["exp_avg"]), ("v", got_v[i], s["exp_avg_sq"])):
            got = got.detach().double().cpu().reshape(want.shape)
            err = float(((got - want).abs() / (ATOL / RTOL + want.abs())).max()) if want.numel() else 0.0
            worst = max(worst, err)
            torch.testing.assert_close(got, want, rtol=RTOL, atol=ATOL, msg=lambda t: f"{name}: tensor {i} {what}: {t}")
    print(f"{name}: worst |err| / (atol/rtol + |ref|) = {worst:.3e} (bar {RTOL:.1e})")


def _adam(ds, start_step=0, preload=False, **kw):
    """wsmgmap.optim.Adam over the set's parameters; start_step > 0 or preload: the set's moments and that step count, through
    load_state_dict (otherwise the first step creates zero moments)."""
    from wsmgmap import optim
    params = ds.params()
    opt = optim.Adam(params, lr=LR, betas=(B1, B2), eps=EPS, **kw)
    if start_step or preload:
        sd = opt.state_dict()
        sd["state"] = {i: {"step": torch.tensor(float(start_step)), "exp_avg": row[2], "exp_avg_sq": row[3]}
                       for i, row in enumerate(ds.views)}
        opt.load_state_dict(sd)
    return params, opt


def _moments(params, opt):
    return [opt.state[p]["exp_avg"] for p in params], [opt.state[p]["exp_avg_sq"] for p in params]


# ----------------------------------------------------------------------------- 1. the norm
@pytest.mark.parametrize("gscale", [None, 1e30], ids=["unit", "1e30"])
def test_global_grad_norm_matches_float64_and_is_deterministic(gscale):
    """rtol 2e-7: float64 accumulation, one float32 rounding of the result (6e-8).  At 1e30 a float32 accumulator overflows
    (squares of 1e58) while the float32 norm itself is finite."""
    from wsmgmap import _abi, optim
    ds = DevSet(fresh=True, gscale=gscale)
    params = ds.params()
    want = float(torch.linalg.vector_norm(torch.cat([row[1].cpu().double() for row in ds.views])))
    a = optim.global_grad_norm(params)
    b = optim.global_grad_norm(params)
    torch.cuda.synchronize()
    assert a.dim() == 0 and a.dtype == torch.float32 and a.is_cuda
    print(f"norm {float(a):.9e}, float64 {want:.9e}, rel err {abs(float(a) - want) / want:.3e}")
    assert np.isfinite(float(a)) and abs(float(a) - want) <= 2e-7 * want
    if gscale is not None:
        assert want * want > float(np.finfo(np.float32).max)            # what a float32 sum of squares would have to hold
    assert torch.equal(_bits(a), _bits(b))
    assert ds.slack_untouched()
    # the entry point itself: the partials' used prefix, the four-float record and the step count are all it writes
    partials = torch.full((TOTAL_BLOCKS + 5,), -7.0, device="cuda", dtype=torch.float64)
    guard = torch.full((12,), -7.0, device="cuda")
    guard[4:8] = 0.0
    step = torch.full((3,), 41.0, device="cuda")
    _abi.call("wsmg_grad_norm_multi", ds.descs(), len(ds.views), _ptr(partials), TOTAL_BLOCKS, 0.0, 1, _ptr(guard[4:]), _ptr(step[1:]),
              _stream())
    torch.cuda.synchronize()
    assert bool((partials[TOTAL_BLOCKS:] == -7.0).all()) and bool((partials[:TOTAL_BLOCKS] >= 0).all())
    assert bool((guard[:4] == -7.0).all()) and bool((guard[8:] == -7.0).all())
    assert torch.equal(_bits(guard[4]), _bits(a)) and guard[5:8].tolist() == [1.0, 0.0, 0.0]
    assert step.tolist() == [41.0, 42.0, 41.0]
    assert ds.slack_untouched() and (gscale is not None or ds.grads_unchanged())


# ----------------------------------------------------------------------------- 2. clip + step
@pytest.mark.parametrize("step", [1, 1000])
@pytest.mark.parametrize("mode", ["below", "above", "below-wd"])
def test_clipped_step_matches_float64_clip_grad_norm_and_adam(mode, step):
    """max_grad_norm half the norm (coef < 1, also with weight_decay = 0.01) and twice it (coef = 1: then bit-identical to the unguarded
    wsmg_adam_step_multi_dev on the same inputs), from zero moments at step 1 and with moments at step 1000.  p.grad is not
    modified: the clip is applied where the Adam kernel reads the gradient."""
    from wsmgmap import _abi
    wd = 0.01 if mode == "below-wd" else 0.0
    fresh = step == 1
    values = _values()
    norm = _norm64(values)
    max_norm = norm * (2.0 if mode == "above" else 0.5)
    ps, ref = _oracle(values, fresh, step - 1, 1, wd=wd, max_norm=max_norm)
    ds = DevSet(fresh)
    params, opt = _adam(ds, start_step=step - 1, weight_decay=wd, max_grad_norm=max_norm, skip_nonfinite=(step == 1))
    opt.step()
    torch.cuda.synchronize()
    assert abs(float(opt.grad_norm) - norm) <= 2e-7 * norm
    ms, vs = _moments(params, opt)
    _check(f"clip {mode} step {step}", [p for p in params], ms, vs, ps, ref)
    assert ds.grads_unchanged() and ds.slack_untouched()
    assert opt.skipped_steps == 0 and float(opt.state_dict()["state"][0]["step"]) == step
    if mode == "above":
        plain = DevSet(fresh)
        sd = torch.full((), float(step), device="cuda", dtype=torch.float32)
        _abi.call("wsmg_adam_step_multi_dev", plain.descs(), len(plain.views), LR, B1, B2, EPS, wd, _ptr(sd), _stream())
        torch.cuda.synchronize()
        for i, row in enumerate(plain.views):
            assert torch.equal(_bits(row[0]), _bits(params[i])), f"tensor {i}: p differs from the unguarded step"
            assert torch.equal(_bits(row[2]), _bits(ms[i])) and torch.equal(_bits(row[3]), _bits(vs[i])), f"tensor {i}: moments differ"


# ----------------------------------------------------------------------------- 3. skip
BAD = [("nan-last-of-last", len(ALL_SIZES) - 1, ALL_SIZES[-1] - 1, float("nan")),      # scalar tail, second launch
       ("inf-first-of-unaligned", len(SIZES) + 3, 0, float("inf")),
       ("neginf-middle-of-8193", SIZES.index(8193), 4096, -float("inf"))]


def test_nonfinite_gradients_skip_the_whole_step():
    """One good step, then a NaN / +Inf / -Inf in turn: nothing of any tensor is written, skipped_steps counts, the norm reads
    non-finite, the device step count stays; the next good step is the float64 oracle's SECOND step."""
    assert ALL_SIZES[-1] % 4 != 0
    values = _values()
    ds = DevSet(fresh=True)
    params, opt = _adam(ds, skip_nonfinite=True)
    opt.step()
    attempted = 1
    for k, (name, ti, ei, bad) in enumerate(BAD):
        g = ds.views[ti][1]
        assert ds.views[ti][0].data_ptr() % 16 == (4 if name.startswith("inf") else 0)
        good = g[ei].clone()
        g[ei] = bad
        ms, vs = _moments(params, opt)
        before = [(_bits(p).clone(), _bits(m).clone(), _bits(v).clone()) for p, m, v in zip(params, ms, vs)]
        step_before = float(opt._guard_step)
        opt.step()
        attempted += 1
        torch.cuda.synchronize()
        for i, (p, m, v) in enumerate(zip(params, ms, vs)):
            assert torch.equal(_bits(p), before[i][0]) and torch.equal(_bits(m), before[i][1]) and torch.equal(_bits(v), before[i][2]), \
                f"{name}: tensor {i} was written by a skipped step"
        assert opt.skipped_steps == k + 1 and not np.isfinite(float(opt.grad_norm)), name
        assert float(opt._guard_step) == step_before == 1.0, name
        assert float(opt.state_dict()["state"][0]["step"]) == attempted - (k + 1) == 1.0
        g[ei] = good
    opt.step()
    attempted += 1
    torch.cuda.synchronize()
    ps, ref = _oracle(values, True, 0, 2)
    ms, vs = _moments(params, opt)
    _check("good step after three skipped", params, ms, vs, ps, ref)
    sd = opt.state_dict()
    assert all(float(sd["state"][i]["step"]) == attempted - 3 == 2.0 for i in range(len(params)))
    assert opt.skipped_steps == 3 and np.isfinite(float(opt.grad_norm)) and ds.slack_untouched() and ds.grads_unchanged()


def test_clipping_without_skip_lets_a_nan_through_as_torch_does():
    """skip_nonfinite=False, max_grad_norm=1.0: the NaN norm makes clip_grad_norm_'s coefficient NaN and with it every gradient, so
    every parameter — the two options are independent."""
    values = _values()
    ds = DevSet(fresh=True)
    params, opt = _adam(ds, max_grad_norm=1.0)
    ds.views[-1][1][-1] = float("nan")
    opt.step()
    torch.cuda.synchronize()
    ps = [torch.nn.Parameter(T(p).double()) for _, (p, _, _, _) in values]
    for q, (_, (_, g, _, _)) in zip(ps, values):
        q.grad = T(g).double().clone()
    ps[-1].grad[-1] = float("nan")
    torch.nn.utils.clip_grad_norm_(ps, 1.0)
    torch.optim.Adam(ps, lr=LR, betas=(B1, B2), eps=EPS).step()
    assert all(bool(q.isnan().all()) for q in ps)
    for i, (p, q) in enumerate(zip(params, ps)):
        assert torch.equal(p.isnan().cpu(), q.isnan()), f"tensor {i}"
    assert opt.skipped_steps == 0 and np.isnan(float(opt.grad_norm))


# ----------------------------------------------------------------------------- 4. inside a HIP graph
def test_guarded_step_replays_in_a_graph_and_skips_there():
    """opt.step() alone, captured (a linear chain of norm launches, finalize, guarded Adam launches) over six small tensors with
    static gradient buffers; replayed with finite gradients, with a NaN, with the finite gradients again: two steps taken."""
    from wsmgmap import optim
    pick = [1, 2, 5, 6, len(SIZES) + 6, len(ALL_SIZES) - 1]            # 3, 4, 4097, 8193 elements, 8193 unaligned, 250
    values = [_values()[i] for i in pick]
    norm = _norm64(values)
    ps, ref = _oracle(values, True, 0, 2, max_norm=0.5 * norm)
    ds, twin = DevSet(True, values=values), DevSet(True, values=values)
    params, opt = _adam(ds, preload=True, max_grad_norm=0.5 * norm, skip_nonfinite=True)    # moments exist before the capture
    _, warm = _adam(twin, max_grad_norm=0.5 * norm, skip_nonfinite=True)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        warm.step()                        # the kernels' first launches happen outside the capture, on another optimizer
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    from wsmgmap import _abi
    _, lazy = _adam(twin, skip_nonfinite=True)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        with pytest.raises(_abi.WsmgError):    # zero fills of first-step moments would be replayed: refused under capture
            lazy.step()
        opt.step()
    opt.note_replayed_steps(-1)            # capture ran the host bookkeeping once without executing anything
    torch.cuda.synchronize()
    assert all(torch.equal(_bits(p), _bits(T(v[1][0]).cuda())) for p, v in zip(params, values)), "capture executed the step"
    g0 = ds.views[3][1]
    good = g0.clone()
    for k in range(3):
        if k == 1:
            g0[4096] = float("nan")
        if k == 2:
            g0.copy_(good)
        graph.replay()
        opt.note_replayed_steps(1)
    torch.cuda.synchronize()
    ms, vs = _moments(params, opt)
    _check("graph, two of three replays stepped", params, ms, vs, ps, ref)
    assert opt.skipped_steps == 1 and float(opt._guard_step) == 2.0
    assert float(opt.state_dict()["state"][0]["step"]) == 2.0 and np.isfinite(float(opt.grad_norm))


# ----------------------------------------------------------------------------- 5. the policy's update
class _Box:
    shape = (2,)


def test_policy_update_skips_a_poisoned_gradient_and_clips_a_clean_one():
    """A T = 4 x N = 2 float32 update: a NaN in one element of one live gradient and skip_nonfinite: every parameter bitwise
    unchanged; a second, clean update steps, clipped to half its measured norm, as float64 clip_grad_norm_ + Adam do over the
    same live tensors (THE BAR above)."""
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

    def backward():
        for p in policy.parameters():
            p.grad = None
        AuxLosses.activate(); AuxLosses.clear()
        pred, aux = policy(dict(obs), torch.zeros(2, 2, 512, device="cuda"), prev, masks, weights)
        ((pred ** 2).mean() + aux).backward()
        AuxLosses.deactivate()
    backward()
    live = [p for p in policy.parameters() if p.grad is not None]
    norm = float(optim.global_grad_norm(policy.parameters()))
    want = float(torch.linalg.vector_norm(torch.cat([p.grad.double().flatten() for p in live])))
    print(f"live tensors {len(live)}, floats {sum(p.numel() for p in live)}, norm {norm:.6e} (float64 {want:.6e})")
    assert len(live) > 96 and abs(norm - want) <= 2e-7 * want          # three launches of the table
    opt = optim.Adam(policy.parameters(), lr=LR, max_grad_norm=0.5 * norm, skip_nonfinite=True)
    before = [_bits(p).clone() for p in policy.parameters()]
    live[len(live) // 2].grad.view(-1)[7 % live[len(live) // 2].numel()] = float("nan")
    opt.step()
    torch.cuda.synchronize()
    assert all(torch.equal(_bits(p), b) for p, b in zip(policy.parameters(), before)), "a skipped step wrote a parameter"
    assert opt.skipped_steps == 1
    backward()
    live2 = [p for p in policy.parameters() if p.grad is not None]
    assert [id(p) for p in live2] == [id(p) for p in live]
    twins = [torch.nn.Parameter(p.detach().double().cpu()) for p in live]
    for t, p in zip(twins, live):
        t.grad = p.grad.double().cpu()
    grads = [_bits(p.grad).clone() for p in live]
    opt.step()
    torch.cuda.synchronize()
    torch.nn.utils.clip_grad_norm_(twins, 0.5 * norm)
    torch.optim.Adam(twins, lr=LR).step()
    assert opt.skipped_steps == 1 and {float(st["step"]) for st in opt.state_dict()["state"].values()} == {1.0}
    for i, (t, p) in enumerate(zip(twins, live)):
        torch.testing.assert_close(p.detach().double().cpu(), t.detach(), rtol=RTOL, atol=ATOL, msg=lambda s: f"live tensor {i}: {s}")
        assert torch.equal(_bits(p.grad), grads[i]), "p.grad was modified"
    assert any(not torch.equal(_bits(p), b) for p, b in zip(policy.parameters(), before))


# ----------------------------------------------------------------------------- 6. argument checks, before any launch
def test_rejected_arguments_launch_nothing():
    from wsmgmap import _abi
    L = _abi.lib()
    ds = DevSet(fresh=True)
    descs, n = ds.descs(), len(ds.views)
    partials = torch.full((TOTAL_BLOCKS + 4,), -7.0, device="cuda", dtype=torch.float64)
    guard = torch.full((4,), -7.0, device="cuda")
    step = torch.full((), 5.0, device="cuda")
    snap = [buf.clone() for _, _, buf in ds.bufs]
    torch.cuda.synchronize()
    args = dict(descs=descs, n=n, partials=_ptr(partials), cap=TOTAL_BLOCKS, max_norm=1.0, skip=1, guard=_ptr(guard), step=_ptr(step))

    def norm(**kw):
        a = {**args, **kw}
        return L.wsmg_grad_norm_multi(a["descs"], a["n"], a["partials"], a["cap"], a["max_norm"], a["skip"], a["guard"], a["step"], _stream())
    assert norm(cap=TOTAL_BLOCKS - 1) == -2                  # WSMG_ENOMEM: one partial short
    assert norm(guard=None) == -1                            # WSMG_EINVAL
    assert norm(partials=None) == -1 and norm(n=-1) == -1 and norm(cap=-1) == -1 and norm(descs=None) == -1
    assert norm(max_norm=-1.0) == -1 and norm(max_norm=float("nan")) == -1
    hp = (LR, B1, B2, EPS, 0.0)
    assert L.wsmg_adam_step_multi_guarded(descs, n, *hp, _ptr(step), None, _stream()) == -1
    assert L.wsmg_adam_step_multi_guarded(descs, n, *hp, None, _ptr(guard), _stream()) == -1
    torch.cuda.synchronize()
    assert bool((partials == -7.0).all()) and bool((guard == -7.0).all()) and float(step) == 5.0
    assert all(torch.equal(_bits(buf), _bits(s)) for (_, _, buf), s in zip(ds.bufs, snap))
    assert norm() == 0                                       # and the same arguments, complete, run
    torch.cuda.synchronize()
    assert float(step) == 6.0 and bool((partials[TOTAL_BLOCKS:] == -7.0).all()) and float(guard[2]) == 0.0
