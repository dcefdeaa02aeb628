"""GPU: the single-query attention kernels of csrc/wsmg_attn.hip at their token-count and mask edges.  Inputs, float64 references,
elementwise derived bars and the (kind, mask) table are those of tests/attn_cases.py (checked on the CPU by
tests/test_attn_cases_cpu.py, whose header maps every tail guard of the kernels to the fault model and the named case that catch its
removal).  Every comparison prints the measured error beside its bar; the module prints the worst ratio per form and output at its end.

Section, kernels it pins, and the test that held them before:
1. through ops      attn_fwd_kernel / attn_bwd_kernel <f32 | bf16> (ops.attention, distinct k and v) and attn_same_fwd_kernel /
                    attn_same_bwd_kernel <f32 | bf16, 16> (ops.attention_folded) at 1 ... 2560 tokens — test_gpu_kernels.py::
                    test_attention_fwd_bwd / test_attention_map_sized / test_attention_bf16 (I = 160, 576, generic) and
                    test_attention_with_folded_key_projection (I = 37; bf16 at 2e-2 of the tensor maximum)
2. direct calls     the same kernels through wsmg_attn_fwd[_bf16] / wsmg_attn_bwd[_bf16] into NaN-guarded buffers, with dattn = NULL,
                    with dout = 0 and with both; two launches bit-identical — nothing entered the dattn == NULL branch on purpose
3. the two forms    one tensor (k == v, dk == dv: the dispatch is by pointer equality) against two tensors of equal values; two tensors
                    with ONE gradient buffer (k != v, dk == dv: the generic backward's own one-tensor branch)
4. shared sets      attn_fwd_kernel / attn_bwd_kernel with a row index (ops.attention_shared, wsmg_attn_shared_*), dlogits itself,
                    masks that are no prefix, unused sets — test_gpu_kernels.py::test_attention_over_shared_sets (prefix masks)
5. refusals         I = 2561, I = 0, C != 256, a NULL row index: WSMG_EINVAL, nothing written

The largest tensor is 3 x 2560 x 256 float32."""
import ctypes

import numpy as np
import pytest
import torch

import attn_cases as ac

pytestmark = pytest.mark.gpu

EINVAL = -1
GUARD = 64                # elements of guard in front of and behind a direct call's output (keeps 16-byte alignment)
DTYPES = [torch.float32, torch.bfloat16]
DT_IDS = ["f32", "bf16"]
WORST = {}                # (form, output) -> (worst error / bar, where)


@pytest.fixture(scope="module")
def ops():
    from wsmgmap import ops as o
    yield o
    for (form, n), (x, where) in sorted(WORST.items()):
        print(f"\nworst measured error / bar, {form} {n}: {x:.3f} at {where}", end="")
    print()


def sfx(dtype):
    return "_bf16" if dtype == torch.bfloat16 else ""


def close(name, got, ref, bar, key=None):
    """|got - ref| <= bar elementwise (bar: a float64 tensor of ref's shape); prints the measured error beside the bar at the element
    that comes closest to it.  A NaN in got fails."""
    got = got.detach().double().cpu()
    ref = torch.as_tensor(ref).detach().double().cpu()
    assert got.shape == ref.shape == bar.shape, (name, got.shape, ref.shape, bar.shape)
    err = (got - ref).abs()
    rel = err / bar
    finite = bool(torch.isfinite(got).all())
    k = int(rel.flatten().argmax()) if finite else 0
    worst = float(rel.flatten()[k]) if finite else float("inf")
    print(f"{name}: max abs err {float(err.max()):.3e} (ref max {float(ref.abs().max()):.3e}); closest to its bar: err "
          f"{float(err.flatten()[k]):.3e} of {float(bar.flatten()[k]):.3e}")
    if key is not None and worst > WORST.get(key, (0.0,))[0]:
        WORST[key] = (worst, name)
    assert finite and worst <= 1.0, f"{name}: err {float(err.flatten()[k]):.3e} against a bar of {float(bar.flatten()[k]):.3e} ({worst:.2f} x)"


class Guarded:
    """A device tensor of `shape` in the middle of a larger buffer filled with NaN."""

    def __init__(self, shape, dtype):
        self.n = int(np.prod(shape))
        self.buf = torch.full((self.n + 2 * GUARD,), float("nan"), dtype=dtype, device="cuda")
        self.t = self.buf[GUARD:GUARD + self.n].view(shape)
        assert self.t.data_ptr() % 16 == 0

    def guards_intact(self):
        torch.cuda.synchronize()
        return bool(torch.isnan(self.buf[:GUARD]).all()) and bool(torch.isnan(self.buf[GUARD + self.n:]).all())

    def untouched(self):
        torch.cuda.synchronize()
        return bool(torch.isnan(self.buf).all())


def call(name, *args):
    from wsmgmap import _abi
    _abi.call(name, *args)


def rc_of(name, *args):
    from wsmgmap import _abi
    return getattr(_abi.lib(), name)(*args)


def P(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def S():
    from wsmgmap import ops as o
    return o._stream()


def case_id(inp):
    return f"{inp['form']}.I{inp['I']}.{inp['kind']}.{inp['mask_name']}.{DT_IDS[inp['bf16']]}" + (f".{inp['shared']}" if inp["shared"] else "")


def dev_mask(inp):
    return None if inp["mask"] is None else inp["mask"].to(torch.uint8).cuda()


def check_fully_masked(name, inp, attn):
    """The fully masked row of the grid kind: finite weights that sum to 1 (the comparison with the float32-semantics reference is the
    caller's close())."""
    if inp["mask_name"] != "full_row":
        return
    rows = inp["mask"][inp["inverse"]].all(dim=1)
    assert bool(rows.any())
    a = attn.detach().double().cpu()[rows]
    assert bool(torch.isfinite(a).all()) and float((a.sum(dim=1) - 1).abs().max()) <= 1e-5, name


FORM_COUNTS = [(f, I) for f in ac.FORMS for I in ac.COUNTS[f]]
# section 1 takes a count below 2304 whole and the two large counts one kind at a time (kind None: every kind)
OPS_CASES = [(f, I, k) for f, I in FORM_COUNTS for k in ((None,) if I < ac.LARGE else tuple(ac.KINDS) + ("grid",))]


# ============================================================================= 1. through ops
@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("form,I,only", OPS_CASES, ids=[f"{f}-{I}" + (f"-{k}" if k else "") for f, I, k in OPS_CASES])
def test_forward_and_backward_through_ops(ops, form, I, only, dtype):
    """ops.attention (distinct k and v: the generic kernels) / ops.attention_folded (the keys-are-values kernels; the key projection
    applied explicitly in the reference) at every (kind, mask) of the count: out, attn and every gradient under the derived bars."""
    bf16 = dtype == torch.bfloat16
    for kind, mask in ac.combos(form, I, only):
        inp = ac.inputs(form, I, kind, mask, bf16)
        ref = ac.reference(inp)
        bar = ac.bars(inp, ref)
        gr = ref["grads"]["both"]
        name = case_id(inp)
        m = dev_mask(inp)
        if form == "generic":
            q, k, v = (inp[n].to(dtype if n != "q" else torch.float32).cuda().requires_grad_(True) for n in ("q", "k", "v"))
            assert k.data_ptr() != v.data_ptr()
            out, attn = ops.attention(q, k, v, m, ac.SCALE)
            leaves = {"dq": q, "dk": k, "dv": v}
        else:
            q0 = inp["q0"].float().cuda().requires_grad_(True)
            w = inp["W"].float().reshape(ac.C, ac.C, 1).cuda().requires_grad_(True)
            b = inp["b"].float().cuda().requires_grad_(True)
            x = inp["k"].to(dtype).cuda().requires_grad_(True)
            out, attn = ops.attention_folded(q0, w, b, x, None if m is None else m.bool(), ac.SCALE)
            leaves = {"dq0": q0, "dW": w, "dx": x}
        ((out * inp["dout"].cuda()).sum() + (attn * inp["dattn"].cuda()).sum()).backward()
        close(name + ".out", out, ref["out"], bar["out"], (form, "out"))
        close(name + ".attn", attn, ref["attn"], bar["attn"], (form, "attn"))
        check_fully_masked(name, inp, attn)
        for n, leaf in leaves.items():
            close(f"{name}.{n}", leaf.grad.float().reshape(gr[n].shape), gr[n], bar[n], (form, n))
        if form == "same":
            assert float(b.grad.abs().max()) == 0.0          # the key bias: constant over the tokens, exactly no gradient


# ============================================================================= 2. direct calls
def direct_combos(form, I):
    want = [("plain", "none"), ("plain", "scattered"), ("ascending", "none"), ("peak_last", "prefix_I-1"), ("grid", "full_row")]
    return [c for c in want if c in ac.combos(form, I)]


def run_direct(inp, dtype, mode):
    """wsmg_attn_fwd / wsmg_attn_bwd (or the shared entry points) into guarded buffers; the backward reads the forward's own weights.
    form "same": k == v and dk == dv as pointers, which is what selects the keys-are-values kernels."""
    form, I, B, U = inp["form"], inp["I"], inp["B"], inp["U"]
    same = form == "same"
    q, g = inp["q"].cuda(), inp["dout"].cuda()
    k = inp["k"].to(dtype).cuda()
    v = k if same else inp["v"].to(dtype).cuda().clone()
    assert (k.data_ptr() == v.data_ptr()) == same
    if mode == "dattn":
        g = torch.zeros_like(g)
    ga = None if mode == "dout" else inp["dattn"].cuda()
    m = dev_mask(inp)
    out, attn, dq = Guarded((B, ac.C), torch.float32), Guarded((B, I), torch.float32), Guarded((B, ac.C), torch.float32)
    res = {"out": out, "attn": attn, "dq": dq}
    if inp["shared"]:
        inv = inp["inverse"].cuda()
        dl = res["dlogits"] = Guarded((B, I), torch.float32)
        call("wsmg_attn_shared_fwd" + sfx(dtype), P(q), P(k), P(v), P(m), P(inv), ac.SCALE, B, I, ac.C, P(out.t), P(attn.t), S())
        call("wsmg_attn_shared_bwd" + sfx(dtype), P(q), P(k), P(v), P(attn.t), P(g), P(ga), P(inv), ac.SCALE, B, I, ac.C, P(dq.t), P(dl.t), S())
    else:
        dk = Guarded((U, I, ac.C), dtype)
        dv = dk if same else Guarded((U, I, ac.C), dtype)
        res.update({"dx": dk} if same else {"dk": dk, "dv": dv})
        call("wsmg_attn_fwd" + sfx(dtype), P(q), P(k), P(v), P(m), ac.SCALE, B, I, ac.C, P(out.t), P(attn.t), S())
        call("wsmg_attn_bwd" + sfx(dtype), P(q), P(k), P(v), P(attn.t), P(g), P(ga), ac.SCALE, B, I, ac.C, P(dq.t), P(dk.t), P(dv.t), S())
    for n, t in res.items():
        assert t.guards_intact(), n
    return {n: t.t.clone() for n, t in res.items()}


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("form,I", FORM_COUNTS, ids=[f"{f}-{I}" for f, I in FORM_COUNTS])
def test_direct_calls_write_their_extent_only_and_take_every_gradient_input(form, I, dtype):
    """wsmg_attn_fwd[_bf16] / wsmg_attn_bwd[_bf16] with k == v and dk == dv (keys-are-values kernels: the dispatch is by pointer equality)
    or distinct tensors (generic kernels): only the outputs' own extents change; dout alone (dattn = NULL), dattn alone (dout zeros)
    and both are each the float64 gradient; a second launch is bit-identical (no atomics)."""
    bf16 = dtype == torch.bfloat16
    for kind, mask in direct_combos(form, I):
        inp = ac.inputs(form, I, kind, mask, bf16)
        ref = ac.reference(inp)
        for mode in ("both", "dout", "dattn"):
            bar = ac.bars(inp, ref, mode)
            got = run_direct(inp, dtype, mode)
            want = dict(ref["grads"][mode], out=ref["out"], attn=ref["attn"])
            for n, t in got.items():
                if mode == "both" or n not in ("out", "attn"):
                    close(f"direct.{case_id(inp)}.{mode}.{n}", t.float(), want[n], bar[n], (form, n))
            check_fully_masked(case_id(inp), inp, got["attn"])
            if mode == "both":
                again = run_direct(inp, dtype, mode)
                for n in got:
                    assert torch.equal(got[n].view(torch.int16 if got[n].dtype == torch.bfloat16 else torch.int32),
                                       again[n].view(torch.int16 if got[n].dtype == torch.bfloat16 else torch.int32)), (case_id(inp), n)


# ============================================================================= 3. the two forms agree
@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("I", [1, 9, 136, 257, 2304])
def test_one_tensor_and_two_equal_tensors_meet_the_same_reference(I, dtype):
    """Identical data as one tensor (keys-are-values kernels) and as two tensors of equal values (generic kernels): both inside the bars
    of the same float64 reference — dk + dv of the generic form is the one-tensor form's dx."""
    bf16 = dtype == torch.bfloat16
    for kind, mask in (("plain", "none"), ("lane_tagged", "prefix_I-1" if I > 1 else "prefix_I"), ("grid", "full_row")):
        inp = ac.inputs("same", I, kind, mask, bf16)
        ref = ac.reference(inp)
        one = run_direct(inp, dtype, "both")
        two_inp = dict(inp, form="generic", v=inp["k"].clone())
        two_ref = ac.reference(two_inp)
        two = run_direct(two_inp, dtype, "both")
        b1, b2 = ac.bars(inp, ref), ac.bars(two_inp, two_ref)
        name = case_id(inp)
        want1, want2 = dict(ref["grads"]["both"], out=ref["out"], attn=ref["attn"]), dict(two_ref["grads"]["both"], out=two_ref["out"], attn=two_ref["attn"])
        for n in ("out", "attn", "dq"):
            assert float((want1[n] - want2[n]).abs().max()) <= 1e-12 * (1 + float(want1[n].abs().max()))      # one reference
            close(f"one.{name}.{n}", one[n], want1[n], b1[n], ("same", n))
            close(f"two.{name}.{n}", two[n], want2[n], b2[n], ("generic", n))
        close(f"one.{name}.dx", one["dx"].float(), ref["grads"]["both"]["dx"], b1["dx"], ("same", "dx"))
        close(f"two.{name}.dk+dv", two["dk"].double() + two["dv"].double(), ref["grads"]["both"]["dx"], b2["dk"] + b2["dv"])


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("I", [9, 257])
def test_two_equal_tensors_with_one_gradient_buffer(I, dtype):
    """k != v as pointers (equal values) with dk == dv: the launcher wants k == v AND dk == dv for the keys-are-values kernels, so this
    call stays on the generic ones, whose backward then writes the ONE tensor dk[i] = dl[i] q + attn[i] dout into the buffer — the float64
    dx, under the bar of the two-tensor form's dk + dv."""
    bf16 = dtype == torch.bfloat16
    for kind, mask in (("plain", "none"), ("lane_tagged", "prefix_I-1"), ("grid", "full_row")):
        inp = ac.inputs("same", I, kind, mask, bf16)
        ref = ac.reference(inp)
        two_inp = dict(inp, form="generic", v=inp["k"].clone())
        b2 = ac.bars(two_inp, ac.reference(two_inp))
        B, U = inp["B"], inp["U"]
        q, g, ga, m = inp["q"].cuda(), inp["dout"].cuda(), inp["dattn"].cuda(), dev_mask(inp)
        k = inp["k"].to(dtype).cuda()
        v = k.clone()
        assert k.data_ptr() != v.data_ptr()
        out, attn, dq = Guarded((B, ac.C), torch.float32), Guarded((B, I), torch.float32), Guarded((B, ac.C), torch.float32)
        dx = Guarded((U, I, ac.C), dtype)
        call("wsmg_attn_fwd" + sfx(dtype), P(q), P(k), P(v), P(m), ac.SCALE, B, I, ac.C, P(out.t), P(attn.t), S())
        call("wsmg_attn_bwd" + sfx(dtype), P(q), P(k), P(v), P(attn.t), P(g), P(ga), ac.SCALE, B, I, ac.C, P(dq.t), P(dx.t), P(dx.t), S())
        name = "two_one_buffer." + case_id(inp)
        for n, t in (("out", out), ("attn", attn), ("dq", dq), ("dx", dx)):
            assert t.guards_intact(), (name, n)
        close(f"{name}.out", out.t, ref["out"], b2["out"], ("generic", "out"))
        close(f"{name}.attn", attn.t, ref["attn"], b2["attn"], ("generic", "attn"))
        close(f"{name}.dq", dq.t, ref["grads"]["both"]["dq"], b2["dq"], ("generic", "dq"))
        close(f"{name}.dx", dx.t.float(), ref["grads"]["both"]["dx"], b2["dk"] + b2["dv"])


# ============================================================================= 4. shared sets
def shared_combos(I):
    want = [("plain", "none"), ("plain", "scattered"), ("plain", "first_sweep"), ("plain", "one_wave"), ("ascending", "prefix_I-1"),
            ("peak_last", "scattered"), ("shifted-200", "none"), ("lane_tagged", "prefix_1"), ("grid", "full_row")]
    return [(k, m) for k, m in want if ac.applies("generic", I, m)]


SHARED_IDS = [f"{n}-{I}" for n in ac.SHARED for I in ac.SHARED_COUNTS]


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("name,I", [(n, I) for n in ac.SHARED for I in ac.SHARED_COUNTS], ids=SHARED_IDS)
def test_shared_sets_with_masks_that_are_no_prefix(ops, name, I, dtype):
    """ops.attention_shared and the direct wsmg_attn_shared_* calls over every index vector of attn_cases.SHARED with per-set masks:
    out, attn, dq, dK, dV and dlogits itself; a set that no row uses gets exactly zero dK and dV; the None gradients that
    set_materialize_grads(False) lets through (only out used, only attn used) are each the float64 gradient."""
    bf16 = dtype == torch.bfloat16
    for kind, mask in shared_combos(I):
        inp = ac.inputs("generic", I, kind, mask, bf16, name)
        ref = ac.reference(inp)
        m, inv = dev_mask(inp), inp["inverse"].cuda()
        cid = case_id(inp)
        for mode in ("both", "dout", "dattn"):
            bar = ac.bars(inp, ref, mode)
            gr = ref["grads"][mode]
            q = inp["q"].cuda().requires_grad_(True)
            k, v = (inp[n].to(dtype).cuda().requires_grad_(True) for n in ("k", "v"))
            out, attn = ops.attention_shared(q, k, v, m, inv, ac.SCALE)
            lo, la = (out * inp["dout"].cuda()).sum(), (attn * inp["dattn"].cuda()).sum()
            {"both": lo + la, "dout": lo, "dattn": la}[mode].backward()          # "dout" / "dattn": the other gradient arrives as None
            if mode == "both":
                close(f"shared.{cid}.out", out, ref["out"], bar["out"], ("shared", "out"))
                close(f"shared.{cid}.attn", attn, ref["attn"], bar["attn"], ("shared", "attn"))
                check_fully_masked(cid, inp, attn)
            for n, leaf in (("dq", q), ("dk", k), ("dv", v)):
                close(f"shared.{cid}.{mode}.{n}", leaf.grad.float(), gr[n], bar[n], ("shared", n))
            for u in set(range(inp["U"])) - set(inp["inverse"].tolist()):
                assert float(k.grad[u].float().abs().max()) == 0.0 and float(v.grad[u].float().abs().max()) == 0.0, (cid, u)
            got = run_direct(inp, dtype, mode)
            for n in ("dq", "dlogits"):
                close(f"shared_direct.{cid}.{mode}.{n}", got[n], gr[n], bar[n], ("shared", n))
        again = run_direct(inp, dtype, "dattn")
        assert all(torch.equal(got[n].view(torch.int32), again[n].view(torch.int32)) for n in got), cid


# ============================================================================= 5. refusals
@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
def test_refused_sizes_return_einval_and_write_nothing(dtype):
    """I = AMAX_I + 1 = 2561, I = 0, C != 256 and (shared form) a NULL row index or a NULL dlogits: WSMG_EINVAL from every entry point,
    in both dispatch branches, and the guarded outputs stay all-NaN.  (I = 2561 would overrun the logits in LDS.)"""
    B, I = 2, ac.REFUSED_I
    q = torch.zeros(B, ac.C, device="cuda")
    k = torch.zeros(B, I, ac.C, dtype=dtype, device="cuda")
    v = torch.zeros_like(k)
    a = torch.zeros(B, I, device="cuda")
    inv = torch.zeros(B, dtype=torch.int64, device="cuda")
    out, attn, dq, dl = (Guarded(s, torch.float32) for s in ((B, ac.C), (B, I), (B, ac.C), (B, I)))
    dk, dv = Guarded((B, I, ac.C), dtype), Guarded((B, I, ac.C), dtype)
    x = sfx(dtype)
    for i, c, idx in ((I, ac.C, inv), (0, ac.C, inv), (16, 128, inv), (16, 264, inv), (16, ac.C, None)):
        if idx is not None:
            for kk, vv, dkk, dvv in ((k, v, dk, dv), (k, k, dk, dk)):
                assert rc_of("wsmg_attn_fwd" + x, P(q), P(kk), P(vv), None, ac.SCALE, B, i, c, P(out.t), P(attn.t), S()) == EINVAL
                assert rc_of("wsmg_attn_bwd" + x, P(q), P(kk), P(vv), P(a), P(q), None, ac.SCALE, B, i, c, P(dq.t), P(dkk.t), P(dvv.t), S()) == EINVAL
        assert rc_of("wsmg_attn_shared_fwd" + x, P(q), P(k), P(v), None, P(idx), ac.SCALE, B, i, c, P(out.t), P(attn.t), S()) == EINVAL
        assert rc_of("wsmg_attn_shared_bwd" + x, P(q), P(k), P(v), P(a), P(q), None, P(idx), ac.SCALE, B, i, c, P(dq.t), P(dl.t), S()) == EINVAL
    assert rc_of("wsmg_attn_shared_bwd" + x, P(q), P(k), P(v), P(a), P(q), None, P(inv), ac.SCALE, B, 16, ac.C, P(dq.t), None, S()) == EINVAL
    for t in (out, attn, dq, dl, dk, dv):
        assert t.untouched()
