"""GPU: the kernels of csrc/wsmg_norm.hip at the edges of their column reduction and of its finalize pass.  Inputs, float64 references
and bars are those of tests/norm_cases.py (checked on the CPU by tests/test_norm_cases_cpu.py); the BatchNorm bars are the project's
own of test_gpu_kernels.py::test_bn_act_train / test_bn_act_bf16, not widened for the large cases.  Every comparison prints its
measured error over its bar; the module prints the worst ratio per section, type and output at its end (profiles/norm_edges.txt).

Section, what it pins, and what held it before:
a. reduction edges   col_reduce_kernel<1 | 2>, bn_stats_finalize_kernel, sum_finalize_kernel<true>, the apply kernels, forward + backward
                     at 2 ... rpi + 1 ... 8 rpi + 1 rows, at 63 ... 257 blocks (both loops of reduce_partials), at the cap of 1024
                     blocks, one row past it and two rounds past it; C = 256 everywhere, C = 32 and 512 at 65 / 193 blocks and the cap
                     — test_bn_act_train / test_bn_act_bf16: at most 59 blocks, C <= 256
b. mode matrix       {f32, bf16} x {residual} x {ReLU} at every C of chan_ok, train forward + backward; eval forward, its untouched
                     running statistics and its refused backward — bf16 without ReLU and residual without ReLU had no test
c. strided dy        wsmg_bn_act_bwd_ld[_bf16]: dy a channel slice of a wider tensor read in place (ops.core._rows_of), the
                     misaligned slice through its copy, the refusals of the entry point itself — whole-policy tests only;
                     wsmg_bn_act_bwd[_bf16] (the same with ld = C, no longer on the ops route) directly
d. dx_lo             wsmg_bn_act_bwd_ld_bf16_lo through ops.GradLoSink — whole-policy tests only
e. slabs             wsmg_bn_act_fwd_bf16_pre at 1 ... 257 slabs (the model uses 8 and 64), wsmg_bn_stats_finalize +
                     wsmg_bn_bwd_apply_bf16 directly, in place too — the classifier tail's C = 32 only
f. channel sums      wsmg_channel_sum[_bf16] (col_reduce_kernel<0>, sum_finalize_kernel<false>) at every C — no direct test
g. refusals          unsupported C, rows = 0: WSMG_EINVAL; a workspace one byte short: WSMG_ENOMEM; nothing written
h. GroupNorm         group_norm_nhwc_bf16_kernel<float | bf16> at groups of 1, 3, 5 ... elements, fewer than 256, no multiple of 256,
                     C / G no power of two, H W = 1 — G = 16 on the backbone's shapes and one G = 1 case

NOT reached on purpose: the cap of 4096 blocks of stream_grid (the apply kernels' grid).  It needs 16.7 M float32 /
33.5 M bf16 elements, and it only changes the stride of a grid-stride loop that every case here already walks four or more times per
thread.  The largest case is 32 775 x 512 = 16.8 M elements (section a, "beyond" at C = 512)."""
import ctypes

import pytest
import torch

import norm_cases as nc
from norm_cases import BF16_EPS

pytestmark = pytest.mark.gpu

EINVAL, ENOMEM = -1, -2
NAN = float("nan")
DTYPES = [torch.float32, torch.bfloat16]
DT_IDS = ["f32", "bf16"]
MODES = [(False, False), (False, True), (True, False), (True, True)]        # (residual, relu)
MODE_IDS = ["plain", "relu", "res", "res_relu"]
WORST = {}                # (section, type, output) -> (worst error / bar, where)


@pytest.fixture(scope="module")
def ops():
    from wsmgmap import ops as o
    yield o
    for (sec, dt, n), (x, where) in sorted(WORST.items()):
        print(f"\nworst measured error / bar, {sec} {dt} {n}: {x:.3f} at {where}", end="")
    print()


def lib():
    from wsmgmap import _abi
    return _abi.lib()


def P(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def S():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def sfx(bf16):
    return "_bf16" if bf16 else ""


def close(name, got, ref, rtol, atol, key=None):
    """|got - ref| <= atol + rtol |ref| elementwise against the float64 reference; prints the measured error over the bar.  NaN fails."""
    got = got.detach().double().cpu().reshape(ref.shape)
    ref = ref.detach().double()
    err = (got - ref).abs()
    finite = bool(torch.isfinite(got).all())
    ratio = float((err / (atol + rtol * ref.abs())).max()) if finite else float("inf")
    print(f"{name}: max abs err {float(err.max()):.3e} (ref max {float(ref.abs().max()):.3e}), error / bar {ratio:.3f}")
    if key is not None and ratio > WORST.get(key, (-1.0,))[0]:
        WORST[key] = (ratio, name)
    assert finite and ratio <= 1.0, f"{name}: max abs err {float(err.max()):.3e} (ref max {float(ref.abs().max()):.3e}), {ratio:.3f} x its bar"


def close_bar(name, got, ref, bar, key=None):
    """As close(), with an elementwise float64 bar."""
    got = got.detach().double().cpu().reshape(ref.shape)
    err = (got - ref).abs()
    finite = bool(torch.isfinite(got).all())
    ratio = float((err / bar).max()) if finite else float("inf")
    print(f"{name}: max abs err {float(err.max()):.3e} (ref max {float(ref.abs().max()):.3e}), error / bar {ratio:.3f}")
    if key is not None and ratio > WORST.get(key, (-1.0,))[0]:
        WORST[key] = (ratio, name)
    assert finite and ratio <= 1.0, f"{name}: max abs err {float(err.max()):.3e}, {ratio:.3f} x its bar"


def library_nblk(rows, C):
    return int(lib().wsmg_channel_reduce_workspace_bytes(rows, C)) // (16 * C)


def run_bn(ops, c, bf16, res, relu, wide=None, lo_sink=None, stats=None, copy_expected=False):
    """One train-mode forward + backward of case c through ops.bn_act.  wide = (Ctot, c0): the gradient arrives as channels
    [c0, c0 + C) of a contiguous [B, H, W, Ctot] tensor, the way autograd hands back one part of a torch.cat.
    -> dict(y, dx, dgamma, dbeta, dres, rm, rv, mean, invstd)."""
    dt = torch.bfloat16 if bf16 else torch.float32
    B, H, W = c["shape"]
    C = c["x"].shape[1]
    xg = c["x"].to(dt).view(B, H, W, C).cuda().requires_grad_(True)
    rg = c["res"].to(dt).view(B, H, W, C).cuda().requires_grad_(True) if res else None
    gg, bg = c["gamma"].cuda().requires_grad_(True), c["beta"].cuda().requires_grad_(True)
    rm, rv = c["rm"].cuda(), c["rv"].cuda()
    y = ops.bn_act(xg, gg, bg, rm, rv, True, relu, rg, nc.MOMENTUM, nc.EPS, stats, lo_sink)
    assert y.dtype == dt and y.shape == xg.shape
    saved = y.grad_fn.saved_tensors
    dy = c["dy"].to(dt).view(B, H, W, C)
    if wide is None:
        y.backward(dy.cuda())
    else:
        Ctot, c0 = wide
        g = nc.T(nc.df.uniform("normedge.wide", (B, H, W, Ctot), 2.0)).to(dt)
        g[..., c0:c0 + C] = dy
        g = g.cuda()
        part = g[..., c0:c0 + C]
        got, ld = ops.core._rows_of(part, C)
        assert (ld == C and got.is_contiguous()) if copy_expected else (ld == Ctot and got.data_ptr() == part.data_ptr()), (ld, Ctot)
        parts = ([torch.zeros(B, H, W, c0, dtype=dt, device="cuda")] if c0 else []) + [y]
        if Ctot - C - c0:
            parts.append(torch.zeros(B, H, W, Ctot - C - c0, dtype=dt, device="cuda"))
        torch.cat(parts, dim=-1).backward(g)
    torch.cuda.synchronize()
    return dict(y=y.detach(), dx=xg.grad, dgamma=gg.grad, dbeta=bg.grad, dres=rg.grad if res else None, rm=rm, rv=rv,
                mean=saved[4], invstd=saved[5])


def check_bn(name, sec, c, bf16, res, out, forward_only=False):
    bars, dt = nc.bn_bars(c, bf16), DT_IDS[bf16]
    close(name + ".y", out["y"], c["fwd"]["y"], *bars["y"], key=(sec, dt, "y"))
    close(name + ".running_mean", out["rm"], c["fwd"]["running_mean"], *bars["running_mean"], key=(sec, dt, "running_mean"))
    close(name + ".running_var", out["rv"], c["fwd"]["running_var"], *bars["running_var"], key=(sec, dt, "running_var"))
    if forward_only:
        return
    close(name + ".dx", out["dx"], c["bwd"]["dx"], *bars["dx"], key=(sec, dt, "dx"))
    close(name + ".dgamma", out["dgamma"], c["bwd"]["dgamma"], *bars["dgamma"], key=(sec, dt, "dgamma"))
    close(name + ".dbeta", out["dbeta"], c["bwd"]["dbeta"], *bars["dbeta"], key=(sec, dt, "dbeta"))
    if res:     # dy masked, copied: exact (dy is 0 wherever the float32 and the float64 mask could differ)
        assert torch.equal(out["dres"].double().cpu().reshape(c["bwd"]["dres"].shape), c["bwd"]["dres"]), name + ".dres"


# ----------------------------------------------------------------------------- a. row and block edges of the reduction
@pytest.mark.parametrize("bf16", [False, True], ids=DT_IDS)
@pytest.mark.parametrize("C,edge", nc.EDGE_CASES, ids=[f"C{C}.{e}" for C, e in nc.EDGE_CASES])
def test_bn_reduction_edges(ops, C, edge, bf16):
    rows, nblk = nc.edge_rows(C)[edge]
    assert library_nblk(rows, C) == nblk, f"{edge} at C = {C}: the library reduces {rows} rows with {library_nblk(rows, C)} blocks, not {nblk}"
    c = nc.bn_case(C, rows, bf16, True, True)
    check_bn(f"a.C{C}.{edge}.{DT_IDS[bf16]}", "a", c, bf16, True, run_bn(ops, c, bf16, True, True))


# ----------------------------------------------------------------------------- b. mode matrix
@pytest.mark.parametrize("bf16", [False, True], ids=DT_IDS)
@pytest.mark.parametrize("res,relu", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("C", nc.CHANNELS)
def test_bn_mode_matrix_train(ops, C, res, relu, bf16):
    B, H, W = nc.MODE_SHAPES[C]
    c = dict(nc.bn_case(C, B * H * W, bf16, res, relu), shape=(B, H, W))
    out = run_bn(ops, c, bf16, res, relu)
    check_bn(f"b.C{C}.{MODE_IDS[MODES.index((res, relu))]}.{DT_IDS[bf16]}", "b", c, bf16, res, out)
    close(f"b.C{C}.mean", out["mean"], c["fwd"]["mean"], 1e-6, 1e-6)
    close(f"b.C{C}.invstd", out["invstd"], c["fwd"]["invstd"], 1e-6, 0.0)


@pytest.mark.parametrize("bf16", [False, True], ids=DT_IDS)
@pytest.mark.parametrize("res", [False, True], ids=["plain", "res"])
@pytest.mark.parametrize("C", nc.CHANNELS)
def test_bn_mode_matrix_eval(ops, C, res, bf16):
    """Eval mode: the running statistics are used and stay bit-unchanged; backward raises the documented WsmgError."""
    from wsmgmap import _abi
    dt = torch.bfloat16 if bf16 else torch.float32
    B, H, W = nc.MODE_SHAPES[C]
    c = nc.bn_case(C, B * H * W, bf16, res, True)
    d = {k: (c[k].double() if c[k] is not None else None) for k in ("x", "gamma", "beta", "res", "rm", "rv")}
    ref = nc.bn_forward_ref(d["x"], d["gamma"], d["beta"], d["res"], True, d["rm"], d["rv"], train=False)
    xg = c["x"].to(dt).view(B, H, W, C).cuda().requires_grad_(True)
    rg = c["res"].to(dt).view(B, H, W, C).cuda() if res else None
    rm, rv = c["rm"].cuda(), c["rv"].cuda()
    y = ops.bn_act(xg, c["gamma"].cuda(), c["beta"].cuda(), rm, rv, False, True, rg, nc.MOMENTUM, nc.EPS)
    close(f"b.eval.C{C}.{DT_IDS[bf16]}.y", y, ref["y"], *nc.bn_bars(c, bf16)["y"], key=("b.eval", DT_IDS[bf16], "y"))
    assert torch.equal(rm.cpu(), c["rm"]) and torch.equal(rv.cpu(), c["rv"])
    with pytest.raises(_abi.WsmgError, match="eval-mode BatchNorm"):
        y.backward(torch.ones_like(y))
    assert torch.equal(rm.cpu(), c["rm"]) and torch.equal(rv.cpu(), c["rv"])


# ----------------------------------------------------------------------------- c. strided dy
@pytest.mark.parametrize("bf16", [False, True], ids=DT_IDS)
@pytest.mark.parametrize("res", [False, True], ids=["relu", "res_relu"])
@pytest.mark.parametrize("C,Ctot,c0", nc.STRIDED, ids=[f"C{a}of{b}at{c}" for a, b, c in nc.STRIDED])
def test_bn_backward_reads_a_channel_slice_in_place(ops, monkeypatch, C, Ctot, c0, res, bf16):
    from wsmgmap import _abi
    B, H, W = nc.STRIDED_SHAPE
    c = dict(nc.bn_case(C, B * H * W, bf16, res, True), shape=(B, H, W))
    called, real = [], _abi.call
    monkeypatch.setattr(_abi, "call", lambda name, *a: (called.append(name), real(name, *a))[1])
    out = run_bn(ops, c, bf16, res, True, wide=(Ctot, c0))
    assert "wsmg_bn_act_bwd_ld" + sfx(bf16) in called, called
    check_bn(f"c.C{C}of{Ctot}at{c0}.{'res_relu' if res else 'relu'}.{DT_IDS[bf16]}", "c", c, bf16, res, out)


@pytest.mark.parametrize("res", [False, True], ids=["relu", "res_relu"])
def test_bn_backward_copies_a_misaligned_slice(ops, monkeypatch, res):
    """c0 = 4 bf16 elements: rows start 8 bytes off a 16-byte boundary, _rows_of must hand the kernel a contiguous copy."""
    from wsmgmap import _abi
    C, Ctot, c0 = nc.MISALIGNED
    B, H, W = nc.STRIDED_SHAPE
    c = dict(nc.bn_case(C, B * H * W, True, res, True), shape=(B, H, W))
    called, real = [], _abi.call
    monkeypatch.setattr(_abi, "call", lambda name, *a: (called.append((name, a[1] if len(a) > 1 else None)), real(name, *a))[1])
    out = run_bn(ops, c, True, res, True, wide=(Ctot, c0), copy_expected=True)
    strides = [ld for name, ld in called if name == "wsmg_bn_act_bwd_ld_bf16"]     # the one backward entry point, told the copy's stride
    assert strides == [C] and not any(name.startswith("wsmg_bn_act_bwd") and name != "wsmg_bn_act_bwd_ld_bf16" for name, _ in called), called
    check_bn(f"c.misaligned.{'res_relu' if res else 'relu'}.bf16", "c", c, True, res, out)


@pytest.mark.parametrize("bf16", [False, True], ids=DT_IDS)
def test_bn_backward_ld_refuses_bad_strides_before_anything_is_queued(bf16):
    C, rows = 64, 70
    dt = torch.bfloat16 if bf16 else torch.float32
    wide = torch.zeros(rows + 1, 96, dtype=dt, device="cuda")
    x = torch.zeros(rows, C, dtype=dt, device="cuda")
    par = torch.ones(C, device="cuda")
    dx = torch.full((rows, C), NAN, dtype=dt, device="cuda")
    dg, db = torch.full((C,), NAN, device="cuda"), torch.full((C,), NAN, device="cuda")
    ws = torch.empty(1024 * 2 * 64, dtype=torch.float64, device="cuda")
    fn = getattr(lib(), "wsmg_bn_act_bwd_ld" + sfx(bf16))
    off = ctypes.c_void_p(wide.data_ptr() + 4)         # 4 bytes: one float32, two bf16 — off every 16-byte boundary

    def rc(dy, ld):
        return fn(dy, ld, P(x), None, P(par), P(par), P(par), P(par), 0, rows, C, P(dx), None, P(dg), P(db), P(ws), ws.numel() * 8, S())
    assert rc(P(wide), 96) == 0                        # the same call with a good stride is taken
    torch.cuda.synchronize()
    dx.fill_(NAN), dg.fill_(NAN), db.fill_(NAN)
    assert rc(P(wide), C - 8) == EINVAL                # ld_dy < C
    assert rc(P(wide), 92) == EINVAL                   # ld_dy % 8 != 0
    assert rc(off, 96) == EINVAL                       # dy not 16-byte aligned
    torch.cuda.synchronize()
    assert bool(torch.isnan(dx).all()) and bool(torch.isnan(dg).all()) and bool(torch.isnan(db).all())


# ----------------------------------------------------------------------------- d. dx_lo
@pytest.mark.parametrize("C,rows,res", [(256, nc.edge_rows(256)["nblk65"][0], False), (64, 2 * 13 * 19, True)], ids=["nblk65", "res"])
def test_bn_backward_low_half_of_the_gradient(ops, C, rows, res):
    """dx with a GradLoSink is bit-identical to dx without; dx + dx_lo is the float32 gradient to 16 mantissa bits: lo is at most
    2^-9 |dx| and itself rounded to 8 bits, so 2^-17 |ref| beside the float32 kernel's bar of test_bn_act_train (1e-4, 2e-5)."""
    c = nc.bn_case(C, rows, True, res, True)
    assert nc.nblk_of(rows, C) == library_nblk(rows, C) and (res or library_nblk(rows, C) == 65)
    plain = run_bn(ops, c, True, res, True)
    sink = ops.GradLoSink()
    out = run_bn(ops, c, True, res, True, lo_sink=sink)
    lo = sink.take()
    assert lo is not None and lo.dtype == torch.bfloat16 and lo.shape == out["dx"].shape
    assert torch.equal(out["dx"], plain["dx"]) and torch.equal(out["dgamma"], plain["dgamma"]) and torch.equal(out["dbeta"], plain["dbeta"])
    check_bn(f"d.C{C}.rows{rows}", "d", c, True, res, out)
    ref = c["bwd"]["dx"]
    close_bar(f"d.C{C}.rows{rows}.hi+lo", out["dx"].float().double() + lo.float().double(), ref.reshape(out["dx"].shape),
              (2.0 ** -17 * ref.abs() + 1e-4 * ref.abs() + 2e-5).reshape(out["dx"].shape), key=("d", "bf16", "dx+lo"))
    assert float(lo.float().abs().max()) > 0.0
    assert bool((lo.float().abs().cpu().double() <= 2.0 ** -8 * out["dx"].float().abs().cpu().double() + 1e-30).all())


# ----------------------------------------------------------------------------- e. statistics from slabs
@pytest.mark.parametrize("nslab", nc.NSLABS)
@pytest.mark.parametrize("C", [32, 256])
def test_bn_forward_takes_its_statistics_from_slabs(ops, C, nslab):
    B, H, W = nc.MODE_SHAPES[C]
    c = dict(nc.bn_case(C, B * H * W, True, False, True), shape=(B, H, W))
    slabs = nc.slab_split(c["x"].double(), nslab, f"normedge.slabs.{C}.{nslab}").cuda()
    assert int((slabs != 0).sum()) > 0
    out = run_bn(ops, c, True, False, True, stats=slabs)
    name = f"e.C{C}.nslab{nslab}"
    check_bn(name, "e", c, True, False, out)
    close(name + ".mean", out["mean"], c["fwd"]["mean"], 1e-6, 1e-6, key=("e", "bf16", "mean"))
    close(name + ".invstd", out["invstd"], c["fwd"]["invstd"], 1e-6, 0.0, key=("e", "bf16", "invstd"))
    assert int((slabs != 0).sum()) == 0 and not bool(torch.signbit(slabs).any()), "the slabs must come back exactly 0.0"


@pytest.mark.parametrize("C", [64, 256])
def test_bn_stats_finalize_and_backward_apply_direct(C):
    """wsmg_bn_stats_finalize, then wsmg_bn_bwd_apply_bf16 with an already masked dy and caller-supplied sums, out of place and in
    place (dx == dy, as ops/heads.py calls it).  Reference: the float64 formula of the float32 operands handed to the kernel."""
    B, H, W = nc.MODE_SHAPES[C]
    rows, nslab = B * H * W, 65
    c = nc.bn_case(C, rows, True, False, True)
    slabs = nc.slab_split(c["x"].double(), nslab, f"normedge.direct.{C}").cuda()
    rm, rv = c["rm"].cuda(), c["rv"].cuda()
    mean, invstd = torch.full((C,), NAN, device="cuda"), torch.full((C,), NAN, device="cuda")
    assert lib().wsmg_bn_stats_finalize(P(slabs), nslab, C, rows, nc.MOMENTUM, nc.EPS, P(rm), P(rv), P(mean), P(invstd), S()) == 0
    torch.cuda.synchronize()
    name = f"e.direct.C{C}"
    close(name + ".mean", mean, c["fwd"]["mean"], 1e-6, 1e-6, key=("e", "bf16", "mean"))
    close(name + ".invstd", invstd, c["fwd"]["invstd"], 1e-6, 0.0, key=("e", "bf16", "invstd"))
    close(name + ".running_mean", rm, c["fwd"]["running_mean"], 1e-6, 1e-6)
    close(name + ".running_var", rv, c["fwd"]["running_var"], 1e-5, 1e-6)
    assert int((slabs != 0).sum()) == 0
    g = c["bwd"]["g"]                                               # dy masked by the ReLU: bf16 values
    assert torch.equal(nc.bf_round(g.float()).double(), g)
    dgamma, dbeta = c["bwd"]["dgamma"].float(), c["bwd"]["dbeta"].float()
    m64, i64, gm = mean.cpu().double(), invstd.cpu().double(), c["gamma"].double()
    xhat = (c["x"].double() - m64) * i64
    ref = gm * i64 * (g - dbeta.double() / rows - xhat * (dgamma.double() / rows))
    dy = g.to(torch.bfloat16).cuda()
    x = c["x"].to(torch.bfloat16).cuda()
    dx = torch.full((rows, C), NAN, dtype=torch.bfloat16, device="cuda")
    keep = [c["gamma"].cuda(), dgamma.cuda(), dbeta.cuda()]
    args = (P(x), P(keep[0]), P(mean), P(invstd), P(keep[1]), P(keep[2]), rows, C)
    assert lib().wsmg_bn_bwd_apply_bf16(P(dy), *args, P(dx), S()) == 0
    torch.cuda.synchronize()
    bar = (BF16_EPS, 2e-3 * float(ref.abs().max()))
    close(name + ".dx", dx, ref, *bar, key=("e", "bf16", "dx"))
    inplace = dy.clone()
    assert lib().wsmg_bn_bwd_apply_bf16(P(inplace), *args, P(inplace), S()) == 0
    torch.cuda.synchronize()
    assert torch.equal(inplace, dx), "dx == dy must give the out-of-place result"


@pytest.mark.parametrize("bf16", [False, True], ids=DT_IDS)
def test_bn_backward_without_a_stride_direct(ops, bf16):
    """wsmg_bn_act_bwd[_bf16], which ops.bn_act no longer calls (it hands wsmg_bn_act_bwd_ld its stride, C for a contiguous dy): the
    entry point itself after wsmg_bn_act_fwd[_bf16], residual + ReLU, against the reference and bars of the ops route (check_bn)."""
    C = 64
    B, H, W = nc.MODE_SHAPES[C]
    rows = B * H * W
    c = dict(nc.bn_case(C, rows, bf16, True, True), shape=(B, H, W))
    dt = torch.bfloat16 if bf16 else torch.float32
    x, r, dy = c["x"].to(dt).cuda(), c["res"].to(dt).cuda(), c["dy"].to(dt).cuda()
    gamma, beta, rm, rv = c["gamma"].cuda(), c["beta"].cuda(), c["rm"].cuda(), c["rv"].cuda()
    y, dx, dres = (torch.full((rows, C), NAN, dtype=dt, device="cuda") for _ in range(3))
    mean, invstd, dg, db = _nan(C), _nan(C), _nan(C), _nan(C)
    need = int(lib().wsmg_channel_reduce_workspace_bytes(rows, C))
    ws = torch.empty(need // 8, dtype=torch.float64, device="cuda")
    assert getattr(lib(), "wsmg_bn_act_fwd" + sfx(bf16))(P(x), P(r), P(gamma), P(beta), P(rm), P(rv), nc.MOMENTUM, nc.EPS, 1, 1, rows, C, P(y),
                                                         P(mean), P(invstd), P(ws), need, S()) == 0
    assert getattr(lib(), "wsmg_bn_act_bwd" + sfx(bf16))(P(dy), P(x), P(y), P(gamma), P(beta), P(mean), P(invstd), 1, rows, C, P(dx), P(dres),
                                                         P(dg), P(db), P(ws), need, S()) == 0
    torch.cuda.synchronize()
    check_bn(f"c.direct.C{C}.{DT_IDS[bf16]}", "c", c, bf16, True, dict(y=y, dx=dx, dgamma=dg, dbeta=db, dres=dres, rm=rm, rv=rv))


# ----------------------------------------------------------------------------- f. channel sums
@pytest.mark.parametrize("bf16", [False, True], ids=DT_IDS)
@pytest.mark.parametrize("edge", nc.SUM_EDGES)
@pytest.mark.parametrize("C", nc.CHANNELS)
def test_channel_sum_edges(ops, C, edge, bf16):
    rows, nblk = nc.edge_rows(C)[edge]
    assert library_nblk(rows, C) == nblk
    x = nc.sum_input(C, rows, bf16, "plain")
    ref = x.double().sum(dim=0)
    got = ops.channel_sum(x.to(torch.bfloat16 if bf16 else torch.float32).cuda())
    assert got.dtype == torch.float32 and got.shape == (C,)
    close_bar(f"f.C{C}.{edge}.{DT_IDS[bf16]}", got, ref, nc.sum_bar(ref), key=("f", DT_IDS[bf16], "sum"))


@pytest.mark.parametrize("bf16", [False, True], ids=DT_IDS)
@pytest.mark.parametrize("C", nc.CHANNELS)
def test_channel_sum_of_a_zero_column_and_of_alternating_signs(ops, C, bf16):
    dt = torch.bfloat16 if bf16 else torch.float32
    for edge in ("8rpi+1", "nblk193"):
        rows = nc.edge_rows(C)[edge][0]
        x = nc.sum_input(C, rows, bf16, "zero_col")
        ref = x.double().sum(dim=0)
        got = ops.channel_sum(x.to(dt).cuda())
        close_bar(f"f.zero_col.C{C}.{edge}.{DT_IDS[bf16]}", got, ref, nc.sum_bar(ref), key=("f", DT_IDS[bf16], "sum"))
        assert float(got[5]) == 0.0 and float(ref[5]) == 0.0
        x = nc.sum_input(C, rows, bf16, "pm1")
        got = ops.channel_sum(x.to(dt).cuda())
        assert torch.equal(got.cpu().double(), x.double().sum(dim=0)), f"C = {C}, {rows} rows of +-1: the sum is exact"
        assert set(got.cpu().tolist()) == ({1.0, -1.0} if rows % 2 else {0.0})


# ----------------------------------------------------------------------------- g. refusals
def _nan(n, dtype=torch.float32):
    return torch.full((n,), NAN, dtype=dtype, device="cuda")


def _bn_entry_points(rows, C, ws, ws_bytes, outs):
    """[(name, rc)] of every BatchNorm / channel-sum entry point called with `rows` x `C`; outputs go to NaN-filled buffers (outs)."""
    L, st = lib(), S()
    src, par = outs["src"], outs["par"]
    y, mean, invstd, rm, rv, dx, dres, dg, db, out = (outs[k] for k in ("y", "mean", "invstd", "rm", "rv", "dx", "dres", "dg", "db", "out"))
    r = []
    for s in ("", "_bf16"):
        r.append(("wsmg_channel_sum" + s, getattr(L, "wsmg_channel_sum" + s)(P(src), rows, C, P(out), P(ws), ws_bytes, st)))
        r.append(("wsmg_bn_act_fwd" + s, getattr(L, "wsmg_bn_act_fwd" + s)(
            P(src), None, P(par), P(par), P(rm), P(rv), 0.1, 1e-5, 1, 1, rows, C, P(y), P(mean), P(invstd), P(ws), ws_bytes, st)))
        r.append(("wsmg_bn_act_bwd" + s, getattr(L, "wsmg_bn_act_bwd" + s)(
            P(src), P(src), None, P(par), P(par), P(par), P(par), 1, rows, C, P(dx), None, P(dg), P(db), P(ws), ws_bytes, st)))
        r.append(("wsmg_bn_act_bwd_ld" + s, getattr(L, "wsmg_bn_act_bwd_ld" + s)(
            P(src), max(C, 8), P(src), None, P(par), P(par), P(par), P(par), 1, rows, C, P(dx), None, P(dg), P(db), P(ws), ws_bytes, st)))
    r.append(("wsmg_bn_act_bwd_ld_bf16_lo", L.wsmg_bn_act_bwd_ld_bf16_lo(
        P(src), max(C, 8), P(src), None, P(par), P(par), P(par), P(par), 1, rows, C, P(dx), P(dres), None, P(dg), P(db), P(ws), ws_bytes, st)))
    return r


def _outs():
    o = {k: _nan(4096) for k in ("y", "mean", "invstd", "rm", "rv", "dx", "dres", "dg", "db", "out")}
    o["src"], o["par"] = torch.zeros(70 * 512, device="cuda"), torch.ones(1024, device="cuda")
    return o


def _untouched(o):
    torch.cuda.synchronize()
    return all(bool(torch.isnan(v).all()) for k, v in o.items() if k not in ("src", "par"))


def test_bn_entry_points_refuse_unsupported_sizes_before_anything_is_queued():
    o = _outs()
    ws = torch.empty(1024 * 2 * 512, dtype=torch.float64, device="cuda")
    L, st = lib(), S()
    for rows, C in [(70, 0), (70, 8), (70, 96), (70, 160), (70, 1024), (0, 64), (0, 512)]:
        for name, rc in _bn_entry_points(rows, C, ws, ws.numel() * 8, o):
            assert rc == EINVAL, (name, rows, C, rc)
        slabs = torch.ones(8, 2, max(C, 8), dtype=torch.float64, device="cuda")
        assert L.wsmg_bn_act_fwd_bf16_pre(P(o["src"]), None, P(o["par"]), P(o["par"]), P(o["rm"]), P(o["rv"]), 0.1, 1e-5, 1, rows, C,
                                          P(o["y"]), P(o["mean"]), P(o["invstd"]), P(slabs), 8, st) == EINVAL
        assert L.wsmg_bn_stats_finalize(P(slabs), 8, C, rows, 0.1, 1e-5, P(o["rm"]), P(o["rv"]), P(o["mean"]), P(o["invstd"]), st) == EINVAL
        assert L.wsmg_bn_bwd_apply_bf16(P(o["src"]), P(o["src"]), P(o["par"]), P(o["par"]), P(o["par"]), P(o["par"]), P(o["par"]), rows, C,
                                        P(o["dx"]), st) == EINVAL
        torch.cuda.synchronize()
        assert bool((slabs == 1).all()), "a refused call cleared the slabs"
        assert int(L.wsmg_channel_reduce_workspace_bytes(70, C)) == (0 if C != 64 and C != 512 else 16 * C * nc.nblk_of(70, C))
    assert _untouched(o)


@pytest.mark.parametrize("C,rows", [(64, 494), (512, 105), (512, nc.edge_rows(512)["cap"][0])], ids=["C64", "C512", "C512.cap"])
def test_bn_entry_points_refuse_a_workspace_one_byte_short(C, rows):
    o = _outs()
    o["src"] = torch.zeros(rows * C, device="cuda")                 # the second pass below launches: full-size buffers
    o.update({k: _nan(rows * C) for k in ("y", "dx", "dres")})
    need = int(lib().wsmg_channel_reduce_workspace_bytes(rows, C))
    assert need == 16 * C * nc.nblk_of(rows, C)
    ws = torch.empty(need // 8, dtype=torch.float64, device="cuda")
    for name, rc in _bn_entry_points(rows, C, ws, need - 1, o):
        assert rc == ENOMEM, (name, rows, C, rc)
    assert _untouched(o)
    for name, rc in _bn_entry_points(rows, C, ws, need, o):         # and with exactly what it asked for, every one is taken
        assert rc == 0, (name, rows, C, rc)
    torch.cuda.synchronize()


# ----------------------------------------------------------------------------- h. GroupNorm
@pytest.mark.parametrize("bf16", [False, True], ids=DT_IDS)
@pytest.mark.parametrize("res,relu", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("shape", nc.GN_SHAPES, ids=["x".join(map(str, s)) for s in nc.GN_SHAPES])
@pytest.mark.parametrize("C,G", nc.GN_CG, ids=[f"C{C}G{G}" for C, G in nc.GN_CG])
def test_group_norm_small_and_ragged_groups(ops, C, G, shape, res, relu, bf16):
    inp = nc.gn_inputs(C, G, shape, bf16, res)
    x, g, b = inp["x"].double(), inp["gamma"].double(), inp["beta"].double()
    ref = nc.gn_ref(x, g, b, G, nc.EPS, inp["res"].double() if res else None, relu)
    bar, _ = nc.gn_bar(inp, ref, G, nc.EPS)
    xg = inp["x"].to(torch.bfloat16 if bf16 else torch.float32).cuda()
    rg = inp["res"].to(torch.bfloat16).cuda() if res else None
    # the output is a fresh allocation: leave NaN where the allocator will find its block, so an element that is never written shows
    gam, bet = inp["gamma"].cuda(), inp["beta"].cuda()
    poison = torch.full(xg.shape, NAN, dtype=torch.bfloat16, device="cuda")
    del poison
    y = ops.group_norm_nhwc(xg, gam, bet, G, nc.EPS, relu, rg)
    assert y.dtype == torch.bfloat16 and y.shape == xg.shape
    name = f"h.C{C}G{G}.{'x'.join(map(str, shape))}.{MODE_IDS[MODES.index((res, relu))]}.{DT_IDS[bf16]}"
    close_bar(name, y.float(), ref["y"], bar, key=("h", DT_IDS[bf16], "y"))
    # and the same call into a NaN-guarded buffer of our own
    B, H, W = shape
    n = xg.numel()
    buf = torch.full((n + 128,), NAN, dtype=torch.bfloat16, device="cuda")
    rc = lib().wsmg_group_norm_nhwc_bf16(P(xg), int(not bf16), P(rg), P(gam), P(bet), B, H * W, C, G, nc.EPS, int(relu),
                                         ctypes.c_void_p(buf.data_ptr() + 128), S())
    torch.cuda.synchronize()
    assert rc == 0 and bool(torch.isnan(buf[:64]).all()) and bool(torch.isnan(buf[64 + n:]).all())
    assert torch.equal(buf[64:64 + n].view(xg.shape), y)


def test_group_norm_refuses_bad_groups_before_anything_is_queued():
    x = torch.zeros(2 * 4 * 64, device="cuda")
    par = torch.ones(64, device="cuda")
    y = torch.full((2 * 4 * 64,), NAN, dtype=torch.bfloat16, device="cuda")
    for x_f32 in (0, 1):
        for B, HW, C, G in [(2, 4, 64, 24), (2, 4, 40, 16), (2, 4, 64, 0), (65536, 1, 64, 16), (0, 4, 64, 16), (2, 0, 64, 16)]:
            rc = lib().wsmg_group_norm_nhwc_bf16(P(x), x_f32, None, P(par), P(par), B, HW, C, G, 1e-5, 0, P(y), S())
            assert rc == EINVAL, (B, HW, C, G, rc)
    torch.cuda.synchronize()
    assert bool(torch.isnan(y).all())
