"""GPU tests per compiled kernel INSTANTIATION: the entry points of libwsmgmap.so are host-side dispatchers that pick one of several
template instantiations from the shape, and a test proves only the instantiation its shape selects.  Every case here is chosen so
that the dispatcher takes a form that profiles/kernel_coverage_before.txt lists as never launched by the rest of the suite (the
selection is asserted where the ABI exposes it — for the bf16 convolutions the kernel family and tile that wsmg_conv_route_bf16 reports,
the function the launchers switch on; otherwise profiles/kernel_coverage.txt, the trace of the suite with this file, is the proof), and
is compared with a float64 CPU evaluation of the same operator on oracle.detfill inputs.  Tolerances are those of
the neighbouring test of the same kernel family; they are quoted at each assert."""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import conv_route_util as cr
from oracle import detfill as df
from util import T

pytestmark = pytest.mark.gpu

BF16_EPS = 2.0 ** -8     # as tests/test_gpu_kernels.py: round-to-nearest error of one bf16 rounding


@pytest.fixture(scope="module")
def ops():
    from wsmgmap import ops as o
    return o


def nhwc(x):
    return x.permute(0, 2, 3, 1).contiguous()


def nchw(x):
    return x.permute(0, 3, 1, 2).contiguous()


def close(name, got, ref, rtol, atol):
    got = got.detach().double().cpu()
    ref = ref.detach().double().cpu()
    assert got.shape == ref.shape, (name, got.shape, ref.shape)
    err = (got - ref).abs()
    worst = float((err - (atol + rtol * ref.abs())).max())
    print(f"{name}: max abs err {float(err.max()):.3e}, ref max {float(ref.abs().max()):.3e}")
    assert worst <= 0, f"{name}: max abs err {float(err.max()):.3e} (ref max {float(ref.abs().max()):.3e}), exceeds by {worst:.3e}"


# ----------------------------------------------------------------------------- wsmg_rows_gemm_f32: every launch form
ROWS_K = [64, 128, 192, 384, 256, 512, 768, 1024, 1536, 2048]     # 4-wave forms (U = 1, 2, 3, 6), then 16-wave forms (U = 1 .. 8)
SEG3_A = {192: (64, 48, 80), 1024: (496, 272, 256)}               # three operand segments: one NT case per wave count
SEG3_C = {384, 1536}                                              # three output segments: one NN case per wave count


def _rows_bar(K):
    """tests/test_gpu_round5.py holds this kernel to 2e-6 max(1, |ref|) for K up to 1536.  The rounding error of a float32 sum of K
    products is bounded by about K 2^-24 sum|a w|, linear in K, so the one longer reduction (K = 2048, the LSTM core's dxc product)
    gets the same bar scaled by 2048 / 1536; shorter reductions keep the written bar."""
    return 2e-6 * max(1.0, K / 1536.0)


@pytest.mark.parametrize("M", [1, 16, 37, 512])
@pytest.mark.parametrize("nn", [False, True], ids=["NT", "NN"])
@pytest.mark.parametrize("K", ROWS_K)
def test_rows_gemm_every_launch_form_matches_float64(K, nn, M):
    """rows_gemm_f32_kernel<WAVES, U, NN> for every K the library advertises, both weight layouts: bias + ReLU, then the
    ReLU-backward mask + accumulate-into (in place), on rows [r0, r0 + M) of larger tensors whose other rows are NaN before and
    after; operand segments are column slices of a wider tensor (lda > K); two runs are bit-identical."""
    from wsmgmap import _abi, recurrent
    assert _abi.lib().wsmg_rows_gemm_supported(K) == 1
    r0, N = 5, 48
    Bf = r0 + M + 3
    tag = f"rows.{K}.{int(nn)}.{M}"
    a_np = df.uniform(tag + ".a", (Bf, K + 32), 1.0)
    w_np = df.uniform(tag + ".w", (K, N) if nn else (N, K), 0.1)
    b_np = df.uniform(tag + ".b", (N,), 0.5)
    mk_np = df.uniform(tag + ".mask", (Bf, N), 1.0)
    c0_np = df.uniform(tag + ".c0", (Bf, N), 1.0)
    a_wide = T(a_np).cuda()
    widths = SEG3_A[K] if (not nn and K in SEG3_A) else (K,)
    a_segs, col = [], 16                                            # the operand starts at column 16 of the wide tensor
    for wd in widths:
        a_segs.append(a_wide[:, col:col + wd])
        col += wd
    A = a_np[:, 16:16 + K].astype(np.float64)
    w, bias, mask = T(w_np).cuda(), T(b_np).cuda(), T(mk_np).cuda()
    prod = A @ (w_np.astype(np.float64) if nn else w_np.astype(np.float64).T)
    rows = slice(r0, r0 + M)
    three_c = nn and K in SEG3_C

    def outputs(fill):
        full = torch.full((Bf, N), float("nan"), device="cuda")
        if fill is not None:
            full[rows] = T(fill[rows]).cuda()
        if three_c:                                                 # three tensors of 16 columns each
            return [full[:, i * 16:(i + 1) * 16].contiguous() for i in range(3)]
        return [full]

    def check(name, segs, want):
        got = torch.cat(segs, 1)
        d = float((got[rows].double().cpu() - T(want[rows])).abs().max())
        ref_max = float(np.abs(want[rows]).max())
        print(f"{tag} {name}: max abs err {d:.3e}, ref max {ref_max:.3e}")
        assert d <= _rows_bar(K) * max(1.0, ref_max), (name, d, ref_max)
        assert torch.isnan(got[:r0]).all() and torch.isnan(got[r0 + M:]).all(), name + ": rows outside the chunk were written"

    want1 = np.maximum(prod + b_np.astype(np.float64), 0.0)
    c1 = outputs(None)
    recurrent._rg(a_segs, w, nn, c1, r0, M, bias=bias, relu=True)
    check("bias+relu", c1, want1)
    c1b = outputs(None)
    recurrent._rg(a_segs, w, nn, c1b, r0, M, bias=bias, relu=True)
    assert all(torch.equal(x[rows], y[rows]) for x, y in zip(c1, c1b))
    want2 = np.where(mk_np > 0, prod + c0_np.astype(np.float64), 0.0)
    c2 = outputs(c0_np)
    recurrent._rg(a_segs, w, nn, c2, r0, M, mask=mask, cin_segs=c2)    # in place: C = mask > 0 ? C + A W : 0
    check("mask+accumulate", c2, want2)


def test_rows_gemm_refuses_unsupported_k_before_anything_is_queued():
    """Every multiple of 64 up to 2048 that has no launch form is refused with WSMG_EINVAL, and a CHAINED call (wait_count set) leaves
    no kernel behind: the gate launch in front of a chained product used to be queued before the K switch refused.  The counter
    already holds the target, so a gate that did get launched would finish at once and write 0 into the gate word: the word keeps
    its sentinel, and the status word stays 0."""
    from wsmgmap import _abi
    L = _abi.lib()
    refused = [K for K in range(64, 2049, 64) if K not in ROWS_K]
    assert all(L.wsmg_rows_gemm_supported(K) == 0 for K in refused) and {320, 448, 576, 1280, 1792} <= set(refused)
    words = torch.tensor([1, 0x5EED5EED], device="cuda", dtype=torch.int32)       # [arrival counter (= target), gate word]
    M, N = 16, 16
    c = torch.full((M, N), float("nan"), device="cuda")
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    P = lambda t: ctypes.c_void_p(t.data_ptr())   # noqa: E731
    torch.cuda.synchronize()
    assert int(L.wsmg_rnn_status(1)) == 0
    for K in refused:
        a, w = torch.zeros(M, K, device="cuda"), torch.zeros(N, K, device="cuda")
        for chained in (False, True):
            rc = L.wsmg_rows_gemm_f32(P(a), K, K, None, 0, 0, None, 0, 0, P(w), K, 0, None, None, 0, 0,
                                      P(c), N, N, None, 0, 0, None, 0, 0, None, 0, None, 0, None, 0, M,
                                      P(words) if chained else None, 1 if chained else 0, None, 1,
                                      ctypes.c_void_p(words.data_ptr() + 4) if chained else None, st)
            assert rc == -1, (K, chained, rc)                                     # WSMG_EINVAL
    torch.cuda.synchronize()
    assert int(L.wsmg_rnn_status(0)) == 0
    assert words.tolist() == [1, 0x5EED5EED], "a refused chained call launched its gate"
    assert torch.isnan(c).all()


# ----------------------------------------------------------------------------- implicit-GEMM convolutions, both engines
def _conv_case(ops, name, dtype, B, Cin, Cout, k, s, p, H, W):
    """Forward, backward-data and weight gradient of one layer through ops.conv2d against float64 (bf16: of the same bf16-rounded
    operands), inputs and bars exactly as tests/test_gpu_kernels.py test_conv2d_fwd_bwd / test_conv2d_bf16_fwd_bwd."""
    bf16 = dtype == torch.bfloat16
    rnd = (lambda t: t.to(torch.bfloat16)) if bf16 else (lambda t: t)
    x = rnd(T(df.uniform(f"inst.{name}.x", (B, Cin, H, W), 2.0)))
    w = T(df.uniform(f"inst.{name}.w", (Cout, Cin, k, k), float(np.sqrt(12.0 / (Cin * k * k)))))
    b = T(df.uniform(f"inst.{name}.b", (Cout,), 0.5))
    xr, wr, br = x.double().requires_grad_(True), rnd(w).double().requires_grad_(True), b.double().requires_grad_(True)
    yr = F.conv2d(xr, wr, br, stride=s, padding=p)
    gy = rnd(T(df.uniform(f"inst.{name}.gy", tuple(yr.shape), 2.0)))
    yr.backward(gy.double())
    # (no bias gradient: it is a channel reduction of its own, wsmg_channel_sum, which refuses widths such as 96 and 160)
    xg, wg, bg = nhwc(x).cuda().requires_grad_(True), w.cuda().requires_grad_(True), b.cuda()
    y = ops.conv2d(xg, wg, bg, s, p)
    assert y.dtype == dtype and tuple(y.shape) == (B, yr.shape[2], yr.shape[3], Cout)
    y.backward(nhwc(gy).cuda())
    if bf16:     # one bf16 rounding of each output (<= 2^-8 relative) + float32 accumulation order
        close(name + ".y", nchw(y.float()), yr, BF16_EPS, 1e-3)
        close(name + ".dx", nchw(xg.grad.float()), xr.grad, BF16_EPS, 1e-3)
        close(name + ".dw", wg.grad, wr.grad, 1e-4, 3e-4 * float(wr.grad.abs().max()) + 1e-6)
    else:        # f32 MFMA = fmaf chain over K = Cin*k*k terms of magnitude <= ~0.5: error ~ K * 2^-24 * |terms|
        close(name + ".y", nchw(y), yr, 2e-5, 2e-5)
        close(name + ".dx", nchw(xg.grad), xr.grad, 2e-5, 2e-5)
        close(name + ".dw", wg.grad, wr.grad, 2e-5, 2e-4 * float(wr.grad.abs().max()) + 1e-6)


# (name, B, Cin, Cout, k, stride, pad, H, W).  The implicit-GEMM tile is <BN, BK>: BK = 64 when the reduction channels (forward: Cin,
# backward-data: Cout) are a multiple of 64, else 32; BN = 128 when the produced channels (forward: Cout, backward: Cin) are >= 128.
# The pixel counts one below / at / one above the 128-pixel tile run on the 1 x 1 layer only: the handling of the last, partial M tile
# is code the four <BN, BK> forms share, not code of one of them.
IGEMM = [
    ("f6432_b6432_s2_25x31", 2, 32, 96, 3, 2, 1, 25, 31),       # fwd <64,32>, bwd <64,32>; stride 2, odd unequal H, W; Cout = 96: last N tile partial
    ("f12864_b6432_s2_7x13_pad2", 3, 64, 160, 3, 2, 2, 7, 13),  # fwd <128,64>, bwd <64,32>; pad > k / 2; Cout = 160: last 128-wide tile partial
    ("f12832_b6464_k5_pad0", 2, 96, 128, 5, 1, 0, 9, 12),       # fwd <128,32>, bwd <64,64>; pad 0
    ("f6464_b12832_s2_9x15", 2, 128, 96, 3, 2, 1, 9, 15),       # fwd <64,64>, bwd <128,32>; stride 2, the four parity classes all differ in size
    ("f6464_b12864_1x1_m127", 1, 128, 64, 1, 1, 0, 127, 1),     # fwd <64,64>, bwd <128,64>; B OH OW one below the 128-pixel tile
    ("f6464_b12864_1x1_m128", 1, 128, 64, 1, 1, 0, 8, 16),      # ... at it
    ("f6464_b12864_1x1_m129", 1, 128, 64, 1, 1, 0, 3, 43),      # ... one above
    ("f12864_b12864_s2_k4_13x11", 2, 128, 128, 4, 2, 1, 13, 11),  # both <128,64>; even kernel, stride 2, odd sizes
]


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "f32"])
@pytest.mark.parametrize("cfg", IGEMM, ids=[c[0] for c in IGEMM])
def test_implicit_gemm_conv_tiles_match_float64(ops, cfg, dtype):
    name, *geom = cfg
    _conv_case(ops, f"{name}.{'bf16' if dtype == torch.bfloat16 else 'f32'}", dtype, *geom)


def test_conv_fwd_ex_channel_slice_on_the_implicit_gemm_route(ops):
    """wsmg_conv2d_fwd_bf16_ex (y_ld: the output is a channel slice of a wider tensor) on the implicit-GEMM kernel — a 5 x 5 layer, which
    no window kernel takes (asserted on the route): the slice equals float64 within one bf16 rounding, the other channels of the wide
    tensor keep their value."""
    B, Cin, Cout, H, W, Ctot, c_off = 2, 64, 96, 11, 14, 160, 32
    assert cr.route(cr.FWD, cr.dims(B, Cin, Cout, 5, 1, 2, H, W), cr.SLICE)["kind"] == "IGEMM"
    x = T(df.uniform("inst.ex.x", (B, Cin, H, W), 2.0)).to(torch.bfloat16)
    w = T(df.uniform("inst.ex.w", (Cout, Cin, 5, 5), float(np.sqrt(12.0 / (Cin * 25)))))
    b = T(df.uniform("inst.ex.b", (Cout,), 0.5))
    yr = torch.relu(F.conv2d(x.double(), w.to(torch.bfloat16).double(), b.double(), stride=1, padding=2))
    base = torch.full((B, H, W, Ctot), 7.0, device="cuda", dtype=torch.bfloat16)
    y = ops.conv2d(nhwc(x).cuda(), w.cuda(), b.cuda(), 1, 2, relu=True, into=(base, c_off))
    assert y.data_ptr() == base.data_ptr() + 2 * c_off
    close("ex.y", nchw(base[..., c_off:c_off + Cout].float()), yr, BF16_EPS, 1e-3)
    assert bool((base[..., :c_off] == 7.0).all()) and bool((base[..., c_off + Cout:] == 7.0).all())


def test_stem_window_conv_statistics_match_the_implicit_gemm_route():
    """The k8 s2 p3 64 -> 64 stem through wsmg_conv2d_fwd_bf16_stats: conv_win_fwd_kernel flushes its BatchNorm sums once per workgroup run
    (the half-wave exchange on float64), the one statistics path no test held against a second route.  52 x 52 -> 26 x 26 with 5 x 25 tiles: a
    partial tile column (1 of 25) and a partial tile row (1 of 5), B = 3, 8 slabs.  The second route is the implicit-GEMM kernel, which
    wsmg_conv2d_fwd_bf16_ex takes when the output is a channel slice (y_ld != Cout; both routes asserted).  Outputs bit for bit; both routes'
    sums against float64 sums of the returned bf16 output to 1e-6 relative (the bar of tests/test_gpu_round6.py for this quantity)."""
    from wsmgmap import _abi, ops
    B, H, C, OH, nslab = 3, 52, 64, 26, 8
    x = nhwc(T(df.uniform("inst.stem.x", (B, C, H, H), 2.0)).to(torch.bfloat16)).cuda()
    w = T(df.uniform("inst.stem.w", (C, 8, 8, C), float(np.sqrt(12.0 / (C * 64))))).to(torch.bfloat16).cuda()      # OHWI
    bias = T(df.uniform("inst.stem.b", (C,), 0.5)).cuda()
    args = (B, H, H, C, C, 8, 8, 2, 3, OH, OH)
    assert cr.route(cr.FWD, args, cr.STATS)["kind"] == "STEM_WIN" and cr.route(cr.FWD, args, cr.STATS | cr.SLICE)["kind"] == "IGEMM"
    P, st = ops._p, ops._stream
    y_win = torch.empty(B, OH, OH, C, device="cuda", dtype=torch.bfloat16)
    wide = torch.full((B, OH, OH, C + 64), 7.0, device="cuda", dtype=torch.bfloat16)
    s_win = torch.zeros(nslab, 2, C, device="cuda", dtype=torch.float64)
    s_ig = torch.zeros_like(s_win)
    _abi.call("wsmg_conv2d_fwd_bf16_stats", P(x), P(w), P(bias), P(y_win), 2, P(s_win), nslab, *args, st())
    _abi.call("wsmg_conv2d_fwd_bf16_ex", P(x), P(w), P(bias), wide.data_ptr() + 32 * 2, 2, P(s_ig), nslab, C + 64, *args, st())
    torch.cuda.synchronize()
    assert torch.equal(y_win, wide[..., 32:32 + C])
    assert bool((wide[..., :32] == 7).all()) and bool((wide[..., 32 + C:] == 7).all())
    assert float(y_win.float().abs().max()) > 0.5                    # (a real output, not the ReLU's zeros)
    want = torch.stack([y_win.double().sum((0, 1, 2)), (y_win.double() ** 2).sum((0, 1, 2))])
    for name, got in (("window", s_win.sum(0)), ("implicit-GEMM", s_ig.sum(0))):
        rel = float((got - want).abs().max() / want.abs().max())
        print(f"stem statistics, {name} route: max rel err {rel:.3e}")
        assert rel < 1e-6, (name, rel)


def _bwd_data_ex_case(name, B, Cin, Cout, k, s, p, H, W, ca, family, mt=0, by_shape=0):
    """wsmg_conv2d_bwd_data_bf16_ex with relu_y (the gradient is masked with the consumed tensor's ReLU) and dx2 / split_c (it is stored
    as two contiguous channel parts) against the masked float64 input gradient of the same bf16 operands; bar of the bf16 engine.
    family, mt, by_shape: the route the call must report before it is launched."""
    from wsmgmap import _abi, ops
    OH, OW = (H + 2 * p - k) // s + 1, (W + 2 * p - k) // s + 1
    r = cr.route(cr.BWD_DATA, (B, H, W, Cin, Cout, k, k, s, p, OH, OW), cr.RELU_Y | cr.SPLIT)
    assert (r["kind"], r["mt"], r["by_shape"]) == (family, mt, by_shape), (name, r)
    w = T(df.uniform(f"inst.{name}.w", (Cout, Cin, k, k), float(np.sqrt(12.0 / (Cout * k * k))))).to(torch.bfloat16)
    gy = T(df.uniform(f"inst.{name}.gy", (B, Cout, OH, OW), 2.0)).to(torch.bfloat16)
    z = T(df.uniform(f"inst.{name}.z", (B, Cin, H, W), 2.0)).to(torch.bfloat16)         # the tensor whose ReLU masks the gradient
    want = torch.nn.grad.conv2d_input((B, Cin, H, W), w.double(), gy.double(), stride=s, padding=p) * (z.double() > 0)
    w_ihwo = w.permute(1, 2, 3, 0).contiguous().cuda()
    da = torch.full((B, H, W, ca), float("nan"), device="cuda", dtype=torch.bfloat16)
    db = torch.full((B, H, W, Cin - ca), float("nan"), device="cuda", dtype=torch.bfloat16)
    P = ops._p
    gyg, zg = nhwc(gy).cuda(), nhwc(z).cuda()      # (named: a temporary's memory would be reused by the next allocation)
    _abi.call("wsmg_conv2d_bwd_data_bf16_ex", P(gyg), P(w_ihwo), P(da), P(zg), P(db), ca,
              B, H, W, Cin, Cout, k, k, s, p, OH, OW, ops._stream())
    torch.cuda.synchronize()
    close(name + ".da", nchw(da.float()), want[:, :ca], BF16_EPS, 1e-3)
    close(name + ".db", nchw(db.float()), want[:, ca:], BF16_EPS, 1e-3)


def test_conv_bwd_data_ex_mask_and_split_on_the_implicit_gemm_route():
    """The mask / split arguments on the implicit-GEMM kernel, stride 2 with odd unequal sizes (four parity classes of different
    size) — a geometry no window kernel takes (asserted on the route)."""
    _bwd_data_ex_case("bex.igemm", 2, 96, 64, 3, 2, 1, 11, 15, 32, "IGEMM")


# (name, forced tile (1 = by shape), B, H = W, Cin = produced channels N, Cout = reduction channels Kc).  The window kernel takes a tile
# of mt pixels when window_bound(mt, H, W) <= 128 NPW entries (wsmg_win3_window_bound, csrc/wsmg_conv_tile.h), and at least 256 * 256 pixels:
#   48 x 48: window_bound(512) = 737 <= 768, window_bound(256) = 471 <= 512: both tiles fit; B = 29: 66 816 pixels.
#   mixed512_n64: 48 x 48, B = 58: 133 632 pixels, by shape 261 tiles of 512 = one whole round over 256 CUs + 5 -> the remainder runs
#     as 256-pixel tiles (window_bound(256) = 471 <= 512): conv_win3_mixed_kernel<512, 6, 4, 64, 1>.
#   mixed256_n128: the 128-pixel remainder tiles need window_bound(128) <= 256, which 48 x 48 misses (337) and 24 x 24 meets
#     (128 + 12 + 52 + 54 + 1 = 247; window_bound(256) = 385 <= 512); B = 232: the same 133 632 pixels, 522 tiles of 256 = two whole
#     rounds + 10: conv_win3_mixed_kernel<256, 4, 2, 128, 1>.
# The test asserts the family, the tile (the forced one, or 256 / 512 by shape as the case's name says) and by_shape on the queried route;
# the choice between the mixed and the plain launch of a tile stays inside the kernel's file (the arithmetic above).
WIN3_AUX = [
    ("t256_n128", 256, 29, 48, 128, 64), ("t256_n64", 256, 29, 48, 64, 64), ("t256_n32", 256, 29, 48, 32, 32),
    ("t512_n128", 512, 29, 48, 128, 64), ("t512_n64", 512, 29, 48, 64, 64), ("t512_n32", 512, 29, 48, 32, 32),
    ("mixed256_n128", 1, 232, 24, 128, 64), ("mixed512_n64", 1, 58, 48, 64, 128),
]


@pytest.mark.parametrize("cfg", WIN3_AUX, ids=[c[0] for c in WIN3_AUX])
def test_window_conv_mask_and_split_store_forms(cfg):
    """conv_win3_kernel<MT, NPW, NT, 1> / conv_win3_mixed_kernel<..., 1>: the window kernels' store loop with the ReLU mask and the split
    output (AUX = 1), per tile size and channel-tile width.  The suite's concatenation layers are too small for the window route
    (< 65 536 pixels), so only the update at bench size ever ran these forms, against nothing."""
    from wsmgmap import _abi
    name, tile, B, HW, Cin, Cout = cfg
    L = _abi.lib()
    prev = L.wsmg_conv_debug_win3_tile(tile)
    try:
        mt = tile if tile != 1 else int(name[len("mixed"):name.index("_")])
        _bwd_data_ex_case("w3aux." + name, B, Cin, Cout, 3, 1, 1, HW, HW, Cin // 4 if Cin > 32 else 8, "WIN3", mt, int(tile == 1))
    finally:
        L.wsmg_conv_debug_win3_tile(prev)


# ----------------------------------------------------------------------------- generic bf16 weight gradient: every (TC, TU, UPT) form
# conv_wgrad_bf16_kernel<TC, TU, 1, UPT> (csrc/wsmg_conv_bf16.hip, wsmg_conv_wgrad_plan / launch_wgrad_bf16), units = k k Cin / 32:
#   TC = 4 (128 output channels per tile) when Cout % 128 == 0 and units >= 48, then TU = 2;  else TC = 2, and TU = 2 only for
#   Cin == 64 with units >= 128 (an 8 x 8 kernel);  UPT = the largest power of two <= 4 TU that divides Cin / 32.
# None of these geometries is one a window kernel takes (1 x 1, 3 x 3 stride 2, 4 x 4, 5 x 5 stride 1, 7 x 7 stride 1, 8 x 8 stride 1): the
# test asserts that the queried route is the generic kernel with the (TC, TU) of _wgrad_form and the plan call's nsplit.
# (name, (TC, TU, UPT), B, Cin, Cout, k, stride, pad, H, W)
WGRAD = [
    ("t42u8_k3s2_c256", (4, 2, 8), 11, 256, 128, 3, 2, 1, 13, 17),
    ("t42u4_k5_c128", (4, 2, 4), 7, 128, 128, 5, 1, 2, 11, 9),
    ("t42u2_k5_c64", (4, 2, 2), 5, 64, 128, 5, 1, 2, 13, 10),
    ("t42u1_k7_c32", (4, 2, 1), 5, 32, 128, 7, 1, 3, 12, 11),
    ("t42u1_k5_c96", (4, 2, 1), 5, 96, 128, 5, 1, 2, 9, 14),
    ("t22u2_k8_c64", (2, 2, 2), 3, 64, 32, 8, 1, 3, 14, 17),
    ("t21u4_k1_c128", (2, 1, 4), 5, 128, 64, 1, 1, 0, 13, 9),
    ("t21u4_k3s2_c256", (2, 1, 4), 13, 256, 96, 3, 2, 1, 15, 11),
    ("t21u2_k3s2_c64", (2, 1, 2), 3, 64, 96, 3, 2, 1, 25, 31),
    ("t21u1_k1_c32", (2, 1, 1), 5, 32, 32, 1, 1, 0, 21, 13),
    ("t21u1_k3s2_c96", (2, 1, 1), 5, 96, 64, 3, 2, 1, 19, 23),
]
WKP = 32   # pixels per k-step of the weight-gradient kernel (csrc/wsmg_conv_bf16.hip): chunks are multiples of it


def _wgrad_form(Cin, Cout, k):
    units = k * k * (Cin // 32)
    tc = 4 if (Cout % 128 == 0 and units >= 48) else 2
    tu = 2 if (tc == 4 or (Cin == 64 and units >= 128)) else 1
    upt = next((c for c in (8, 4, 2) if c <= 4 * tu and (Cin // 32) % c == 0), 1)
    return tc, tu, upt


@pytest.mark.parametrize("cfg", WGRAD, ids=[c[0] for c in WGRAD])
def test_generic_bf16_weight_gradient_forms(cfg):
    """Atomic form and slab form against the float64 weight gradient of the same bf16 operands (post-ReLU inputs, a gradient that is
    zero on a band of rows), bar as tests/test_gpu_round4.py test_stride2_window_weight_gradients: 2e-5 max|ref|; the slab form is
    bit-identical over repeated launches; the pixel count is not a multiple of the chunk, so the last split is short."""
    from wsmgmap import _abi, ops
    name, form, B, Cin, Cout, k, s, p, H, W = cfg
    assert _wgrad_form(Cin, Cout, k) == form, "the case no longer selects the form it is named for"
    OH, OW = (H + 2 * p - k) // s + 1, (W + 2 * p - k) // s + 1
    x = torch.relu(T(df.uniform(f"inst.wg.{name}.x", (B, H, W, Cin), 4.0))).to(torch.bfloat16)
    dy = T(df.uniform(f"inst.wg.{name}.dy", (B, OH, OW, Cout), 0.4)).clone()
    dy[:, OH // 2] = 0
    dy = dy.to(torch.bfloat16)
    dims = (B, H, W, Cin, Cout, k, k, s, p, OH, OW)
    ns, fl = ctypes.c_int(0), ctypes.c_longlong(0)
    _abi.call("wsmg_conv2d_bwd_weight_bf16_plan", *dims, ctypes.cast(ctypes.byref(ns), ctypes.c_void_p), ctypes.cast(ctypes.byref(fl), ctypes.c_void_p))
    npix = B * OH * OW
    # the generic kernel's plan: nsplit chunks of a multiple of 32 pixels (the window kernels' plans are tile counts of their own)
    chunk = -(-(-(-npix // ns.value)) // WKP) * WKP
    assert ns.value >= 1 and -(-npix // chunk) == ns.value and fl.value == ns.value * Cout * k * k * Cin, (ns.value, npix)
    assert npix % chunk != 0, "choose a pixel count that leaves the last split short"
    r = cr.route(cr.BWD_WEIGHT, dims)
    assert (r["kind"], r["tc"], r["tu"]) == ("WGRAD",) + form[:2] and r["nsplit"] == ns.value, r
    assert r["chunk"] % WKP == 0 and -(-npix // r["chunk"]) == ns.value and npix % r["chunk"] != 0, r      # (the kernel's own chunk)
    want = torch.nn.grad.conv2d_weight(x.double().permute(0, 3, 1, 2), (Cout, Cin, k, k), dy.double().permute(0, 3, 1, 2), stride=s, padding=p)
    scale = float(want.abs().max())
    xg, dyg = x.cuda(), dy.cuda()
    dw = torch.zeros(Cout, k, k, Cin, device="cuda")
    _abi.call("wsmg_conv2d_bwd_weight_bf16", ops._p(xg), ops._p(dyg), ops._p(dw), *dims, ops._stream())
    torch.cuda.synchronize()
    err = float((dw.permute(0, 3, 1, 2).double().cpu() - want).abs().max())
    print(f"{name}: nsplit {ns.value}, atomic form err / scale {err / scale:.3e}")
    assert err <= 2e-5 * scale, err / scale
    slabs = [ops._weight_grad("_bf16", xg, dyg, dims, 0.0, Cin) for _ in range(3)]
    torch.cuda.synchronize()
    assert torch.equal(slabs[0], slabs[1]) and torch.equal(slabs[0], slabs[2])
    err = float((slabs[0].double().cpu() - want).abs().max())
    print(f"{name}: slab form err / scale {err / scale:.3e}")
    assert err <= 2e-5 * scale, err / scale


# ----------------------------------------------------------------------------- k8 stem weight gradient: tile groups that find no tile
# conv_win_wgrad_kernel (csrc/wsmg_conv_win_wgrad.hip): 8 roles x G groups of 5 x 25-pixel tiles, G = min(64, tiles) rounded up to whole
# rounds of 8, one slab per group.  A group beyond the tile count must still write its slab (zeros): nothing else does.
# (name, H = W, tiles, groups)
STEM_FEW = [("b1_100", 100, 20, 24),      # OH = 50: whole blocks, fewer tiles than groups, a tile count that is no multiple of 8
            ("b1_36", 36, 4, 8)]          # OH = 18: every block hangs over the right and bottom edges (the per-pixel dY test)


@pytest.mark.parametrize("cfg", STEM_FEW, ids=[c[0] for c in STEM_FEW])
def test_stem_window_weight_gradient_with_tile_less_groups(cfg):
    """64 -> 64, k8 s2 p3, B = 1 through plan / slabs / reduce on a NaN-FILLED workspace, against the float64 weight gradient of the same
    bf16 operands at the family's bar, 2e-5 max|ref| (test_generic_bf16_weight_gradient_forms); bit-identical over three launches; the
    atomic form at the same bar."""
    from wsmgmap import _abi, ops
    name, H, tiles, groups = cfg
    B, C, k, s, p = 1, 64, 8, 2, 3
    dims = cr.dims(B, C, C, k, s, p, H)
    OH = dims[-1]
    assert B * -(-OH // 5) * -(-OH // 25) == tiles and tiles < groups
    r = cr.route(cr.BWD_WEIGHT, dims)
    assert (r["kind"], r["nsplit"]) == ("WGRAD_STEM_WIN", groups), r
    assert cr.plan_nsplit(dims) == groups
    x = torch.relu(T(df.uniform(f"inst.stemw.{name}.x", (B, H, H, C), 4.0))).to(torch.bfloat16)
    dy = T(df.uniform(f"inst.stemw.{name}.dy", (B, OH, OH, C), 0.4)).clone()
    dy[:, OH // 2] = 0
    dy = dy.to(torch.bfloat16)
    want = torch.nn.grad.conv2d_weight(x.double().permute(0, 3, 1, 2), (C, C, k, k), dy.double().permute(0, 3, 1, 2), stride=s, padding=p)
    scale = float(want.abs().max())
    xg, dyg = x.cuda(), dy.cuda()
    slab = C * k * k * C
    outs = []
    for _ in range(3):
        ws = torch.full((groups * slab,), float("nan"), device="cuda")
        _abi.call("wsmg_conv2d_bwd_weight_bf16_slabs", ops._p(xg), ops._p(dyg), ops._p(ws), groups, groups * slab, *dims, ops._stream())
        dw = torch.full((C, C, k, k), float("nan"), device="cuda")
        _abi.call("wsmg_weight_grad_reduce_oihw", ops._p(ws), groups, C, C, k, k, C, ops._p(dw), ops._stream())
        torch.cuda.synchronize()
        outs.append(dw.cpu())
    left = int(torch.isnan(outs[0]).sum())
    print(f"{name}: {left} of {outs[0].numel()} elements of dW are NaN (slabs left unwritten)")
    assert left == 0
    assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0], outs[2])
    err = float((outs[0].double() - want).abs().max())
    print(f"{name}: slab form err / scale {err / scale:.3e}")
    assert err <= 2e-5 * scale, err / scale
    dwa = torch.zeros(C, k, k, C, device="cuda")
    _abi.call("wsmg_conv2d_bwd_weight_bf16", ops._p(xg), ops._p(dyg), ops._p(dwa), *dims, ops._stream())
    torch.cuda.synchronize()
    err = float((dwa.permute(0, 3, 1, 2).double().cpu() - want).abs().max())
    print(f"{name}: atomic form err / scale {err / scale:.3e}")
    assert err <= 2e-5 * scale, err / scale


# ----------------------------------------------------------------------------- Adam: vector path, scalar tail, unaligned path
ADAM_SIZES = [1, 3, 4, 4095, 4096, 4097, 8193]


def _adam_tensors(tag, wd_tag):
    """50 tensors (two launches of 48 + 2): the sizes above aligned, the same sizes as views offset by ONE float from a 16-byte
    boundary (the kernel's scalar path), the rest small ragged sizes."""
    sizes = ADAM_SIZES + ADAM_SIZES + [5 + 7 * i for i in range(50 - 2 * len(ADAM_SIZES))]
    out = []
    for i, n in enumerate(sizes):
        off = 1 if len(ADAM_SIZES) <= i < 2 * len(ADAM_SIZES) else 0
        vals = [df.uniform(f"adam.{tag}.{wd_tag}.{i}.{what}", (n,), sc) for what, sc in (("p", 2.0), ("g", 0.2), ("m", 0.02))]
        vals.append(np.abs(df.uniform(f"adam.{tag}.{wd_tag}.{i}.v", (n,), 0.002)))
        out.append((off, vals))
    return out


@pytest.mark.parametrize("dev_step", [False, True], ids=["host-step", "dev-step"])
@pytest.mark.parametrize("step", [1, 1000])
@pytest.mark.parametrize("wd", [0.0, 0.01])
def test_adam_kernel_paths_match_float64_torch_adam(wd, step, dev_step):
    """adam_multi_kernel through wsmg_adam_step_multi / _dev: 16-byte vector path, its scalar tail (n % 4 != 0), one-element tensors
    and parameter views one float off a 16-byte boundary, 50 tensors (more than one launch's table), at step 1 and 1000 with the
    moments of that step, against torch.optim.Adam in float64.  Bar as test_adam_multi_tensor_matches_torch_adam: rtol 2e-6,
    atol 1e-7 (one float32 rounding of p is 6e-8 relative)."""
    from wsmgmap import _abi
    from wsmgmap.optim import _AdamDesc
    lr, b1, b2, eps = 2.5e-4, 0.9, 0.999, 1e-8
    tensors = _adam_tensors(step, wd)
    fresh = step == 1                                    # step 1 starts from zero moments, as the optimizer does
    keep, descs, refs = [], (_AdamDesc * len(tensors))(), []
    for d, (off, (p, g, m, v)) in zip(descs, tensors):
        if fresh:
            m, v = np.zeros_like(m), np.zeros_like(v)
        dev = []
        for a in (p, g, m, v):
            buf = torch.zeros(a.size + 8, device="cuda")
            assert buf.data_ptr() % 16 == 0
            view = buf[off:off + a.size]
            view.copy_(T(a))
            dev.append(view)
            keep.append(buf)
        assert dev[0].data_ptr() % 16 == 4 * off
        d.param, d.grad, d.exp_avg, d.exp_avg_sq, d.n = (*[t.data_ptr() for t in dev], p.size)
        rp = torch.nn.Parameter(T(p).double())
        rp.grad = T(g).double()
        refs.append((rp, T(m).double(), T(v).double(), dev))
    opt = torch.optim.Adam([r[0] for r in refs], lr=lr, betas=(b1, b2), eps=eps, weight_decay=wd)
    for rp, m, v, _ in refs:
        opt.state[rp] = {"step": torch.tensor(float(step - 1)), "exp_avg": m.clone(), "exp_avg_sq": v.clone()}
    opt.step()
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    if dev_step:
        sd = torch.full((), float(step), device="cuda", dtype=torch.float32)
        _abi.call("wsmg_adam_step_multi_dev", descs, len(tensors), lr, b1, b2, eps, wd, ctypes.c_void_p(sd.data_ptr()), st)
    else:
        _abi.call("wsmg_adam_step_multi", descs, len(tensors), lr, b1, b2, eps, wd, 1.0 - b1 ** step, 1.0 - b2 ** step, st)
    torch.cuda.synchronize()
    for i, (rp, _, _, dev) in enumerate(refs):
        s = opt.state[rp]
        for name, got, want in (("p", dev[0], rp.detach()), ("m", dev[2], s["exp_avg"]), ("v", dev[3], s["exp_avg_sq"])):
            torch.testing.assert_close(got.double().cpu(), want, rtol=2e-6, atol=1e-7, msg=lambda t: f"tensor {i} {name}: {t}")
    for (off, (p, *_)), buf in zip([t for t in tensors for _ in range(4)], keep):   # nothing outside the views was written
        assert bool((buf[:off] == 0).all()) and bool((buf[off + p.size:] == 0).all())


# ----------------------------------------------------------------------------- bf16 4-element fallbacks, collate of uint8 / float32 sensors
def test_relu_bf16_four_element_kernels(ops):
    """relu_fwd_kernel<bf16> / relu_bwd_kernel<bf16>: the 4-element kernels a bf16 tensor takes when its element count is not a multiple
    of 8 (12 channels x an odd pixel count), against float64; bars as test_small_ops_and_layout_bf16 (ReLU is exact in bf16)."""
    B, C, H, W = 3, 12, 5, 7
    assert (B * C * H * W) % 8 == 4
    x = T(df.uniform("inst.relu4.x", (B, C, H, W), 2.0)).to(torch.bfloat16)
    xr = x.double().requires_grad_(True)
    yr = F.relu(xr)
    gy = T(df.uniform("inst.relu4.gy", tuple(yr.shape), 2.0)).to(torch.bfloat16)
    yr.backward(gy.double())
    xg = nhwc(x).cuda().requires_grad_(True)
    y = ops.relu(xg)
    assert y.dtype == torch.bfloat16
    y.backward(nhwc(gy).cuda())
    close("relu4.y", nchw(y.float()), yr, BF16_EPS, 1e-6)
    close("relu4.dx", nchw(xg.grad.float()), xr.grad, BF16_EPS, 1e-6)


def test_maxpool_bwd_bf16_from_the_input():
    """maxpool_bwd_kernel<bf16> (wsmg_maxpool3x3s2_bwd_bf16: the arg-max recomputed from x; the training route keeps an index and never
    calls it) against the float64 gradient of F.max_pool2d(3, 2, 1) on the same bf16 input; inputs and bar as
    test_small_ops_and_layout_bf16."""
    from wsmgmap import _abi, ops
    B, C, H = 3, 64, 12
    x = torch.relu(T(df.uniform("pool.x", (B, C, H, H), 2.0))).to(torch.bfloat16)
    xr = x.double().requires_grad_(True)
    yr = F.max_pool2d(xr, 3, 2, 1)
    gy = T(df.uniform("pool.gy.maxpool", tuple(yr.shape), 2.0)).to(torch.bfloat16)
    yr.backward(gy.double())
    xg, gyg = nhwc(x).cuda(), nhwc(gy).cuda()
    dx = torch.full((B, H, H, C), float("nan"), device="cuda", dtype=torch.bfloat16)
    _abi.call("wsmg_maxpool3x3s2_bwd_bf16", ops._p(gyg), ops._p(xg), ops._p(dx), B, H, H, C, yr.shape[2], yr.shape[3], ops._stream())
    torch.cuda.synchronize()
    close("maxpool_bwd16.dx", nchw(dx.float()), xr.grad, BF16_EPS, 1e-6)


def test_upsample_bwd_bf16_twelve_channels():
    """upsample_bwdn_kernel<bf16, 4>: 12 channels (not a multiple of 8), the gradient read in place as a channel slice of a 16-wide tensor
    (wsmg_upsample2x_bwd_ld_bf16), against the float64 gradient of the bilinear align_corners upsampling; bar as
    test_small_ops_and_layout_bf16."""
    from wsmgmap import _abi, ops
    B, C, H, W, ld = 2, 12, 7, 9, 16
    xr = torch.zeros(B, C, H, W, dtype=torch.float64, requires_grad=True)
    yr = F.interpolate(xr, scale_factor=2, mode="bilinear", align_corners=True)
    wide = T(df.uniform("inst.up12.gy", (B, 2 * H, 2 * W, ld), 2.0)).to(torch.bfloat16)
    yr.backward(nchw(wide[..., :C]).double())
    wg = wide.cuda()
    dx = torch.full((B, H, W, C), float("nan"), device="cuda", dtype=torch.bfloat16)
    _abi.call("wsmg_upsample2x_bwd_ld_bf16", ops._p(wg), ld, ops._p(dx), B, H, W, C, ops._stream())
    torch.cuda.synchronize()
    close("up12.dx", nchw(dx.float()), xr.grad, BF16_EPS, 1e-6)


@pytest.mark.parametrize("dt", ["uint8", "float32"])
def test_collate_pad_four_element_form_of_uint8_and_float32_sensors(dt):
    """collate_pad_kernel<uint8 | float32, 4> (elems % 4 == 0; the feeder's sensors of these types have odd widths and take the
    one-element form): dst[t][n] = episode n's step t as float32, `pad` past its length, episodes longer than T truncated — exact."""
    from wsmgmap import _abi, ops
    N, Tn, elems = 3, 5, 20
    lengths = [5, 2, 7]
    code = {"uint8": 1, "float32": 3}[dt]
    eps = []
    for n, ln in enumerate(lengths):
        u = df.uniform(f"inst.collate.{dt}.{n}", (ln, elems), 1.0)
        eps.append(T(((u + 0.5) * 255).astype(np.uint8)) if dt == "uint8" else T(u))
    want = torch.full((Tn, N, elems), 1.5, dtype=torch.float64)
    for n, e in enumerate(eps):
        k = min(Tn, e.shape[0])
        want[:k, n] = e[:k].double()
    dev = [e.cuda() for e in eps]
    ptrs = torch.tensor([e.data_ptr() for e in dev], dtype=torch.int64).cuda()
    lens = torch.tensor(lengths, dtype=torch.int32).cuda()
    dst = torch.full((Tn, N, elems), float("nan"), device="cuda")
    _abi.call("wsmg_collate_pad", ops._p(ptrs), ops._p(lens), N, Tn, elems, code, 1.5, ops._p(dst), ops._stream())
    torch.cuda.synchronize()
    assert torch.equal(dst.double().cpu(), want)
