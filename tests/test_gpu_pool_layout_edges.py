"""GPU: the pooling kernels of csrc/wsmg_pool.hip and the layout kernels of csrc/wsmg_layout.hip away from the square, even
3 x 64 x 12 x 12 case on which their older tests stand: H != W in both orientations, odd sizes, channel counts that are no multiple of 8, every branch of the transpose dispatcher,
KH != KW weights.  Inputs, float64 references and derived bars are those of tests/pool_layout_cases.py (checked on the CPU by
tests/test_pool_layout_cases_cpu.py); a bar copied from an older test is quoted at its assert.  Direct C-ABI calls write into buffers
with NaN guards on both sides: only the tensor's own extent may change.

Section, kernels it pins, and the test that held them before:
1. max-pool    maxpool_fwd_kernel<f32 | bf16>, maxpool_bwd_kernel<f32 | bf16>, maxpool_fwd_idx_kernel<bf16>, maxpool_bwd_idx_kernel<bf16>
               — test_gpu_kernels.py::test_small_nhwc_ops / test_small_ops_and_layout_bf16 (12 x 12, through autograd) and
               test_gpu_kernel_instances.py::test_maxpool_bwd_bf16_from_the_input (12 x 12); nothing read the index words
2. avg-pool    avgpool_fwd_kernel / avgpool_bwd_kernel <f32 | bf16> — the same two 12 x 12 tests
   upsampling  upsample_fwd_kernel<f32 | bf16> — the same two; upsample_bwdn_kernel<f32, 4 | bf16, 4 | bf16, 8> at H = 1 / W = 1
               — test_gpu_round6.py::test_upsample_backward_with_eight_channels_per_thread and
               test_gpu_kernel_instances.py::test_upsample_bwd_bf16_twelve_channels hold them at other non-square sizes;
               test_upsample_backward_is_the_same_bits_at_either_channel_width holds the 4- and the 8-channel form to each other
3. transposes  nchw_to_nhwc64_kernel<f32 | bf16>, transpose_kernel<true, f32, f32 | bf16>, transpose_kernel<false, f32 | bf16, f32>
               — test_gpu_kernels.py::test_layout_roundtrip_and_padding / test_small_ops_and_layout_bf16 (27 -> 32 at 48 x 48, 64 at 100 x 100)
4. merge       token_grad_merge_kernel<f32 | bf16> — no test of its own (whole-policy gradients of test_gpu_policy.py / test_gpu_round2.py)
5. weights     weight_relayout_kernel<f32 | bf16>, weight_relayout_multi_kernel<f32 | bf16>, weight_grad_reduce_oihw_kernel,
               weight_grad_to_oihw_kernel — through square-kernel convolutions only (test_gpu_kernels.py::test_conv2d_fwd_bwd,
               test_gpu_round3.py's deterministic weight gradient)

The slab workspace of the (64, 32, 3, 3) weight at nsplit = 8 (147456 floats) is the largest tensor here; the largest activation is the
merge's 5 x 576 x 8."""
import ctypes
import math

import numpy as np
import pytest
import torch

import pool_layout_cases as pc
from oracle import detfill as df
from pool_layout_cases import BF16_EPS, T, nchw, nhwc

pytestmark = pytest.mark.gpu

EINVAL = -1
GUARD = 64                # elements of guard in front of and behind a direct call's output (keeps 16-byte alignment)
DTYPES = [torch.float32, torch.bfloat16]
DT_IDS = ["f32", "bf16"]
GEOM_IDS = [pc.geom_id(g) for g in pc.MAXPOOL_GEOMS]


@pytest.fixture(scope="module")
def ops():
    from wsmgmap import ops as o
    return o


def sfx(dtype):
    return "_bf16" if dtype == torch.bfloat16 else ""


def close(name, got, ref, rtol, atol):
    """|got - ref| <= atol + rtol |ref| elementwise (atol: a number or a float64 tensor of ref's shape); prints the measured error
    beside the bar at the element that comes closest to it."""
    got = got.detach().double().cpu()
    ref = torch.as_tensor(ref).detach().double().cpu()
    assert got.shape == ref.shape, (name, got.shape, ref.shape)
    err = (got - ref).abs()
    bound = (atol + rtol * ref.abs()).expand_as(err) if torch.is_tensor(atol) else atol + rtol * ref.abs()
    over = err - bound
    worst = float(over.max())
    k = int(over.flatten().argmax()) if not math.isnan(worst) else 0
    print(f"{name}: max abs err {float(err.max()):.3e} (ref max {float(ref.abs().max()):.3e}); closest to its bar: err "
          f"{float(err.flatten()[k]):.3e} of {float(bound.flatten()[k]):.3e}")
    assert worst <= 0, f"{name}: max abs err {float(err.max()):.3e} (ref max {float(ref.abs().max()):.3e}), exceeds by {worst:.3e}"


def exact(name, got, want):
    """Bit-for-bit as values (torch.equal; -inf equals -inf, a NaN equals nothing)."""
    got, want = got.detach().cpu(), torch.as_tensor(want).detach().cpu()
    assert got.shape == want.shape, (name, got.shape, want.shape)
    if got.dtype != want.dtype:
        got, want = got.double(), want.double()
    bad = int((got != want).sum())
    print(f"{name}: {bad} of {got.numel()} elements differ")
    assert torch.equal(got, want), f"{name}: {bad} of {got.numel()} elements differ"


class Guarded:
    """A device tensor of `shape` in the middle of a larger buffer filled with NaN (integers: -1)."""

    def __init__(self, shape, dtype):
        self.n = int(np.prod(shape))
        self.fill = float("nan") if dtype.is_floating_point else -1
        self.buf = torch.full((self.n + 2 * GUARD,), self.fill, dtype=dtype, device="cuda")
        self.t = self.buf[GUARD:GUARD + self.n].view(shape)
        assert self.t.data_ptr() % 16 == 0

    def _is_fill(self, v):
        return bool(torch.isnan(v).all()) if self.buf.dtype.is_floating_point else bool((v == self.fill).all())

    def guards_intact(self):
        torch.cuda.synchronize()
        return self._is_fill(self.buf[:GUARD]) and self._is_fill(self.buf[GUARD + self.n:])

    def untouched(self):
        torch.cuda.synchronize()
        return self._is_fill(self.buf)


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


# ============================================================================= 1. MaxPool2d(3, 2, 1)
@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("geom", pc.MAXPOOL_GEOMS, ids=GEOM_IDS)
def test_maxpool_forward_is_exact_and_autograd_matches_float64(ops, geom, dtype):
    """ops.maxpool3x3s2, inference and training route (bf16 training keeps the winning taps): the output equals F.max_pool2d of the
    float64 copy exactly — a max selects, it does not round —, the gradient the float64 gradient."""
    bf16 = dtype == torch.bfloat16
    for kind in pc.MAXPOOL_KINDS:
        c = pc.maxpool_case(geom, kind, bf16)
        name = f"maxpool.{pc.geom_id(geom)}.{kind}.{DT_IDS[bf16]}"
        x = nhwc(c["x"]).to(dtype).cuda()
        y0 = ops.maxpool3x3s2(x)
        assert y0.dtype == dtype
        exact(name + ".y(inference)", nchw(y0), c["y"])
        xg = x.clone().requires_grad_(True)
        y = ops.maxpool3x3s2(xg)
        exact(name + ".y", nchw(y), c["y"])
        y.backward(nhwc(c["gy"]).to(dtype).cuda())
        if bf16:
            close(name + ".dx", nchw(xg.grad.float()), c["dx"], BF16_EPS, 1e-6)      # bar of test_small_ops_and_layout_bf16
        else:
            close(name + ".dx", nchw(xg.grad), c["dx"], 1e-5, 1e-6)                  # bar of test_small_nhwc_ops
        if kind == "ties":      # gradients on the 0.25 grid: a sum of at most four is exact in float32, and in bf16 (|sum| <= 4)
            exact(name + ".dx(exact)", nchw(xg.grad), c["dx"])


@pytest.mark.parametrize("geom", pc.MAXPOOL_GEOMS, ids=GEOM_IDS)
def test_maxpool_index_words_name_the_tap_aten_reports(geom):
    """wsmg_maxpool3x3s2_fwd_idx_bf16 called directly: every byte of every index word is 3 ky + kx of the element
    F.max_pool2d(..., return_indices=True) reports on the float64 copy — at the borders, where the first valid tap is not tap 0, under
    ties and in an all -inf window; wsmg_maxpool3x3s2_bwd_idx_bf16 fed those words gives the float64 gradient."""
    B, H, W, C = geom
    OH, OW = pc.pool_out(H), pc.pool_out(W)
    for kind in pc.MAXPOOL_KINDS:
        c = pc.maxpool_case(geom, kind, True)
        name = f"maxpool_idx.{pc.geom_id(geom)}.{kind}"
        x = nhwc(c["x"]).to(torch.bfloat16).cuda()
        gy = nhwc(c["gy"]).to(torch.bfloat16).cuda()
        y, idx = Guarded((B, OH, OW, C), torch.bfloat16), Guarded((B, OH, OW, C // 4), torch.int32)
        call("wsmg_maxpool3x3s2_fwd_idx_bf16", P(x), P(y.t), P(idx.t), B, H, W, C, OH, OW, S())
        assert y.guards_intact() and idx.guards_intact()
        exact(name + ".y", nchw(y.t), c["y"])
        taps = idx.t.cpu().contiguous().view(torch.uint8).view(B, OH, OW, C)       # byte j of a word: channel 4 i + j
        exact(name + ".taps", taps, c["taps"])
        dx = Guarded((B, H, W, C), torch.bfloat16)
        call("wsmg_maxpool3x3s2_bwd_idx_bf16", P(gy), P(idx.t), P(dx.t), B, H, W, C, OH, OW, S())
        assert dx.guards_intact()
        close(name + ".dx", nchw(dx.t.float()), c["dx"], BF16_EPS, 1e-6)             # bar of test_small_ops_and_layout_bf16
        if kind == "ties":
            exact(name + ".dx(exact)", nchw(dx.t), c["dx"])


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("geom", pc.MAXPOOL_GEOMS, ids=GEOM_IDS)
def test_maxpool_recompute_route_direct(geom, dtype):
    """wsmg_maxpool3x3s2_fwd[_bf16] and wsmg_maxpool3x3s2_bwd[_bf16] (the arg-max recomputed from x) called directly into guarded
    buffers."""
    bf16 = dtype == torch.bfloat16
    B, H, W, C = geom
    OH, OW = pc.pool_out(H), pc.pool_out(W)
    for kind in pc.MAXPOOL_KINDS:
        c = pc.maxpool_case(geom, kind, bf16)
        name = f"maxpool_direct.{pc.geom_id(geom)}.{kind}.{DT_IDS[bf16]}"
        x = nhwc(c["x"]).to(dtype).cuda()
        gy = nhwc(c["gy"]).to(dtype).cuda()
        y, dx = Guarded((B, OH, OW, C), dtype), Guarded((B, H, W, C), dtype)
        call("wsmg_maxpool3x3s2_fwd" + sfx(dtype), P(x), P(y.t), B, H, W, C, OH, OW, S())
        call("wsmg_maxpool3x3s2_bwd" + sfx(dtype), P(gy), P(x), P(dx.t), B, H, W, C, OH, OW, S())
        assert y.guards_intact() and dx.guards_intact()
        exact(name + ".y", nchw(y.t), c["y"])
        if bf16:
            close(name + ".dx", nchw(dx.t.float()), c["dx"], BF16_EPS, 1e-6)         # bar of test_maxpool_bwd_bf16_from_the_input
        else:
            close(name + ".dx", nchw(dx.t), c["dx"], 1e-5, 1e-6)                     # bar of test_small_nhwc_ops
        if kind == "ties":
            exact(name + ".dx(exact)", nchw(dx.t), c["dx"])


def test_maxpool_refuses_an_output_size_that_is_not_its_own():
    """OH / OW other than (H - 1) / 2 + 1 (5 x 8 -> 3 x 4): WSMG_EINVAL from all six entry points, nothing written."""
    B, H, W, C = 2, 5, 8, 12
    n_in = B * H * W * C
    for dtype in DTYPES:
        x = torch.zeros(n_in, dtype=dtype, device="cuda")
        for OH, OW in [(2, 4), (4, 4), (3, 3), (3, 5), (4, 3)]:
            out = Guarded((n_in,), dtype)          # as large as the larger of the two tensors
            idx = Guarded((n_in,), torch.int32)
            assert rc_of("wsmg_maxpool3x3s2_fwd" + sfx(dtype), P(x), P(out.t), B, H, W, C, OH, OW, S()) == EINVAL
            assert rc_of("wsmg_maxpool3x3s2_bwd" + sfx(dtype), P(x), P(x), P(out.t), B, H, W, C, OH, OW, S()) == EINVAL
            if dtype == torch.bfloat16:
                assert rc_of("wsmg_maxpool3x3s2_fwd_idx_bf16", P(x), P(out.t), P(idx.t), B, H, W, C, OH, OW, S()) == EINVAL
                assert rc_of("wsmg_maxpool3x3s2_bwd_idx_bf16", P(x), P(idx.t), P(out.t), B, H, W, C, OH, OW, S()) == EINVAL
            assert out.untouched() and idx.untouched()


# ============================================================================= 2. avg_pool2d(2), bilinear x2
def _smooth(ops, op, fn, geom, dtype, backward):
    bf16 = dtype == torch.bfloat16
    c = pc.smooth_case(op, geom, bf16)
    name = f"{op}.{pc.geom_id(geom)}.{DT_IDS[bf16]}"
    xg = nhwc(c["x"]).to(dtype).cuda().requires_grad_(True)
    y = fn(xg)
    assert y.dtype == dtype
    # bars of test_small_nhwc_ops (float32: 1e-6, 1e-6 / 1e-5, 1e-6) and test_small_ops_and_layout_bf16 (BF16_EPS, 1e-6)
    if bf16:
        close(name + ".y", nchw(y.float()), c["y"], BF16_EPS, 1e-6)
    else:
        close(name + ".y", nchw(y), c["y"], 1e-6, 1e-6)
    if backward:
        y.backward(nhwc(c["gy"]).to(dtype).cuda())
        if bf16:
            close(name + ".dx", nchw(xg.grad.float()), c["dx"], BF16_EPS, 1e-6)
        else:
            close(name + ".dx", nchw(xg.grad), c["dx"], 1e-5, 1e-6)


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("geom", pc.AVGPOOL_GEOMS, ids=pc.geom_id)
def test_avgpool_forward_and_backward(ops, geom, dtype):
    _smooth(ops, "avgpool", ops.avgpool2, geom, dtype, True)


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("geom", pc.AVGPOOL_ODD, ids=pc.geom_id)
def test_avgpool_refuses_odd_sizes(geom, dtype):
    B, H, W, C = geom
    x = torch.zeros(B * H * W * C, dtype=dtype, device="cuda")
    out = Guarded((B * H * W * C,), dtype)
    assert rc_of("wsmg_avgpool2_fwd" + sfx(dtype), P(x), P(out.t), B, H, W, C, S()) == EINVAL
    assert rc_of("wsmg_avgpool2_bwd" + sfx(dtype), P(x), P(out.t), B, H, W, C, S()) == EINVAL
    assert out.untouched()


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("geom", pc.UPSAMPLE_GEOMS, ids=pc.geom_id)
def test_upsample_forward_and_the_one_row_one_column_backward(ops, geom, dtype):
    """Forward at every geometry; backward only where H = 1 or W = 1 (that axis's scale is 0 and every output row / column reads the
    one input row / column) — other non-square backward sizes are held by test_upsample_backward_with_eight_channels_per_thread and
    test_upsample_bwd_bf16_twelve_channels."""
    _smooth(ops, "upsample", ops.upsample2x, geom, dtype, geom[1] == 1 or geom[2] == 1)


# (B, H, W, C, ld_dy), the smallest sizes at which the lists of candidate output rows / columns differ: one source with both scales 0;
# H = 2, where an input row is read by six output rows; a 16-channel slice of a 24-channel gradient read in place; 5 x 4
UPSAMPLE_BWD_WIDTH_GEOMS = [(1, 1, 1, 8, 8), (1, 2, 3, 8, 8), (2, 3, 2, 16, 24), (1, 5, 4, 8, 8)]


@pytest.mark.parametrize("geom", UPSAMPLE_BWD_WIDTH_GEOMS, ids=pc.geom_id)
def test_upsample_backward_is_the_same_bits_at_either_channel_width(geom):
    """wsmg_upsample2x_bwd_ld_bf16 called directly, twice on the same 16-byte-aligned dy: into a 16-byte-aligned dx (8 channels per
    thread) and into a dx that starts 8 bytes into a larger buffer (4 channels per thread).  The two results are the same bits, and
    each is the float64 gradient of F.interpolate(scale_factor=2, mode="bilinear", align_corners=True) under the bf16 bar of this
    module's other upsample tests, so an error the two widths share cannot hide.  Where ld_dy > C the slice is the gradient's LAST C
    channels (its first channel is 16 bytes in, still aligned); the others are never read."""
    B, H, W, C, ld = geom
    n, c0 = B * H * W * C, ld - C
    full = T(df.uniform("pledge.upsample_bwd_width." + pc.geom_id(geom), (B, 2 * H, 2 * W, ld), 2.0)).to(torch.bfloat16)
    dy = full.cuda()
    dyp = ctypes.c_void_p(dy.data_ptr() + 2 * c0)
    assert dyp.value % 16 == 0
    wide = Guarded((B, H, W, C), torch.bfloat16)
    call("wsmg_upsample2x_bwd_ld_bf16", dyp, ld, P(wide.t), B, H, W, C, S())
    room = Guarded((n + 8,), torch.bfloat16)
    narrow = room.t[4:4 + n].view(B, H, W, C)
    assert narrow.data_ptr() % 16 == 8
    call("wsmg_upsample2x_bwd_ld_bf16", dyp, ld, P(narrow), B, H, W, C, S())
    assert wide.guards_intact() and room.guards_intact()
    assert bool(torch.isnan(room.t[:4]).all()) and bool(torch.isnan(room.t[4 + n:]).all())
    name = "upsample_bwd_width." + pc.geom_id(geom)
    exact(name + ".8_against_4", wide.t, narrow)
    xr = torch.zeros(B, C, H, W, dtype=torch.float64, requires_grad=True)
    pc._up(xr).backward(nchw(full[..., c0:].double()))
    close(name + ".dx(8 per thread)", nchw(wide.t.float()), xr.grad, BF16_EPS, 1e-6)
    close(name + ".dx(4 per thread)", nchw(narrow.float()), xr.grad, BF16_EPS, 1e-6)


# ============================================================================= 3. transposes
@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("case", pc.TO_NHWC_CASES, ids=pc.geom_id)
def test_nchw_to_nhwc_direct_is_a_permutation_with_zero_padding(case, dtype):
    """wsmg_nchw_to_nhwc[_bf16] on both sides of the dispatcher (pool_layout_cases.TO_NHWC_64_FORM): bit-exact against permute (bf16:
    torch's round-to-nearest-even), pad channels exactly 0, nothing outside the tensor written."""
    B, Cs, H, W, Cd = case
    x, want = pc.to_nhwc_case(case)
    y, xd = Guarded((B, H, W, Cd), dtype), x.cuda()
    call("wsmg_nchw_to_nhwc" + sfx(dtype), P(xd), P(y.t), B, Cs, H, W, Cd, S())
    assert y.guards_intact()
    name = f"to_nhwc.{pc.geom_id(case)}.{DT_IDS[dtype == torch.bfloat16]}"
    exact(name, y.t, want.to(dtype))
    if Cd > Cs:
        assert float(y.t[..., Cs:].float().abs().max()) == 0.0


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("case", pc.TO_NCHW_CASES, ids=pc.geom_id)
def test_nhwc_to_nchw_direct_is_a_permutation_of_the_leading_channels(case, dtype):
    B, Cs, H, W, Cd = case
    x, want = pc.to_nchw_case(case, dtype == torch.bfloat16)
    y, xd = Guarded((B, Cd, H, W), torch.float32), x.to(dtype).cuda()
    call("wsmg_nhwc_to_nchw" + sfx(dtype), P(xd), P(y.t), B, Cs, H, W, Cd, S())
    assert y.guards_intact()
    exact(f"to_nchw.{pc.geom_id(case)}.{DT_IDS[dtype == torch.bfloat16]}", y.t, want)


def test_layout_wrappers_pass_height_and_width_in_order(ops):
    """ops.to_nhwc / ops.to_nchw at H != W: shapes and values, one case per direction, in both dtypes."""
    case = pc.TO_NHWC_CASES[5]                      # (1, 33, 7, 5, 64)
    B, Cs, H, W, Cd = case
    x, want = pc.to_nhwc_case(case)
    for dtype in DTYPES:
        y = ops.to_nhwc(x.cuda(), Cd, dtype=dtype)
        assert tuple(y.shape) == (B, H, W, Cd) and y.dtype == dtype
        exact(f"ops.to_nhwc.{dtype}", y, want.to(dtype))
    case = pc.TO_NCHW_CASES[0]                      # (2, 32, 3, 11, 27)
    B, Cs, H, W, Cd = case
    for dtype in DTYPES:
        x, want = pc.to_nchw_case(case, dtype == torch.bfloat16)
        z = ops.to_nchw(x.to(dtype).cuda(), Cd)
        assert tuple(z.shape) == (B, Cd, H, W) and z.dtype == torch.float32
        exact(f"ops.to_nchw.{dtype}", z, want)


def test_transposes_refuse_a_batch_beyond_the_grid_limit():
    """B = 65536 does not fit gridDim.z: WSMG_EINVAL from all four entry points before anything is launched (the pointers are tiny)."""
    tiny = torch.zeros(16, device="cuda")
    out = Guarded((16,), torch.float32)
    for name in ("wsmg_nchw_to_nhwc", "wsmg_nchw_to_nhwc_bf16", "wsmg_nhwc_to_nchw", "wsmg_nhwc_to_nchw_bf16"):
        assert rc_of(name, P(tiny), P(out.t), 65536, 1, 1, 1, 1, S()) == EINVAL
        assert rc_of(name, P(tiny), P(out.t), 65536, 64, 2, 2, 64, S()) == EINVAL
    assert out.untouched()
    call("wsmg_nchw_to_nhwc", P(tiny), P(out.t), 1, 1, 1, 1, 1, S())      # the same pointers are accepted at B = 1
    assert out.guards_intact() and float(out.t[0]) == 0.0


# ============================================================================= 4. token-gradient merge
@pytest.mark.parametrize("relu", [0, 1])
@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("case", pc.MERGE_CASES, ids=pc.geom_id)
def test_token_grad_merge_direct(case, dtype, relu):
    """wsmg_token_grad_merge[_bf16], in place on dx: (dx + g[b] / I) * (x > 0 if relu else 1) in float64 under the derived bar of
    pool_layout_cases.merge_bar; masked elements exactly 0; with relu = 0 x is never read (it is all NaN here)."""
    bf16 = dtype == torch.bfloat16
    B, I, C = case
    dx, x, g = pc.merge_inputs(case, bf16)
    ref = pc.merge_ref(dx, x, g, relu)
    buf = Guarded((B, I, C), dtype)
    buf.t.copy_(dx.to(dtype))
    xd = x.to(dtype).cuda() if relu else torch.full((B, I, C), float("nan"), dtype=dtype, device="cuda")
    gd = g.cuda()
    call("wsmg_token_grad_merge" + sfx(dtype), P(buf.t), P(xd), P(gd), B, I, C, relu, S())
    assert buf.guards_intact()
    got = buf.t.float().cpu()
    assert bool(torch.isfinite(got).all())
    close(f"merge.{pc.geom_id(case)}.{DT_IDS[bf16]}.relu{relu}", got, ref, 0.0, pc.merge_bar(dx, g, ref, bf16))
    if relu:
        assert bool((got[x <= 0] == 0).all())
    assert torch.equal(gd.cpu(), g)


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
def test_token_mean_merges_a_parked_gradient_through_its_sink(ops, dtype):
    """The public route: ops.token_mean(x, sink) with the attention's gradient parked in the sink (TokenGradSink.park, as
    _AttnFolded.backward does) and sink.relu set (as the producing convolution does) — against plain torch: tokens = relu(z),
    loss = <mean over tokens, g> + <tokens, parked>, gradient with respect to z."""
    bf16 = dtype == torch.bfloat16
    case = pc.MERGE_CASES[1]                        # (3, 7, 12)
    B, I, C = case
    parked, z, g = pc.merge_inputs(case, bf16)
    tokens = torch.relu(z)
    zr = z.double().requires_grad_(True)
    yr = torch.relu(zr)
    mr = yr.mean(dim=1)
    ((mr * g.double()).sum() + (yr * parked.double()).sum()).backward()
    sink = ops.TokenGradSink()
    sink.relu = True
    xg = tokens.to(dtype).cuda().requires_grad_(True)
    m = ops.token_mean(xg, sink)
    assert m.dtype == torch.float32
    close(f"token_mean.{DT_IDS[bf16]}.mean", m, mr, 1e-6, 1e-6)
    sink.park(parked.to(dtype).cuda())
    m.backward(g.cuda())
    assert sink.masked and sink.dx is None
    ops.TokenGradSink.check_none_pending()
    ref = zr.grad
    close(f"token_mean.{DT_IDS[bf16]}.dx", xg.grad.float(), ref, 0.0, pc.merge_bar(parked, g, ref, bf16))
    assert bool((xg.grad.float().cpu()[z <= 0] == 0).all())


# ============================================================================= 5. weight re-layout, slab reduction
def _relayout_want(case, dtype):
    ohwi, ihwo = pc.relayout_ref(pc.weight_param(case), case[4])
    return T(ohwi).to(dtype), T(ihwo).to(dtype)


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("case", pc.WEIGHT_CASES, ids=pc.geom_id)
def test_weight_relayout_is_the_numpy_permutation(case, dtype):
    """wsmg_weight_relayout[_bf16]: OHWI and IHWO of the OIHW parameter, padded to I_pad with exact zeros; float32 exact, bf16 the
    round-to-nearest-even value; without the IHWO output (null pointer) the OHWI output is the same."""
    O, I, KH, KW, I_pad = case
    w = T(pc.weight_param(case)).cuda()
    want_ohwi, want_ihwo = _relayout_want(case, dtype)
    name = f"relayout.{pc.geom_id(case)}.{DT_IDS[dtype == torch.bfloat16]}"
    ohwi, ihwo = Guarded((O, KH, KW, I_pad), dtype), Guarded((I_pad, KH, KW, O), dtype)
    call("wsmg_weight_relayout" + sfx(dtype), P(w), O, I, KH, KW, I_pad, P(ohwi.t), P(ihwo.t), S())
    assert ohwi.guards_intact() and ihwo.guards_intact()
    exact(name + ".ohwi", ohwi.t, want_ohwi)
    exact(name + ".ihwo", ihwo.t, want_ihwo)
    if I_pad > I:
        assert float(ohwi.t[..., I:].float().abs().max()) == 0.0 and float(ihwo.t[I:].float().abs().max()) == 0.0
    only = Guarded((O, KH, KW, I_pad), dtype)
    call("wsmg_weight_relayout" + sfx(dtype), P(w), O, I, KH, KW, I_pad, P(only.t), None, S())
    assert only.guards_intact()
    exact(name + ".ohwi(alone)", only.t, want_ohwi)
    assert rc_of("wsmg_weight_relayout" + sfx(dtype), P(w), O, I, KH, KW, I - 1, P(only.t), None, S()) == EINVAL


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
def test_weight_relayout_multi_equals_the_single_calls(dtype):
    """wsmg_weight_relayout_multi: the four shapes as one batch in one launch, bit-identical to the single-tensor calls and to numpy."""
    from wsmgmap import _abi
    keep, descs, outs = [], [], []
    for case in pc.WEIGHT_CASES:
        O, I, KH, KW, I_pad = case
        w = T(pc.weight_param(case)).cuda()
        ohwi, ihwo = Guarded((O, KH, KW, I_pad), dtype), Guarded((I_pad, KH, KW, O), dtype)
        s_ohwi, s_ihwo = Guarded((O, KH, KW, I_pad), dtype), Guarded((I_pad, KH, KW, O), dtype)
        call("wsmg_weight_relayout" + sfx(dtype), P(w), O, I, KH, KW, I_pad, P(s_ohwi.t), P(s_ihwo.t), S())
        descs.append(_abi.RelayoutDesc(w.data_ptr(), ohwi.t.data_ptr(), ihwo.t.data_ptr(), O, I, KH, KW, I_pad, 0))
        keep.append(w)
        outs.append((case, ohwi, ihwo, s_ohwi, s_ihwo))
    arr = (_abi.RelayoutDesc * len(descs))(*descs)
    call("wsmg_weight_relayout_multi", ctypes.cast(arr, ctypes.c_void_p), len(descs), int(dtype == torch.bfloat16), S())
    for case, ohwi, ihwo, s_ohwi, s_ihwo in outs:
        assert ohwi.guards_intact() and ihwo.guards_intact()
        want_ohwi, want_ihwo = _relayout_want(case, dtype)
        name = f"relayout_multi.{pc.geom_id(case)}.{DT_IDS[dtype == torch.bfloat16]}"
        exact(name + ".ohwi", ohwi.t, want_ohwi)
        exact(name + ".ihwo", ihwo.t, want_ihwo)
        assert torch.equal(ohwi.t, s_ohwi.t) and torch.equal(ihwo.t, s_ihwo.t)


@pytest.mark.parametrize("nsplit", pc.NSPLITS)
@pytest.mark.parametrize("case", pc.WEIGHT_CASES, ids=pc.geom_id)
def test_weight_grad_reduce_sums_the_slabs_and_never_reads_the_pad(case, nsplit):
    """wsmg_weight_grad_reduce_oihw: the OIHW sum over nsplit OHWI slabs whose pad columns are NaN, against the float64 sum under
    nsplit 2^-24 sum |slab| (pool_layout_cases.reduce_ref); two runs bit-identical."""
    O, I, KH, KW, I_pad = case
    ws_np = pc.slabs(case, nsplit)
    ref, bar = pc.reduce_ref(ws_np, I)
    ws = T(ws_np).cuda()
    runs = []
    for _ in range(2):
        out = Guarded((O, I, KH, KW), torch.float32)
        call("wsmg_weight_grad_reduce_oihw", P(ws), nsplit, O, I, KH, KW, I_pad, P(out.t), S())
        assert out.guards_intact()
        runs.append(out.t.cpu())
    close(f"reduce.{pc.geom_id(case)}.nsplit{nsplit}", runs[0], T(ref), 0.0, T(bar))
    assert torch.equal(runs[0], runs[1])
    assert rc_of("wsmg_weight_grad_reduce_oihw", P(ws), nsplit, O, I, KH, KW, I - 1, P(out.t), S()) == EINVAL


@pytest.mark.parametrize("case", pc.WEIGHT_CASES, ids=pc.geom_id)
def test_weight_grad_to_oihw_is_an_exact_permutation(case):
    """wsmg_weight_grad_to_oihw: [O][KH][KW][I_pad] -> OIHW with the pad columns (NaN here) dropped."""
    O, I, KH, KW, I_pad = case
    dw = pc.slabs(case, 1)[0]
    out, dwd = Guarded((O, I, KH, KW), torch.float32), T(dw).cuda()
    call("wsmg_weight_grad_to_oihw", P(dwd), O, I, KH, KW, I_pad, P(out.t), S())
    assert out.guards_intact()
    exact(f"to_oihw.{pc.geom_id(case)}", out.t, T(np.ascontiguousarray(dw[..., :I].transpose(0, 3, 1, 2))))
