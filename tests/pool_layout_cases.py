"""Inputs, float64 references and derived bars shared by test_pool_layout_cases_cpu.py and test_gpu_pool_layout_edges.py: the
kernels of csrc/wsmg_pool.hip and csrc/wsmg_layout.hip away from the square, even 3 x 64 x 12 x 12 case on which their older tests
stand.  Nothing here touches a GPU.  Inputs are oracle.detfill values under tags of their own; every arithmetic reference is evaluated in float64 by torch / numpy
on the CPU, for bf16 from the bf16-rounded operands; a reference that only moves values (a transpose, a weight re-layout) keeps its
operand's type, because it has no arithmetic to round."""
import functools

import numpy as np
import torch
import torch.nn.functional as F

from oracle import detfill as df

BF16_EPS = 2.0 ** -8      # as tests/test_gpu_kernels.py: the bar of one bf16 rounding
NINF = float("-inf")


def T(a):
    return torch.from_numpy(np.ascontiguousarray(a))


def bf_round(t):
    """float32 values that bf16 holds exactly (torch's round-to-nearest-even)."""
    return t.to(torch.bfloat16).float()


def nhwc(x):
    return x.permute(0, 2, 3, 1).contiguous()


def nchw(x):
    return x.permute(0, 3, 1, 2).contiguous()


def grid(tag, shape):
    """float32 values on {-1, -0.75, ..., 1}: exact in bf16, and sums of a few of them are exact in float32 and in bf16."""
    return T(np.round(df.uniform(tag, shape, 2.0).astype(np.float64) * 4.0) / 4.0).float() + 0.0     # + 0.0: no -0.0


def differs_from_the_square_case(H, W, C):
    """What a geometry must have to see what 12 x 12 x 64 cannot: an odd size, H != W, or channels that are no multiple of 8."""
    return bool(H % 2 or W % 2 or H != W or C % 8)


# ----------------------------------------------------------------------------- 1. MaxPool2d(3, 2, 1)
# (B, H, W, C): odd and even sizes in each axis on its own, both orientations; C = 4 is one thread per pixel, 12 and 20 are no multiple
# of 8.  25 rows is the decoder's map when the ego map has 100 cells.
MAXPOOL_GEOMS = [(2, 1, 1, 4), (1, 2, 3, 4), (1, 3, 2, 8), (2, 5, 8, 12), (1, 25, 9, 8), (3, 7, 12, 20)]
MAXPOOL_KINDS = ["ties", "signed"]


def geom_id(g):
    return "x".join(str(v) for v in g)


def pool_out(n):
    return (n - 1) // 2 + 1


def maxpool_input(geom, kind, bf16):
    """NCHW float32 input of a max-pool case (bf16: rounded to bf16 first).
    "ties":   relu of values on the grid {-1, -0.75, ..., 1}.  Neighbouring detfill values are evenly spaced, so a plain grid of them
              seldom repeats inside a window (a third of the windows tied); the values are therefore stretched (6 u - 2.5, clipped
              to [-1, 1]) before they are put on the grid: 72 % zeros, 22 % ones, 2 % on each level between.  Most windows then hold
              several ones or nothing but zeros (window_stats; asserted by test_pool_layout_cases_cpu.py).
    "signed": signed values, no ReLU; element [0, 0, 0, W - 1] (a corner, so a border window) is -inf, and where the geometry has more
              than one window the whole last window of the last image's last channel is -inf."""
    B, H, W, C = geom
    tag = f"pledge.maxpool.{geom_id(geom)}.{kind}"
    if kind == "ties":
        u = df.uniform(tag, (B, C, H, W), 2.0).astype(np.float64)
        return torch.relu(T(np.round(np.clip(6.0 * u - 2.5, -1.0, 1.0) * 4.0) / 4.0).float()) + 0.0     # + 0.0: no -0.0
    x = T(df.uniform(tag, (B, C, H, W), 2.0))
    if bf16:
        x = bf_round(x)
    x[0, 0, 0, W - 1] = NINF
    OH, OW = pool_out(H), pool_out(W)
    if OH * OW > 1:
        oy, ox = OH - 1, OW - 1
        x[B - 1, C - 1, max(0, 2 * oy - 1):min(H, 2 * oy + 2), max(0, 2 * ox - 1):min(W, 2 * ox + 2)] = NINF
    return x


@functools.lru_cache(maxsize=None)
def maxpool_case(geom, kind, bf16):
    """{x, gy: NCHW float32; y, dx: float64 NCHW (F.max_pool2d on the float64 copy and its gradient); taps: uint8 [B, OH, OW, C],
    3 ky + kx of the input element that F.max_pool2d(..., return_indices=True) reports for every output element}."""
    B, H, W, C = geom
    x = maxpool_input(geom, kind, bf16)
    xr = x.double().requires_grad_(True)
    yr, flat = F.max_pool2d(xr, 3, 2, 1, return_indices=True)
    tag = f"pledge.maxpool.{geom_id(geom)}.{kind}.gy"
    # gradients on the grid beside the tie-heavy input: a sum of at most four of them is exact in float32 (and in bf16)
    gy = grid(tag, tuple(yr.shape)) if kind == "ties" else T(df.uniform(tag, tuple(yr.shape), 2.0))
    if bf16:
        gy = bf_round(gy)
    yr.backward(gy.double())
    OH, OW = yr.shape[2], yr.shape[3]
    oy = torch.arange(OH).view(1, 1, OH, 1)
    ox = torch.arange(OW).view(1, 1, 1, OW)
    taps = 3 * (flat // W - (2 * oy - 1)) + (flat % W - (2 * ox - 1))
    assert int(taps.min()) >= 0 and int(taps.max()) <= 8
    return {"x": x, "gy": gy, "y": yr.detach(), "dx": xr.grad, "taps": nhwc(taps).to(torch.uint8)}


def _windows(x):
    """The 3 x 3 windows of MaxPool2d(3, 2, 1) over NCHW x, spelled out: (holds [B C, 9, L]: the valid taps that equal their window's
    maximum; valid [1, 9, L]: the taps inside the image), L = OH OW windows per plane, taps in (ky, kx) scan order."""
    B, C, H, W = x.shape
    xd = F.pad(x.double(), (1, 1, 1, 1), value=NINF)
    ok = F.pad(torch.ones(1, 1, H, W, dtype=torch.float64), (1, 1, 1, 1), value=0.0)
    win = F.unfold(xd.view(B * C, 1, H + 2, W + 2), 3, stride=2)
    valid = F.unfold(ok, 3, stride=2).bool()
    assert win.dtype == torch.float64 and win.shape[2] == pool_out(H) * pool_out(W)
    best = win.masked_fill(~valid, NINF).max(dim=1, keepdim=True).values
    return (win == best) & valid, valid


def scan_taps(x):
    """uint8 [B, OH, OW, C]: the first maximum of every window in scan order, found by comparing the nine taps — the rule of
    maxpool_fwd_idx_kernel written without F.max_pool2d, to hold maxpool_case's decoding of ATen's flat indices against."""
    B, C, H, W = x.shape
    holds, _ = _windows(x)
    return nhwc(holds.int().argmax(dim=1).view(B, C, pool_out(H), pool_out(W))).to(torch.uint8)


def window_stats(x):
    """Of the windows (one per output element) of MaxPool2d(3, 2, 1) over the NCHW tensor x, in float64:
    tied        the fraction whose maximum is held by two or more of its valid taps;
    all_zero    the fraction whose maximum is 0;
    border      how many have their first valid tap at a position other than tap 0 (they hang over the top or the left edge);
    border_won  how many of those are tied AND won by that first valid tap — where a kernel that numbers taps from the window's first
                valid element instead of from its corner, or lets the last maximum win, reports another tap."""
    holds, valid = _windows(x)
    tied = holds.sum(dim=1) >= 2
    first_valid = valid.int().argmax(dim=1)                                # [1, L]
    winner = holds.int().argmax(dim=1)                                     # the first maximum in scan order, [B C, L]
    border = (first_valid != 0).expand_as(winner)
    return {"tied": float(tied.double().mean()), "all_zero": float((F.max_pool2d(x.double(), 3, 2, 1) == 0).double().mean()),
            "border": int(border.sum()), "border_won": int((border & tied & (winner == first_valid)).sum())}


# ----------------------------------------------------------------------------- 2. avg_pool2d(2) and bilinear x2
AVGPOOL_GEOMS = [(1, 2, 2, 4), (2, 4, 10, 12), (1, 6, 2, 8)]
AVGPOOL_ODD = [(1, 3, 4, 4), (1, 4, 5, 8)]          # refused: odd H, odd W
UPSAMPLE_GEOMS = [(1, 1, 1, 4), (2, 1, 5, 8), (1, 5, 1, 8), (2, 3, 7, 12)]       # H - 1 = 0 / W - 1 = 0: that axis's scale is 0


def _avg(t):
    return F.avg_pool2d(t, 2, 2)


def _up(t):
    return F.interpolate(t, scale_factor=2, mode="bilinear", align_corners=True)


@functools.lru_cache(maxsize=None)
def smooth_case(op, geom, bf16):
    """{x, gy: NCHW float32; y, dx: float64 NCHW} of op = "avgpool" | "upsample"; inputs scaled as in test_small_nhwc_ops."""
    B, H, W, C = geom
    tag = f"pledge.{op}.{geom_id(geom)}"
    x = T(df.uniform(tag + ".x", (B, C, H, W), 2.0))
    if bf16:
        x = bf_round(x)
    xr = x.double().requires_grad_(True)
    yr = {"avgpool": _avg, "upsample": _up}[op](xr)
    gy = T(df.uniform(tag + ".gy", tuple(yr.shape), 2.0))
    if bf16:
        gy = bf_round(gy)
    yr.backward(gy.double())
    return {"x": x, "gy": gy, "y": yr.detach(), "dx": xr.grad}


# ----------------------------------------------------------------------------- 3. transposes
# (B, C_src, H, W, C_dst).  transpose_t takes nchw_to_nhwc64_kernel for C_src == C_dst, C % 64 == 0 and HW % 4 == 0, else the 32 x 33 tile
TO_NHWC_CASES = [
    (2, 64, 2, 2, 64),        # 64-channel form, HW = 4: less than one 64-pixel tile
    (1, 128, 5, 12, 128),     # 64-channel form, HW = 60: a multiple of 4, not of 64; two channel tiles
    (2, 64, 3, 3, 64),        # HW = 9: 64 channels that fall to the tile kernel
    (1, 64, 4, 8, 96),        # padding from a 64-multiple: tile kernel
    (3, 5, 1, 33, 8),         # one pixel past a 32-pixel tile
    (1, 33, 7, 5, 64),        # one channel past a 32-channel tile
]
TO_NHWC_64_FORM = [True, True, False, False, False, False]
TO_NCHW_CASES = [(2, 32, 3, 11, 27), (1, 8, 33, 1, 8), (2, 96, 2, 6, 64)]      # (B, C_src, H, W, C_dst): the first and last are slices


def takes_64_form(C_src, H, W, C_dst):
    return C_src == C_dst and C_src % 64 == 0 and (H * W) % 4 == 0


def to_nhwc_case(case):
    """(x NCHW float32, want [B, H, W, C_dst] float32: x's channels, then exact zeros)."""
    B, Cs, H, W, Cd = case
    x = T(df.uniform("pledge.to_nhwc." + geom_id(case), (B, Cs, H, W), 2.0))
    want = torch.zeros(B, H, W, Cd)
    want[..., :Cs] = x.permute(0, 2, 3, 1)
    return x, want


def to_nchw_case(case, bf16):
    """(x NHWC float32 — bf16: rounded —, want [B, C_dst, H, W] float32: the first C_dst channels)."""
    B, Cs, H, W, Cd = case
    x = T(df.uniform("pledge.to_nchw." + geom_id(case), (B, H, W, Cs), 2.0))
    if bf16:
        x = bf_round(x)
    return x, x.permute(0, 3, 1, 2)[:, :Cd].contiguous()


# ----------------------------------------------------------------------------- 4. token-gradient merge
MERGE_CASES = [(1, 1, 4), (3, 7, 12), (2, 37, 256), (5, 576, 8)]      # (B, I, C); the last is the largest activation of these tests


def merge_inputs(case, bf16):
    """(dx [B, I, C], x [B, I, C], g [B, C] float32): x has exact zeros (about a fifth) and negative values; g differs per batch row
    (its rows are consecutive detfill runs), so the row of another b shows.  bf16: dx and x rounded; g stays float32 as in the ABI."""
    B, I, C = case
    tag = "pledge.merge." + geom_id(case)
    dx = T(df.uniform(tag + ".dx", (B, I, C), 2.0))
    x = T(df.uniform(tag + ".x", (B, I, C), 2.0))
    x = torch.where(x.abs() < 0.1, torch.zeros_like(x), x)
    x.view(-1)[0], x.view(-1)[1] = 0.0, -0.5          # the four-element case has its zero and its negative too
    g =T(df.uniform(tag + ".g", (B, C), 4.0))
    if bf16:
        dx, x = bf_round(dx), bf_round(x)
    return dx, x, g


def merge_ref(dx, x, g, relu):
    """float64: (dx + g[b] / I) * (x > 0 if relu else 1)."""
    I = dx.shape[1]
    out = dx.double() + g.double().unsqueeze(1) / I
    return torch.where(x.double() > 0, out, torch.zeros_like(out)) if relu else out


def merge_bar(dx, g, ref, bf16):
    """Elementwise bar of token_grad_merge_kernel, derived: the kernel is ONE fmaf(g, float32(1 / I), dx).  float32(1 / I) is off by at
    most 2^-24 relative, the fmaf rounds once (2^-24 of a result no larger than |dx| + |g| / I, to first order): together below
    2^-23 (|dx| + |g| / I); the bar is twice that.  bf16 adds the one rounding of the stored result, BF16_EPS |ref|."""
    I = dx.shape[1]
    bar = 2.0 ** -22 * (dx.double().abs() + g.double().abs().unsqueeze(1) / I)
    return bar + BF16_EPS * ref.abs() if bf16 else bar


# ----------------------------------------------------------------------------- 5. weight re-layout and slab reduction
# (O, I, KH, KW, I_pad): KH != KW in both orientations, a square one with no padding, and 2 x 5 with 27 -> 32 channels
WEIGHT_CASES = [(8, 5, 1, 3, 8), (8, 5, 3, 1, 8), (64, 32, 3, 3, 32), (3, 27, 2, 5, 32)]
NSPLITS = [1, 3, 8]


def weight_param(case):
    O, I, KH, KW, _ = case
    return df.uniform("pledge.weight." + geom_id(case), (O, I, KH, KW), 2.0)


def relayout_ref(w, I_pad):
    """numpy float32 (OHWI [O][KH][KW][I_pad], IHWO [I_pad][KH][KW][O]) of the OIHW parameter, pad channels 0."""
    O, I, KH, KW = w.shape
    ohwi = np.zeros((O, KH, KW, I_pad), np.float32)
    ohwi[..., :I] = w.transpose(0, 2, 3, 1)
    ihwo = np.zeros((I_pad, KH, KW, O), np.float32)
    ihwo[:I] = w.transpose(1, 2, 3, 0)
    return ohwi, ihwo


def slabs(case, nsplit):
    """numpy float32 [nsplit][O][KH][KW][I_pad] with the pad columns NaN: a pad column that reaches the result poisons it."""
    O, I, KH, KW, I_pad = case
    ws = df.uniform(f"pledge.slabs.{geom_id(case)}.{nsplit}", (nsplit, O, KH, KW, I_pad), 2.0)
    ws[..., I:] = np.nan
    return ws


def reduce_ref(ws, I):
    """(float64 OIHW sum over the slabs, elementwise bar nsplit 2^-24 sum_z |slab|: the rounding bound of a float32 sum of nsplit terms
    in any fixed order — each of its nsplit - 1 additions rounds by at most 2^-24 of a partial sum no larger than the sum of the
    magnitudes)."""
    v = ws[..., :I].astype(np.float64)
    ref = v.sum(axis=0).transpose(0, 3, 1, 2)
    bar = ws.shape[0] * 2.0 ** -24 * np.abs(v).sum(axis=0).transpose(0, 3, 1, 2)
    return np.ascontiguousarray(ref), np.ascontiguousarray(bar)
