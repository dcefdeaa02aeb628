"""Inputs, float64 references and bars shared by test_norm_cases_cpu.py and test_gpu_norm_edges.py: the kernels of csrc/wsmg_norm.hip
(train / eval BatchNorm with residual and ReLU, the per-channel column sums, the inference GroupNorm) at the edges of their column
reduction and of its finalize pass.  Nothing here touches a GPU.  Inputs are oracle.detfill values under tags of their own; every
reference is the formula written out in float64 (no F.batch_norm, no F.group_norm: test_norm_cases_cpu.py holds the formulas against
those), for bf16 from the bf16-rounded operands.

The reduction (col_reduce_kernel): 256 threads, 4 channels per thread, so a block covers rpi = 1024 / C rows per trip and
nblk = min(1024, ceil(rows / (8 rpi))) blocks walk the rows with a stride of nblk rpi, four rows in flight.  One wave per channel then
adds the nblk partials (reduce_partials): 4 x 64 per trip from 193 partials up, 64 per trip below.  A case is named after the edge it
sits on; `nblk_of` is the arithmetic above, and both test files assert that every case still has the block count of its name.

All inputs are well conditioned: x is uniform of scale 3 plus a per-channel offset of scale 2 (|channel mean| <= 1.2 sigma), gamma is
detfill.positive (0.5 ... 1).  ReLU and the mask: the backward kernels decide `pre > 0` in float32 (from x, or from the stored y), a
float64 reference decides differently on an element whose pre-activation is within rounding of 0.  The case builder therefore sets dy
to exactly 0 wherever |pre| < delta (float32: 1e-3; bf16: 2^-7 (|gamma xhat| + |beta| + |res|), elementwise): the mask cannot matter
there and no element is left out of any comparison.  At most 1 % of dy may be zeroed this way (asserted on the CPU)."""
import functools
import math

import numpy as np
import torch

from oracle import detfill as df
from util import T

BF16_EPS = 2.0 ** -8      # as tests/test_gpu_kernels.py: the bar of one bf16 rounding
MOMENTUM, EPS = 0.1, 1e-5
CHANNELS = [32, 64, 128, 256, 512]          # chan_ok of csrc/wsmg_norm.hip
RED_MAX_BLOCKS = 1024
ZEROED_DY_CAP = 0.01


def bf_round(t):
    """float32 values that bf16 holds exactly (torch's round-to-nearest-even)."""
    return t.to(torch.bfloat16).float()


def rpi_of(C):
    return 1024 // C


def nblk_of(rows, C):
    return min(RED_MAX_BLOCKS, -(-rows // (8 * rpi_of(C))))


def shape_of(rows):
    """(B, H, W) with B H W = rows: pairwise unequal where rows has such a factorisation (the most balanced one), else as unequal as
    its divisors allow (a prime has only 1 x 1 x p).  The kernels see rows alone; the shape only keeps the tests off square images."""
    best, best_key = (1, 1, rows), None
    for b in range(1, int(round(rows ** (1 / 3))) + 2):
        if rows % b:
            continue
        m = rows // b
        for h in range(b, int(math.isqrt(m)) + 1):
            if m % h:
                continue
            w = m // h
            key = (len({b, h, w}), -(w - b))
            if best_key is None or key > best_key:
                best, best_key = (b, h, w), key
    return best


# ----------------------------------------------------------------------------- a. row and block edges of the reduction
def _rows_for_nblk(k, C):
    """A row count with exactly k blocks whose last block is ragged: one row more than a whole trip of the block before the last."""
    per = 8 * rpi_of(C)
    return (k - 1) * per + rpi_of(C) + 1 if k > 1 else rpi_of(C) + 1


def edge_rows(C):
    """{edge name: (rows, nblk the name promises)} of table a for C channels."""
    r = rpi_of(C)
    out = {"rows2": (2, 1), "rpi-1": (r - 1, 1), "rpi": (r, 1), "rpi+1": (r + 1, 1), "8rpi-1": (8 * r - 1, 1), "8rpi+1": (8 * r + 1, 2)}
    for k in (63, 64, 65, 192, 193, 256, 257):
        out[f"nblk{k}"] = (_rows_for_nblk(k, C), k)
    out["cap"] = (8192 * r, 1024)                               # 1024 blocks exactly, eight rows per thread: two whole four-row trips
    out["cap+1"] = (8192 * r + 1, 1024)                         # the cap bites: one block makes a ninth row
    out["beyond"] = (2 * 8192 * r + 3 * r + 1, 1024)            # every thread several trips of the four-in-flight loop and a ragged tail
    return out


SMALL = ["rows2", "rpi-1", "rpi", "rpi+1", "8rpi-1", "8rpi+1"]
TAIL_ONLY = ["nblk63", "nblk64", "nblk65", "nblk192"]           # reduce_partials: the 64-per-trip loop alone
UNROLLED = ["nblk193", "nblk256", "nblk257"]                    # reduce_partials: the 4 x 64 loop (and its remainder)
CAP = ["cap", "cap+1", "beyond"]
WIDE_EDGES = ["nblk65", "nblk193"] + CAP                        # also run at C = 32 and C = 512
# (C, edge): every edge at C = 256 (rpi = 4, the cheapest), the cap rows and nblk 65 / 193 at the narrowest and the widest C too
EDGE_CASES = [(256, e) for e in SMALL + TAIL_ONLY + UNROLLED + CAP] + [(C, e) for C in (32, 512) for e in WIDE_EDGES]
# table f (channel_sum): the small rows, nblk 65 / 193 and the cap rows, at every width
SUM_EDGES = SMALL + ["nblk65", "nblk193"] + CAP

# b. one mid-size non-square shape per C, rows no multiple of 8 rpi, several blocks
MODE_SHAPES = {32: (3, 11, 17), 64: (2, 13, 19), 128: (3, 7, 13), 256: (2, 9, 11), 512: (3, 5, 7)}

# c. (C, Ctot, c0): dy is channels [c0, c0 + C) of a contiguous [B, H, W, Ctot] tensor; Ctot - C and c0 multiples of 8 elements
STRIDED = [(64, 96, 0), (64, 96, 24), (256, 264, 0), (256, 264, 8)]
STRIDED_SHAPE = (3, 7, 13)
MISALIGNED = (64, 96, 4)        # bf16: 8 bytes off a 16-byte boundary, _rows_of must copy

# e. slab counts of wsmg_bn_act_fwd_bf16_pre: one, the two the model uses (8, 64), and both sides of reduce_partials' trips
NSLABS = [1, 8, 64, 65, 192, 193, 257]

# h. GroupNorm
GN_CG = [(64, 64), (64, 1), (96, 32), (40, 8), (256, 32)]
GN_SHAPES = [(1, 1, 1), (3, 1, 5), (2, 7, 9), (1, 16, 16)]


def case_tag(C, rows, bf16, res, relu, seed=""):
    return f"normedge.{C}.{rows}.{'bf16' if bf16 else 'f32'}.{int(res)}{int(relu)}{seed}"


# ----------------------------------------------------------------------------- BatchNorm (+ residual)(+ ReLU), float64
def bn_forward_ref(x, gamma, beta, res, relu, rm, rv, train=True, momentum=MOMENTUM, eps=EPS):
    """x [rows, C] float64.  -> dict(mean, var (biased), invstd, xhat, pre, y, running_mean, running_var).  train: batch statistics,
    running statistics updated with the UNBIASED variance; eval: the running statistics, left as they are."""
    n = x.shape[0]
    if train:
        mean = x.sum(dim=0) / n
        var = ((x - mean) ** 2).sum(dim=0) / n
        new_rm = (1 - momentum) * rm + momentum * mean
        new_rv = (1 - momentum) * rv + momentum * (var * n / (n - 1) if n > 1 else var)
    else:
        mean, var, new_rm, new_rv = rm, rv, rm, rv
    invstd = 1.0 / torch.sqrt(var + eps)
    xhat = (x - mean) * invstd
    pre = xhat * gamma + beta
    if res is not None:
        pre = pre + res
    y = torch.where(pre > 0, pre, torch.zeros_like(pre)) if relu else pre
    return dict(mean=mean, var=var, invstd=invstd, xhat=xhat, pre=pre, y=y, running_mean=new_rm, running_var=new_rv)


def bn_backward_ref(dy, fwd, gamma, relu, has_res):
    """Closed form of the train-mode backward: g = dy [pre > 0]; dbeta = sum g; dgamma = sum g xhat;
    dx = gamma invstd (g - dbeta / n - xhat dgamma / n); dres = g."""
    n = dy.shape[0]
    g = torch.where(fwd["pre"] > 0, dy, torch.zeros_like(dy)) if relu else dy
    dbeta = g.sum(dim=0)
    dgamma = (g * fwd["xhat"]).sum(dim=0)
    dx = gamma * fwd["invstd"] * (g - dbeta / n - fwd["xhat"] * (dgamma / n))
    return dict(dx=dx, dgamma=dgamma, dbeta=dbeta, dres=g if has_res else None, g=g)


def bn_inputs(C, rows, bf16, res, relu, seed=""):
    """float32 tensors (x, res, dy rounded to bf16 for a bf16 case): x, res [rows, C]; gamma, beta, rm, rv [C]; dy before zeroing."""
    tag = case_tag(C, rows, bf16, res, relu, seed)
    x = T(df.uniform(tag + ".x", (rows, C), 3.0)) + T(df.uniform(tag + ".off", (1, C), 2.0))
    r = T(df.uniform(tag + ".r", (rows, C), 2.0)) if res else None
    dy = T(df.uniform(tag + ".gy", (rows, C), 2.0))
    if bf16:
        x, dy = bf_round(x), bf_round(dy)
        r = bf_round(r) if res else None
    return dict(x=x, res=r, dy=dy, gamma=T(df.positive(tag + ".g", (C,))), beta=T(df.uniform(tag + ".b", (C,), 0.5)),
                rm=T(df.uniform(tag + ".rm", (C,), 0.2)), rv=T(df.positive(tag + ".rv", (C,))))


@functools.lru_cache(maxsize=3)
def bn_case(C, rows, bf16, res, relu, seed=""):
    """Inputs (float32, dy already zeroed near pre = 0) and the float64 reference of one train-mode case:
    {x, res, dy, gamma, beta, rm, rv, shape (B, H, W), nblk, zeroed (fraction of dy set to 0), fwd {...}, bwd {...}}."""
    inp = bn_inputs(C, rows, bf16, res, relu, seed)
    d = {k: (v.double() if v is not None else None) for k, v in inp.items()}
    fwd = bn_forward_ref(d["x"], d["gamma"], d["beta"], d["res"], relu, d["rm"], d["rv"])
    zeroed = 0.0
    if relu:
        if bf16:
            delta = 2.0 ** -7 * ((fwd["xhat"] * d["gamma"]).abs() + d["beta"].abs() + (d["res"].abs() if res else 0.0))
        else:
            delta = 1e-3
        near = fwd["pre"].abs() < delta
        inp["dy"] = torch.where(near, torch.zeros_like(inp["dy"]), inp["dy"])
        zeroed = float(near.double().mean())
    bwd = bn_backward_ref(inp["dy"].double(), fwd, d["gamma"], relu, res)
    inp.update(shape=shape_of(rows), nblk=nblk_of(rows, C), zeroed=zeroed, fwd=fwd, bwd=bwd)
    return inp


def bn_bars(ref, bf16):
    """(rtol, atol) per output: the project's own bars of test_bn_act_train / test_bn_act_bf16."""
    gmax, bmax = float(ref["bwd"]["dgamma"].abs().max()), float(ref["bwd"]["dbeta"].abs().max())
    bars = {"running_mean": (1e-6, 1e-6), "running_var": (1e-5, 1e-6), "dgamma": (1e-4, 1e-4 * gmax), "dbeta": (1e-4, 1e-4 * bmax)}
    if bf16:
        bars.update(y=(BF16_EPS, 1e-6), dx=(BF16_EPS, 2e-3 * float(ref["bwd"]["dx"].abs().max())))
    else:
        bars.update(y=(1e-5, 1e-5), dx=(1e-4, 2e-5))
    return bars


def bn_float32_model(c, bf16, res, relu):
    """The kernels' arithmetic on the CPU: float32 elementwise expressions in their order (bn_apply_kernel, bn_bwd_apply_kernel), the
    statistics and the two backward sums from float64 accumulation rounded once, bf16 outputs rounded once.  test_norm_cases_cpu.py
    holds it inside every bar: a bar that plain float32 cannot meet would say nothing about a kernel."""
    f = torch.float32
    x, dy, gm, bt = c["x"], c["dy"], c["gamma"], c["beta"]
    mu, inv = c["fwd"]["mean"].to(f), c["fwd"]["invstd"].to(f)
    xh = (x - mu) * inv
    pre = xh * gm + bt
    if res:
        pre = pre + c["res"]
    y = torch.relu(pre) if relu else pre
    if bf16:
        y = bf_round(y)
    g = torch.where((y if res else pre) > 0, dy, torch.zeros_like(dy)) if relu else dy
    db = g.double().sum(dim=0).to(f)
    dg = (g.double() * xh.double()).sum(dim=0).to(f)
    inv_n = torch.tensor(1.0, dtype=f) / torch.tensor(float(x.shape[0]), dtype=f)
    dx = (gm * inv) * (g - db * inv_n - xh * (dg * inv_n))
    return dict(y=y, dx=bf_round(dx) if bf16 else dx, dgamma=dg, dbeta=db, dres=g if res else None)


def slab_split(x, nslab, tag):
    """float64 [nslab, 2, C]: sum x and sum x^2 of x [rows, C] (float64) over nslab uneven runs of rows — the cut points are squares of
    detfill values, so the runs differ in length and, where nslab comes near rows or passes it, many are empty; from 4 slabs up slab 2
    is forced empty.  The slabs add up to the sums of all rows."""
    rows, C = x.shape
    cuts = np.sort(np.floor(rows * (df._u(tag + ".cuts", max(nslab - 1, 1)) + 0.5) ** 2).astype(np.int64))[:nslab - 1]
    if nslab >= 4:
        cuts[2] = cuts[1]
    edges = [0] + [int(c) for c in cuts] + [rows]
    out = torch.zeros(nslab, 2, C, dtype=torch.float64)
    for k in range(nslab):
        part = x[edges[k]:edges[k + 1]]
        out[k, 0], out[k, 1] = part.sum(dim=0), (part * part).sum(dim=0)
    return out


# ----------------------------------------------------------------------------- channel sums
def sum_input(C, rows, bf16, kind):
    """[rows, C] float32.  "plain": detfill of scale 3 plus the per-channel offset; "zero_col": the same with column 5 all zeros;
    "pm1": +1 / -1 alternating by row with the sign flipped on odd channels (exact sums: 0, or +-1 for an odd row count)."""
    tag = f"normedge.sum.{C}.{rows}.{kind}"
    if kind == "pm1":
        s = 1.0 - 2.0 * ((torch.arange(rows).view(-1, 1) + torch.arange(C).view(1, -1)) % 2).float()
        return s.contiguous()
    x = T(df.uniform(tag + ".x", (rows, C), 3.0)) + T(df.uniform(tag + ".off", (1, C), 2.0))
    if kind == "zero_col":
        x[:, 5] = 0.0
    return bf_round(x) if bf16 else x


def sum_bar(ref):
    """One float32 rounding of the result: 2^-23 relative, with 2^-23 max|sum| as the absolute floor."""
    return torch.clamp(2.0 ** -23 * ref.abs(), min=2.0 ** -23 * float(ref.abs().max()))


# ----------------------------------------------------------------------------- GroupNorm, float64
def gn_ref(x, gamma, beta, G, eps, res, relu):
    """x [B, H, W, C] float64: statistics per (sample, group) over H W (C / G) elements, biased variance, eps under the root.
    -> dict(y, mean [B, G], var [B, G], xhat)."""
    B, H, W, C = x.shape
    Cg = C // G
    v = x.reshape(B, H * W, G, Cg)
    n = H * W * Cg
    mean = v.sum(dim=(1, 3), keepdim=True) / n
    var = ((v - mean) ** 2).sum(dim=(1, 3), keepdim=True) / n
    xhat = ((v - mean) / torch.sqrt(var + eps)).reshape(B, H, W, C)
    y = xhat * gamma + beta
    if res is not None:
        y = y + res
    if relu:
        y = torch.where(y > 0, y, torch.zeros_like(y))
    return dict(y=y, mean=mean.reshape(B, G), var=var.reshape(B, G), xhat=xhat)


def gn_inputs(C, G, shape, bf16, res):
    B, H, W = shape
    tag = f"normedge.gn.{C}.{G}.{B}x{H}x{W}.{'bf16' if bf16 else 'f32'}"
    x = T(df.uniform(tag + ".x", (B, H, W, C), 3.0)) + T(df.uniform(tag + ".off", (1, 1, 1, C), 2.0))
    if bf16:
        x = bf_round(x)
    r = bf_round(T(df.uniform(tag + ".r", (B, H, W, C), 2.0))) if res else None      # the residual is bf16 in both forms
    return dict(x=x, res=r, gamma=T(df.positive(tag + ".g", (C,))), beta=T(df.uniform(tag + ".b", (C,), 0.5)))


GN_STAGE_BAR = 2e-2       # tests/test_gpu_round2.py's stage test: the whole allowance beside which the bar below must stay


def gn_bar(inp, ref, G, eps):
    """Elementwise bar of group_norm_nhwc_bf16_kernel: one bf16 rounding of the float64 result, BF16_EPS |ref|, plus what its float32
    statistics and float32 normalisation can be off by, derived:
    * every thread adds its m = ceil(n / 256) elements (and, by fmaf, their squares) in float32: each addition rounds by at most 2^-24
      of a partial sum no larger than the sum of the magnitudes, so mean is off by at most d_mean = m 2^-24 mean|x| and E[x^2] by
      m 2^-24 E[x^2]; var = E[x^2] - mean^2 (float64 from there on) by d_var <= 3 m 2^-24 E[x^2] (|mean| d_mean <= E[x^2] m 2^-24);
      the casts of mean and 1 / sqrt(var + eps) to float32 add 2^-24 relative each;
    * xhat = (x - mean) invstd in float32: |d xhat| <= invstd (d_mean + 2^-23 (|x| + |mean|)) + |xhat| (d_var / (2 (var + eps)) + 2^-22);
    * y = xhat gamma + beta (+ res): three more roundings of values no larger than |gamma xhat| + |beta| + |res|.
    The bar is twice the sum.  A group of ONE element has x - mean = 0 exactly and the result beta (+ res) whatever invstd is; the
    terms above are then 0 but for the last.  test_norm_cases_cpu.py asserts that the float32 part never exceeds GN_STAGE_BAR."""
    x, g, b = inp["x"].double(), inp["gamma"].double(), inp["beta"].double()
    B, H, W, C = x.shape
    Cg = C // G
    n = H * W * Cg
    m = -(-n // 256)
    v = x.reshape(B, H * W, G, Cg)
    mean_abs = v.abs().sum(dim=(1, 3), keepdim=True) / n
    ex2 = (v * v).sum(dim=(1, 3), keepdim=True) / n
    mean = ref["mean"].reshape(B, 1, G, 1)
    var = ref["var"].reshape(B, 1, G, 1)
    invstd = 1.0 / torch.sqrt(var + eps)
    d_mean = m * 2.0 ** -24 * mean_abs
    d_var = 3 * m * 2.0 ** -24 * ex2
    xhat = ref["xhat"].reshape(B, H * W, G, Cg).abs()
    d_xhat = (invstd * (d_mean + 2.0 ** -23 * (v.abs() + mean.abs())) + xhat * (d_var / (2 * (var + eps)) + 2.0 ** -22)).reshape(B, H, W, C)
    mag = ref["xhat"].abs() * g + b.abs() + (inp["res"].double().abs() if inp["res"] is not None else 0.0)
    f32_part = 2.0 * (g * d_xhat + 3 * 2.0 ** -24 * mag)
    return BF16_EPS * ref["y"].abs() + f32_part, f32_part
