"""Cases, a float64 model and the comparison functions shared by test_cls_tail_cases_cpu.py and test_gpu_cls_tail_edges.py: the fused
classifier tail of csrc/wsmg_cls_tail.hip (BatchNorm with given statistics + ReLU + 1 x 1 convolution + cross-entropy against the
nearest-resized ground truth + AvgPool2d(2), one pass each way, and cls_tail_finish_kernel's sum over samples) at the edges of its
patch loop, of its label arithmetic and of its sample reduction.  Nothing here touches a GPU.

The kernels: one 512-thread workgroup (8 waves) per sample, a wave takes patches of 2 rows x 16 columns, patch p of a sample is row
pair p // (W / 16), column block p % (W / 16), wave w walks p = w, w + 8, ...  The backward leaves a record part[b] of PART = 1120
floats per sample — sum dy [32], sum dy xhat [32], dW [32][32], db [32] — and cls_tail_finish_kernel adds the records in 16 groups
of per = ceil(B / 16) samples, eight at a time and then a tail, in float64.

The model (`model`) is the reference's lines in plain torch with an explicit backward.  `rounding=True` applies the kernel's
documented rounding points (its comments): the 1 x 1 weight to bf16 (w6_frags' pack8), the activation to bf16 (act_frags' pack8),
the stored logits to bf16 before the pool ("the logits as the unfused path stores them"), d logits to bf16 before the bias gradient,
dW and dA ("bf16, as the MFMA consumes it; the bias gradient sums the same rounded values"), dbn to bf16 before BatchNorm's two sums
("what BatchNorm's apply pass will read back").  With rounding off it is torch autograd in float64 (asserted on the CPU).

Two kinds of input per geometry:
* exact (no ground truth): the products y2 scale are quarter-integers in [-2, 2] and y2 itself is a quarter-integer, scale =
  invstd gamma is in {0.5, 1, 2} and the shift beta - mean scale an integer in -1 ... 3 — the (scale, shift) pair, or failing that (invstd, mean), differs
  between any two channels and the scale between channels c and c ^ 1 —, w6 has three entries of +-1 per class at places of its own,
  b6 and d pooled / 4 are small integers.  No rounding point rounds and every float32 partial sum is exact (`_check_exact` asserts
  both on the model alone), so the kernel must give the float64 model's bits.
* ce: the same constants with y2 scale an integer in -3 ... 3, so the logits are exact integers spanning at least +-6; a random
  ground truth, random positive g_rows and a real-valued d pooled of the cross-entropy gradient's size.  sem and pooled stay exact; the loss rows
  and the backward get derived bars (`_ce_bars`)."""
import functools
import zlib

import numpy as np
import torch
import torch.nn.functional as F

CH, WAVES, PART = 32, 8, 2 * 32 + 32 * 32 + 32
FIN_GRP = 16
SEG = {"dbeta": (0, CH), "dgamma": (CH, 2 * CH), "dw6": (2 * CH, 2 * CH + CH * CH), "db6": (2 * CH + CH * CH, PART)}
REDUCED = ("dbeta", "dgamma", "dw6", "db6")
OUT_KEYS = ("sem", "pooled", "dbn", "part", "dgamma", "dbeta", "dw6", "db6")
MUTATIONS = ("drop_last_patch", "swap_sy_sx", "row_bound_from_Wg", "skip_finish_tail", "bn_of_c_xor_1")

# name -> (B, H, W, Hg, Wg, classes)
GEOMETRIES = {
    "one_patch": (1, 2, 16, 3, 5, 27),             # seven idle waves: their zero records enter the wave sum
    "seven_in_a_row": (2, 2, 112, 2, 200, 8),      # fewer patches than waves; classes at a lane-half boundary
    "nine_tall": (3, 18, 16, 7, 4, 5),             # one patch per row pair; wave 0 takes two, the others one
    "nine_3x3": (2, 6, 48, 100, 60, 27),           # three patches per row pair; down-scaling, another ratio per axis
    "fifteen": (2, 10, 48, 25, 100, 17),           # the last wave has one patch fewer
    "seventeen_wide": (1, 2, 272, 2, 272, 32),     # 2 x 8 + 1 patches; identity resize; no padded class
    "one_class": (2, 6, 48, 6, 48, 1),             # a lane half (and most of the other) without a valid class; soft-max over one class
    "four_classes": (2, 6, 48, 6, 48, 4),          # exactly the first accumulator group of lane half 0
}
PATCHES = {"one_patch": 1, "seven_in_a_row": 7, "nine_tall": 9, "nine_3x3": 9, "fifteen": 15, "seventeen_wide": 17, "one_class": 9,
           "four_classes": 9}
# sample counts: one patch per sample, four classes.  name -> (B, per)
BATCHES = {"B16": (16, 1), "B17": (17, 2), "B128": (128, 8), "B130": (130, 9)}
for _n, (_b, _per) in BATCHES.items():
    GEOMETRIES[_n] = (_b, 2, 16, 3, 5, 4)
    PATCHES[_n] = 1
EXACT_CASES = list(GEOMETRIES)
CE_CASES = [n for n in GEOMETRIES if n not in ("B16", "B17", "B128")]


def bf_round(t):
    return t.to(torch.bfloat16).to(t.dtype)


def group_bounds(B):
    """per and [(b0, b1)] of cls_tail_finish_kernel's 16 sample groups (a group with b0 >= b1 is empty)."""
    per = -(-B // FIN_GRP)
    return per, [(g * per, min(g * per + per, B)) for g in range(FIN_GRP)]


def finish_tail_samples(B):
    """Samples that the finish kernel adds in its one-at-a-time tail loop (after the walk of eight)."""
    _, groups = group_bounds(B)
    out = []
    for b0, b1 in groups:
        if b1 > b0:
            out += list(range(b0 + 8 * ((b1 - b0) // 8), b1))
    return out


def _u(tag, n):
    """n float64 values in [0, 1), a function of (tag, index) alone: splitmix64 of crc32(tag) 2^32 + index.  (oracle.detfill's
    i -> i 2654435761 mod 2^32 is an arithmetic progression: elements a fixed distance apart, here the channels a class reads, would
    be functions of each other, and the logits would not reach their range.)"""
    with np.errstate(over="ignore"):
        x = (np.uint64(zlib.crc32(tag.encode())) << np.uint64(32)) + np.arange(n, dtype=np.uint64) + np.uint64(0x9E3779B97F4A7C15)
        x = (x ^ (x >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        x = (x ^ (x >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        x = x ^ (x >> np.uint64(31))
    return (x >> np.uint64(11)).astype(np.float64) / 2.0 ** 53


def _ri(tag, shape, lo, hi):
    """Integers lo ... hi (inclusive), float64."""
    n = int(np.prod(shape))
    return torch.from_numpy(np.floor(_u(tag, n) * (hi - lo + 1)).clip(0, hi - lo).reshape(shape) + lo).double()


def constants():
    """Per-channel BatchNorm constants and the 1 x 1 convolution, float64 (all float32- and bf16-exact)."""
    c = torch.arange(CH)
    scale = torch.tensor([0.5, 1.0, 2.0], dtype=torch.float64)[c % 3]
    shift = torch.tensor([3.0, -1.0, 0.0, 1.0, 2.0], dtype=torch.float64)[(c // 3) % 5]
    invstd = torch.tensor([1.0, 2.0, 0.5], dtype=torch.float64)[c // 15]
    mean = ((c * 7) % 4 - 1).double()
    gamma = scale / invstd
    beta = shift + mean * scale
    w6 = torch.zeros(CH, CH, dtype=torch.float64)
    m = torch.arange(CH)
    w6[m, m], w6[m, (m + 7) % CH], w6[m, (m + 13) % CH] = 1.0, -1.0, 1.0
    b6 = ((m * 5) % 7 - 4).double()
    return dict(scale=scale, shift=shift, mean=mean, invstd=invstd, gamma=gamma, beta=beta, w6=w6, b6=b6)


def labels_of(gt, H, W, mut=None):
    """The kernel's label_of written out: torch's nearest source index min(floorf(dst * (float)in / out), in - 1) in float32, then the
    truncation of the float map.  gt [B, Hg, Wg] -> int64 [B, H, W].  (CPU test: equal to F.interpolate(...).long() without mut.)"""
    B, Hg, Wg = gt.shape
    sy, sx = np.float32(Hg) / np.float32(H), np.float32(Wg) / np.float32(W)
    if mut == "swap_sy_sx":
        sy, sx = sx, sy
    yi = np.floor(np.arange(H, dtype=np.float32) * sy).astype(np.int64)
    xi = np.floor(np.arange(W, dtype=np.float32) * sx).astype(np.int64)
    yi = np.minimum(yi, (Wg if mut == "row_bound_from_Wg" else Hg) - 1)
    xi = np.minimum(xi, Wg - 1)
    yi, xi = np.minimum(yi, Hg - 1), np.minimum(xi, Wg - 1)        # (a mutated index stays inside the map: the model must not fault)
    return gt[:, torch.from_numpy(yi)][:, :, torch.from_numpy(xi)].long()


def _patches(t, H, W):
    """[B, H, W, ...] -> [B, P, 32, ...]: the pixels of each 2 x 16 patch, patches in the kernel's order."""
    B = t.shape[0]
    rest = t.shape[3:]
    v = t.reshape(B, H // 2, 2, W // 16, 16, *rest)
    perm = (0, 1, 3, 2, 4) + tuple(range(5, 5 + len(rest)))
    return v.permute(*perm).reshape(B, (H // 2) * (W // 16), 32, *rest)


def model(inp, rounding, dtype=torch.float64, ce=False, dp=True, mut=None):
    """The operation on inp (y2 [B,H,W,32], mean, invstd, gamma, beta [32], w6 [classes,32], b6 [classes], gt [B,Hg,Wg], g_rows [B],
    dpooled [B,H/2,W/2,32]) in `dtype`.  ce: with the cross-entropy (forward and g_rows); dp: with d pooled.
    -> dict: act, logits, sem, pooled [.., 32] (channels >= classes 0), ce [B] or None, dl, dbn, patch_part [B, P, PART] (each patch's
    share of the record), abs_part [B, PART] (sum of |terms|), part [B, PART], dbeta, dgamma [32], dw6 [32, 32], db6 [32]."""
    f = dtype
    y2 = inp["y2"].to(f)
    B, H, W, _ = y2.shape
    classes = inp["w6"].shape[0]
    mean, invstd, gamma, beta = (inp[k].to(f) for k in ("mean", "invstd", "gamma", "beta"))
    if mut == "bn_of_c_xor_1":
        sw = torch.arange(CH) ^ 1
        mean, invstd, gamma, beta = mean[sw], invstd[sw], gamma[sw], beta[sw]
    scale = invstd * gamma
    shift = beta - mean * scale
    pre = y2 * scale + shift
    act = torch.relu(pre)
    w = torch.zeros(CH, CH, dtype=f)
    w[:classes] = inp["w6"].to(f)
    b = torch.zeros(CH, dtype=f)
    b[:classes] = inp["b6"].to(f)
    if rounding:
        act, w = bf_round(act), bf_round(w)
    logits = act @ w.t() + b
    sem = bf_round(logits) if rounding else logits
    pooled = F.avg_pool2d(sem.permute(0, 3, 1, 2), 2).permute(0, 2, 3, 1)
    dl = torch.zeros(B, H, W, CH, dtype=f)
    ce_rows = pix = None
    if ce:
        gt = inp["gt"]
        if mut in ("swap_sy_sx", "row_bound_from_Wg"):
            target = labels_of(gt, H, W, mut)
        else:
            target = F.interpolate(gt.unsqueeze(1), size=(H, W)).squeeze(1).long()
        lg = logits[..., :classes]
        pix = F.cross_entropy(lg.permute(0, 3, 1, 2), target, reduction="none")
        coef = inp["g_rows"].to(f) / torch.tensor(float(H * W), dtype=f)
        dl[..., :classes] = coef.view(B, 1, 1, 1) * (torch.softmax(lg, dim=-1) - F.one_hot(target, classes).to(f))
    if dp:
        up = inp["dpooled"].to(f).repeat_interleave(2, dim=1).repeat_interleave(2, dim=2)
        dl[..., :classes] += 0.25 * up[..., :classes]
    if rounding:
        dl = bf_round(dl)
    da = dl @ w
    dbn = torch.where(pre > 0, da, torch.zeros_like(da))
    if rounding:
        dbn = bf_round(dbn)
    xhat = (y2 - mean) * invstd
    pdl, pact, pdy, pdyx = (_patches(t, H, W) for t in (dl, act, dbn, dbn * xhat))
    patch_part = torch.cat([pdy.sum(2), pdyx.sum(2), torch.einsum("bpim,bpik->bpmk", pdl, pact).flatten(2), pdl.sum(2)], dim=2)
    abs_part = torch.cat([pdy.abs().sum(2), pdyx.abs().sum(2), torch.einsum("bpim,bpik->bpmk", pdl.abs(), pact.abs()).flatten(2),
                          pdl.abs().sum(2)], dim=2).sum(1)
    keep = patch_part
    if mut == "drop_last_patch":
        keep = patch_part[:, :-1]
        ppr = W // 16
        py, px = (patch_part.shape[1] - 1) // ppr, (patch_part.shape[1] - 1) % ppr
        sem, dbn, pooled = sem.clone(), dbn.clone(), pooled.clone()
        sem[:, 2 * py:2 * py + 2, 16 * px:16 * px + 16] = 0
        dbn[:, 2 * py:2 * py + 2, 16 * px:16 * px + 16] = 0
        pooled[:, py, 8 * px:8 * px + 8] = 0
        if pix is not None:
            pix = pix.clone()
            pix[:, 2 * py:2 * py + 2, 16 * px:16 * px + 16] = 0
    if pix is not None:
        ce_rows = pix.mean([1, 2])
    part = keep.sum(1)
    rows = part
    if mut == "skip_finish_tail":
        gone = finish_tail_samples(B)
        rows = part.clone()
        rows[gone] = 0
    tot = rows.sum(0)
    out = dict(act=act, w=w, logits=logits, sem=sem, pooled=pooled, ce=ce_rows, dl=dl, dbn=dbn, patch_part=patch_part, abs_part=abs_part,
               part=part)
    for k, (a, e) in SEG.items():
        out[k] = tot[a:e].reshape(CH, CH) if k == "dw6" else tot[a:e]
    return out


def outputs_of(m, classes):
    """The model's results in the kernels' output types and shapes (float64 -> bf16 / float32 is exact for an exact case)."""
    bf = torch.bfloat16
    out = dict(sem=m["sem"].to(bf), pooled=m["pooled"].to(bf), dbn=m["dbn"].to(bf), part=m["part"].float(), dgamma=m["dgamma"].float(),
               dbeta=m["dbeta"].float(), dw6=m["dw6"][:classes].float(), db6=m["db6"][:classes].float())
    if m["ce"] is not None:
        out["ce"] = m["ce"].float()
    return out


def _quantum_bits(t):
    """Smallest k with every element of t a multiple of 2^-k."""
    for k in range(0, 13):
        s = t * 2.0 ** k
        if bool((s == s.round()).all()):
            return k
    raise ValueError("not a multiple of 2^-12")


def _check_exact(name, inp, m):
    """On the float64 model alone: no rounding point rounds, every float32 partial sum is exact, the matrix pipe aligns nothing away."""
    for k in ("act", "w", "logits", "pooled", "dl", "dbn"):
        if not torch.equal(bf_round(m[k]), m[k]):
            raise ValueError(f"{name}: {k} is not bf16-representable: the case is not exact")
    for k in ("sem", "pooled", "dbn", "part") + REDUCED:
        if not torch.equal(m[k].float().double(), m[k]):
            raise ValueError(f"{name}: {k} is not float32-representable")
    tot_abs = m["abs_part"].sum(0)
    for k, (a, e) in SEG.items():
        bits = _quantum_bits(m["patch_part"][..., a:e])
        if not float(tot_abs[a:e].max()) < 2.0 ** (24 - bits):
            raise ValueError(f"{name}: sum |terms| of {k} = {float(tot_abs[a:e].max())} reaches 2^(24 - {bits})")
    # the three matrix products: (w6, act) -> logits, (w6, dl) -> dA, (dl, act) -> dW; largest product over the products' quantum
    for x, y in (("w", "act"), ("w", "dl"), ("dl", "act")):
        span = float(m[x].abs().max() * m[y].abs().max()) * 2.0 ** (_quantum_bits(m[x]) + _quantum_bits(m[y]))
        if span > 2.0 ** 10:
            raise ValueError(f"{name}: products of {x} and {y} span 2^{np.log2(span):.1f} > 2^10")


def _inputs(name, kind):
    B, H, W, Hg, Wg, classes = GEOMETRIES[name]
    k = constants()
    tag = f"clstail.{name}.{kind}"
    scale = k["scale"]
    if kind == "exact":
        # y2 scale: quarter-integers in [-2, 2] (half-integers where scale = 2, so that y2 is a quarter-integer)
        q = torch.where(scale == 2.0, 0.5 * _ri(tag + ".y", (B, H, W, CH), -4, 4), 0.25 * _ri(tag + ".y", (B, H, W, CH), -8, 8))
    else:
        q = _ri(tag + ".y", (B, H, W, CH), -3, 3)
    inp = dict(y2=q / scale, mean=k["mean"], invstd=k["invstd"], gamma=k["gamma"], beta=k["beta"], w6=k["w6"][:classes].clone(),
               b6=k["b6"][:classes].clone(), gt=None, g_rows=None)
    if kind == "exact":
        inp["dpooled"] = 4.0 * _ri(tag + ".dp", (B, H // 2, W // 2, CH), -2, 2)          # the padded classes' too: the kernel masks them
    else:
        inp["gt"] = _ri(tag + ".gt", (B, Hg, Wg), 0, classes - 1).float()
        inp["g_rows"] = torch.from_numpy(_u(tag + ".g", B) + 0.5).float().double()
        inp["dpooled"] = bf_round(torch.from_numpy((_u(tag + ".dp", B * (H // 2) * (W // 2) * CH) - 0.5) * 8.0 / (H * W))
                                  .float().reshape(B, H // 2, W // 2, CH)).double()
    for key in ("y2", "dpooled"):
        assert torch.equal(bf_round(inp[key]), inp[key]), key
    return inp


def _ce_bars(name, inp, m64, m32):
    """Bars of the cross-entropy path, from the two models alone.
    ce_rows: 8 max|float32 - float64| of the reference's loss lines over the rows, at least 1e-6 max|ce| (the kernel's __expf and its
    sum order are not torch's float32); the case fails if that exceeds 1e-4 max|ce|.
    Backward, per output: 4 d + n 2^-24 sum|terms| elementwise, d = max|model32 - model64| with rounding on (what flips of the
    rounding points do on this input), n the float32 additions behind an element: H W for the records (and the finished sums, which
    add the records in float64), 32 for dbn (the class axis of dA).  The case fails if the bar of a reduced output exceeds half of
    what some patch contributes to it (at the element where that patch contributes most): a dropped patch cannot hide."""
    B, H, W, _ = inp["y2"].shape
    classes = inp["w6"].shape[0]
    ce64 = m64["ce"]
    ce_max = float(ce64.abs().max())
    ce_bar = max(8.0 * float((m32["ce"].double() - ce64).abs().max()), 1e-6 * ce_max)
    if ce_bar > 1e-4 * ce_max:
        raise ValueError(f"{name}: the loss bar {ce_bar:.3e} exceeds 1e-4 max|ce| = {1e-4 * ce_max:.3e}")
    eps = 2.0 ** -24
    bars = {}
    d = float((m32["dbn"].double() - m64["dbn"]).abs().max())
    bars["dbn"] = 4.0 * d + CH * eps * (m64["dl"].abs() @ m64["w"].abs())
    part_bar = torch.zeros(B, PART, dtype=torch.float64)
    for k, (a, e) in SEG.items():
        dk = float((m32["part"][:, a:e].double() - m64["part"][:, a:e]).abs().max())
        part_bar[:, a:e] = 4.0 * dk + H * W * eps * m64["abs_part"][:, a:e]
        dt = float((m32[k].double() - m64[k]).abs().max())
        tb = 4.0 * dt + H * W * eps * m64["abs_part"][:, a:e].sum(0)
        bars[k] = (tb.reshape(CH, CH) if k == "dw6" else tb)[:classes if k in ("dw6", "db6") else CH]
        # a dropped patch cannot hide
        pp = m64["patch_part"][..., a:e]                                   # [B, P, n]
        big, at = pp.abs().max(dim=2)
        for bb in range(B):
            for p in range(pp.shape[1]):
                if float(big[bb, p]) > 0.0:
                    i = int(at[bb, p])
                    worst = max(float(part_bar[bb, a + i]), float(tb[i]))
                    if worst > 0.5 * float(big[bb, p]):
                        raise ValueError(f"{name}: the bar of {k} ({worst:.3e}) exceeds half of patch {p} of sample {bb} ({float(big[bb, p]):.3e})")
    bars["part"] = part_bar
    return ce_bar, bars


@functools.lru_cache(maxsize=None)
def case(name, kind):
    """kind "exact": dict(inp, geom, want = the outputs every kernel bit must equal, want_nodp = the same without d pooled).
    kind "ce": dict(inp, geom, want (sem, pooled exact; the rest the float64 model with rounding on), ce64, ce_bar, bars)."""
    B, H, W, Hg, Wg, classes = GEOMETRIES[name]
    inp = _inputs(name, kind)
    if kind == "exact":
        m = model(inp, False)
        _check_exact(name, inp, m)
        r = model(inp, True)
        for k in OUT_KEYS:
            if not torch.equal(r[k], m[k]):
                raise ValueError(f"{name}: {k} changes under the rounding points")
        return dict(inp=inp, geom=GEOMETRIES[name], want=outputs_of(m, classes), want_nodp=outputs_of(model(inp, False, dp=False), classes))
    m64, m32 = model(inp, True, ce=True), model(inp, True, torch.float32, ce=True)
    lg = m64["logits"][..., :classes]
    if not (torch.equal(lg, lg.round()) and float(lg.min()) <= -6.0 and float(lg.max()) >= 6.0):
        raise ValueError(f"{name}: the logits are not integers spanning +-6 ({float(lg.min())} ... {float(lg.max())})")
    for k in ("act", "logits", "pooled"):
        if not torch.equal(bf_round(m64[k]), model(inp, False, ce=True)[k]):
            raise ValueError(f"{name}: {k} of the ce case is not exact")
    ce_bar, bars = _ce_bars(name, inp, m64, m32)
    return dict(inp=inp, geom=GEOMETRIES[name], want=outputs_of(m64, classes), ce64=m64["ce"], ce32=m32["ce"], ce_bar=ce_bar, bars=bars)


# ----------------------------------------------------------------------------- the comparisons of the GPU test
def compare_exact(got, want, report=None):
    """-> [failure]: every output of OUT_KEYS equal to the model's, element for element (NaN never equal)."""
    fails = []
    for k in OUT_KEYS:
        g, w = got[k].detach().cpu(), want[k]
        if g.shape != w.shape or g.dtype != w.dtype:
            fails.append(f"{k}: {tuple(g.shape)} {g.dtype} for {tuple(w.shape)} {w.dtype}")
            continue
        bad = ~(g == w)
        n = int(bad.sum())
        if report is not None:
            report.append(f"{k}: {n} of {g.numel()} elements differ (bar: none may)")
        if n:
            err = (g.double() - w.double()).abs()[bad]
            fails.append(f"{k}: {n} of {g.numel()} elements differ, largest by {float(torch.nan_to_num(err, nan=float('inf')).max()):.3e}")
    return fails


def compare_ce(c, got, report=None):
    """-> [failure]: sem and pooled exact; ce against the float64 loss within c["ce_bar"]; dbn, part and the four finished sums
    against the float64 model with rounding on, elementwise within c["bars"]."""
    fails = []
    for k in ("sem", "pooled"):
        g, w = got[k].detach().cpu(), c["want"][k]
        n = int((~(g == w)).sum()) if g.shape == w.shape else g.numel()
        if report is not None:
            report.append(f"{k}: {n} of {g.numel()} elements differ (bar: none may)")
        if n:
            fails.append(f"{k}: {n} of {g.numel()} elements differ")
    g = got["ce"].detach().double().cpu()
    err = float(torch.nan_to_num((g - c["ce64"]).abs(), nan=float("inf")).max())
    if report is not None:
        report.append(f"ce: max abs err {err:.3e}, bar {c['ce_bar']:.3e}, float32 torch {float((c['ce32'].double() - c['ce64']).abs().max()):.3e},"
                      f" max|ce| {float(c['ce64'].abs().max()):.3e}")
    if not err <= c["ce_bar"]:
        fails.append(f"ce: max abs err {err:.3e} over its bar {c['ce_bar']:.3e}")
    for k in ("dbn", "part") + REDUCED:
        g, w, bar = got[k].detach().double().cpu(), c["want"][k].double(), c["bars"][k]
        if g.shape != w.shape:
            fails.append(f"{k}: shape {tuple(g.shape)} for {tuple(w.shape)}")
            continue
        e = torch.nan_to_num((g - w).abs(), nan=float("inf"))
        over = e > bar
        ratio = torch.where(bar > 0, e / bar.clamp_min(1e-300), torch.where(e > 0, torch.full_like(e, float("inf")), torch.zeros_like(e)))
        i = int(torch.argmax(ratio))
        if report is not None:
            report.append(f"{k}: max abs err {float(e.max()):.3e} (bar there {float(bar.flatten()[int(torch.argmax(e))]):.3e}, ref max"
                          f" {float(w.abs().max()):.3e}), worst err / bar {float(ratio.max()):.3f}, {int(over.sum())} of {e.numel()} over")
        if bool(over.any()):
            fails.append(f"{k}: {int(over.sum())} of {e.numel()} elements over their bar, worst err {float(e.flatten()[i]):.3e} against {float(bar.flatten()[i]):.3e}")
    return fails
