"""wsmgmap.ops.heads — losses and heads as fused launches: NHWC cross-entropy, the contrastive monitor's KL, the classifier tail, the
update path's heads / auxiliary-loss reduction / DAgger loss, and the rollout's one-launch dense layers and heads.
"""
import ctypes

import torch

from .. import _abi
from ..debug import sw
from .core import _p, _raw_stream, _stream, _req, _f32, _sfx, _workspace, _rows_of, _conv_out, _launch, _zeros_f32, _prelaid, _join_side_at_end, TokenGradSink


# ----------------------------------------------------------------------------- persistent masked GRU
class _CrossEntropyNHWC(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits, target, classes):
        _req(logits, target)
        if logits.shape[-1] != 32 or target.dtype != torch.int64:
            raise _abi.WsmgError("cross_entropy_nhwc: logits [..., 32] (padded classes), target int64")
        rows = logits.numel() // 32
        loss = torch.empty(target.shape, device=logits.device, dtype=torch.float32)
        _abi.call("wsmg_ce_nhwc_fwd" + _sfx(logits), _p(logits), _p(target), rows, int(classes), _p(loss), _stream())
        ctx.save_for_backward(logits, target)
        ctx.classes = int(classes)
        return loss

    @staticmethod
    def backward(ctx, gloss):
        logits, target = ctx.saved_tensors
        g = gloss.contiguous().float()
        d = torch.empty_like(logits)
        _abi.call("wsmg_ce_nhwc_bwd" + _sfx(logits), _p(logits), _p(target), _p(g), logits.numel() // 32, ctx.classes, _p(d), _stream())
        return d, None, None


def cross_entropy_nhwc(logits, target, classes):
    """F.cross_entropy(logits_nchw[:, :classes], target, reduction='none') computed from NHWC logits [..., 32].
    The contract for a label outside [0, classes), shared with `cls_tail`: `F.cross_entropy` of the reference faults on it; here
    that row's loss is NaN and so is its whole 32-wide gradient row — loud, not a finite wrong number.  The int64 label itself is
    compared, not a truncation of it.  -100 is NOT treated as `ignore_index`: the reference never produces it, and it poisons
    its row like any other out-of-range label.  Rows with a label in range are unaffected; their padded channels get gradient 0."""
    return _CrossEntropyNHWC.apply(logits.contiguous(), target.contiguous(), classes)


class _PathKL(torch.autograd.Function):
    """kl[b] of the contrastive monitor (policy.py:72-82 of the reference) in one launch per direction (csrc/wsmg_loss.hip)."""

    @staticmethod
    def forward(ctx, dis, att, size, tau):
        _req(dis, att)
        _f32(dis, att)
        B, H, W = dis.shape
        if att.shape != (B, size * size):
            raise _abi.WsmgError(f"path_kl: attention {tuple(att.shape)} does not match {B} x {size}^2")
        lo, hi = torch.aminmax(dis)      # batch-global normalisation, as the reference does (dis.max(), dis.min())
        target = torch.empty(B, size * size, device=dis.device, dtype=torch.float32)
        kl = torch.empty(B, device=dis.device, dtype=torch.float32)
        _abi.call("wsmg_path_kl_fwd", _p(dis), _p(lo), _p(hi), _p(att), B, H, W, size, float(tau), _p(target), _p(kl), _stream())
        ctx.save_for_backward(target, att)
        return kl

    @staticmethod
    def backward(ctx, gkl):
        target, att = ctx.saved_tensors
        B, n = target.shape
        datt = torch.empty_like(att)
        _abi.call("wsmg_path_kl_bwd", _p(gkl.contiguous().float()), _p(target), _p(att), B, n, _p(datt), _stream())
        return None, datt, None, None


def path_kl(dis, att, size, tau):
    """F.kl_div(log(att), softmax(area_resize((hi - dis) / (hi - lo), size) / tau), reduction='none').mean(-1) with lo, hi the
    batch-global extremes of dis [B, H, W]; att [B, size*size] (a probability row); -> [B]."""
    return _PathKL.apply(dis.contiguous(), att.contiguous(), int(size), float(tau))


# ----------------------------------------------------------------------------- the semantic classifier's tail, fused
class _ClsTail(torch.autograd.Function):
    """BatchNorm2d(32, batch statistics) + ReLU + Conv2d(32, classes, 1) + { per-sample cross-entropy against the nearest-resized
    ground truth, AvgPool2d(2), the logits } in one pass per direction over the 32-channel activation (csrc/wsmg_cls_tail.hip):
    mg_map_policy.py:78-86,93-96,195 and policy.py:61-66 of the reference.  bf16 training mode only."""

    @staticmethod
    def forward(ctx, y2, stats, gamma, beta, running_mean, running_var, momentum, eps, w6, b6, gt):
        _req(y2, stats, gamma, beta, running_mean, running_var, w6, b6, gt)
        _f32(gamma, beta, running_mean, running_var, w6, b6, gt)
        B, H, W, C = y2.shape
        classes = w6.shape[0]
        if y2.dtype != torch.bfloat16 or C != 32 or w6.numel() != classes * 32 or b6.numel() != classes or stats.dtype != torch.float64:
            raise _abi.WsmgError("cls_tail: bf16 [B,H,W,32] activation, [classes,32,1,1] weight, float64 statistics slabs")
        if gt is not None and (gt.dim() != 3 or gt.shape[0] != B):
            raise _abi.WsmgError("cls_tail: ground truth [B, Hg, Wg] float32")
        dev = y2.device
        mean, invstd = torch.empty(32, device=dev), torch.empty(32, device=dev)
        _abi.call("wsmg_bn_stats_finalize", _p(stats), stats.shape[0], 32, B * H * W, float(momentum), float(eps), _p(running_mean),
                  _p(running_var), _p(mean), _p(invstd), _stream())
        torch.autograd.graph.increment_version([running_mean, running_var])
        sem = torch.empty(B, H, W, 32, device=dev, dtype=torch.bfloat16)
        pooled = torch.empty(B, H // 2, W // 2, 32, device=dev, dtype=torch.bfloat16)
        ce = torch.empty(B, device=dev, dtype=torch.float32) if gt is not None else None
        Hg, Wg = (gt.shape[1], gt.shape[2]) if gt is not None else (0, 0)
        _abi.call("wsmg_cls_tail_fwd_bf16", _p(y2), _p(gamma), _p(beta), _p(mean), _p(invstd), _p(w6), _p(b6), classes, _p(gt), Hg, Wg,
                  B, H, W, _p(sem), _p(pooled), _p(ce), _stream())
        ctx.save_for_backward(y2, gamma, beta, mean, invstd, w6, b6, gt)
        ctx.mark_non_differentiable(sem)
        ctx.set_materialize_grads(False)
        return sem, pooled, ce

    @staticmethod
    def backward(ctx, _dsem, dpooled, dce):
        y2, gamma, beta, mean, invstd, w6, b6, gt = ctx.saved_tensors
        B, H, W, _ = y2.shape
        classes = w6.shape[0]
        dev = y2.device
        dpooled = None if dpooled is None else dpooled.contiguous()
        dce = None if dce is None else dce.contiguous().float()
        if dpooled is not None and dpooled.dtype != torch.bfloat16:
            raise _abi.WsmgError("cls_tail: the pooled map's gradient must be bf16")
        Hg, Wg = (gt.shape[1], gt.shape[2]) if gt is not None else (0, 0)
        dbn = torch.empty_like(y2)
        nws = int(_abi.lib().wsmg_cls_tail_workspace_floats(B))
        ws = torch.empty(nws, device=dev, dtype=torch.float32)
        dgamma, dbeta = torch.empty(32, device=dev), torch.empty(32, device=dev)
        dw6, db6 = torch.empty_like(w6), torch.empty_like(b6)
        _abi.call("wsmg_cls_tail_bwd_bf16", _p(y2), _p(gamma), _p(beta), _p(mean), _p(invstd), _p(w6), _p(b6), classes,
                  _p(gt if dce is not None else None), Hg, Wg, _p(dce), _p(dpooled), B, H, W, _p(dbn), _p(ws), nws, _p(dgamma), _p(dbeta),
                  _p(dw6), _p(db6), _stream())
        # BatchNorm's apply pass, in place (element i of dx depends on element i of dy and x only)
        _abi.call("wsmg_bn_bwd_apply_bf16", _p(dbn), _p(y2), _p(gamma), _p(mean), _p(invstd), _p(dgamma), _p(dbeta), B * H * W, 32, _p(dbn),
                  _stream())
        return dbn, None, dgamma, dbeta, None, None, None, None, dw6, db6, None


def cls_tail_ok(y2, classes):
    """Can `cls_tail` take this activation?  bf16 [B, H, W, 32] with H even and W a multiple of 16, at most 32 classes."""
    return (y2.is_cuda and y2.dtype == torch.bfloat16 and y2.dim() == 4 and y2.shape[3] == 32 and y2.shape[1] % 2 == 0
            and y2.shape[2] % 16 == 0 and classes <= 32 and sw.fused_cls_tail)


def cls_tail(y2, stats, bn, conv1x1, gt=None):
    """-> (logits [B,H,W,32] bf16 — not differentiable, for inspection / pred_sem_map —, pooled [B,H/2,W/2,32] bf16, ce_rows [B] or
    None): train-mode `bn` (nn.BatchNorm2d(32), statistics in `stats` from the producing convolution's epilogue) + ReLU + `conv1x1`
    (nn.Conv2d(32, classes, 1)) + the prediction monitor's per-sample cross-entropy against gt [B,Hg,Wg] + AvgPool2d(2).
    A label outside [0, classes) — `F.cross_entropy` of the reference faults on it — makes that sample's loss row NaN (and with it
    the loss and the gradients behind it): loud, not a finite wrong number.  The loss is taken from the float32 logits; the
    unfused route takes it from the stored bf16 logits (the difference is inside the 5e-3 bar of the tests)."""
    w, b = conv1x1.weight, conv1x1.bias
    return _ClsTail.apply(y2.contiguous(), stats, bn.weight, bn.bias, bn.running_mean, bn.running_var, bn.momentum, bn.eps,
                          w.contiguous(), b, None if gt is None else gt.contiguous())


# ----------------------------------------------------------------------------- scoring the semantic-map head
NO_PRED = 255     # `pred` of a pixel without a prediction: a NaN among its class logits, or a masked-out row


@torch.no_grad()
def sem_confusion(logits_nhwc, gt, classes, confusion=None, ignored=None, row_mask=None, want_pred=False):
    """-> (confusion int64 [classes, classes], ignored int64 [2], pred uint8 [B, H, W] or None): one launch (csrc/wsmg_sem_eval.hip)
    over the NHWC logits [B, H, W, 32] (float32 or bf16, channels >= classes padding) and gt float32 [B, Hg, Wg].
    confusion[label][prediction] counts the pixels whose prediction — the argmax over the first `classes` channels, ties to the
    lowest index — meets the label `F.interpolate(gt.unsqueeze(1), size=(H, W)).long()` (policy.py:61-66 of the reference).
    ignored[0]: pixels whose label is outside [0, classes) — judged on the float, so NaN and +-Inf are outside and -0.5 is a valid 0 —;
    ignored[1]: pixels with a valid label and a NaN among their class logits (pred = NO_PRED).  Neither enters the matrix.
    `confusion` / `ignored` passed in are ACCUMULATED into (and returned); they are allocated and zeroed only when not passed.
    row_mask [B] bool or uint8: rows with 0 contribute nothing and get pred = NO_PRED.  Exact: no arithmetic touches the logits.
    gt=None is the prediction-only use: (None, None, pred), nothing is counted."""
    _req(logits_nhwc, gt, confusion, ignored, row_mask)
    classes = int(classes)
    if logits_nhwc.dim() != 4 or logits_nhwc.shape[-1] != 32 or not 1 <= classes <= 32:
        raise _abi.WsmgError("sem_confusion: logits [B, H, W, 32] (padded classes), 1 <= classes <= 32")
    B, H, W, _ = logits_nhwc.shape
    dev = logits_nhwc.device
    if row_mask is not None:
        if row_mask.dtype not in (torch.bool, torch.uint8) or row_mask.numel() != B:
            raise _abi.WsmgError(f"sem_confusion: row_mask must be bool or uint8 with one entry per row ({B})")
    if gt is None:
        if confusion is not None or ignored is not None:
            raise _abi.WsmgError("sem_confusion: without gt nothing is counted (the prediction-only use takes no confusion / ignored)")
        Hg = Wg = 0
        want_pred = True
    else:
        _f32(gt)
        if gt.dim() != 3 or gt.shape[0] != B:
            raise _abi.WsmgError(f"sem_confusion: ground truth [B, Hg, Wg] float32 with B = {B}, got {tuple(gt.shape)}")
        Hg, Wg = gt.shape[1], gt.shape[2]
        if confusion is None:
            confusion = torch.zeros(classes, classes, device=dev, dtype=torch.int64)
        if ignored is None:
            ignored = torch.zeros(2, device=dev, dtype=torch.int64)
        if confusion.dtype != torch.int64 or confusion.shape != (classes, classes) or ignored.dtype != torch.int64 or ignored.numel() != 2:
            raise _abi.WsmgError("sem_confusion: confusion int64 [classes, classes] and ignored int64 [2]")
    pred = torch.empty(B, H, W, device=dev, dtype=torch.uint8) if want_pred else None
    _abi.call("wsmg_sem_confusion" + (_sfx(logits_nhwc) or "_f32"), _p(logits_nhwc), classes, _p(gt), Hg, Wg, B, H, W, _p(row_mask),
              _p(confusion), _p(ignored), _p(pred), _stream())
    return confusion, ignored, pred


@torch.no_grad()
def sem_scores(confusion, out=None):
    """-> float64 [3 + 3 classes] on the device, one launch: pixels counted, pixel accuracy, mIoU, then per class IoU, ground-truth
    pixels, predicted pixels, from an int64 confusion matrix [classes, classes] (rows: labels).  A class with no pixel on either
    side has IoU NaN and is left out of the mIoU; NaN accuracy / mIoU for an empty matrix.  `out`: a float64 vector to write into."""
    _req(confusion, out)
    classes = confusion.shape[0] if confusion.dim() == 2 else 0
    if confusion.dtype != torch.int64 or confusion.dim() != 2 or confusion.shape[1] != classes or not 1 <= classes <= 32:
        raise _abi.WsmgError("sem_scores: confusion int64 [classes, classes], 1 <= classes <= 32")
    if out is None:
        out = torch.empty(3 + 3 * classes, device=confusion.device, dtype=torch.float64)
    elif out.dtype != torch.float64 or out.numel() != 3 + 3 * classes:
        raise _abi.WsmgError("sem_scores: out must be float64 [3 + 3 classes]")
    _abi.call("wsmg_sem_scores", _p(confusion), classes, _p(out), _stream())
    return out


# ----------------------------------------------------------------------------- scoring the attention, action and progress heads
# the row record and the accumulator block of csrc/wsmg_nav_eval.hip, as include/wsmgmap.h names them
NAV_ROW, NAV_COUNTS, NAV_SUMS = 18, 13, 12
NAV_ABSENT, NAV_COUNTED, NAV_INVALID = 0, 1, 2
NAV_FIELDS = dict(att_state=0, att_target=1, att_peak=2, att_cheb=3, att_euclid=4, att_mass=5, att_entropy=6, act_state=7, act_sq=8,
                  act_l2=9, act_abs=10, prog_state=14, prog_abs=15, prog_sq=16, prog_stop=17)
NAV_SUM_FIELDS = (3, 4, 5, 6, 8, 9, 10, 11, 12, 13, 15, 16)          # the row field behind sums[k]
NAV_N = dict(att=0, att_invalid=1, hit0=2, act=5, act_invalid=6, prog=7, prog_invalid=8, stop=9)


@torch.no_grad()
def nav_rows(att=None, dis=None, S=0, pred=None, waypoint=None, prog=None, progress=None, row_mask=None, stop_threshold=0.8,
             out=None, B=None):
    """-> rows float64 [B, NAV_ROW], one launch (csrc/wsmg_nav_eval.hip), one record per row of three groups, each given as a
    pair or left None (absent):
      attention  att float32 [B, S*S] against dis float32 [B, H, W]: the target cell (argmin of the area-resized dis, the argmax of
                 the contrastive monitor's target), the attention's peak cell, their Chebyshev / Euclidean distance in cells, the
                 attention mass within one cell of the target, the entropy;
      action     pred float32 [B, A <= 4] against waypoint float32 [B, >= A]: sum e^2, its root and |e_j| of e = tanh(pred) - waypoint;
      progress   prog / progress float32 with B elements: |d|, d^2 and the stop code 2 (progress >= thr) + (prog >= thr).
    Field positions: NAV_FIELDS; each group's state field is NAV_COUNTED, NAV_INVALID (NaN / negative attention, NaN in dis,
    non-finite pred / waypoint / prog / progress) or NAV_ABSENT (group not given, or row_mask[b] == 0), the group's other fields NaN
    unless counted.  row_mask [B] bool or uint8.  B is read from the first tensor given (`B=` with none); `out`: a record to write."""
    _req(att, dis, pred, waypoint, prog, progress, row_mask, out)
    _f32(att, dis, pred, waypoint, prog, progress)
    given = [t for t in (att, dis, pred, waypoint, prog, progress) if t is not None]
    if (att is None) != (dis is None) or (pred is None) != (waypoint is None) or (prog is None) != (progress is None):
        raise _abi.WsmgError("nav_rows: att / dis, pred / waypoint and prog / progress come in pairs")
    if given:
        B = given[0].shape[0] if given[0].dim() else 0
    elif B is None:
        B = out.shape[0] if out is not None and out.dim() == 2 else 0
    B, S = int(B), int(S)
    if B <= 0:
        raise _abi.WsmgError("nav_rows: no rows (with no group given, pass B or out)")
    H = W = A = ld = 0
    if att is not None:
        if not 1 <= S <= 64 or att.dim() != 2 or tuple(att.shape) != (B, S * S) or dis.dim() != 3 or dis.shape[0] != B or dis.numel() == 0:
            raise _abi.WsmgError(f"nav_rows: attention [B, S*S] (1 <= S <= 64) and dis [B, H, W] with B = {B}, S = {S}, got "
                                 f"{tuple(att.shape)} and {tuple(dis.shape)}")
        H, W = dis.shape[1], dis.shape[2]
    else:
        S = S if 1 <= S <= 64 else 1
    if pred is not None:
        A = pred.shape[-1] if pred.dim() == 2 else 0
        if pred.dim() != 2 or pred.shape[0] != B or not 1 <= A <= 4 or waypoint.dim() != 2 or waypoint.shape[0] != B or waypoint.shape[1] < A:
            raise _abi.WsmgError(f"nav_rows: pred [B, A <= 4] and waypoint [B, >= A] with B = {B}, got {tuple(pred.shape)} and "
                                 f"{tuple(waypoint.shape)}")
        ld = waypoint.shape[1]
    if prog is not None and (prog.numel() != B or progress.numel() != B):
        raise _abi.WsmgError(f"nav_rows: prog and progress with {B} elements, got {tuple(prog.shape)} and {tuple(progress.shape)}")
    if row_mask is not None and (row_mask.dtype not in (torch.bool, torch.uint8) or row_mask.numel() != B):
        raise _abi.WsmgError(f"nav_rows: row_mask must be bool or uint8 with one entry per row ({B})")
    if out is None:
        dev = given[0].device if given else (row_mask.device if row_mask is not None else torch.device("cuda"))
        out = torch.empty(B, NAV_ROW, device=dev, dtype=torch.float64)
    elif out.dtype != torch.float64 or tuple(out.shape) != (B, NAV_ROW):
        raise _abi.WsmgError(f"nav_rows: out must be float64 [{B}, {NAV_ROW}], got {out.dtype} {tuple(out.shape)}")
    _abi.call("wsmg_nav_rows", _p(att), _p(dis), S, H, W, _p(pred), _p(waypoint), ld, A, _p(prog), _p(progress), float(stop_threshold),
              _p(row_mask), B, _p(out), _stream())
    return out


@torch.no_grad()
def nav_accumulate(rows, counts=None, sums=None):
    """-> (counts int64 [NAV_COUNTS], sums float64 [NAV_SUMS]): one launch, one workgroup, folds a `nav_rows` record into the
    counts (NAV_N: counted and invalid rows per group, attention hits at Chebyshev distance <= 0 / 1 / 2, the 2 x 2 stop confusion)
    and the sums of the float fields (NAV_SUM_FIELDS) over each group's counted rows.  Both are ACCUMULATED into when passed (and
    allocated zeroed when not); every sum continues from its stored value and adds the rows in order, so it is repeatable to the bit."""
    _req(rows, counts, sums)
    if rows.dtype != torch.float64 or rows.dim() != 2 or rows.shape[1] != NAV_ROW or rows.shape[0] == 0:
        raise _abi.WsmgError(f"nav_accumulate: rows float64 [B, {NAV_ROW}], got {rows.dtype} {tuple(rows.shape)}")
    if counts is None:
        counts = torch.zeros(NAV_COUNTS, device=rows.device, dtype=torch.int64)
    if sums is None:
        sums = torch.zeros(NAV_SUMS, device=rows.device, dtype=torch.float64)
    if counts.dtype != torch.int64 or counts.numel() != NAV_COUNTS or sums.dtype != torch.float64 or sums.numel() != NAV_SUMS:
        raise _abi.WsmgError(f"nav_accumulate: counts int64 [{NAV_COUNTS}] and sums float64 [{NAV_SUMS}]")
    _abi.call("wsmg_nav_accumulate", _p(rows), rows.shape[0], _p(counts), _p(sums), _stream())
    return counts, sums


# ----------------------------------------------------------------------------- update-path heads, auxiliary reduction, trainer loss
HEADS_MAX_A = 4           # HEADS_MAXA of csrc/wsmg_heads_common.h: the action dimensions update_heads and eval_heads take
EVAL_HEADS_MAX_A = HEADS_MAX_A      # (the name it had while only eval_heads checked it on the host)


def _grad_f32(t):
    """An upstream gradient as the backward kernels read it (contiguous float32); None — nothing reached that output — stays None."""
    return None if t is None else t.contiguous().float()


class _UpdateHeads(torch.autograd.Function):
    """(pred [B,A], prog [B,1], progress-loss rows [B]) of the update path in one launch per direction (csrc/wsmg_heads.hip):
    `action_distribution.fc_mean`, `tanh(prog_pred(.))` and `mse_loss(prog, progress, 'none').mean(-1)` of the reference's
    BasePolicy.forward / aux_prediction (models/policy.py:59,86-88,96-97)."""

    @staticmethod
    def forward(ctx, x, wm, bm, wp, bp, progress):
        _req(x, wm, bm, wp, bp, progress)
        _f32(x, wm, bm, wp, bp, progress)
        B, K = x.shape
        A = wm.shape[0]
        if wm.shape != (A, K) or wp.numel() != K or bm.numel() != A or bp.numel() != 1 or (progress is not None and progress.numel() != B):
            raise _abi.WsmgError("update_heads: head shapes do not fit the features")
        pred = torch.empty(B, A, device=x.device, dtype=torch.float32)
        prog = torch.empty(B, 1, device=x.device, dtype=torch.float32)
        rows = torch.empty(B, device=x.device, dtype=torch.float32) if progress is not None else None
        _abi.call("wsmg_update_heads_fwd", _p(x), _p(wm), _p(bm), _p(wp), _p(bp), _p(progress), B, K, A, _p(pred), _p(prog), _p(rows), _stream())
        ctx.save_for_backward(x, wm, wp, prog, progress)
        ctx.set_materialize_grads(False)
        return pred, prog, rows

    @staticmethod
    def backward(ctx, dpred, dprog, drows):
        x, wm, wp, prog, progress = ctx.saved_tensors
        B, K = x.shape
        A = wm.shape[0]
        dpred, dprog, drows = _grad_f32(dpred), _grad_f32(dprog), _grad_f32(drows)
        dx = torch.empty_like(x)
        dwm, dbm = torch.empty_like(wm), torch.empty(A, device=x.device, dtype=torch.float32)
        dwp, dbp = torch.empty_like(wp), torch.empty(1, device=x.device, dtype=torch.float32)
        _abi.call("wsmg_update_heads_bwd", _p(x), _p(wm), _p(wp), _p(prog), _p(progress), _p(dpred), _p(dprog), _p(drows), B, K, A,
                  _p(dx), _p(dwm), _p(dbm), _p(dwp), _p(dbp), _stream())
        return dx, dwm, dbm, dwp, dbp, None


def update_heads(features, fc_mean, prog_pred, progress=None):
    """-> (pred [B,A], prog [B,1], rows [B] or None): action mean, tanh progress head and — with `progress` [B,1] — the progress
    monitor's per-row squared error, one launch; fc_mean / prog_pred are the nn.Linear modules."""
    return _UpdateHeads.apply(features.contiguous(), fc_mean.weight, fc_mean.bias, prog_pred.weight, prog_pred.bias,
                              None if progress is None else progress.contiguous())


class _AuxReduce(torch.autograd.Function):
    """_AuxLosses.reduce(mask) (common/aux_losses.py:24-35) over up to 4 per-row loss vectors: one launch per direction."""

    @staticmethod
    def forward(ctx, mask, alphas, *rows):
        _req(mask, *rows)
        _f32(*rows)
        B = rows[0].numel()
        if mask.dtype != torch.bool or mask.numel() != B or any(r.numel() != B for r in rows) or not 1 <= len(rows) <= 4:
            raise _abi.WsmgError("aux_reduce: 1-4 float32 loss vectors and a bool mask of one length")
        L = len(rows)
        ptrs = (ctypes.c_void_p * L)(*[r.data_ptr() for r in rows])
        al = (ctypes.c_float * L)(*[float(a) for a in alphas])
        out = torch.empty(2, device=mask.device, dtype=torch.float32)
        _abi.call("wsmg_aux_reduce_fwd", ctypes.cast(ptrs, ctypes.c_void_p), ctypes.cast(al, ctypes.c_void_p), L, _p(mask), B, _p(out), _stream())
        ctx.save_for_backward(mask, out)
        ctx.alphas, ctx.shapes = tuple(float(a) for a in alphas), [r.shape for r in rows]
        return out[0]

    @staticmethod
    def backward(ctx, daux):
        mask, out = ctx.saved_tensors
        L, B = len(ctx.alphas), mask.numel()
        al = (ctypes.c_float * L)(*ctx.alphas)
        drows = torch.empty(L, B, device=mask.device, dtype=torch.float32)
        _abi.call("wsmg_aux_reduce_bwd", ctypes.cast(al, ctypes.c_void_p), L, _p(mask), _p(out[1:]), _p(daux.contiguous().float()), B, _p(drows),
                  _stream())
        return (None, None) + tuple(drows[k].view(shp) for k, shp in enumerate(ctx.shapes))


def aux_reduce(rows, alphas, mask):
    """sum_k alphas[k] * mean(rows[k][mask]) as a 0-dim tensor (rows: list of [B] float32 CUDA tensors, mask [B] bool)."""
    return _AuxReduce.apply(mask.contiguous(), tuple(alphas), *[r.contiguous() for r in rows])


class _DaggerLoss(torch.autograd.Function):
    """The trainer's loss of one update (dagger_trainer.py:526-534): weighted squared error of tanh(pred) against the waypoint,
    per-episode weight normalisation, mean over episodes, + the auxiliary loss — one launch per direction."""

    @staticmethod
    def forward(ctx, pred, waypoint, weights, aux):
        _req(pred, waypoint, weights, aux)
        _f32(pred, waypoint, weights, aux)
        T, N = weights.shape
        A = pred.shape[-1]
        if pred.numel() != T * N * A or waypoint.shape[0] != T * N or waypoint.shape[-1] < A or waypoint.dim() != 2:
            raise _abi.WsmgError("dagger_loss: pred [T*N, A], waypoint [T*N, >= A], weights [T, N]")
        out = torch.empty(2, device=pred.device, dtype=torch.float32)
        den = torch.empty(N, device=pred.device, dtype=torch.float32)
        _abi.call("wsmg_dagger_loss_fwd", _p(pred), _p(waypoint), waypoint.shape[-1], _p(weights), _p(aux), T, N, A, _p(out), _p(den), _stream())
        ctx.save_for_backward(pred, waypoint, weights, den)
        ctx.has_aux = aux is not None
        loss, action = out[0], out[1]
        ctx.mark_non_differentiable(action)
        return loss, action

    @staticmethod
    def backward(ctx, dloss, _daction):
        pred, waypoint, weights, den = ctx.saved_tensors
        T, N = weights.shape
        A = pred.shape[-1]
        dloss = dloss.contiguous().float()
        dpred = torch.empty_like(pred)
        _abi.call("wsmg_dagger_loss_bwd", _p(pred), _p(waypoint), waypoint.shape[-1], _p(weights), _p(den), _p(dloss), T, N, A, _p(dpred), _stream())
        return dpred, None, None, (dloss.reshape(1) if ctx.has_aux else None)


def dagger_loss(pred, aux_loss, waypoint, weights):
    """-> (loss, action_loss) as 0-dim tensors; pred [T*N, A], waypoint [T*N, >= A] (its first A columns are the target),
    weights [T, N]; aux_loss a 0-dim tensor, a Python number (added on the host side of the graph) or None."""
    aux_t = aux_loss if torch.is_tensor(aux_loss) else None
    loss, action = _DaggerLoss.apply(pred.contiguous(), waypoint.contiguous(), weights.contiguous(),
                                     None if aux_t is None else aux_t.reshape(1).float())
    if aux_t is None and aux_loss is not None:
        loss = loss + float(aux_loss)
    return loss, action


# ----------------------------------------------------------------------------- policy-gradient heads and the PPO loss
PPO_MAX_ROWS = 1 << 20


class _EvalHeads(torch.autograd.Function):
    """(value [B,1], logp [B], entropy 0-dim) of habitat's `Policy.evaluate_actions` in one launch per direction
    (csrc/wsmg_pg_heads.hip): `CriticHead`, `DiagGaussian` and the patched Normal's `log_probs` / `entropy().mean()`
    (common/distributions.py:21-29,42-57 of the reference)."""

    @staticmethod
    def forward(ctx, x, wm, bm, logstd, wc, bc, action):
        _req(x, wm, bm, logstd, wc, bc, action)
        _f32(x, wm, bm, logstd, wc, bc, action)
        if x.dim() != 2 or wm.dim() != 2:
            raise _abi.WsmgError("eval_heads: features [B, K] and an fc_mean weight [A, K]")
        B, K = x.shape
        A = wm.shape[0]
        if (wm.shape != (A, K) or bm.numel() != A or logstd.numel() != A or wc.numel() != K or bc.numel() != 1
                or tuple(action.shape) != (B, A)):
            raise _abi.WsmgError("eval_heads: head shapes do not fit the features, or action is not [B, A]")
        if B < 1 or K % 4 or not 1 <= A <= HEADS_MAX_A:
            raise _abi.WsmgError(f"eval_heads: B >= 1, K % 4 == 0 and 1 <= A <= {HEADS_MAX_A}, got B = {B}, K = {K}, A = {A}")
        if any(t.data_ptr() % 16 for t in (x, wm, wc)):     # the forward reads them four floats at a time
            raise _abi.WsmgError("eval_heads: features, fc_mean.weight and critic.fc.weight must start on a 16-byte boundary "
                                 "(a view with a storage offset that is no multiple of 4 floats: clone it)")
        dev = x.device
        value, logp = torch.empty(B, 1, device=dev), torch.empty(B, device=dev)
        mean, ent = torch.empty(B, A, device=dev), torch.empty(1, device=dev)
        _abi.call("wsmg_eval_heads_fwd", _p(x), _p(wm), _p(bm), _p(logstd), _p(wc), _p(bc), _p(action), B, K, A, _p(value), _p(logp),
                  _p(mean), _p(ent), _stream())
        ctx.save_for_backward(x, wm, wc, logstd, action, mean)
        ctx.set_materialize_grads(False)
        return value, logp, ent[0]

    @staticmethod
    def backward(ctx, dvalue, dlogp, dent):
        x, wm, wc, logstd, action, mean = ctx.saved_tensors
        B, K = x.shape
        A = wm.shape[0]
        dvalue, dlogp, dent = _grad_f32(dvalue), _grad_f32(dlogp), _grad_f32(dent)
        dev = x.device
        dx, dwm, dwc = torch.empty_like(x), torch.empty_like(wm), torch.empty_like(wc)
        dbm, dbc, dls = torch.empty(A, device=dev), torch.empty(1, device=dev), torch.empty_like(logstd)
        _abi.call("wsmg_eval_heads_bwd", _p(x), _p(wm), _p(wc), _p(logstd), _p(action), _p(mean), _p(dvalue), _p(dlogp), _p(dent), B, K, A,
                  _p(dx), _p(dwm), _p(dbm), _p(dls), _p(dwc), _p(dbc), _stream())
        return dx, dwm, dbm, dls, dwc, dbc, None


def eval_heads_ok(features, action_dim):
    """Can `eval_heads` take these features?  float32 [B >= 1, K % 4 == 0] on the GPU, at most 4 action dimensions."""
    return (features.is_cuda and features.dtype == torch.float32 and features.dim() == 2 and features.shape[0] >= 1
            and features.shape[1] % 4 == 0 and 1 <= action_dim <= HEADS_MAX_A)


def eval_heads(features, fc_mean, logstd, critic_fc, action):
    """-> (value [B,1], logp [B], entropy 0-dim): the critic, sum_a Normal(fc_mean(f), exp(logstd)).log_prob(action) and the
    distribution's entropy (the same for every row, so also its batch mean), one launch per direction.  fc_mean / critic_fc: the
    nn.Linear modules; logstd: the [A, 1] parameter of DiagGaussian.logstd (its gradient comes back in that shape); action [B, A]
    takes no gradient."""
    return _EvalHeads.apply(features.contiguous(), fc_mean.weight, fc_mean.bias, logstd, critic_fc.weight, critic_fc.bias,
                            action.contiguous())


class _PpoLoss(torch.autograd.Function):
    """The clipped-surrogate loss of habitat-baselines' PPO.update in one launch per direction (csrc/wsmg_pg_heads.hip)."""

    @staticmethod
    def forward(ctx, logp, value, entropy, old_logp, adv, old_value, returns, mask, clip, value_coef, entropy_coef, clipped_value,
                gate=None, sums=None, kl_limit=None):
        rows = (logp, old_logp, adv, value, old_value, returns)
        _req(*rows, entropy, mask, gate, sums)
        _f32(*rows, entropy, gate, sums)
        B = logp.numel()
        if B < 1 or B > PPO_MAX_ROWS or any(r.numel() != B for r in rows) or entropy.numel() != 1:
            raise _abi.WsmgError(f"ppo_loss: six float32 row vectors of one length in [1, {PPO_MAX_ROWS}] and a one-element entropy, got "
                                 f"{[tuple(r.shape) for r in rows]} and {tuple(entropy.shape)}")
        if mask is not None and (mask.dtype not in (torch.bool, torch.uint8) or mask.numel() != B):
            raise _abi.WsmgError(f"ppo_loss: mask must be bool or uint8 with one entry per row ({B})")
        out = torch.empty(5, device=logp.device, dtype=torch.float32)
        nsel = torch.empty(1, device=logp.device, dtype=torch.float32)
        if gate is None:
            _abi.call("wsmg_ppo_loss_fwd", _p(logp), _p(old_logp), _p(adv), _p(value), _p(old_value), _p(returns), _p(mask), _p(entropy),
                      clip, value_coef, entropy_coef, int(clipped_value), B, _p(out), _p(nsel), _stream())
        else:
            _abi.call("wsmg_ppo_loss_fwd_gated", _p(logp), _p(old_logp), _p(adv), _p(value), _p(old_value), _p(returns), _p(mask),
                      _p(entropy), clip, value_coef, entropy_coef, int(clipped_value), B, kl_limit, _p(out), _p(nsel), _p(gate), _p(sums),
                      _stream())
            torch.autograd.graph.increment_version([gate, sums])       # written through raw pointers
        ctx.save_for_backward(logp, old_logp, adv, value, old_value, returns, mask, nsel)
        ctx.hyper = (clip, value_coef, entropy_coef, int(clipped_value))
        ctx.shapes = (logp.shape, value.shape, entropy.shape)
        outs = tuple(out[i] for i in range(5))
        ctx.mark_non_differentiable(*outs[1:])
        return outs

    @staticmethod
    def backward(ctx, dloss, *_):
        logp, old_logp, adv, value, old_value, returns, mask, nsel = ctx.saved_tensors
        B = logp.numel()
        dloss = dloss.contiguous().float().reshape(1)
        dev = logp.device
        dlogp, dvalue, dent = torch.empty(B, device=dev), torch.empty(B, device=dev), torch.empty(1, device=dev)
        _abi.call("wsmg_ppo_loss_bwd", _p(logp), _p(old_logp), _p(adv), _p(value), _p(old_value), _p(returns), _p(mask), _p(nsel),
                  _p(dloss), *ctx.hyper, B, _p(dlogp), _p(dvalue), _p(dent), _stream())
        s_logp, s_value, s_ent = ctx.shapes
        return (dlogp.view(s_logp), dvalue.view(s_value), dent.view(s_ent)) + (None,) * 12


# The KL gate record of wsmg_ppo_loss_fwd_gated (include/wsmgmap.h): KL_GATE float32 words, zeroed by the host at the start of an
# update, written by that kernel alone.  Word 0 is what `wsmgmap.optim.Adam.set_step_gate` reads.
KL_GATE = 8
KL_STOPPED, KL_TAKEN, KL_SEEN, KL_STOP_ORDINAL, KL_STOP_KL = 0, 1, 2, 3, 4


def kl_limit_of(target_kl):
    """Spinning Up's threshold as the gated loss compares it: float32(1.5 * target_kl), the product formed in double and rounded once
    (returned as the Python float of that float32)."""
    return float(torch.tensor(1.5 * float(target_kl), dtype=torch.float64).to(torch.float32))


def ppo_loss(logp, old_logp, adv, value, old_value, returns, entropy, clip, value_coef, entropy_coef, clipped_value=True, mask=None,
             gate=None, sums=None, kl_limit=None):
    """-> (loss, action_loss, value_loss, clip_frac, approx_kl), 0-dim tensors; only `loss` is differentiable, towards logp,
    value and entropy (old_logp, adv, old_value and returns take no gradient).
        ratio = exp(logp - old_logp);  action_loss = -mean(min(ratio adv, clamp(ratio, 1 - clip, 1 + clip) adv))
        value_loss = 0.5 mean(max((value - returns)^2, (vc - returns)^2)), vc = old_value + clamp(value - old_value, -clip, clip)
                     (clipped_value=False: 0.5 mean((returns - value)^2))
        loss = value_coef value_loss + action_loss - entropy_coef entropy
        clip_frac = mean(|ratio - 1| > clip);  approx_kl = mean(old_logp - logp)
    The rows are float32 GPU tensors with B elements each ([B] or [B, 1]); entropy has one element; mask [B] bool or uint8 selects
    the rows the means run over (none selected: NaN, as `aux_reduce`).

    gate, sums, kl_limit (all three or none): the same launch behind a KL gate — a PPO update's early stop, decided on the device.
    `gate` is a contiguous float32 GPU record of KL_GATE words that the caller zeroes at the start of an update:
        gate[KL_STOPPED]       set to 1 by the first call whose approx_kl > float32(kl_limit), and left set until the caller clears it
                               (a NaN approx_kl does not set it); word 0: what `Adam.set_step_gate(gate)` makes the step obey
        gate[KL_TAKEN]         calls that left the gate open (the steps taken)      gate[KL_SEEN]  calls since the record was cleared
        gate[KL_STOP_ORDINAL], gate[KL_STOP_KL]   the ordinal (from 0) and the approx_kl of the call that closed the gate
    and while the gate is open `sums[0:5] += (value_loss, action_loss, entropy, clip_frac, approx_kl)` in float32 (`sums`: a contiguous
    float32 GPU tensor of at least 5 elements); the call that closes the gate and the calls after it add nothing.  The five outputs
    and the gradients are those of the call without a gate, bit for bit: a stopped call's gradients are computed, and it is the gated
    optimizer step that applies none of them.  No host synchronisation; capturable."""
    c = lambda t: t.contiguous()    # noqa: E731
    if (gate is None) != (sums is None) or (gate is None) != (kl_limit is None):
        raise _abi.WsmgError("ppo_loss: gate, sums and kl_limit come together (all three, or none)")
    if gate is not None:
        for name, t, n in (("gate", gate, KL_GATE), ("sums", sums, 5)):
            if not (torch.is_tensor(t) and t.is_contiguous() and t.dim() == 1 and t.numel() >= n and not t.requires_grad):
                raise _abi.WsmgError(f"ppo_loss: {name} must be a contiguous 1-d float32 GPU tensor of at least {n} elements (it is "
                                     "written in place)")
        kl_limit = float(kl_limit)
        if kl_limit != kl_limit:
            raise _abi.WsmgError("ppo_loss: kl_limit is NaN (no approx_kl compares above it: pass inf for a gate that never closes)")
    return _PpoLoss.apply(c(logp), c(value), c(entropy), c(old_logp), c(adv), c(old_value), c(returns),
                          None if mask is None else c(mask), float(clip), float(value_coef), float(entropy_coef), bool(clipped_value),
                          gate, sums, kl_limit)


ROWS_MAX = 16     # rollout-size dense layers: up to this many rows go through linear_rows / act_heads


def rows_route(x):
    """True when a dense layer on x [B, ...] should take the one-launch rollout route: no autograd, float32 on the GPU, at most
    ROWS_MAX rows.  debug.sw.rows_linear = False turns it off (the nn.Linear modules run)."""
    return (not torch.is_grad_enabled() and x.is_cuda and x.dtype == torch.float32 and x.shape[0] <= ROWS_MAX
            and sw.rows_linear)


@torch.no_grad()
def linear_rows(x, weight, bias, act=None, pool=1):
    """act(x @ weight.T + bias) for a few rows in one launch (wsmg_linear_rows).  x [B, K] — or [B, K, pool], averaged over its
    last axis first; weight [O, K]; act None / "relu" / "tanh"."""
    x = x.contiguous()
    _req(x, weight, bias)
    _f32(x, weight, bias)
    B = x.shape[0]
    O, K = weight.shape
    if x.numel() != B * K * pool or (bias is not None and bias.numel() != O):
        raise _abi.WsmgError(f"linear_rows: x {tuple(x.shape)} does not fit weight {tuple(weight.shape)} (pool {pool})")
    y = torch.empty(B, O, device=x.device, dtype=torch.float32)
    _abi.call("wsmg_linear_rows", _p(x), _p(weight), _p(bias), _p(y), B, K, O, {None: 0, "relu": 1, "tanh": 2}[act], int(pool), _stream())
    return y


@torch.no_grad()
def act_heads(features, prog_pred, fc_mean, logstd, critic_fc, noise=None):
    """(prog [B,1], value [B,1], action [B,A], log-probability [B]) of one rollout step in one launch (wsmg_act_heads).
    prog_pred / fc_mean / critic_fc: nn.Linear modules; logstd: the [A, 1] parameter of DiagGaussian.logstd; noise: [B, A]
    standard normals for a sampled action, None for the mode."""
    features = features.contiguous()
    B, K = features.shape
    A = fc_mean.weight.shape[0]
    ls = logstd.reshape(-1)
    _req(features, prog_pred.weight, prog_pred.bias, fc_mean.weight, fc_mean.bias, ls, critic_fc.weight, critic_fc.bias, noise)
    _f32(features, prog_pred.weight, prog_pred.bias, fc_mean.weight, fc_mean.bias, ls, critic_fc.weight, critic_fc.bias, noise)
    if prog_pred.weight.shape != (1, K) or critic_fc.weight.shape != (1, K) or fc_mean.weight.shape[1] != K or ls.numel() != A or (
            noise is not None and noise.shape != (B, A)):
        raise _abi.WsmgError("act_heads: head shapes do not fit the features")
    dev = features.device
    prog, value = torch.empty(B, 1, device=dev), torch.empty(B, 1, device=dev)
    action, logp = torch.empty(B, A, device=dev), torch.empty(B, device=dev)
    _abi.call("wsmg_act_heads", _p(features), B, K, _p(prog_pred.weight), _p(prog_pred.bias), _p(fc_mean.weight), _p(fc_mean.bias),
              _p(ls), A, _p(critic_fc.weight), _p(critic_fc.bias), _p(noise), _p(prog), _p(value), _p(action), _p(logp), _stream())
    return prog, value, action, logp


@torch.no_grad()
def colsum_multi(mats):
    """[x.sum(0) for x in mats] for up to 16 contiguous float32 [rows, cols] GPU matrices in ONE launch (wsmg_colsum_multi): the bias
    gradients of the recurrent core's dense layers.  Fixed summation order (bit-reproducible)."""
    import ctypes
    _req(*mats)
    _f32(*mats)
    outs = [torch.empty(m.shape[1], device=m.device, dtype=torch.float32) for m in mats]
    for i in range(0, len(mats), 16):
        grp = list(zip(mats[i:i + 16], outs[i:i + 16]))
        arr = (_abi.ColsumDesc * len(grp))()
        for j, (m, o) in enumerate(grp):
            arr[j].x, arr[j].out, arr[j].rows, arr[j].cols = m.data_ptr(), o.data_ptr(), m.shape[0], m.shape[1]
        _abi.call("wsmg_colsum_multi", ctypes.cast(arr, ctypes.c_void_p), len(grp), _stream())
    return outs
