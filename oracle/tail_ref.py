"""The float64 yardstick of the update's loss tail (TEST INFRASTRUCTURE — part of oracle/).

Plain torch restatements of the reference's lines that the small float32 kernels at the end of every update compute
(csrc/wsmg_heads.hip and wsmg_loss.hip, which holds path_kl and the ce_nhwc kernels):

    update_heads   models/policy.py:58-59,86-88,96-97   action mean, tanh progress head, its squared error per row
    aux_reduce     common/aux_losses.py:24-35            sum_k alpha_k * masked_select(loss_k, mask).mean()
    dagger_loss    dagger_trainer.py:526-534             weighted squared error of tanh(pred), per-episode normalisation
    path_kl        models/policy.py:72-82                the contrastive monitor's KL against the resized distance map
    ce_nhwc        models/policy.py:61-66                per-pixel cross-entropy, from channels-last logits padded to 32

Every function casts its floating inputs to `dtype` (float64 by default; float32 shows what the reference's own arithmetic
gives at the precision of the kernels) and stays differentiable with respect to them.  Nothing in the product path imports this.
"""
import torch
import torch.nn.functional as F


def _c(t, dtype):
    return None if t is None else t.to(dtype)


def update_heads(x, Wm, bm, Wp, bp, progress=None, dtype=torch.float64):
    """-> (pred [B, A], prog [B, 1], rows [B] or None): `fc_mean(x)`, `tanh(prog_pred(x))` and, with progress [B, 1], the
    progress monitor's `mse_loss(prog, progress, 'none').mean(-1)`."""
    x, Wm, bm, Wp, bp, progress = (_c(t, dtype) for t in (x, Wm, bm, Wp, bp, progress))
    pred = x @ Wm.t() + bm
    prog = torch.tanh(x @ Wp.reshape(1, -1).t() + bp.reshape(1))
    rows = None if progress is None else ((prog - progress.reshape(-1, 1)) ** 2).mean(-1)
    return pred, prog, rows


def aux_reduce(rows, alphas, mask, dtype=torch.float64):
    """sum_k alphas[k] * masked_select(rows[k], mask).mean(): masked rows are dropped, not multiplied by zero, and an empty
    selection is NaN (the mean of nothing)."""
    total = 0.0
    for a, r in zip(alphas, rows):
        total = total + a * torch.masked_select(_c(r, dtype).reshape(-1), mask.reshape(-1)).mean()
    return total


def dagger_loss(pred, aux, waypoint, weights, dtype=torch.float64):
    """-> (loss, action_loss): pred [T*N, A], waypoint [T*N, >= A] (its first A columns are the target; the reference has
    A = 2), weights [T, N], aux a 0-dim tensor, a number or None."""
    pred, waypoint, weights = _c(pred, dtype), _c(waypoint, dtype), _c(weights, dtype)
    T, N = weights.shape
    A = pred.shape[-1]
    logits = torch.tanh(pred).view(T, N, A)
    al = ((logits - waypoint[:, :A].reshape(T, N, A)) ** 2).sum(dim=2)
    action = ((weights * al).sum(0) / weights.sum(0)).mean()
    if aux is None:
        return action, action
    return action + (_c(aux, dtype) if torch.is_tensor(aux) else aux), action


def path_kl_target(dis, S, tau, dtype=torch.float64):
    """softmax(area_resize((hi - dis) / (hi - lo), S x S) / tau) over the S*S bins, lo / hi the batch-global extremes of
    dis [B, H, W]; -> [B, S*S].  A constant dis is 0 / 0: NaN everywhere."""
    d = _c(dis, dtype)
    t = (d.max() - d) / (d.max() - d.min())
    t = F.interpolate(t.unsqueeze(1), size=[S, S], mode="area").squeeze(1)
    return F.softmax(t.reshape(t.shape[0], -1) / tau, dim=1)


def path_kl(dis, att, S, tau, dtype=torch.float64):
    """kl_div(log att, target, 'none').mean(-1) -> [B]; a target bin that is exactly 0 contributes 0 (xlogy)."""
    return F.kl_div(torch.log(_c(att, dtype)), path_kl_target(dis, S, tau, dtype), reduction="none").mean(-1)


def ce_nhwc(logits, target, classes, dtype=torch.float64):
    """Per-row cross-entropy over the first `classes` of the 32 padded channels of logits [..., 32]; target int64 [...] ->
    loss [...].  Rows whose label is in [0, classes) are `F.cross_entropy(..., reduction='none')`.  `F.cross_entropy` faults on
    any other label (-100, torch's ignore_index, is never produced by the reference and is not special here); the library's
    contract is that such a row is NaN, and this function states it: the row is NaN and takes no part in the gradient of the
    other rows (its own gradient row is left at zero here; the kernels write NaN into it)."""
    x = _c(logits, dtype).reshape(-1, 32)[:, :classes]
    t = target.reshape(-1)
    ok = (t >= 0) & (t < classes)
    ce = F.cross_entropy(x, torch.where(ok, t, torch.zeros_like(t)), reduction="none")
    return torch.where(ok, ce, torch.full_like(ce, float("nan"))).reshape(target.shape)
