"""The oracle of the semantic-map scoring (csrc/wsmg_sem_eval.hip, ops.sem_confusion), numpy and torch on the CPU, and the input
makers its tests share.  Every comparison of counts and predictions made with it is exact equality."""
import numpy as np
import torch
import torch.nn.functional as F

NO_PRED = 255


def resized_labels(gt, H, W):
    """float32 [B, H, W]: the reference's F.interpolate(gt.unsqueeze(1), size=(H, W)) (nearest) on the float ground truth."""
    return F.interpolate(gt.detach().cpu().float().unsqueeze(1), size=(H, W)).squeeze(1).numpy()


def oracle(logits, gt, classes, row_mask=None):
    """-> (confusion int64 [classes, classes], ignored int64 [2], pred uint8 [B, H, W]) of logits [B, H, W, 32] (any float dtype:
    widened to float32) against gt float32 [B, Hg, Wg].  gt=None: predictions only (the matrix and the pair stay zero)."""
    x = logits.detach().cpu().float().numpy()[..., :classes]
    B, H, W, _ = x.shape
    nan = np.isnan(x).any(-1)
    arg = np.argmax(np.where(np.isnan(x), -np.inf, x), axis=-1)          # first occurrence = the tie rule; NaN rows are overridden
    on = np.ones(B, bool) if row_mask is None else row_mask.detach().cpu().numpy().astype(bool)
    on = np.broadcast_to(on[:, None, None], (B, H, W))
    pred = np.where(nan | ~on, NO_PRED, arg).astype(np.uint8)
    conf, ign = np.zeros((classes, classes), np.int64), np.zeros(2, np.int64)
    if gt is None:
        return conf, ign, pred
    g = resized_labels(gt, H, W)
    with np.errstate(invalid="ignore"):
        valid = (g > np.float32(-1.0)) & (g < np.float32(classes))      # on the float: NaN and +-Inf fail, -0.5 passes
    ign[0] = int((on & ~valid).sum())
    ign[1] = int((on & valid & nan).sum())
    take = on & valid & ~nan
    np.add.at(conf, (np.trunc(g[take]).astype(np.int64), arg[take].astype(np.int64)), 1)
    return conf, ign, pred


def make_logits(B, H, W, classes, dtype, seed):
    """Random logits [B, H, W, 32] of `dtype` (distinct values with near certainty), padding channels filled with noise too."""
    g = torch.Generator().manual_seed(seed)
    return torch.randn(B, H, W, 32, generator=g).to(dtype)


def make_gt(B, Hg, Wg, classes, seed):
    """float32 class ids uniform in [0, classes)."""
    g = torch.Generator().manual_seed(seed + 1000)
    return torch.randint(0, classes, (B, Hg, Wg), generator=g).float()


def sampled_sources(H, W, Hg, Wg):
    """(rows, columns) of the ground truth that the nearest resize to (H, W) reads, as torch computes them — found by resizing an
    index map, not by re-deriving the rule."""
    idx = torch.arange(Hg * Wg, dtype=torch.float32).view(1, 1, Hg, Wg)          # exact in float32 below 2^24
    src = F.interpolate(idx, size=(H, W)).long().view(-1)
    return sorted(set((src // Wg).tolist())), sorted(set((src % Wg).tolist()))
