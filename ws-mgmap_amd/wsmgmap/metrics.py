"""wsmgmap.metrics — how good is the predicted semantic map?  Pixel accuracy, per-class IoU and mIoU of the semantic hallucination
head, accumulated on the device from what every forward pass leaves behind (`net.sem_logits_nhwc` and
`observations['gt_semantic_map']`): one kernel launch per update, no allocation after the first call at a batch size, no host
synchronisation — so it can sit inside a captured update.  Not a reference module: the reference reports the prediction monitor's
mean cross-entropy only (policy.py:61-66), which moves when the logits sharpen whether or not a pixel changes class.

    meter = SemanticMapMeter()                      # off by default: nothing constructs one unless the trainer does
    pred, aux = policy(obs, h, prev, masks, weights)
    meter.update(policy, obs, weights)              # one launch (+ the mask's compare), no sync
    ...
    print(meter.compute()["miou"])                  # one launch, one read-back
"""
import math

import torch

from . import _abi, ops
from .models.mg_map_policy import SEM_CLASSES


class SemanticMapMeter:
    """Confusion counts of the semantic-map head over the updates of an epoch.  The matrix (int64 [classes, classes], rows: labels),
    the `ignored` pair (labels outside [0, classes); NaN-logit pixels) and the score vector live in ONE device block allocated here,
    so `compute()` reads the pair and the scores back in one copy."""

    def __init__(self, classes=SEM_CLASSES, device=None):
        classes = int(classes)
        if not 1 <= classes <= 32:
            raise ValueError("SemanticMapMeter: 1 <= classes <= 32 (the logits carry 32 padded channels)")
        self.classes = classes
        self.device = torch.device("cuda" if device is None else device)
        if self.device.type != "cuda":
            raise _abi.WsmgError("SemanticMapMeter counts on the GPU: the HIP path is the only path (no CPU fallback); "
                                 "SemanticMapMeter.scores_from(confusion) scores a matrix on the host")
        n = classes * classes
        self._block = torch.zeros(n + 2 + 3 + 3 * classes, device=self.device, dtype=torch.int64)
        self.confusion = self._block[:n].view(classes, classes)          # the live tensor
        self.ignored = self._block[n:n + 2]
        self._scores = self._block[n + 2:].view(torch.float64)
        self._mask = None                                                # uint8-sized bool [B] of the last batch size seen

    def reset(self):
        self._block[:self.classes * self.classes + 2].zero_()

    @torch.no_grad()
    def update(self, policy_or_net, observations, weights=None):
        """Add the last forward pass of `policy_or_net` (a BasePolicy or its MGMapNet) to the counts.  weights: the update's
        weights — rows with weight <= 0 are left out, the mask `AuxLosses.reduce` gets."""
        net = getattr(policy_or_net, "net", policy_or_net)
        logits = getattr(net, "sem_logits_nhwc", None)
        if logits is None:
            raise _abi.WsmgError("SemanticMapMeter.update: no forward pass has parked semantic logits on this network yet "
                                 "(net.sem_logits_nhwc is None)")
        gt = observations.get("gt_semantic_map") if hasattr(observations, "get") else None
        if gt is None:
            raise _abi.WsmgError("SemanticMapMeter.update: observations carry no 'gt_semantic_map'")
        if not gt.is_cuda or gt.dtype != torch.float32 or gt.dim() != 3:
            raise _abi.WsmgError(f"SemanticMapMeter.update: 'gt_semantic_map' must be a float32 [B, Hg, Wg] tensor on the GPU, got "
                                 f"{gt.dtype} {tuple(gt.shape)} on {gt.device}")
        B = logits.shape[0]
        if gt.shape[0] != B:
            raise _abi.WsmgError(f"SemanticMapMeter.update: {gt.shape[0]} ground-truth maps for {B} rows of logits")
        mask = None
        if weights is not None:
            if weights.numel() != B:
                raise _abi.WsmgError(f"SemanticMapMeter.update: {weights.numel()} weights for {B} rows of logits")
            if self._mask is None or self._mask.numel() != B:
                self._mask = torch.empty(B, device=self.device, dtype=torch.bool)
            mask = torch.gt(weights.reshape(-1), 0, out=self._mask)
        ops.sem_confusion(logits, gt if gt.is_contiguous() else gt.contiguous(), self.classes, self.confusion, self.ignored, mask)

    def compute(self):
        """One `sem_scores` launch and one read-back -> dict(pixels, ignored_labels, nan_pixels, pixel_accuracy, miou, iou[classes],
        gt_pixels[classes], pred_pixels[classes]).  IoU of a class absent on both sides is NaN and left out of the mIoU."""
        ops.sem_scores(self.confusion, out=self._scores)
        host = self._block[self.classes * self.classes:].cpu()
        s = host[2:].view(torch.float64).tolist()
        return self._as_dict(s, int(host[0]), int(host[1]), self.classes)

    @staticmethod
    def _as_dict(s, ignored_labels, nan_pixels, classes):
        return dict(pixels=int(s[0]), ignored_labels=ignored_labels, nan_pixels=nan_pixels, pixel_accuracy=s[1], miou=s[2],
                    iou=[s[3 + 3 * c] for c in range(classes)], gt_pixels=[int(s[4 + 3 * c]) for c in range(classes)],
                    pred_pixels=[int(s[5 + 3 * c]) for c in range(classes)])

    @staticmethod
    def score_vector(confusion):
        """The host form of `ops.sem_scores`: float64 [3 + 3 classes] from an int64 matrix, in float64 torch on the CPU — row and
        column sums in int64, one float64 division per figure, the mIoU's sum over the present classes in class order."""
        m = confusion.detach().cpu()
        if m.dtype != torch.int64 or m.dim() != 2 or m.shape[0] != m.shape[1]:
            raise ValueError("scores_from: an int64 [classes, classes] confusion matrix")
        classes = m.shape[0]
        gt_n, pr_n, tp = m.sum(1), m.sum(0), m.diagonal()
        union = gt_n + pr_n - tp
        iou = torch.where(union != 0, tp.double() / union.double(), torch.full((classes,), math.nan, dtype=torch.float64))
        total, right = int(gt_n.sum()), int(tp.sum())
        present = [v for v in iou.tolist() if v == v]
        acc = float(right) / float(total) if total else math.nan
        miou = _ordered_sum(present) / float(len(present)) if present else math.nan
        out = torch.empty(3 + 3 * classes, dtype=torch.float64)
        out[0], out[1], out[2] = float(total), acc, miou
        out[3::3], out[4::3], out[5::3] = iou, gt_n.double(), pr_n.double()
        return out

    @staticmethod
    def scores_from(confusion, ignored=None):
        """The dict of `compute()` from a confusion matrix on either device (a CPU int64 tensor included: the documented host
        form); ignored: the pair, when known."""
        s = SemanticMapMeter.score_vector(confusion).tolist()
        ign = [0, 0] if ignored is None else [int(v) for v in ignored.detach().cpu().tolist()]
        return SemanticMapMeter._as_dict(s, ign[0], ign[1], confusion.shape[0])

    def state_dict(self):
        return {"classes": self.classes, "confusion": self.confusion.clone(), "ignored": self.ignored.clone()}

    def load_state_dict(self, state):
        c = state["confusion"]
        if int(state.get("classes", c.shape[0])) != self.classes or tuple(c.shape) != (self.classes, self.classes):
            raise ValueError(f"SemanticMapMeter.load_state_dict: a matrix of {tuple(c.shape)} for {self.classes} classes")
        self.confusion.copy_(c)
        self.ignored.copy_(state["ignored"])


def _ordered_sum(values):
    s = 0.0
    for v in values:
        s += v
    return s
