"""wsmgmap.metrics — how good are the policy's supervised heads?  Two meters, each accumulated on the device from what every forward
pass leaves behind, with no allocation after the first call at a batch size and no host synchronisation — so they can sit inside a
captured update.  Not reference modules: the reference reports the monitors' loss scalars only (policy.py:61-88), which move when
the outputs sharpen whether or not a pixel changes class, the attention finds the path or the agent would stop at the right step.

  SemanticMapMeter   pixel accuracy, per-class IoU and mIoU of the semantic hallucination head (`net.sem_logits_nhwc` against
                     `observations['gt_semantic_map']`): one launch per update
  NavigationMeter    the waypoint attention (`net.att_map_t_m` against `gt_path`: does it peak on the path?), the action mean (`pred`
                     against `waypoint`) and the progress head (`policy.prog` against `progress`, also as the rollout's stop rule):
                     two launches per update

    meter, nav = SemanticMapMeter(), NavigationMeter()      # off by default: nothing constructs one unless the trainer does
    pred, aux = policy(obs, h, prev, masks, weights)
    meter.update(policy, obs, weights)                      # one launch (+ the mask's compare), no sync
    nav.update(policy, obs, pred, weights)                  # two launches (+ the mask's compare), no sync
    ...
    print(meter.compute()["miou"], nav.compute()["hit_at_1"])      # one read-back each
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


def _rate(num, den):
    return float(num) / float(den) if den else math.nan


class NavigationMeter:
    """Scores of the waypoint attention, the action mean and the progress head over the updates of an epoch.  `update` writes one
    float64 record per row (`rows`, ops.NAV_FIELDS) and folds it, in row order, into 13 int64 counts and 12 float64 sums that live in
    ONE device block allocated here, so `compute()` is one copy.  The target cell of the attention is the argmin of the area-resized
    `gt_path` — the argmax of the contrastive monitor's softmax target, without its batch-global extremes."""

    def __init__(self, stop_threshold=0.8, device=None):
        stop_threshold = float(stop_threshold)
        if not math.isfinite(stop_threshold):
            raise ValueError("NavigationMeter: stop_threshold must be finite (the rollout's PROG_THRESHOLD)")
        self.stop_threshold = stop_threshold
        self.device = torch.device("cuda" if device is None else device)
        if self.device.type != "cuda":
            raise _abi.WsmgError("NavigationMeter scores on the GPU: the HIP path is the only path (no CPU fallback); "
                                 "NavigationMeter.rows_from(...) is the host form of the row record")
        self._block = torch.zeros(ops.NAV_COUNTS + ops.NAV_SUMS, device=self.device, dtype=torch.int64)
        self.counts = self._block[:ops.NAV_COUNTS]                          # the live tensors
        self.sums = self._block[ops.NAV_COUNTS:].view(torch.float64)
        self.rows = None                                                     # float64 [B, NAV_ROW] of the last update
        self.axes = 4                                                        # action axes of the last update that had the group
        self._mask = None

    def reset(self):
        self._block.zero_()

    def _check(self, name, t, B, dims):
        if not torch.is_tensor(t) or t.device != self._block.device or t.dtype != torch.float32 or t.dim() not in dims or (
                B is not None and t.shape[0] != B):
            what = f"{t.dtype} {tuple(t.shape)} on {t.device}" if torch.is_tensor(t) else type(t).__name__
            raise _abi.WsmgError(f"NavigationMeter.update: {name} must be a float32 tensor of {B if B is not None else 'B'} rows on "
                                 f"{self._block.device}, got {what}")
        return t if t.is_contiguous() else t.contiguous()

    @torch.no_grad()
    def update(self, policy, observations, pred=None, weights=None):
        """Add the last forward pass of `policy` (a BasePolicy; its MGMapNet alone scores the attention only) to the scores: two
        launches and the mask's compare.  pred: what `forward` returned.  A group whose inputs are absent — no `net.att_map_t_m` or no
        'gt_path' / 'waypoint_distribution'; no `pred` or no 'waypoint'; no `policy.prog` or no 'progress' — is skipped.  weights:
        the update's weights; rows with weight <= 0 are left out, the mask `AuxLosses.reduce` gets."""
        net = getattr(policy, "net", policy)
        get = observations.get if hasattr(observations, "get") else (lambda k: None)
        att, dis = getattr(net, "att_map_t_m", None), get("gt_path")
        if dis is None:
            dis = get("waypoint_distribution")
        wp, prog, progress = get("waypoint"), getattr(policy, "prog", None), get("progress")
        B, S = None, 1
        att_on, act_on, prog_on = att is not None and dis is not None, pred is not None and wp is not None, prog is not None and progress is not None
        if att_on:
            att = self._check("net.att_map_t_m", att, B, (2,))
            B = att.shape[0]
            dis = self._check("'gt_path'", dis, B, (3,))
            S = math.isqrt(att.shape[1])
            if S * S != att.shape[1] or not 1 <= S <= 64 or dis.numel() == 0:
                raise _abi.WsmgError(f"NavigationMeter.update: attention {tuple(att.shape)} is no [B, S*S] map with S <= 64, or "
                                     f"'gt_path' {tuple(dis.shape)} is empty")
        if act_on:
            pred = self._check("pred", pred, B, (2,))
            B = pred.shape[0]
            wp = self._check("'waypoint'", wp, B, (2,))
            if not 1 <= pred.shape[1] <= 4 or wp.shape[1] < pred.shape[1]:
                raise _abi.WsmgError(f"NavigationMeter.update: pred {tuple(pred.shape)} must be [B, A <= 4] and 'waypoint' "
                                     f"{tuple(wp.shape)} [B, >= A]")
            self.axes = pred.shape[1]
        if prog_on:
            prog = self._check("policy.prog", prog, B, (1, 2))
            B = prog.shape[0]
            progress = self._check("'progress'", progress, B, (1, 2))
            if prog.numel() != B or progress.numel() != B:
                raise _abi.WsmgError(f"NavigationMeter.update: policy.prog {tuple(prog.shape)} and 'progress' {tuple(progress.shape)} "
                                     f"must hold one value per row ({B})")
        if B is None:
            raise _abi.WsmgError("NavigationMeter.update: nothing to score — no attention / 'gt_path', no pred / 'waypoint' and no "
                                 "policy.prog / 'progress'")
        mask = None
        if weights is not None:
            if weights.numel() != B:
                raise _abi.WsmgError(f"NavigationMeter.update: {weights.numel()} weights {tuple(weights.shape)} for {B} rows")
            if self._mask is None or self._mask.numel() != B:
                self._mask = torch.empty(B, device=self.device, dtype=torch.bool)
            mask = torch.gt(weights.reshape(-1), 0, out=self._mask)
        if self.rows is None or self.rows.shape[0] != B:
            self.rows = torch.empty(B, ops.NAV_ROW, device=self.device, dtype=torch.float64)
        ops.nav_rows(att if att_on else None, dis if att_on else None, S, pred if act_on else None, wp if act_on else None,
                     prog if prog_on else None, progress if prog_on else None, mask, self.stop_threshold, out=self.rows)
        ops.nav_accumulate(self.rows, self.counts, self.sums)

    def compute(self):
        """One read-back, no launch -> dict: attention_rows, attention_invalid, hit_at_0 / _1 / _2 (the rate of counted rows whose
        peak lies within that Chebyshev distance of the target cell), mean_cell_distance (Euclidean, in cells),
        mean_chebyshev_distance, mean_mass_near_target, mean_entropy; action_rows, action_invalid, action_mse (mean over rows of
        sum_j e_j^2, the DAgger loss's term), action_l2, action_abs (per axis); progress_rows, progress_invalid, progress_mae,
        progress_mse, stop_confusion ([progress >= threshold][prog >= threshold]), stop_precision, stop_recall.  A rate whose
        denominator is 0 is NaN."""
        host = self._block.cpu()
        return self.scores_from(host[:ops.NAV_COUNTS], host[ops.NAV_COUNTS:].view(torch.float64), self.axes)

    @staticmethod
    def scores_from(counts, sums, axes=4):
        """The dict of `compute()` from a counts / sums pair on either device."""
        c = [int(v) for v in counts.detach().cpu().tolist()]
        s = [float(v) for v in sums.detach().cpu().tolist()]
        N = ops.NAV_N
        na, nc, npg = c[N["att"]], c[N["act"]], c[N["prog"]]
        stop = c[N["stop"]:N["stop"] + 4]                                  # code = 2 * truth + prediction
        out = dict(attention_rows=na, attention_invalid=c[N["att_invalid"]])
        for k in range(3):
            out[f"hit_at_{k}"] = _rate(c[N["hit0"] + k], na)
        out.update(mean_chebyshev_distance=_rate(s[0], na), mean_cell_distance=_rate(s[1], na), mean_mass_near_target=_rate(s[2], na),
                   mean_entropy=_rate(s[3], na))
        out.update(action_rows=nc, action_invalid=c[N["act_invalid"]], action_mse=_rate(s[4], nc), action_l2=_rate(s[5], nc),
                   action_abs=[_rate(s[6 + j], nc) for j in range(int(axes))])
        out.update(progress_rows=npg, progress_invalid=c[N["prog_invalid"]], progress_mae=_rate(s[10], npg), progress_mse=_rate(s[11], npg),
                   stop_confusion=[[stop[0], stop[1]], [stop[2], stop[3]]], stop_precision=_rate(stop[3], stop[3] + stop[1]),
                   stop_recall=_rate(stop[3], stop[3] + stop[2]))
        return out

    @staticmethod
    def rows_from(att=None, dis=None, S=0, pred=None, waypoint=None, prog=None, progress=None, mask=None, stop_threshold=0.8):
        """The documented host form of `ops.nav_rows`: float64 [B, NAV_ROW] on the CPU from tensors on either device, numpy in
        float64 with the definitions of include/wsmgmap.h — the cell means alone are float32, summed over each window in row-major
        order as the kernel sums them.  Every pair may be None (the group is absent); mask: rows with 0 are not counted."""
        import numpy as np

        def host(t, dtype=np.float32):
            if t is None:
                return None
            a = t.detach().cpu().numpy() if torch.is_tensor(t) else np.asarray(t)
            if dtype is np.float32 and a.dtype != np.float32:
                raise ValueError(f"rows_from: float32 inputs, got {a.dtype}")
            return a
        att, dis, pred, waypoint, prog, progress = (host(t) for t in (att, dis, pred, waypoint, prog, progress))
        mask = host(mask, None)
        if (att is None) != (dis is None) or (pred is None) != (waypoint is None) or (prog is None) != (progress is None):
            raise ValueError("rows_from: att / dis, pred / waypoint and prog / progress come in pairs")
        first = next((t for t in (att, pred, prog, mask) if t is not None), None)
        if first is None:
            raise ValueError("rows_from: no group and no mask: the number of rows is unknown")
        B, F = first.shape[0], ops.NAV_FIELDS
        on = np.ones(B, bool) if mask is None else mask.reshape(-1).astype(bool)
        rows = np.full((B, ops.NAV_ROW), np.nan)
        rows[:, [F["att_state"], F["act_state"], F["prog_state"]]] = ops.NAV_ABSENT

        def put(state, live, bad, fields):
            rows[live, state] = np.where(bad[live], ops.NAV_INVALID, ops.NAV_COUNTED)
            ok = live & ~bad
            for f, v in fields.items():
                rows[ok, f] = np.asarray(v, np.float64)[ok]
        with np.errstate(all="ignore"):
            if att is not None:
                S = int(S)
                if att.shape != (B, S * S) or dis.ndim != 3 or dis.shape[0] != B:
                    raise ValueError(f"rows_from: att [B, S*S] and dis [B, H, W], got {att.shape} and {dis.shape} with S = {S}")
                cells = _area_mean_f32(dis, S)
                target = np.where(np.isnan(cells), np.float32(np.inf), cells).argmin(1)          # first occurrence: the lowest index
                peak = np.where(np.isnan(att), -np.inf, att).argmax(1)
                bad = np.isnan(att).any(1) | (att < 0).any(1) | np.isnan(dis).reshape(B, -1).any(1)
                ty, tx, py, px = target // S, target % S, peak // S, peak % S
                dy, dx = np.abs(py - ty), np.abs(px - tx)
                a64 = att.astype(np.float64)
                mass = np.zeros(B)
                for oy in (-1, 0, 1):                                       # row-major over the clipped 3 x 3 neighbourhood
                    for ox in (-1, 0, 1):
                        y, x = ty + oy, tx + ox
                        inside = (y >= 0) & (y < S) & (x >= 0) & (x < S)
                        v = a64[np.arange(B), np.clip(y, 0, S - 1) * S + np.clip(x, 0, S - 1)]
                        mass = np.where(inside, mass + v, mass)
                pos = a64 > 0
                entropy = -np.where(pos, a64 * np.log(np.where(pos, a64, 1.0)), 0.0).sum(1)
                put(F["att_state"], on, bad, {F["att_target"]: target, F["att_peak"]: peak, F["att_cheb"]: np.maximum(dy, dx),
                                              F["att_euclid"]: np.sqrt((dy * dy + dx * dx).astype(np.float64)), F["att_mass"]: mass,
                                              F["att_entropy"]: entropy})
            if pred is not None:
                A = pred.shape[1]
                if pred.ndim != 2 or not 1 <= A <= 4 or waypoint.ndim != 2 or waypoint.shape[0] != B or waypoint.shape[1] < A:
                    raise ValueError(f"rows_from: pred [B, A <= 4] and waypoint [B, >= A], got {pred.shape} and {waypoint.shape}")
                w = waypoint[:, :A]
                e = np.tanh(pred.astype(np.float64)) - w.astype(np.float64)
                sq = np.zeros(B)
                for j in range(A):
                    sq = sq + e[:, j] * e[:, j]
                fields = {F["act_sq"]: sq, F["act_l2"]: np.sqrt(sq)}
                for j in range(4):
                    fields[F["act_abs"] + j] = np.abs(e[:, j]) if j < A else np.zeros(B)
                put(F["act_state"], on, ~(np.isfinite(pred).all(1) & np.isfinite(w).all(1)), fields)
            if prog is not None:
                p, q, thr = prog.reshape(-1), progress.reshape(-1), np.float32(stop_threshold)
                if p.shape[0] != B or q.shape[0] != B:
                    raise ValueError(f"rows_from: prog and progress with {B} elements, got {prog.shape} and {progress.shape}")
                d = p.astype(np.float64) - q.astype(np.float64)
                put(F["prog_state"], on, ~(np.isfinite(p) & np.isfinite(q)),
                    {F["prog_abs"]: np.abs(d), F["prog_sq"]: d * d, F["prog_stop"]: 2 * (q >= thr).astype(np.int64) + (p >= thr)})
        return torch.from_numpy(rows)

    @staticmethod
    def totals_from(rows, counts=None, sums=None):
        """The host form of `ops.nav_accumulate`: (counts int64 [13], sums float64 [12]) of a row record, continuing from a pair
        when given; every sum adds the rows in order in float64."""
        r = rows.detach().cpu().tolist()
        c = [0] * ops.NAV_COUNTS if counts is None else [int(v) for v in counts.detach().cpu().tolist()]
        s = [0.0] * ops.NAV_SUMS if sums is None else [float(v) for v in sums.detach().cpu().tolist()]
        F, N = ops.NAV_FIELDS, ops.NAV_N
        for row in r:
            for state, n_ok, n_bad in ((F["att_state"], N["att"], N["att_invalid"]), (F["act_state"], N["act"], N["act_invalid"]),
                                       (F["prog_state"], N["prog"], N["prog_invalid"])):
                c[n_ok] += row[state] == ops.NAV_COUNTED
                c[n_bad] += row[state] == ops.NAV_INVALID
            if row[F["att_state"]] == ops.NAV_COUNTED:
                for k in range(3):
                    c[N["hit0"] + k] += row[F["att_cheb"]] <= k
            if row[F["prog_state"]] == ops.NAV_COUNTED:
                c[N["stop"] + int(row[F["prog_stop"]])] += 1
            for k, f in enumerate(ops.NAV_SUM_FIELDS):
                state = F["prog_state"] if f >= F["prog_state"] else F["act_state"] if f >= F["act_state"] else F["att_state"]
                if row[state] == ops.NAV_COUNTED:
                    s[k] += row[f]
        return torch.tensor(c, dtype=torch.int64), torch.tensor(s, dtype=torch.float64)

    def state_dict(self):
        return {"stop_threshold": self.stop_threshold, "axes": self.axes, "counts": self.counts.clone(), "sums": self.sums.clone()}

    def load_state_dict(self, state):
        c, s = state["counts"], state["sums"]
        if float(state.get("stop_threshold", self.stop_threshold)) != self.stop_threshold:
            raise ValueError(f"NavigationMeter.load_state_dict: counts taken at stop threshold {state['stop_threshold']}, this meter's "
                             f"is {self.stop_threshold}")
        if c.numel() != ops.NAV_COUNTS or s.numel() != ops.NAV_SUMS or c.dtype != torch.int64 or s.dtype != torch.float64:
            raise ValueError(f"NavigationMeter.load_state_dict: counts int64 [{ops.NAV_COUNTS}] and sums float64 [{ops.NAV_SUMS}], got "
                             f"{c.dtype} {tuple(c.shape)} and {s.dtype} {tuple(s.shape)}")
        self.counts.copy_(c)
        self.sums.copy_(s)
        self.axes = int(state.get("axes", self.axes))


def _area_mean_f32(dis, S):
    """float32 [B, S*S]: F.interpolate(dis, size=(S, S), mode="area") with each window — [floor(i*L/S), ceil((i+1)*L/S)) along an axis
    of length L — summed in float32 in row-major order and divided by its count in float32."""
    import numpy as np
    B, H, W = dis.shape
    i = np.arange(S, dtype=np.int64)
    y0, y1, x0, x1 = i * H // S, -(-(i + 1) * H // S), i * W // S, -(-(i + 1) * W // S)
    hy, wx = y1 - y0, x1 - x0
    acc = np.zeros((B, S, S), np.float32)
    for oy in range(int(hy.max())):
        yy = np.minimum(y0 + oy, H - 1)
        for ox in range(int(wx.max())):
            xx = np.minimum(x0 + ox, W - 1)
            inside = (oy < hy)[:, None] & (ox < wx)[None, :]
            acc = np.where(inside[None], acc + dis[:, yy[:, None], xx[None, :]], acc)
    return (acc / (hy[:, None] * wx[None, :]).astype(np.float32)[None]).reshape(B, S * S)
