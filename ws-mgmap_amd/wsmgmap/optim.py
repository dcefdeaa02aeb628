"""Adam for the update path, as ONE multi-tensor HIP launch per 48 tensors (csrc/wsmg_optim.hip).

The reference builds `torch.optim.Adam(self.actor_critic.parameters(), lr=...)` (common_trainer.py:67-69) and steps it after
`loss.backward()` (dagger_trainer.py:540-541).  This class is that optimizer — same constructor arguments, same arithmetic
in the same order, `state_dict()` interchangeable with torch.optim.Adam's (`step`, `exp_avg`, `exp_avg_sq`, and `max_exp_avg_sq`
with amsgrad=True) — with the step
issued as 3 kernel launches for the policy's 102 live tensors instead of the stock multi-tensor path's 15 (0.25 ms of GPU time
per update -> 0.06 ms).  float32 CUDA parameters only: anything else raises (there is no fallback path).

`Adam(max_grad_norm=..., skip_nonfinite=True)` guards the step on the device: the global gradient norm (deterministic float64
sums, wsmg_grad_norm_multi), `clip_grad_norm_`'s coefficient and a skip flag go into a small guard record that the Adam kernel
reads — no host synchronisation, capturable in a HIP graph.  `global_grad_norm(params)` is the norm alone.

`Adam(skip_nonfinite=True, guard_buffers=module)` extends the skip to what the forward pass already wrote: `zero_grad()` snapshots the
BatchNorm running statistics below `module` on the device (wsmg_copy_multi), and a skipped step copies them back
(wsmg_copy_multi_guarded, which reads the same guard record and writes nothing after a step that was taken).

`Adam(capturable=True or a guard option, hyper_on_device=True)` keeps `lr`, `betas`, `eps`, `weight_decay` of every parameter group
and `max_grad_norm` in a small device record that the kernels read (wsmg_adam_step_multi_hyper, wsmg_grad_norm_multi_hyper): a
captured step then follows `param_groups` edits and `torch.optim.lr_scheduler` steps, which kernel arguments frozen at capture
cannot.  `sync_hyper()` refreshes the record, outside the graph; an eager `step()` and `GraphedUpdate` call it themselves.

`Adam(a guard option, grad_report=True)` names the tensor behind a skipped step: behind the norm, wsmg_grad_report_multi writes one
row per parameter {norm, max |g| over the finite elements, NaN count, Inf count} and, only when the guard skips, copies the rows and a
header into a latch that keeps them until the host reads it, however many clean steps (or graph replays) follow.  `grad_report()`
and `last_skipped()` read them back; `grad_stats(params)` is the table alone, beside `global_grad_norm`.

`Adam(a guard option).set_step_gate(word)` puts the guarded step behind a device word that another kernel owns (the KL early stop of
`wsmgmap.ppo.PPO`): while it is non-zero the finalize of the norm (wsmg_grad_norm_multi_gated) forces the skip, with everything a skip
entails (no write, no step count, the BatchNorm roll-back) except the latch of the gradient report.

`Adam(amsgrad=True)`, `Adam(maximize=True)` and `AdamW(...)` (torch.optim.AdamW's decoupled weight decay, default 1e-2) step through
the `_ext` entry points (wsmg_adam_step_multi_ext and its three siblings): the same element step with the option's roundings added,
behind kernels of their own.  They combine with each other and with every option above.  With none of the three set, `step()` calls
the entry points without `_ext`, as it always did."""
import collections
import ctypes
import inspect
import math

import torch

from . import _abi


_AdamDesc = _abi.AdamDesc   # WsmgAdamDesc of include/wsmgmap.h: param, grad, exp_avg, exp_avg_sq, n

ADAM_CHUNK = 4096         # elements per workgroup (csrc/wsmg_optim.hip): one float64 partial each in the norm's workspace
ADAM_MAX = 48             # tensors (or copies) per launch (csrc/wsmg_common.h): longer lists are cut into several launches
FLAG_AMSGRAD, FLAG_MAXIMIZE, FLAG_DECOUPLED_WD = 1, 2, 4      # WSMG_ADAM_* of include/wsmgmap.h
# torch.optim.Adam grew the keyword in 2.7: where it exists `param_groups` carries it, as torch's do
_TORCH_HAS_DECOUPLED = "decoupled_weight_decay" in inspect.signature(torch.optim.Adam.__init__).parameters
HYPER_ROW = 8             # floats per row of the hyper record (include/wsmgmap.h): {lr, beta1, beta2, eps, weight_decay, 0, 0, 0} per
#                           parameter group, then the guard's row {max_grad_norm or 0, 0, ...}


def _check_max_grad_norm(max_grad_norm):
    if max_grad_norm is not None and not (math.isfinite(max_grad_norm) and max_grad_norm > 0.0):
        raise ValueError(f"invalid max_grad_norm: {max_grad_norm} (a finite positive number, or None for no clipping)")


def _check_hyper(lr, betas, eps, weight_decay):
    if lr < 0.0 or eps < 0.0 or weight_decay < 0.0 or not (0.0 <= betas[0] < 1.0 and 0.0 <= betas[1] < 1.0):
        raise ValueError(f"invalid Adam hyper-parameters: lr={lr} betas={betas} eps={eps} weight_decay={weight_decay}")


def _norm_blocks(descs):
    return sum((d.n + ADAM_CHUNK - 1) // ADAM_CHUNK for d in descs)


GradStat = collections.namedtuple("GradStat", "index name norm max_abs nan inf")
GradStat.__doc__ = """One row of the per-tensor gradient report: `index` in the flattened `param_groups` order, `norm` the tensor's L2 norm
(float32 of a float64 sum), `max_abs` the largest |g| among the finite elements (0.0 if there is none), `nan` / `inf` element counts."""
SkippedStep = collections.namedtuple("SkippedStep", "attempt skipped first_nonfinite largest nonfinite_tensors stats")
SkippedStep.__doc__ = """The latched report of the most recent skipped step: `attempt` its ordinal (steps taken + steps skipped, the host's
`state[p]["step"]` of that step), `skipped` how many steps had been skipped then, `first_nonfinite` the GradStat of the lowest-index
tensor with a NaN or Inf (None: every element was finite and the float32 norm overflowed), `largest` the GradStat with the largest norm
(a NaN norm counts as the largest), `nonfinite_tensors` how many tensors held a NaN or Inf, `stats` every row of that step."""
LATCH_HEADER = 8          # words in front of the latch's rows (include/wsmgmap.h)


def stats_as_float(table):
    """The float32 view of words 0-1 (norm, max |g|) of a report table ([n, 4] int32, as `grad_stats` returns it): [n, 2]."""
    return table[:, :2].view(torch.float32)


def _stats_rows(table, names):
    """[GradStat] of a report table on the host."""
    f = stats_as_float(table).tolist()
    c = table[:, 2:].tolist()
    return [GradStat(i, names[i], f[i][0], f[i][1], c[i][0] & 0xffffffff, c[i][1] & 0xffffffff) for i in range(len(f))]


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr())


def _stream(dev):
    return ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)


def _adam_descs(items):
    """The _AdamDesc array of [(p, g, exp_avg, exp_avg_sq, max_exp_avg_sq or None)]."""
    descs = (_AdamDesc * len(items))()
    for d, (p, g, m, v, _) in zip(descs, items):
        d.param, d.grad, d.exp_avg, d.exp_avg_sq, d.n = p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), p.numel()
    return descs


def _vmax_ptrs(items):
    """The host array of max_exp_avg_sq addresses parallel to `_adam_descs(items)` (what the _ext entry points take beside the
    descriptors), or None when no item has one."""
    if not items or items[0][4] is None:
        return None
    return (ctypes.c_void_p * len(items))(*[it[4].data_ptr() for it in items])


def _grad_descs(grads):
    """Gradient-only descriptors, one per entry: None and gradients without elements get a zero-length one (no chunk, a zero row)."""
    descs = (_AdamDesc * len(grads))()
    for d, g in zip(descs, grads):
        if g is not None and g.numel():
            d.grad, d.n = g.data_ptr(), g.numel()
    return descs


def _checked_grad_descs(what, grads):
    """Check a gradient list (None: no gradient) -> (device, descriptors, the contiguous gradients: copies live until the launches
    are queued)."""
    some = [g for g in grads if g is not None]
    if not some:
        raise _abi.WsmgError(f"wsmgmap.optim.{what}: no parameter has a gradient")
    dev = some[0].device
    for g in some:
        if g.is_sparse or not (g.is_cuda and g.dtype == torch.float32 and g.device == dev):
            raise _abi.WsmgError(f"wsmgmap.optim.{what}: gradients must be dense float32 CUDA tensors on one device")
    grads = [g if g is None or g.is_contiguous() else g.contiguous() for g in grads]
    return dev, _grad_descs(grads), grads


def grad_stats(params):
    """Per-tensor gradient statistics, one row per parameter in the order given: an [n, 4] int32 device table whose words are
    {float32 L2 norm, float32 max |g| over the finite elements, NaN count, Inf count} (`stats_as_float` views the first two).  A
    parameter without a gradient, or with no elements, has an all-zero row.  Deterministic (float64 sums in a fixed order: two calls
    return the same bits), a few launches per 48 tensors, no host synchronisation.  Dense float32 CUDA gradients on one device only."""
    dev, descs, grads = _checked_grad_descs("grad_stats", [p.grad for p in params])
    with torch.cuda.device(dev):
        cap = max(1, _norm_blocks(descs))
        partials = torch.empty(cap, device=dev, dtype=torch.float64)
        scan = torch.empty(4 * cap, device=dev, dtype=torch.int32)
        report = torch.empty(len(grads), 4, device=dev, dtype=torch.int32)
        _abi.call("wsmg_grad_stats_multi", descs, len(grads), _ptr(partials), cap, _ptr(scan), cap, _ptr(report), _stream(dev))
    return report


def global_grad_norm(params):
    """L2 norm over the `.grad` of every parameter that has one (as `clip_grad_norm_` over them computes it, but accumulated in
    float64 in a fixed order: two calls return the same bits): a 0-dim float32 tensor on the gradients' device.  A few launches per
    48 tensors and no host synchronisation; nothing is scaled.  Dense float32 CUDA gradients on one device only."""
    dev, descs, grads = _checked_grad_descs("global_grad_norm", [p.grad for p in params if p.grad is not None])
    with torch.cuda.device(dev):
        guard = torch.zeros(4, device=dev, dtype=torch.float32)
        cap = max(1, _norm_blocks(descs))
        partials = torch.empty(cap, device=dev, dtype=torch.float64)
        _abi.call("wsmg_grad_norm_multi", descs, len(grads), _ptr(partials), cap, 0.0, 0, _ptr(guard), None, _stream(dev))
    return guard[0]


class Adam(torch.optim.Optimizer):
    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, amsgrad=False, maximize=False,
                 capturable=False, max_grad_norm=None, skip_nonfinite=False, guard_buffers=None, hyper_on_device=False,
                 grad_report=False, decoupled_weight_decay=False):
        """amsgrad=True: the state gains `max_exp_avg_sq`, the running maximum of `exp_avg_sq` (a NaN propagates, as torch.maximum's
        does), allocated with the moments, and the step divides by its root; the parameters must be CUDA tensors (anything else is
        refused at construction: the variant exists on the device only).  maximize=True: the step reads -grad; the guard's norm
        and clip coefficient are those of grad.  decoupled_weight_decay=True (accepted where the installed torch.optim.Adam has the
        keyword; `AdamW` is this class with it set): a non-zero weight_decay multiplies the parameter by 1 - lr * weight_decay in
        front of the moments and is not added to the gradient.  All three are torch's arithmetic in torch's order, and combine with
        each other and with every option below.

        capturable=True: the step count also lives in a device scalar (one per parameter group, incremented on the device)
        and the kernel computes the bias corrections from it — the form `wsmgmap.graph.GraphedUpdate` captures into a HIP graph
        (kernel arguments are frozen at capture).  All stepped parameters of a group must then share one step count.

        max_grad_norm / skip_nonfinite (either one turns the GUARDED step on): before the step, the L2 norm over the gradients of
        every stepped tensor of every group is computed on the device; with max_grad_norm the step reads g * min(1, max_grad_norm /
        (norm + 1e-6)) — `clip_grad_norm_`'s arithmetic, but `p.grad` itself is NOT modified, the factor is applied where the Adam
        kernel reads it; with skip_nonfinite a NaN / Inf norm makes the step write nothing (parameters, moments and the step count
        stay as they were).  The step count lives on the device (one for the whole optimizer: all stepped parameters must share
        it and one device), `step()` never synchronises with the host and can be captured in a HIP graph whether or not
        capturable=True was passed.  `grad_norm`, `skipped_steps` and `state_dict()` report what happened.

        guard_buffers=module (needs skip_nonfinite=True): a skipped step also rolls back `running_mean`, `running_var` and
        `num_batches_tracked` of every BatchNorm layer below `module` that tracks running statistics — a poisoned forward pass has
        written them before any gradient exists.  `zero_grad()` (or `snapshot_buffers()`) copies them into one flat device
        allocation, on the current stream; the guarded step copies them back when, and only when, the guard record says the step
        was skipped.  Both are device launches behind the same record: no host synchronisation, capturable together with the
        step (after one eager snapshot: the allocation is never made under capture).  A `step()` with no snapshot since the
        previous one raises.  The snapshot is not optimizer state: `state_dict()` does not hold it.

        hyper_on_device=True (needs capturable=True or the guarded step: only those keep the step count on the device): the
        kernels read `lr`, `betas`, `eps`, `weight_decay` of their parameter group, and `max_grad_norm`, from a float32 record in
        device memory, not from their launch arguments, so a step captured in a HIP graph follows later `param_groups` edits,
        `torch.optim.lr_scheduler` steps and assignments to `max_grad_norm`.  `amsgrad`, `maximize` and the form of the weight decay
        are not in the record: they are structural (they choose the kernel and its arguments), are passed by value at each eager
        step, and a capture freezes them like any other argument.  `sync_hyper()` compares those values with a host
        mirror and, if one changed, refreshes the record with one asynchronous copy on the current stream: an eager `step()` and
        `GraphedUpdate` call it; around a graph of your own (`torch.cuda.graph`) call it before each replay.  Under capture
        nothing can be copied: a `step()` whose values differ from the mirror raises there.  Same arithmetic, bit for bit, as
        without the flag.  The record has one row per parameter group: `add_param_group` is refused after construction.

        grad_report=True (needs the guarded step): behind the norm, every guarded step also writes a per-tensor report on the device
        — one row per parameter in the flattened `param_groups` order, whether or not it has a gradient in this step (none: a zero
        row), so a parameter that comes and goes never shifts another tensor's row — and, only when the guard skips, copies it into
        a latch together with the attempt's ordinal and the index of the first tensor that held a NaN or Inf.  The latch keeps that
        until the next skipped step: `last_skipped()` reads it whenever the host gets round to it, `grad_report()` reads the most
        recent step's rows.  A few launches more per step, no host synchronisation, capturable with the step; parameters, moments,
        the guard record and the step count are what they are without the flag, bit for bit.  The tables are not optimizer state
        (`state_dict()` does not hold them) and are laid out once: `add_param_group` is refused after construction."""
        self._capturable = bool(capturable)
        self._step_dev = {}
        _check_max_grad_norm(max_grad_norm)
        self._max_grad_norm = None if max_grad_norm is None else float(max_grad_norm)
        self._skip_nonfinite = bool(skip_nonfinite)
        self._guarded = self._max_grad_norm is not None or self._skip_nonfinite
        self._guard = None        # device tensors of the guarded step: the record {norm, coef, skip, skipped}, the step count
        self._guard_step = None   # and the norm's float64 workspace (allocated below, never by a default construction)
        self._partials = None
        self._step_gate = None    # set_step_gate: a device word that forces the guarded step to skip while it is non-zero
        if guard_buffers is not None and not self._skip_nonfinite:
            raise ValueError("guard_buffers needs skip_nonfinite=True: nothing else ever triggers the roll-back")
        self._guard_buffers = guard_buffers
        self._snap = None          # guard_buffers only, all created by the first snapshot: the flat device allocation,
        self._snap_save = None     # the copy lists buffers -> snapshot and snapshot -> buffers (CopyDesc arrays),
        self._snap_restore = None
        self._snap_slots = None    # (name, the layer's buffer table, key) per protected buffer: the module tree is walked once
        self._snap_bufs = None     # the protected buffers (and the addresses the lists were built for)
        self._snap_ptrs = None
        self._snap_fresh = False   # a snapshot was taken since the previous step()
        self._hyper_on_device = bool(hyper_on_device)
        if self._hyper_on_device and not (self._capturable or self._guarded):
            raise ValueError("hyper_on_device=True needs capturable=True or the guarded step (max_grad_norm / skip_nonfinite): only "
                             "those keep the step count on the device, which the record-reading kernels take it from")
        self._hyper = None         # hyper_on_device only: the device record, a pinned staging tensor of its size, the host mirror of
        self._hyper_stage = None   # what the record holds (one tuple per row) and the event behind the last copy out of the staging
        self._hyper_mirror = None  # tensor (allocated by _reset_hyper, never by a default construction)
        self._hyper_event = None
        self._hyper_fixed = False  # the record's rows are laid out: no further parameter group
        self._grad_report = bool(grad_report)
        if self._grad_report and not self._guarded:
            raise ValueError("grad_report=True needs the guarded step (max_grad_norm / skip_nonfinite): the report is written behind "
                             "the guard's norm and latched by its skip flag")
        self._report = None        # grad_report only: the [parameters][4] report, the latch [8 + 4 parameters] and the scan workspace
        self._latch = None         # (4 words per chunk), all int32 (allocated by _reset_guard, never by a default construction)
        self._scan = None
        self._report_fixed = False  # the report's rows are laid out: no further parameter group
        if decoupled_weight_decay and not (_TORCH_HAS_DECOUPLED or isinstance(self, AdamW)):
            raise ValueError("decoupled_weight_decay is a keyword of wsmgmap.optim.Adam only where the installed torch.optim.Adam has "
                             "it; wsmgmap.optim.AdamW is the decoupled form everywhere")
        self._decoupled = bool(decoupled_weight_decay)      # of a group without the key (a torch that has no such keyword)
        _check_hyper(lr, betas, eps, weight_decay)
        defaults = dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, amsgrad=bool(amsgrad), maximize=bool(maximize))
        if _TORCH_HAS_DECOUPLED:
            defaults["decoupled_weight_decay"] = self._decoupled
        super().__init__(params, defaults)
        if self._guarded:
            self._reset_guard()
        if self._hyper_on_device:
            self._reset_hyper()
            self._hyper_fixed = True
        self._report_fixed = self._grad_report

    def _flat_params(self):
        return [p for group in self.param_groups for p in group["params"]]

    def _reset_guard(self):
        """(Re-)create the guard's device tensors from the host-side step counts: at construction and after load_state_dict, so
        that step() itself allocates and fills nothing — a fill captured into a HIP graph would reset the record at every replay."""
        self._guard = self._guard_step = self._partials = self._report = self._latch = self._scan = None
        params = self._flat_params()
        if not params or not all(p.is_cuda for p in params):
            return                 # step() refuses such parameters
        steps = {st["step"] for st in self.state.values() if "step" in st}
        if len(steps) > 1:
            return                 # step() refuses stepped parameters that do not share one count
        dev = params[0].device
        self._guard = torch.zeros(4, device=dev, dtype=torch.float32)
        self._guard_step = torch.full((), float(steps.pop() if steps else 0), device=dev, dtype=torch.float32)
        blocks = sum((p.numel() + ADAM_CHUNK - 1) // ADAM_CHUNK for p in params)
        self._partials = torch.empty(max(1, blocks), device=dev, dtype=torch.float64)
        if self._grad_report:      # the latch starts at zero: word 0 == 0 reads "never skipped"
            self._scan = torch.empty(4 * max(1, blocks), device=dev, dtype=torch.int32)
            self._report = torch.zeros(len(params), 4, device=dev, dtype=torch.int32)
            self._latch = torch.zeros(LATCH_HEADER + 4 * len(params), device=dev, dtype=torch.int32)

    def _reset_hyper(self):
        """(Re-)create the hyper record, its staging tensor and the mirror from `param_groups` and `max_grad_norm`: at construction
        and after load_state_dict, where the guard's tensors are made — never in step()."""
        self._hyper = self._hyper_stage = self._hyper_mirror = self._hyper_event = None
        params = self._flat_params()
        if not params or not all(p.is_cuda for p in params):
            return                 # step() refuses such parameters
        dev = params[0].device
        n = (len(self.param_groups) + 1) * HYPER_ROW
        with torch.cuda.device(dev):
            self._hyper = torch.zeros(n, device=dev, dtype=torch.float32)
            self._hyper_stage = torch.zeros(n, dtype=torch.float32, pin_memory=True)
            self.sync_hyper()

    def _hyper_values(self):
        """What the record should hold now, one tuple per row, validated with the constructor's rules (ValueError)."""
        rows = []
        for group in self.param_groups:
            lr, (b1, b2), eps, wd = float(group["lr"]), group["betas"], float(group["eps"]), float(group["weight_decay"])
            b1, b2 = float(b1), float(b2)
            _check_hyper(lr, (b1, b2), eps, wd)
            rows.append((lr, b1, b2, eps, wd))
        _check_max_grad_norm(self._max_grad_norm)
        rows.append((self._max_grad_norm or 0.0,))
        return rows

    def _hyper_is_stale(self, rows):
        if self._hyper is not None and len(rows) * HYPER_ROW != self._hyper.numel():
            raise _abi.WsmgError("wsmgmap.optim.Adam(hyper_on_device=True): the number of parameter groups changed since the hyper "
                                 "record was laid out (one row per group)")
        return rows != self._hyper_mirror

    def sync_hyper(self):
        """hyper_on_device=True: bring the device record up to `param_groups` (lr, betas, eps, weight_decay; a tensor-valued lr is
        read with float()) and `max_grad_norm` -> whether a copy was issued.  Nothing changed since the last call: nothing is done.
        Otherwise the values are validated (ValueError, the record keeps its contents), written to the pinned staging tensor and
        copied into the record with one non-blocking copy on the current stream.  Cannot copy under stream capture: raises there
        if the record is stale.  Without hyper_on_device: returns False."""
        if not self._hyper_on_device or self._hyper is None:
            return False
        rows = self._hyper_values()
        if not self._hyper_is_stale(rows):
            return False
        if torch.cuda.is_current_stream_capturing():
            raise _abi.WsmgError("wsmgmap.optim.Adam(hyper_on_device=True): param_groups / max_grad_norm changed since the last "
                                 "sync_hyper() and the record cannot be refreshed under stream capture; call sync_hyper() before "
                                 "the capture")
        if self._hyper_event is not None:
            self._hyper_event.synchronize()     # the previous copy has read the staging tensor (it was queued before the last step)
        flat = [0.0] * self._hyper.numel()
        for i, row in enumerate(rows):
            flat[i * HYPER_ROW:i * HYPER_ROW + len(row)] = row
        self._hyper_stage.copy_(torch.tensor(flat, dtype=torch.float32))      # rounds to float32 as a by-value c_float argument does
        dev = self._hyper.device
        with torch.cuda.device(dev):
            self._hyper.copy_(self._hyper_stage, non_blocking=True)
            self._hyper_event = torch.cuda.Event()
            self._hyper_event.record(torch.cuda.current_stream(dev))
        self._hyper_mirror = rows
        return True

    def _hyper_row(self, i):
        """Device address of row i of the hyper record (i = len(param_groups): the guard's row)."""
        return ctypes.c_void_p(self._hyper.data_ptr() + 4 * HYPER_ROW * i)

    def _hyper_before_step(self):
        """step() with hyper_on_device: refresh the record (eager), or refuse a stale one (under capture) — before any launch."""
        if self._hyper is None:
            raise _abi.WsmgError("wsmgmap.optim.Adam(hyper_on_device=True): the hyper record does not exist (construct the optimizer "
                                 "over the CUDA parameters it steps)")
        if torch.cuda.is_current_stream_capturing():
            if self._hyper_is_stale(self._hyper_values()):
                raise _abi.WsmgError("wsmgmap.optim.Adam(hyper_on_device=True): param_groups / max_grad_norm changed since the last "
                                     "sync_hyper(); the record cannot be refreshed under stream capture — call sync_hyper() before "
                                     "capturing step()")
        else:
            self.sync_hyper()

    @property
    def hyper_record(self):
        """hyper_on_device=True: the device record as a [groups + 1][8] float32 view (read-only use; reading it synchronises)."""
        return None if self._hyper is None else self._hyper.view(-1, HYPER_ROW)

    @property
    def max_grad_norm(self):
        return self._max_grad_norm

    @max_grad_norm.setter
    def max_grad_norm(self, value):
        """A new clip threshold.  Only between positive values: turning clipping on or off would change which path a graph captured
        (and whether the step is guarded at all).  Takes effect at the next eager step, or at the next sync_hyper() with
        hyper_on_device=True."""
        if (value is None) != (self._max_grad_norm is None):
            raise ValueError("max_grad_norm cannot be turned on or off after construction (None <-> a number): construct the "
                             "optimizer with the clipping it should have")
        if value is not None:
            value = float(value)
            _check_max_grad_norm(value)
        self._max_grad_norm = value

    def set_step_gate(self, gate):
        """Put the guarded step behind an external gate: `gate` is a float32 CUDA tensor on the parameters' device whose element 0
        another kernel owns (the `stopped` word of `ops.ppo_loss(..., gate=...)`), or None to take the gate away.  While gate[0] is
        non-zero every `step()` is skipped on the device, whatever its gradients are — parameters, moments and the device step count
        stay, `guard_buffers` rolls back, `skipped_steps` advances (so `state_dict()`'s `step` stays the steps taken, and
        `note_replayed_steps` stays right) — and `grad_norm` keeps the last judged step's norm; such a skip is no finding about the
        gradients, so `last_skipped()` does not report it.  With gate[0] == 0 the step is the step without a gate, bit for bit.
        The word is read on the device at each step (wsmg_grad_norm_multi_gated): no host synchronisation, and a step captured in a
        graph obeys it at every replay — set the gate before capturing.  Only the guarded step has a skip to force: an optimizer
        without max_grad_norm / skip_nonfinite refuses (ValueError)."""
        if gate is None:
            self._step_gate = None
            return
        if not self._guarded:
            raise ValueError("wsmgmap.optim.Adam.set_step_gate needs the guarded step (max_grad_norm / skip_nonfinite): only that step "
                             "reads a skip flag on the device; construct the optimizer with skip_nonfinite=True")
        if not (torch.is_tensor(gate) and gate.is_cuda and gate.dtype == torch.float32 and gate.numel() >= 1 and gate.is_contiguous()):
            raise ValueError("wsmgmap.optim.Adam.set_step_gate: the gate must be a contiguous float32 CUDA tensor with at least one "
                             f"element (element 0 is read), got {gate!r}")
        self._step_gate = gate

    def add_param_group(self, param_group):
        if self._hyper_fixed:
            raise ValueError("wsmgmap.optim.Adam(hyper_on_device=True): add_param_group after construction is refused — the hyper "
                             "record has one row per group and captured graphs hold its rows' addresses; pass every group to the "
                             "constructor")
        if self._report_fixed:
            raise ValueError("wsmgmap.optim.Adam(grad_report=True): add_param_group after construction is refused — the report has "
                             "one row per parameter and captured graphs hold its tables' addresses; pass every group to the "
                             "constructor")
        super().add_param_group(param_group)
        group = self.param_groups[-1]
        if group.get("amsgrad", False) and not all(p.is_cuda for p in group["params"]):
            self.param_groups.pop()
            raise ValueError("wsmgmap.optim.Adam(amsgrad=True) needs CUDA parameters: max_exp_avg_sq is a fifth array of the device "
                             "step, and this optimizer has no CPU path")

    def _protected_buffers(self):
        """[(qualified name, tensor)]: running_mean, running_var and num_batches_tracked of every BatchNorm layer below the
        guarded module that tracks running statistics, in module order.  The module tree is walked ONCE (0.9 ms of host time for
        the policy's 63 layers); afterwards the layers' buffer tables are read directly, which still sees a buffer that was
        replaced (`module.to(...)`, `load_state_dict(assign=True)`)."""
        if self._snap_slots is None:
            self._snap_slots = [(f"{mname}.{bname}" if mname else bname, m._buffers, bname)
                                for mname, m in self._guard_buffers.named_modules()
                                if isinstance(m, torch.nn.modules.batchnorm._BatchNorm) and m.track_running_stats
                                for bname in ("running_mean", "running_var", "num_batches_tracked")
                                if m._buffers.get(bname) is not None]
        return [(name, table[bname]) for name, table, bname in self._snap_slots]

    def _build_snapshot(self, named):
        """Check the protected buffers, lay them out in the flat allocation (16-byte slots: the copies take the vector path) and
        write the two copy lists.  The allocation is made once; under stream capture it must already exist."""
        what = "wsmgmap.optim.Adam(guard_buffers=...)"
        if not named:
            raise _abi.WsmgError(f"{what}: the module has no BatchNorm layer that tracks running statistics")
        params = self._flat_params()
        dev = params[0].device
        for name, b in named:
            if not (b.is_cuda and b.device == dev and b.is_contiguous()):
                raise _abi.WsmgError(f"{what}: buffer {name} must be a contiguous CUDA tensor on the parameters' device ({dev})")
        offsets, total = [], 0
        for _, b in named:
            offsets.append(total)
            total += (b.numel() * b.element_size() + 15) // 16 * 16
        if self._snap is None or self._snap.numel() < total or self._snap.device != dev:
            if torch.cuda.is_current_stream_capturing():
                raise _abi.WsmgError(f"{what}: the snapshot storage does not exist yet; take a snapshot (zero_grad() or "
                                     "snapshot_buffers()) before capturing into a graph")
            with torch.cuda.device(dev):
                self._snap = torch.empty(max(16, total), device=dev, dtype=torch.uint8)
        base = self._snap.data_ptr()
        save, restore = (_abi.CopyDesc * len(named))(), (_abi.CopyDesc * len(named))()
        for sv, rs, off, (_, b) in zip(save, restore, offsets, named):
            nbytes = b.numel() * b.element_size()
            sv.dst, sv.src, sv.bytes = base + off, b.data_ptr(), nbytes
            rs.dst, rs.src, rs.bytes = b.data_ptr(), base + off, nbytes
        self._snap_save, self._snap_restore = save, restore
        self._snap_bufs = [b for _, b in named]
        self._snap_ptrs = [b.data_ptr() for b in self._snap_bufs]

    @torch.no_grad()
    def snapshot_buffers(self):
        """Copy the protected buffers into the snapshot, on the current stream (one wsmg_copy_multi call: a launch per 32 buffers).
        `zero_grad()` does this; call it directly in a loop that zeroes the gradients some other way, before the forward pass."""
        if self._guard_buffers is None:
            raise _abi.WsmgError("wsmgmap.optim.Adam.snapshot_buffers: the optimizer was constructed without guard_buffers")
        if (self._snap_bufs is None or any(table[bname] is not b for (_, table, bname), b in zip(self._snap_slots, self._snap_bufs))
                or [b.data_ptr() for b in self._snap_bufs] != self._snap_ptrs):
            self._build_snapshot(self._protected_buffers())
        dev = self._snap.device
        with torch.cuda.device(dev):
            _abi.call("wsmg_copy_multi", ctypes.cast(self._snap_save, ctypes.c_void_p), len(self._snap_save), _stream(dev))
        self._snap_fresh = True

    def zero_grad(self, set_to_none=True):
        """torch.optim.Optimizer.zero_grad; with guard_buffers it also takes the snapshot — the reference's update and
        GraphedUpdate both call it in front of the forward pass, which is where the snapshot belongs."""
        super().zero_grad(set_to_none=set_to_none)
        if self._guard_buffers is not None:
            self.snapshot_buffers()

    def _flags(self, group):
        """WSMG_ADAM_* of a parameter group: 0 steps through the entry points without `_ext`."""
        return ((FLAG_AMSGRAD if group.get("amsgrad", False) else 0) | (FLAG_MAXIMIZE if group.get("maximize", False) else 0) |
                (FLAG_DECOUPLED_WD if group.get("decoupled_weight_decay", self._decoupled) else 0))

    def _stepped_items(self, group, guarded=False, dev=None):
        """The parameters of `group` that have a gradient, checked, their state created and their step count advanced ->
        ([(p, g, exp_avg, exp_avg_sq, max_exp_avg_sq or None)], [step count of each], dev).  guarded: they must all sit on `dev`
        (None: the first one's device), and moments that do not exist yet are refused under stream capture."""
        items, steps = [], []
        amsgrad = bool(group.get("amsgrad", False))
        for p in group["params"]:
            g = p.grad
            if g is None:
                continue
            if not (p.is_cuda and p.dtype == torch.float32 and p.is_contiguous()):
                raise _abi.WsmgError("wsmgmap.optim.Adam: parameters must be contiguous float32 CUDA tensors")
            if g.is_sparse or g.dtype != torch.float32 or g.device != p.device:
                raise _abi.WsmgError("wsmgmap.optim.Adam: gradients must be dense float32 tensors on the parameter's device")
            if guarded:
                if dev is None:
                    dev = p.device
                if p.device != dev:
                    raise _abi.WsmgError("wsmgmap.optim.Adam: the guarded step takes one norm over all parameters: they must share a device")
            if not g.is_contiguous():
                g = g.contiguous()
                g.record_stream(torch.cuda.current_stream(p.device))   # the copy must outlive the launch queued below
            st = self.state[p]
            if not st:
                if guarded and torch.cuda.is_current_stream_capturing():      # the zero fills would be replayed: moments reset every time
                    raise _abi.WsmgError("wsmgmap.optim.Adam: the moments do not exist yet; take a step (or load_state_dict) "
                                         "before capturing step() into a graph")
                st["step"] = 0    # a Python int while training (102 CPU-tensor increments per step cost 1 ms of host time);
                #                   state_dict() / load_state_dict() convert from / to torch.optim.Adam's float32 tensor
                st["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                st["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
            if amsgrad and "max_exp_avg_sq" not in st:      # with the moments, or at the first step after amsgrad was turned on
                if torch.cuda.is_current_stream_capturing():
                    raise _abi.WsmgError("wsmgmap.optim.Adam(amsgrad=True): max_exp_avg_sq does not exist yet; take a step (or "
                                         "load_state_dict) before capturing step() into a graph")
                st["max_exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
            st["step"] += 1       # guarded: ATTEMPTED steps; the device count (attempted - skipped) is what the kernel uses
            items.append((p, g, st["exp_avg"], st["exp_avg_sq"], st["max_exp_avg_sq"] if amsgrad else None))
            steps.append(st["step"])
        return items, steps, dev

    def _launch_step(self, descs, n, gi, group, stream, step=None, sd=None, guard=None, vmax=None):
        """The step's entry point for this optimizer: the record's row (hyper_on_device), else by value behind the guard record,
        with the device step count `sd` (capturable), or with the host's bias corrections of `step`.  A group with amsgrad,
        maximize or the decoupled decay goes through the `_ext` form of the same entry point, with its flags and `vmax`, the array
        of max_exp_avg_sq addresses parallel to descs (None without amsgrad); any other group through the entry points without it."""
        flags = self._flags(group)
        ext, more = ("_ext", (vmax, flags)) if flags else ("", ())
        if self._hyper_on_device:
            _abi.call("wsmg_adam_step_multi_hyper" + ext, descs, n, *more, self._hyper_row(gi), sd, guard, stream)
            return
        b1, b2 = group["betas"]
        by_value = (float(group["lr"]), float(b1), float(b2), float(group["eps"]), float(group["weight_decay"]))
        if guard is not None:
            _abi.call("wsmg_adam_step_multi_guarded" + ext, descs, n, *more, *by_value, sd, guard, stream)
        elif sd is not None:
            _abi.call("wsmg_adam_step_multi_dev" + ext, descs, n, *more, *by_value, sd, stream)
        else:
            _abi.call("wsmg_adam_step_multi" + ext, descs, n, *more, *by_value, 1.0 - b1 ** step, 1.0 - b2 ** step, stream)

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        if self._hyper_on_device:
            self._hyper_before_step()
        if self._guarded:
            self._guarded_step()
            return loss
        for gi, group in enumerate(self.param_groups):
            by_step = {}
            for item, step in zip(*self._stepped_items(group)[:2]):
                by_step.setdefault(step, []).append(item)
            if self._capturable and len(by_step) > 1:
                raise _abi.WsmgError("wsmgmap.optim.Adam(capturable=True): the stepped parameters of a group must share one step count")
            for step, items in by_step.items():
                dev = items[0][0].device
                with torch.cuda.device(dev):
                    if self._hyper_on_device and self._hyper.device != dev:
                        raise _abi.WsmgError("wsmgmap.optim.Adam(hyper_on_device=True): the hyper record is not on the stepped "
                                             "parameters' device")
                    sd = None
                    if self._capturable:
                        key = id(group)
                        if key not in self._step_dev:
                            self._step_dev[key] = torch.full((), float(step - 1), device=dev, dtype=torch.float32)
                        self._step_dev[key].add_(1.0)      # on the device: a replayed graph advances it without the host
                        sd = _ptr(self._step_dev[key])
                    self._launch_step(_adam_descs(items), len(items), gi, group, _stream(dev), step=step, sd=sd,
                                      vmax=_vmax_ptrs(items))
                # the kernel wrote the parameters through raw pointers: advance their autograd version counters, which is what
                # caches of derived operands (FoldCache, InstructionEncoder.packed_rnn_weights) compare
                torch.autograd.graph.increment_version([it[0] for it in items])
        return loss

    def _guarded_step(self):
        if self._guard_buffers is not None and not self._snap_fresh:
            raise _abi.WsmgError("wsmgmap.optim.Adam(guard_buffers=...): no snapshot was taken since the previous step() — call "
                                 "zero_grad() or snapshot_buffers() before the forward pass (an older snapshot would roll the "
                                 "statistics back by more than one update)")
        groups, steps, dev = [], set(), None
        for gi, group in enumerate(self.param_groups):
            items, counts, dev = self._stepped_items(group, guarded=True, dev=dev)
            steps.update(counts)
            if items:
                groups.append((gi, group, items))
        if not groups:
            return
        if len(steps) > 1:
            raise _abi.WsmgError("wsmgmap.optim.Adam: the guarded step keeps one step count on the device: all stepped parameters "
                                 "must share it")
        every = [it for _, _, items in groups for it in items]
        rows = None
        if self._grad_report:      # the gradient behind every report row (the stepped list's, in its order), None where there is none
            stepped = iter(every)
            rows = [None if p.grad is None else next(stepped)[1] for p in self._flat_params()]
        descs = _adam_descs(every)
        stream = _stream(dev)
        with torch.cuda.device(dev):
            if self._guard is None or self._guard.device != dev or self._partials.numel() < _norm_blocks(descs):
                raise _abi.WsmgError("wsmgmap.optim.Adam: the guard's device state does not fit the stepped parameters (construct the "
                                     "optimizer over the CUDA parameters it steps)")
            if self._guard_buffers is not None and self._snap.device != dev:
                raise _abi.WsmgError("wsmgmap.optim.Adam(guard_buffers=...): the snapshot is not on the stepped parameters' device")
            if self._hyper_on_device and self._hyper.device != dev:
                raise _abi.WsmgError("wsmgmap.optim.Adam(hyper_on_device=True): the hyper record is not on the stepped parameters' device")
            if rows is not None and (self._report is None or self._report.shape[0] != len(rows)):
                raise _abi.WsmgError("wsmgmap.optim.Adam(grad_report=True): the report's tables do not fit the parameters")
            guard, sd, partials = _ptr(self._guard), _ptr(self._guard_step), _ptr(self._partials)
            # the finalize advances the step count by 1 - skip: a skipped step does not advance the bias corrections
            norm, max_norm = (("wsmg_grad_norm_multi_hyper", self._hyper_row(len(self.param_groups))) if self._hyper_on_device
                              else ("wsmg_grad_norm_multi", self._max_grad_norm or 0.0))
            if self._step_gate is None:
                _abi.call(norm, descs, len(every), partials, self._partials.numel(), max_norm, int(self._skip_nonfinite), guard, sd, stream)
            else:     # the same norm; the finalize also reads the gate's word and skips while it is set
                if self._step_gate.device != dev:
                    raise _abi.WsmgError("wsmgmap.optim.Adam.set_step_gate: the gate is not on the stepped parameters' device")
                _abi.call(norm + "_gated", descs, len(every), partials, self._partials.numel(), max_norm, int(self._skip_nonfinite),
                          _ptr(self._step_gate), guard, sd, stream)
            if rows is not None:
                # descriptors of their own over ALL parameters: the stepped list with a zero-length one for every parameter without a
                # gradient — those own no chunk, so the norm's partials line up, and no row ever shifts
                _abi.call("wsmg_grad_report_multi", _grad_descs(rows), len(rows), partials, self._partials.numel(), _ptr(self._scan),
                          self._scan.numel() // 4, guard, sd, _ptr(self._report), _ptr(self._latch), stream)
            at = 0
            for gi, group, items in groups:
                self._launch_step(ctypes.byref(descs, at * ctypes.sizeof(_AdamDesc)), len(items), gi, group, stream, sd=sd, guard=guard,
                                  vmax=_vmax_ptrs(items))
                at += len(items)
            written = [it[0] for it in every]
            if self._guard_buffers is not None:
                _abi.call("wsmg_copy_multi_guarded", ctypes.cast(self._snap_restore, ctypes.c_void_p), len(self._snap_restore), guard,
                          stream)
                self._snap_fresh = False
                written = written + self._snap_bufs
        torch.autograd.graph.increment_version(written)

    @property
    def grad_norm(self):
        """The last guarded step's gradient norm before clipping: a 0-dim device tensor, a view of the guard record (reading it is
        the caller's synchronisation, holding it costs nothing).  None before the first guarded step."""
        return None if self._guard is None else self._guard[0]

    @property
    def skipped_steps(self):
        """How many guarded steps found a non-finite norm, or a step gate that was set, and wrote nothing (since construction or
        load_state_dict): one readback."""
        return 0 if self._guard is None else int(self._guard[3].item())

    def _report_names(self, names):
        """One name per report row: the `named_parameters()` keys of a module (matched by identity), a sequence of strings, or
        "group{g}.param{i}"."""
        default = [f"group{gi}.param{i}" for gi, group in enumerate(self.param_groups) for i in range(len(group["params"]))]
        if names is None:
            return default
        if isinstance(names, torch.nn.Module):
            by_id = {id(p): name for name, p in names.named_parameters()}
            params = self._flat_params()
            return [by_id.get(id(p), d) for p, d in zip(params, default)]
        names = [str(x) for x in names]
        if len(names) != len(default):
            raise ValueError(f"wsmgmap.optim.Adam: {len(names)} names for {len(default)} parameters")
        return names

    def grad_report(self, names=None):
        """grad_report=True: the per-tensor report of the most recent guarded step as a list of GradStat, one per parameter in the
        flattened `param_groups` order (a parameter without a gradient in that step: zeros) — one synchronising readback.  `names`:
        an `nn.Module` (its `named_parameters()` keys, the state_dict keys), a sequence of strings, or None for "group{g}.param{i}".
        An empty list when the report does not exist (constructed without the flag, or over parameters that are not on a device)."""
        if self._report is None:
            return []
        return _stats_rows(self._report.cpu(), self._report_names(names))

    def last_skipped(self, names=None):
        """grad_report=True: what the device latched at the most recent SKIPPED step, however many steps were taken since — a
        SkippedStep, or None if no step was skipped since construction / load_state_dict (or the latch does not exist).  One
        synchronising readback; `names` as for `grad_report`."""
        if self._latch is None:
            return None
        latch = self._latch.cpu()
        skipped, attempt, first, largest, bad = (x & 0xffffffff for x in latch[:5].tolist())
        if skipped == 0:
            return None
        stats = _stats_rows(latch[LATCH_HEADER:].view(-1, 4), self._report_names(names))
        return SkippedStep(attempt, skipped, None if first == 0xffffffff else stats[first],
                           None if largest == 0xffffffff else stats[largest], bad, stats)

    def note_replayed_steps(self, n=1):
        """A captured graph that contains this optimizer's step was replayed n times: advance the host-side step counts (the
        device counters advanced inside the graph).  With the guard on the host count is the ATTEMPTED steps; the device count,
        which skipped steps do not advance, is the one the kernel uses."""
        stepped = []
        for p, st in self.state.items():
            if "step" in st:
                st["step"] += n
                stepped.append(p)
        if n > 0 and stepped:     # the replay rewrote them without any version counter noticing
            torch.autograd.graph.increment_version(stepped)

    def state_dict(self):
        sd = super().state_dict()
        skipped = self.skipped_steps        # guarded: `step` = attempted - skipped, the steps that were taken
        sd["state"] = {k: {**v, "step": torch.tensor(float(v["step"] - skipped), dtype=torch.float32)} if "step" in v else v
                       for k, v in sd["state"].items()}
        return sd

    def load_state_dict(self, state_dict):
        super().load_state_dict(state_dict)
        for st in self.state.values():
            if "step" in st:
                st["step"] = int(round(float(st["step"])))
        self._step_dev = {}       # re-created from the loaded step counts at the next capturable step
        if self._guarded:
            self._reset_guard()   # the guard record (skipped = 0) and its step count, from the loaded step counts; the report, zeroed
        if self._hyper_on_device:
            self._reset_hyper()   # the hyper record and its mirror, from the loaded param_groups


class AdamW(Adam):
    """torch.optim.AdamW on the same multi-tensor step: `Adam` with the decoupled weight decay (a non-zero `weight_decay` multiplies the
    parameter by 1 - lr * weight_decay in front of the moments and is not added to the gradient) and torch.optim.AdamW's default
    `weight_decay=1e-2`.  Every other argument, option and method is `Adam`'s; `state_dict()` is interchangeable with
    torch.optim.AdamW's."""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, amsgrad=False, maximize=False, **options):
        if "decoupled_weight_decay" in options:
            raise TypeError("wsmgmap.optim.AdamW is the decoupled form: it takes no decoupled_weight_decay argument")
        super().__init__(params, lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, amsgrad=amsgrad, maximize=maximize,
                         decoupled_weight_decay=True, **options)
