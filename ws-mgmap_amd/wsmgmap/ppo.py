"""The PPO update after DAgger: habitat-baselines' `PPO` by constructor, attribute and method name, restated (habitat-baselines is
not a dependency and no version of it is pinned: DESIGN.md §2).  It calls, in sequence, what the package already has:
`RolloutStorage.get_advantages` and `recurrent_generator` (each minibatch one launch: ops.gather_columns), the policy's
`evaluate_actions` (ops.eval_heads), `ops.ppo_loss` and `wsmgmap.optim.Adam`, whose device-side guard does the clipping.

What differs from the stock class, and only in cost: no `.item()` per minibatch (the five sums live in one device tensor that is
read once per update), no rewrite of `p.grad` by `clip_grad_norm_` (the Adam step reads g * min(1, max_grad_norm / |g|)), and
minibatch tensors that are views of staging buffers of the storage.  For a policy on the CPU the same update is composed from
torch (`torch.optim.Adam`, `clip_grad_norm_`, the loss written out): the stock arm of the tests, not a product path.

`PPO(target_kl=...)` adds Spinning Up's early stop without giving that up: the decision is taken in the loss kernel and obeyed by the
optimizer's guarded step on the device (`ops.ppo_loss(gate=...)`, `Adam.set_step_gate`), and reaches the host with the same one read."""
import torch
import torch.nn as nn

from . import ops
from .optim import Adam

STAT_NAMES = ("value_loss", "action_loss", "dist_entropy", "clip_frac", "approx_kl")


def ppo_loss_torch(logp, old_logp, adv, value, old_value, returns, entropy, clip, value_coef, entropy_coef, clipped_value=True):
    """`ops.ppo_loss` composed in torch, habitat-baselines' expressions in their order -> the same five 0-dim tensors."""
    logp, old_logp, adv, value, old_value, returns = (t.reshape(-1) for t in (logp, old_logp, adv, value, old_value, returns))
    ratio = torch.exp(logp - old_logp)
    surr1 = ratio * adv
    surr2 = torch.clamp(ratio, 1.0 - clip, 1.0 + clip) * adv
    action_loss = -torch.min(surr1, surr2).mean()
    if clipped_value:
        value_pred_clipped = old_value + (value - old_value).clamp(-clip, clip)
        value_loss = 0.5 * torch.max((value - returns).pow(2), (value_pred_clipped - returns).pow(2)).mean()
    else:
        value_loss = 0.5 * (returns - value).pow(2).mean()
    loss = value_loss * value_coef + action_loss - entropy.reshape(()) * entropy_coef
    with torch.no_grad():
        clip_frac = ((ratio - 1.0).abs() > clip).to(ratio.dtype).mean()
        approx_kl = (old_logp - logp).mean()
    return loss, action_loss, value_loss, clip_frac, approx_kl


def _bn_buffers(module):
    """The running statistics a train-mode forward writes: running_mean, running_var, num_batches_tracked of every BatchNorm layer
    below `module` that tracks them (what `Adam(guard_buffers=module)` protects)."""
    return [b for m in module.modules() if isinstance(m, nn.modules.batchnorm._BatchNorm) and m.track_running_stats
            for b in (m.running_mean, m.running_var, m.num_batches_tracked) if b is not None]


class PPO(nn.Module):
    """PPO(actor_critic, clip_param, ppo_epoch, num_mini_batch, value_loss_coef, entropy_coef, lr, eps, max_grad_norm, ...).

    actor_critic: a policy with `evaluate_actions(observations, rnn_hidden_states, prev_actions, masks, action) -> (value,
    action_log_probs, dist_entropy, rnn_hidden_states)`.  `optimizer`: wsmgmap.optim.Adam over the parameters that require grad,
    with `max_grad_norm` as its device-side guard and `optimizer_options` (skip_nonfinite, grad_report, ...) passed through; for
    parameters on the CPU torch.optim.Adam, with `clip_grad_norm_` in front of its step.

    target_kl (None: every minibatch steps, as in habitat): Spinning Up's early stop.  With limit = float32(1.5 * target_kl), in
    minibatch order: once a minibatch's approx_kl = mean(old_logp - logp) exceeds the limit the update has stopped, and that
    minibatch and every later one of the update takes no optimizer step, adds nothing to the statistics, and leaves the BatchNorm
    running statistics as they were before its forward.  A NaN approx_kl stops nothing (the comparison is false).  On the GPU the
    decision never reaches the host: `ops.ppo_loss(gate=...)` latches it in a device record, the optimizer's guarded step obeys the
    record (`Adam.set_step_gate`), and the same kernel adds the five figures of the steps taken into the sums — so the loop cannot
    `break`, runs every minibatch and draws the generator for every epoch exactly as without a limit.  The optimizer is then always
    guarded: `skip_nonfinite=True` is passed unless the caller said otherwise, and `guard_buffers=actor_critic` when the policy has
    BatchNorm layers that track running statistics (the roll-back needs both; `skip_nonfinite=False` with such a policy is refused by
    `Adam`).  A step that the non-finite guard skips is still counted in `steps_taken` and the statistics, as it is without a limit.

    kl_sync (needs target_kl): None — no synchronisation, as above; "epoch" — the one `stopped` word is read after each epoch and a
    stopped update returns there: one small copy per epoch for the compute it saves.  What it leaves (parameters, moments, BatchNorm
    buffers, statistics) is the same, bit for bit; only the generator's draws differ."""

    def __init__(self, actor_critic, clip_param, ppo_epoch, num_mini_batch, value_loss_coef, entropy_coef, lr=None, eps=None,
                 max_grad_norm=None, use_clipped_value_loss=True, use_normalized_advantage=True, target_kl=None, kl_sync=None,
                 **optimizer_options):
        super().__init__()
        self.actor_critic = actor_critic
        self.clip_param = clip_param
        self.ppo_epoch = ppo_epoch
        self.num_mini_batch = num_mini_batch
        self.value_loss_coef = value_loss_coef
        self.entropy_coef = entropy_coef
        self.max_grad_norm = max_grad_norm
        self.use_clipped_value_loss = use_clipped_value_loss
        self.use_normalized_advantage = use_normalized_advantage
        if target_kl is not None:
            target_kl = float(target_kl)
            if target_kl != target_kl:
                raise ValueError("PPO: target_kl is NaN (None for no early stop, inf for a limit that is never reached)")
        if kl_sync not in (None, "epoch"):
            raise ValueError(f"PPO: kl_sync must be None or 'epoch', got {kl_sync!r}")
        if kl_sync is not None and target_kl is None:
            raise ValueError("PPO: kl_sync needs a target_kl (there is no stop to look for)")
        self.target_kl = target_kl
        self.kl_sync = kl_sync
        self.kl_limit = None if target_kl is None else ops.kl_limit_of(target_kl)      # float32(1.5 * target_kl)
        params = [p for p in actor_critic.parameters() if p.requires_grad]
        if not params:
            raise ValueError("PPO: the policy has no parameter that requires grad")
        self.device = params[0].device
        given = {k: v for k, v in (("lr", lr), ("eps", eps)) if v is not None}
        self._kl_buf = None       # target_kl on the GPU: the five sums, the last gradient norm, then the KL gate record
        if self.device.type == "cuda":
            if target_kl is not None:
                optimizer_options = dict(optimizer_options)
                optimizer_options.setdefault("skip_nonfinite", True)
                if "guard_buffers" not in optimizer_options and _bn_buffers(actor_critic):
                    optimizer_options["guard_buffers"] = actor_critic
            self.optimizer = Adam(params, max_grad_norm=max_grad_norm, **given, **optimizer_options)
            if target_kl is not None:
                with torch.cuda.device(self.device):
                    self._kl_buf = torch.zeros(len(STAT_NAMES) + 1 + ops.KL_GATE, device=self.device)
                self.optimizer.set_step_gate(self._kl_gate)
        else:
            self.optimizer = torch.optim.Adam(params, **given, **optimizer_options)
        self.last_stats = {}

    @property
    def _kl_gate(self):
        """The KL gate record (ops.KL_GATE words), a view of the update's one device buffer behind the sums and the norm."""
        return self._kl_buf[len(STAT_NAMES) + 1:]

    def forward(self, *x):
        raise NotImplementedError

    def get_advantages(self, rollouts):
        return rollouts.get_advantages(self.use_normalized_advantage)

    def update(self, rollouts):
        """ppo_epoch passes over the rollout in num_mini_batch minibatches, an optimizer step each -> (value_loss_epoch,
        action_loss_epoch, dist_entropy_epoch), the means over the steps, as Python floats.  `last_stats` keeps them with the means
        of clip_frac and approx_kl and the last step's gradient norm before clipping (None without max_grad_norm / a guarded
        step).  The one device-to-host copy of the update is the read of those figures at its end.  `rollouts.after_update()` is the
        caller's, as in habitat.

        With target_kl the means run over the steps TAKEN (NaN if there was none, and grad_norm is then None), grad_norm is the last
        taken step's, and `last_stats` also holds `steps_taken`, `stopped`, and — None unless stopped — `stop_ordinal` (the minibatch
        that tripped the limit, counted from 0 within the update; it is itself not stepped) and `stop_kl` (its approx_kl).  The read
        at the end carries the gate record too; kl_sync="epoch" adds one read of one word per epoch."""
        if self.target_kl is not None:
            return self._update_kl(rollouts)
        advantages = self.get_advantages(rollouts)
        on_gpu = self.device.type == "cuda"
        sums = torch.zeros(len(STAT_NAMES) + 1, device=self.device)          # the five sums, then the last gradient norm
        params = [p for g in self.optimizer.param_groups for p in g["params"]]
        grad_norm = None
        for _ in range(self.ppo_epoch):
            for sample in rollouts.recurrent_generator(advantages, self.num_mini_batch, reuse_buffers=True):
                (obs_batch, recurrent_hidden_states_batch, actions_batch, prev_actions_batch, value_preds_batch, return_batch,
                 masks_batch, old_action_log_probs_batch, adv_targ) = sample
                values, action_log_probs, dist_entropy, _ = self.actor_critic.evaluate_actions(
                    obs_batch, recurrent_hidden_states_batch, prev_actions_batch, masks_batch, actions_batch)
                loss_fn = ops.ppo_loss if action_log_probs.is_cuda else ppo_loss_torch
                total_loss, action_loss, value_loss, clip_frac, approx_kl = loss_fn(
                    action_log_probs, old_action_log_probs_batch, adv_targ, values, value_preds_batch, return_batch, dist_entropy,
                    self.clip_param, self.value_loss_coef, self.entropy_coef, clipped_value=self.use_clipped_value_loss)
                self.optimizer.zero_grad()
                self.before_backward(total_loss)
                total_loss.backward()
                self.after_backward(total_loss)
                self.before_step()
                if not on_gpu and self.max_grad_norm is not None:
                    grad_norm = nn.utils.clip_grad_norm_(params, self.max_grad_norm)
                self.optimizer.step()
                self.after_step()
                with torch.no_grad():
                    sums[:len(STAT_NAMES)] += torch.stack([t.detach().reshape(()).to(sums.dtype) for t in
                                                           (value_loss, action_loss, dist_entropy, clip_frac, approx_kl)])
        if on_gpu:
            grad_norm = self.optimizer.grad_norm
        if grad_norm is not None:
            sums[len(STAT_NAMES)] = grad_norm.detach()
        host = sums.tolist()                                                  # THE read of the update
        steps = self.ppo_epoch * self.num_mini_batch
        self.last_stats = {k: v / steps for k, v in zip(STAT_NAMES, host)}
        self.last_stats["grad_norm"] = None if grad_norm is None else host[len(STAT_NAMES)]
        return tuple(self.last_stats[k] for k in STAT_NAMES[:3])

    def _update_kl(self, rollouts):
        """`update` with a target_kl: the same minibatches behind the early stop (the class docstring has the rule)."""
        advantages = self.get_advantages(rollouts)
        on_gpu = self.device.type == "cuda"
        n = len(STAT_NAMES)
        params = [p for g in self.optimizer.param_groups for p in g["params"]]
        if on_gpu:
            buf = self._kl_buf
            buf.zero_()           # one device fill: the sums and the gate record (stopped = 0, no step taken, ordinal 0)
            sums, gate = buf[:n], self._kl_gate
        else:
            sums = torch.zeros(n)
            bn = _bn_buffers(self.actor_critic)
        stopped, taken, seen, stop_ordinal, stop_kl, grad_norm = False, 0, 0, None, None, None
        for _ in range(self.ppo_epoch):
            for sample in rollouts.recurrent_generator(advantages, self.num_mini_batch, reuse_buffers=True):
                (obs_batch, recurrent_hidden_states_batch, actions_batch, prev_actions_batch, value_preds_batch, return_batch,
                 masks_batch, old_action_log_probs_batch, adv_targ) = sample
                if on_gpu:
                    self.optimizer.zero_grad()        # (in front of the forward: with guard_buffers it snapshots what the forward writes)
                else:
                    saved = [b.clone() for b in bn]
                values, action_log_probs, dist_entropy, _ = self.actor_critic.evaluate_actions(
                    obs_batch, recurrent_hidden_states_batch, prev_actions_batch, masks_batch, actions_batch)
                if on_gpu:
                    total_loss = ops.ppo_loss(
                        action_log_probs, old_action_log_probs_batch, adv_targ, values, value_preds_batch, return_batch, dist_entropy,
                        self.clip_param, self.value_loss_coef, self.entropy_coef, clipped_value=self.use_clipped_value_loss,
                        gate=gate, sums=sums, kl_limit=self.kl_limit)[0]
                else:
                    total_loss, action_loss, value_loss, clip_frac, approx_kl = ppo_loss_torch(
                        action_log_probs, old_action_log_probs_batch, adv_targ, values, value_preds_batch, return_batch, dist_entropy,
                        self.clip_param, self.value_loss_coef, self.entropy_coef, clipped_value=self.use_clipped_value_loss)
                    kl = approx_kl.detach().float()
                    if not stopped and bool(kl > self.kl_limit):
                        stopped, stop_ordinal, stop_kl = True, seen, float(kl)
                    seen += 1
                    self.optimizer.zero_grad()
                self.before_backward(total_loss)
                total_loss.backward()
                self.after_backward(total_loss)
                self.before_step()
                if on_gpu:
                    self.optimizer.step()             # the gate's word decides on the device whether anything is written
                elif stopped:
                    with torch.no_grad():
                        for b, s in zip(bn, saved):
                            b.copy_(s)
                else:
                    if self.max_grad_norm is not None:
                        grad_norm = nn.utils.clip_grad_norm_(params, self.max_grad_norm)
                    self.optimizer.step()
                    taken += 1
                    with torch.no_grad():
                        sums += torch.stack([t.detach().reshape(()).to(sums.dtype) for t in
                                             (value_loss, action_loss, dist_entropy, clip_frac, approx_kl)])
                self.after_step()
            if self.kl_sync == "epoch" and (bool(gate[ops.KL_STOPPED].item() != 0.0) if on_gpu else stopped):
                break
        if on_gpu:
            buf[n] = self.optimizer.grad_norm.detach()
            host = buf.tolist()                                               # THE read of the update: sums, norm, gate record
            rec = host[n + 1:]
            stopped, taken = rec[ops.KL_STOPPED] != 0.0, int(rec[ops.KL_TAKEN])
            if stopped:
                stop_ordinal, stop_kl = int(rec[ops.KL_STOP_ORDINAL]), rec[ops.KL_STOP_KL]
            grad_norm = host[n] if taken else None
        else:
            host = sums.tolist()
            grad_norm = None if grad_norm is None else float(grad_norm)
        self.last_stats = {k: (v / taken if taken else float("nan")) for k, v in zip(STAT_NAMES, host)}
        self.last_stats.update(grad_norm=grad_norm, steps_taken=taken, stopped=stopped, stop_ordinal=stop_ordinal, stop_kl=stop_kl)
        return tuple(self.last_stats[k] for k in STAT_NAMES[:3])

    # habitat's hooks: no-ops here (after_backward is where a GradAllReducer's finish() goes)
    def before_backward(self, loss):
        pass

    def after_backward(self, loss):
        pass

    def before_step(self):
        pass

    def after_step(self):
        pass
