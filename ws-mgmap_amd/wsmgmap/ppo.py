"""The PPO update after DAgger: habitat-baselines' `PPO` by constructor, attribute and method name, restated (habitat-baselines is
not a dependency and no version of it is pinned: DESIGN.md §2).  It calls, in sequence, what the package already has:
`RolloutStorage.get_advantages` and `recurrent_generator` (each minibatch one launch: ops.gather_columns), the policy's
`evaluate_actions` (ops.eval_heads), `ops.ppo_loss` and `wsmgmap.optim.Adam`, whose device-side guard does the clipping.

What differs from the stock class, and only in cost: no `.item()` per minibatch (the five sums live in one device tensor that is
read once per update), no rewrite of `p.grad` by `clip_grad_norm_` (the Adam step reads g * min(1, max_grad_norm / |g|)), and
minibatch tensors that are views of staging buffers of the storage.  For a policy on the CPU the same update is composed from
torch (`torch.optim.Adam`, `clip_grad_norm_`, the loss written out): the stock arm of the tests, not a product path."""
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


class PPO(nn.Module):
    """PPO(actor_critic, clip_param, ppo_epoch, num_mini_batch, value_loss_coef, entropy_coef, lr, eps, max_grad_norm, ...).

    actor_critic: a policy with `evaluate_actions(observations, rnn_hidden_states, prev_actions, masks, action) -> (value,
    action_log_probs, dist_entropy, rnn_hidden_states)`.  `optimizer`: wsmgmap.optim.Adam over the parameters that require grad,
    with `max_grad_norm` as its device-side guard and `optimizer_options` (skip_nonfinite, grad_report, ...) passed through; for
    parameters on the CPU torch.optim.Adam, with `clip_grad_norm_` in front of its step."""

    def __init__(self, actor_critic, clip_param, ppo_epoch, num_mini_batch, value_loss_coef, entropy_coef, lr=None, eps=None,
                 max_grad_norm=None, use_clipped_value_loss=True, use_normalized_advantage=True, **optimizer_options):
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
        params = [p for p in actor_critic.parameters() if p.requires_grad]
        if not params:
            raise ValueError("PPO: the policy has no parameter that requires grad")
        self.device = params[0].device
        given = {k: v for k, v in (("lr", lr), ("eps", eps)) if v is not None}
        if self.device.type == "cuda":
            self.optimizer = Adam(params, max_grad_norm=max_grad_norm, **given, **optimizer_options)
        else:
            self.optimizer = torch.optim.Adam(params, **given, **optimizer_options)
        self.last_stats = {}

    def forward(self, *x):
        raise NotImplementedError

    def get_advantages(self, rollouts):
        return rollouts.get_advantages(self.use_normalized_advantage)

    def update(self, rollouts):
        """ppo_epoch passes over the rollout in num_mini_batch minibatches, an optimizer step each -> (value_loss_epoch,
        action_loss_epoch, dist_entropy_epoch), the means over the steps, as Python floats.  `last_stats` keeps them with the means
        of clip_frac and approx_kl and the last step's gradient norm before clipping (None without max_grad_norm / a guarded
        step).  The one device-to-host copy of the update is the read of those figures at its end.  `rollouts.after_update()` is the
        caller's, as in habitat."""
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

    # habitat's hooks: no-ops here (after_backward is where a GradAllReducer's finish() goes)
    def before_backward(self, loss):
        pass

    def after_backward(self, loss):
        pass

    def before_step(self):
        pass

    def after_step(self):
        pass
