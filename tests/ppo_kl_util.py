"""The yardstick of `wsmgmap.ppo.PPO(target_kl=...)`: Spinning Up's early stop, written out as the loop a user writes today, with a
host read of every minibatch's approx_kl and a host `if`:

    limit = float32(1.5 * target_kl)                  formed in double, rounded once
    for every minibatch, in order (tests/ppo_util.py's loop: the stock generator, drawn for every epoch):
        the BatchNorm running statistics are cloned;  evaluate_actions, the loss and its five figures
        if not stopped and approx_kl > limit:  stopped = True                      approx_kl: the float32 the loss returned
        if stopped:  the clones are copied back; no step, no statistics
        else:        zero_grad, backward, [CPU: clip_grad_norm_], step; the five figures are added to the float32 sums; steps_taken += 1
    -> the means over steps_taken (NaN for none), steps_taken, stopped, the stopping minibatch's ordinal and approx_kl, the last taken
       step's gradient norm, and every minibatch's approx_kl

The optimizer is the one tests/ppo_util.py's loop takes — `wsmgmap.optim.Adam(max_grad_norm=...)` on the GPU, with no gate and no
BatchNorm protection of its own, `torch.optim.Adam` on the CPU — so nothing of what this file is the yardstick for runs in it."""
import numpy as np
import torch
import torch.nn as nn

import ppo_util as pu


def limit_of(target_kl):
    """float32(1.5 * target_kl) with numpy: the product in double, one rounding."""
    return np.float32(1.5 * float(target_kl))


def bn_buffers(module):
    """{name: tensor}: running_mean, running_var, num_batches_tracked of every BatchNorm layer below module that tracks them."""
    out = {}
    for mname, m in module.named_modules():
        if isinstance(m, nn.modules.batchnorm._BatchNorm) and m.track_running_stats:
            for b in ("running_mean", "running_var", "num_batches_tracked"):
                if getattr(m, b) is not None:
                    out[f"{mname}.{b}"] = getattr(m, b)
    return out


def written_out_kl_update(policy, rollouts, optimizer, clip_param, ppo_epoch, num_mini_batch, value_loss_coef, entropy_coef,
                          target_kl=None, limit=None, max_grad_norm=None, use_clipped_value_loss=True, use_normalized_advantage=True):
    """The loop of the module docstring -> dict.  `limit` (a float32 value) stands for float32(1.5 * target_kl) when given."""
    from wsmgmap import ops
    limit = limit_of(target_kl) if limit is None else np.float32(limit)
    params = [p for g in optimizer.param_groups for p in g["params"]]
    bufs = list(bn_buffers(policy).values())
    advantages = rollouts.get_advantages(use_normalized_advantage)
    sums = torch.zeros(len(pu.STATS), device=params[0].device)
    stopped, taken, stop_ordinal, stop_kl, grad_norm, kls = False, 0, None, None, None, []
    for _ in range(ppo_epoch):
        for obs, hidden, actions, prev_actions, value_preds, returns, masks, old_logp, adv in rollouts.recurrent_generator(
                advantages, num_mini_batch):
            saved = [b.clone() for b in bufs]
            values, logp, entropy, _ = policy.evaluate_actions(obs, hidden, prev_actions, masks, actions)
            if logp.is_cuda:
                loss, action_loss, value_loss, clip_frac, approx_kl = ops.ppo_loss(
                    logp, old_logp, adv, values, value_preds, returns, entropy, clip_param, value_loss_coef, entropy_coef,
                    clipped_value=use_clipped_value_loss)
            else:
                loss, action_loss, value_loss, clip_frac, approx_kl = pu.ppo_loss_written_out(
                    logp, old_logp, adv, values, value_preds, returns, entropy, clip_param, value_loss_coef, entropy_coef,
                    use_clipped_value_loss)
            kl = approx_kl.detach().float().cpu().numpy().reshape(())[()]          # the host read
            assert kl.dtype == np.float32
            if not stopped and kl > limit:
                stopped, stop_ordinal, stop_kl = True, len(kls), float(kl)
            kls.append(float(kl))
            if stopped:
                with torch.no_grad():
                    for b, s in zip(bufs, saved):
                        b.copy_(s)
                continue
            optimizer.zero_grad()
            loss.backward()
            if logp.is_cuda:
                optimizer.step()
                grad_norm = optimizer.grad_norm
            else:
                if max_grad_norm is not None:
                    grad_norm = nn.utils.clip_grad_norm_(params, max_grad_norm)
                optimizer.step()
            grad_norm = None if grad_norm is None else float(grad_norm)
            taken += 1
            with torch.no_grad():
                sums += torch.stack([t.detach().reshape(()).float() for t in (value_loss, action_loss, entropy, clip_frac, approx_kl)])
    out = {k: (v / taken if taken else float("nan")) for k, v in zip(pu.STATS, sums.tolist())}
    out.update(steps_taken=taken, stopped=stopped, stop_ordinal=stop_ordinal, stop_kl=stop_kl, grad_norm=grad_norm, kls=kls)
    return out


def same_stats(got, want, keys=pu.STATS):
    """Equal Python floats, NaN equal to NaN."""
    return all((got[k] == want[k]) or (got[k] != got[k] and want[k] != want[k]) for k in keys)


def first_running_maximum(kls):
    """The first ordinal k >= 1 whose approx_kl exceeds every earlier one -> (k, the largest earlier one), or None."""
    for k in range(1, len(kls)):
        if kls[k] > max(kls[:k]):
            return k, max(kls[:k])
    return None


def target_between(lo, hi):
    """A target_kl whose limit float32(1.5 * target_kl) satisfies lo <= limit < hi (lo < hi float32 values): the midpoint's, or lo's
    own when the two are neighbours."""
    for want in (0.5 * (float(lo) + float(hi)), float(lo)):
        t = want / 1.5
        if np.float32(lo) <= limit_of(t) < np.float32(hi):
            return t
    raise AssertionError((lo, hi))
