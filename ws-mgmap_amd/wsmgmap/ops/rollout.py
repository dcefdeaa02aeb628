"""wsmgmap.ops.rollout — the rollout's returns and advantages in one launch (csrc/wsmg_pg_rollout.hip): habitat-baselines'
`RolloutStorage.compute_returns` + `PPO.get_advantages`, restated.  No autograd: none of these quantities is differentiated in PPO.
"""
import torch

from .. import _abi
from .core import _p, _stream, _req, _f32

GAE_MAX_ENVS = 1024          # GAE_MAXN of csrc/wsmg_pg_rollout.hip: one workgroup, a thread per environment, four columns each
GAE_MAX_ENTRIES = 1 << 24    # T N must stay below it


def gae_returns_ok(rewards, T=None):
    """Can `gae_returns` take this rollout?  float32 on the GPU, at least one step, at most GAE_MAX_ENVS environments and fewer than
    GAE_MAX_ENTRIES step x environment entries.  rewards [T', N, ...]; T: the steps in use (default: all T')."""
    T = rewards.shape[0] if T is None else T
    N = rewards.numel() // rewards.shape[0] if rewards.dim() >= 2 and rewards.shape[0] else 0
    return rewards.is_cuda and rewards.dtype == torch.float32 and T >= 1 and 1 <= N <= GAE_MAX_ENVS and T * N < GAE_MAX_ENTRIES


def _rows(name, t, rows, N):
    """t is [rows, N] with any number of trailing 1s ([rows, N, 1] as the storage keeps it)."""
    if t.dim() < 2 or t.shape[0] != rows or t.shape[1] != N or t.numel() != rows * N:
        raise _abi.WsmgError(f"gae_returns: {name} must be [{rows}, {N}] or [{rows}, {N}, 1], got {tuple(t.shape)}")


@torch.no_grad()
def gae_returns(rewards, value_preds, masks, next_value, gamma, tau, use_gae=True, eps=1e-5, out=None):
    """-> (returns [T+1, N, ...], adv [T, N, ...], adv_norm [T, N, ...], stats float64 [2] = {mean, std of adv}), one launch.

        use_gae:  value_preds[T] = next_value (value_preds is WRITTEN);  g = 0;  for s = T-1 .. 0:
                      d = rewards[s] + gamma * value_preds[s+1] * masks[s+1] - value_preds[s]
                      g = d + gamma * tau * masks[s+1] * g;   returns[s] = g + value_preds[s]       (returns[T] is left as it was)
        else:     returns[T] = next_value;  for s = T-1 .. 0:  returns[s] = returns[s+1] * gamma * masks[s+1] + rewards[s]
        adv = returns[:T] - value_preds[:T];   adv_norm = (adv - adv.mean()) / (adv.std() + eps)

    returns, adv and value_preds[T] are the bits of that float32 torch loop on the CPU (gamma * tau is formed in double and rounded
    once, as torch does with two Python floats); the statistics are float64 sums in a fixed order.
    rewards [T, N] or [T, N, 1]; value_preds and masks [T+1, N(, 1)]; next_value with N elements: contiguous float32 GPU tensors,
    1 <= N <= GAE_MAX_ENVS, T >= 1, T N < GAE_MAX_ENTRIES.  out = (returns, adv, adv_norm, stats): tensors to write into; an entry
    that is None is allocated (returns as zeros: its row T is not written under GAE), and nothing is allocated when all four are
    given."""
    _req(rewards, value_preds, masks, next_value)
    _f32(rewards, value_preds, masks, next_value)
    if rewards.dim() < 2 or rewards.shape[0] < 1 or rewards.shape[1] < 1 or rewards.numel() != rewards.shape[0] * rewards.shape[1]:
        raise _abi.WsmgError(f"gae_returns: rewards must be [T, N] or [T, N, 1] with T, N >= 1, got {tuple(rewards.shape)}")
    T, N = rewards.shape[0], rewards.shape[1]
    if N > GAE_MAX_ENVS or T * N >= GAE_MAX_ENTRIES:
        raise _abi.WsmgError(f"gae_returns: at most {GAE_MAX_ENVS} environments and fewer than {GAE_MAX_ENTRIES} entries, got T = {T}, N = {N}")
    _rows("value_preds", value_preds, T + 1, N)
    _rows("masks", masks, T + 1, N)
    if next_value.numel() != N:
        raise _abi.WsmgError(f"gae_returns: next_value must have one element per environment ({N}), got {tuple(next_value.shape)}")
    returns, adv, adv_norm, stats = out if out is not None else (None, None, None, None)
    _req(returns, adv, adv_norm, stats)
    _f32(returns, adv, adv_norm)
    dev = rewards.device
    if returns is None:
        returns = torch.zeros_like(value_preds)
    if adv is None:
        adv = torch.empty_like(rewards)
    if adv_norm is None:
        adv_norm = torch.empty_like(rewards)
    if stats is None:
        stats = torch.empty(2, device=dev, dtype=torch.float64)
    _rows("returns", returns, T + 1, N)
    _rows("adv", adv, T, N)
    _rows("adv_norm", adv_norm, T, N)
    if stats.dtype != torch.float64 or stats.numel() != 2:
        raise _abi.WsmgError(f"gae_returns: stats must be float64 [2], got {stats.dtype} {tuple(stats.shape)}")
    _abi.call("wsmg_gae_returns", _p(rewards), _p(value_preds), _p(masks), _p(next_value), float(gamma), float(gamma) * float(tau),
              int(bool(use_gae)), T, N, _p(returns), _p(adv), _p(adv_norm), _p(stats), float(eps), _stream())
    return returns, adv, adv_norm, stats
