"""wsmgmap.ops.rollout — the rollout's returns and advantages in one launch (csrc/wsmg_pg_rollout.hip): habitat-baselines'
`RolloutStorage.compute_returns` + `PPO.get_advantages`, restated; and a minibatch of its `recurrent_generator` in one launch
(csrc/wsmg_rollout_gather.hip).  No autograd: none of these quantities is differentiated in PPO.
"""
import ctypes

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


def _rows(name, t, rows, N, op="gae_returns"):
    """t is [rows, N] with any number of trailing 1s ([rows, N, 1] as the storage keeps it)."""
    if t.dim() < 2 or t.shape[0] != rows or t.shape[1] != N or t.numel() != rows * N:
        raise _abi.WsmgError(f"{op}: {name} must be [{rows}, {N}] or [{rows}, {N}, 1], got {tuple(t.shape)}")


def _rollout_shape(op, rewards):
    """(T, N) of rewards [T, N] or [T, N, 1] inside the kernels' limits."""
    if rewards.dim() < 2 or rewards.shape[0] < 1 or rewards.shape[1] < 1 or rewards.numel() != rewards.shape[0] * rewards.shape[1]:
        raise _abi.WsmgError(f"{op}: rewards must be [T, N] or [T, N, 1] with T, N >= 1, got {tuple(rewards.shape)}")
    T, N = rewards.shape[0], rewards.shape[1]
    if N > GAE_MAX_ENVS or T * N >= GAE_MAX_ENTRIES:
        raise _abi.WsmgError(f"{op}: at most {GAE_MAX_ENVS} environments and fewer than {GAE_MAX_ENTRIES} entries, got T = {T}, N = {N}")
    return T, N


def _gae_operands(op, rewards, value_preds, masks, next_value, out):
    """The checks of `gae_returns` on its operands and `out`; -> (T, N, returns, adv, adv_norm, stats), what `out` left out allocated."""
    _req(rewards, value_preds, masks, next_value)
    _f32(rewards, value_preds, masks, next_value)
    T, N = _rollout_shape(op, rewards)
    _rows("value_preds", value_preds, T + 1, N, op)
    _rows("masks", masks, T + 1, N, op)
    if next_value.numel() != N:
        raise _abi.WsmgError(f"{op}: next_value must have one element per environment ({N}), got {tuple(next_value.shape)}")
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
    _rows("returns", returns, T + 1, N, op)
    _rows("adv", adv, T, N, op)
    _rows("adv_norm", adv_norm, T, N, op)
    if stats.dtype != torch.float64 or stats.numel() != 2:
        raise _abi.WsmgError(f"{op}: stats must be float64 [2], got {stats.dtype} {tuple(stats.shape)}")
    return T, N, returns, adv, adv_norm, stats


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
    T, N, returns, adv, adv_norm, stats = _gae_operands("gae_returns", rewards, value_preds, masks, next_value, out)
    _abi.call("wsmg_gae_returns", _p(rewards), _p(value_preds), _p(masks), _p(next_value), float(gamma), float(gamma) * float(tau),
              int(bool(use_gae)), T, N, _p(returns), _p(adv), _p(adv_norm), _p(stats), float(eps), _stream())
    return returns, adv, adv_norm, stats


def reward_normalize_ok(rewards, masks, state, T=None):
    """Can `normalize_rewards` take this rollout?  `gae_returns_ok`, float32 masks and a float64 state [3 + N] beside the rewards."""
    T = rewards.shape[0] if T is None else T
    return (gae_returns_ok(rewards, T) and masks.is_cuda and masks.dtype == torch.float32 and state.device == rewards.device
            and state.dtype == torch.float64 and state.numel() == 3 + rewards.numel() // rewards.shape[0])


def _norm_operands(op, rewards, masks, state, first_row, out, T, N):
    """The normaliser's operands beside float32 GPU rewards [T, N]; -> out (zeros where it was None)."""
    _req(masks, state, out)
    _f32(masks, out)
    _rows("masks", masks, T + 1, N, op)
    if state.dtype != torch.float64 or state.dim() != 1 or state.numel() != 3 + N:
        raise _abi.WsmgError(f"{op}: state must be float64 [3 + {N}] = (mean, var, count, returns), got {state.dtype} {tuple(state.shape)}")
    first_row = int(first_row)
    if not 0 <= first_row <= T:
        raise _abi.WsmgError(f"{op}: first_row = {first_row} is outside [0, {T}]")
    if out is None:
        out = torch.zeros_like(rewards)
    _rows("rewards_out", out, T, N, op)
    return first_row, out


@torch.no_grad()
def normalize_rewards(rewards, masks, state, gamma, clip, eps, *, first_row=0, update=True, out=None):
    """-> out [T, N, ...]: rewards divided by the running standard deviation of the discounted return, one launch; rows
    [first_row, T) of `out` are written and `state` advanced in place (baselines' `VecNormalize` return path, restated).

        state = {mean, var, count, ret[N]} float64;  for s = first_row .. T-1, in float64:
            ret = ret * gamma + rewards[s];   mean, var, count <- merged with ret's mean and sum of squared deviations over n
            out[s] = float32(clamp(rewards[s] / sqrt(var + eps), -clip, clip));   ret *= masks[s+1]
        update=False: only the `out` line, with the stored var; state is not written.

    rewards [T, N] or [T, N, 1], masks [T+1, N(, 1)]: contiguous float32 GPU tensors inside `gae_returns`' limits; state: float64
    [3 + N] on the same device.  gamma, clip and eps reach the kernel as float32.  out: the tensor to write into (default: zeros)."""
    _req(rewards)
    _f32(rewards)
    T, N = _rollout_shape("normalize_rewards", rewards)
    first_row, out = _norm_operands("normalize_rewards", rewards, masks, state, first_row, out, T, N)
    _abi.call("wsmg_reward_normalize", _p(rewards), _p(masks), _p(state), float(gamma), float(clip), float(eps), T, N, first_row,
              int(bool(update)), _p(out), _stream())
    return out


@torch.no_grad()
def normalized_gae_returns(rewards, value_preds, masks, next_value, gamma, tau, state, norm_gamma, clip, norm_eps, *, use_gae=True,
                           eps=1e-5, first_row=0, update=True, rewards_out=None, out=None):
    """`normalize_rewards(rewards, masks, state, norm_gamma, clip, norm_eps, first_row=, update=, out=rewards_out)` followed by
    `gae_returns(rewards_out, value_preds, masks, next_value, gamma, tau, use_gae, eps, out)` in ONE launch, with the bits of the two.
    -> (returns, adv, adv_norm, stats, rewards_out).  Rows [:first_row] of rewards_out are read as an earlier call left them, so
    with first_row > 0 rewards_out must be given."""
    T, N, returns, adv, adv_norm, stats = _gae_operands("normalized_gae_returns", rewards, value_preds, masks, next_value, out)
    first_row, rewards_out = _norm_operands("normalized_gae_returns", rewards, masks, state, first_row, rewards_out, T, N)
    _abi.call("wsmg_gae_returns_normalized", _p(rewards), _p(masks), _p(state), float(norm_gamma), float(clip), float(norm_eps),
              first_row, int(bool(update)), _p(rewards_out), _p(value_preds), _p(next_value), float(gamma), float(gamma) * float(tau),
              int(bool(use_gae)), T, N, _p(returns), _p(adv), _p(adv_norm), _p(stats), float(eps), _stream())
    return returns, adv, adv_norm, stats, rewards_out


GATHER_MAX_FIELDS = 32       # GATHER_MAX of csrc/wsmg_common.h: fields per launch (a longer list is several launches)


def _row_bytes(t):
    return (t.numel() // (t.shape[0] * t.shape[1]) if t.shape[0] and t.shape[1] else 0) * t.element_size()


def gather_kernel_ok(src, dst):
    """Does the grouped launch take this field?  GPU tensors whose rows (everything behind [R, N]) are a positive multiple of 4
    bytes between 4-byte aligned bases.  Anything else (a uint8 observation of odd width) goes through `index_select`."""
    rb = _row_bytes(src)
    return src.is_cuda and rb > 0 and rb % 4 == 0 and src.data_ptr() % 4 == 0 and dst.data_ptr() % 4 == 0


@torch.no_grad()
def gather_columns(fields, ind, rows=None, out=None):
    """-> [fields[f][:rows_f].index_select(1, ind) for f], on the GPU in one launch per GATHER_MAX_FIELDS fields.

    fields: tensors [R_f, N, ...] with one N, of any dtype (bytes are copied); ind: int64 [n] on their device, every entry in
    [0, N) (on the GPU an entry outside copies nothing); rows: an int or one per field, 0 <= rows_f <= R_f (default R_f).  The
    results are [rows_f, n, ...]: the caller flattens them.  out: a list of tensors to write into; an entry that is None is
    allocated, and nothing is allocated when all are given.  Operands are contiguous and on one device.  CPU tensors, and fields
    the kernel does not take (`gather_kernel_ok`), go through `index_select`, field by field."""
    fields = list(fields)
    if not isinstance(ind, torch.Tensor) or ind.dtype != torch.int64 or ind.dim() != 1 or ind.numel() < 1:
        raise _abi.WsmgError("gather_columns: ind must be an int64 tensor [n] with n >= 1, got "
                             + (f"{ind.dtype} {tuple(ind.shape)}" if isinstance(ind, torch.Tensor) else type(ind).__name__))
    if not ind.is_contiguous():
        raise _abi.WsmgError(f"gather_columns: ind is not contiguous (strides {ind.stride()})")
    n, dev = ind.numel(), ind.device
    if rows is None or isinstance(rows, int):
        rows = [rows] * len(fields)
    out = [None] * len(fields) if out is None else list(out)
    if len(rows) != len(fields) or len(out) != len(fields):
        raise _abi.WsmgError(f"gather_columns: {len(fields)} fields, but {len(rows)} rows and {len(out)} out entries")
    N = None
    res, descs = [], []
    for f, (src, r, dst) in enumerate(zip(fields, rows, out)):
        if src.dim() < 2:
            raise _abi.WsmgError(f"gather_columns: fields[{f}] must be [R, N, ...], got {tuple(src.shape)}")
        if src.device != dev:
            raise _abi.WsmgError(f"gather_columns: fields[{f}] is on {src.device}, ind on {dev}")
        if not src.is_contiguous():
            raise _abi.WsmgError(f"gather_columns: fields[{f}] is not contiguous: shape {tuple(src.shape)} strides {src.stride()}")
        N = src.shape[1] if N is None else N
        if src.shape[1] != N or N < 1:
            raise _abi.WsmgError(f"gather_columns: fields[{f}] has {src.shape[1]} columns, fields[0] has {N} (at least one is needed)")
        r = src.shape[0] if r is None else int(r)
        if not 0 <= r <= src.shape[0]:
            raise _abi.WsmgError(f"gather_columns: rows[{f}] = {r} is outside fields[{f}]'s {src.shape[0]} rows")
        shape = (r, n) + tuple(src.shape[2:])
        if dst is None:
            dst = torch.empty(shape, dtype=src.dtype, device=dev)
        elif tuple(dst.shape) != shape or dst.dtype != src.dtype or dst.device != dev:
            raise _abi.WsmgError(f"gather_columns: out[{f}] must be {src.dtype} {shape} on {dev}, got {dst.dtype} {tuple(dst.shape)} "
                                 f"on {dst.device}")
        elif not dst.is_contiguous():
            raise _abi.WsmgError(f"gather_columns: out[{f}] is not contiguous: shape {tuple(dst.shape)} strides {dst.stride()}")
        res.append(dst)
        if dst.numel() == 0:
            continue
        if gather_kernel_ok(src, dst):
            descs.append((dst.data_ptr(), src.data_ptr(), r, _row_bytes(src)))
        else:
            torch.index_select(src[:r], 1, ind, out=dst)
    if descs:
        k = len(descs)
        dsts, srcs, rs, rbs = zip(*descs)                  # the launcher's four parallel host arrays
        _abi.call("wsmg_rollout_gather", (ctypes.c_void_p * k)(*dsts), (ctypes.c_void_p * k)(*srcs), (ctypes.c_longlong * k)(*rs),
                  (ctypes.c_longlong * k)(*rbs), k, _p(ind), n, N, _stream())
    return res
