"""Rollout storage for a PPO / A2C update after DAgger: habitat-baselines' `RolloutStorage` by attribute and method name, restated
(habitat-baselines is not a dependency and no version of it is pinned: DESIGN.md §2), plus `PPO.get_advantages`.

What is new against the stock class: on float32 GPU storage `compute_returns` is ONE launch (ops.gae_returns,
csrc/wsmg_pg_rollout.hip) over the rows in use, which also fills the raw and the normalised advantages that `get_advantages` then
hands out as views — no Python loop over steps, and after the first call no allocation and no synchronisation, so the pair can be
captured in a HIP graph on one stream.  `returns`, the raw advantages and `value_preds[step]` are the bits of the torch loop.
CPU storage, other dtypes, more than ops.GAE_MAX_ENVS environments or `fused=False` run that torch loop (the stock arm of the tests),
as `evaluate_actions` composes stock modules outside its kernels' limits.

`insert` and `after_update` are torch indexing.  On GPU storage each minibatch of `recurrent_generator` is ONE launch
(ops.gather_columns, csrc/wsmg_rollout_gather.hip) over every stored tensor, the advantages and the row-0 hidden state, where the
stock class runs an `index_select` and an allocation per field behind a host copy of the index list; the bits are the same.
A rollout may be partial: everything works on the rows `[:step]` that `insert` has filled."""
import numpy as np
import torch

from . import ops

EPS_PPO = 1e-5


def _torch_dtype(dt):
    if isinstance(dt, torch.dtype):
        return dt
    return torch.from_numpy(np.zeros(0, dtype=dt)).dtype


def _shapes_of(observation_shapes):
    """name -> (shape, torch dtype) from a dict of (shape, dtype) pairs, or from a gym `Dict` space if one happens to be passed."""
    spaces = getattr(observation_shapes, "spaces", None)
    if spaces is not None:
        return {k: (tuple(sp.shape), _torch_dtype(sp.dtype)) for k, sp in spaces.items()}
    return {k: (tuple(shape), _torch_dtype(dt)) for k, (shape, dt) in observation_shapes.items()}


def _f32_scalar(v):
    """The float32 value a Python float becomes on its way to a kernel: the stock arm sees the numbers the launch sees."""
    return float(np.float32(v))


class RewardNormalizer:
    """Rewards divided by the running standard deviation of the discounted return: the return path of baselines' `VecNormalize`
    (`ret = ret * gamma + reward`, a running mean / variance of `ret` over steps and environments, `reward / sqrt(var + eps)`
    clipped to +-clip, `ret` restarted where an episode ended), restated; baselines is not a dependency and there is no golden
    (DESIGN.md §2).  The state lives on the device in ONE float64 tensor `state` [3 + N] = {mean, var, count, ret[N]}, initially
    0, 1, count0 and zeros; `mean`, `var`, `count` and `returns` are views of it.  For rows s = first_row .. T-1 in order, in float64:

        ret = ret * gamma + rewards[s]
        bmean = sum_n ret / N;  bM2 = sum_n (ret - bmean)^2;  delta = bmean - mean;  tot = count + N
        mean += delta * N / tot;  var = (var * count + bM2 + delta^2 * count * N / tot) / tot;  count = tot
        out[s] = clamp(rewards[s] / sqrt(var + eps), -clip, clip), rounded once to out's dtype (NaN stays NaN)
        ret *= masks[s+1]

    After `eval()` (evaluation, or statistics loaded from a checkpoint and frozen) only the `out` line runs, with the stored var,
    and the state is not written; `train()` switches the update back on.  gamma, clip, eps and count0 are used as the float32
    numbers a launch is handed.  `normalize` is ONE launch (ops.normalize_rewards) on contiguous float32 GPU tensors within
    ops.GAE_MAX_ENVS environments, and `normalize_stock`, the same loop in float64 torch operators, for everything else.
    Under data parallelism each rank keeps the statistics of its own environments: they are not synchronised between ranks."""

    def __init__(self, num_envs, gamma, clip=10.0, eps=1e-8, count0=1e-4):
        self.num_envs = int(num_envs)
        if self.num_envs < 1:
            raise ValueError(f"RewardNormalizer: num_envs must be at least 1, got {num_envs}")
        self.gamma, self.clip, self.eps = float(gamma), float(clip), float(eps)
        self.state = torch.zeros(3 + self.num_envs, dtype=torch.float64)
        self.state[1] = 1.0
        self.state[2] = _f32_scalar(count0)
        self.training = True

    mean = property(lambda self: self.state[0])
    var = property(lambda self: self.state[1])
    count = property(lambda self: self.state[2])
    returns = property(lambda self: self.state[3:])

    def to(self, device):
        self.state = self.state.to(device)
        return self

    def train(self, mode=True):
        self.training = bool(mode)
        return self

    def eval(self):
        return self.train(False)

    def state_dict(self):
        return {"state": self.state.detach().clone(), "gamma": self.gamma, "clip": self.clip, "eps": self.eps}

    def load_state_dict(self, sd):
        state = sd["state"]
        if tuple(state.shape) != tuple(self.state.shape) or state.dtype != torch.float64:
            raise ValueError(f"RewardNormalizer.load_state_dict: state must be float64 {tuple(self.state.shape)}, got {state.dtype} "
                             f"{tuple(state.shape)}")
        self.state.copy_(state)          # in place: a captured graph keeps reading this tensor
        self.gamma, self.clip, self.eps = float(sd["gamma"]), float(sd["clip"]), float(sd["eps"])

    def _operands(self, rewards, masks, out):
        T, N = rewards.shape[0], self.num_envs
        if rewards.dim() < 2 or T < 1 or rewards.shape[1] != N or rewards.numel() != T * N:
            raise ValueError(f"RewardNormalizer: rewards must be [T, {N}] or [T, {N}, 1] with T >= 1, got {tuple(rewards.shape)}")
        if masks.dim() < 2 or masks.shape[0] != T + 1 or masks.shape[1] != N or masks.numel() != (T + 1) * N:
            raise ValueError(f"RewardNormalizer: masks must be [{T + 1}, {N}] or [{T + 1}, {N}, 1], got {tuple(masks.shape)}")
        if out is None:
            out = torch.zeros_like(rewards, memory_format=torch.contiguous_format)
        if tuple(out.shape) != tuple(rewards.shape) or not out.is_contiguous() or out.device != rewards.device:
            raise ValueError(f"RewardNormalizer: out must be contiguous {tuple(rewards.shape)} on {rewards.device}, got "
                             f"{tuple(out.shape)} strides {out.stride()} on {out.device}")
        if self.state.device != rewards.device or masks.device != rewards.device:
            raise ValueError(f"RewardNormalizer: rewards on {rewards.device}, masks on {masks.device}, state on {self.state.device}: "
                             "move the normaliser with .to()")
        return T, out

    def kernel_ok(self, rewards, masks, out=None):
        """Does `normalize` run the launch on these tensors?"""
        return (ops.reward_normalize_ok(rewards, masks, self.state) and rewards.is_contiguous() and masks.is_contiguous()
                and (out is None or (out.is_cuda and out.dtype == torch.float32)))

    @torch.no_grad()
    def normalize(self, rewards, masks, first_row=0, out=None):
        """-> out, shaped as rewards [T, N(, 1)], rows [first_row, T) written (default: a new tensor, zeros below first_row); the
        statistics advance by those rows unless `eval()`.  masks [T+1, N(, 1)]: masks[s+1] = 0 where step s ended an episode."""
        T, out = self._operands(rewards, masks, out)
        if not 0 <= first_row <= T:
            raise ValueError(f"RewardNormalizer: first_row = {first_row} is outside [0, {T}]")
        if not self.kernel_ok(rewards, masks, out):
            return self.normalize_stock(rewards, masks, first_row, out)
        return ops.normalize_rewards(rewards, masks, self.state, self.gamma, self.clip, self.eps, first_row=first_row,
                                     update=self.training, out=out)

    @torch.no_grad()
    def normalize_stock(self, rewards, masks, first_row=0, out=None):
        """`normalize` as the loop of the class docstring in float64 torch operators, on any device and dtype: the stock arm.  The two
        sums over n are taken in index order (`cumsum`)."""
        T, out = self._operands(rewards, masks, out)
        if not 0 <= first_row <= T:
            raise ValueError(f"RewardNormalizer: first_row = {first_row} is outside [0, {T}]")
        N, st = self.num_envs, self.state
        r, m, o = rewards.reshape(T, N), masks.reshape(T + 1, N), out.view(T, N)
        gamma, clip, eps = _f32_scalar(self.gamma), _f32_scalar(self.clip), _f32_scalar(self.eps)
        if not self.training:
            if first_row < T:
                o[first_row:] = torch.clamp(r[first_row:].double() / torch.sqrt(st[1] + eps), -clip, clip).to(o.dtype)
            return out
        mean, var, count, ret = st[0].clone(), st[1].clone(), st[2].clone(), st[3:].clone()
        for s in range(first_row, T):
            rs = r[s].double()
            ret = ret * gamma + rs
            bmean = ret.cumsum(0)[-1] / N
            d = ret - bmean
            bm2 = (d * d).cumsum(0)[-1]
            delta, tot = bmean - mean, count + N
            mean = mean + delta * N / tot
            var = (var * count + bm2 + delta * delta * count * N / tot) / tot
            count = tot
            o[s] = torch.clamp(rs / torch.sqrt(var + eps), -clip, clip).to(o.dtype)
            ret = ret * m[s + 1].double()
        st[0], st[1], st[2] = mean, var, count
        st[3:] = ret
        return out


class RolloutStorage:
    """Tensors (T = num_steps, N = num_envs): observations[k] [T+1, N, *shape] in its own dtype; recurrent_hidden_states
    [T+1, layers, N, H] (the layout `BasePolicy.act` takes a row of); rewards, action_log_probs [T, N, 1]; value_preds, returns, masks
    [T+1, N, 1]; actions [T, N, A]; prev_actions [T+1, N, A]; `step`: rows filled so far (a host int).

    reward_normalizer: a `RewardNormalizer` over the same N.  `compute_returns` then works on `rewards_normalized` [T, N, 1]
    (allocated on first use) and `rewards` stays raw for logging.  The storage remembers how many rows of this rollout it has
    normalised: a second `compute_returns` over the same rows re-uses them and leaves the statistics alone, one after further
    `insert`s normalises the new rows only, with the carry continuing; `after_update` forgets the rows, not the statistics or the
    carry.  On the fused route normalising and the returns are ONE launch (ops.normalized_gae_returns); elsewhere the normaliser's
    stock arm is followed by the torch loop.  Each data-parallel rank keeps its own statistics."""

    def __init__(self, num_steps, num_envs, observation_shapes, action_dim, recurrent_hidden_state_size, num_recurrent_layers=1,
                 fused=True, reward_normalizer=None):
        T, N = int(num_steps), int(num_envs)
        self.observations = {k: torch.zeros(T + 1, N, *shape, dtype=dt) for k, (shape, dt) in _shapes_of(observation_shapes).items()}
        self.recurrent_hidden_states = torch.zeros(T + 1, num_recurrent_layers, N, recurrent_hidden_state_size)
        self.rewards = torch.zeros(T, N, 1)
        self.value_preds = torch.zeros(T + 1, N, 1)
        self.returns = torch.zeros(T + 1, N, 1)
        self.action_log_probs = torch.zeros(T, N, 1)
        self.actions = torch.zeros(T, N, action_dim)
        self.prev_actions = torch.zeros(T + 1, N, action_dim)
        self.masks = torch.zeros(T + 1, N, 1)
        self.num_steps, self.num_envs = T, N
        self.step = 0
        self.fused = bool(fused)
        # the one launch's other outputs: raw and normalised advantages and {mean, std}; `_adv_step`: the rows they hold, and the eps
        self._adv = self._adv_norm = self._stats = None
        self._adv_step, self._adv_eps = None, None
        self._staging = None      # recurrent_generator(reuse_buffers=True): one minibatch's tensors, kept between minibatches
        if reward_normalizer is not None and reward_normalizer.num_envs != N:
            raise ValueError(f"RolloutStorage: the reward normaliser has {reward_normalizer.num_envs} environments, the storage {N}")
        self.reward_normalizer = reward_normalizer
        self.rewards_normalized = None      # [T, N, 1], allocated by the first compute_returns with a normaliser
        self._norm_step = 0                 # rows of rewards_normalized that hold this rollout's normalised rewards

    _TENSORS = ("recurrent_hidden_states", "rewards", "value_preds", "returns", "action_log_probs", "actions", "prev_actions", "masks")

    def to(self, device):
        self.observations = {k: v.to(device) for k, v in self.observations.items()}
        for name in self._TENSORS:
            setattr(self, name, getattr(self, name).to(device))
        self._adv = self._adv_norm = self._stats = None
        self._adv_step = None
        self._staging = None
        if self.reward_normalizer is not None:
            self.reward_normalizer.to(device)
        if self.rewards_normalized is not None:
            self.rewards_normalized = self.rewards_normalized.to(device)
        return self

    # -- plumbing ----------------------------------------------------------------------------------------------------------------
    def insert(self, observations, recurrent_hidden_states, actions, action_log_probs, value_preds, rewards, masks):
        """Observations, hidden state, `prev_actions` (= actions) and masks go to row step + 1, the rest to row step."""
        s = self.step
        if s >= self.num_steps:
            raise ValueError(f"RolloutStorage.insert: the storage is full ({self.num_steps} steps): call after_update() first")
        for k, v in observations.items():
            self.observations[k][s + 1].copy_(v)
        put = lambda dst, src: dst.copy_(src.reshape(dst.shape))     # noqa: E731   ([N] log-probabilities into [N, 1])
        put(self.recurrent_hidden_states[s + 1], recurrent_hidden_states)
        put(self.actions[s], actions)
        put(self.prev_actions[s + 1], actions)
        put(self.action_log_probs[s], action_log_probs)
        put(self.value_preds[s], value_preds)
        put(self.rewards[s], rewards)
        put(self.masks[s + 1], masks)
        self.step = s + 1
        self._adv_step = None

    def after_update(self):
        """Row `step` of observations, hidden state, masks and prev_actions becomes row 0 of the next rollout."""
        s = self.step
        for v in self.observations.values():
            v[0].copy_(v[s])
        self.recurrent_hidden_states[0].copy_(self.recurrent_hidden_states[s])
        self.masks[0].copy_(self.masks[s])
        self.prev_actions[0].copy_(self.prev_actions[s])
        self.step = 0
        self._adv_step = None
        self._norm_step = 0

    # -- returns and advantages --------------------------------------------------------------------------------------------------
    def _fused_route(self):
        return (self.fused and self.step >= 1 and ops.gae_returns_ok(self.rewards, self.step)
                and all(t.is_cuda and t.dtype == torch.float32 for t in (self.value_preds, self.returns, self.masks)))

    def compute_returns(self, next_value, use_gae, gamma, tau):
        """habitat-baselines' `compute_returns` over the rows [:step]: under GAE `value_preds[step] = next_value` and returns[s] =
        gae[s] + value_preds[s]; else `returns[step] = next_value` and the discounted sum.  next_value: [N, 1] (or N elements)."""
        T = self.step
        rewards, nz = self.rewards, self.reward_normalizer
        fresh = 0          # with a normaliser: the first row it has not normalised yet
        if nz is not None and T >= 1:
            if self.rewards_normalized is None:
                self.rewards_normalized = torch.zeros_like(self.rewards)
            rewards, fresh = self.rewards_normalized, min(self._norm_step, T)
            self._norm_step = T
        fused = self._fused_route() and (nz is None or nz.kernel_ok(self.rewards[:T], self.masks[:T + 1], rewards[:T]))
        if nz is not None and fresh < T and not fused:
            nz.normalize_stock(self.rewards[:T], self.masks[:T + 1], fresh, rewards[:T])
        if fused:
            if self._adv is None:
                self._adv, self._adv_norm = torch.empty_like(self.rewards), torch.empty_like(self.rewards)
                self._stats = torch.empty(2, device=self.rewards.device, dtype=torch.float64)
            if not (next_value.is_cuda and next_value.dtype == torch.float32 and next_value.is_contiguous()):
                next_value = next_value.to(device=self.rewards.device, dtype=torch.float32).contiguous()
            out = (self.returns[:T + 1], self._adv[:T], self._adv_norm[:T], self._stats)
            if fresh < T and nz is not None:
                ops.normalized_gae_returns(self.rewards[:T], self.value_preds[:T + 1], self.masks[:T + 1], next_value, gamma, tau,
                                           nz.state, nz.gamma, nz.clip, nz.eps, use_gae=use_gae, eps=EPS_PPO, first_row=fresh,
                                           update=nz.training, rewards_out=rewards[:T], out=out)
            else:
                ops.gae_returns(rewards[:T], self.value_preds[:T + 1], self.masks[:T + 1], next_value, gamma, tau, use_gae=use_gae,
                                eps=EPS_PPO, out=out)
            self._adv_step, self._adv_eps = T, EPS_PPO
            return
        self._adv_step = None
        with torch.no_grad():
            next_value = next_value.reshape(self.value_preds[T].shape)
            if use_gae:
                self.value_preds[T] = next_value
                gae = 0
                for s in reversed(range(T)):
                    delta = rewards[s] + gamma * self.value_preds[s + 1] * self.masks[s + 1] - self.value_preds[s]
                    gae = delta + gamma * tau * self.masks[s + 1] * gae
                    self.returns[s] = gae + self.value_preds[s]
            else:
                self.returns[T] = next_value
                for s in reversed(range(T)):
                    self.returns[s] = self.returns[s + 1] * gamma * self.masks[s + 1] + rewards[s]

    def get_advantages(self, use_normalized_advantage=True, eps=EPS_PPO):
        """habitat-baselines' `PPO.get_advantages` over the rows [:step]: returns - value_preds, normalised to (a - mean) / (std + eps)
        with the unbiased std over all entries.  After a fused `compute_returns` this is a view of what that launch wrote (valid until
        the next insert / after_update / compute_returns; the stored tensors must not have been edited in between)."""
        T = self.step
        if self._adv_step == T and T >= 1:
            if not use_normalized_advantage:
                return self._adv[:T]
            if eps == self._adv_eps:
                return self._adv_norm[:T]
            a = self._adv[:T].double()        # another eps than the launch's: from its statistics, still no loop over steps
            return ((a - self._stats[0]) / (self._stats[1] + eps)).float()
        with torch.no_grad():
            advantages = self.returns[:T] - self.value_preds[:T]
            if not use_normalized_advantage:
                return advantages
            return (advantages - advantages.mean()) / (advantages.std() + eps)

    # -- minibatches -------------------------------------------------------------------------------------------------------------
    def recurrent_generator(self, advantages, num_mini_batch, *, reuse_buffers=False):
        """Minibatches of whole environments, habitat-baselines' order of fields: (observations, recurrent_hidden_states, actions,
        prev_actions, value_preds, returns, masks, old_action_log_probs, advantages).  A `torch.randperm` over the environments is cut
        into num_mini_batch chunks of num_envs // num_mini_batch (environments beyond the last whole chunk sit this epoch out);
        each batch is the [:step] rows of its columns flattened to [step * n, ...] (row t * n + j: step t of the chunk's j-th
        environment) and the hidden state of row 0 as [layers, n, H].

        On GPU storage with `fused` each minibatch is ONE `ops.gather_columns` call over all of these fields (one launch; a field
        whose rows are no multiple of 4 bytes is an `index_select` beside it), and the permutation goes to the device once per call
        of the generator: the same draw, tuple, shapes and bits as the stock route, which CPU storage and `fused=False` run.
        reuse_buffers: yield views of staging buffers the storage keeps (valid until the next minibatch; dropped by `to()`) instead
        of fresh tensors."""
        N, T = self.num_envs, self.step
        if N < num_mini_batch:
            raise ValueError(f"RolloutStorage.recurrent_generator: {N} environments cannot fill {num_mini_batch} minibatches")
        per = N // num_mini_batch
        perm = torch.randperm(N)
        if self.fused and self.rewards.is_cuda and T >= 1:
            yield from self._gathered_minibatches(advantages, perm.to(self.rewards.device), num_mini_batch, per, reuse_buffers)
            return
        for b in range(num_mini_batch):
            ind = perm[b * per:(b + 1) * per].to(self.rewards.device)
            cols = lambda t, rows=T: t[:rows].index_select(1, ind).flatten(0, 1)      # noqa: E731
            obs = {k: cols(v) for k, v in self.observations.items()}
            hidden = self.recurrent_hidden_states[0].index_select(1, ind)
            yield (obs, hidden, cols(self.actions), cols(self.prev_actions), cols(self.value_preds), cols(self.returns),
                   cols(self.masks), cols(self.action_log_probs), cols(advantages))

    def _gathered_minibatches(self, advantages, perm, num_mini_batch, per, reuse_buffers):
        """The fused route of `recurrent_generator`; perm is on the device."""
        T, keys = self.step, list(self.observations)
        if not advantages.is_contiguous():
            advantages = advantages.contiguous()
        fields = [self.observations[k] for k in keys] + [self.recurrent_hidden_states[0], self.actions, self.prev_actions,
                                                        self.value_preds, self.returns, self.masks, self.action_log_probs, advantages]
        rows = [T] * len(fields)
        rows[len(keys)] = self.recurrent_hidden_states.shape[1]
        out = None
        if reuse_buffers:
            want = [(r, per) + tuple(f.shape[2:]) for f, r in zip(fields, rows)]
            st = self._staging
            if st is None or [(tuple(t.shape), t.dtype) for t in st] != [(w, f.dtype) for w, f in zip(want, fields)]:
                st = self._staging = [torch.empty(w, dtype=f.dtype, device=f.device) for w, f in zip(want, fields)]
            out = st
        for b in range(num_mini_batch):
            got = ops.gather_columns(fields, perm[b * per:(b + 1) * per], rows, out)
            flat = [g.flatten(0, 1) for g in got]
            flat[len(keys)] = got[len(keys)]                # the hidden state stays [layers, n, H]
            yield (dict(zip(keys, flat[:len(keys)])), *flat[len(keys):])
