"""The yardsticks of the PPO trainer (wsmgmap/ppo.py) and of the grouped column gather (csrc/wsmg_rollout_gather.hip).

`written_out_update` is habitat-baselines' `PPO.update`, restated as the loop a user writes today around this package's methods
(habitat is not a dependency), and it is what `wsmgmap.ppo.PPO` is held to:

    advantages = rollouts.get_advantages(use_normalized_advantage)                        once
    for e in range(ppo_epoch):
        for (obs, hidden, actions, prev_actions, value_preds, returns, masks, old_logp, adv) in
                rollouts.recurrent_generator(advantages, num_mini_batch):                  the stock call: fresh tensors
            values, logp, entropy, _ = policy.evaluate_actions(obs, hidden, prev_actions, masks, actions)
            ratio = exp(logp - old_logp);  action_loss = -mean(min(ratio adv, clamp(ratio, 1 - clip, 1 + clip) adv))
            value_loss = 0.5 mean(max((values - returns)^2, (vc - returns)^2)),  vc = value_preds + clamp(values - value_preds, -clip, clip)
                         (unclipped: 0.5 mean((returns - values)^2))
            loss = value_loss value_loss_coef + action_loss - entropy entropy_coef
            zero_grad; before_backward; backward; after_backward; before_step; [CPU: clip_grad_norm_]; step; after_step
    -> the means of value_loss, action_loss and entropy (and of clip_frac = mean(|ratio - 1| > clip), approx_kl = mean(old_logp -
       logp)) over the ppo_epoch * num_mini_batch steps: float32 sums in one tensor, read once, divided on the host

On GPU tensors the loss is `ops.ppo_loss` (held to its float64 oracle by tests/test_gpu_pg_heads.py) and the clip is the device-side
guard of `wsmgmap.optim.Adam(max_grad_norm=...)` (tests/test_gpu_adam_guard.py); on CPU tensors the expressions above in torch and
`torch.nn.utils.clip_grad_norm_` in front of `torch.optim.Adam.step`.

The gather's yardstick is `index_select` on the same tensors; a gather has no rounding, so every comparison is of bits."""
import torch
import torch.nn as nn

import rollout_util as ru

STATS = ("value_loss", "action_loss", "dist_entropy", "clip_frac", "approx_kl")
HOOKS = ("before_backward", "after_backward", "before_step", "after_step")

# Row widths of the gather's case table: name -> (trailing shape, dtype).  4, 8, 12 bytes: the scalar, action and waypoint fields on
# the 4-byte path; 16; 140 (140 % 16 != 0: 4-byte path at a width past one 16-byte unit); 2048 (H = 512); 16 384 (with rows = 5,
# n = 3 more than one workgroup's run of 2 048 units x 16 bytes, so runs end inside a row and between rows); a uint8 row of 3 bytes
# (no multiple of 4: the index_select route inside the same call); int32 and float16 rows of even width (bytes, not dtypes).
WIDTHS = {
    "w4": ((1,), torch.float32), "w8": ((2,), torch.float32), "w12": ((3,), torch.float32), "w16": ((4,), torch.float32),
    "w140": ((7, 5), torch.float32), "w2048": ((512,), torch.float32), "w16384": ((64, 64), torch.float32),
    "u8x3": ((3,), torch.uint8), "i32x6": ((6,), torch.int32), "f16x10": ((10,), torch.float16),
}
GATHER_RUN_BYTES = 2048 * 16         # GATHER_RUN units of 16 bytes: one workgroup's run of csrc/wsmg_rollout_gather.hip
GATHER_MAX_FIELDS = 32               # GATHER_MAX of csrc/wsmg_common.h


def same_bytes(a, b):
    """Equal shapes, dtypes and bytes (rollout_util.same_bits for float32, its like for every other dtype)."""
    if a.dtype != b.dtype or tuple(a.shape) != tuple(b.shape):
        return False
    if a.dtype == torch.float32:
        return ru.same_bits(a, b)
    a, b = a.detach().cpu().contiguous().reshape(-1), b.detach().cpu().contiguous().reshape(-1)
    return torch.equal(a.view(torch.uint8), b.view(torch.uint8))


def random_tensor(shape, dtype, g):
    """Seeded content of any of the table's dtypes, on the CPU; every byte pattern of an integer type can occur."""
    if dtype == torch.uint8:
        return torch.randint(0, 256, shape, generator=g, dtype=torch.uint8)
    if dtype == torch.int32:
        return torch.randint(-2 ** 31, 2 ** 31 - 1, shape, generator=g, dtype=torch.int64).to(torch.int32)
    return torch.randn(shape, generator=g).to(dtype)


def gather_fields(R, N, names=tuple(WIDTHS), seed=0, device="cpu"):
    """One [R, N, *shape] tensor per name of WIDTHS."""
    g = torch.Generator(); g.manual_seed(7001 + 131 * R + 17 * N + seed)
    return [random_tensor((R, N) + WIDTHS[k][0], WIDTHS[k][1], g).to(device) for k in names]


def perm_prefix(N, n, seed=0, device="cpu"):
    """The first n entries of a permutation of N that is not sorted where one exists (N >= 2)."""
    g = torch.Generator(); g.manual_seed(311 + 7 * N + n + seed)
    p = torch.randperm(N, generator=g)
    if N >= 2 and bool((p[1:] > p[:-1]).all()):
        p = p.flip(0)
    return p[:n].contiguous().to(device)


def gather_ref(fields, ind, rows=None):
    """What `ops.gather_columns` returns: `index_select` field by field."""
    rows = [rows] * len(fields) if rows is None or isinstance(rows, int) else rows
    return [f[:(f.shape[0] if r is None else r)].index_select(1, ind) for f, r in zip(fields, rows)]


# -- the written-out trainer loop ----------------------------------------------------------------------------------------------------
def ppo_loss_written_out(logp, old_logp, adv, values, value_preds, returns, entropy, clip, value_loss_coef, entropy_coef, clipped):
    logp, old_logp, adv, values, value_preds, returns = (t.reshape(-1) for t in (logp, old_logp, adv, values, value_preds, returns))
    ratio = torch.exp(logp - old_logp)
    surr1 = ratio * adv
    surr2 = torch.clamp(ratio, 1.0 - clip, 1.0 + clip) * adv
    action_loss = -torch.min(surr1, surr2).mean()
    if clipped:
        value_pred_clipped = value_preds + (values - value_preds).clamp(-clip, clip)
        value_loss = 0.5 * torch.max((values - returns).pow(2), (value_pred_clipped - returns).pow(2)).mean()
    else:
        value_loss = 0.5 * (returns - values).pow(2).mean()
    loss = value_loss * value_loss_coef + action_loss - entropy.reshape(()) * entropy_coef
    with torch.no_grad():
        clip_frac = ((ratio - 1.0).abs() > clip).to(ratio.dtype).mean()
        approx_kl = (old_logp - logp).mean()
    return loss, action_loss, value_loss, clip_frac, approx_kl


def written_out_update(policy, rollouts, optimizer, clip_param, ppo_epoch, num_mini_batch, value_loss_coef, entropy_coef,
                       max_grad_norm=None, use_clipped_value_loss=True, use_normalized_advantage=True, hooks=None):
    """The loop of the module docstring -> dict of the five means (Python floats).  optimizer: `wsmgmap.optim.Adam` constructed with
    max_grad_norm for a GPU policy (the clip is its guard), `torch.optim.Adam` for a CPU one (the clip is clip_grad_norm_ here).
    hooks: a dict of callables by the names of HOOKS."""
    from wsmgmap import ops
    hooks = hooks or {}
    call = lambda name, *a: hooks[name](*a) if name in hooks else None       # noqa: E731
    params = [p for g in optimizer.param_groups for p in g["params"]]
    advantages = rollouts.get_advantages(use_normalized_advantage)
    sums = torch.zeros(len(STATS), device=params[0].device)
    for _ in range(ppo_epoch):
        for obs, hidden, actions, prev_actions, value_preds, returns, masks, old_logp, adv in rollouts.recurrent_generator(
                advantages, num_mini_batch):
            values, logp, entropy, _ = policy.evaluate_actions(obs, hidden, prev_actions, masks, actions)
            if logp.is_cuda:
                loss, action_loss, value_loss, clip_frac, approx_kl = ops.ppo_loss(
                    logp, old_logp, adv, values, value_preds, returns, entropy, clip_param, value_loss_coef, entropy_coef,
                    clipped_value=use_clipped_value_loss)
            else:
                loss, action_loss, value_loss, clip_frac, approx_kl = ppo_loss_written_out(
                    logp, old_logp, adv, values, value_preds, returns, entropy, clip_param, value_loss_coef, entropy_coef,
                    use_clipped_value_loss)
            optimizer.zero_grad()
            call("before_backward", loss)
            loss.backward()
            call("after_backward", loss)
            call("before_step")
            if not logp.is_cuda and max_grad_norm is not None:
                nn.utils.clip_grad_norm_(params, max_grad_norm)
            optimizer.step()
            call("after_step")
            with torch.no_grad():
                sums += torch.stack([t.detach().reshape(()).float() for t in (value_loss, action_loss, entropy, clip_frac, approx_kl)])
    steps = ppo_epoch * num_mini_batch
    return {k: v / steps for k, v in zip(STATS, sums.tolist())}


# -- small builders ------------------------------------------------------------------------------------------------------------------
class StandInPolicy(nn.Module):
    """A policy small enough for the CPU: a linear trunk over one observation and the previous action, a diagonal Gaussian head and
    a critic, with `evaluate_actions` in the shape `BasePolicy` gives it (log-probabilities [B], a 0-dim entropy)."""

    def __init__(self, obs_dim=3, action_dim=2, hidden=8, seed=0):
        super().__init__()
        from wsmgmap.common.distributions import DiagGaussian
        torch.manual_seed(1000 + seed)
        self.trunk = nn.Linear(obs_dim + action_dim, hidden)
        self.action_distribution = DiagGaussian(hidden, action_dim)
        self.critic = nn.Linear(hidden, 1)
        self.frozen = nn.Parameter(torch.ones(2), requires_grad=False)

    def evaluate_actions(self, observations, rnn_hidden_states, prev_actions, masks, action):
        features = torch.tanh(self.trunk(torch.cat([observations["x"], prev_actions * masks], dim=-1)))
        dist = self.action_distribution(features)
        return self.critic(features), dist.log_probs(action).reshape(-1), dist.entropy().mean(), rnn_hidden_states


def fill_storage(st, steps, seed=0):
    """`steps` inserts of seeded content into a storage whose only observation is "x" [3] (tests/test_gpu_gae_returns.py's `_fill`,
    for any storage): an [N, 3] observation, the hidden state, [N, A] actions, log-probabilities, values, rewards, 20 % zero masks."""
    N, A = st.num_envs, st.actions.shape[-1]
    layers, H = st.recurrent_hidden_states.shape[1], st.recurrent_hidden_states.shape[3]
    g = torch.Generator(); g.manual_seed(900 + 10 * st.num_steps + N + seed)
    for _ in range(steps):
        obs = {k: random_tensor((N,) + tuple(v.shape[2:]), v.dtype, g) for k, v in st.observations.items()}
        st.insert(obs, torch.randn(layers, N, H, generator=g), torch.randn(N, A, generator=g), torch.randn(N, generator=g),
                  torch.randn(N, 1, generator=g), torch.randn(N, 1, generator=g), (torch.rand(N, 1, generator=g) >= 0.2).float())


class _Box:
    shape = (2,)


def build_policy():
    """The T = 4 float32 policy of tests/test_gpu_gae_returns.py's policy-step test (its construction, copied), num_proc = 2."""
    from util import state_dict_values
    from wsmgmap.config import default_model_config
    from wsmgmap.models.policy import BasePolicy
    pol = BasePolicy(None, _Box(), default_model_config(num_proc=2, compute_dtype="f32"))
    pol.load_state_dict(state_dict_values(), strict=True)
    pol.net.instruction_encoder.embedding_layer.weight.requires_grad_(False)
    pol = pol.cuda()
    pol.train()
    pol.net.depth_encoder.eval()
    pol.net.rgb_encoder.eval()
    return pol


def policy_storages(T=4, N=4, seed=0):
    """(fused, stock): two GPU storages of N environments x T steps with the same content — the update path's observations of
    `cases.update_inputs(T, N, tag="ppo")` (an instruction length per environment), everything else drawn from a seeded generator (no act() rollout).  The returns are
    computed ONCE, by the stock storage's torch loop, and copied into the fused one, so that both hand out the advantages of the
    same torch expression: the two differ by the minibatch route alone (the one-launch returns normalise the advantages with float64
    statistics, which tests/test_gpu_gae_returns.py holds to their own bar)."""
    from oracle import cases
    from util import T as tt
    from wsmgmap.rollout import RolloutStorage
    obs_np, _, _, _ = cases.update_inputs(T, N, n_tok=tuple((80, 37, 64, 51)[i % 4] for i in range(N)), tag="ppo")
    obs = {k: tt(v).view(T, N, *v.shape[1:]) for k, v in obs_np.items()}
    shapes = {k: (tuple(v.shape[2:]), v.dtype) for k, v in obs.items()}
    g = torch.Generator(); g.manual_seed(4242 + seed)
    drawn = dict(actions=torch.randn(T, N, 2, generator=g), action_log_probs=-2.0 + 0.5 * torch.randn(T, N, 1, generator=g),
                 value_preds=torch.randn(T + 1, N, 1, generator=g), rewards=torch.randn(T, N, 1, generator=g),
                 masks=(torch.rand(T + 1, N, 1, generator=g) >= 0.2).float(), recurrent_hidden_states=0.1 * torch.randn(T + 1, 2, N, 512, generator=g))
    drawn["prev_actions"] = torch.cat([torch.zeros(1, N, 2), drawn["actions"]])
    drawn["masks"][0] = 0.0
    next_value = torch.randn(N, 1, generator=g)
    pair = []
    for fused in (True, False):
        st = RolloutStorage(T, N, shapes, 2, 512, 2, fused=fused).to("cuda")
        for k, v in obs.items():
            st.observations[k][:T].copy_(v)
        for k, v in drawn.items():
            getattr(st, k).copy_(v)
        st.step = T
        pair.append(st)
    fused, stock = pair
    stock.compute_returns(next_value.cuda(), True, 0.99, 0.95)
    fused.returns.copy_(stock.returns)
    fused.value_preds.copy_(stock.value_preds)
    return fused, stock
