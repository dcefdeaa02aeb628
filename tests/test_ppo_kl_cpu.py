"""`wsmgmap.ppo.PPO(target_kl=...)` on the CPU (no GPU needed): the stock arm of the KL early stop — a host `if`, `ppo_loss_torch`,
torch.optim.Adam — against tests/ppo_kl_util.py's written-out loop, to the bit; the limit's rounding; a NaN approx_kl; and the
refusals.  Before the feature every test here that constructs PPO(target_kl=...) fails with torch.optim.Adam's TypeError."""
import copy

import numpy as np
import pytest
import torch
import torch.nn as nn

import ppo_kl_util as ku
import ppo_util as pu

HYPER = dict(clip_param=0.2, ppo_epoch=3, num_mini_batch=2, value_loss_coef=0.5, entropy_coef=0.01)
STEPS = HYPER["ppo_epoch"] * HYPER["num_mini_batch"]
T, N, LR, EPS, MAX_NORM, SEED = 5, 4, 2.5e-2, 1e-5, 0.2, 5


class BnPolicy(pu.StandInPolicy):
    """The stand-in policy with a train-mode BatchNorm behind its trunk: a forward writes running statistics."""

    def __init__(self):
        super().__init__()
        self.bn = nn.BatchNorm1d(8)

    def evaluate_actions(self, observations, rnn_hidden_states, prev_actions, masks, action):
        features = self.bn(torch.tanh(self.trunk(torch.cat([observations["x"], prev_actions * masks], dim=-1))))
        dist = self.action_distribution(features)
        return self.critic(features), dist.log_probs(action).reshape(-1), dist.entropy().mean(), rnn_hidden_states


def _storage(seed=0, nan_logp=False):
    from wsmgmap.rollout import RolloutStorage
    st = RolloutStorage(T, N, {"x": ((3,), torch.float32)}, 2, 4)
    pu.fill_storage(st, T, seed)
    if nan_logp:
        st.action_log_probs[2] = float("nan")
    st.compute_returns(torch.linspace(-1.0, 1.0, N).view(N, 1), True, 0.99, 0.95)
    return st


def _loop(pol, target_kl=None, limit=None, **kw):
    opt = torch.optim.Adam([p for p in pol.parameters() if p.requires_grad], lr=LR, eps=EPS)
    torch.manual_seed(SEED)
    return ku.written_out_kl_update(pol, _storage(**kw), opt, target_kl=target_kl, limit=limit, max_grad_norm=MAX_NORM, **HYPER)


def _agent(pol, target_kl, **more):
    from wsmgmap.ppo import PPO
    return PPO(pol, lr=LR, eps=EPS, max_grad_norm=MAX_NORM, target_kl=target_kl, **HYPER, **more)


def _state_equal(a, b):
    return [k for (k, x), y in zip(a.state_dict().items(), b.state_dict().values()) if not pu.same_bytes(x, y)]


@pytest.fixture(scope="module")
def free_run():
    """The written-out loop with a limit nothing reaches: every minibatch's approx_kl, computed once."""
    out = _loop(BnPolicy(), limit=np.float32(np.inf))
    assert out["steps_taken"] == STEPS and not out["stopped"] and len(out["kls"]) == STEPS
    return out


@pytest.mark.parametrize("where", ["first", "mid", "never"])
def test_update_with_a_target_kl_is_the_written_out_loop_to_the_bit(free_run, where):
    kls = free_run["kls"]
    if where == "first":
        target, k = -1.0, 0                       # limit -1.5: the first approx_kl is above it (asserted below)
        assert kls[0] > -1.5
    elif where == "never":
        target, k = float("inf"), None
    else:
        found = ku.first_running_maximum(kls)
        assert found is not None, kls
        k, below = found
        target = ku.target_between(np.float32(below), np.float32(kls[k]))
    pol_a = BnPolicy()
    pol_b = copy.deepcopy(pol_a)
    before = copy.deepcopy(pol_a.state_dict())
    want = _loop(pol_b, target_kl=target)
    agent = _agent(pol_a, target)
    assert isinstance(agent.optimizer, torch.optim.Adam)
    torch.manual_seed(SEED)
    got = agent.update(_storage())
    stats = agent.last_stats
    print(f"{where}: approx_kl per minibatch {kls}; limit {agent.kl_limit!r}; stop at {want['stop_ordinal']} after {want['steps_taken']} steps")
    assert want["stopped"] == (k is not None) and want["stop_ordinal"] == k and want["steps_taken"] == (STEPS if k is None else k)
    assert set(stats) == set(pu.STATS) | {"grad_norm", "steps_taken", "stopped", "stop_ordinal", "stop_kl"}
    for key in ("steps_taken", "stopped", "stop_ordinal", "stop_kl", "grad_norm"):
        assert stats[key] == want[key], key
    assert ku.same_stats(stats, want) and len(got) == 3 and ku.same_stats(dict(zip(pu.STATS, got)), want, pu.STATS[:3])
    assert _state_equal(pol_a, pol_b) == []
    if k == 0:      # nothing was taken: NaN means, no norm, and the policy — BatchNorm statistics included — is what it was
        assert all(stats[s] != stats[s] for s in pu.STATS) and stats["grad_norm"] is None
        assert [n for n, v in pol_a.state_dict().items() if not pu.same_bytes(v, before[n])] == []
    else:
        assert int(pol_a.bn.num_batches_tracked) == want["steps_taken"]          # the stopped forwards were rolled back
        assert stats["stop_kl"] is None or stats["stop_kl"] == kls[k]


def test_without_a_target_kl_the_update_is_todays(free_run):
    """target_kl=None: tests/ppo_util.py's loop, to the bit, with today's keys in last_stats — and target_kl=inf moves the policy to
    the same bits."""
    pol_a, pol_b, pol_c = BnPolicy(), BnPolicy(), BnPolicy()
    agent = _agent(pol_a, None)
    torch.manual_seed(SEED)
    agent.update(_storage())
    opt = torch.optim.Adam([p for p in pol_b.parameters() if p.requires_grad], lr=LR, eps=EPS)
    torch.manual_seed(SEED)
    want = pu.written_out_update(pol_b, _storage(), opt, max_grad_norm=MAX_NORM, **HYPER)
    assert set(agent.last_stats) == set(pu.STATS) | {"grad_norm"} and agent.kl_limit is None
    assert {k: agent.last_stats[k] for k in pu.STATS} == want
    assert _state_equal(pol_a, pol_b) == []
    inf = _agent(pol_c, float("inf"))
    torch.manual_seed(SEED)
    inf.update(_storage())
    assert _state_equal(pol_c, pol_b) == [] and ku.same_stats(inf.last_stats, want) and inf.last_stats["steps_taken"] == STEPS
    assert inf.last_stats["grad_norm"] == agent.last_stats["grad_norm"]


def test_the_limit_is_float32_of_one_and_a_half_target_kl(free_run):
    """A target whose product 1.5 * target_kl lies, in double, just BELOW a minibatch's approx_kl K and rounds to K in float32: a
    comparison in double stops there, the rule's (float32 limit == K, K > K false) does not."""
    from wsmgmap import ops
    for t in (0.01, 0.015, 1.0 / 3.0, 2.0 ** -30, 1e30, -0.02):
        assert ops.kl_limit_of(t) == float(np.float32(1.5 * t)) and _agent(BnPolicy(), t).kl_limit == ops.kl_limit_of(t)
    assert any(np.float32(1.5 * np.float32(t)) != np.float32(1.5 * t) for t in (0.01, 0.015, 1.0 / 3.0))    # not float32 arithmetic
    kls = free_run["kls"]
    k, _ = ku.first_running_maximum(kls)
    K = np.float32(kls[k])
    target = float(K) * (1.0 - 2.0 ** -27) / 1.5
    assert 1.5 * target < float(K) and np.float32(1.5 * target) == K        # the premise
    agent = _agent(BnPolicy(), target)
    torch.manual_seed(SEED)
    agent.update(_storage())
    assert agent.kl_limit == float(K)
    assert agent.last_stats["steps_taken"] > k and agent.last_stats["stop_ordinal"] != k
    below = _agent(BnPolicy(), float(np.nextafter(K, np.float32(-np.inf))) / 1.5)
    assert below.kl_limit < float(K)
    torch.manual_seed(SEED)
    below.update(_storage())
    assert below.last_stats["stopped"] and below.last_stats["stop_ordinal"] == k and below.last_stats["stop_kl"] == float(K)


def test_a_nan_approx_kl_does_not_stop():
    """A NaN among every environment's stored log-probabilities: every minibatch has a NaN approx_kl, NaN > limit is false whatever
    the limit (here a negative one, which any number would exceed), and the update steps through all of them, as it does without a
    limit."""
    agent = _agent(BnPolicy(), -1.0)
    torch.manual_seed(SEED)
    agent.update(_storage(nan_logp=True))
    want = _loop(BnPolicy(), target_kl=-1.0, nan_logp=True)
    assert len(want["kls"]) == STEPS and all(k != k for k in want["kls"]), want["kls"]
    assert want["steps_taken"] == STEPS and not want["stopped"]
    stats = agent.last_stats
    assert stats["steps_taken"] == STEPS and stats["stopped"] is False and stats["stop_ordinal"] is None and stats["stop_kl"] is None
    assert stats["approx_kl"] != stats["approx_kl"]


def test_set_step_gate_on_an_unguarded_optimizer_is_refused():
    from wsmgmap.optim import Adam
    p = nn.Parameter(torch.zeros(4))
    opt = Adam([p], lr=1e-3)
    with pytest.raises(ValueError, match="guarded step"):
        opt.set_step_gate(torch.zeros(8))
    opt.set_step_gate(None)                                  # taking a gate away needs nothing
    guarded = Adam([p], lr=1e-3, skip_nonfinite=True)
    with pytest.raises(ValueError, match="float32 CUDA tensor"):
        guarded.set_step_gate(torch.zeros(8))                # a gate on the host is no device word


def test_refusals_of_the_trainer():
    with pytest.raises(ValueError, match="NaN"):
        _agent(BnPolicy(), float("nan"))
    with pytest.raises(ValueError, match="kl_sync"):
        _agent(BnPolicy(), 0.01, kl_sync="minibatch")
    with pytest.raises(ValueError, match="needs a target_kl"):
        _agent(BnPolicy(), None, kl_sync="epoch")


def test_kl_sync_epoch_leaves_the_same_policy(free_run):
    kls = free_run["kls"]
    k, below = ku.first_running_maximum(kls)
    target = ku.target_between(np.float32(below), np.float32(kls[k]))
    pol_a, pol_b = BnPolicy(), BnPolicy()
    a, b = _agent(pol_a, target), _agent(pol_b, target, kl_sync="epoch")
    for agent in (a, b):
        torch.manual_seed(SEED)
        agent.update(_storage())
    assert _state_equal(pol_a, pol_b) == [] and a.last_stats["stop_ordinal"] == b.last_stats["stop_ordinal"] == k
    assert ku.same_stats(a.last_stats, b.last_stats) and a.last_stats["steps_taken"] == b.last_stats["steps_taken"]
