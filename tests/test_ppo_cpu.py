"""`wsmgmap.ppo.PPO` and `ops.gather_columns` on the CPU (no GPU needed): the trainer's stock arm — torch.optim.Adam, clip_grad_norm_,
the loss composed in torch, the stock minibatch generator — against tests/ppo_util.py's written-out loop, to the bit; and the
gather's `index_select` route over the width table."""
import copy

import pytest
import torch

import ppo_util as pu

HYPER = dict(clip_param=0.2, ppo_epoch=3, num_mini_batch=2, value_loss_coef=0.5, entropy_coef=0.01)
T, N = 5, 4


def _storage(seed=0, steps=T):
    from wsmgmap.rollout import RolloutStorage
    st = RolloutStorage(T, N, {"x": ((3,), torch.float32)}, 2, 4)
    pu.fill_storage(st, steps, seed)
    st.compute_returns(torch.linspace(-1.0, 1.0, N).view(N, 1), True, 0.99, 0.95)
    return st


@pytest.mark.parametrize("normalized", [True, False], ids=["normalized_adv", "raw_adv"])
@pytest.mark.parametrize("clipped", [True, False], ids=["clipped_value", "plain_value"])
@pytest.mark.parametrize("max_grad_norm", [0.2, None], ids=["clip0.2", "noclip"])
def test_update_is_the_written_out_loop_to_the_bit(clipped, normalized, max_grad_norm):
    from wsmgmap.ppo import PPO
    pol_a = pu.StandInPolicy()
    pol_b = copy.deepcopy(pol_a)
    before = {k: v.detach().clone() for k, v in pol_a.state_dict().items()}
    st_a, st_b = _storage(), _storage()
    agent = PPO(pol_a, lr=2.5e-3, eps=1e-5, max_grad_norm=max_grad_norm, use_clipped_value_loss=clipped,
                use_normalized_advantage=normalized, **HYPER)
    assert isinstance(agent.optimizer, torch.optim.Adam) and agent.device.type == "cpu"
    assert all(p.requires_grad for g in agent.optimizer.param_groups for p in g["params"])
    torch.manual_seed(5)
    got = agent.update(st_a)
    opt = torch.optim.Adam([p for p in pol_b.parameters() if p.requires_grad], lr=2.5e-3, eps=1e-5)
    torch.manual_seed(5)
    want = pu.written_out_update(pol_b, st_b, opt, max_grad_norm=max_grad_norm, use_clipped_value_loss=clipped,
                                 use_normalized_advantage=normalized, **HYPER)
    assert isinstance(got, tuple) and len(got) == 3 and all(type(v) is float for v in got)
    assert got == tuple(want[k] for k in pu.STATS[:3])
    assert {k: agent.last_stats[k] for k in pu.STATS} == want
    assert (agent.last_stats["grad_norm"] is None) == (max_grad_norm is None)
    if max_grad_norm is not None:
        assert agent.last_stats["grad_norm"] > max_grad_norm      # the clip was live
    for (k, a), b in zip(pol_a.state_dict().items(), pol_b.state_dict().values()):
        assert pu.same_bytes(a, b), k
    moved = {k: float((v - before[k]).abs().max()) for k, v in pol_a.state_dict().items()}
    assert moved["critic.weight"] > 0.0 and moved["action_distribution.fc_mean.weight"] > 0.0 and moved["frozen"] == 0.0
    assert st_a.step == T                                          # update() leaves after_update() to the caller


def test_the_two_advantage_forms_and_value_losses_differ():
    """The four arms above are four different updates (a switch that did nothing would pass them all)."""
    from wsmgmap.ppo import PPO
    outs = []
    for clipped, normalized in ((True, True), (False, True), (True, False)):
        torch.manual_seed(5)
        outs.append(PPO(pu.StandInPolicy(), lr=2.5e-3, eps=1e-5, use_clipped_value_loss=clipped, use_normalized_advantage=normalized,
                        **HYPER).update(_storage()))
    assert outs[0] != outs[1] and outs[0] != outs[2]


def test_get_advantages_is_the_storages():
    from wsmgmap.ppo import PPO
    st = _storage()
    for normalized in (True, False):
        agent = PPO(pu.StandInPolicy(), use_normalized_advantage=normalized, **HYPER)
        assert pu.same_bytes(agent.get_advantages(st), st.get_advantages(normalized))


def test_hooks_run_in_habitats_order_once_per_step():
    from wsmgmap.ppo import PPO
    calls = []

    class Traced(PPO):
        def before_backward(self, loss):
            calls.append("before_backward")

        def after_backward(self, loss):
            calls.append("after_backward")

        def before_step(self):
            calls.append("before_step")

        def after_step(self):
            calls.append("after_step")

    Traced(pu.StandInPolicy(), **HYPER).update(_storage())
    assert calls == list(pu.HOOKS) * (HYPER["ppo_epoch"] * HYPER["num_mini_batch"])


def test_more_minibatches_than_environments_is_the_storages_error():
    from wsmgmap.ppo import PPO
    agent = PPO(pu.StandInPolicy(), **dict(HYPER, num_mini_batch=N + 1))
    with pytest.raises(ValueError, match="cannot fill"):
        agent.update(_storage())


def test_partial_rollout_and_reuse_buffers_on_cpu_storage():
    """CPU storage runs the stock generator whatever `reuse_buffers` says; a partial rollout yields step * n rows."""
    st = _storage(steps=3)
    torch.manual_seed(2)
    a = list(st.recurrent_generator(st.get_advantages(), 2, reuse_buffers=True))
    torch.manual_seed(2)
    b = list(st.recurrent_generator(st.get_advantages(), 2))
    assert len(a) == len(b) == 2
    for x, y in zip(a, b):
        assert tuple(x[2].shape) == (3 * 2, 2) and tuple(x[1].shape) == (1, 2, 4)
        assert pu.same_bytes(x[0]["x"], y[0]["x"]) and all(pu.same_bytes(p, q) for p, q in zip(x[1:], y[1:]))


@pytest.mark.parametrize("R,N_,n", [(1, 1, 1), (2, 3, 2), (5, 8, 3), (5, 8, 8)])
def test_gather_columns_on_cpu_tensors_is_index_select(R, N_, n):
    from wsmgmap import ops
    fields = pu.gather_fields(R, N_)
    ind = pu.perm_prefix(N_, n)
    got = ops.gather_columns(fields, ind)
    for name, g, w in zip(pu.WIDTHS, got, pu.gather_ref(fields, ind)):
        assert pu.same_bytes(g, w), name
    # rows: one fewer than stored for every field but the first, and `out` is what is written
    rows = [R] + [R - 1] * (len(fields) - 1)
    out = [torch.zeros((r, n) + tuple(f.shape[2:]), dtype=f.dtype) for f, r in zip(fields, rows)]
    again = ops.gather_columns(fields, ind, rows=rows, out=out)
    for name, g, o, w in zip(pu.WIDTHS, again, out, pu.gather_ref(fields, ind, rows)):
        assert g is o and pu.same_bytes(g, w), name


def test_gather_columns_refusals_name_the_operand():
    from wsmgmap import _abi, ops
    f = torch.zeros(2, 3, 4)
    ind = torch.tensor([1, 0])
    with pytest.raises(_abi.WsmgError, match=r"fields\[0\] is not contiguous"):
        ops.gather_columns([f.transpose(0, 1)], ind)
    with pytest.raises(_abi.WsmgError, match=r"out\[0\] must be"):
        ops.gather_columns([f], ind, out=[torch.zeros(2, 3, 4)])
    with pytest.raises(_abi.WsmgError, match="ind must be an int64"):
        ops.gather_columns([f], ind.int())
    with pytest.raises(_abi.WsmgError, match=r"rows\[0\] = 3"):
        ops.gather_columns([f], ind, rows=3)
    with pytest.raises(_abi.WsmgError, match=r"fields\[1\] has 2 columns"):
        ops.gather_columns([f, torch.zeros(2, 2, 1)], ind)
