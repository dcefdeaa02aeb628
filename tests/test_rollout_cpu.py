"""CPU: the yardstick of the rollout's returns and advantages (tests/rollout_util.py) against an independent restatement and against
the properties that make the recurrence checkable by eye, and `wsmgmap.rollout.RolloutStorage` on CPU tensors (its torch-loop route
and its plumbing: insert, after_update, the minibatch generator)."""
import numpy as np
import pytest
import torch

import rollout_util as ru


# ----------------------------------------------------------------------------- the yardstick
@pytest.mark.parametrize("use_gae", [True, False], ids=["gae", "discounted"])
@pytest.mark.parametrize("gamma,tau", [(0.99, 0.95), (1.0, 1.0), (0.9, 0.0)])
@pytest.mark.parametrize("T,N", [(1, 1), (5, 3), (64, 8), (200, 65)])
def test_float32_torch_loop_is_the_elementwise_float32_restatement_to_the_bit(T, N, gamma, tau, use_gae):
    rewards, value_preds, masks, next_value = ru.inputs(T, N, "random_20")
    ref = ru.gae_ref(rewards, value_preds, masks, next_value, gamma, tau, use_gae)
    ret, v, adv = ru.gae_numpy(rewards, value_preds, masks, next_value, gamma, tau, use_gae)
    assert ru.same_bits(ref["returns"], ret) and ru.same_bits(ref["value_preds"], v) and ru.same_bits(ref["adv"], adv)
    assert bool(torch.isnan(ref["returns"][T]).all()) == use_gae          # GAE leaves row T alone
    assert ru.same_bits(ref["value_preds"][T], next_value if use_gae else torch.full((N, 1), 123.0))


@pytest.mark.parametrize("use_gae", [True, False], ids=["gae", "discounted"])
def test_float32_loop_sits_within_rounding_of_the_float64_oracle(use_gae):
    """T = 200 steps of four operations each, |values| of a few units: the float32 loop's distance from float64 stays below
    T x 8 ulp of the largest return (a loose ceiling: the recurrence damps with gamma = 0.99; what matters is that it is small and
    not zero, so that the 4 x rule of the GPU tests has a bar above its floor)."""
    T, N = 200, 65
    inp = ru.inputs(T, N, "random_20")
    r32, r64 = ru.gae_ref(*inp, 0.99, 0.95, use_gae), ru.gae_ref(*inp, 0.99, 0.95, use_gae, dtype=torch.float64)
    for k in ("adv", "adv_norm", "stats"):
        e = float((r32[k].double() - r64[k]).abs().max())
        scale = float(r64["returns"][:T].abs().max())
        print(f"{k}: float32 loop off float64 by {e:.3e} (max |returns| {scale:.3e})")
        assert 0.0 < e <= T * 8 * 2.0 ** -24 * scale


def test_tau_zero_gives_the_one_step_return():
    T, N = 7, 5
    rewards, value_preds, masks, next_value = ru.inputs(T, N, "random_20")
    ref = ru.gae_ref(rewards, value_preds, masks, next_value, 0.9, 0.0, True)
    v = ref["value_preds"]
    # returns[s] = (delta + 0 * g) + v[s] with delta = r + gamma v' m - v: the one-step target up to the two roundings of - v + v
    want = rewards + 0.9 * v[1:] * masks[1:]
    assert torch.allclose(ref["returns"][:T], want, rtol=0, atol=4 * 2.0 ** -24 * float(want.abs().max() + v.abs().max()))


@pytest.mark.parametrize("use_gae", [True, False], ids=["gae", "discounted"])
def test_gamma_zero_gives_the_rewards(use_gae):
    T, N = 7, 5
    rewards, value_preds, masks, next_value = ru.inputs(T, N, "random_20")
    ref = ru.gae_ref(rewards, value_preds, masks, next_value, 0.0, 0.95, use_gae)
    if use_gae:     # (r + 0 - v) + v: two roundings
        assert torch.allclose(ref["returns"][:T], rewards, rtol=0, atol=4 * 2.0 ** -24 * float(rewards.abs().max() + value_preds.abs().max()))
    else:
        assert torch.equal(ref["returns"][:T], rewards)


@pytest.mark.parametrize("use_gae", [True, False], ids=["gae", "discounted"])
def test_a_zero_mask_cuts_everything_after_it_off(use_gae):
    """masks[s+1] = 0 for one environment: its rows <= s do not depend on anything after s (rewards, values, next_value)."""
    T, N, cut = 9, 3, 4
    rewards, value_preds, masks, next_value = ru.inputs(T, N, "ones")
    masks[cut + 1, 1] = 0
    a = ru.gae_ref(rewards, value_preds, masks, next_value, 0.99, 0.95, use_gae)
    r2, v2 = rewards.clone(), value_preds.clone()
    r2[cut + 1:, 1] += 5.0
    v2[cut + 1:, 1] -= 3.0
    b = ru.gae_ref(r2, v2, masks, next_value * 2 + 1, 0.99, 0.95, use_gae)
    assert ru.same_bits(a["returns"][:cut + 1, 1], b["returns"][:cut + 1, 1])
    assert not torch.equal(a["returns"][:cut + 1, 0], b["returns"][:cut + 1, 0])        # the live neighbour sees next_value
    assert not torch.equal(a["returns"][cut + 1:T, 1], b["returns"][cut + 1:T, 1])


@pytest.mark.parametrize("use_gae", [True, False], ids=["gae", "discounted"])
def test_a_zero_last_mask_makes_next_value_irrelevant(use_gae):
    T, N = 6, 4
    rewards, value_preds, masks, next_value = ru.inputs(T, N, "zero_row_T")
    a = ru.gae_ref(rewards, value_preds, masks, next_value, 0.99, 0.95, use_gae)
    b = ru.gae_ref(rewards, value_preds, masks, next_value * -7 + 2, 0.99, 0.95, use_gae)
    assert ru.same_bits(a["returns"][:T], b["returns"][:T]) and ru.same_bits(a["adv"], b["adv"])


def test_case_table_holds_what_the_gpu_tests_promise():
    Ts, Ns = {t for t, _ in ru.SHAPES}, {n for _, n in ru.SHAPES}
    assert set(range(1, ru.PREFETCH + 3)) | {64, 200} <= Ts and set(ru.ENVS) <= Ns
    assert all(t * n < 60000 for t, n in ru.SHAPES)          # large N only with small T: nothing is slow
    assert len(ru.MASKS) == 6 and len(ru.GAMMA_TAU) == 4


# ----------------------------------------------------------------------------- RolloutStorage on CPU tensors
T_, N_, A_, H_, L_ = 3, 4, 2, 6, 2
OBS = {"rgb": ((5, 5, 3), torch.uint8), "depth": ((5, 5, 1), torch.float32), "progress": ((1,), np.float32)}


def _storage(**kw):
    from wsmgmap.rollout import RolloutStorage
    return RolloutStorage(T_, N_, OBS, A_, H_, L_, **kw)


def _step_data(i):
    g = torch.Generator(); g.manual_seed(50 + i)
    obs = {"rgb": torch.randint(0, 256, (N_, 5, 5, 3), generator=g, dtype=torch.uint8), "depth": torch.rand(N_, 5, 5, 1, generator=g),
           "progress": torch.rand(N_, 1, generator=g)}
    return dict(observations=obs, recurrent_hidden_states=torch.randn(L_, N_, H_, generator=g), actions=torch.randn(N_, A_, generator=g),
                action_log_probs=torch.randn(N_, generator=g), value_preds=torch.randn(N_, 1, generator=g),
                rewards=torch.randn(N_, 1, generator=g), masks=(torch.rand(N_, 1, generator=g) > 0.3).float())


def _filled(steps=T_, **kw):
    st = _storage(**kw)
    data = [_step_data(i) for i in range(steps)]
    for d in data:
        st.insert(**d)
    return st, data


def test_storage_shapes_and_dtypes():
    st = _storage()
    assert st.observations["rgb"].dtype == torch.uint8 and tuple(st.observations["rgb"].shape) == (T_ + 1, N_, 5, 5, 3)
    assert st.observations["progress"].dtype == torch.float32 and tuple(st.observations["progress"].shape) == (T_ + 1, N_, 1)
    assert tuple(st.recurrent_hidden_states.shape) == (T_ + 1, L_, N_, H_)
    for name, shape in (("rewards", (T_, N_, 1)), ("value_preds", (T_ + 1, N_, 1)), ("returns", (T_ + 1, N_, 1)),
                        ("action_log_probs", (T_, N_, 1)), ("actions", (T_, N_, A_)), ("prev_actions", (T_ + 1, N_, A_)),
                        ("masks", (T_ + 1, N_, 1))):
        t = getattr(st, name)
        assert tuple(t.shape) == shape and t.dtype == torch.float32 and float(t.abs().max()) == 0.0, name
    assert st.step == 0 and st.to("cpu") is st


def test_storage_reads_a_dict_space_by_shape_and_dtype():
    from wsmgmap.rollout import RolloutStorage

    class Space:
        def __init__(self, shape, dtype):
            self.shape, self.dtype = shape, dtype

    class Dict:
        spaces = {"rgb": Space((4, 4, 3), np.uint8), "depth": Space((4, 4, 1), np.float32)}

    st = RolloutStorage(2, 3, Dict(), 2, 4)
    assert st.observations["rgb"].dtype == torch.uint8 and tuple(st.observations["depth"].shape) == (3, 3, 4, 4, 1)
    assert tuple(st.recurrent_hidden_states.shape) == (3, 1, 3, 4)


def test_insert_puts_every_field_where_habitat_puts_it():
    st, data = _filled(2)
    assert st.step == 2
    for s, d in enumerate(data):
        for k, v in d["observations"].items():
            assert torch.equal(st.observations[k][s + 1], v) and st.observations[k].dtype == v.dtype, k
        assert torch.equal(st.recurrent_hidden_states[s + 1], d["recurrent_hidden_states"])
        assert torch.equal(st.actions[s], d["actions"]) and torch.equal(st.prev_actions[s + 1], d["actions"])
        assert torch.equal(st.action_log_probs[s], d["action_log_probs"].view(N_, 1))
        assert torch.equal(st.value_preds[s], d["value_preds"]) and torch.equal(st.rewards[s], d["rewards"])
        assert torch.equal(st.masks[s + 1], d["masks"])
    # row 0 of the step + 1 fields and everything past the inserted rows are untouched
    assert float(st.masks[0].abs().max()) == 0.0 and float(st.prev_actions[0].abs().max()) == 0.0
    assert float(st.observations["rgb"][0].max()) == 0 and float(st.rewards[2].abs().max()) == 0.0 and float(st.masks[3].abs().max()) == 0.0


def test_insert_past_num_steps_is_refused():
    st, _ = _filled()
    before = st.rewards.clone()
    with pytest.raises(ValueError, match="full"):
        st.insert(**_step_data(9))
    assert st.step == T_ and torch.equal(st.rewards, before)


def test_after_update_carries_the_last_row_to_row_zero():
    st, data = _filled(2)
    st.after_update()
    last = data[1]
    assert st.step == 0
    for k, v in last["observations"].items():
        assert torch.equal(st.observations[k][0], v)
    assert torch.equal(st.recurrent_hidden_states[0], last["recurrent_hidden_states"])
    assert torch.equal(st.masks[0], last["masks"]) and torch.equal(st.prev_actions[0], last["actions"])


@pytest.mark.parametrize("use_gae", [True, False], ids=["gae", "discounted"])
def test_compute_returns_on_cpu_is_the_yardstick_and_mutates_what_habitat_mutates(use_gae):
    st, _ = _filled()
    nv = torch.tensor([[0.5], [-1.5], [2.0], [0.25]])
    st.returns.fill_(7.0)
    st.value_preds[T_] = 123.0
    ref = ru.gae_ref(st.rewards, st.value_preds, st.masks, nv, 0.99, 0.95, use_gae, returns=st.returns)
    st.compute_returns(nv, use_gae, 0.99, 0.95)
    assert ru.same_bits(st.returns, ref["returns"]) and ru.same_bits(st.value_preds, ref["value_preds"])
    if use_gae:
        assert torch.equal(st.value_preds[T_], nv) and float((st.returns[T_] - 7.0).abs().max()) == 0.0
    else:
        assert torch.equal(st.returns[T_], nv) and float((st.value_preds[T_] - 123.0).abs().max()) == 0.0


@pytest.mark.parametrize("use_gae", [True, False], ids=["gae", "discounted"])
def test_a_partial_rollout_touches_only_the_rows_in_use(use_gae):
    st, _ = _filled(2)
    nv = torch.tensor([[0.5], [-1.5], [2.0], [0.25]])
    st.returns.fill_(7.0)
    st.value_preds[2:] = 123.0
    ref = ru.gae_ref(st.rewards[:2], st.value_preds[:3], st.masks[:3], nv, 0.99, 0.95, use_gae, returns=st.returns[:3])
    st.compute_returns(nv, use_gae, 0.99, 0.95)
    assert ru.same_bits(st.returns[:3], ref["returns"]) and ru.same_bits(st.value_preds[:3], ref["value_preds"])
    assert float((st.returns[3] - 7.0).abs().max()) == 0.0 and float((st.value_preds[3] - 123.0).abs().max()) == 0.0
    adv = st.get_advantages(use_normalized_advantage=False)
    assert tuple(adv.shape) == (2, N_, 1) and ru.same_bits(adv, ref["adv"])


def test_get_advantages_is_torchs_own_mean_and_std_expression():
    st, _ = _filled()
    st.compute_returns(torch.zeros(N_, 1), True, 0.99, 0.95)
    a = st.returns[:-1] - st.value_preds[:-1]
    assert torch.equal(st.get_advantages(use_normalized_advantage=False), a)
    assert torch.equal(st.get_advantages(), (a - a.mean()) / (a.std() + 1e-5))
    assert torch.equal(st.get_advantages(eps=1e-3), (a - a.mean()) / (a.std() + 1e-3))


@pytest.mark.parametrize("num_mini_batch", [1, 2, 4])
def test_recurrent_generator_batches_against_a_loop_built_yardstick(num_mini_batch):
    """habitat-baselines' generator, loop for loop: per chunk of the permutation, per environment of the chunk, append the [:step]
    column; stack along dimension 1; flatten (step, n)."""
    st, _ = _filled()
    st.compute_returns(torch.ones(N_, 1), True, 0.99, 0.95)
    adv = st.get_advantages()
    torch.manual_seed(11)
    batches = list(st.recurrent_generator(adv, num_mini_batch))
    torch.manual_seed(11)
    perm = torch.randperm(N_)
    per = N_ // num_mini_batch
    assert len(batches) == num_mini_batch
    flat = lambda cols: torch.stack(cols, 1).reshape(T_ * per, *cols[0].shape[1:])      # noqa: E731
    for b, got in enumerate(batches):
        envs = [int(perm[b * per + j]) for j in range(per)]
        want = ({k: flat([v[:T_, e] for e in envs]) for k, v in st.observations.items()},
                torch.stack([st.recurrent_hidden_states[0, :, e] for e in envs], 1),
                *(flat([t[:T_, e] for e in envs]) for t in (st.actions, st.prev_actions, st.value_preds, st.returns, st.masks,
                                                            st.action_log_probs, adv)))
        assert len(got) == 9 and set(got[0]) == set(OBS)
        for k in OBS:
            assert torch.equal(got[0][k], want[0][k]) and got[0][k].dtype == st.observations[k].dtype, k
        assert tuple(got[1].shape) == (L_, per, H_)
        for i in range(1, 9):
            assert torch.equal(got[i], want[i]), i
    seen = sorted(int(e) for b in range(num_mini_batch) for e in perm[b * per:(b + 1) * per])
    assert seen == list(range(N_))


def test_recurrent_generator_refuses_more_minibatches_than_environments():
    st, _ = _filled()
    with pytest.raises(ValueError, match="minibatches"):
        next(st.recurrent_generator(torch.zeros(T_, N_, 1), N_ + 1))


def test_uint8_observations_stay_uint8_through_insert_update_and_batches():
    st, data = _filled()
    st.after_update()
    assert st.observations["rgb"].dtype == torch.uint8 and torch.equal(st.observations["rgb"][0], data[-1]["observations"]["rgb"])
    st.insert(**data[0])
    batch = next(st.recurrent_generator(torch.zeros(T_, N_, 1), 1))
    assert batch[0]["rgb"].dtype == torch.uint8 and tuple(batch[0]["rgb"].shape) == (1 * N_, 5, 5, 3)


def test_cpu_storage_takes_the_torch_route_whatever_fused_says():
    a, _ = _filled(fused=True)
    b, _ = _filled(fused=False)
    nv = torch.full((N_, 1), 0.5)
    for st in (a, b):
        st.compute_returns(nv, True, 0.99, 0.95)
    assert not a._fused_route() and ru.same_bits(a.returns[:T_], b.returns[:T_])
    assert torch.equal(a.get_advantages(), b.get_advantages())
