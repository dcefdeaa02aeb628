"""CPU: the yardstick of the reward normaliser (tests/reward_norm_util.py) against an independent restatement, the stock arm of
`wsmgmap.rollout.RewardNormalizer` against the yardstick to the bit, `RolloutStorage(reward_normalizer=...)` on its torch route, and
the argument checks of the two ops and the two launchers (which refuse before anything touches a device)."""
import ctypes

import numpy as np
import pytest
import torch

import reward_norm_util as rn
import rollout_util as ru

G, CLIP, EPS = rn.GAMMA, rn.CLIP, rn.EPS


def _normalizer(N, **kw):
    from wsmgmap.rollout import RewardNormalizer
    return RewardNormalizer(N, G, **kw)


# ----------------------------------------------------------------------------- the yardstick
@pytest.mark.parametrize("T,N", [(1, 1), (9, 8), (40, 65), (7, 257)])
@pytest.mark.parametrize("kind", ["randn", "scaled_100", "zeros"])
def test_the_oracle_is_the_elementwise_welford_restatement(T, N, kind):
    """Batch merges of two-pass moments against one-value-at-a-time Welford updates: the same quantity rounded differently.  T N
    values enter a running mean / variance of order-one conditioning here: 1e-12 relative leaves three decimal orders over
    T N 2^-53 at the largest case, and an output formed from such a var is the oracle's float32 or its neighbour."""
    rewards, masks = rn.inputs(T, N, "random_20", kind)
    out, st = rn.reward_norm_ref(rewards, masks, rn.fresh_state(N, rn.case_count0(kind)))
    out_w, st_w = rn.reward_norm_welford(rewards, masks, rn.fresh_state(N, rn.case_count0(kind)))
    scale = abs(st[0]) + st[1] ** 0.5
    assert abs(st_w[0] - st[0]) <= 1e-12 * scale and abs(st_w[1] - st[1]) <= 1e-12 * st[1] and abs(st_w[2] - st[2]) <= 1e-12 * st[2]
    assert np.allclose(st_w[3:], st[3:], rtol=1e-13, atol=0)
    rn.assert_outputs(f"welford T{T} N{N} {kind}", torch.from_numpy(out_w.astype(np.float32)), out)


def test_case_table_holds_what_the_gpu_tests_promise():
    Ts, Ns = {t for t, _ in rn.SHAPES}, {n for _, n in rn.SHAPES}
    assert Ts == {1, 2, rn.PREFETCH - 1, rn.PREFETCH + 1, 40} and Ns == set(ru.ENVS) and (1, 1) in rn.SHAPES
    assert all(t * n <= 40 * 1024 for t, n in rn.SHAPES)


def test_the_clip_binds_on_scaled_rewards_and_nan_stays_nan():
    rewards, masks = rn.inputs(9, 8, "ones", "scaled_100")
    out, _ = rn.reward_norm_ref(rewards, masks, rn.fresh_state(8, rn.SCALED_COUNT0))
    assert (np.abs(out[:2]) == np.float32(CLIP)).any() and (np.abs(out) <= np.float32(CLIP)).all()
    rewards, masks = rn.inputs(9, 8, "ones", "nan_3_2")
    out, st = rn.reward_norm_ref(rewards, masks, rn.fresh_state(8))
    assert np.isnan(out[3, 2]) and not np.isnan(out[:3]).any() and np.isnan(out[3:]).all() and np.isnan(st[:2]).all()
    assert not np.isnan(st[3:][[0, 1, 3, 4, 5, 6, 7]]).any() and st[2] == rn.f32_scalar(rn.COUNT0) + 72


def test_a_zero_mask_restarts_the_carry():
    rewards, masks = rn.inputs(5, 3, "ones")
    masks[5, 1] = 0
    _, st = rn.reward_norm_ref(rewards, masks, rn.fresh_state(3))
    assert st[3 + 1] == 0.0 and st[3] != 0.0 and st[3 + 2] != 0.0


# ----------------------------------------------------------------------------- the stock arm
@pytest.mark.parametrize("T,N", rn.SHAPES)
def test_stock_arm_is_the_oracle_to_the_bit(T, N):
    for mask_kind in ru.MASKS:
        rewards, masks = rn.inputs(T, N, mask_kind)
        nz = _normalizer(N)
        assert rn.same_bits64(nz.state, rn.fresh_state(N))
        out = nz.normalize(rewards, masks)
        ref, st = rn.reward_norm_ref(rewards, masks, rn.fresh_state(N))
        assert tuple(out.shape) == (T, N, 1) and ru.same_bits(out, ref), (T, N, mask_kind)
        assert rn.same_bits64(nz.state, st), (T, N, mask_kind)


@pytest.mark.parametrize("kind", ["scaled_100", "zeros", "nan_3_2"])
def test_stock_arm_on_the_special_inputs(kind):
    T, N = 9, 8
    rewards, masks = rn.inputs(T, N, "random_20", kind)
    nz = _normalizer(N, count0=rn.case_count0(kind))
    out = nz.normalize(rewards, masks)
    ref, st = rn.reward_norm_ref(rewards, masks, rn.fresh_state(N, rn.case_count0(kind)))
    assert ru.same_bits(out, ref) and rn.same_bits64(nz.state, st)
    if kind == "scaled_100":
        assert (out.abs() == CLIP).any()
    if kind == "zeros":
        assert float(out.abs().max()) == 0.0 and float(nz.returns.abs().max()) == 0.0 and 0.0 < float(nz.var) < 1.0


@pytest.mark.parametrize("T,N,T1", [(9, 8, 4), (40, 65, 17), (2, 1, 1), (7, 3, 0), (7, 3, 7)])
def test_two_calls_are_one_call(T, N, T1):
    """Rows [0, T1) in a first call over the T1-row prefix, the rest with first_row = T1: state and outputs of the one call."""
    rewards, masks = rn.inputs(T, N)
    one = _normalizer(N)
    ref = one.normalize(rewards, masks)
    two = _normalizer(N)
    out = torch.full_like(rewards, 7.0)
    if T1:
        two.normalize(rewards[:T1], masks[:T1 + 1], out=out[:T1])
    got = two.normalize(rewards, masks, first_row=T1, out=out)
    assert got.data_ptr() == out.data_ptr() and ru.same_bits(out, ref) and rn.same_bits64(one.state, two.state)
    o, st = rn.reward_norm_ref(rewards, masks, rn.fresh_state(N))
    assert ru.same_bits(ref, o) and rn.same_bits64(one.state, st)


def test_first_row_leaves_the_rows_below_it_alone():
    T, N = 9, 8
    rewards, masks = rn.inputs(T, N)
    nz = _normalizer(N)
    out = torch.full_like(rewards, 7.0)
    nz.normalize(rewards, masks, first_row=4, out=out)
    ref, st = rn.reward_norm_ref(rewards, masks, rn.fresh_state(N), first_row=4)
    assert float((out[:4] - 7.0).abs().max()) == 0.0 and ru.same_bits(out[4:], ref[4:]) and rn.same_bits64(nz.state, st)
    assert float(nz.count) == rn.f32_scalar(rn.COUNT0) + 5 * N


def test_state_dict_round_trip_continues_the_sequence():
    T, N = 9, 8
    a_r, a_m = rn.inputs(T, N, seed=1)
    b_r, b_m = rn.inputs(T, N, seed=2)
    one = _normalizer(N)
    one.normalize(a_r, a_m)
    sd = one.state_dict()
    want = one.normalize(b_r, b_m)
    two = _normalizer(N, clip=3.0, eps=1e-3)
    two.load_state_dict(sd)
    assert (two.gamma, two.clip, two.eps) == (one.gamma, one.clip, one.eps)
    got = two.normalize(b_r, b_m)
    assert ru.same_bits(got, want) and rn.same_bits64(one.state, two.state)
    assert not rn.same_bits64(sd["state"], one.state)          # (the dict holds a copy, not the live tensor)
    with pytest.raises(ValueError, match="state"):
        _normalizer(N + 1).load_state_dict(sd)


def test_eval_leaves_the_state_untouched_and_uses_the_stored_var():
    T, N = 9, 8
    rewards, masks = rn.inputs(T, N)
    nz = _normalizer(N)
    nz.normalize(rewards, masks)
    before = nz.state.clone()
    assert nz.eval() is nz and not nz.training
    out = nz.normalize(rewards * 100.0, masks)
    ref, st = rn.reward_norm_ref(rewards * 100.0, masks, before, update=False)
    assert rn.same_bits64(nz.state, before) and rn.same_bits64(st, before) and ru.same_bits(out, ref)
    assert (out.abs() == CLIP).any()
    sd = float(torch.sqrt(before[1] + rn.f32_scalar(EPS)))
    assert float(out[0, 0]) == float(np.float32(min(max(float((rewards * 100.0)[0, 0]) / sd, -CLIP), CLIP)))
    assert nz.train() is nz and nz.training
    nz.normalize(rewards, masks)
    assert not rn.same_bits64(nz.state, before)


def test_views_and_argument_checks_of_the_class():
    nz = _normalizer(4, count0=0.5)
    assert float(nz.mean) == 0.0 and float(nz.var) == 1.0 and float(nz.count) == 0.5 and tuple(nz.returns.shape) == (4,)
    nz.returns[2] = 3.0
    assert float(nz.state[5]) == 3.0 and nz.state.dtype == torch.float64 and nz.to("cpu") is nz
    rewards, masks = rn.inputs(3, 4)
    for bad in (lambda: nz.normalize(rewards[:, :3], masks), lambda: nz.normalize(rewards, masks[:3]),
                lambda: nz.normalize(rewards, masks, first_row=4), lambda: nz.normalize(rewards, masks, first_row=-1),
                lambda: nz.normalize(rewards, masks, out=torch.zeros(3, 4)),
                lambda: nz.normalize(rewards, masks, out=torch.zeros(3, 8, 1)[:, ::2])):
        before = nz.state.clone()
        with pytest.raises(ValueError, match="RewardNormalizer"):
            bad()
        assert rn.same_bits64(nz.state, before)
    with pytest.raises(ValueError, match="num_envs"):
        _normalizer(0)
    # other dtypes go through the stock arm and are rounded once to the output's dtype
    out = _normalizer(4).normalize(rewards.double(), masks.double())
    ref, _ = rn.reward_norm_ref(rewards, masks, rn.fresh_state(4))
    assert out.dtype == torch.float64 and ru.same_bits(out.float(), ref)


# ----------------------------------------------------------------------------- RolloutStorage on CPU tensors
def _storage(T, N, nz, **kw):
    from wsmgmap.rollout import RolloutStorage
    return RolloutStorage(T, N, {"x": ((3,), torch.float32)}, 2, 4, reward_normalizer=nz, **kw)


def _fill(st, N, steps, seed=0, first=0):
    g = torch.Generator(); g.manual_seed(4000 + N + seed)
    rows = [({"x": torch.randn(N, 3, generator=g)}, torch.randn(1, N, 4, generator=g), torch.randn(N, 2, generator=g),
             torch.randn(N, generator=g), torch.randn(N, 1, generator=g), torch.randn(N, 1, generator=g),
             (torch.rand(N, 1, generator=g) >= 0.2).float()) for _ in range(first + steps)]
    for row in rows[first:]:
        st.insert(*row)


@pytest.mark.parametrize("use_gae", [True, False], ids=["gae", "discounted"])
def test_storage_returns_are_the_float32_loop_on_its_own_normalised_rewards(use_gae):
    T, N = 9, 5
    nz = _normalizer(N)
    st = _storage(T, N, nz, fused=False)
    assert st.rewards_normalized is None
    _fill(st, N, T)
    raw = st.rewards.clone()
    st.returns.fill_(7.0)
    nv = torch.linspace(-1.0, 1.0, N).view(N, 1)
    before = st.value_preds.clone()
    st.compute_returns(nv, use_gae, 0.99, 0.95)
    want, state = rn.reward_norm_ref(raw, st.masks, rn.fresh_state(N))
    assert tuple(st.rewards_normalized.shape) == (T, N, 1) and ru.same_bits(st.rewards_normalized, want)
    assert rn.same_bits64(nz.state, state) and torch.equal(st.rewards, raw)
    ref = ru.gae_ref(st.rewards_normalized, before, st.masks, nv, 0.99, 0.95, use_gae, returns=torch.full((T + 1, N, 1), 7.0))
    assert ru.same_bits(st.returns, ref["returns"]) and ru.same_bits(st.value_preds, ref["value_preds"])
    assert ru.same_bits(st.get_advantages(use_normalized_advantage=False), ref["adv"])
    # a second compute_returns over the same rows: nothing moves
    snap = [t.clone() for t in (st.returns, st.value_preds, st.rewards_normalized, nz.state)]
    st.compute_returns(nv, use_gae, 0.99, 0.95)
    for a, b in zip(snap, (st.returns, st.value_preds, st.rewards_normalized, nz.state)):
        assert torch.equal(a, b)
    assert torch.equal(st.rewards, raw)


def test_storage_inserts_then_compute_returns_equal_the_one_shot_result():
    T, N = 9, 5
    nv = torch.linspace(-1.0, 1.0, N).view(N, 1)
    one_nz, two_nz = _normalizer(N), _normalizer(N)
    one, two = _storage(T, N, one_nz), _storage(T, N, two_nz)          # (fused=True on the CPU: the torch route all the same)
    _fill(one, N, T)
    one.compute_returns(nv, True, 0.99, 0.95)
    _fill(two, N, 4)
    two.compute_returns(nv, True, 0.99, 0.95)
    assert float(two_nz.count) == rn.f32_scalar(rn.COUNT0) + 4 * N
    _fill(two, N, T - 4, first=4)
    assert torch.equal(one.rewards, two.rewards)
    two.compute_returns(nv, True, 0.99, 0.95)
    assert ru.same_bits(one.rewards_normalized, two.rewards_normalized) and rn.same_bits64(one_nz.state, two_nz.state)
    assert ru.same_bits(one.returns, two.returns)
    # after_update forgets the rows, not the statistics or the carry: the next rollout continues the sequence
    carry = two_nz.state.clone()
    for st in (one, two):
        st.after_update()
        _fill(st, N, 3, seed=9)
        st.compute_returns(nv, True, 0.99, 0.95)
    want, state = rn.reward_norm_ref(two.rewards[:3], two.masks[:4], carry)
    assert ru.same_bits(two.rewards_normalized[:3], want) and rn.same_bits64(two_nz.state, state)
    assert rn.same_bits64(one_nz.state, two_nz.state) and float(two_nz.count) == rn.f32_scalar(rn.COUNT0) + (T + 3) * N


def test_storage_without_a_normaliser_is_what_it_was():
    T, N = 5, 3
    st = _storage(T, N, None)
    _fill(st, N, T)
    nv = torch.zeros(N, 1)
    ref = ru.gae_ref(st.rewards, st.value_preds, st.masks, nv, 0.99, 0.95, True, returns=st.returns)
    st.compute_returns(nv, True, 0.99, 0.95)
    assert st.rewards_normalized is None and st.reward_normalizer is None and ru.same_bits(st.returns, ref["returns"])


def test_storage_checks_the_normalisers_width_and_moves_it():
    with pytest.raises(ValueError, match="environments"):
        _storage(4, 3, _normalizer(2))
    nz = _normalizer(3)
    st = _storage(4, 3, nz)
    assert st.to("cpu") is st and st.reward_normalizer is nz and nz.state.device.type == "cpu"


# ----------------------------------------------------------------------------- the ops and the launchers refuse bad input
def test_ops_refuse_cpu_tensors():
    from wsmgmap import ops
    rewards, masks = rn.inputs(4, 3)
    state = torch.from_numpy(rn.fresh_state(3))
    with pytest.raises(ops._abi.WsmgError, match="GPU"):
        ops.normalize_rewards(rewards, masks, state, G, CLIP, EPS)
    with pytest.raises(ops._abi.WsmgError, match="GPU"):
        ops.normalized_gae_returns(rewards, torch.zeros(5, 3, 1), masks, torch.zeros(3, 1), 0.99, 0.95, state, G, CLIP, EPS)
    assert not ops.reward_normalize_ok(rewards, masks, state)


def test_the_launchers_refuse_their_limits_before_touching_a_device():
    """WSMG_EINVAL is answered before anything is enqueued, so the pointers need not be device memory here: host buffers stand in
    and stay as they were."""
    from wsmgmap import _abi
    L = _abi.lib()
    for name in ("wsmg_reward_normalize", "wsmg_gae_returns_normalized"):
        assert name in _abi.exported_names() and hasattr(L, name)
    bufs = {k: torch.full((64,), 7.0) for k in ("rewards", "masks", "out", "vp", "nv", "ret")}
    state = torch.full((8,), 7.0, dtype=torch.float64)
    p = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())      # noqa: E731

    def norm(T, N, s0, drop=None):
        a = [bufs["rewards"], bufs["masks"], state, bufs["out"]]
        if drop is not None:
            a[drop] = None
        return L.wsmg_reward_normalize(p(a[0]), p(a[1]), p(a[2]), 0.99, 10.0, 1e-8, T, N, s0, 1, p(a[3]), None)

    def fused(T, N, s0, drop=None):
        a = [bufs["rewards"], bufs["masks"], state, bufs["out"], bufs["vp"], bufs["nv"], bufs["ret"]]
        if drop is not None:
            a[drop] = None
        return L.wsmg_gae_returns_normalized(p(a[0]), p(a[1]), p(a[2]), 0.99, 10.0, 1e-8, s0, 1, p(a[3]), p(a[4]), p(a[5]), 0.99,
                                             0.9405, 1, T, N, p(a[6]), None, None, None, 1e-5, None)

    for fn, ptrs in ((norm, 4), (fused, 7)):
        for T, N, s0 in ((0, 3, 0), (-1, 3, 0), (2, 0, 0), (2, 1025, 0), (16384, 1024, 0), (2, 3, 3), (2, 3, -1)):
            assert fn(T, N, s0) == -1, (fn.__name__, T, N, s0)
        for drop in range(ptrs):
            assert fn(2, 3, 0, drop) == -1, (fn.__name__, drop)
    assert all(float((t - 7.0).abs().max()) == 0.0 for t in bufs.values()) and float((state - 7.0).abs().max()) == 0.0
