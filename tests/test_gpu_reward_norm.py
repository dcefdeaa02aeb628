"""GPU: the reward normaliser (csrc/wsmg_pg_rollout.hip) through `ops.normalize_rewards`, `ops.normalized_gae_returns`, the C ABI and
`wsmgmap.rollout.RewardNormalizer` / `RolloutStorage(reward_normalizer=...)`, against the yardsticks of tests/reward_norm_util.py.

The bars are derived there, not tuned.  `count` equals the oracle's exactly.  `mean`, `var` and the carry differ from the oracle by
the order of two float64 sums of N terms per step: (N + 16) T 2^-53, times 4.  An output is formed in float64 and rounded once: it is
within one float32 ulp of the oracle's, exact at the clip, NaN where the oracle's is.  The one-launch form is held to the BITS of the
normalising launch alone and of `wsmg_gae_returns` / the float32 torch loop fed its `rewards_out`.  Every comparison of a state prints
its figures before it asserts (`-s` shows them; profiles/reward_norm.txt keeps a run's).

Measured on the MI355X (worst error / bar over the file): mean 0.0003, var 0.015, the carry equal to the oracle's everywhere."""
import ctypes

import pytest
import torch

import reward_norm_util as rn
import rollout_util as ru

pytestmark = pytest.mark.gpu

NAN = float("nan")
G, CLIP, EPS = rn.GAMMA, rn.CLIP, rn.EPS


def _launch(rewards, masks, state, first_row=0, update=True, clip=CLIP):
    """ops.normalize_rewards on copies, the output NaN-filled and a row too long.  -> (out [T, N, 1] on the CPU, state on the CPU)"""
    from wsmgmap import ops
    T, N = rewards.shape[0], rewards.shape[1]
    r, m = rewards.cuda(), masks.cuda()
    st = torch.full((4 + N,), NAN, device="cuda", dtype=torch.float64)
    st[:3 + N] = torch.as_tensor(state)
    big = torch.full((T + 1, N, 1), NAN, device="cuda")
    out = ops.normalize_rewards(r, m, st[:3 + N], G, clip, EPS, first_row=first_row, update=update, out=big[:T])
    torch.cuda.synchronize()
    assert out.data_ptr() == big.data_ptr() and torch.isnan(big[T]).all() and torch.isnan(st[3 + N]), "a guard was written"
    assert torch.isnan(big[:first_row]).all(), "a row below first_row was written"
    assert ru.same_bits(r, rewards) and ru.same_bits(m, masks), "an input was written"
    return big[:T].cpu(), st[:3 + N].cpu()


# ----------------------------------------------------------------------------- the normalising launch
@pytest.mark.parametrize("T,N", rn.SHAPES)
def test_state_and_outputs_sit_within_the_derived_bars(T, N):
    for mask_kind in ru.MASKS:
        rewards, masks = rn.inputs(T, N, mask_kind)
        ref, want = rn.reward_norm_ref(rewards, masks, rn.fresh_state(N))
        out, state = _launch(rewards, masks, rn.fresh_state(N))
        tag = f"T{T} N{N} {mask_kind}"
        rn.assert_state(tag, state, want, N, T)
        rn.assert_outputs(tag, out, ref)


@pytest.mark.parametrize("T,N", [(9, 8), (7, 1), (40, 257)])
def test_scaled_rewards_are_clipped_exactly(T, N):
    rewards, masks = rn.inputs(T, N, "random_20", "scaled_100")
    st0 = rn.fresh_state(N, rn.SCALED_COUNT0)
    ref, want = rn.reward_norm_ref(rewards, masks, st0)
    out, state = _launch(rewards, masks, st0)
    rn.assert_state(f"scaled T{T} N{N}", state, want, N, T)
    at_clip = rn.assert_outputs(f"scaled T{T} N{N}", out, ref)
    assert at_clip > 0 and (out[:2].abs() == CLIP).any() and float(out.abs().max()) == CLIP


def test_zero_rewards_a_single_entry_and_a_nan():
    rewards, masks = rn.inputs(9, 8, "random_20", "zeros")
    ref, want = rn.reward_norm_ref(rewards, masks, rn.fresh_state(8))
    out, state = _launch(rewards, masks, rn.fresh_state(8))
    assert float(out.abs().max()) == 0.0 and rn.same_bits64(state, want)          # sums of zeros have no order
    rewards, masks = rn.inputs(1, 1, "ones")
    ref, want = rn.reward_norm_ref(rewards, masks, rn.fresh_state(1))
    out, state = _launch(rewards, masks, rn.fresh_state(1))
    assert rn.same_bits64(state, want) and ru.same_bits(out, ref)                  # one term: no order either
    rewards, masks = rn.inputs(9, 8, "ones", "nan_3_2")
    ref, want = rn.reward_norm_ref(rewards, masks, rn.fresh_state(8))
    out, state = _launch(rewards, masks, rn.fresh_state(8))
    rn.assert_state("nan", state, want, 8, 9)
    rn.assert_outputs("nan", out, ref)
    assert torch.isnan(out[3, 2]) and torch.isnan(out[3:]).all() and not torch.isnan(out[:3]).any() and torch.isnan(state[:2]).all()


@pytest.mark.parametrize("T,N", [(9, 8), (40, 65), (7, 1024)])
def test_update_false_uses_the_stored_var_and_writes_no_state(T, N):
    rewards, masks = rn.inputs(T, N)
    _, st0 = rn.reward_norm_ref(rewards, masks, rn.fresh_state(N))
    for first_row in (0, T // 2):
        ref, _ = rn.reward_norm_ref(rewards * 100.0, masks, st0, update=False, first_row=first_row)
        out, state = _launch(rewards * 100.0, masks, st0, first_row=first_row, update=False)
        assert rn.same_bits64(state, st0)
        assert rn.assert_outputs(f"frozen T{T} N{N}", out[first_row:], ref[first_row:]) > 0


@pytest.mark.parametrize("T,N,T1", [(9, 8, 4), (40, 257, 17), (9, 1024, 8), (2, 1, 1)])
def test_first_row_in_the_middle_continues_a_first_call(T, N, T1):
    """Two launches (T1 rows, then the rest with first_row = T1) against one launch: the same operations in the same order, so the
    same bits, state and outputs; and both inside the bars of the oracle."""
    from wsmgmap import ops
    rewards, masks = rn.inputs(T, N)
    one_out, one_state = _launch(rewards, masks, rn.fresh_state(N))
    r, m = rewards.cuda(), masks.cuda()
    st = torch.from_numpy(rn.fresh_state(N)).cuda()
    out = torch.full((T, N, 1), NAN, device="cuda")
    ops.normalize_rewards(r[:T1], m[:T1 + 1], st, G, CLIP, EPS, out=out[:T1])
    ops.normalize_rewards(r, m, st, G, CLIP, EPS, first_row=T1, out=out)
    torch.cuda.synchronize()
    assert ru.same_bits(out, one_out) and rn.same_bits64(st, one_state)
    ref, want = rn.reward_norm_ref(rewards, masks, rn.fresh_state(N))
    rn.assert_state(f"two calls T{T} N{N}", st, want, N, T)
    rn.assert_outputs(f"two calls T{T} N{N}", out, ref)
    # first_row = T: nothing to do
    before = st.clone()
    ops.normalize_rewards(r, m, st, G, CLIP, EPS, first_row=T, out=out)
    torch.cuda.synchronize()
    assert torch.equal(st, before) and ru.same_bits(out, one_out)


@pytest.mark.parametrize("T,N", [(9, 3), (40, 257), (7, 1024)])
def test_two_launches_give_the_same_bits_state_included(T, N):
    rewards, masks = rn.inputs(T, N)
    _, st0 = rn.reward_norm_ref(rewards, masks, rn.fresh_state(N))          # (a state with history)
    a, b = _launch(rewards, masks, st0), _launch(rewards, masks, st0)
    assert ru.same_bits(a[0], b[0]) and rn.same_bits64(a[1], b[1]) and torch.isfinite(a[1]).all()


# ----------------------------------------------------------------------------- the one-launch form
@pytest.mark.parametrize("use_gae", [True, False], ids=["gae", "discounted"])
@pytest.mark.parametrize("T,N", [(5, 3), (18, 8), (64, 257), (3, 1024)])
def test_fused_form_has_the_bits_of_its_two_halves(T, N, use_gae):
    from wsmgmap import ops
    inp = ru.inputs(T, N, "random_20", seed=3)
    rewards, value_preds, masks, next_value = (t.cuda() for t in inp)
    _, st0 = rn.reward_norm_ref(inp[0], inp[2], rn.fresh_state(N))
    for first_row, update in ((0, True), (T // 2, True), (0, False)):
        # the halves: the normalising launch alone (rows below first_row from a full first call), then wsmg_gae_returns on its output
        st_a = torch.from_numpy(st0).cuda()
        base = ops.normalize_rewards(rewards, masks, st_a.clone(), G, CLIP, EPS)
        norm = ops.normalize_rewards(rewards, masks, st_a, G, CLIP, EPS, first_row=first_row, update=update, out=base.clone())
        vp_a = value_preds.clone()
        ret_a = torch.full((T + 1, N, 1), 7.0, device="cuda")
        _, adv_a, advn_a, stats_a = ops.gae_returns(norm, vp_a, masks, next_value, 0.99, 0.95, use_gae=use_gae, out=(ret_a, None, None, None))
        # the one launch
        st_b, vp_b = torch.from_numpy(st0).cuda(), value_preds.clone()
        ret_b = torch.full((T + 1, N, 1), 7.0, device="cuda")
        rout = base.clone()
        got = ops.normalized_gae_returns(rewards, vp_b, masks, next_value, 0.99, 0.95, st_b, G, CLIP, EPS, use_gae=use_gae,
                                         first_row=first_row, update=update, rewards_out=rout, out=(ret_b, None, None, None))
        torch.cuda.synchronize()
        tag = f"T{T} N{N} gae={use_gae} first_row={first_row} update={update}"
        assert got[4].data_ptr() == rout.data_ptr() and got[0].data_ptr() == ret_b.data_ptr()
        assert ru.same_bits(rout, norm) and rn.same_bits64(st_b, st_a), tag + ": rewards_out / state"
        assert update or rn.same_bits64(st_b, st0)
        assert ru.same_bits(ret_b, ret_a) and ru.same_bits(vp_b, vp_a) and ru.same_bits(got[1], adv_a), tag + ": returns / adv"
        assert ru.same_bits(got[2], advn_a) and rn.same_bits64(got[3], stats_a), tag + ": adv_norm / stats"
        ref = ru.gae_ref(rout.cpu(), inp[1], inp[2], inp[3], 0.99, 0.95, use_gae, returns=torch.full((T + 1, N, 1), 7.0))
        assert ru.same_bits(ret_b, ref["returns"]) and ru.same_bits(got[1], ref["adv"]) and ru.same_bits(vp_b, ref["value_preds"]), tag
        assert torch.equal(rewards.cpu(), inp[0])


# ----------------------------------------------------------------------------- the C ABI directly
def test_the_launchers_refuse_their_limits_with_nothing_written():
    from wsmgmap import _abi, ops
    L = _abi.lib()
    p = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())      # noqa: E731
    EINVAL = -1

    def refused(T, N, s0, Tb, Nb, drop=None):
        rewards, masks = torch.zeros(Tb, Nb, device="cuda"), torch.ones(Tb + 1, Nb, device="cuda")
        for which in ("norm", "fused"):
            state = torch.full((3 + Nb,), NAN, device="cuda", dtype=torch.float64)
            outs = [torch.full((Tb, Nb), NAN, device="cuda"), torch.full((Tb + 1, Nb), NAN, device="cuda"),      # rewards_norm, value_preds
                    torch.full((Nb,), NAN, device="cuda"), torch.full((Tb + 1, Nb), NAN, device="cuda"),          # next_value, returns
                    torch.full((Tb, Nb), NAN, device="cuda"), torch.full((Tb, Nb), NAN, device="cuda"),           # adv, adv_norm
                    torch.full((2,), NAN, device="cuda", dtype=torch.float64)]
            a = [rewards, masks, state] + outs
            if drop is not None:
                if which == "norm" and drop > 3:
                    continue
                a[drop] = None
            if which == "norm":
                rc = L.wsmg_reward_normalize(p(a[0]), p(a[1]), p(a[2]), 0.99, 10.0, 1e-8, T, N, s0, 1, p(a[3]), ops._stream())
            else:
                rc = L.wsmg_gae_returns_normalized(p(a[0]), p(a[1]), p(a[2]), 0.99, 10.0, 1e-8, s0, 1, p(a[3]), p(a[4]), p(a[5]), 0.99,
                                                   0.9405, 1, T, N, p(a[6]), p(a[7]), p(a[8]), p(a[9]), 1e-5, ops._stream())
            torch.cuda.synchronize()
            assert rc == EINVAL, (which, T, N, s0, drop)
            assert torch.isnan(state).all() and all(torch.isnan(o).all() for o in outs), (which, T, N, s0, drop)

    refused(0, 3, 0, 2, 3)
    refused(2, 0, 0, 2, 3)
    refused(2, 1025, 0, 2, 1025)
    refused(2, 3, 3, 2, 3)            # first_row > T
    refused(2, 3, -1, 2, 3)
    refused(16384, 1024, 0, 16384, 1024)          # T N = 2^24
    for drop in (0, 1, 2, 3, 4, 5, 6):            # rewards, masks, state, rewards_norm; value_preds, next_value, returns
        refused(2, 3, 0, 2, 3, drop=drop)


def test_ops_refuse_what_is_not_a_float32_contiguous_gpu_rollout_and_float64_state():
    from wsmgmap import ops
    E = ops._abi.WsmgError
    T, N = 4, 3
    rewards, value_preds, masks, next_value = (t.cuda() for t in ru.inputs(T, N))
    state = torch.from_numpy(rn.fresh_state(N)).cuda()
    norm = lambda r=rewards, m=masks, s=state, **k: ops.normalize_rewards(r, m, s, G, CLIP, EPS, **k)      # noqa: E731
    fused = lambda r=rewards, m=masks, s=state, **k: ops.normalized_gae_returns(r, value_preds.clone(), m, next_value, 0.99, 0.95, s,      # noqa: E731
                                                                                G, CLIP, EPS, **k)
    wide = torch.zeros(T, 2 * N, 1, device="cuda")
    for call in (norm, fused):
        before = state.clone()
        with pytest.raises(E, match="GPU"):
            call(r=rewards.cpu())
        with pytest.raises(E, match="GPU"):
            call(s=state.cpu())
        with pytest.raises(E, match="float32"):
            call(r=rewards.double())
        with pytest.raises(E, match="float32"):
            call(m=masks.bool())
        with pytest.raises(E, match="non-contiguous"):
            call(r=wide[:, ::2])
        with pytest.raises(E, match="masks"):
            call(m=masks[:T])
        with pytest.raises(E, match="state"):
            call(s=state.float())
        with pytest.raises(E, match="state"):
            call(s=torch.zeros(4 + N, device="cuda", dtype=torch.float64))
        with pytest.raises(E, match="first_row"):
            call(first_row=T + 1)
        with pytest.raises(E, match="at most 1024"):
            call(r=torch.zeros(1, 1025, device="cuda"), m=torch.ones(2, 1025, device="cuda"),
                 s=torch.zeros(1028, device="cuda", dtype=torch.float64))
        torch.cuda.synchronize()
        assert torch.equal(state, before)
    with pytest.raises(E, match="rewards_out"):
        norm(out=torch.zeros(T + 1, N, 1, device="cuda"))
    with pytest.raises(E, match="rewards_out"):
        fused(rewards_out=torch.zeros(T, N + 1, 1, device="cuda"))
    with pytest.raises(E, match="returns"):
        fused(out=(torch.zeros(T, N, 1, device="cuda"), None, None, None))
    # [T, N] operands, no `out`
    out = ops.normalize_rewards(rewards.reshape(T, N), masks.reshape(T + 1, N), state.clone(), G, CLIP, EPS)
    ref, _ = rn.reward_norm_ref(rewards, masks, rn.fresh_state(N))
    assert tuple(out.shape) == (T, N)
    rn.assert_outputs("flat", out, ref)


# ----------------------------------------------------------------------------- RewardNormalizer and RolloutStorage on the GPU
def test_normalizer_class_launches_on_the_gpu_and_falls_to_the_stock_arm_beyond_the_limits():
    from wsmgmap.rollout import RewardNormalizer
    T, N = 9, 8
    rewards, masks = rn.inputs(T, N)
    nz = RewardNormalizer(N, G).to("cuda")
    assert nz.state.is_cuda and nz.kernel_ok(rewards.cuda(), masks.cuda())
    out = nz.normalize(rewards.cuda(), masks.cuda())
    ref, want = rn.reward_norm_ref(rewards, masks, rn.fresh_state(N))
    rn.assert_state("class", nz.state, want, N, T)
    rn.assert_outputs("class", out, ref)
    nz.eval()
    before = nz.state.clone()
    frozen = nz.normalize(rewards.cuda(), masks.cuda())
    rn.assert_outputs("class eval", frozen, rn.reward_norm_ref(rewards, masks, before, update=False)[0])
    assert torch.equal(nz.state, before)
    # N = 1025 and float64 rewards: the float64 torch loop, on the GPU
    wide_r, wide_m = rn.inputs(2, 1025)
    wz = RewardNormalizer(1025, G).to("cuda")
    assert not wz.kernel_ok(wide_r.cuda(), wide_m.cuda())
    out = wz.normalize(wide_r.cuda(), wide_m.cuda())
    ref, want = rn.reward_norm_ref(wide_r, wide_m, rn.fresh_state(1025))
    rn.assert_state("stock N1025", wz.state, want, 1025, 2)
    rn.assert_outputs("stock N1025", out, ref)
    dz = RewardNormalizer(N, G).to("cuda")
    out = dz.normalize(rewards.cuda().double(), masks.cuda().double())
    assert out.dtype == torch.float64
    rn.assert_outputs("stock float64", out.float(), rn.reward_norm_ref(rewards, masks, rn.fresh_state(N))[0])


def _fill(st, N, steps, seed=0, first=0):
    g = torch.Generator(); g.manual_seed(4000 + N + seed)
    rows = [({"x": torch.randn(N, 3, generator=g)}, torch.randn(1, N, 4, generator=g), torch.randn(N, 2, generator=g),
             torch.randn(N, generator=g), torch.randn(N, 1, generator=g), torch.randn(N, 1, generator=g),
             (torch.rand(N, 1, generator=g) >= 0.2).float()) for _ in range(first + steps)]
    for row in rows[first:]:
        st.insert(*row)


def _pair(T, N):
    from wsmgmap.rollout import RewardNormalizer, RolloutStorage
    pair = []
    for fused in (True, False):
        st = RolloutStorage(T, N, {"x": ((3,), torch.float32)}, 2, 4, fused=fused, reward_normalizer=RewardNormalizer(N, G)).to("cuda")
        st.returns.fill_(7.0)
        pair.append(st)
    return pair


@pytest.mark.parametrize("use_gae", [True, False], ids=["gae", "discounted"])
@pytest.mark.parametrize("T,N,steps", [(5, 3, 5), (64, 8, 64), (20, 3, 18)], ids=["T5N3", "T64N8", "partial_18_then_20"])
def test_storage_fused_route_against_the_stock_route(T, N, steps, use_gae):
    """The one launch against the float64 torch loop + the float32 torch loop on the same GPU: the statistics and the normalised
    rewards inside the bars of the oracle on both routes, the fused returns the bits of the float32 loop on the fused rewards."""
    fused, stock = _pair(T, N)
    nv = torch.linspace(-1.0, 1.0, N, device="cuda").view(N, 1)
    for st in (fused, stock):
        _fill(st, N, steps)
        st.value_preds[steps:] = 123.0
    vp0 = fused.value_preds.cpu()

    def check(rows):
        raw = fused.rewards.clone()
        for st in (fused, stock):
            st.compute_returns(nv, use_gae, 0.99, 0.95)
        ref, want = rn.reward_norm_ref(fused.rewards[:rows].cpu(), fused.masks[:rows + 1].cpu(), rn.fresh_state(N))
        for name, st in (("fused", fused), ("stock", stock)):
            rn.assert_state(f"storage {name} T{T} N{N} rows {rows}", st.reward_normalizer.state, want, N, rows)
            rn.assert_outputs(f"storage {name}", st.rewards_normalized[:rows], ref)
        assert torch.equal(fused.rewards, raw) and torch.equal(stock.rewards, raw)
        loop = ru.gae_ref(fused.rewards_normalized[:rows].cpu(), vp0[:rows + 1], fused.masks[:rows + 1].cpu(), nv.cpu(), 0.99, 0.95, use_gae,
                          returns=torch.full((rows + 1, N, 1), 7.0))
        assert ru.same_bits(fused.returns[:rows + 1], loop["returns"]) and ru.same_bits(fused.get_advantages(False), loop["adv"])
        assert float((fused.returns[rows + 1:] - 7.0).abs().max() if rows < T else 0.0) == 0.0
        # a repeated compute_returns re-uses the rows: no bit moves, the state included
        snap = [t.clone() for t in (fused.returns, fused.value_preds, fused.rewards_normalized, fused.reward_normalizer.state,
                                    fused.get_advantages())]
        fused.compute_returns(nv, use_gae, 0.99, 0.95)
        torch.cuda.synchronize()
        for a, b in zip(snap, (fused.returns, fused.value_preds, fused.rewards_normalized, fused.reward_normalizer.state,
                               fused.get_advantages())):
            assert torch.equal(a, b)

    assert fused._fused_route() and not stock._fused_route()
    check(steps)
    if steps < T:          # filled to T: only the new rows are normalised, the carry continues: the one-shot result
        for st in (fused, stock):
            st.value_preds[steps] = vp0[steps].cuda()
            _fill(st, N, T - steps, first=steps)
        vp0 = fused.value_preds.cpu()
        check(T)


def test_storage_pair_with_a_normaliser_replays_in_a_captured_graph():
    """A first eager rollout (which allocates), after_update, a second rollout; compute_returns + get_advantages captured with
    torch.cuda.graph on one stream (the storage has no normalised row then: the capture records the one launch), then replayed
    twice with the rewards overwritten in place.  Each replay gives what an eager call from the same state gives and advances the
    statistics once: count grows by T N."""
    from wsmgmap.rollout import RewardNormalizer, RolloutStorage
    T, N = 5, 3
    nv = torch.linspace(-1.0, 1.0, N, device="cuda").view(N, 1)
    build = lambda: RolloutStorage(T, N, {"x": ((3,), torch.float32)}, 2, 4, reward_normalizer=RewardNormalizer(N, G)).to("cuda")      # noqa: E731
    st, eager = build(), build()
    for s in (st, eager):
        _fill(s, N, T)
        s.compute_returns(nv, True, 0.99, 0.95)
        s.get_advantages()
        s.after_update()
        _fill(s, N, T, seed=1)
    torch.cuda.synchronize()
    assert rn.same_bits64(st.reward_normalizer.state, eager.reward_normalizer.state)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        st.compute_returns(nv, True, 0.99, 0.95)
        adv = st.get_advantages()
    for k in (1, 2):
        g = torch.Generator(); g.manual_seed(k)
        new = torch.randn(T, N, 1, generator=g)
        before = st.reward_normalizer.state.clone()
        eager.reward_normalizer.load_state_dict(st.reward_normalizer.state_dict())
        eager.after_update()
        _fill(eager, N, T, seed=1)
        for s in (st, eager):
            s.rewards.copy_(new)
            s.returns.fill_(7.0)
        graph.replay()
        eager.compute_returns(nv, True, 0.99, 0.95)
        torch.cuda.synchronize()
        assert ru.same_bits(st.returns, eager.returns) and ru.same_bits(adv, eager.get_advantages())
        assert ru.same_bits(st.rewards_normalized, eager.rewards_normalized)
        assert rn.same_bits64(st.reward_normalizer.state, eager.reward_normalizer.state)
        assert abs(float(st.reward_normalizer.count) - (float(before[2]) + T * N)) <= 1e-9          # (T additions of N, each rounded)
        ref, want = rn.reward_norm_ref(new, st.masks.cpu(), before.cpu().numpy())
        rn.assert_state(f"graph replay {k}", st.reward_normalizer.state, want, N, T)
        rn.assert_outputs(f"graph replay {k}", st.rewards_normalized, ref)


def test_storage_without_a_normaliser_launches_what_it_launched():
    from wsmgmap.rollout import RolloutStorage
    T, N = 5, 3
    st = RolloutStorage(T, N, {"x": ((3,), torch.float32)}, 2, 4).to("cuda")
    _fill(st, N, T)
    nv = torch.linspace(-1.0, 1.0, N, device="cuda").view(N, 1)
    ref = ru.gae_ref(st.rewards.cpu(), st.value_preds.cpu(), st.masks.cpu(), nv.cpu(), 0.99, 0.95, True, returns=st.returns.cpu())
    st.compute_returns(nv, True, 0.99, 0.95)
    assert st.rewards_normalized is None and ru.same_bits(st.returns, ref["returns"])
    assert ru.same_bits(st.get_advantages(use_normalized_advantage=False), ref["adv"])
