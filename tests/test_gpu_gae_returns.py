"""GPU: the rollout's returns and advantages in one launch (csrc/wsmg_pg_rollout.hip) through `ops.gae_returns`, through the C ABI
directly and through `wsmgmap.rollout.RolloutStorage`, against the yardsticks of tests/rollout_util.py.

`returns`, `adv` and `value_preds[T]` are held to the BITS of the float32 torch loop on the CPU.  The normalised advantages and their
statistics are held to the float64 loop with the bar of tests/pg_util.py's rule, computed at run time from the same inputs:
bar = max(4 x the float32 torch loop's own error, 1e-6 x max |oracle|).  Each such comparison prints its figures before it asserts
(`-s` shows them; profiles/gae_returns.txt keeps a run's worst per quantity).

Measured on the MI355X (worst error / bar over the file): adv_norm 0.250, stats 0.116, storage adv_norm 0.141; policy step: loss and
critic.fc.weight gradient 0 (equal to the oracle-fed run's), fc_mean.weight gradient 0.098 (profiles/gae_returns.txt)."""
import ctypes

import pytest
import torch

import pg_util as pu
import rollout_util as ru

pytestmark = pytest.mark.gpu

NAN = float("nan")
WORST = {}


def _check(family, tag, got, ref64, stock32):
    e, _, bar = pu.check(tag, got, ref64, stock32)
    if bar > 0:
        WORST[family] = max(WORST.get(family, 0.0), e / bar)


def teardown_module(module):
    for k, v in sorted(WORST.items()):
        print(f"\nworst error / bar, {k}: {v:.3f}", end="")
    print()


def _launch(inp, gamma, tau, use_gae, eps=ru.EPS):
    """ops.gae_returns on copies of `inp` with NaN-filled outputs allocated one row too long.  -> (value_preds, returns, adv, adv_norm,
    stats) on the CPU after the guard rows were checked."""
    from wsmgmap import ops
    rewards, value_preds, masks, next_value = (t.cuda() for t in inp)
    T, N = rewards.shape[0], rewards.shape[1]
    big = [torch.full((rows + 1, N, 1), NAN, device="cuda") for rows in (T + 1, T, T)]
    stats = torch.full((3,), NAN, device="cuda", dtype=torch.float64)
    out = ops.gae_returns(rewards, value_preds, masks, next_value, gamma, tau, use_gae=use_gae, eps=eps,
                          out=(big[0][:T + 1], big[1][:T], big[2][:T], stats[:2]))
    torch.cuda.synchronize()
    assert out[0].data_ptr() == big[0].data_ptr() and out[3].data_ptr() == stats.data_ptr()
    for b, rows in zip(big, (T + 1, T, T)):
        assert torch.isnan(b[rows]).all(), "the guard row behind an output was written"
    assert torch.isnan(stats[2])
    assert torch.equal(rewards.cpu(), inp[0]) and torch.equal(masks.cpu(), inp[2]) and torch.equal(next_value.cpu(), inp[3])
    return value_preds.cpu(), big[0][:T + 1].cpu(), big[1][:T].cpu(), big[2][:T].cpu(), stats[:2].cpu()


# ----------------------------------------------------------------------------- bit identity
@pytest.mark.parametrize("T,N", ru.SHAPES)
def test_returns_advantages_and_the_written_value_row_are_the_float32_loops_bits(T, N):
    """Every T from 1 to two past the kernel's prefetch depth, 64 and 200; N on both sides of a wave (63 / 64 / 65) and of the
    workgroup (255 / 256 / 257: a thread's second column) up to the limit of 1024; both modes, the four (gamma, tau), the six mask
    patterns."""
    for kind in ru.MASKS:
        inp = ru.inputs(T, N, kind)
        for gamma, tau in ru.GAMMA_TAU:
            for use_gae in (True, False):
                ref = ru.gae_ref(*inp, gamma, tau, use_gae)
                value_preds, returns, adv, _, _ = _launch(inp, gamma, tau, use_gae)
                tag = f"T{T} N{N} {kind} gamma {gamma} tau {tau} gae {use_gae}"
                assert ru.same_bits(returns, ref["returns"]), tag + ": returns"        # (row T under GAE: still the NaN fill)
                assert ru.same_bits(adv, ref["adv"]), tag + ": adv"
                assert ru.same_bits(value_preds, ref["value_preds"]), tag + ": value_preds"


# ----------------------------------------------------------------------------- normalised advantages and statistics
@pytest.mark.parametrize("use_gae", [True, False], ids=["gae", "discounted"])
@pytest.mark.parametrize("T,N", [(2, 1), (5, 3), (17, 2), (18, 8), (64, 8), (200, 65), (33, 256), (64, 257), (3, 1024)])
def test_normalised_advantages_and_statistics_sit_within_the_bar_of_the_float64_loop(T, N, use_gae):
    for kind, (gamma, tau) in (("random_20", (0.99, 0.95)), ("ones", (1.0, 1.0)), ("one_env_masked", (0.9, 0.0))):
        inp = ru.inputs(T, N, kind, seed=3)
        ref = ru.gae_ref(*inp, gamma, tau, use_gae, dtype=torch.float64)
        stock = ru.gae_ref(*inp, gamma, tau, use_gae)
        _, _, _, adv_norm, stats = _launch(inp, gamma, tau, use_gae)
        tag = f"gae_returns T{T} N{N} {kind} gae={use_gae}"
        _check("adv_norm", tag + " adv_norm", adv_norm, ref["adv_norm"], stock["adv_norm"])
        # `stats` = {mean, std} is ONE compared quantity, as pg_util's rule takes a tensor: its scale is the std.  The mean on its own
        # is a cancelling sum (|mean| ~ 1e-3 of the entries at N = 1024): its distance from float64 is set by the float32 rounding of
        # adv's entries, which the bit contract fixes, and a float32 summation that lands nearer by luck cannot be outdone (measured
        # at T = 3, N = 1024: the exact mean of the float32 entries is off by 3.5e-9, torch's float32 mean by 4.1e-10).  Its use is
        # adv - mean, on the scale of the std.  The per-entry figures are printed for the record.
        print(f"{tag} mean: error {abs(float(stats[0] - ref['stats'][0])):.3e}  float32 torch {abs(float(stock['stats'][0] - ref['stats'][0])):.3e};"
              f"  std: error {abs(float(stats[1] - ref['stats'][1])):.3e}  float32 torch {abs(float(stock['stats'][1] - ref['stats'][1])):.3e}")
        _check("stats", tag + " stats", stats, ref["stats"], stock["stats"])


def test_a_larger_eps_reaches_the_kernel():
    inp = ru.inputs(5, 3, "ones")
    ref = ru.gae_ref(*inp, 0.99, 0.95, True, dtype=torch.float64, eps=0.5)
    stock = ru.gae_ref(*inp, 0.99, 0.95, True, eps=0.5)
    adv_norm = _launch(inp, 0.99, 0.95, True, eps=0.5)[3]
    _check("adv_norm", "gae_returns eps 0.5 adv_norm", adv_norm, ref["adv_norm"], stock["adv_norm"])


@pytest.mark.parametrize("use_gae", [True, False], ids=["gae", "discounted"])
def test_a_single_entry_has_no_standard_deviation(use_gae):
    """T N = 1: torch's unbiased std of one number is NaN, and so is the normalised advantage; the mean is the number."""
    inp = ru.inputs(1, 1, "ones")
    ref = ru.gae_ref(*inp, 0.99, 0.95, use_gae)
    _, returns, adv, adv_norm, stats = _launch(inp, 0.99, 0.95, use_gae)
    assert torch.isnan(ref["adv_norm"]).all() and torch.isnan(ref["stats"][1])
    assert torch.isnan(adv_norm).all() and torch.isnan(stats[1]) and float(stats[0]) == float(adv.double().reshape(()))
    assert ru.same_bits(adv, ref["adv"])


@pytest.mark.parametrize("use_gae", [True, False], ids=["gae", "discounted"])
def test_a_constant_advantage_normalises_to_exactly_zero(use_gae):
    T, N = 7, 65
    inp = (torch.zeros(T, N, 1), torch.zeros(T + 1, N, 1), torch.ones(T + 1, N, 1), torch.zeros(N, 1))
    _, returns, adv, adv_norm, stats = _launch(inp, 0.99, 0.95, use_gae)
    assert float(adv.abs().max()) == 0.0 and float(adv_norm.abs().max()) == 0.0 and not torch.isnan(adv_norm).any()
    assert float(stats[0]) == 0.0 and float(stats[1]) == 0.0


# ----------------------------------------------------------------------------- the C ABI directly
def _abi_call(rewards, value_preds, masks, next_value, gamma, gamma_tau, use_gae, T, N, returns, adv, adv_norm, stats, eps=ru.EPS):
    from wsmgmap import _abi, ops
    p = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())      # noqa: E731
    rc = _abi.lib().wsmg_gae_returns(p(rewards), p(value_preds), p(masks), p(next_value), gamma, gamma_tau, use_gae, T, N, p(returns),
                                     p(adv), p(adv_norm), p(stats), eps, ops._stream())
    torch.cuda.synchronize()
    return rc


def _abi_buffers(T, N, kind="random_20"):
    inp = [t.cuda() for t in ru.inputs(T, N, kind)]
    outs = [torch.full((T + 1, N), NAN, device="cuda"), torch.full((T, N), NAN, device="cuda"), torch.full((T, N), NAN, device="cuda"),
            torch.full((2,), NAN, device="cuda", dtype=torch.float64)]
    return inp, outs


@pytest.mark.parametrize("T,N", [(5, 3), (19, 257)])
def test_two_launches_give_the_same_bits_statistics_included(T, N):
    runs = []
    for _ in range(2):
        inp, outs = _abi_buffers(T, N)
        assert _abi_call(*inp, 0.99, pu.f32_scalar(0.99 * 0.95), 1, T, N, *outs) == 0
        runs.append([inp[1].cpu()] + [o.cpu() for o in outs])
    for a, b in zip(*runs):
        assert torch.equal(a.view(torch.int64 if a.dtype == torch.float64 else torch.int32),
                           b.view(torch.int64 if b.dtype == torch.float64 else torch.int32))
    assert torch.isfinite(runs[0][4]).all() and torch.isfinite(runs[0][3]).all()


@pytest.mark.parametrize("use_gae", [1, 0], ids=["gae", "discounted"])
@pytest.mark.parametrize("absent", [(1,), (2,), (3,), (1, 2), (1, 3), (2, 3), (1, 2, 3)], ids=lambda a: "no_" + "_".join(("", "adv", "norm", "stats")[i] for i in a))
def test_each_optional_output_may_be_null(absent, use_gae):
    """adv, adv_norm and stats are each left out alone and together: what is still asked for has the bits of the full call, and what
    was left out of the call is not written (its tensor keeps the NaN fill)."""
    T, N = 19, 65
    full_in, full = _abi_buffers(T, N)
    assert _abi_call(*full_in, 0.99, pu.f32_scalar(0.99 * 0.95), use_gae, T, N, *full) == 0
    inp, outs = _abi_buffers(T, N)
    args = [None if i in absent else o for i, o in enumerate(outs)]
    assert _abi_call(*inp, 0.99, pu.f32_scalar(0.99 * 0.95), use_gae, T, N, *args) == 0
    assert ru.same_bits(inp[1], full_in[1]) and ru.same_bits(outs[0], full[0])
    for i in (1, 2):
        if i in absent:
            assert torch.isnan(outs[i]).all()
        else:
            assert ru.same_bits(outs[i], full[i]) and torch.isfinite(outs[i]).all()
    assert torch.isnan(outs[3]).all() if 3 in absent else torch.equal(outs[3], full[3])


def test_the_launcher_refuses_its_limits_with_nothing_written():
    """Every WSMG_EINVAL: T < 1, N < 1, N > 1024, T N >= 2^24 (the buffers of that case have the size the arguments name), and each
    of the five required pointers NULL.  Afterwards the outputs are still NaN and value_preds[T] is untouched."""
    from wsmgmap import ops
    EINVAL = -1

    def refused(T, N, Tb, Nb, drop=None, use_gae=1):
        inp, outs = _abi_buffers(Tb, Nb, "ones")
        before = inp[1].clone()
        args = list(inp) + [0.99, 0.9405, use_gae, T, N] + outs
        if drop is not None:
            args[drop] = None
        assert _abi_call(*args) == EINVAL, (T, N, drop)
        assert all(torch.isnan(o).all() for o in outs) and torch.equal(inp[1], before)

    for use_gae in (1, 0):
        refused(0, 3, 2, 3, use_gae=use_gae)
        refused(-1, 3, 2, 3, use_gae=use_gae)
        refused(2, 0, 2, 3, use_gae=use_gae)
        refused(2, 1025, 2, 1025, use_gae=use_gae)
        for drop in (0, 1, 2, 3, 9):          # rewards, value_preds, masks, next_value, returns
            refused(2, 3, 2, 3, drop=drop, use_gae=use_gae)
    refused(16384, 1024, 16384, 1024)         # T N = 2^24
    assert ops.GAE_MAX_ENVS == 1024 and ops.GAE_MAX_ENTRIES == 1 << 24
    assert not ops.gae_returns_ok(torch.zeros(2, 1025, 1, device="cuda")) and ops.gae_returns_ok(torch.zeros(2, 1024, 1, device="cuda"))
    assert not ops.gae_returns_ok(torch.zeros(2, 3, 1)) and not ops.gae_returns_ok(torch.zeros(2, 3, 1, device="cuda"), T=0)


def test_ops_gae_returns_refuses_what_is_not_a_float32_contiguous_gpu_rollout():
    from wsmgmap import ops
    E = ops._abi.WsmgError
    T, N = 4, 3
    good = [t.cuda() for t in ru.inputs(T, N)]
    call = lambda *a, **k: ops.gae_returns(*a, 0.99, 0.95, **k)      # noqa: E731
    with pytest.raises(E, match="GPU"):
        call(good[0].cpu(), *good[1:])
    with pytest.raises(E, match="GPU"):
        call(*good[:3], good[3].cpu())
    with pytest.raises(E, match="float32"):
        call(good[0].double(), *good[1:])
    with pytest.raises(E, match="float32"):
        call(good[0], good[1], good[2].bool(), good[3])
    wide = torch.zeros(T + 1, 2 * N, 1, device="cuda")
    with pytest.raises(E, match="non-contiguous"):
        call(good[0], wide[:, ::2], good[2], good[3])
    with pytest.raises(E, match="value_preds"):
        call(good[0], good[1][:T], good[2], good[3])
    with pytest.raises(E, match="masks"):
        call(good[0], good[1], torch.ones(T + 1, N + 1, 1, device="cuda"), good[3])
    with pytest.raises(E, match="next_value"):
        call(*good[:3], torch.zeros(N + 1, 1, device="cuda"))
    with pytest.raises(E, match="rewards"):
        call(torch.zeros(T * N, device="cuda"), *good[1:])
    with pytest.raises(E, match="at most 1024"):
        call(torch.zeros(1, 1025, device="cuda"), torch.zeros(2, 1025, device="cuda"), torch.ones(2, 1025, device="cuda"),
             torch.zeros(1025, device="cuda"))
    outs = lambda: [torch.full((T + 1, N, 1), NAN, device="cuda"), torch.full((T, N, 1), NAN, device="cuda"),      # noqa: E731
                    torch.full((T, N, 1), NAN, device="cuda"), torch.full((2,), NAN, device="cuda", dtype=torch.float64)]
    for i, bad, match in ((0, torch.zeros(T, N, 1, device="cuda"), "returns"), (1, torch.zeros(T + 1, N, 1, device="cuda"), "adv"),
                          (2, torch.zeros(T, N, 1), "GPU"), (3, torch.zeros(2, device="cuda"), "stats")):
        o = outs()
        o[i] = bad
        vp = good[1].clone()
        with pytest.raises(E, match=match):
            call(good[0], vp, good[2], good[3], out=tuple(o))
        torch.cuda.synchronize()
        assert torch.equal(vp, good[1]) and all(torch.isnan(t).all() for j, t in enumerate(o) if j != i)
    # [T, N] operands and no `out`: the outputs come back in the operands' shapes
    flat = [t.reshape(t.shape[0], -1).contiguous() for t in good[:3]] + [good[3].reshape(-1)]
    returns, adv, adv_norm, stats = call(*flat)
    ref = ru.gae_ref(*ru.inputs(T, N), 0.99, 0.95, True)
    assert tuple(returns.shape) == (T + 1, N) and tuple(adv.shape) == tuple(adv_norm.shape) == (T, N) and stats.dtype == torch.float64
    assert ru.same_bits(returns[:T], ref["returns"][:T]) and ru.same_bits(adv, ref["adv"]) and float(returns[T].abs().max()) == 0.0


# ----------------------------------------------------------------------------- RolloutStorage on the GPU
def _fill(st, T, N, steps, seed=0):
    g = torch.Generator(); g.manual_seed(900 + 10 * T + N + seed)
    for _ in range(steps):
        st.insert({"x": torch.randn(N, 3, generator=g)}, torch.randn(1, N, 4, generator=g), torch.randn(N, 2, generator=g),
                  torch.randn(N, generator=g), torch.randn(N, 1, generator=g), torch.randn(N, 1, generator=g),
                  (torch.rand(N, 1, generator=g) >= 0.2).float())


def _pair(T, N, steps=None):
    from wsmgmap.rollout import RolloutStorage
    pair = []
    for fused in (True, False):
        st = RolloutStorage(T, N, {"x": ((3,), torch.float32)}, 2, 4, fused=fused).to("cuda")
        _fill(st, T, N, T if steps is None else steps)
        st.returns.fill_(7.0)
        st.value_preds[st.step:] = 123.0
        pair.append(st)
    return pair


@pytest.mark.parametrize("use_gae", [True, False], ids=["gae", "discounted"])
@pytest.mark.parametrize("T,N,steps", [(5, 3, 5), (64, 8, 64), (20, 3, 18)], ids=["T5N3", "T64N8", "partial_18_of_20"])
def test_storage_fused_route_against_the_torch_loop_route(T, N, steps, use_gae):
    """Two storages with the same inserted data, one launch against the torch loop on the same GPU: returns, value_preds and the raw
    advantages to the bit; the normalised advantages inside the bar of the float64 loop.  The partial rollout leaves the rows past
    `step` as they were."""
    fused, stock = _pair(T, N, steps)
    assert fused._fused_route() and not stock._fused_route()
    nv = torch.linspace(-1.0, 1.0, N, device="cuda").view(N, 1)
    cpu = [t[:rows].cpu() for t, rows in ((fused.rewards, steps), (fused.value_preds, steps + 1), (fused.masks, steps + 1))]
    for st in (fused, stock):
        st.compute_returns(nv, use_gae, 0.99, 0.95)
    raw, norm = fused.get_advantages(use_normalized_advantage=False), fused.get_advantages()
    assert tuple(raw.shape) == tuple(norm.shape) == (steps, N, 1)
    assert ru.same_bits(fused.returns, stock.returns) and ru.same_bits(fused.value_preds, stock.value_preds)
    assert ru.same_bits(raw, stock.get_advantages(use_normalized_advantage=False))
    assert float((fused.returns[steps + 1:] - 7.0).abs().max() if steps < T else 0.0) == 0.0
    assert float((fused.value_preds[steps + 1:] - 123.0).abs().max() if steps < T else 0.0) == 0.0
    ref = ru.gae_ref(*cpu, nv.cpu(), 0.99, 0.95, use_gae, dtype=torch.float64)
    _check("storage adv_norm", f"storage T{T} N{N} steps {steps} gae={use_gae} adv_norm", norm, ref["adv_norm"], stock.get_advantages())
    other = fused.get_advantages(eps=1e-2)          # not the launch's eps: from its statistics
    _check("storage adv_norm", f"storage T{T} N{N} steps {steps} gae={use_gae} adv_norm eps 1e-2", other,
           (ref["adv"] - ref["stats"][0]) / (ref["stats"][1] + pu.f32_scalar(1e-2)), stock.get_advantages(eps=1e-2))
    # an insert after the launch invalidates its advantages: the storage computes them from its tensors again
    if steps < T:
        _fill(fused, T, N, 1, seed=5)
        assert tuple(fused.get_advantages(use_normalized_advantage=False).shape) == (steps + 1, N, 1)


def test_storage_pair_replays_in_a_captured_graph():
    """compute_returns + get_advantages captured with torch.cuda.graph on one stream after a first eager call (which allocates the
    advantage buffers); the rewards are then overwritten in place and the graph replayed, twice: each replay gives what an eager
    fused call gives on the new data."""
    T, N = 5, 3
    st, _ = _pair(T, N)
    nv = torch.linspace(-1.0, 1.0, N, device="cuda").view(N, 1)
    st.compute_returns(nv, True, 0.99, 0.95)
    st.get_advantages()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        st.compute_returns(nv, True, 0.99, 0.95)
        adv = st.get_advantages()
    for k in (1, 2):
        g = torch.Generator(); g.manual_seed(k)
        new = torch.randn(T, N, 1, generator=g)
        st.rewards.copy_(new)
        st.returns.fill_(7.0)
        graph.replay()
        torch.cuda.synchronize()
        eager, _ = _pair(T, N)
        eager.rewards.copy_(new)
        eager.compute_returns(nv, True, 0.99, 0.95)
        assert ru.same_bits(st.returns, eager.returns) and ru.same_bits(adv, eager.get_advantages())
        ref = ru.gae_ref(new, eager.value_preds.cpu(), eager.masks.cpu(), nv.cpu(), 0.99, 0.95, True, returns=torch.full((T + 1, N, 1), 7.0))
        assert ru.same_bits(st.returns, ref["returns"])


# ----------------------------------------------------------------------------- one policy step end to end
class _Box:
    shape = (2,)


def _build_policy():
    """The T = 4 x N = 2 float32 policy of tests/test_gpu_pg_heads.py (its construction, copied)."""
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


def test_one_policy_step_from_act_to_the_ppo_gradient():
    """Four act() steps inserted into a fused and a `fused=False` storage (the observations kept are the update path's form of the
    same steps, as a trajectory cache keeps them), get_value, compute_returns(GAE), get_advantages, one minibatch, evaluate_actions,
    ops.ppo_loss, backward.  The loss and two head gradients of the fused storage's run are held to the run fed the float64 loop's
    normalised advantages, with the `fused=False` storage's run as the float32 composition of the 4 x rule."""
    from oracle import cases
    from util import T as tt
    from wsmgmap import ops
    from wsmgmap.common.aux_losses import AuxLosses
    from wsmgmap.rollout import RolloutStorage
    Tn, N = 4, 2
    AuxLosses.deactivate()
    AuxLosses.clear()
    pol = _build_policy()
    upd_np, _, _, _ = cases.update_inputs(Tn, N, tag="pg")
    upd = {k: tt(v).view(Tn, N, *v.shape[1:]) for k, v in upd_np.items()}
    shapes = {k: (tuple(v.shape[2:]), v.dtype) for k, v in upd.items()}
    stores = [RolloutStorage(Tn, N, shapes, 2, 512, 2, fused=f).to("cuda") for f in (True, False)]
    for st in stores:
        for k, v in upd.items():
            st.observations[k][0].copy_(v[0])
    h, prev = torch.zeros(2, N, 512, device="cuda"), torch.zeros(N, 2, device="cuda")
    g = torch.Generator(); g.manual_seed(4)
    torch.manual_seed(4)          # act() samples
    with torch.no_grad():
        for s in range(Tn):
            obs_np, masks = cases.act_inputs(s)
            obs, m = {k: tt(v).cuda() for k, v in obs_np.items()}, tt(masks).cuda()
            value, action, logp, h = pol.act(obs, h, prev, m)
            reward = torch.randn(N, 1, generator=g)
            for st in stores:
                st.insert({k: v[min(s + 1, Tn - 1)] for k, v in upd.items()}, h, action, logp, value, reward, torch.ones(N, 1))
            prev = action
        obs_np, _ = cases.act_inputs(Tn)
        next_value = pol.get_value({k: tt(v).cuda() for k, v in obs_np.items()}, h, prev, torch.ones(N, 1, device="cuda")).clone()
    assert tuple(next_value.shape) == (N, 1) and stores[0]._fused_route() and not stores[1]._fused_route()
    advs = []
    for st in stores:
        st.compute_returns(next_value, True, 0.99, 0.95)
        advs.append(st.get_advantages())
    assert ru.same_bits(stores[0].returns, stores[1].returns)
    cpu = [t.cpu() for t in (stores[1].rewards, stores[1].value_preds, stores[1].masks)]
    ref = ru.gae_ref(*cpu, next_value.cpu(), 0.99, 0.95, True, dtype=torch.float64)
    advs.append(ref["adv_norm"].float().cuda())

    def step(st, adv):
        pol.zero_grad(set_to_none=True)
        torch.manual_seed(21)
        batch = next(st.recurrent_generator(adv, 1))
        obs, hidden, actions, prev_actions, value_preds, returns, masks_b, old_logp, adv_b = batch
        assert tuple(hidden.shape) == (2, N, 512) and tuple(actions.shape) == (Tn * N, 2) and tuple(masks_b.shape) == (Tn * N, 1)
        value, logp, entropy, _ = pol.evaluate_actions(obs, hidden, prev_actions, masks_b, actions)
        loss = ops.ppo_loss(logp, old_logp, adv_b, value, value_preds, returns, entropy, pu.CLIP, pu.VALUE_COEF, pu.ENTROPY_COEF)[0]
        loss.backward()
        torch.cuda.synchronize()
        return [t.detach().cpu().clone() for t in (loss, pol.critic.fc.weight.grad, pol.action_distribution.fc_mean.weight.grad)]

    fused, stock, oracle = step(stores[0], advs[0]), step(stores[1], advs[1]), step(stores[1], advs[2])
    for name, a, b, c in zip(("loss", "critic.fc.weight grad", "fc_mean.weight grad"), fused, stock, oracle):
        assert torch.isfinite(c).all() and float(c.abs().max()) > 0.0, name
        _check("policy step " + name, "policy step " + name, a, c.double(), b)
    pol.zero_grad(set_to_none=True)
