"""GPU: the KL early stop of `wsmgmap.ppo.PPO`, decided on the device — the gated PPO loss forward (csrc/wsmg_pg_heads.hip:
ppo_loss_fwd_gated_kernel), the guard's finalize behind an external gate (csrc/wsmg_optim.hip: grad_guard_finalize_gated_kernel,
`Adam.set_step_gate`) and `PPO(target_kl=..., kl_sync=...)` against tests/ppo_kl_util.py's written-out loop.

Every comparison is of bits.  The gated forward shares its row loop and reduction with the ungated one; the decision compares two
float32 values; a gated step with an open gate is the ungated step; and the written-out loop of tests/test_gpu_ppo.py repeats to the
bit on this policy (profiles/ppo_update.txt), so the trainer must meet it to the bit as well.  No tolerance is chosen anywhere.

The mid-update stop needs a minibatch k >= 1 whose approx_kl exceeds every earlier one; with SEED and LR below the written-out loop's
sequence on the MI355X is the one recorded in profiles/ppo_kl_gate.txt, and the test asserts that such a k exists."""
import copy
import ctypes

import numpy as np
import pytest
import torch

import ppo_kl_util as ku
import ppo_util as pu
from adam_util import _bits, _ptr, _stream

pytestmark = pytest.mark.gpu

INF = float("inf")


def _same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(_bits(a), _bits(b))


def _f32(t):
    """A 0-dim float32 device tensor as the numpy float32 it holds."""
    return t.detach().float().cpu().numpy().reshape(())[()]


# ----------------------------------------------------------------------------- 1. the gated forward against the ungated one
ROWS = [1, 63, 64, 65, 255, 256, 257, 1025]          # the wave and workgroup edges of "thread t adds rows t, t + 256, ..."
LOSS = dict(clip=0.2, value_coef=0.5, entropy_coef=0.01)


def _rows(B, seed=0):
    """Seeded inputs of one loss call: [logp, old_logp, adv, value, old_value, returns] and the one-element entropy, on the device."""
    g = torch.Generator(); g.manual_seed(8800 + 13 * B + seed)
    logp = -2.0 + 0.5 * torch.randn(B, generator=g)
    rows = [logp, logp + 0.3 * torch.randn(B, generator=g), torch.randn(B, generator=g), torch.randn(B, 1, generator=g),
            torch.randn(B, 1, generator=g), torch.randn(B, 1, generator=g)]
    return [t.cuda() for t in rows], torch.randn(1, generator=g).cuda()


def _call(rows, ent, clipped=True, mask=None, **gate):
    """One loss call and its backward on fresh leaves -> ([five outputs], [d logp, d value, d entropy])."""
    from wsmgmap import ops
    logp, old_logp, adv, value, old_value, ret = rows
    leaves = [t.clone().requires_grad_(True) for t in (logp, value, ent)]
    out = ops.ppo_loss(leaves[0], old_logp, adv, leaves[1], old_value, ret, leaves[2], LOSS["clip"], LOSS["value_coef"],
                       LOSS["entropy_coef"], clipped_value=clipped, mask=mask, **gate)
    out[0].backward()
    return [o.detach() for o in out], [t.grad for t in leaves]


def _masks(B):
    one = torch.zeros(B, dtype=torch.bool)
    one[B // 2] = True
    return {"all": None, "one": one.cuda(), "none": torch.zeros(B, dtype=torch.bool).cuda()}


@pytest.mark.parametrize("B", ROWS)
def test_gated_forward_is_the_ungated_one_to_the_bit(B):
    """All rows, one row, no row; both value-loss forms: the five outputs and the three gradients.  The record of each call is checked
    too: one call seen; with rows selected and an infinite limit one step taken and the figures in `sums`; with no row selected every
    figure is NaN, and even a limit of -inf (which any number exceeds) does not close the gate."""
    rows, ent = _rows(B)
    for name, mask in _masks(B).items():
        for clipped in (True, False):
            gate, sums = torch.zeros(8, device="cuda"), torch.zeros(5, device="cuda")
            want, dwant = _call(rows, ent, clipped, mask)
            got, dgot = _call(rows, ent, clipped, mask, gate=gate, sums=sums, kl_limit=-INF if name == "none" else INF)
            torch.cuda.synchronize()
            assert all(_same(g, w) for g, w in zip(got, want)), (name, clipped)
            assert all(_same(g, w) for g, w in zip(dgot, dwant)), (name, clipped)
            assert bool(torch.isnan(want[4])) == (name == "none")
            assert gate.tolist() == [0.0, 1.0, 1.0, 0.0, 0.0, 0.0, 0.0, 0.0], (name, clipped, gate.tolist())
            figures = torch.stack([want[2], want[1], ent[0], want[3], want[4]])      # the order the trainer sums them in
            if name == "none":
                assert torch.isnan(sums).tolist() == [True, True, False, True, True] and _same(sums[2], ent[0])
            else:
                assert _same(sums, figures), (name, clipped)                           # 0 + x == x


# ----------------------------------------------------------------------------- 2. the decision
def test_the_gate_closes_exactly_above_the_limit_and_stays_closed():
    B = 257
    calls = [_rows(B, seed) for seed in (1, 2, 3)]
    outs = [_call(r, e)[0] for r, e in calls]
    kl = _f32(outs[2][4])
    assert kl.dtype == np.float32 and np.isfinite(kl)
    below, above = np.nextafter(kl, np.float32(-np.inf)), np.nextafter(kl, np.float32(np.inf))
    assert below < kl < above

    # two calls under an infinite limit, then the third under a limit one float32 below its approx_kl: ordinal 2, that KL
    gate, sums = torch.zeros(8, device="cuda"), torch.zeros(5, device="cuda")
    running = np.zeros(5, np.float32)
    for i, (r, e) in enumerate(calls[:2]):
        _call(r, e, gate=gate, sums=sums, kl_limit=INF)
        o = outs[i]
        running = (running + np.array([_f32(o[2]), _f32(o[1]), _f32(e[0]), _f32(o[3]), _f32(o[4])], np.float32)).astype(np.float32)
        assert gate.tolist()[:3] == [0.0, float(i + 1), float(i + 1)]
        assert np.array_equal(sums.cpu().numpy().view(np.uint32), running.view(np.uint32)), i     # the float32 running sum, in call order
    got, _ = _call(*calls[2], gate=gate, sums=sums, kl_limit=float(below))
    assert all(_same(g, w) for g, w in zip(got, outs[2]))
    rec = gate.cpu().numpy()
    assert rec[:4].tolist() == [1.0, 2.0, 3.0, 2.0] and rec[4].view(np.uint32) == kl.view(np.uint32) and not rec[5:].any()
    assert np.array_equal(sums.cpu().numpy().view(np.uint32), running.view(np.uint32))       # the call that closes the gate adds nothing

    # once closed: a later call whose approx_kl is below its limit leaves it closed, and touches neither sums nor the step count
    gate_rec = _bits(gate).clone()
    _call(*calls[0], gate=gate, sums=sums, kl_limit=INF)
    rec = gate.cpu().numpy()
    assert rec[:4].tolist() == [1.0, 2.0, 4.0, 2.0] and rec[4].view(np.uint32) == kl.view(np.uint32)
    assert torch.equal(_bits(gate)[[0, 1, 3, 4, 5, 6, 7]], gate_rec[[0, 1, 3, 4, 5, 6, 7]])
    assert np.array_equal(sums.cpu().numpy().view(np.uint32), running.view(np.uint32))

    # a limit equal to the approx_kl, and one float32 above it: the gate stays open (the comparison is >)
    for limit in (kl, above):
        gate, sums = torch.zeros(8, device="cuda"), torch.zeros(5, device="cuda")
        _call(*calls[2], gate=gate, sums=sums, kl_limit=float(limit))
        assert gate.tolist() == [0.0, 1.0, 1.0, 0.0, 0.0, 0.0, 0.0, 0.0], float(limit)


def test_gated_entry_points_refuse_a_missing_or_misaligned_record():
    """WSMG_EINVAL before anything is enqueued: the record and the sums are as they were."""
    from wsmgmap import _abi, optim
    rows, ent = _rows(8)
    flat = [t.reshape(-1).contiguous() for t in rows]
    out, nsel = torch.zeros(5, device="cuda"), torch.zeros(1, device="cuda")
    store = torch.full((16,), 7.0, device="cuda")
    gate, sums = store[:8], store[8:13]

    def loss(gp, sp):
        _abi.call("wsmg_ppo_loss_fwd_gated", *[_ptr(t) for t in flat], None, _ptr(ent), 0.2, 0.5, 0.01, 1, 8, 1.0, _ptr(out), _ptr(nsel),
                  gp, sp, _stream())

    for gp, sp in ((None, _ptr(sums)), (_ptr(gate), None), (_ptr(gate, 2), _ptr(sums)), (_ptr(gate), _ptr(sums, 1))):
        with pytest.raises(_abi.WsmgError, match="WSMG_EINVAL"):
            loss(gp, sp)
    g = torch.ones(16, device="cuda")
    descs = (optim._AdamDesc * 1)()
    descs[0].grad, descs[0].n = g.data_ptr(), 16
    partials = torch.zeros(1, device="cuda", dtype=torch.float64)
    guard, hyper = torch.full((4,), 7.0, device="cuda"), torch.zeros(8, device="cuda")
    for gp in (None, _ptr(gate, 2)):
        with pytest.raises(_abi.WsmgError, match="WSMG_EINVAL"):
            _abi.call("wsmg_grad_norm_multi_gated", descs, 1, _ptr(partials), 1, 0.0, 1, gp, _ptr(guard), None, _stream())
        with pytest.raises(_abi.WsmgError, match="WSMG_EINVAL"):
            _abi.call("wsmg_grad_norm_multi_hyper_gated", descs, 1, _ptr(partials), 1, _ptr(hyper), 1, gp, _ptr(guard), None, _stream())
    torch.cuda.synchronize()
    assert bool((store == 7.0).all()) and bool((guard == 7.0).all()) and not bool(out.any())


# ----------------------------------------------------------------------------- 3. the gated Adam step
def _small(seed=0):
    """Three small tensors (a weight, BatchNorm's gamma and beta) and one BatchNorm's running statistics."""
    torch.manual_seed(seed)
    return torch.nn.Sequential(torch.nn.Linear(8, 8, bias=False), torch.nn.BatchNorm1d(8)).cuda().train()


def _small_update(m, opt, x):
    opt.zero_grad(set_to_none=True)
    m(x).pow(2).mean().backward()
    opt.step()


def _opt_state(m, opt):
    out = {**dict(m.named_parameters()), **dict(m.named_buffers()), "guard": opt._guard, "device_step": opt._guard_step}
    for name, p in m.named_parameters():
        for k in ("exp_avg", "exp_avg_sq"):
            out[f"{name}.{k}"] = opt.state[p][k]
    return out


def _record(tensors):
    return {k: _bits(v).clone() for k, v in tensors.items()}


@pytest.mark.parametrize("hyper", [False, True], ids=["by_value", "hyper_on_device"])
def test_a_set_gate_skips_the_step_and_an_open_one_changes_nothing(hyper):
    from wsmgmap import optim
    m = _small()
    twin = copy.deepcopy(m)
    kw = dict(lr=1e-2, max_grad_norm=0.5, skip_nonfinite=True, grad_report=True, hyper_on_device=hyper)
    opt, topt = optim.Adam(m.parameters(), guard_buffers=m, **kw), optim.Adam(twin.parameters(), guard_buffers=twin, **kw)
    gate = torch.zeros(8, device="cuda")
    opt.set_step_gate(gate)
    g = torch.Generator().manual_seed(11)
    xs = [torch.randn(4, 8, generator=g).cuda() for _ in range(3)]
    bad = xs[0].clone()
    bad[1, 2] = float("inf")

    def differing():
        a, b = _opt_state(m, opt), _opt_state(twin, topt)
        return [k for k in a if not _same(a[k], b[k])]

    # gate[0] = 0: the step taken through the ungated entry points, to the bit (guard record and device step count included)
    _small_update(m, opt, xs[0]); _small_update(twin, topt, xs[0])
    torch.cuda.synchronize()
    assert differing() == [] and float(opt._guard_step) == 1.0 and float(opt.grad_norm) > 0.0
    # gate[0] = 1: parameters, both moments, the device step count and the BatchNorm buffers stay; skipped advances; nothing is latched
    rec, norm = _record(_opt_state(m, opt)), float(opt.grad_norm)
    gate[0] = 1.0
    _small_update(m, opt, xs[1])
    torch.cuda.synchronize()
    now = _opt_state(m, opt)
    assert [k for k in now if k != "guard" and not torch.equal(_bits(now[k]), rec[k])] == []
    assert opt._guard.tolist()[2:] == [2.0, 1.0] and torch.equal(_bits(opt._guard)[:2], rec["guard"][:2])
    assert opt.skipped_steps == 1 and opt.last_skipped() is None and float(opt.grad_norm) == norm
    assert int(m[1].num_batches_tracked) == 1
    assert {float(st["step"]) for st in opt.state_dict()["state"].values()} == {1.0}       # attempted 2, skipped 1: the steps taken
    # gate[0] = 0 again: the next step is the twin's second, which never saw the gated batch
    gate[0] = 0.0
    _small_update(m, opt, xs[2]); _small_update(twin, topt, xs[2])
    torch.cuda.synchronize()
    a, b = _opt_state(m, opt), _opt_state(twin, topt)
    assert [k for k in a if k != "guard" and not _same(a[k], b[k])] == []
    assert opt._guard.tolist()[2:] == [0.0, 1.0] and torch.equal(_bits(opt._guard)[:2], _bits(topt._guard)[:2])
    assert float(opt._guard_step) == 2.0 and int(m[1].num_batches_tracked) == 2
    # a non-finite gradient behind an open gate still skips, and still latches
    rec = _record(_opt_state(m, opt))
    _small_update(m, opt, bad)
    torch.cuda.synchronize()
    now = _opt_state(m, opt)
    assert [k for k in now if k != "guard" and not torch.equal(_bits(now[k]), rec[k])] == []
    latched = opt.last_skipped()
    assert opt.skipped_steps == 2 and opt._guard.tolist()[2] == 1.0 and latched is not None
    assert latched.skipped == 2 and latched.attempt == 4 and latched.nonfinite_tensors >= 1
    # and a set gate over a non-finite gradient is a gate skip: the latch keeps the earlier report
    gate[0] = 1.0
    _small_update(m, opt, bad)
    torch.cuda.synchronize()
    assert opt.skipped_steps == 3 and opt._guard.tolist()[2] == 2.0 and opt.last_skipped().attempt == 4


# ----------------------------------------------------------------------------- 4. PPO.update on the T = 4 policy
HYPER = dict(clip_param=0.2, ppo_epoch=2, num_mini_batch=2, value_loss_coef=0.5, entropy_coef=0.01)
STEPS = HYPER["ppo_epoch"] * HYPER["num_mini_batch"]
LR, EPS, MAX_NORM, SEED = 2.5e-4, 1e-5, 0.5, 77
KL_KEYS = ("steps_taken", "stopped", "stop_ordinal", "stop_kl", "grad_norm")


def _moments(pol, opt):
    return {f"{n}.{k}": opt.state[p][k] for n, p in pol.named_parameters() if p in opt.state for k in ("exp_avg", "exp_avg_sq")}


@pytest.fixture(scope="module")
def runs():
    """Everything the tests below compare, computed once from one state: the written-out loop without a reachable limit (every
    minibatch's approx_kl) and with the mid-update limit; `PPO.update` with target_kl None, inf, negative, the mid-update target, and
    that target with kl_sync="epoch"."""
    from wsmgmap.common.aux_losses import AuxLosses
    from wsmgmap.optim import Adam
    from wsmgmap.ppo import PPO
    AuxLosses.deactivate()
    AuxLosses.clear()
    fused, stock = pu.policy_storages()
    pol_loop, pol = pu.build_policy(), pu.build_policy()
    state0 = {k: v.detach().clone() for k, v in pol.state_dict().items()}

    def loop(**limit):
        pol_loop.load_state_dict(state0, strict=True)
        opt = Adam([p for p in pol_loop.parameters() if p.requires_grad], lr=LR, eps=EPS, max_grad_norm=MAX_NORM)
        torch.manual_seed(SEED)
        out = ku.written_out_kl_update(pol_loop, stock, opt, max_grad_norm=MAX_NORM, **limit, **HYPER)
        return out, {k: v.detach().clone() for k, v in pol_loop.state_dict().items()}

    def ppo(target_kl, **more):
        pol.load_state_dict(state0, strict=True)
        agent = PPO(pol, lr=LR, eps=EPS, max_grad_norm=MAX_NORM, target_kl=target_kl, **HYPER, **more)
        torch.manual_seed(SEED)
        got = agent.update(fused)
        torch.cuda.synchronize()
        moments = {k: v.detach().clone() for k, v in _moments(pol, agent.optimizer).items()}
        steps = {float(st["step"]) for st in agent.optimizer.state_dict()["state"].values()}
        return dict(got=got, stats=dict(agent.last_stats), state={k: v.detach().clone() for k, v in pol.state_dict().items()},
                    moments=moments, steps=steps, skipped=agent.optimizer.skipped_steps, agent=agent)

    free, _ = loop(limit=np.float32(np.inf))
    print(f"written-out loop, lr {LR}, seed {SEED}: approx_kl per minibatch {free['kls']}")
    out = dict(free=free, state0=state0, none=ppo(None), inf=ppo(INF), negative=ppo(-1.0), mid=None)
    found = ku.first_running_maximum(free["kls"])
    if found is not None:
        k, below = found
        target = ku.target_between(np.float32(below), np.float32(free["kls"][k]))
        out.update(k=k, target=target, mid_loop=loop(target_kl=target), mid=ppo(target), mid_epoch=ppo(target, kl_sync="epoch"))
    return out


def _differing(a, b):
    assert a.keys() == b.keys()
    return [k for k in a if not pu.same_bytes(a[k], b[k])]


def test_an_infinite_target_kl_is_the_update_without_one(runs):
    none, inf = runs["none"], runs["inf"]
    assert _differing(inf["state"], none["state"]) == [] and _differing(inf["moments"], none["moments"]) == []
    assert {k: inf["stats"][k] for k in pu.STATS} == {k: none["stats"][k] for k in pu.STATS} and inf["got"] == none["got"]
    assert inf["stats"]["grad_norm"] == none["stats"]["grad_norm"] and inf["steps"] == none["steps"] == {float(STEPS)}
    assert set(none["stats"]) == set(pu.STATS) | {"grad_norm"}                # without a target_kl: today's keys
    assert [inf["stats"][k] for k in KL_KEYS[:4]] == [STEPS, False, None, None] and inf["skipped"] == 0
    assert any(not pu.same_bytes(v, runs["state0"][k]) for k, v in inf["state"].items())
    assert ku.same_stats(inf["stats"], runs["free"])                            # and both are the written-out loop's figures


def test_a_limit_below_the_first_approx_kl_takes_no_step(runs):
    neg, kls = runs["negative"], runs["free"]["kls"]
    assert kls[0] > -1.5                                                        # the premise: the first minibatch trips float32(-1.5)
    stats = neg["stats"]
    assert [stats[k] for k in KL_KEYS] == [0, True, 0, kls[0], None] and neg["skipped"] == STEPS and neg["steps"] == {0.0}
    assert all(stats[k] != stats[k] for k in pu.STATS) and all(v != v for v in neg["got"])
    assert _differing(neg["state"], runs["state0"]) == []                       # every parameter and BatchNorm buffer, to the bit
    assert len(neg["moments"]) > 2 * 96 and all(not bool(_bits(v).any()) for v in neg["moments"].values())
    assert len(ku.bn_buffers(neg["agent"].actor_critic)) == 3 * 63


def test_a_mid_update_stop_is_the_written_out_loops(runs):
    assert runs["mid"] is not None, f"no minibatch k >= 1 exceeds every earlier approx_kl: {runs['free']['kls']}"
    k, kls = runs["k"], runs["free"]["kls"]
    (want, want_state), mid = runs["mid_loop"], runs["mid"]
    print(f"stop at minibatch {k} of {STEPS}: target_kl {runs['target']!r}, limit {mid['agent'].kl_limit!r}, approx_kl {kls[k]!r} "
          f"(largest earlier {max(kls[:k])!r})")
    assert want["stopped"] and want["stop_ordinal"] == k and want["steps_taken"] == k and want["kls"][:k + 1] == kls[:k + 1]
    for key in KL_KEYS:
        assert mid["stats"][key] == want[key], key
    assert ku.same_stats(mid["stats"], want) and mid["stats"]["stop_kl"] == kls[k]
    assert _differing(mid["state"], want_state) == []
    assert mid["steps"] == {float(k)} and mid["skipped"] == STEPS - k
    assert _differing(mid["state"], runs["state0"]) != [] and _differing(mid["state"], runs["inf"]["state"]) != []


def test_kl_sync_epoch_leaves_the_same_bits(runs):
    assert runs["mid"] is not None, runs["free"]["kls"]
    mid, ep = runs["mid"], runs["mid_epoch"]
    assert _differing(ep["state"], mid["state"]) == [] and _differing(ep["moments"], mid["moments"]) == []
    assert ep["steps"] == mid["steps"] and ku.same_stats(ep["stats"], mid["stats"])
    assert [ep["stats"][k] for k in KL_KEYS] == [mid["stats"][k] for k in KL_KEYS]
    if runs["k"] < HYPER["num_mini_batch"]:        # stopped inside the first epoch: the second was not run
        assert ep["skipped"] == HYPER["num_mini_batch"] - runs["k"] < mid["skipped"]


# ----------------------------------------------------------------------------- 5. inside a HIP graph
class _Heads(torch.nn.Module):
    """A linear model small enough to read: column 0 of its output is the log-probability, column 1 the value."""

    def __init__(self):
        super().__init__()
        torch.manual_seed(21)
        self.fc = torch.nn.Linear(6, 2)
        self.entropy = torch.nn.Parameter(torch.tensor([0.7]))


def _gated_update(m, opt, inp, gate, sums, limit):
    from wsmgmap import ops
    x, old_logp, adv, old_value, ret = inp
    opt.zero_grad(set_to_none=True)
    y = m.fc(x)
    loss = ops.ppo_loss(y[:, 0], old_logp, adv, y[:, 1:2], old_value, ret, m.entropy, 0.2, 0.5, 0.01, gate=gate, sums=sums,
                        kl_limit=limit)[0]
    loss.backward()
    opt.step()


def test_gated_loss_backward_and_gated_step_replay_in_a_graph():
    """The gated loss forward, its backward through a small linear model and the gated guarded Adam step, captured once on one stream
    after one eager update, replayed four times; the third input's approx_kl is above the limit.  Parameters, moments, the step
    count, the guard record, the gate record and the sums equal the eager sequence's, to the bit."""
    from wsmgmap import optim
    B, LIMIT = 65, 1.0
    g = torch.Generator().manual_seed(31)

    def inputs(shift):      # approx_kl = mean(old_logp - logp) is about `shift`: logp is O(1)
        return [t.cuda() for t in (torch.randn(B, 6, generator=g), shift + 0.1 * torch.randn(B, generator=g), torch.randn(B, generator=g),
                                   torch.randn(B, 1, generator=g), torch.randn(B, 1, generator=g))]

    warm, seq = inputs(-10.0), [inputs(-10.0), inputs(-10.0), inputs(10.0), inputs(-10.0)]
    arms = []
    for _ in range(2):
        m = _Heads().cuda()
        opt = optim.Adam(m.parameters(), lr=1e-2, max_grad_norm=0.5, skip_nonfinite=True)
        buf = torch.zeros(13, device="cuda")
        opt.set_step_gate(buf[5:])
        arms.append((m, opt, buf))
    (m, opt, buf), (twin, topt, tbuf) = arms
    static = [t.clone() for t in warm]
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        _gated_update(m, opt, static, buf[5:], buf[:5], LIMIT)          # eager: the moments exist before the capture
        _gated_update(twin, topt, warm, tbuf[5:], tbuf[:5], LIMIT)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    assert buf.tolist()[5:8] == [0.0, 1.0, 1.0]
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        _gated_update(m, opt, static, buf[5:], buf[:5], LIMIT)
    opt.note_replayed_steps(-1)                                          # the capture ran the host bookkeeping once and executed nothing
    buf.zero_(); tbuf.zero_()                                            # the start of an update: the device fill
    for i, inp in enumerate(seq):
        for dst, src in zip(static, inp):
            dst.copy_(src)
        graph.replay()
        opt.note_replayed_steps(1)
        with torch.cuda.stream(side):
            _gated_update(twin, topt, inp, tbuf[5:], tbuf[:5], LIMIT)
        torch.cuda.synchronize()
        assert buf.tolist()[5:8] == [float(i >= 2), float(min(i + 1, 2)), float(i + 1)], (i, buf.tolist())
    assert buf.tolist()[8] == 2.0 and buf.tolist()[9] > LIMIT and _same(buf, tbuf)
    a = {**dict(m.named_parameters()), "guard": opt._guard, "device_step": opt._guard_step,
         **{f"{n}.{k}": opt.state[p][k] for n, p in m.named_parameters() for k in ("exp_avg", "exp_avg_sq")}}
    b = {**dict(twin.named_parameters()), "guard": topt._guard, "device_step": topt._guard_step,
         **{f"{n}.{k}": topt.state[p][k] for n, p in twin.named_parameters() for k in ("exp_avg", "exp_avg_sq")}}
    assert [k for k in a if not _same(a[k], b[k])] == []
    assert float(opt._guard_step) == 3.0 and opt.skipped_steps == 2 == topt.skipped_steps      # the warm-up and two taken; two gated
    assert opt.state_dict()["state"][0]["step"] == topt.state_dict()["state"][0]["step"] == 3.0
