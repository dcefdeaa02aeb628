"""`wsmgmap.ppo.PPO.update` on the GPU against tests/ppo_util.py's written-out loop: the T = 4 float32 policy of the policy-step test,
N = 4 environments in two minibatches (each the 4 x 2-row batch that test proves the net takes), ppo_epoch = 2.

The bar is measured, not assumed.  The written-out loop (stock minibatches, the same wsmgmap.optim.Adam, the same seeds) runs TWICE
from the same state.  If the two runs agree to the bit, `PPO.update` (whose only difference is the bit-exact one-launch gather and
its staging buffers) must agree with them to the bit; if they do not (an unordered sum somewhere in the net's backward), the bar per
compared tensor is 4 x the largest difference between those two runs, floored at 1e-6 of max |value| (tests/pg_util.py's rule).
Every figure is printed before it is asserted (profiles/ppo_update.txt keeps a run's)."""
import pytest
import torch

import ppo_util as pu

pytestmark = pytest.mark.gpu

HYPER = dict(clip_param=0.2, ppo_epoch=2, num_mini_batch=2, value_loss_coef=0.5, entropy_coef=0.01)
LR, EPS, MAX_NORM, SEED = 2.5e-4, 1e-5, 0.5, 77


def _state(pol):
    return {k: v.detach().clone() for k, v in pol.state_dict().items()}


def _params(pol):
    return {k: v.detach().clone() for k, v in pol.named_parameters()}


@pytest.fixture(scope="module")
def runs():
    """Everything the tests below compare, computed once: two runs of the written-out loop, one `PPO.update`."""
    from wsmgmap.common.aux_losses import AuxLosses
    from wsmgmap.optim import Adam
    from wsmgmap.ppo import PPO
    AuxLosses.deactivate()
    AuxLosses.clear()
    fused, stock = pu.policy_storages()
    pol_loop, pol_ppo = pu.build_policy(), pu.build_policy()
    state0 = _state(pol_loop)
    loops = []
    for _ in range(2):
        pol_loop.load_state_dict(state0, strict=True)
        opt = Adam([p for p in pol_loop.parameters() if p.requires_grad], lr=LR, eps=EPS, max_grad_norm=MAX_NORM)
        torch.manual_seed(SEED)
        stats = pu.written_out_update(pol_loop, stock, opt, max_grad_norm=MAX_NORM, **HYPER)
        loops.append((stats, _params(pol_loop), float(opt.grad_norm)))
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

    agent = Traced(pol_ppo, lr=LR, eps=EPS, max_grad_norm=MAX_NORM, **HYPER)
    prog = pol_ppo.prog = torch.full((3,), 5.0, device="cuda")
    torch.manual_seed(SEED)
    got = agent.update(fused)
    torch.cuda.synchronize()
    return dict(loops=loops, got=got, agent=agent, calls=calls, params=_params(pol_ppo), state0=state0, pol=pol_ppo, prog=prog,
                fused=fused, aux_entries=len(AuxLosses._entries))


def test_update_against_the_written_out_loop(runs):
    (s1, p1, n1), (s2, p2, n2) = runs["loops"]
    agent, got = runs["agent"], runs["got"]
    assert isinstance(got, tuple) and len(got) == 3 and all(type(v) is float for v in got)
    assert got == tuple(agent.last_stats[k] for k in pu.STATS[:3])
    exact = all(s1[k] == s2[k] for k in pu.STATS) and all(pu.same_bytes(p1[k], p2[k]) for k in p1) and n1 == n2
    print(f"written-out loop, two runs from one state: {'bit-identical' if exact else 'NOT bit-identical'}")
    worst = 0.0

    def check(name, g, a, b):
        nonlocal worst
        g, a, b = (torch.as_tensor(t).detach().double().cpu() for t in (g, a, b))
        spread = float((a - b).abs().max())
        bar = 0.0 if exact else max(4.0 * spread, 1e-6 * float(a.abs().max()))
        err = float((g - a).abs().max())
        ratio = err / bar if bar > 0.0 else (0.0 if err == 0.0 else float("inf"))
        worst = max(worst, ratio)
        if spread > 0.0 or err > 0.0:
            print(f"{name}: run-to-run {spread:.3e}  PPO.update - run 1 {err:.3e}  bar {bar:.3e}  ratio {ratio:.3f}")
        assert err <= bar, (name, err, bar)

    for k in pu.STATS:
        check(k, agent.last_stats[k], s1[k], s2[k])
    check("grad_norm", agent.last_stats["grad_norm"], n1, n2)
    for k in p1:
        if exact:
            assert pu.same_bytes(runs["params"][k], p1[k]), k
        check(k, runs["params"][k], p1[k], p2[k])
    print(f"worst ratio of an error to its bar: {worst:.3f} over {len(p1)} parameters and {len(pu.STATS) + 1} figures")
    for k in pu.STATS:
        print(f"  {k}: {agent.last_stats[k]!r} (loop {s1[k]!r})")


def test_the_trainable_parameters_moved_and_the_frozen_embedding_did_not(runs):
    moved = {k: float((v - runs["state0"][k]).abs().max()) for k, v in runs["params"].items()}
    assert moved["critic.fc.weight"] > 0.0 and moved["action_distribution.fc_mean.weight"] > 0.0
    assert moved["net.instruction_encoder.embedding_layer.weight"] == 0.0
    assert all(torch.isfinite(v).all() for v in runs["params"].values())


def test_hooks_aux_losses_prog_and_step_are_as_habitat_leaves_them(runs):
    steps = HYPER["ppo_epoch"] * HYPER["num_mini_batch"]
    assert runs["calls"] == list(pu.HOOKS) * steps
    assert runs["aux_entries"] == 0
    assert runs["pol"].prog is runs["prog"] and bool((runs["prog"] == 5.0).all())
    assert runs["fused"].step == 4                 # update() did not call after_update()
    assert runs["fused"]._staging is not None      # and ran on the storage's staging buffers
    assert set(runs["agent"].last_stats) == set(pu.STATS) | {"grad_norm"}


def test_a_tiny_max_grad_norm_reaches_the_device_guard(runs):
    """max_grad_norm = 1e-3 with lr = eps = 1: the reported norm (before clipping) exceeds it, and no parameter moves further than
    steps * lr * max_grad_norm / eps — per step |m_hat| / (sqrt(v_hat) + eps) <= |m_hat| / eps elementwise, and m_hat is a convex
    combination of clipped gradients, each of norm <= max_grad_norm.  (Unclipped, a gradient of norm g moves some parameter by
    about lr * g / (g + eps) per step.)  `p.grad` is what backward left: the guard does not rewrite it."""
    from wsmgmap.ppo import PPO
    pol = runs["pol"]
    pol.load_state_dict(runs["state0"], strict=True)
    hyper = dict(HYPER, ppo_epoch=1)
    agent = PPO(pol, lr=1.0, eps=1.0, max_grad_norm=1e-3, **hyper)
    torch.manual_seed(SEED)
    agent.update(runs["fused"])
    norm = agent.last_stats["grad_norm"]
    steps = hyper["ppo_epoch"] * hyper["num_mini_batch"]
    bound = steps * 1.0 * 1e-3 / 1.0
    moved = max(float((v.detach() - runs["state0"][k]).abs().max()) for k, v in pol.named_parameters())
    grads = [p.grad for p in pol.parameters() if p.grad is not None]
    left = float(torch.sqrt(sum((g.double() ** 2).sum() for g in grads)))
    print(f"reported gradient norm {norm:.4e} (max_grad_norm 1e-3), |p.grad| after the update {left:.4e}, largest parameter move "
          f"{moved:.4e} (bound {bound:.1e})")
    assert norm > 1e-3
    largest = max(float(v.abs().max()) for v in runs["state0"].values() if v.is_floating_point())
    assert 0.0 < moved <= bound * (1.0 + 1e-4) + steps * largest * 2.0 ** -23      # (+ the rounding of p - step in float32)
    assert abs(left - norm) <= 1e-3 * norm         # p.grad was not scaled by 1e-3 / norm
