"""GPU: the policy with MODEL.TEXT_ATTENTION = "fp8" — the instruction attention (mg_map_policy.py:229-232) through
ops.attention_fp8_shared in both directions (e4m3 storage, S = Q K^T on the fp8 matrix pipe, backward wsmg_attn_fp8_mfma_bwd) —
at T = 4 x N = 2, float32 mode, deterministic fill; and the default option, which leaves every path as it was."""
import pytest
import torch

from oracle import cases, policy_ref
from util import T, state_dict_values

pytestmark = pytest.mark.gpu

Tn, N = 4, 2
# Closeness of the "fp8" option to the "f32" option on the same state (e4m3 storage of q, K, V of the instruction attention is the only
# difference; its size at this depth was not known in advance, so the bars are twice the measured values):
#   measured on an MI355X: max |d logits| 1.343e-4 (max |logit| 0.813), loss 1.77806139 against 1.77806866: relative 4.090e-6
MEASURED_DLOGITS = 1.343e-4
MEASURED_DLOSS = 4.090e-6


class _Box:
    shape = (2,)


@pytest.fixture(autouse=True)
def _aux_losses_off():
    from wsmgmap.common.aux_losses import AuxLosses
    AuxLosses.deactivate()
    AuxLosses.clear()
    yield
    AuxLosses.deactivate()
    AuxLosses.clear()


def _policy(text_attention=None):
    from wsmgmap.config import default_model_config
    from wsmgmap.models.policy import BasePolicy
    kw = {} if text_attention is None else dict(text_attention=text_attention)
    pol = BasePolicy(None, _Box(), default_model_config(num_proc=2, **kw))
    pol.load_state_dict(state_dict_values(), strict=True)
    pol = pol.cuda()
    pol.train()
    pol.net.depth_encoder.eval()
    pol.net.rgb_encoder.eval()
    return pol


@pytest.fixture
def counted(monkeypatch):
    """Call counts of the two instruction-attention ops and of the pipelined recurrent block."""
    from wsmgmap import ops, recurrent
    n = dict(f32=0, fp8=0, block=0)

    def wrap(fn, key):
        def inner(*a, **k):
            n[key] += 1
            return fn(*a, **k)
        return inner
    monkeypatch.setattr(ops, "attention_shared", wrap(ops.attention_shared, "f32"))
    monkeypatch.setattr(ops, "attention_fp8_shared", wrap(ops.attention_fp8_shared, "fp8"))
    monkeypatch.setattr(recurrent, "recurrent_block", wrap(recurrent.recurrent_block, "block"))
    return n


def _update(pol):
    """One teacher-forcing update (forward, DAgger loss, backward) on the deterministic T = 4 x N = 2 case -> (logits, loss)."""
    from wsmgmap.common.aux_losses import AuxLosses
    obs_np, prev, masks, weights = cases.update_inputs(Tn, N)
    for p in pol.parameters():
        p.grad = None
    AuxLosses.activate()
    AuxLosses.clear()
    og = {k: T(v).cuda() for k, v in obs_np.items()}
    w = T(weights).cuda()
    pred, aux = pol(og, torch.zeros(2, N, 512, device="cuda"), T(prev).cuda(), T(masks).cuda(), w)
    loss, _ = policy_ref.dagger_loss(pred, aux, og["waypoint"], w.view(Tn, N))
    loss.backward()
    torch.cuda.synchronize()
    AuxLosses.deactivate()
    return pred.detach().clone(), float(loss.detach())


def test_fp8_option_update_runs_staged_and_reaches_the_text_parameters(counted):
    """One update with the option on: the instruction attention is ops.attention_fp8_shared (once), the update is staged — the
    pipelined block is not entered and the status says so —, and the query layer, the key layer and the instruction encoder's RNN
    weights (the three tensors the attention's dq, dK_u, dV_u reach) get finite, non-zero gradients.  Against the "f32" option on the
    same state: max |d logits| and the relative loss difference within twice the measured values (module docstring)."""
    from wsmgmap import ops
    from wsmgmap.fallback import RecurrentCoreFallback
    pol = _policy("fp8")
    assert pol.net.recurrent_chunks > 0            # the core is not switched off by hand: the option keeps the update out of it
    name = RecurrentCoreFallback(pol, verbose=False).report()["recurrent_core"]
    assert name.startswith("staged") and "fp8" in name, name
    pred8, loss8 = _update(pol)
    ops.check_rnn_status()
    assert counted == dict(f32=0, fp8=1, block=0), counted
    got = dict(pol.named_parameters())
    names = ["net.state_text_q_layer.weight", "net.state_text_k_layer.weight"] + [
        k for k in got if k.startswith("net.instruction_encoder.encoder_rnn.weight")]
    assert len(names) >= 4, names
    for k in names:
        g = got[k].grad
        assert g is not None and bool(torch.isfinite(g).all()) and float(g.abs().max()) > 0.0, k
    assert bool(torch.isfinite(pred8).all())

    ref = _policy("f32")
    ref.net.recurrent_chunks = 0                  # the same (staged) route, float32 attention
    pred32, loss32 = _update(ref)
    assert counted == dict(f32=1, fp8=1, block=0), counted
    dlogits = float((pred8 - pred32).abs().max())
    dloss = abs(loss8 - loss32) / abs(loss32)
    print(f"TEXT_ATTENTION fp8 vs f32 at T = {Tn} x N = {N}: max |d logits| {dlogits:.3e} (max |logit| {float(pred32.abs().max()):.3e}), "
          f"loss {loss8:.9g} vs {loss32:.9g}: relative {dloss:.3e}")
    assert dlogits <= 2 * MEASURED_DLOGITS, dlogits
    assert dloss <= 2 * MEASURED_DLOSS, dloss


def test_fp8_option_act_runs_and_default_still_selects_the_float32_op(counted):
    """`act` (B = 2, deterministic) with the option on goes through ops.attention_fp8_shared; the default config goes through
    ops.attention_shared, in a rollout step and in a staged update, and enters the pipelined block in a default update as before."""
    obs_np, masks = cases.act_inputs(0, B=2)
    obs = {k: T(v).cuda() for k, v in obs_np.items()}
    args = (torch.zeros(2, 2, 512, device="cuda"), torch.zeros(2, 2, device="cuda"), T(masks).cuda())
    pol = _policy("fp8").eval()
    with torch.no_grad():
        value, action, logp, h = pol.act(dict(obs), *args, deterministic=True)
    torch.cuda.synchronize()
    assert counted == dict(f32=0, fp8=1, block=0), counted
    assert tuple(action.shape) == (2, 2) and all(bool(torch.isfinite(t).all()) for t in (value, action, logp, h))

    dflt = _policy()
    assert dflt.net.text_attention == "f32"
    with torch.no_grad():
        v0, a0, _, _ = dflt.eval().act(dict(obs), *args, deterministic=True)
    assert counted == dict(f32=1, fp8=1, block=0), counted
    assert tuple(a0.shape) == tuple(action.shape) and tuple(v0.shape) == tuple(value.shape)
    dflt.train()
    dflt.net.depth_encoder.eval()
    dflt.net.rgb_encoder.eval()
    _update(dflt)                                            # default update: the pipelined block, as before
    assert counted == dict(f32=1, fp8=1, block=1), counted
    dflt.net.recurrent_chunks = 0
    _update(dflt)                                            # staged by hand: the float32 op
    assert counted == dict(f32=2, fp8=1, block=1), counted
