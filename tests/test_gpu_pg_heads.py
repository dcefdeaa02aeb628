"""GPU: the policy-gradient heads and the PPO loss (csrc/wsmg_pg_heads.hip) through wsmgmap.ops and through
`BasePolicy.evaluate_actions` / `get_value`, against the float64 oracle of tests/pg_util.py.

Every compared quantity has the bar of pg_util's rule, computed at run time from the same inputs:
bar = max(4 x the error of the stock float32 torch composition against the oracle, 1e-6 x max |oracle|); a quantity the oracle has
at exactly zero must be exactly zero.  Each comparison prints its error, the float32 composition's and the bar before it asserts
(`-s` shows them; profiles/pg_heads.txt keeps a run's worst per quantity)."""
import itertools

import pytest
import torch

import pg_util as pu

pytestmark = pytest.mark.gpu

EVAL_KEYS = ("value", "logp", "entropy", "dx", "dwm", "dbm", "dlogstd", "dwc", "dbc")


# ----------------------------------------------------------------------------- eval_heads
def _modules(inp):
    x, wm, bm, ls, wc, bc, action = inp
    K, A = wm.shape[1], wm.shape[0]
    fc, cr = torch.nn.Linear(K, A), torch.nn.Linear(K, 1)
    with torch.no_grad():
        fc.weight.copy_(wm); fc.bias.copy_(bm); cr.weight.copy_(wc); cr.bias.copy_(bc)
    return fc.cuda(), cr.cuda(), ls.clone().cuda().requires_grad_(True)


def _eval_fused(inp, grads, x_cuda=None):
    """Forward + backward through ops.eval_heads.  -> the dict of pg_util.eval_heads_run, on the CPU."""
    from wsmgmap import ops
    fc, cr, ls = _modules(inp)
    x = inp[0].cuda().requires_grad_(True) if x_cuda is None else x_cuda
    value, logp, entropy = ops.eval_heads(x, fc, ls, cr, inp[6].cuda())
    assert tuple(value.shape) == (x.shape[0], 1) and tuple(logp.shape) == (x.shape[0],) and entropy.dim() == 0
    total = sum((o * g.cuda()).sum() for o, g in zip((value, logp, entropy), grads) if g is not None)
    total.backward()
    torch.cuda.synchronize()
    out = dict(value=value, logp=logp, entropy=entropy, dx=None if x_cuda is not None else x.grad, dwm=fc.weight.grad, dbm=fc.bias.grad,
               dlogstd=ls.grad, dwc=cr.weight.grad, dbc=cr.bias.grad)
    return {k: v.detach().cpu() for k, v in out.items() if v is not None}


def _compare_eval(tag, inp, grads):
    got = _eval_fused(inp, grads)
    ref = pu.eval_heads_run(inp, grads, torch.float64)
    stock = pu.eval_heads_run(inp, grads, torch.float32)
    assert tuple(got["dlogstd"].shape) == tuple(inp[3].shape)
    for k in EVAL_KEYS:
        pu.check(f"{tag} {k}", got[k].reshape(ref[k].shape), ref[k], stock[k])
    return got, ref


@pytest.mark.parametrize("B,K,A", list(itertools.product((1, 3, 4, 5, 33), (4, 256, 512), (1, 2, 4))))
def test_eval_heads_forward_and_six_gradients_match_the_oracle(B, K, A):
    """Wave (B % 4), workgroup (B = 4 / 5) and row-group (B = 33 > 32) edges, one to two feature passes per lane, every A."""
    inp, grads = pu.eval_inputs(B, K, A)
    _compare_eval(f"eval_heads B{B} K{K} A{A}", inp, grads)


@pytest.mark.parametrize("far", [False, True], ids=["one_sigma", "five_sigma"])
@pytest.mark.parametrize("B,K,A", [(5, 256, 2), (33, 512, 4)])
def test_eval_heads_at_logstd_of_plus_minus_three(B, K, A, far):
    inp, grads = pu.eval_inputs(B, K, A, logstd="pm3", far=far)
    _, ref = _compare_eval(f"eval_heads logstd+-3 far={far} B{B} A{A}", inp, grads)
    assert torch.isfinite(ref["logp"]).all() and torch.isfinite(ref["dlogstd"]).all()


@pytest.mark.parametrize("only", [0, 1, 2], ids=["value_only", "logp_only", "entropy_only"])
def test_eval_heads_with_one_output_gradient_present(only):
    """`set_materialize_grads(False)`: the two absent gradients reach the kernel as null.  What the oracle leaves at exactly zero is
    exactly zero (the bar of a zero quantity is zero)."""
    inp, grads = pu.eval_inputs(5, 256, 2)
    grads = tuple(g if i == only else None for i, g in enumerate(grads))
    got, ref = _compare_eval(f"eval_heads only={only}", inp, grads)
    zero = {0: ("dwm", "dbm", "dlogstd"), 1: ("dwc", "dbc"), 2: ("dx", "dwm", "dbm", "dwc", "dbc")}[only]
    for k in zero:
        assert float(ref[k].abs().max()) == 0.0 and float(got[k].abs().max()) == 0.0, k
    if only == 2:
        assert torch.equal(got["dlogstd"], torch.full_like(got["dlogstd"], 0.75))


def test_eval_heads_takes_a_non_contiguous_features_view():
    B, K, A = 5, 256, 2
    inp, grads = pu.eval_inputs(B, K, A)
    wide = torch.zeros(B, 2 * K)
    wide[:, ::2] = inp[0]
    wide = wide.cuda().requires_grad_(True)
    view = wide[:, ::2]
    assert not view.is_contiguous()
    got = _eval_fused(inp, grads, x_cuda=view)
    plain = _eval_fused(inp, grads)
    for k in got:
        assert torch.equal(got[k], plain[k]), k
    dwide = wide.grad.cpu()
    assert torch.equal(dwide[:, ::2], plain["dx"]) and float(dwide[:, 1::2].abs().max()) == 0.0


def test_eval_heads_refuses_features_off_a_16_byte_boundary():
    """The forward kernel reads features and weights four floats at a time: a contiguous view whose storage offset is 1 to 3
    floats is refused (WsmgError, nothing launched), an offset of 4 floats is taken and gives the aligned call's bits."""
    from wsmgmap import ops
    B, K, A = 3, 8, 2
    inp, grads = pu.eval_inputs(B, K, A)
    fc, cr, ls = _modules(inp)
    action = inp[6].cuda()
    flat = torch.zeros(B * K + 4, device="cuda")
    for off in (1, 2, 3):
        x = flat[off:off + B * K].view(B, K)
        x.copy_(inp[0])
        assert x.is_contiguous() and x.data_ptr() % 16 != 0
        with pytest.raises(ops._abi.WsmgError, match="16-byte"):
            ops.eval_heads(x, fc, ls, cr, action)
    x = flat[4:4 + B * K].view(B, K)
    x.copy_(inp[0])
    got, plain = ops.eval_heads(x, fc, ls, cr, action), ops.eval_heads(inp[0].cuda(), fc, ls, cr, action)
    assert all(torch.equal(a, b) for a, b in zip(got, plain))


def test_eval_heads_is_repeatable_to_the_bit():
    inp, grads = pu.eval_inputs(33, 512, 4)
    a, b = _eval_fused(inp, grads), _eval_fused(inp, grads)
    for k in EVAL_KEYS:
        assert torch.equal(a[k], b[k]), k


def test_eval_heads_agrees_with_act_heads_on_the_action_it_sampled():
    """The rollout's one-launch heads and the update's: value and log-probability of the SAME features, parameters and action.
    Both are float32 evaluations of the oracle's formula, each allowed its bar: they may differ by the two bars' sum."""
    from wsmgmap import ops
    B, K, A = 5, 512, 2
    inp, _ = pu.eval_inputs(B, K, A)
    fc, cr, ls = _modules(inp)
    pp = torch.nn.Linear(K, 1).cuda()
    g = torch.Generator(); g.manual_seed(5)
    noise = torch.randn(B, A, generator=g).cuda()
    x = inp[0].cuda()
    _, value_a, action, logp_a = ops.act_heads(x, pp, fc, ls.detach(), cr, noise)
    value, logp, _ = ops.eval_heads(x, fc, ls, cr, action)
    torch.cuda.synchronize()
    inp = inp[:6] + (action.cpu(),)
    ref = pu.eval_heads_run(inp, (None, None, torch.tensor(1.0)), torch.float64)
    stock = pu.eval_heads_run(inp, (None, None, torch.tensor(1.0)), torch.float32)
    for k, mine, theirs in (("value", value, value_a), ("logp", logp, logp_a)):
        pu.check(f"eval_heads vs act_heads {k} (against the oracle)", mine.reshape(ref[k].shape), ref[k], stock[k])
        bar, _ = pu.bar_of(ref[k], stock[k])
        d = float((mine.detach().reshape(-1) - theirs.reshape(-1)).abs().max())
        print(f"eval_heads vs act_heads {k}: differ by {d:.3e}, two bars {2 * bar:.3e}")
        assert d <= 2 * bar


# ----------------------------------------------------------------------------- ppo_loss
HYPER = (pu.CLIP, pu.VALUE_COEF, pu.ENTROPY_COEF)
PPO_KEYS = pu.PPO_OUT + ("dlogp", "dvalue", "dentropy")


def _ppo_fused(rows, entropy, clipped_value, mask, dloss=1.0):
    from wsmgmap import ops
    logp, old_logp, adv, value, old_value, ret = (t.cuda() for t in rows)
    logp.requires_grad_(True); value.requires_grad_(True)
    ent = entropy.cuda().requires_grad_(True)
    outs = ops.ppo_loss(logp, old_logp, adv, value, old_value, ret, ent, *HYPER, clipped_value=clipped_value,
                        mask=None if mask is None else mask.cuda())
    assert len(outs) == 5 and all(o.dim() == 0 for o in outs) and outs[0].requires_grad and not any(o.requires_grad for o in outs[1:])
    (outs[0] * dloss).backward()
    torch.cuda.synchronize()
    res = {k: v.detach().cpu() for k, v in zip(pu.PPO_OUT, outs)}
    res.update(dlogp=logp.grad.cpu(), dvalue=value.grad.cpu(), dentropy=ent.grad.cpu())
    return res


def _compare_ppo(tag, B, clipped_value, mask, dloss=1.0):
    rows, entropy = pu.ppo_inputs(B)
    got = _ppo_fused(rows, entropy, clipped_value, mask, dloss)
    ref = pu.ppo_loss_run(rows, entropy, HYPER, clipped_value, mask, torch.float64, dloss)
    stock = pu.ppo_loss_run(rows, entropy, HYPER, clipped_value, mask, torch.float32, dloss)
    for k in PPO_KEYS:
        pu.check(f"{tag} {k}", got[k].reshape(ref[k].shape), ref[k], stock[k])
    return got, ref


@pytest.mark.parametrize("clipped_value", [True, False], ids=["clipped_value", "plain_value"])
@pytest.mark.parametrize("B", [1, 2, 255, 256, 257, 2049])
def test_ppo_loss_outputs_and_gradients_match_the_oracle(B, clipped_value):
    """One thread's single row up to nine rows per thread; from 255 rows on every branch combination of pg_util.PPO_PATTERN is
    there (tests/test_pg_heads_cpu.py counts them): ratio below / inside / above the clip range and exactly 1, adv of either
    sign and zero, the value step inside and outside its clip with either squared error the larger."""
    got, ref = _compare_ppo(f"ppo_loss B{B} clipped={clipped_value}", B, clipped_value, None, dloss=1.5)
    assert torch.isfinite(ref["loss"]) and torch.isfinite(ref["dlogp"]).all()
    if B >= 255:
        assert 0.0 < float(got["clip_frac"]) < 1.0


@pytest.mark.parametrize("clipped_value", [True, False], ids=["clipped_value", "plain_value"])
@pytest.mark.parametrize("select", ["all", "one", "some", "none"])
def test_ppo_loss_under_a_mask(select, clipped_value):
    """The means run over the selected rows: all of them (the same numbers as without a mask), one row, a scattered half, and no
    row — loss 0 / 0 and the rows' gradients 0 * inf, NaN as in the oracle; d entropy stays -entropy_coef * d loss."""
    B = 257
    mask = torch.zeros(B, dtype=torch.bool)
    if select == "all":
        mask[:] = True
    elif select == "one":
        mask[200] = True
    elif select == "some":
        mask[torch.arange(B) % 3 != 1] = True
    got, ref = _compare_ppo(f"ppo_loss mask={select} clipped={clipped_value}", B, clipped_value, mask)
    if select == "all":
        rows, entropy = pu.ppo_inputs(B)
        plain = _ppo_fused(rows, entropy, clipped_value, None)
        for k in PPO_KEYS:
            assert torch.equal(got[k], plain[k]), k
    if select == "none":
        for k in pu.PPO_OUT:
            assert torch.isnan(got[k]) and torch.isnan(ref[k]), k
        # (`check` held the gradients' NaNs to the oracle's places: every row but those where a lost min / max branch or a clamp
        #  outside its interval puts an exact zero, as torch's backward nodes do)
        assert torch.isnan(got["dlogp"]).any() and not torch.isfinite(got["dlogp"][got["dlogp"] != 0]).any()
        assert torch.isfinite(got["dentropy"]).all()
    else:
        assert float(got["dlogp"][~mask].abs().max() if (~mask).any() else 0.0) == 0.0
        assert float(got["dvalue"][~mask].abs().max() if (~mask).any() else 0.0) == 0.0


def test_ppo_loss_accepts_a_uint8_mask_and_column_rows():
    from wsmgmap import ops
    B = 33
    rows, entropy = pu.ppo_inputs(B)
    mask = torch.arange(B) % 2 == 0
    a = _ppo_fused(rows, entropy, True, mask)
    b = _ppo_fused(rows, entropy, True, mask.to(torch.uint8))
    for k in PPO_KEYS:
        assert torch.equal(a[k], b[k]), k
    logp, old_logp, adv, value, old_value, ret = (t.cuda() for t in rows)
    value2 = value.view(B, 1).clone().requires_grad_(True)
    loss = ops.ppo_loss(logp, old_logp, adv, value2, old_value.view(B, 1), ret.view(B, 1), entropy.cuda()[0], *HYPER, mask=mask.cuda())[0]
    loss.backward()
    assert torch.equal(loss.cpu(), a["loss"]) and tuple(value2.grad.shape) == (B, 1) and torch.equal(value2.grad.view(-1).cpu(), a["dvalue"])
    with pytest.raises(ops._abi.WsmgError, match="one length"):
        ops.ppo_loss(logp, old_logp[:-1], adv, value, old_value, ret, entropy.cuda(), *HYPER)
    with pytest.raises(ops._abi.WsmgError, match="mask"):
        ops.ppo_loss(logp, old_logp, adv, value, old_value, ret, entropy.cuda(), *HYPER, mask=mask.cuda().float())


def test_ppo_loss_is_repeatable_to_the_bit():
    rows, entropy = pu.ppo_inputs(2049)
    mask = torch.arange(2049) % 5 != 0
    a, b = _ppo_fused(rows, entropy, True, mask), _ppo_fused(rows, entropy, True, mask)
    for k in PPO_KEYS:
        assert torch.equal(a[k], b[k]), k


def test_eval_heads_feeds_ppo_loss_end_to_end():
    """The two operators chained as an update chains them: gradients of the loss on all five head parameters and the features."""
    from wsmgmap import ops
    B, K, A = 33, 256, 2
    inp, _ = pu.eval_inputs(B, K, A)
    rows, _ = pu.ppo_inputs(B)
    _, _, adv, _, _, ret = rows
    fc, cr, ls = _modules(inp)
    x = inp[0].cuda().requires_grad_(True)
    value, logp, entropy = ops.eval_heads(x, fc, ls, cr, inp[6].cuda())
    old_logp, old_value = (logp.detach() - 0.05).clone(), (value.detach() + 0.05).clone()
    loss = ops.ppo_loss(logp, old_logp, adv.cuda(), value, old_value, ret.cuda().view(B, 1), entropy, *HYPER)[0]
    loss.backward()
    torch.cuda.synchronize()
    # the oracle, from the same float32 inputs
    leaves = [t.detach().double().requires_grad_(True) for t in inp[:6]]
    v64, lp64, e64, _ = pu.eval_heads_ref(*leaves, inp[6])
    l64 = pu.ppo_loss_ref(lp64, old_logp.cpu(), adv, v64, old_value.cpu(), ret, e64, *HYPER)[0]
    l64.backward()
    lv32 = [t.detach().clone().requires_grad_(True) for t in inp[:6]]
    v32, lp32, e32, _ = pu.eval_heads_ref(*lv32, inp[6], dtype=torch.float32)
    l32 = pu.ppo_loss_ref(lp32, old_logp.cpu(), adv, v32, old_value.cpu(), ret, e32, *HYPER, dtype=torch.float32)[0]
    l32.backward()
    pu.check("chain loss", loss, l64.detach(), l32.detach())
    for name, got, a, b in zip(("dx", "dwm", "dbm", "dlogstd", "dwc", "dbc"), (x, fc.weight, fc.bias, ls, cr.weight, cr.bias), leaves, lv32):
        pu.check(f"chain {name}", got.grad.reshape(a.grad.shape), a.grad, b.grad)


# ----------------------------------------------------------------------------- policy level
class _Box:
    shape = (2,)


def _build_policy():
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


@pytest.fixture(scope="module")
def policy():
    return _build_policy()


def _update_batch():
    from oracle import cases
    from util import T
    Tn, N = 2, 2
    obs_np, prev, masks, weights = cases.update_inputs(Tn, N, tag="pg")
    obs = {k: T(v).cuda() for k, v in obs_np.items()}
    action = torch.tensor([[0.3, -0.2], [-0.6, 0.1], [0.05, 0.4], [-0.15, -0.45]], device="cuda")
    return obs, T(prev).cuda(), T(masks).cuda(), T(weights).cuda(), action, N


def _h0(N):
    return torch.zeros(2, N, 512, device="cuda")


def test_evaluate_actions_on_the_policy(policy):
    """T = 2, N = 2, deterministic fill, float32 mode.  Value and log-probability against the oracle heads on the features of a plain
    `policy.net(...)` call from the same state; gradients reach logstd, the critic and the first map-encoder convolution;
    AuxLosses and `prog` are untouched; `forward()` gives the same bits before and after."""
    from wsmgmap.common.aux_losses import AuxLosses
    pol = policy
    obs, prev, masks, weights, action, N = _update_batch()
    AuxLosses.deactivate()
    AuxLosses.clear()
    AuxLosses.activate()          # (forward() reduces the registry: the monitors of the default configuration run)
    pred0, aux0 = pol(obs, _h0(N), prev, masks, weights)
    AuxLosses.deactivate()
    AuxLosses.clear()
    sentinel = pol.prog = torch.full((1,), 7.0)
    h_in = _h0(N)
    features, h_net, _ = pol.net(obs, _h0(N), prev, masks)
    pol.zero_grad(set_to_none=True)
    value, logp, entropy, h_out = pol.evaluate_actions(obs, h_in, prev, masks, action)
    assert tuple(value.shape) == (4, 1) and tuple(logp.shape) == (4,) and entropy.dim() == 0
    assert torch.equal(h_out, h_net)
    ad = pol.action_distribution
    inp = tuple(t.detach().cpu() for t in (features, ad.fc_mean.weight, ad.fc_mean.bias, ad.logstd._bias, pol.critic.fc.weight,
                                           pol.critic.fc.bias, action))
    one = (None, None, torch.tensor(1.0))
    ref, stock = pu.eval_heads_run(inp, one, torch.float64), pu.eval_heads_run(inp, one, torch.float32)
    for k, got in (("value", value), ("logp", logp), ("entropy", entropy)):
        pu.check(f"evaluate_actions {k}", got.reshape(ref[k].shape), ref[k], stock[k])
    (logp.sum() + value.sum() + entropy).backward()
    torch.cuda.synchronize()
    for p in (ad.logstd._bias, pol.critic.fc.weight, pol.net.map_encoder.cnn[0].weight):
        assert p.grad is not None and torch.isfinite(p.grad).all() and float(p.grad.abs().max()) > 0.0
    assert not AuxLosses._entries and not AuxLosses.is_active() and pol.prog is sentinel
    assert pol.net.skip_pred_map_nchw is False and pol.net._gt_semantic_map is None and pol.net._cls_tail_allowed is False
    AuxLosses.activate()
    pred1, aux1 = pol(obs, _h0(N), prev, masks, weights)
    AuxLosses.deactivate()
    AuxLosses.clear()
    assert torch.equal(pred0, pred1), "forward() changed its action mean across an evaluate_actions call"
    assert torch.is_tensor(aux0) and torch.equal(aux0.detach(), aux1.detach()), "forward() changed its auxiliary loss likewise"
    pol.zero_grad(set_to_none=True)


def test_get_value_is_the_value_act_returns():
    """Two policies from the same deterministic state (act() writes the map state): get_value on one, act() on the other, each
    with a hook on `net` that keeps the features it really saw.  Each value is held to the bar of pg_util's rule on its own
    features (float64 critic as the oracle, float32 F.linear as the stock composition), and the two values may differ by the two
    bars' sum (+ the oracles' own difference, which is zero when the two nets gave the same features)."""
    import torch.nn.functional as F
    from oracle import cases
    from util import T
    from wsmgmap.common.aux_losses import AuxLosses
    AuxLosses.deactivate()
    obs_np, masks = cases.act_inputs(0)
    vals, refs, bars = [], [], []
    for which in ("get_value", "act"):
        pol = _build_policy()
        pol.eval()
        seen = {}
        hk = pol.net.register_forward_hook(lambda m, i, o: seen.update(x=o[0].detach().clone()))
        obs = {k: T(v).cuda() for k, v in obs_np.items()}
        h, prev, m = torch.zeros(2, 2, 512, device="cuda"), torch.zeros(2, 2, device="cuda"), T(masks).cuda()
        with torch.no_grad():
            v = pol.get_value(obs, h, prev, m) if which == "get_value" else pol.act(obs, h, prev, m, deterministic=True)[0]
        hk.remove()
        assert tuple(v.shape) == (2, 1)
        x, w, b = seen["x"].cpu(), pol.critic.fc.weight.detach().cpu(), pol.critic.fc.bias.detach().cpu()
        ref, stock = F.linear(x.double(), w.double(), b.double()), F.linear(x, w, b)
        _, _, bar = pu.check(f"evaluate_actions get_value/{which} value", v, ref, stock)
        vals.append(v.cpu().double()); refs.append(ref); bars.append(bar)
    d = float((vals[0] - vals[1]).abs().max())
    allowed = bars[0] + bars[1] + float((refs[0] - refs[1]).abs().max())
    print(f"get_value vs act(): differ by {d:.3e}, allowed {allowed:.3e}")
    assert d <= allowed
