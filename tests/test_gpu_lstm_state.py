"""GPU: the LSTM state encoders (MODEL.STATE_ENCODER.rnn_type = "LSTM") on the persistent masked-LSTM kernels of
csrc/wsmg_rnn.hip — kernel against a float64 restatement of habitat's split-at-zeros encoder, the policy update against the
reference's g10 golden, rollout, graphs, the stock route, concurrent load and the timeout path."""
import numpy as np
import pytest
import torch

from wsmgmap.debug import sw as _SW

from lstm_state_util import build_lstm_policy, lstm_config, lstm_split_at_zeros, restart_masks, seeded
from oracle import detfill as df
from oracle import policy_ref
from util import NULL_GRAD, T, golden

pytestmark = pytest.mark.gpu


def close(name, got, ref, rtol, atol):
    got = got.detach().double().cpu()
    ref = ref.detach().double().cpu()
    err = (got - ref).abs()
    worst = float((err - (atol + rtol * ref.abs())).max())
    assert worst <= 0, f"{name}: max excess {worst:.3e} (max err {float(err.max()):.3e})"


# ----------------------------------------------------------------------------- kernel level
def _kernel_case(Tn, N, final):
    from wsmgmap.models.rnn_state_encoder import RNNStateEncoder
    In, Hd = 640, 512
    enc = RNNStateEncoder(In, Hd, rnn_type="LSTM")
    sd = {k: T(df.uniform(f"lstm_state.{k}", tuple(v.shape), 0.2 if "bias" in k else float(np.sqrt(12.0 / v.shape[1]))))
          for k, v in enc.rnn.state_dict().items()}
    enc.rnn.load_state_dict(sd)
    x = T(df.uniform(f"lstm_state.x.{Tn}.{N}", (Tn * N, In), 2.0))
    hc0 = T(df.uniform(f"lstm_state.hc0.{N}", (2, N, Hd), 1.0))
    masks = restart_masks(Tn, N)
    gy = T(df.uniform(f"lstm_state.gy.{Tn}.{N}", (Tn * N, Hd), 2.0))
    gh = T(df.uniform(f"lstm_state.gh.{N}", (2, N, Hd), 2.0))
    # float64 truth
    P = {k: v.double().requires_grad_(True) for k, v in sd.items()}
    xr, hr = x.double().requires_grad_(True), hc0.double().requires_grad_(True)
    yr, hTr, cTr = lstm_split_at_zeros(xr, hr[0:1], hr[1:2], masks.double(), P["weight_ih_l0"], P["weight_hh_l0"],
                                       P["bias_ih_l0"], P["bias_hh_l0"])
    lr = (yr * gy.double()).sum()
    if final:
        lr = lr + (hTr * gh[0:1].double()).sum() + (cTr * gh[1:2].double()).sum()
    lr.backward()
    enc = enc.cuda()

    def run():
        enc.zero_grad(set_to_none=True)
        xg, hg = x.cuda().requires_grad_(True), hc0.cuda().requires_grad_(True)
        y, hT = enc(xg, hg, masks.view(-1, 1).cuda())
        loss = (y * gy.cuda()).sum()
        if final:
            loss = loss + (hT * gh.cuda()).sum()
        loss.backward()
        return [y.detach(), hT.detach(), xg.grad, hg.grad] + [getattr(enc.rnn, k).grad.clone() for k in sd]

    out = run()
    torch.cuda.synchronize()
    _SW_check()
    y, hT, dx, dhc = out[:4]
    assert hT.shape == (2, N, Hd)
    # 1e-5 absolute: measured on MI355X, the float32 input-projection GEMM (up to 2e-5 off in gi at 640 inputs) dominates — the
    # kernel on an exactly rounded gi stays within 7e-7 of the truth at T = 200, the stock nn.LSTM route within 7e-6
    close("lstm.y", y, yr, 0, 1e-5)
    close("lstm.hT", hT[0:1], hTr, 0, 1e-5)
    close("lstm.cT", hT[1:2], cTr, 0, 1e-5)
    close("lstm.dx", dx, xr.grad, 1e-4, 1e-5 * float(xr.grad.abs().max()))
    close("lstm.dh0", dhc[0], hr.grad[0], 1e-4, 1e-5 * float(hr.grad[0].abs().max()) + 1e-9)
    close("lstm.dc0", dhc[1], hr.grad[1], 1e-4, 1e-5 * float(hr.grad[1].abs().max()) + 1e-9)
    for k, g in zip(sd, out[4:]):
        ref = P[k].grad
        close("lstm.d" + k, g, ref, 1e-4, 2e-5 * float(ref.abs().max()) + 1e-9)
    again = run()
    for a, b in zip(out, again):
        assert torch.equal(a, b), "two runs of the LSTM kernels differ"


def _SW_check():
    from wsmgmap import ops
    ops.check_rnn_status()


@pytest.mark.parametrize("N", [1, 3, 8, 11])
@pytest.mark.parametrize("Tn", [1, 4, 64, 200])
def test_lstm_state_kernel_vs_float64_split_at_zeros(Tn, N):
    """dh_T and dc_T given (the loss reads the final [h; c])."""
    _kernel_case(Tn, N, final=True)


@pytest.mark.parametrize("Tn,N", [(1, 3), (4, 11), (64, 8), (200, 3)])
def test_lstm_state_kernel_without_final_state_gradient(Tn, N):
    """dh_T and dc_T absent: the kernel's final-state gradient inputs are NULL."""
    _kernel_case(Tn, N, final=False)


def test_lstm_state_kernel_bit_identical_next_to_concurrent_mfma_load():
    """As test_rnn_handoff_under_concurrent_load for the GRU: the LSTM state kernels (built without packed-fp32 instructions,
    like the GRU pair) run beside a stream of bf16 MFMA convolutions, their exchange images poisoned with NaN before every launch:
    a stale or missed hand-off or a wrong partial sum shows as a NaN or a bitwise difference from the unloaded run."""
    from wsmgmap import ops
    torch.manual_seed(0)
    Tn, N, Hd = 64, 8, 512
    gi = torch.randn(Tn, N, 4 * Hd, device="cuda")
    whh = torch.randn(4 * Hd, Hd, device="cuda") * 0.04
    bhh = torch.randn(4 * Hd, device="cuda") * 0.1
    h0 = torch.randn(N, Hd, device="cuda")
    c0 = torch.randn(N, Hd, device="cuda")
    masks = torch.ones(Tn, N, device="cuda")
    masks[0] = 0
    masks[Tn // 2, 3] = 0
    gy = torch.randn(Tn, N, Hd, device="cuda")
    gc = torch.randn(N, Hd, device="cuda")

    def run():
        g = gi.clone().requires_grad_(True)
        hh, cc = h0.clone().requires_grad_(True), c0.clone().requires_grad_(True)
        y, c_t = ops.masked_lstm(g, whh, bhh, hh, cc, masks)
        ((y * gy).sum() + (c_t * gc).sum()).backward()
        return [y.detach(), c_t.detach(), g.grad, hh.grad, cc.grad]

    ref = run()
    torch.cuda.synchronize()
    assert all(bool(torch.isfinite(t).all()) for t in ref)
    old = _SW.rnn_poison
    _SW.rnn_poison = True
    try:
        side = torch.cuda.Stream()
        x = torch.randn(256, 24, 24, 256, device="cuda").to(torch.bfloat16)
        wconv = torch.randn(256, 256, 3, 3, device="cuda") * 0.02
        for i in range(20):
            with torch.cuda.stream(side):
                for _ in range(4):
                    ops.conv2d(x, wconv, None, 1, 1)
            out = run()
            for name, a, b in zip(["y", "c_T", "dgates", "dh0", "dc0"], ref, out):
                assert torch.equal(a, b), f"repeat {i}: {name} differs under load (max {float((a - b).abs().max()):.3e})"
        torch.cuda.synchronize()
    finally:
        _SW.rnn_poison = old
    ops.check_rnn_status()


def test_lstm_state_timeout_bits_reach_the_caller():
    """The status bits of the LSTM state kernels (32 forward, 64 backward) name them in the error the caller sees."""
    from wsmgmap import _abi, ops
    torch.cuda.synchronize()
    ops.check_rnn_status()
    names = dict((n, b) for b, n in _abi.STATUS_BITS)
    assert names["lstm_state_fwd"] == 32 and names["lstm_state_bwd"] == 64
    L = _abi.lib()
    pol = build_lstm_policy().cuda()
    for bit, name in ((32, "lstm_state_fwd"), (64, "lstm_state_bwd")):
        assert L.wsmg_rnn_debug_inject(bit) & bit
        with pytest.raises(_abi.WsmgError, match=name):
            pol.check_status()
        ops.check_rnn_status()             # cleared by the raising check
    assert L.wsmg_rnn_debug_inject(32 | 64) & 96
    assert _abi.status_names(_abi.take_rnn_status()) == ["lstm_state_fwd", "lstm_state_bwd"]
    ops.check_rnn_status()


# ----------------------------------------------------------------------------- policy level
def _update(pol, obs_np, prev, masks, weights, Tn, N):
    from wsmgmap.common.aux_losses import AuxLosses
    pol.train()
    pol.net.depth_encoder.eval()
    pol.net.rgb_encoder.eval()
    obs = {k: T(v).cuda() for k, v in obs_np.items()}
    w = T(weights).cuda()
    AuxLosses.activate()
    AuxLosses.clear()
    h0 = torch.zeros(pol.net.num_recurrent_layers, N, 512, device="cuda")
    pred, aux = pol(obs, h0, T(prev).cuda(), T(masks).cuda(), w)
    loss, _ = policy_ref.dagger_loss(pred, aux, obs["waypoint"], w.view(Tn, N))
    loss.backward()
    torch.cuda.synchronize()
    mon = {n: AuxLosses.get_loss(n).detach().cpu().numpy() for n in ["prediction_monitor", "contrastive_monitor", "progress_monitor"]}
    AuxLosses.deactivate()
    return pred, aux, loss, h0, mon


def _g10_inputs():
    from oracle import cases
    g = golden("g10_lstm_update.npz")
    obs_np, prev, masks, weights = cases.update_inputs(4, 2)
    assert float(g["masks"].reshape(4, 2)[2, 1]) == 0.0      # the golden's own mid-sequence restart
    return g, obs_np, prev, g["masks"], weights


def test_lstm_update_path_forward_backward_g10():
    g, obs_np, prev, masks, weights = _g10_inputs()
    pol = build_lstm_policy().cuda()
    assert pol.net.num_recurrent_layers == 4
    pred, aux, loss, h0, mon = _update(pol, obs_np, prev, masks, weights, 4, 2)
    err = np.abs(pred.detach().cpu().numpy() - g["pred"]).max()
    assert err <= 1e-4, f"action logits differ from the reference by {err:.3e} (bar 1e-4)"
    assert abs(float(aux) - float(g["aux_loss"])) <= 1e-4
    assert abs(float(loss) - float(g["loss"])) <= 1e-4
    for n, v in mon.items():
        np.testing.assert_allclose(v, g["aux." + n], atol=1e-4, rtol=1e-4)
    np.testing.assert_allclose(pol.prog.detach().cpu().numpy(), g["prog"], atol=1e-4, rtol=0)
    assert h0.shape == (4, 2, 512)
    np.testing.assert_allclose(h0.detach().cpu().numpy(), g["h_out"], atol=1e-4, rtol=0)   # [h1, c1, h2, c2], in place
    sd = pol.state_dict()
    for k in g.files:
        if k.startswith("bn."):
            np.testing.assert_allclose(sd[k[3:]].cpu().numpy(), g[k], atol=2e-5, rtol=2e-5, err_msg=k)
    named = dict(pol.named_parameters(remove_duplicate=False))
    bad = []
    for i, n in enumerate(g["grad.names"]):
        n = str(n)
        if n in NULL_GRAD:
            continue
        gr = named[n].grad
        assert gr is not None, f"no gradient for {n}"
        gr = gr.detach().cpu().numpy().reshape(-1)
        nr = float(np.sqrt((gr.astype(np.float64) ** 2).sum()))
        ref = float(g["grad.norm"][i])
        if abs(nr - ref) > 1e-2 * ref + 1e-7:
            bad.append((n, nr, ref))
    assert not bad, f"gradient norms off: {bad[:6]}"
    for n in g["grad.none"]:
        assert named[str(n)].grad is None, f"{n} must stay without gradient (unused in forward)"
    pol.check_status()


def test_lstm_stock_route_equals_kernel_route_on_the_update():
    """WSMG_RNN_STOCK (fallback level 2): nn.LSTM over the restart segments instead of the persistent kernels."""
    g, obs_np, prev, masks, weights = _g10_inputs()
    outs = []
    old = _SW.rnn_stock
    try:
        for stock in (False, True):
            _SW.rnn_stock = stock
            pol = build_lstm_policy().cuda()
            pred, aux, loss, h0, _ = _update(pol, obs_np, prev, masks, weights, 4, 2)
            grads = {n: p.grad.detach().clone() for n, p in pol.named_parameters() if p.grad is not None and "state_encoder.rnn" in n}
            outs.append((pred.detach(), float(loss), h0.detach().clone(), grads))
    finally:
        _SW.rnn_stock = old
    (pk, lk, hk, gk), (ps, ls, hs, gs) = outs
    close("pred", pk, ps, 0, 1e-5)
    assert abs(lk - ls) <= 1e-5
    close("h_out", hk, hs, 0, 1e-5)
    assert set(gk) == set(gs) and len(gk) == 8
    for n in gk:
        close("grad " + n, gk[n], gs[n], 1e-3, 1e-4 * float(gs[n].abs().max()) + 1e-9)


def _bench_like_update(mode, Tn, N, state):
    import bench
    from wsmgmap.common.aux_losses import AuxLosses
    from wsmgmap.models.policy import BasePolicy
    from lstm_state_util import Box
    pol = BasePolicy(None, Box(), lstm_config(num_proc=1, compute_dtype=mode))
    pol.load_state_dict(state)
    pol.net.instruction_encoder.embedding_layer.weight.requires_grad_(False)
    pol = pol.cuda()
    pol.train()
    pol.net.depth_encoder.eval()
    pol.net.rgb_encoder.eval()
    obs, prev, masks, weights = bench.synth_batch(Tn, N, "cuda", 77)
    AuxLosses.activate()
    AuxLosses.clear()
    h = torch.zeros(4, N, 512, device="cuda")
    pred, aux = pol(dict(obs), h, prev, masks, weights)
    loss = bench.dagger_loss(pred, aux, obs["waypoint"], weights)
    loss.backward()
    AuxLosses.deactivate()
    assert h.dtype == torch.float32       # the recurrences stay float32 in every mode
    grads = {n: p.grad.detach().float() for n, p in pol.named_parameters() if p.grad is not None}
    return pred.detach().float(), float(loss.detach()), grads


def test_lstm_bf16_mode_tracks_f32_mode():
    """The bars of test_bf16_mode_tracks_f32_mode, with LSTM state encoders."""
    from wsmgmap.models.policy import BasePolicy
    from lstm_state_util import Box
    torch.manual_seed(0)
    state = BasePolicy(None, Box(), lstm_config(num_proc=1)).state_dict()
    p32, l32, g32 = _bench_like_update("f32", 4, 8, state)
    p16, l16, g16 = _bench_like_update("bf16", 4, 8, state)
    assert float((p32 - p16).abs().max()) <= 1e-3
    assert abs(l32 - l16) <= 1e-3 * abs(l32)
    assert set(g32) == set(g16)
    a = torch.cat([g32[n].flatten() for n in g32])
    b = torch.cat([g16[n].flatten() for n in g32])
    assert float(torch.nn.functional.cosine_similarity(a, b, dim=0)) >= 0.999
    low = []
    for n in g32:
        if n in NULL_GRAD or g32[n].numel() < 4096 or float(g32[n].norm()) < 1e-6:
            continue
        cos = float(torch.nn.functional.cosine_similarity(g32[n].flatten(), g16[n].flatten(), dim=0))
        if cos < 0.9:
            low.append((n, round(cos, 4)))
    assert not low, f"bf16 gradients diverge from float32: {low[:8]}"


def _rollout_obs(B, gen, ins):
    return {"rgb": torch.randint(0, 256, (B, 224, 224, 3), device="cuda", generator=gen).float(),
            "depth": torch.rand(B, 256, 256, 1, device="cuda", generator=gen),
            "depth_features": torch.randn(B, 128, 4, 4, device="cuda", generator=gen),
            "instruction": ins.clone(),
            "gps": (torch.rand(B, 2, device="cuda", generator=gen) - 0.5) * 4,
            "compass": (torch.rand(B, 1, device="cuda", generator=gen) - 0.5) * 6.28}


def _instructions(B, gen):
    ins = torch.zeros(B, 200, dtype=torch.int64, device="cuda")
    for b in range(B):
        n = 20 + 17 * b
        ins[b, :n] = torch.randint(1, 2504, (n,), device="cuda", generator=gen)
    return ins


@pytest.mark.parametrize("B", [1, 8])
def test_lstm_act_equals_staged_net_forward(B):
    """act() (rollout: no autograd, one-launch input projections) against the staged update-path net.forward of a twin policy
    on the same steps: hidden states [h1, c1, h2, c2] and the deterministic action within 1e-5."""
    pa, pb = build_lstm_policy(num_proc=B).cuda().eval(), build_lstm_policy(num_proc=B).cuda().eval()
    gen = torch.Generator(device="cuda")
    gen.manual_seed(11)
    ins = _instructions(B, gen)
    ha = torch.randn(4, B, 512, device="cuda", generator=gen) * 0.5
    hb = ha.clone()
    prev = torch.zeros(B, 2, device="cuda")
    for k in range(3):
        obs = _rollout_obs(B, gen, ins)
        masks = torch.ones(B, 1, device="cuda")
        masks[k % B] = 0.0 if k != 2 else 1.0
        with torch.no_grad():
            va, aa, la, ha = pa.act(dict(obs), ha, prev, masks, deterministic=True)
        with torch.enable_grad():
            feats, hb, _ = pb.net(dict(obs), hb, prev, masks)
            ab = pb.action_distribution(feats).mode()
        close(f"step {k} h", ha, hb, 0, 1e-5)
        close(f"step {k} action", aa, ab, 0, 1e-5)
        prev = ab.detach().clone()
        hb = hb.detach()
    pa.check_status()


@pytest.mark.parametrize("mode", ["f32", "bf16"])
def test_lstm_graphed_act_matches_eager_act(mode):
    """GraphedAct with LSTM state encoders: the 4-layer hidden state is captured, replayed and written back like the GRU's
    (tolerances of test_graphed_act_matches_eager_act)."""
    from wsmgmap.graph import GraphedAct
    B = 2
    pa = build_lstm_policy(num_proc=B, compute_dtype=mode).cuda().eval()
    pb = build_lstm_policy(num_proc=B, compute_dtype=mode).cuda().eval()
    ga = GraphedAct(pa, eager_calls=1)
    gen = torch.Generator(device="cuda")
    gen.manual_seed(3)
    ins = _instructions(B, gen)
    ha, hb = torch.zeros(4, B, 512, device="cuda"), torch.zeros(4, B, 512, device="cuda")
    prev = torch.zeros(B, 2, device="cuda")
    tol = 2e-4 if mode == "f32" else 0.0
    for k in range(4):
        obs = _rollout_obs(B, gen, ins)
        masks = torch.ones(B, 1, device="cuda")
        if k in (0, 2):
            masks[k % B] = 0.0
        with torch.no_grad():
            vb, ab, lb, hb = pb.act(dict(obs), hb, prev, masks, deterministic=True)
        va, aa, la, hn = ga(obs, ha, prev, masks, deterministic=True)
        ha = hn.clone()
        for name, x, y in (("value", va, vb), ("action", aa, ab), ("logp", la, lb), ("h", ha, hb), ("prog", pa.prog, pb.prog)):
            assert float((x - y).abs().max()) <= tol * max(1.0, float(y.abs().max())), (k, name)
        prev = ab.clone()
    assert len(ga._graphs) == 1
    pa.check_status()


def test_lstm_graphed_update_matches_eager_updates():
    """GraphedUpdate with LSTM state encoders: four updates (two eager, then capture + replay) against an eager twin, with the
    bars of test_graphed_update_matches_eager_updates; the 4-layer hidden state is written back each time."""
    from wsmgmap import optim
    from wsmgmap.common.aux_losses import AuxLosses
    from wsmgmap.graph import GraphedUpdate
    g, obs_np, prev, masks, weights = _g10_inputs()
    obs = {k: T(v).cuda() for k, v in obs_np.items()}
    prev, masks, weights = T(prev).cuda(), T(masks).cuda(), T(weights).cuda()
    AuxLosses.activate()

    def loss_fn(pred, aux, o, w):
        return (pred ** 2).mean() + aux

    def train_mode(p):
        p.train()
        p.net.depth_encoder.eval()
        p.net.rgb_encoder.eval()
        return p
    pa, pb = train_mode(build_lstm_policy().cuda()), train_mode(build_lstm_policy().cuda())
    oa = optim.Adam(pa.parameters(), lr=1e-5, capturable=True)
    ob = optim.Adam(pb.parameters(), lr=1e-5)
    gu = GraphedUpdate(pa, oa, loss_fn, eager_calls=2)
    la, lb = [], []
    for k in range(4):
        h = torch.zeros(4, 2, 512, device="cuda")
        la.append(float(gu(obs, h, prev, masks, weights)))
        ob.zero_grad(set_to_none=True)
        AuxLosses.clear()
        hb = torch.zeros(4, 2, 512, device="cuda")
        pred, aux = pb(dict(obs), hb, prev, masks, weights)
        loss = loss_fn(pred, aux, obs, weights)
        loss.backward()
        ob.step()
        lb.append(float(loss))
        assert float(hb[1].abs().max()) > 0 and float((h - hb).abs().max()) <= 5e-3
    assert len(gu._graphs) == 1
    np.testing.assert_allclose(la, lb, rtol=3e-3, atol=1e-5)
    for (n, x), y in zip(pa.named_parameters(), pb.parameters()):
        assert float((x - y).abs().max()) <= 2e-4 * max(1.0, float(y.abs().max())), n
    AuxLosses.deactivate()
    pa.check_status()
