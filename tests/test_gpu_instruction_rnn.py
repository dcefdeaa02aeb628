"""GPU: the GRU and unidirectional instruction encoders on the persistent packed kernels of csrc/wsmg_rnn.hip
(wsmg_instr_rnn_fwd / _bwd) — kernel against float64 nn.GRU / nn.LSTM on a packed sequence, the route, the stock fall-back
for other shapes, the policy update against the reference's g11 / g12 goldens, rollout, graphs, status bits and concurrent load."""
import copy

import numpy as np
import pytest
import torch

from wsmgmap.debug import sw as _SW

from instr_rnn_util import ROWS, build_instr_policy, instr_config, instr_encoder
from oracle import cases, policy_ref
from oracle import detfill as df
from util import NULL_GRAD, T, golden

pytestmark = pytest.mark.gpu

LENS = [[1], [80, 37], [5, 1, 200, 64, 64, 199, 3, 120], [10] * 11]


def close(name, got, ref, rtol, atol):
    got = got.detach().double().cpu()
    ref = ref.detach().double().cpu()
    err = (got - ref).abs()
    worst = float((err - (atol + rtol * ref.abs())).max())
    assert worst <= 0, f"{name}: max err {float(err.max()):.3e} (ref max {float(ref.abs().max()):.3e}), exceeds by {worst:.3e}"


def _encoder_case(cell, bidir, hidden, lens, tag):
    enc = instr_encoder(cell, bidir, hidden, tag)
    ref = copy.deepcopy(enc).double()
    instr = T(df.tokens(f"instr.tok.{tag}.{len(lens)}", len(lens), lens).astype(np.float32))
    hr, mr = ref({"instruction": instr})                  # CPU: nn.GRU / nn.LSTM on a packed sequence, float64
    gy = T(df.uniform(f"instr.gy.{tag}.{len(lens)}", tuple(hr.shape), 2.0))
    (hr * gy.double()).sum().backward()
    enc = enc.cuda()
    hid, mask = enc({"instruction": instr.cuda()})
    assert hid.shape == hr.shape and torch.equal(mask.cpu(), mr)
    (hid * gy.cuda()).sum().backward()
    torch.cuda.synchronize()
    from wsmgmap import ops
    ops.check_rnn_status()
    return enc, ref, hid, hr


@pytest.mark.parametrize("lens", LENS)
@pytest.mark.parametrize("row", ["gru2", "lstm1", "gru1"])
def test_instruction_rnn_kernel_vs_float64_packed_module(row, lens):
    """Outputs, pad mask and the gradients of every encoder_rnn parameter and of the embedding, at the bars of
    test_bilstm_persistent_kernel; U = 11 runs as two launches (chunks of 8)."""
    cell, bidir, hidden, _ = ROWS[row]
    enc, ref, hid, hr = _encoder_case(cell, bidir, hidden, lens, row)
    close(f"{row}.out", hid, hr, 1e-5, 2e-6)
    for k, p in ref.encoder_rnn.named_parameters():
        close(f"{row}.d{k}", getattr(enc.encoder_rnn, k).grad, p.grad, 1e-4, 2e-5 * float(p.grad.abs().max()) + 1e-9)
    g = ref.embedding_layer.weight.grad
    close(f"{row}.demb", enc.embedding_layer.weight.grad, g, 1e-4, 2e-5 * float(g.abs().max()) + 1e-9)


@pytest.mark.parametrize("row", ["gru2", "lstm1", "gru1"])
def test_instruction_rnn_never_calls_the_stock_module(row, monkeypatch):
    """On the GPU with sw.rnn_stock off, the forward and backward never reach nn.GRU.forward / nn.LSTM.forward."""
    cell, bidir, hidden, _ = ROWS[row]
    assert not _SW.rnn_stock

    def boom(*a, **k):
        raise AssertionError("stock nn.GRU / nn.LSTM called")
    monkeypatch.setattr(torch.nn.GRU, "forward", boom)
    monkeypatch.setattr(torch.nn.LSTM, "forward", boom)
    enc = instr_encoder(cell, bidir, hidden, "route").cuda()
    instr = T(df.tokens("instr.route", 3, [80, 37, 5]).astype(np.float32)).cuda()
    hid, _ = enc({"instruction": instr})
    hid.sum().backward()
    with torch.no_grad():
        enc({"instruction": instr})
    torch.cuda.synchronize()
    assert enc.encoder_rnn.weight_hh_l0.grad is not None


def test_other_shapes_take_the_stock_route():
    """A bidirectional LSTM with hidden 64 has no kernel: the GPU forward returns the stock packed result (no WsmgError)."""
    enc = instr_encoder("LSTM", True, 64, "h64")
    assert enc.kernel_cell is None
    ref = copy.deepcopy(enc).double()
    instr = T(df.tokens("instr.h64", 3, [80, 37, 5]).astype(np.float32))
    hr, mr = ref({"instruction": instr})
    enc = enc.cuda()
    hid, mask = enc({"instruction": instr.cuda()})
    hid.sum().backward()
    torch.cuda.synchronize()
    assert hid.shape == hr.shape == (3, 128, 80) and torch.equal(mask.cpu(), mr)
    close("h64.out", hid, hr, 1e-5, 2e-6)


def test_instruction_rnn_abi_refuses_unsupported_shapes():
    from wsmgmap import _abi
    L = _abi.lib()
    for cell, hidden, dirs in ((0, 64, 2), (1, 128, 1), (1, 256, 2), (2, 128, 2)):
        assert L.wsmg_instr_rnn_workspace_bytes(cell, hidden, dirs, 10) == 0
        assert L.wsmg_instr_rnn_fwd(cell, None, None, None, None, 1, 10, hidden, dirs, None, None, None, None, None) == -1
    x = torch.zeros(1024, device="cuda")
    p = x.data_ptr()
    assert L.wsmg_instr_rnn_fwd(1, p, p, p, p, 9, 10, 128, 2, p, p, None, p, None) == -1       # U > 8
    assert L.wsmg_instr_rnn_bwd(1, p, p, p, p, p, None, 2, 10, 256, 1, p, None, p, None) == -1  # GRU without dgh


# ----------------------------------------------------------------------------- status bits
def test_instruction_rnn_timeout_bits_reach_the_caller():
    from wsmgmap import _abi, ops
    torch.cuda.synchronize()
    ops.check_rnn_status()
    names = dict((n, b) for b, n in _abi.STATUS_BITS)
    assert names["instr_rnn_fwd"] == 128 and names["instr_rnn_bwd"] == 256
    L = _abi.lib()
    pol = build_instr_policy("gru2").cuda()
    for bit, name in ((128, "instr_rnn_fwd"), (256, "instr_rnn_bwd")):
        assert L.wsmg_rnn_debug_inject(bit) & bit
        with pytest.raises(_abi.WsmgError, match=name):
            pol.check_status()
        ops.check_rnn_status()
    assert L.wsmg_rnn_debug_inject(128 | 256) & 384
    assert _abi.status_names(_abi.take_rnn_status()) == ["instr_rnn_fwd", "instr_rnn_bwd"]
    ops.check_rnn_status()


def test_instruction_rnn_bit_identical_next_to_concurrent_mfma_load():
    """As test_rnn_handoff_under_concurrent_load: the four kernel pairs beside a stream of bf16 MFMA convolutions, their
    exchange images poisoned with NaN before every launch, must repeat the unloaded run bit for bit."""
    from wsmgmap import ops
    torch.manual_seed(0)
    U, L = 8, 60
    lens = torch.tensor([60, 37, 1, 44, 60, 12, 55, 59], device="cuda", dtype=torch.int32)
    cases_ = []
    for cell, D, H in (("LSTM", 2, 128), ("GRU", 2, 128), ("LSTM", 1, 256), ("GRU", 1, 256)):
        G = 3 if cell == "GRU" else 4
        cases_.append((cell, torch.randn(U, L, D, G * H, device="cuda"), torch.randn(D, G * H, H, device="cuda") * (1.0 / H ** 0.5),
                       torch.randn(D, G * H, device="cuda") * 0.1, torch.randn(U, L, D * H, device="cuda")))

    def run():
        res = []
        for cell, gi, w, b, gy in cases_:
            g, ww, bb = gi.clone().requires_grad_(True), w.clone().requires_grad_(True), b.clone().requires_grad_(True)
            y = ops.instr_rnn(g, ww, bb, lens, cell)
            (y * gy).sum().backward()
            res += [y.detach(), g.grad, ww.grad, bb.grad]
        return res

    ref = run()
    torch.cuda.synchronize()
    assert all(bool(torch.isfinite(t).all()) for t in ref)
    old = _SW.rnn_poison
    _SW.rnn_poison = True
    try:
        side = torch.cuda.Stream()
        x = torch.randn(256, 24, 24, 256, device="cuda").to(torch.bfloat16)
        wconv = torch.randn(256, 256, 3, 3, device="cuda") * 0.02
        for i in range(10):
            with torch.cuda.stream(side):
                for _ in range(4):
                    ops.conv2d(x, wconv, None, 1, 1)
            out = run()
            for j, (a, b) in enumerate(zip(ref, out)):
                assert torch.equal(a, b), f"repeat {i}: tensor {j} differs under load (max {float((a - b).abs().max()):.3e})"
        torch.cuda.synchronize()
    finally:
        _SW.rnn_poison = old
    ops.check_rnn_status()


# ----------------------------------------------------------------------------- policy level
def _update(pol, Tn=4, N=2):
    from wsmgmap.common.aux_losses import AuxLosses
    obs_np, prev, masks, weights = cases.update_inputs(Tn, N)
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


@pytest.mark.parametrize("row", ["gru2", "lstm1"])
def test_instruction_rnn_update_path_against_reference_golden(row):
    """One teacher-forcing update against the unmodified reference's g11 (GRU, bidirectional) / g12 (LSTM, unidirectional),
    with the bars of test_lstm_update_path_forward_backward_g10."""
    g = golden(ROWS[row][3])
    pol = build_instr_policy(row).cuda()
    pred, aux, loss, h0, mon = _update(pol)
    err = np.abs(pred.detach().cpu().numpy() - g["pred"]).max()
    assert err <= 1e-4, f"action logits differ from the reference by {err:.3e} (bar 1e-4)"
    assert abs(float(aux) - float(g["aux_loss"])) <= 1e-4
    assert abs(float(loss) - float(g["loss"])) <= 1e-4
    for n, v in mon.items():
        np.testing.assert_allclose(v, g["aux." + n], atol=1e-4, rtol=1e-4)
    np.testing.assert_allclose(pol.net.att_map_t_m.detach().cpu().numpy(), g["att_map_t_m"], atol=2e-6, rtol=2e-3)
    np.testing.assert_allclose(pol.prog.detach().cpu().numpy(), g["prog"], atol=1e-4, rtol=0)
    np.testing.assert_allclose(h0.detach().cpu().numpy(), g["h_out"], atol=1e-4, rtol=0)
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
        if "encoder_rnn" in n:
            s = gr[:: max(1, gr.size // 8)][:8]
            np.testing.assert_allclose(s, g["grad.sample"][i][: s.size], rtol=1e-2, atol=1e-3 * max(ref, 1e-6), err_msg=n)
    assert not bad, f"gradient norms off: {bad[:6]}"
    for n in g["grad.none"]:
        assert named[str(n)].grad is None, f"{n} must stay without gradient (unused in forward)"
    pol.check_status()


def _bench_like_update(row, mode, Tn, N, state):
    import bench
    from wsmgmap.common.aux_losses import AuxLosses
    from wsmgmap.models.policy import BasePolicy
    from instr_rnn_util import Box
    pol = BasePolicy(None, Box(), instr_config(row, num_proc=1, compute_dtype=mode))
    pol.load_state_dict(state)
    pol.net.instruction_encoder.embedding_layer.weight.requires_grad_(False)
    pol = pol.cuda()
    pol.train()
    pol.net.depth_encoder.eval()
    pol.net.rgb_encoder.eval()
    obs, prev, masks, weights = bench.synth_batch(Tn, N, "cuda", 77)
    AuxLosses.activate()
    AuxLosses.clear()
    h = torch.zeros(pol.net.num_recurrent_layers, N, 512, device="cuda")
    pred, aux = pol(dict(obs), h, prev, masks, weights)
    loss = bench.dagger_loss(pred, aux, obs["waypoint"], weights)
    loss.backward()
    AuxLosses.deactivate()
    grads = {n: p.grad.detach().float() for n, p in pol.named_parameters() if p.grad is not None}
    return pred.detach().float(), float(loss.detach()), grads


@pytest.mark.parametrize("row", ["gru2", "lstm1"])
def test_instruction_rnn_bf16_mode_tracks_f32_mode(row):
    from wsmgmap.models.policy import BasePolicy
    from instr_rnn_util import Box
    torch.manual_seed(0)
    state = BasePolicy(None, Box(), instr_config(row, num_proc=1)).state_dict()
    p32, l32, g32 = _bench_like_update(row, "f32", 4, 8, state)
    p16, l16, g16 = _bench_like_update(row, "bf16", 4, 8, state)
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


@pytest.mark.parametrize("B", [1, 2])
@pytest.mark.parametrize("row", ["gru2", "lstm1"])
def test_instruction_rnn_act_equals_staged_net_forward(row, B):
    """act() (rollout: early instruction branch, packed weights, dedup reuse) against the staged update-path net.forward of a
    twin policy on the same steps: hidden states and the deterministic action within 1e-5."""
    pa, pb = build_instr_policy(row, num_proc=B).cuda().eval(), build_instr_policy(row, num_proc=B).cuda().eval()
    gen = torch.Generator(device="cuda")
    gen.manual_seed(11)
    ins = _instructions(B, gen)
    nl = pa.net.num_recurrent_layers
    ha = torch.randn(nl, B, 512, device="cuda", generator=gen) * 0.5
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
@pytest.mark.parametrize("row", ["gru2", "lstm1"])
def test_instruction_rnn_graphed_act_matches_eager_act(row, mode):
    """GraphedAct over 4 steps with restarts; between steps 1 and 2 the encoder's W_hh changes, so the replay must read the
    in-place refreshed packed weights (refresh_folded)."""
    from wsmgmap.graph import GraphedAct
    B = 2
    pa = build_instr_policy(row, num_proc=B, compute_dtype=mode).cuda().eval()
    pb = build_instr_policy(row, num_proc=B, compute_dtype=mode).cuda().eval()
    ga = GraphedAct(pa, eager_calls=1)
    gen = torch.Generator(device="cuda")
    gen.manual_seed(3)
    ins = _instructions(B, gen)
    nl = pa.net.num_recurrent_layers
    ha, hb = torch.zeros(nl, B, 512, device="cuda"), torch.zeros(nl, B, 512, device="cuda")
    prev = torch.zeros(B, 2, device="cuda")
    tol = 2e-4 if mode == "f32" else 0.0
    for k in range(4):
        if k == 3:
            with torch.no_grad():
                for p in (pa, pb):
                    p.net.instruction_encoder.encoder_rnn.weight_hh_l0.mul_(0.5)
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


@pytest.mark.parametrize("row", ["gru2", "lstm1"])
def test_instruction_rnn_graphed_update_matches_eager_updates(row):
    from wsmgmap import optim
    from wsmgmap.common.aux_losses import AuxLosses
    from wsmgmap.graph import GraphedUpdate
    obs_np, prev, masks, weights = cases.update_inputs(4, 2)
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
    pa, pb = train_mode(build_instr_policy(row).cuda()), train_mode(build_instr_policy(row).cuda())
    oa = optim.Adam(pa.parameters(), lr=1e-5, capturable=True)
    ob = optim.Adam(pb.parameters(), lr=1e-5)
    gu = GraphedUpdate(pa, oa, loss_fn, eager_calls=2)
    la, lb = [], []
    nl = pa.net.num_recurrent_layers
    for k in range(4):
        h = torch.zeros(nl, 2, 512, device="cuda")
        la.append(float(gu(obs, h, prev, masks, weights)))
        ob.zero_grad(set_to_none=True)
        AuxLosses.clear()
        hb = torch.zeros(nl, 2, 512, device="cuda")
        pred, aux = pb(dict(obs), hb, prev, masks, weights)
        loss = loss_fn(pred, aux, obs, weights)
        loss.backward()
        ob.step()
        lb.append(float(loss))
        assert float((h - hb).abs().max()) <= 5e-3
    assert len(gu._graphs) == 1
    np.testing.assert_allclose(la, lb, rtol=3e-3, atol=1e-5)
    for (n, x), y in zip(pa.named_parameters(), pb.parameters()):
        assert float((x - y).abs().max()) <= 2e-4 * max(1.0, float(y.abs().max())), n
    AuxLosses.deactivate()
    pa.check_status()
