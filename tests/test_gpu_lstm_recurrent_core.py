"""GPU: the pipelined recurrent core of the update (wsmgmap/recurrent.py) with LSTM state encoders (MODEL.STATE_ENCODER.rnn_type =
"LSTM", habitat's [h; c] state): the chained whole-sequence LSTM launches (wsmg_lstm_state_fwd_chain / _bwd_chain), the chunk-launch
route, the one-stream route a HIP-graph capture records, the route the policy takes, the reference's goldens through the core, and
the in-process fallback after a reported timeout."""
import numpy as np
import pytest
import torch

from lstm_state_util import build_lstm_policy, lstm_config
from util import NULL_GRAD, T, golden

pytestmark = pytest.mark.gpu

CORE = ("net.state_encoder.", "net.second_state_encoder.", "net.state_text_q_layer.", "net.text_map_q_layer.", "net.text_map_k_layer.",
        "net.second_state_compress.", "action_distribution.", "prog_pred.")


@pytest.fixture(autouse=True)
def _aux_losses_off():
    from wsmgmap.common.aux_losses import AuxLosses
    AuxLosses.deactivate()
    AuxLosses.clear()
    yield
    AuxLosses.deactivate()
    AuxLosses.clear()


@pytest.fixture
def core_calls(monkeypatch):
    """Counts the calls of the pipelined block (wsmgmap.recurrent.recurrent_block) the policy makes."""
    from wsmgmap import recurrent
    calls = [0]
    block = recurrent.recurrent_block

    def counted(*a, **k):
        calls[0] += 1
        return block(*a, **k)
    monkeypatch.setattr(recurrent, "recurrent_block", counted)
    return calls


def _train_mode(pol):
    pol.train()
    pol.net.depth_encoder.eval()
    pol.net.rgb_encoder.eval()
    return pol


_STATE = {}


def _lstm_policy(mode):
    """An LSTM policy at torch's default initialisation (seed 0), as test_gpu_round4's GRU policy."""
    from wsmgmap.models.policy import BasePolicy
    from lstm_state_util import Box
    if "sd" not in _STATE:
        torch.manual_seed(0)
        _STATE["sd"] = BasePolicy(None, Box(), lstm_config(num_proc=1)).state_dict()
    pol = BasePolicy(None, Box(), lstm_config(num_proc=1, compute_dtype=mode))
    pol.load_state_dict(_STATE["sd"], strict=True)
    pol.net.instruction_encoder.embedding_layer.weight.requires_grad_(False)
    return _train_mode(pol.cuda())


def _one_update(pol, obs, prev, masks, weights, N, chunks):
    """forward + DAgger loss + backward with the recurrent core staged (chunks = 0) or pipelined; -> (pred, loss, att, [h1, c1, h2, c2],
    grads)."""
    import bench
    from wsmgmap.common.aux_losses import AuxLosses
    pol.net.recurrent_chunks = chunks
    for p in pol.parameters():
        p.grad = None
    AuxLosses.activate()
    AuxLosses.clear()
    h = torch.zeros(4, N, 512, device="cuda")
    o = dict(obs)
    pred, aux = pol(o, h, prev, masks, weights)
    loss = bench.dagger_loss(pred, aux, o["waypoint"], weights)
    loss.backward()
    torch.cuda.synchronize()
    AuxLosses.deactivate()
    grads = {k: (None if p.grad is None else p.grad.detach().clone()) for k, p in pol.named_parameters()}
    return pred.detach().clone(), float(loss), pol.net.att_map_t_m.detach().clone(), h.clone(), grads


def _close(x, y, name, tol=2e-5):
    assert x.shape == y.shape, name
    d = float((x.double() - y.double()).abs().max())
    m = float(y.double().abs().max())
    print(f"{name}: max |diff| {d:.3e}, max |ref| {m:.3e}, bar {tol * max(1e-6, m):.3e}")
    assert d <= tol * max(1e-6, m), (name, d, m)


def _batch(T_, N, seed):
    import bench
    obs, prev, masks, weights = bench.synth_batch(T_, N, torch.device("cuda"), seed)
    masks = masks.clone()
    masks.view(T_, N)[T_ // 2 + 1, N - 1] = 0          # an episode restart inside a chunk
    return obs, prev, masks, weights


# ----------------------------------------------------------------------------- 1. the pipelined LSTM core vs the staged LSTM route
@pytest.mark.parametrize("mode,T_,N", [("bf16", 64, 8), ("f32", 16, 8), ("bf16", 12, 3)])
def test_pipelined_lstm_core_matches_the_staged_route(mode, T_, N, core_calls):
    """The bars of test_gpu_round4::test_pipelined_recurrent_core_matches_the_staged_route, with LSTM state encoders: action logits,
    map attention row and the four carried states [h1, c1, h2, c2] within 2e-5 of the largest element, the loss within 2e-6, every
    gradient within 5e-5 in f32 and for the core's parameters (bf16 map stack: cos >= 0.9999 and 3e-2), and the pipelined route
    repeatable bit for bit."""
    from wsmgmap import ops
    pol = _lstm_policy(mode)
    obs, prev, masks, weights = _batch(T_, N, 77)
    a = _one_update(pol, obs, prev, masks, weights, N, 0)
    assert core_calls[0] == 0
    b = _one_update(pol, obs, prev, masks, weights, N, 4)
    c = _one_update(pol, obs, prev, masks, weights, N, 4)
    assert core_calls[0] == 2, "the LSTM policy did not take the pipelined core"
    ops.check_rnn_status()
    _close(b[0], a[0], "pred")
    print(f"loss: staged {a[1]:.9g}, core {b[1]:.9g}")
    assert abs(a[1] - b[1]) <= 2e-6 * max(1.0, abs(a[1]))
    _close(b[2], a[2], "att_map_t_m")
    assert a[3].shape == (4, N, 512)
    for i, n in enumerate(("h1", "c1", "h2", "c2")):
        _close(b[3][i], a[3][i], "rnn_hidden_states " + n)
    assert set(k for k, g in a[4].items() if g is not None) == set(k for k, g in b[4].items() if g is not None)
    for k, g in a[4].items():
        if g is None or k in NULL_GRAD:
            continue
        if mode == "f32" or k.startswith(CORE):
            _close(b[4][k], g, k, tol=5e-5)
        else:
            x, y = b[4][k].double().flatten(), g.double().flatten()
            if float(y.norm()) > 0:
                cos = float((x @ y) / (x.norm() * y.norm()))
                assert cos >= 0.9999, (k, cos)
            _close(b[4][k], g, k, tol=3e-2)
    assert torch.equal(b[0], c[0]) and b[1] == c[1]
    assert torch.equal(b[3], c[3])
    for k, g in b[4].items():
        if g is not None:
            assert torch.equal(g, c[4][k]), k


# ----------------------------------------------------------------------------- 2. chained == chunk launches
@pytest.mark.parametrize("chunks,T_,N", [(4, 64, 8), (2, 64, 8), (4, 16, 3), (2, 16, 3)])
def test_chained_lstm_core_is_bit_identical_to_the_chunk_launch_route(chunks, T_, N, monkeypatch, core_calls):
    """One whole-sequence LSTM launch per recurrence, chained to the attention stage by per-chunk counters, against K chunk launches
    per recurrence ordered by events (the carried state (y[t0-1], save_c[t0-1]) forward, (dh0, dc0) backward): logits, loss, attention
    row, the four carried states and every gradient equal bit for bit, twice in a row (a missed wait would read a chunk early)."""
    from wsmgmap import debug, ops
    pol = _lstm_policy("bf16")
    obs, prev, masks, weights = _batch(T_, N, 79)
    monkeypatch.setattr(debug.sw, "recurrent_chain", False)
    a = _one_update(pol, obs, prev, masks, weights, N, chunks)
    monkeypatch.setattr(debug.sw, "recurrent_chain", True)
    for rep in range(2):
        b = _one_update(pol, obs, prev, masks, weights, N, chunks)
        ops.check_rnn_status()
        assert torch.equal(a[0], b[0]) and a[1] == b[1], rep
        assert torch.equal(a[2], b[2]) and torch.equal(a[3], b[3]), rep
        for k, g in a[4].items():
            if g is not None:
                assert torch.equal(g, b[4][k]), (rep, k)
    assert core_calls[0] == 3


# ----------------------------------------------------------------------------- 3. the route
def test_lstm_policy_takes_the_chained_core(core_calls, monkeypatch):
    """With recurrent_chunks = 4 an LSTM policy's update runs the pipelined block, and the fallback's level 0 says so; an LSTM on
    the stock route stays staged and is described as staged."""
    from wsmgmap import debug, ops
    from wsmgmap.fallback import RecurrentCoreFallback
    pol = _lstm_policy("bf16")
    assert pol.net.recurrent_chunks == 4
    fb = RecurrentCoreFallback(pol, verbose=False)
    assert fb.level == 0 and fb.name.startswith("chained"), fb.name
    obs, prev, masks, weights = _batch(8, 4, 81)
    _one_update(pol, obs, prev, masks, weights, 4, 4)
    ops.check_rnn_status()
    assert core_calls[0] == 1
    monkeypatch.setattr(debug.sw, "rnn_stock", True)
    assert RecurrentCoreFallback(pol, verbose=False).name.startswith("staged")
    _one_update(pol, obs, prev, masks, weights, 4, 4)
    assert core_calls[0] == 1


# ----------------------------------------------------------------------------- 4. the reference's goldens through the core
def _golden_case(name):
    from oracle import cases
    g = golden(name)
    if name.startswith("g13"):
        obs_np, prev, _, weights = cases.update_inputs(8, 4, n_tok=(80, 37, 1, 55), tag="g13")
        Tn, N = 8, 4
        assert float(g["masks"].reshape(8, 4)[5, 2]) == 0.0      # the golden's restart inside a chunk
    else:
        obs_np, prev, _, weights = cases.update_inputs(4, 2)
        Tn, N = 4, 2
    return g, obs_np, prev, g["masks"], weights, Tn, N


@pytest.mark.parametrize("name", ["g13_lstm_core_update.npz", "g10_lstm_update.npz"])
def test_lstm_core_update_matches_the_reference_golden(name, core_calls):
    """The reference's LSTM policy (g13: T = 8, N = 4, four instructions; g10: T = 4, N = 2) against one update through the chained
    core, with the bars of test_gpu_lstm_state::test_lstm_update_path_forward_backward_g10."""
    import test_gpu_lstm_state as ls
    g, obs_np, prev, masks, weights, Tn, N = _golden_case(name)
    pol = build_lstm_policy().cuda()
    assert pol.net.recurrent_chunks == 4
    pred, aux, loss, h0, mon = ls._update(pol, obs_np, prev, masks, weights, Tn, N)
    assert core_calls[0] == 1, "the update did not run the pipelined core"
    err = float(np.abs(pred.detach().cpu().numpy() - g["pred"]).max())
    print(f"{name}: logits {err:.3e}, aux {abs(float(aux) - float(g['aux_loss'])):.3e}, loss {abs(float(loss) - float(g['loss'])):.3e}, "
          f"h_out {float(np.abs(h0.detach().cpu().numpy() - g['h_out']).max()):.3e}")
    assert err <= 1e-4, f"action logits differ from the reference by {err:.3e} (bar 1e-4)"
    assert abs(float(aux) - float(g["aux_loss"])) <= 1e-4
    assert abs(float(loss) - float(g["loss"])) <= 1e-4
    for n, v in mon.items():
        np.testing.assert_allclose(v, g["aux." + n], atol=1e-4, rtol=1e-4)
    np.testing.assert_allclose(pol.prog.detach().cpu().numpy(), g["prog"], atol=1e-4, rtol=0)
    assert h0.shape == (4, N, 512)
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


# ----------------------------------------------------------------------------- 5. HIP-graph update (the one-stream block)
def test_lstm_graphed_update_matches_eager_pipelined_updates(core_calls):
    """GraphedUpdate of an LSTM policy records the one-stream form of the block; its replays against eager updates of a twin on
    the chained core, with the bars of test 1 (f32): loss within 2e-6, the written-back [h1, c1, h2, c2] within 2e-5 of the largest
    element, every gradient within 5e-5.  lr = 0 keeps both policies at the same parameters for every update."""
    from wsmgmap import optim
    from wsmgmap.common.aux_losses import AuxLosses
    from wsmgmap.graph import GraphedUpdate
    g, obs_np, prev, masks, weights, Tn, N = _golden_case("g10_lstm_update.npz")
    obs = {k: T(v).cuda() for k, v in obs_np.items()}
    prev, masks, weights = T(prev).cuda(), T(masks).cuda(), T(weights).cuda()
    AuxLosses.activate()

    def loss_fn(pred, aux, o, w):
        return (pred ** 2).mean() + aux

    pa, pb = _train_mode(build_lstm_policy().cuda()), _train_mode(build_lstm_policy().cuda())
    oa = optim.Adam(pa.parameters(), lr=0.0, capturable=True)
    ob = optim.Adam(pb.parameters(), lr=0.0)
    gu = GraphedUpdate(pa, oa, loss_fn, eager_calls=2)
    for k in range(4):
        h = torch.zeros(4, N, 512, device="cuda")
        la = float(gu(obs, h, prev, masks, weights))
        ga = {n: p.grad.detach().clone() for n, p in pa.named_parameters() if p.grad is not None}
        ob.zero_grad(set_to_none=True)
        AuxLosses.clear()
        hb = torch.zeros(4, N, 512, device="cuda")
        n_before = core_calls[0]
        pred, aux = pb(dict(obs), hb, prev, masks, weights)
        assert core_calls[0] == n_before + 1
        loss = loss_fn(pred, aux, obs, weights)
        loss.backward()
        ob.step()
        lb = float(loss)
        torch.cuda.synchronize()
        print(f"update {k}: loss graphed {la:.9g} eager {lb:.9g}")
        assert abs(la - lb) <= 2e-6 * max(1.0, abs(lb)), k
        assert float(hb[1].abs().max()) > 0
        for i in range(4):
            _close(h[i], hb[i], f"update {k} state {i}")
        gb = {n: p.grad.detach() for n, p in pb.named_parameters() if p.grad is not None}
        assert set(ga) == set(gb), k
        for n in gb:
            if n not in NULL_GRAD:
                _close(ga[n], gb[n], f"update {k} grad {n}", tol=5e-5)
    assert len(gu._graphs) == 1
    AuxLosses.deactivate()
    pa.check_status()
    pb.check_status()


# ----------------------------------------------------------------------------- 6. status path: the in-process fallback
@pytest.mark.parametrize("bit", [32, 64])
def test_lstm_core_falls_back_to_the_staged_route_in_process(bit, monkeypatch, core_calls):
    """A timeout bit of the LSTM state kernels (injected with wsmg_rnn_debug_inject, as a kernel whose spin ran out would set it)
    moves an LSTM policy from the chained core to the staged route in the same process (RecurrentCoreFallback level 1); the next
    update runs staged and matches a twin's staged update with the bars of test 1."""
    from wsmgmap import _abi, debug
    from wsmgmap.fallback import RecurrentCoreFallback
    monkeypatch.setattr(debug.sw, "decoder_streams", debug.sw.decoder_streams)     # (level 1 switches it off process-wide)
    _abi.take_rnn_status()
    pol = _lstm_policy("f32")
    fb = RecurrentCoreFallback(pol, verbose=False)
    assert fb.name.startswith("chained")
    obs, prev, masks, weights = _batch(16, 4, 83)
    runs = []

    def phase():
        r = _one_update(pol, obs, prev, masks, weights, 4, pol.net.recurrent_chunks)
        runs.append(core_calls[0])
        if len(runs) == 1:
            assert _abi.lib().wsmg_rnn_debug_inject(bit) & bit
        return r
    pol.net.recurrent_chunks = 4
    fb.guarded(phase)
    assert fb.level == 1 and fb.name.startswith("staged (fallback"), fb.report()
    assert pol.net.recurrent_chunks == 0 and runs == [1, 1], runs
    assert "lstm_state_" + ("fwd" if bit == 32 else "bwd") in fb.reasons[0], fb.reasons
    nxt = _one_update(pol, obs, prev, masks, weights, 4, pol.net.recurrent_chunks)
    assert core_calls[0] == 1 and _abi.take_rnn_status() == 0
    twin = _lstm_policy("f32")
    ref = _one_update(twin, obs, prev, masks, weights, 4, 0)
    _close(nxt[0], ref[0], "pred")
    assert abs(nxt[1] - ref[1]) <= 2e-6 * max(1.0, abs(ref[1]))
    _close(nxt[3], ref[3], "rnn_hidden_states")
    for k, g in ref[4].items():
        if g is not None and k not in NULL_GRAD:
            _close(nxt[4][k], g, k, tol=5e-5)
