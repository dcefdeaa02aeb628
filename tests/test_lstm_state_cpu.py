"""CPU: the LSTM state encoders (MODEL.STATE_ENCODER.rnn_type = "LSTM"): construction, state layout, checkpoint contract and
the stock route's semantics (the kernel route is tested on the GPU, tests/test_gpu_lstm_state.py)."""
import numpy as np
import pytest
import torch

from lstm_state_util import build_lstm_policy, lstm_split_at_zeros, restart_masks, seeded
from util import golden, state_spec


def test_lstm_policy_constructs_with_habitat_state_layout():
    pol = build_lstm_policy()
    assert pol.net.num_recurrent_layers == 4
    assert pol.net.state_encoder.num_recurrent_layers == 2 and pol.net.second_state_encoder.num_recurrent_layers == 2
    assert isinstance(pol.net.state_encoder.rnn, torch.nn.LSTM)
    sd = pol.state_dict()
    assert set(sd) == set(state_spec())          # same checkpoint keys as the GRU policy
    g = golden("g10_lstm_update.npz")
    shapes = {k[len("shape."):]: tuple(int(s) for s in g[k]) for k in g.files if k.startswith("shape.")}
    assert len(shapes) == 8
    for k, s in shapes.items():
        assert tuple(sd[k].shape) == s, k


def test_state_encoder_types_and_depth_refused_as_before():
    from wsmgmap.models.rnn_state_encoder import RNNStateEncoder
    for kw in (dict(rnn_type="RNN"), dict(num_layers=2), dict(num_layers=2, rnn_type="LSTM")):
        with pytest.raises(ValueError):
            RNNStateEncoder(16, 512, **kw)
    e = RNNStateEncoder(16, 512, rnn_type="LSTM")
    assert e.num_recurrent_layers == 2
    for name, p in e.rnn.named_parameters():
        if "bias" in name:
            assert float(p.detach().abs().max()) == 0.0
        else:    # orthogonal initialisation
            q = p.detach().double()
            eye = q.t() @ q if q.size(0) > q.size(1) else q @ q.t()
            assert torch.allclose(eye, torch.eye(eye.size(0), dtype=torch.float64), atol=1e-5), name


def test_lstm_policy_checkpoint_round_trip(tmp_path):
    from wsmgmap import checkpoint as ck
    pol = build_lstm_policy()
    path = ck.save_checkpoint(pol, str(tmp_path / "ckpts"), "ckpt.0.pth", extra_state={"dagger_it": 1})
    d = ck.load_checkpoint(path)
    assert tuple(d["state_dict"]["net.state_encoder.rnn.weight_hh_l0"].shape) == (2048, 512)
    fresh = build_lstm_policy()
    with torch.no_grad():
        fresh.net.second_state_encoder.rnn.weight_hh_l0.zero_()
        fresh.net.state_encoder.rnn.bias_ih_l0.add_(1.0)
    it, ep, rep = ck.resume_dagger(fresh, str(tmp_path / "ckpts"), epochs=4)
    assert (it, ep) == (1, 1) and not rep.missing_keys and not rep.unexpected_keys
    a, b = pol.state_dict(), fresh.state_dict()
    assert set(a) == set(b)
    for k in a:
        assert torch.equal(a[k], b[k]), k


@pytest.mark.parametrize("Tn,N,column_only", [(1, 3, False), (4, 2, False), (9, 3, False), (9, 3, True), (7, 11, False)])
def test_lstm_forward_stock_matches_split_at_zeros_float64(Tn, N, column_only):
    from wsmgmap.models.rnn_state_encoder import RNNStateEncoder
    In, Hd = 24, 16
    enc = RNNStateEncoder(In, Hd, rnn_type="LSTM").double()
    with torch.no_grad():
        for i, (name, p) in enumerate(enc.rnn.named_parameters()):
            p.copy_(seeded(tuple(p.shape), 0.4, 100 + i).double())
    x = seeded((Tn * N, In), 1.5, 1).double()
    hc = seeded((2, N, Hd), 1.0, 2).double()
    m = restart_masks(Tn, N, column_only).double()
    if Tn > 1:
        assert float(m[1:].min()) == 0.0        # at least one restart after t = 0
    y, h = enc.forward_stock(x, hc.clone(), m.view(-1, 1))
    r = enc.rnn
    yr, hr, cr = lstm_split_at_zeros(x, hc[0:1], hc[1:2], m, r.weight_ih_l0, r.weight_hh_l0, r.bias_ih_l0, r.bias_hh_l0)
    assert h.shape == (2, N, Hd)
    np.testing.assert_allclose(y.detach().numpy(), yr.detach().numpy(), atol=1e-12, rtol=0)
    np.testing.assert_allclose(h[0:1].detach().numpy(), hr.detach().numpy(), atol=1e-12, rtol=0)
    np.testing.assert_allclose(h[1:2].detach().numpy(), cr.detach().numpy(), atol=1e-12, rtol=0)
