"""CPU: the GRU and unidirectional instruction encoders (MODEL.INSTRUCTION_ENCODER.rnn_type / .bidirectional / .hidden_size):
construction with the reference's encoder_rnn.* keys and shapes, the checkpoint contract, and the CPU (stock) route (the
kernel route is tested on the GPU, tests/test_gpu_instruction_rnn.py)."""
import copy

import numpy as np
import pytest
import torch

from instr_rnn_util import ROWS, build_instr_policy, instr_encoder
from oracle import detfill as df
from util import T, golden


@pytest.mark.parametrize("row", ["gru2", "lstm1"])
def test_instruction_policy_constructs_with_reference_shapes(row):
    cell, bidir, hidden, gold = ROWS[row]
    pol = build_instr_policy(row)
    enc = pol.net.instruction_encoder
    assert isinstance(enc.encoder_rnn, torch.nn.GRU if cell == "GRU" else torch.nn.LSTM)
    assert enc.output_size == 256 and enc.kernel_cell == cell
    g = golden(gold)
    shapes = {k[len("shape."):]: tuple(int(s) for s in g[k]) for k in g.files if k.startswith("shape.")}
    assert len(shapes) == (8 if bidir else 4)
    sd = pol.state_dict()
    assert {k for k in sd if "encoder_rnn." in k} == set(shapes)
    for k, s in shapes.items():
        assert tuple(sd[k].shape) == s, k


def test_kernel_cell_names_the_kernel_shapes_only():
    for (cell, bidir, hidden), want in {("LSTM", True, 128): "LSTM", ("GRU", True, 128): "GRU", ("LSTM", False, 256): "LSTM",
                                        ("GRU", False, 256): "GRU", ("LSTM", True, 64): None, ("GRU", False, 128): None,
                                        ("GRU", True, 256): None}.items():
        assert instr_encoder(cell, bidir, hidden, "kc").kernel_cell == want, (cell, bidir, hidden)


@pytest.mark.parametrize("row", ["gru2", "lstm1"])
def test_instruction_policy_checkpoint_round_trip(row, tmp_path):
    from wsmgmap import checkpoint as ck
    pol = build_instr_policy(row)
    path = ck.save_checkpoint(pol, str(tmp_path / "ckpts"), "ckpt.0.pth", extra_state={"dagger_it": 1})
    d = ck.load_checkpoint(path)
    G = 3 if ROWS[row][0] == "GRU" else 4
    H = ROWS[row][2]
    assert tuple(d["state_dict"]["net.instruction_encoder.encoder_rnn.weight_hh_l0"].shape) == (G * H, H)
    fresh = build_instr_policy(row)
    with torch.no_grad():
        fresh.net.instruction_encoder.encoder_rnn.weight_hh_l0.zero_()
    it, ep, rep = ck.resume_dagger(fresh, str(tmp_path / "ckpts"), epochs=4)
    assert (it, ep) == (1, 1) and not rep.missing_keys and not rep.unexpected_keys
    a, b = pol.state_dict(), fresh.state_dict()
    assert set(a) == set(b)
    for k in a:
        assert torch.equal(a[k], b[k]), k


@pytest.mark.parametrize("row", ["gru2", "lstm1", "gru1"])
def test_cpu_forward_is_the_packed_stock_module(row):
    """On the CPU the encoder is the reference's packed nn.GRU / nn.LSTM (instruction_encoder.py:75-93): same outputs and pad
    mask as the module called directly on a packed sequence."""
    cell, bidir, hidden, _ = ROWS[row]
    enc = instr_encoder(cell, bidir, hidden, row)
    instr = T(df.tokens(f"instr.cpu.{row}", 5, [80, 37, 1, 80, 12]).astype(np.float32))
    hid, mask = enc({"instruction": instr})
    tok = instr.long()
    lengths = (tok != 0).long().sum(1)
    packed = torch.nn.utils.rnn.pack_padded_sequence(enc.embedding_layer(tok), lengths, batch_first=True, enforce_sorted=False)
    out, _ = copy.deepcopy(enc.encoder_rnn)(packed)
    ref = torch.nn.utils.rnn.pad_packed_sequence(out, batch_first=True)[0].permute(0, 2, 1)
    assert hid.shape == (5, 256, 80)
    torch.testing.assert_close(hid, ref, rtol=0, atol=0)
    assert torch.equal(mask, (ref == 0.0).all(dim=1))


def test_packed_rnn_weights_refresh_in_place():
    """packed_rnn_weights (alias packed_lstm_weights) keeps its tensors and rewrites them in place when a parameter changes:
    the contract MGMapNet.refresh_folded relies on for captured rollout steps."""
    for cell, bidir, hidden in (("GRU", True, 128), ("LSTM", False, 256), ("LSTM", True, 128)):
        enc = instr_encoder(cell, bidir, hidden, "pk")
        assert enc.packed_lstm_weights.__func__ is enc.packed_rnn_weights.__func__
        assert enc.packed_rnn_weights(refresh_only=True) == 0
        w = enc.packed_rnn_weights()
        D, G = (2 if bidir else 1), (3 if cell == "GRU" else 4)
        assert [tuple(t.shape) for t in w] == [(D * G * hidden, 50), (D * G * hidden,), (D, G * hidden, hidden), (D, G * hidden)]
        ptrs = [t.data_ptr() for t in w]
        assert enc.packed_rnn_weights(refresh_only=True) == 0
        with torch.no_grad():
            enc.encoder_rnn.weight_hh_l0.mul_(2.0)
        assert enc.packed_rnn_weights(refresh_only=True) == 1
        w2 = enc.packed_rnn_weights()
        assert [t.data_ptr() for t in w2] == ptrs
        assert torch.equal(w2[2][0], enc.encoder_rnn.weight_hh_l0)
