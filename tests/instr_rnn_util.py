"""Shared helpers of the instruction-encoder tests for MODEL.INSTRUCTION_ENCODER.rnn_type / .bidirectional / .hidden_size:
the three settings besides the default bidirectional LSTM whose output width (256) the policy admits."""
import torch

from oracle import detfill
from util import T, state_dict_values

# name -> (rnn_type, bidirectional, hidden_size, golden of the reference's update or None)
ROWS = {"gru2": ("GRU", True, 128, "g11_gru_instr_update.npz"),
        "lstm1": ("LSTM", False, 256, "g12_unilstm_instr_update.npz"),
        "gru1": ("GRU", False, 256, None)}


class Box:
    shape = (2,)


def instr_config(row, num_proc=2, compute_dtype="f32"):
    from wsmgmap.config import default_model_config
    mc = default_model_config(num_proc=num_proc, compute_dtype=compute_dtype)
    cell, bidir, hidden, _ = ROWS[row]
    mc.INSTRUCTION_ENCODER.rnn_type = cell
    mc.INSTRUCTION_ENCODER.bidirectional = bidir
    mc.INSTRUCTION_ENCODER.hidden_size = hidden
    return mc


def instr_state_dict_values(pol):
    """The hash fill of the default tests, with the instruction encoder's encoder_rnn.* tensors filled at this encoder's
    keys and shapes — the values tools/make_goldens.py gave the reference's policy for g11 / g12."""
    own = pol.state_dict()
    sd = {k: v for k, v in state_dict_values().items() if k in own}
    for k, v in own.items():
        if "instruction_encoder.encoder_rnn." in k:
            sd[k] = T(detfill.state_value(k, tuple(v.shape))).to(v.dtype)
    return sd


def build_instr_policy(row, num_proc=2, compute_dtype="f32"):
    from wsmgmap.models.policy import BasePolicy
    pol = BasePolicy(None, Box(), instr_config(row, num_proc, compute_dtype))
    pol.load_state_dict(instr_state_dict_values(pol), strict=True)
    pol.net.instruction_encoder.embedding_layer.weight.requires_grad_(False)
    return pol


def instr_encoder(cell, bidir, hidden, tag):
    """A stand-alone InstructionEncoder with seeded parameters (embedding included)."""
    import numpy as np
    from wsmgmap.config import default_model_config
    from wsmgmap.models.encoders.instruction_encoder import InstructionEncoder
    cfg = default_model_config().INSTRUCTION_ENCODER
    cfg.rnn_type, cfg.bidirectional, cfg.hidden_size = cell, bidir, hidden
    enc = InstructionEncoder(cfg)
    sd = {k: T(detfill.uniform(f"instr.{tag}.{k}", tuple(v.shape), 1.0 if "embedding" in k else float(np.sqrt(3.0 / hidden)) * 2))
          for k, v in enc.state_dict().items()}
    enc.load_state_dict(sd)
    return enc
