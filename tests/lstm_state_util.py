"""Shared helpers of the LSTM state-encoder tests (MODEL.STATE_ENCODER.rnn_type = "LSTM")."""
import numpy as np
import torch

from oracle import detfill
from util import T, state_dict_values


class Box:
    shape = (2,)


def lstm_config(num_proc=2, compute_dtype="f32"):
    from wsmgmap.config import default_model_config
    mc = default_model_config(num_proc=num_proc, compute_dtype=compute_dtype)
    mc.STATE_ENCODER.rnn_type = "LSTM"
    return mc


def lstm_state_dict_values(pol):
    """The hash fill of the GRU tests, with the state encoders' rnn.* tensors filled at their LSTM shapes (4H rows) — the
    values tools/make_goldens.py gave the reference's LSTM policy for g10."""
    sd = state_dict_values()
    for k, v in pol.state_dict().items():
        if "state_encoder.rnn." in k:
            sd[k] = T(detfill.state_value(k, tuple(v.shape))).to(v.dtype)
    return sd


def build_lstm_policy(num_proc=2, compute_dtype="f32"):
    from wsmgmap.models.policy import BasePolicy
    pol = BasePolicy(None, Box(), lstm_config(num_proc, compute_dtype))
    pol.load_state_dict(lstm_state_dict_values(pol), strict=True)
    pol.net.instruction_encoder.embedding_layer.weight.requires_grad_(False)
    return pol


def lstm_split_at_zeros(x, h, c, masks, w_ih, w_hh, b_ih, b_hh):
    """habitat-lab v0.1.5 RNNStateEncoder (rnn_type "LSTM", one layer) restated in the arithmetic of whatever dtype it is given:
    the [T*N, in] sequence is split wherever any mask is 0, and both h and c are multiplied by the masks of each segment's first
    step; inside a segment the plain LSTM cell (gate order i, f, g, o).  -> (y [T*N, H], h_T [1, N, H], c_T [1, N, H])."""
    n = h.size(1)
    t = x.size(0) // n
    x = x.view(t, n, -1)
    m = masks.view(t, n)
    zeros = (m[1:] == 0.0).any(dim=-1).nonzero().flatten().tolist()
    bounds = [0] + [z + 1 for z in zeros] + [t]
    hh, cc = h[0], c[0]
    outs = []
    for s, e in zip(bounds[:-1], bounds[1:]):
        hh = hh * m[s].view(-1, 1)
        cc = cc * m[s].view(-1, 1)
        for k in range(s, e):
            g = x[k] @ w_ih.t() + b_ih + hh @ w_hh.t() + b_hh
            i, f, gg, o = g.chunk(4, dim=1)
            cc = torch.sigmoid(f) * cc + torch.sigmoid(i) * torch.tanh(gg)
            hh = torch.sigmoid(o) * torch.tanh(cc)
            outs.append(hh)
    return torch.stack(outs).reshape(t * n, -1), hh.unsqueeze(0), cc.unsqueeze(0)


def restart_masks(t, n, column_only=False):
    """Episode restarts at t = 0 (half the columns), mid-sequence, and one restart in one column only."""
    m = torch.ones(t, n)
    m[0, : max(1, n // 2)] = 0
    if t > 3 and not column_only:
        m[t // 2, :] = 0
    if t > 2:
        m[t - 2 if t > 3 else 1, n - 1] = 0
    return m


def seeded(shape, scale, seed):
    g = np.random.RandomState(seed)
    return torch.from_numpy(g.uniform(-scale, scale, size=shape).astype(np.float32))
