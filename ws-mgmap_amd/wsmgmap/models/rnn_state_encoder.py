"""Masked GRU / LSTM state encoder with the interface and state_dict keys (`rnn.*`) of habitat-lab
v0.1.5 `RNNStateEncoder`, which the reference imports (mg_map_policy.py:9,118,147).
Semantics: the hidden state is multiplied by `masks` before a step; for a flattened
[T*N, .] sequence that happens wherever an episode restarts.  With rnn_type "LSTM" (the reference's
MODEL.STATE_ENCODER.rnn_type option) the state slice holds habitat's packed layout [h; c] on dim 0
(num_recurrent_layers = 2 * num_layers), and both h and c are masked.

`forward` runs the persistent HIP kernel pairs of csrc/wsmg_rnn.hip: the input
projection of all T*N rows is one GEMM, the recurrence is ONE launch per direction instead of
~30 MIOpen launches per time step, and restarts are applied in-kernel (no host sync).
`forward_stock` keeps the stock PyTorch-ROCm (MIOpen) formulation for comparison in tests; an
LSTM whose hidden size is not the kernels' 512 always takes it.
The `nn.GRU` / `nn.LSTM` child is the parameter container (checkpoint keys rnn.weight_ih_l0, ...).
"""
import torch
import torch.nn as nn

from .. import ops
from ..recurrent import MAX_BATCH  # batch slots of the kernel; wider batches are processed in independent column chunks

KERNEL_HIDDEN = 512  # hidden size of the persistent LSTM kernels


class RNNStateEncoder(nn.Module):
    def __init__(self, input_size, hidden_size, num_layers=1, rnn_type="GRU"):
        super().__init__()
        if rnn_type not in ("GRU", "LSTM") or num_layers != 1:
            raise ValueError("the WS-MGMap policy uses single-layer GRU or LSTM state encoders")
        self._is_lstm = rnn_type == "LSTM"
        self._num_recurrent_layers = num_layers * (2 if self._is_lstm else 1)
        self.rnn = getattr(nn, rnn_type)(input_size=input_size, hidden_size=hidden_size, num_layers=num_layers)
        for name, p in self.rnn.named_parameters():
            if "weight" in name:
                nn.init.orthogonal_(p)
            elif "bias" in name:
                nn.init.constant_(p, 0)

    @property
    def num_recurrent_layers(self):
        return self._num_recurrent_layers

    # habitat's state layout: an LSTM's (h, c) travel as one [2 * num_layers, N, H] tensor
    def _pack_hidden(self, hidden_states):
        if self._is_lstm:
            return torch.cat([hidden_states[0], hidden_states[1]], dim=0)
        return hidden_states

    def _unpack_hidden(self, hidden_states):
        if self._is_lstm:
            n = self.rnn.num_layers
            return hidden_states[0:n], hidden_states[n:]
        return hidden_states

    def forward(self, x, hidden_states, masks):
        """x [T*N, in] (time-major rows) or [N, in]; hidden_states [1, N, H] ([2, N, H] = [h; c] for an LSTM); masks [T*N, 1]."""
        from ..debug import sw
        if sw.rnn_stock:      # no persistent kernel (bench.py's last fallback under a process group; MIOpen, one host read-back)
            return self.forward_stock(x, hidden_states, masks)
        r = self.rnn
        if self._is_lstm and r.hidden_size != KERNEL_HIDDEN:
            return self.forward_stock(x, hidden_states, masks)
        n = hidden_states.size(1)
        t = x.size(0) // n
        if ops.rows_route(x):      # rollout: the input projection of a few rows in one launch
            gi = ops.linear_rows(x, r.weight_ih_l0, r.bias_ih_l0).view(t, n, -1)
        else:
            gi = torch.addmm(r.bias_ih_l0, x, r.weight_ih_l0.t()).view(t, n, -1)
        m = masks.reshape(t, n).float()
        cell = ops.LSTM if self._is_lstm else ops.GRU
        state = [s.clone() for s in hidden_states.unbind(0)]  # the caller overwrites hidden_states in place (reference contract)
        w_hh, b_hh = r.weight_hh_l0, r.bias_hh_l0
        if n <= MAX_BATCH:
            y, *tail = cell.masked(gi, w_hh, b_hh, state, m)
        else:  # independent column chunks: outputs side by side on the batch dimension
            parts = [cell.masked(gi[:, c:c + MAX_BATCH], w_hh, b_hh, [s[c:c + MAX_BATCH] for s in state], m[:, c:c + MAX_BATCH])
                     for c in range(0, n, MAX_BATCH)]
            y, *tail = [torch.cat(p, dim=1 if i == 0 else 0) for i, p in enumerate(zip(*parts))]
        h_n = y[-1:]
        return y.reshape(t * n, -1), torch.cat([h_n] + [c.unsqueeze(0) for c in tail]) if tail else h_n

    # -- stock formulation (MIOpen GRU / LSTM, split at restarts; one host sync) -------------------------
    @staticmethod
    def restart_steps(masks, n):
        t = masks.numel() // n
        if t <= 1:
            return []
        flags = (masks.view(t, n)[1:] == 0.0).any(dim=-1)
        return (flags.nonzero().flatten() + 1).tolist()

    def _masked(self, hidden_states, mask):
        if self._is_lstm:
            return tuple(v * mask for v in hidden_states)
        return hidden_states * mask

    def forward_stock(self, x, hidden_states, masks):
        n = hidden_states.size(1)
        hidden_states = self._unpack_hidden(hidden_states)
        if x.size(0) == n:
            y, h = self.rnn(x.unsqueeze(0), self._masked(hidden_states, masks.unsqueeze(0)))
            return y.squeeze(0), self._pack_hidden(h)
        t = x.size(0) // n
        x = x.view(t, n, x.size(1))
        m = masks.view(t, n, 1)
        bounds = [0] + self.restart_steps(masks, n) + [t]
        h = hidden_states
        outs = []
        for s, e in zip(bounds[:-1], bounds[1:]):
            y, h = self.rnn(x[s:e], self._masked(h, m[s].unsqueeze(0)))
            outs.append(y)
        y = outs[0] if len(outs) == 1 else torch.cat(outs, dim=0)
        return y.reshape(t * n, -1), self._pack_hidden(h)
