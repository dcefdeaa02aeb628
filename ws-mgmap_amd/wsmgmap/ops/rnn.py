"""wsmgmap.ops.rnn — the persistent masked-GRU / masked-LSTM state-encoder and packed instruction GRU / LSTM kernels.
"""
import ctypes

import torch

from .. import _abi
from ..debug import sw
from .core import _p, _raw_stream, _stream, _req, _f32, _sfx, _workspace, _rows_of, _conv_out, _launch, _zeros_f32, _prelaid, _join_side_at_end, TokenGradSink


def _rnn_workspace(nbytes, device):
    """Barrier words + exchange image of the persistent RNN kernels.  debug.sw.rnn_poison (stress tool) fills
    it with NaN first so that any stale or missed hand-off read poisons the results visibly."""
    ws = torch.empty((int(nbytes) + 3) // 4, device=device, dtype=torch.float32)
    if sw.rnn_poison:
        ws.fill_(float("nan"))
    return ws


check_rnn_status = _abi.check_rnn_status


def _prow(t, row):
    """Pointer to row `row` of a contiguous tensor (a view object per kernel argument costs more host time than the launch)."""
    return ctypes.c_void_p(t.data_ptr() + row * t.stride(0) * t.element_size())


class _Cell:
    """One state-encoder cell as the host sees it: every fact in which the GRU's and the LSTM's launches differ, stated once.
    A state travels as its rows ([N, H] each; packed on dim 0 it is habitat's layout): h for a GRU, h and c for an LSTM.  The
    launches take full-sequence tensors [T, N, .] and run `steps` steps from step t0."""

    def __init__(self, G, state_rows, save_widths, own_dgh, bits, fwd, bwd, workspace_bytes, chain_workgroups):
        self.G = G                                # gate rows per unit
        self.state_rows = state_rows              # rows of a packed state: [h] or [h; c]
        self.save_widths = save_widths            # one saved tensor [T, N, w H] per entry (new_saves)
        self.own_dgh = own_dgh                    # d(W_hh h + b_hh) is a tensor of its own (GRU), or the one gate gradient dgi (LSTM)
        self.fwd_bit, self.bwd_bit = bits         # the status bits a wait on this cell's launches reports (_abi.STATUS_BITS)
        self.fwd, self.bwd = fwd, bwd             # entry points: (clearing, owned or None, chained)
        self._wsb, self._nwg = workspace_bytes, chain_workgroups

    def workspace_bytes(self, T):
        return getattr(_abi.lib(), self._wsb)(T)

    def chain_workgroups(self):
        """Arrivals a chained launch adds to a chunk's counter."""
        return int(getattr(_abi.lib(), self._nwg)())

    def new_saves(self, T, N, H, device):
        """What one recurrence saves for its backward: GRU r, z, n, W_hn h + b_hn [T, N, H] each; LSTM save_gates [T, N, 4H]
        (i, f, g, o) and save_c [T, N, H]."""
        return [torch.empty(T, N, w * H, device=device, dtype=torch.float32) for w in self.save_widths]

    def rows(self, packed):
        """Addresses of the rows of a packed state ([N, H] will do for a GRU's)."""
        return [_prow(packed, r) for r in range(self.state_rows)]

    def _start(self, h0, y, saves, t0):
        # the rows before step t0: the caller's, or what step t0 - 1 left — h in y and (LSTM) c in save_c
        return h0 if t0 == 0 else [_prow(s, t0 - 1) for s in (y, saves[-1])[:self.state_rows]]

    def launch_fwd(self, gi, w_hh, b_hh, h0, masks, y, tail, saves, t0, steps, ws, owned=False, chain=None):
        """gi [T, N, G H], masks [T, N] -> y [T, N, H], saves (new_saves).  h0: addresses of the state rows before step 0
        (`rows`); tail: where the final rows below h go ([state_rows - 1, N, H], or [N, H]: an LSTM's c_T).  The clearing entry
        point, the owned one (`ws` zeroed once and used by nothing else) or, with chain = (Tc, in_cnt, in_target, out_cnt), the
        chained one (owned workspace)."""
        _abi.call(self.fwd[2 if chain else 1 if owned else 0], _prow(gi, t0), _p(w_hh), _p(b_hh), *self._start(h0, y, saves, t0), _prow(masks, t0),
                  steps, y.shape[1], y.shape[2], _prow(y, t0), *[_prow(tail, r) for r in range(self.state_rows - 1)],
                  *[_prow(s, t0) for s in saves], _p(ws), *(chain or ()), _stream())

    def launch_bwd(self, dy, d_end, w_hh, h0, masks, y, saves, dgi, dgh, d_start, t0, steps, ws, owned=False, chain=None):
        """dy [T, N, H] -> dgi [T, N, G H] (and dgh where it is a tensor of its own).  d_end: addresses of the gradient rows of
        the state after the last step (None each, or as a whole, for none); d_start: where those of the state before step t0
        go — a later chunk's d_start is the earlier one's d_end.  h0, ws, owned, chain: as launch_fwd."""
        gru = self.own_dgh       # the GRU reads y again and h_{t0-1}; the LSTM c_{t0-1}: the last row either way
        _abi.call(self.bwd[2 if chain else 1 if owned else 0], _prow(dy, t0), *(d_end or [None] * self.state_rows), _p(w_hh),
                  self._start(h0, y, saves, t0)[-1], _prow(masks, t0), *([_prow(y, t0)] if gru else ()), *[_prow(s, t0) for s in saves],
                  steps, y.shape[1], y.shape[2], _prow(dgi, t0), *([_prow(dgh, t0)] if gru else ()), *d_start, _p(ws),
                  *(chain or ()), _stream())

    def final_state(self, y, saves):
        """The state after the last step in habitat's layout, [state_rows, N, H]: y[-1:], or [h; c]."""
        return y[-1:].clone() if self.state_rows == 1 else torch.cat([y[-1:], saves[-1][-1:]])

    def hidden_weight_grads(self, dgh, h0, y, masks):
        """dW_hh = dgh^T (mask * h_prev) over all T N rows; h0: the state before step 0, its h row first."""
        T, N, H = y.shape
        hprev = torch.cat([h0.view(-1, N, H)[:1], y[:-1]], dim=0) * masks.unsqueeze(-1)
        return dgh.view(T * N, -1).t() @ hprev.view(T * N, H)

    def masked(self, gi, w_hh, b_hh, state, masks):
        """The whole sequence in one persistent launch, differentiable: state = the rows before step 0 -> (y [T, N, H], the
        final rows below h [N, H] each; the final h is y[-1])."""
        return _MaskedRNN.apply(self, gi.contiguous(), w_hh.contiguous(), b_hh.contiguous(), masks.contiguous(),
                                *[s.contiguous() for s in state])


GRU = _Cell(3, 1, (1, 1, 1, 1), True, (1, 2), ("wsmg_gru_fwd", "wsmg_gru_fwd_owned", "wsmg_gru_fwd_chain"),
            ("wsmg_gru_bwd", "wsmg_gru_bwd_owned", "wsmg_gru_bwd_chain"), "wsmg_gru_workspace_bytes", "wsmg_gru_chain_workgroups")
LSTM = _Cell(4, 2, (4, 1), False, (32, 64), ("wsmg_lstm_state_fwd", None, "wsmg_lstm_state_fwd_chain"),
             ("wsmg_lstm_state_bwd", None, "wsmg_lstm_state_bwd_chain"), "wsmg_lstm_state_workspace_bytes",
             "wsmg_lstm_state_chain_workgroups")


class _MaskedRNN(torch.autograd.Function):
    """gi [T,N,G H] (input projections), w_hh [G H,H], b_hh [G H], masks [T,N], the state rows [N,H] -> y [T,N,H], final rows below h."""

    @staticmethod
    def forward(ctx, cell, gi, w_hh, b_hh, masks, *state):
        _req(gi, w_hh, b_hh, masks, *state)
        _f32(gi, w_hh, b_hh, masks, *state)
        T, N = gi.shape[:2]
        H = w_hh.shape[1]
        dev = gi.device
        y = torch.empty(T, N, H, device=dev, dtype=torch.float32)
        tail = torch.empty(len(state) - 1, N, H, device=dev, dtype=torch.float32)
        saves = cell.new_saves(T, N, H, dev)
        cell.launch_fwd(gi, w_hh, b_hh, [_p(s) for s in state], masks, y, tail, saves, 0, T, _rnn_workspace(cell.workspace_bytes(T), dev))
        ctx.cell = cell
        ctx.set_materialize_grads(False)
        ctx.save_for_backward(w_hh, masks, y, *state, *saves)
        return (y, *tail.unbind(0))

    @staticmethod
    def backward(ctx, dy, *d_tail):
        cell = ctx.cell
        w_hh, masks, y, *rest = ctx.saved_tensors
        state, saves = rest[:cell.state_rows], rest[cell.state_rows:]
        T, N, H = y.shape
        dev = y.device
        dy = torch.zeros_like(y) if dy is None else dy.contiguous()
        d_tail = [None if d is None else d.contiguous() for d in d_tail]
        dgi = torch.empty(T, N, cell.G * H, device=dev, dtype=torch.float32)
        dgh = torch.empty_like(dgi) if cell.own_dgh else dgi
        d_state = [torch.empty(N, H, device=dev, dtype=torch.float32) for _ in state]
        cell.launch_bwd(dy, [None] + [_p(d) for d in d_tail], w_hh, [_p(s) for s in state], masks, y, saves, dgi, dgh,
                        [_p(d) for d in d_state], 0, T, _rnn_workspace(cell.workspace_bytes(T), dev))
        dw_hh = cell.hidden_weight_grads(dgh, state[0], y, masks)
        db_hh = dgh.view(T * N, -1).sum(dim=0)
        return (None, dgi, dw_hh, db_hh, None, *d_state)


def masked_gru(gi, w_hh, b_hh, h0, masks):
    """Whole-sequence masked GRU in one persistent launch.  Returns y [T,N,H]; final state = y[-1]."""
    return GRU.masked(gi, w_hh, b_hh, (h0,), masks)[0]


def masked_lstm(gi, w_hh, b_hh, h0, c0, masks):
    """Whole-sequence masked LSTM (habitat RNNStateEncoder semantics: h and c times masks[t] before step t) in one persistent
    launch.  Returns (y [T,N,H], c_T [N,H]); the final h = y[-1]."""
    return LSTM.masked(gi, w_hh, b_hh, (h0, c0), masks)


# ----------------------------------------------------------------------------- persistent packed instruction GRU / LSTM
CELLS = {"LSTM": 0, "GRU": 1}        # WSMG_CELL_* of include/wsmgmap.h
INSTR_RNN_SHAPES = ((128, 2), (256, 1))   # (hidden, directions) the kernels take: 256 units in flight


def instr_rnn_supported(cell, hidden, dirs):
    return cell in CELLS and (hidden, dirs) in INSTR_RNN_SHAPES


class _InstrRNN(torch.autograd.Function):
    """gi [U,L,D,G*H], w_hh [D,G*H,H], b_hh [D,G*H], lengths int32 [U] -> out [U,L,D*H]; G = 4 (LSTM) or 3 (GRU)."""

    @staticmethod
    def forward(ctx, gi, w_hh, b_hh, lengths, cell):
        _req(gi, w_hh, b_hh, lengths)
        _f32(gi, w_hh, b_hh)
        U, L, D, GH = gi.shape
        H = w_hh.shape[2]
        code = CELLS[cell]
        dev = gi.device
        out = torch.empty(U, L, D * H, device=dev, dtype=torch.float32)
        sg = torch.zeros(D, U, L, 4, H, device=dev, dtype=torch.float32)
        sc = torch.zeros(D, U, L, H, device=dev, dtype=torch.float32) if cell == "LSTM" else None
        ws = _rnn_workspace(_abi.lib().wsmg_instr_rnn_workspace_bytes(code, H, D, L), dev)
        _abi.call("wsmg_instr_rnn_fwd", code, _p(gi), _p(w_hh), _p(b_hh), _p(lengths), U, L, H, D, _p(out), _p(sg),
                  None if sc is None else _p(sc), _p(ws), _stream())
        ctx.cell = cell
        ctx.save_for_backward(w_hh, lengths, out, sg, sc)
        return out

    @staticmethod
    def backward(ctx, dout):
        w_hh, lengths, out, sg, sc = ctx.saved_tensors
        cell = ctx.cell
        code = CELLS[cell]
        U, L, DH = out.shape
        D, GH, H = w_hh.shape
        dev = out.device
        dout = dout.contiguous()
        dgi = torch.empty(U, L, D, GH, device=dev, dtype=torch.float32)
        dgh = torch.empty_like(dgi) if cell == "GRU" else None
        ws = _rnn_workspace(_abi.lib().wsmg_instr_rnn_workspace_bytes(code, H, D, L), dev)
        _abi.call("wsmg_instr_rnn_bwd", code, _p(dout), _p(w_hh), _p(lengths), _p(out), _p(sg), None if sc is None else _p(sc),
                  U, L, H, D, _p(dgi), None if dgh is None else _p(dgh), _p(ws), _stream())
        zero = torch.zeros(U, 1, H, device=dev, dtype=torch.float32)
        hprev = [torch.cat([zero, out[:, :-1, :H]], dim=1)]               # state before step t (forward direction)
        if D == 2:
            hprev.append(torch.cat([out[:, 1:, H:], zero], dim=1))        # state before step t (reverse direction)
        # one direction's gate gradients as a contiguous [U L, G H] matrix first: on the strided view dgi[:, :, d] (row pitch
        # D G H) the GEMM library picked a 32 x 16 tile kernel that took 340 us for the default encoder's 0.7 GFLOP product
        # (beside the map stack's backward, on the instruction stream)
        dgd = (dgi if dgh is None else dgh).permute(2, 0, 1, 3).contiguous().view(D, U * L, GH)
        dw = torch.stack([dgd[d].t() @ hprev[d].reshape(U * L, H) for d in range(D)])
        from .heads import colsum_multi    # stock sum over (0, 1) of the strided view: 324 us on the instruction stream
        db = torch.stack(colsum_multi([dgd[d] for d in range(D)]))
        return dgi, dw, db, None, None


def instr_rnn(gi, w_hh, b_hh, lengths, cell):
    """Packed instruction GRU / LSTM (hidden 128 x 2 directions or 256 x 1) over <= 8 sequences in one persistent launch."""
    return _InstrRNN.apply(gi.contiguous(), w_hh.contiguous(), b_hh.contiguous(), lengths.contiguous(), cell)


def bilstm(gi, w_hh, b_hh, lengths):
    """The default encoder's packed bidirectional LSTM (hidden 128) over <= 8 sequences: instr_rnn with cell "LSTM"."""
    return instr_rnn(gi, w_hh, b_hh, lengths, "LSTM")
