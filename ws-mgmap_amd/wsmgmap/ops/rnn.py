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


def _rnn_launched():
    pass


class _MaskedGRU(torch.autograd.Function):
    """gi [T,N,3H] (input projections), w_hh [3H,H], b_hh [3H], h0 [N,H], masks [T,N] -> y [T,N,H]."""

    @staticmethod
    def forward(ctx, gi, w_hh, b_hh, h0, masks):
        _req(gi, w_hh, b_hh, h0, masks)
        _f32(gi, w_hh, b_hh, h0, masks)
        T, N, H3 = gi.shape
        H = H3 // 3
        dev = gi.device
        y = torch.empty(T, N, H, device=dev, dtype=torch.float32)
        saves = [torch.empty(T, N, H, device=dev, dtype=torch.float32) for _ in range(4)]
        sync = _rnn_workspace(_abi.lib().wsmg_gru_workspace_bytes(T), dev)
        _abi.call("wsmg_gru_fwd", _p(gi), _p(w_hh), _p(b_hh), _p(h0), _p(masks), T, N, H, _p(y),
                  *[_p(s) for s in saves], _p(sync), _stream())
        _rnn_launched()
        ctx.save_for_backward(w_hh, h0, masks, y, *saves)
        return y

    @staticmethod
    def backward(ctx, dy):
        w_hh, h0, masks, y, sr, sz, sn, sghn = ctx.saved_tensors
        T, N, H = y.shape
        dev = y.device
        dy = dy.contiguous()
        dgi = torch.empty(T, N, 3 * H, device=dev, dtype=torch.float32)
        dgh = torch.empty(T, N, 3 * H, device=dev, dtype=torch.float32)
        dh0 = torch.empty(N, H, device=dev, dtype=torch.float32)
        sync = _rnn_workspace(_abi.lib().wsmg_gru_workspace_bytes(T), dev)
        _abi.call("wsmg_gru_bwd", _p(dy), None, _p(w_hh), _p(h0), _p(masks), _p(y), _p(sr), _p(sz), _p(sn), _p(sghn),
                  T, N, H, _p(dgi), _p(dgh), _p(dh0), _p(sync), _stream())
        _rnn_launched()
        hprev = torch.cat([h0.unsqueeze(0), y[:-1]], dim=0) * masks.unsqueeze(-1)
        g2 = dgh.view(T * N, 3 * H)
        dw_hh = g2.t() @ hprev.view(T * N, H)
        db_hh = g2.sum(dim=0)
        return dgi, dw_hh, db_hh, dh0, None


def masked_gru(gi, w_hh, b_hh, h0, masks):
    """Whole-sequence masked GRU in one persistent launch.  Returns y [T,N,H]; final state = y[-1]."""
    return _MaskedGRU.apply(gi.contiguous(), w_hh.contiguous(), b_hh.contiguous(), h0.contiguous(), masks.contiguous())


class _MaskedLSTM(torch.autograd.Function):
    """gi [T,N,4H] (input projections), w_hh [4H,H], b_hh [4H], h0, c0 [N,H], masks [T,N] -> y [T,N,H], c_T [N,H]."""

    @staticmethod
    def forward(ctx, gi, w_hh, b_hh, h0, c0, masks):
        _req(gi, w_hh, b_hh, h0, c0, masks)
        _f32(gi, w_hh, b_hh, h0, c0, masks)
        T, N, H4 = gi.shape
        H = H4 // 4
        dev = gi.device
        y = torch.empty(T, N, H, device=dev, dtype=torch.float32)
        c_t = torch.empty(N, H, device=dev, dtype=torch.float32)
        sg = torch.empty(T, N, 4 * H, device=dev, dtype=torch.float32)
        sc = torch.empty(T, N, H, device=dev, dtype=torch.float32)
        sync = _rnn_workspace(_abi.lib().wsmg_lstm_state_workspace_bytes(T), dev)
        _abi.call("wsmg_lstm_state_fwd", _p(gi), _p(w_hh), _p(b_hh), _p(h0), _p(c0), _p(masks), T, N, H, _p(y), _p(c_t),
                  _p(sg), _p(sc), _p(sync), _stream())
        _rnn_launched()
        ctx.set_materialize_grads(False)
        ctx.save_for_backward(w_hh, h0, c0, masks, y, sg, sc)
        return y, c_t

    @staticmethod
    def backward(ctx, dy, dc_t):
        w_hh, h0, c0, masks, y, sg, sc = ctx.saved_tensors
        T, N, H = y.shape
        dev = y.device
        dy = torch.zeros_like(y) if dy is None else dy.contiguous()
        dgates = torch.empty(T, N, 4 * H, device=dev, dtype=torch.float32)
        dh0 = torch.empty(N, H, device=dev, dtype=torch.float32)
        dc0 = torch.empty(N, H, device=dev, dtype=torch.float32)
        sync = _rnn_workspace(_abi.lib().wsmg_lstm_state_workspace_bytes(T), dev)
        _abi.call("wsmg_lstm_state_bwd", _p(dy), None, None if dc_t is None else _p(dc_t.contiguous()), _p(w_hh), _p(c0),
                  _p(masks), _p(sg), _p(sc), T, N, H, _p(dgates), _p(dh0), _p(dc0), _p(sync), _stream())
        _rnn_launched()
        hprev = torch.cat([h0.unsqueeze(0), y[:-1]], dim=0) * masks.unsqueeze(-1)
        g2 = dgates.view(T * N, 4 * H)
        dw_hh = g2.t() @ hprev.view(T * N, H)
        db_hh = g2.sum(dim=0)
        return dgates, dw_hh, db_hh, dh0, dc0, None


def masked_lstm(gi, w_hh, b_hh, h0, c0, masks):
    """Whole-sequence masked LSTM (habitat RNNStateEncoder semantics: h and c times masks[t] before step t) in one persistent
    launch.  Returns (y [T,N,H], c_T [N,H]); the final h = y[-1]."""
    return _MaskedLSTM.apply(gi.contiguous(), w_hh.contiguous(), b_hh.contiguous(), h0.contiguous(), c0.contiguous(),
                             masks.contiguous())


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
        _rnn_launched()
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
        _rnn_launched()
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
