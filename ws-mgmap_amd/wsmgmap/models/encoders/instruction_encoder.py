"""Instruction encoder: embedding + packed GRU / LSTM.  State_dict keys and config fields follow the
reference (instruction_encoder.py:10-93).  On the GPU the recurrence of every setting the policy admits
(LSTM or GRU, bidirectional hidden 128 or unidirectional hidden 256) runs as one persistent packed launch
(csrc/wsmg_rnn.hip) instead of ~10 MIOpen launches per token and direction; other shapes take nn.GRU /
nn.LSTM on a packed sequence.

Differences in data flow (results identical):
  * output is token-major [B, L, 256] (what the attention kernel streams), the reference's
    [B, 256, L] is a transpose view of it;
  * identical instructions in a batch (teacher-forcing batches repeat each episode's
    instruction over T time steps) are encoded once and gathered.
"""
import gzip
import json

import os

import torch
import torch.nn as nn


class InstructionEncoder(nn.Module):
    def __init__(self, config):
        super().__init__()
        self.config = config
        if config.use_pretrained_embeddings:
            with gzip.open(config.embedding_file, "rt") as f:
                table = torch.tensor(json.load(f))
            self.embedding_layer = nn.Embedding.from_pretrained(embeddings=table, freeze=not config.fine_tune_embeddings)
        else:
            self.embedding_layer = nn.Embedding(config.vocab_size, config.embedding_size, padding_idx=0)
        cell = nn.GRU if config.rnn_type == "GRU" else nn.LSTM
        self.bidir = config.bidirectional
        self.encoder_rnn = cell(input_size=config.embedding_size, hidden_size=config.hidden_size, bidirectional=self.bidir)
        self.final_state_only = config.final_state_only

    @property
    def output_size(self):
        return self.config.hidden_size * (2 if self.bidir else 1)

    @staticmethod
    def _dedup(tokens):
        """Unique rows of a [B, L] token matrix without a row-wise sort: a 64-bit polynomial hash per
        row, a 1-D unique over the B hashes, and an exact on-device check (a hash collision falls back
        to torch.unique(dim=0)).  Returns (unique rows [U, L], inverse [B], lengths on host, on device)."""
        B, L = tokens.shape
        if tokens.is_cuda and 0 < B <= 4096 and tokens.is_contiguous() and tokens.dtype in (torch.int64, torch.float32):
            return InstructionEncoder._dedup_fused(tokens)
        mult = (torch.arange(1, L + 1, device=tokens.device, dtype=torch.int64) * 0x9E3779B97F4A7C15) | 1
        h = (tokens * mult).sum(dim=1)
        _, inverse = torch.unique(h, return_inverse=True)
        U = int(inverse.max()) + 1 if B else 0  # host sync (the packed LSTM needs host lengths anyway)
        rep = torch.full((U,), B, device=tokens.device, dtype=torch.int64)
        rep.scatter_reduce_(0, inverse, torch.arange(B, device=tokens.device), reduce="amin")
        uniq = tokens[rep]
        lengths = (uniq != 0).long().sum(dim=1)
        exact = (uniq[inverse] == tokens).all().view(1).long()
        host = torch.cat([exact, lengths]).cpu()
        if tokens.is_cuda:
            # the one host read-back of a forward pass: everything queued before it — the previous update's persistent
            # GRU / LSTM launches included — has finished, so their status word (host-mapped memory, no extra sync) is final
            from ... import ops
            ops.check_rnn_status()
        if int(host[0]) != 1:  # hash collision: exact path
            uniq, inverse = torch.unique(tokens, dim=0, return_inverse=True)
            lengths = (uniq != 0).long().sum(dim=1)
            return uniq, inverse, lengths.cpu(), lengths
        return uniq, inverse, host[1:], lengths

    @staticmethod
    def _dedup_fused(tokens):
        """The same result in ONE launch and ONE small read-back (csrc/wsmg_dedup.hip): distinct rows in order of first appearance.
        tokens: int64 or integer-valued float32 [B, L] on the GPU."""
        import ctypes
        from ... import _abi, ops
        B, L = tokens.shape
        dev = tokens.device
        uniq = torch.empty(B, L, device=dev, dtype=torch.int64)
        inverse = torch.empty(B, device=dev, dtype=torch.int64)
        meta = torch.empty(2 + B, device=dev, dtype=torch.int64)
        _abi.call("wsmg_instruction_dedup", ctypes.c_void_p(tokens.data_ptr()), int(tokens.dtype == torch.float32), B, L,
                  ctypes.c_void_p(uniq.data_ptr()), ctypes.c_void_p(inverse.data_ptr()), ctypes.c_void_p(meta.data_ptr()),
                  ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
        host = meta.cpu()        # the one host read-back of a forward pass
        # the persistent kernels' sticky status word: final for everything queued on THIS stream before the read-back — with the
        # dedup on its own early stream the previous update's kernels may still be running, so a timeout can surface one update
        # late here; `BasePolicy.check_status()` / `ops.check_rnn_status(sync=True)` before optimizer.step() is the exact point
        ops.check_rnn_status()
        U = int(host[0])
        return uniq[:U], inverse, host[2:2 + U], meta[2:2 + U]

    _kept = None     # (tokens, dedup of them) of the last rollout-size call

    def dedup(self, instruction, reuse=None):
        """The data-dependent part of the encoder, callable on its own: (unique rows [U, L], inverse [B], lengths on the host,
        lengths on the device).  `wsmgmap.graph.GraphedUpdate` runs it eagerly in front of a captured update and hands the
        result back through `observations["instruction_dedup"]` (U and the longest length fix the shapes the graph was captured
        for).
        reuse (default: without autograd, up to 64 rows — the rollout): the last tokens and their result are kept, and equal
        tokens (one compare + one host read-back) return the kept result: a rollout's instructions change at episode boundaries
        only."""
        tokens = instruction if (instruction.is_cuda and instruction.dtype == torch.float32 and instruction.is_contiguous()) else instruction.long()
        if reuse is None:
            reuse = not torch.is_grad_enabled()
        if not (reuse and tokens.is_cuda and tokens.shape[0] <= 64):
            return self._dedup(tokens)
        kept = self._kept
        if kept is not None and kept[0].shape == tokens.shape and torch.equal(kept[0], tokens):
            from ... import ops
            ops.check_rnn_status()     # (the compare's read-back is this pass's host synchronisation point, as _dedup's is)
            cur = torch.cuda.current_stream()
            for t in kept[1]:
                if t.is_cuda:
                    t.record_stream(cur)
            return kept[1]
        dd = self._dedup(tokens)
        self._kept = (tokens.clone(), dd)
        return dd

    _packed = None

    def _rnn_params(self):
        """(w_ih, b_ih, w_hh, b_hh) of each direction of encoder_rnn, forward direction first."""
        r = self.encoder_rnn
        return [tuple(getattr(r, n + "_l0" + sfx) for n in ("weight_ih", "bias_ih", "weight_hh", "bias_hh"))
                for sfx in (("", "_reverse") if self.bidir else ("",))]

    def _pack(self, per_dir):
        """The directions' parameters as the kernels take them: W_ih / b_ih concatenated, W_hh / b_hh stacked."""
        return (torch.cat([p[0] for p in per_dir], dim=0), torch.cat([p[1] for p in per_dir], dim=0),
                torch.stack([p[2] for p in per_dir]), torch.stack([p[3] for p in per_dir]))

    @torch.no_grad()
    def packed_rnn_weights(self, refresh_only=False):
        """Without autograd: the directions' GRU / LSTM parameters concatenated / stacked as the kernels take them, kept while the
        parameters keep their versions and rewritten IN PLACE otherwise (a captured rollout step reads these addresses;
        MGMapNet.refresh_folded calls this with refresh_only before a replay).  Four launches per step otherwise."""
        if self._packed is None and refresh_only:
            return 0
        per_dir = self._rnn_params()
        src = tuple(p[i] for i in range(4) for p in per_dir)
        ver = tuple(p._version for p in src)
        if self._packed is None:
            self._packed = [None, *self._pack(per_dir)]
        elif self._packed[0] != ver:
            for dst, new in zip(self._packed[1:], self._pack(per_dir)):
                dst.copy_(new)
        elif refresh_only:
            return 0
        self._packed[0] = ver
        return 1 if refresh_only else tuple(self._packed[1:])

    packed_lstm_weights = packed_rnn_weights

    @property
    def kernel_cell(self):
        """"LSTM" / "GRU" if the persistent kernels of csrc/wsmg_rnn.hip take this encoder's shape (hidden 128 x 2 directions
        or 256 x 1), else None (the stock packed route)."""
        from ...ops.rnn import instr_rnn_supported
        cell = "LSTM" if isinstance(self.encoder_rnn, nn.LSTM) else "GRU"
        dirs = 2 if self.bidir else 1
        return cell if instr_rnn_supported(cell, self.encoder_rnn.hidden_size, dirs) and self.encoder_rnn.num_layers == 1 else None

    def encode_unique(self, instruction, stock=False, dedup=None, lstm_after=None):
        """-> (hidden [U, L, D] token-major, pad mask [U, L] bool, inverse [B]) with U unique rows.
        stock=False: persistent HIP GRU / LSTM (csrc/wsmg_rnn.hip) for the shapes they take (`kernel_cell`), the stock route for
        any other; stock=True: nn.GRU / nn.LSTM on a packed sequence (MIOpen / CPU), kept for comparison in tests.  dedup: the result of `dedup()` for these tokens, if the caller
        already has it (no host read-back here then).  lstm_after: an event the persistent GRU / LSTM launches wait for (the
        dedup, the embedding and the input projection do not)."""
        uniq, inverse, len_host, len_dev = self.dedup(instruction) if dedup is None else dedup
        from ...debug import sw
        cell = self.kernel_cell
        if stock or sw.rnn_stock or cell is None or not uniq.is_cuda:
            embedded = self.embedding_layer(uniq)
            packed = nn.utils.rnn.pack_padded_sequence(embedded, len_host, batch_first=True, enforce_sorted=False)
            output, _ = self.encoder_rnn(packed)
            hidden = nn.utils.rnn.pad_packed_sequence(output, batch_first=True)[0]  # [U, L, D]
        else:
            from ... import ops
            lmax = int(len_host.max())
            embedded = self.embedding_layer(uniq[:, :lmax])                     # [U, L, E]
            if torch.is_grad_enabled():
                w_ih, b_ih, w_hh, b_hh = self._pack(self._rnn_params())    # [D*G*H, E], [D*G*H], [D, G*H, H], [D, G*H]
            else:
                w_ih, b_ih, w_hh, b_hh = self.packed_rnn_weights()
            U = uniq.shape[0]
            gi = torch.addmm(b_ih, embedded.reshape(U * lmax, -1), w_ih.t()).view(U, lmax, w_hh.shape[0], -1)
            lens = len_dev.to(torch.int32)
            if lstm_after is not None:
                torch.cuda.current_stream().wait_event(lstm_after)
            parts = [ops.instr_rnn(gi[c:c + 8], w_hh, b_hh, lens[c:c + 8], cell) for c in range(0, U, 8)]
            hidden = parts[0] if len(parts) == 1 else torch.cat(parts, dim=0)
        mask = (hidden == 0.0).all(dim=2)
        return hidden.contiguous(), mask, inverse

    def forward(self, observations):
        """Reference-shaped result: ([B, D, L], mask [B, L])."""
        hidden, mask, inverse = self.encode_unique(observations["instruction"], stock=not observations["instruction"].is_cuda)
        return hidden[inverse].permute(0, 2, 1), mask[inverse]
