"""The recurrent core of the update path as ONE autograd node, software-pipelined over time chunks.

Reference: MGMapNet.forward, vlnce_baselines/models/mg_map_policy.py:220-249 —

    state           = state_encoder(state_in, h[0], masks)                       # recurrence 1, T serial steps
    text_embedding  = _attn(state_text_q_layer(state), text_k, text_v, text_mask) # per row
    map_embedding   = _attn(text_map_q_layer(text_embedding), map_k, map_v)       # per row
    x               = second_state_compress(cat(state, text_embedding, map_embedding))
    x               = second_state_encoder(x, h[1], masks)                        # recurrence 2, T serial steps

Only the two state encoders are recurrent — GRUs by default, LSTMs with MODEL.STATE_ENCODER.rnn_type = "LSTM" (both encoders share
the type; the cell is described once in ops/rnn.py: ops.GRU / ops.LSTM) — and everything between them, the attention STAGE, is per
ROW.  Run stage after stage the update's critical path holds 2 x T dependent steps forward and 2 x T backward (4 x 64 steps of
5.6-6.0 us = 1.5 ms with 224 of the 256 CUs idle) plus ~60 dependent small launches around them.  Here the T steps are cut into K
chunks: while recurrence 1 runs chunk k+1 on one stream, the stage of chunk k runs on a second and recurrence 2 of chunk k on a third
(the carried hidden state is bit-exact across split launches: tests/test_gpu_kernels.py::test_fullsize_gru_sequence_split_cfg2),
and the reverse order in backward: T + T/K serial steps each way instead of 2 T.

The schedule is written once for both directions (_pipeline: it alone knows how chunks are ordered — an event per chunk and edge, or
whole-sequence launches chained through _ChainCounters — and the one-stream case); the stage's dense layers come in two forms, each
a "chunk forward / chunk backward" pair over one namespace of named buffers, chosen once per call (_RowsStage, _LibStage).

Weight and bias gradients are NOT part of the chain: the backward chain only produces activation gradients into full-batch
buffers, and every parameter gradient is one full-batch GEMM / column sum on a "leaf" stream that joins the main stream when the
whole backward pass ends (nothing but the optimizer waits for them).

Arithmetic: the same kernels and the same float32 GEMMs as the staged route, row for row; chunking changes no reduction order
inside a row except where the GEMM library picks another kernel for 128 rows than for 512 (float32 rounding differences, <= 1e-6
relative; tests/test_gpu_round4.py holds the block against the staged route)."""
import contextlib
import ctypes
import functools
from types import SimpleNamespace

import torch

from . import _abi
from . import ops as _ops
from .ops import core as _core
from .debug import sw as _sw
from .ops import _join_side_at_end, _p, _prow, _rnn_workspace, _sfx, _stream

MAX_BATCH = 8          # batch slots of the persistent state-encoder kernels (GRU and LSTM)


_owned = {}      # (device index, role, stream handle) -> [workspace, bytes, timeouts seen]: the GRU chunk launches' persistent exchange images


def _owned_ws(dev, role, nbytes):
    """A zeroed workspace that only this role's launches ON THE CURRENT STREAM ever use (wsmg_gru_*_owned: no clear per launch).
    One per (role, stream) — GRU 1 / GRU 2, forward / backward: launches of one role follow each other on one stream, launches of
    different roles overlap; a second policy or a caller on another stream gets an image of its own.  A workspace
    that is outgrown is told which stream may still be using it before it is dropped."""
    sid = torch.cuda.current_stream(dev).cuda_stream
    key = (dev.index, role, sid)
    e = _owned.get(key)
    if e is None or e[1] < nbytes or e[2] != _abi.rnn_timeouts:
        if e is not None:
            e[0].record_stream(torch.cuda.current_stream(dev))
        e = _owned[key] = [torch.zeros((int(nbytes) + 3) // 4, device=dev, dtype=torch.float32), int(nbytes), _abi.rnn_timeouts]
    return e[0]


_hooks_probe = None


def _post_hooks_visible():
    """Does this torch keep `register_post_accumulate_grad_hook` hooks in the private dict the multi-stream backward runs by hand
    (`Tensor._post_accumulate_grad_hooks`)?  Probed once on a scratch tensor; if a torch version moves it, the block stays on the
    one-stream route (gradients through AccumulateGrad) instead of silently skipping the reducer's hooks."""
    global _hooks_probe
    if _hooks_probe is None:
        try:
            t = torch.zeros(1, requires_grad=True)
            seen = []
            h = t.register_post_accumulate_grad_hook(seen.append)
            d = getattr(t, "_post_accumulate_grad_hooks", None)
            _hooks_probe = bool(d) and len(d) == 1
            for f in list((d or {}).values()):
                f(t)
            _hooks_probe = _hooks_probe and len(seen) == 1
            h.remove()
        except Exception:
            _hooks_probe = False
    return _hooks_probe


def _rg(a_segs, w, w_is_kn, out_segs, r0, M, bias=None, cin_segs=None, mask=None, relu=False, wait=None, signal=None, fail_bit=1):
    """One launch of wsmg_rows_gemm_f32 on rows r0 .. r0 + M of full-batch row-major tensors: C = epilogue([A0|A1|A2] W^T) (w_is_kn
    False: W an nn.Linear weight [N, K]) or ([A0|A1|A2] W) (True: W [K, N], the backward product dY W).  a_segs / out_segs /
    cin_segs: lists of up to three 2-D tensors (their column counts are the segment widths); mask: the ReLU-backward mask source.
    wait = (counter address, target, gate word address): the product waits for the counter before reading (operands produced by a
    chained GRU launch that is still running), through a one-workgroup gate launch that reports in the gate word — a word of the
    caller's per-pass counter tensor, one per chunk; signal = counter address: every workgroup adds an arrival when its tile is stored."""
    z = (None, 0, 0)
    A = [(_prow(t, r0), t.stride(0), t.shape[1]) for t in a_segs] + [z] * (3 - len(a_segs))
    Cs = [(_prow(t, r0), t.stride(0), t.shape[1]) for t in out_segs] + [z] * (3 - len(out_segs))
    Ci = [(_prow(t, r0), t.stride(0)) for t in (cin_segs or [])] + [(None, 0)] * (3 - len(cin_segs or []))
    _abi.call("wsmg_rows_gemm_f32", *A[0], *A[1], *A[2], _p(w), w.stride(0), int(bool(w_is_kn)), _p(bias),
              None if mask is None else _prow(mask, r0), 0 if mask is None else mask.stride(0), int(bool(relu)),
              *Cs[0], *Cs[1], *Cs[2], *Ci[0], *Ci[1], *Ci[2], int(M),
              None if wait is None else ctypes.c_void_p(wait[0]), 0 if wait is None else int(wait[1]),
              None if signal is None else ctypes.c_void_p(signal), int(fail_bit),
              None if wait is None else ctypes.c_void_p(wait[2]), _stream())


def rows_gemm_ok(H, C, in1, G):
    """Shapes wsmg_rows_gemm_f32 takes for the attention stage's products (hidden size H, attention width C, GRU-2 input, G gate rows
    per unit of the second recurrence): every product's reduction length is asked of the library (a multiple of 256
    alone admitted K = 1280, which it refuses)."""
    if not (_sw.rows_gemm and H % 256 == 0 and C % 256 == 0 and in1 % 256 == 0):
        return False
    ok = _abi.lib().wsmg_rows_gemm_supported
    # forward: q1 (K = H), q2 / qf (C), compress (H + 2 C), gi2 (in1); backward: dxc (G H), its split (in1), the queries (C, H)
    return all(ok(int(k)) for k in (H, C, H + 2 * C, in1, G * H))


def core_cell(net):
    """The cell the pipelined core runs for this policy's state encoders: "GRU", "LSTM" when both encoders run the persistent LSTM
    kernels (hidden 512, not the stock route), or None: the staged route (an LSTM of another size, or on the stock route)."""
    from .models.rnn_state_encoder import KERNEL_HIDDEN
    encs = [getattr(net, n, None) for n in ("state_encoder", "second_state_encoder")]
    lstm = [bool(getattr(e, "_is_lstm", False)) for e in encs]
    if not any(lstm):
        return "GRU"
    if all(lstm) and not _sw.rnn_stock and all(e.rnn.hidden_size == KERNEL_HIDDEN for e in encs):
        return "LSTM"
    return None


def _roles(streams, main):
    """(attention stream, GRU-2 stream, leaf stream) out of the caller's helper streams.  The block creates NO stream of its own: HIP
    multiplexes a process's streams onto 4 hardware queues, and two streams that share a queue run their work in submission order
    — with three private streams on top of the policy's (instruction branch, decoder branch) the attention stage of chunk k+1
    queued behind GRU 2 of chunk k (measured: 200 us per chunk instead of 117).  The policy's two helper streams are idle while
    this block runs, in both directions, so they are what it uses.  The attention stream is the instruction branch's — the stream
    that branch's backward, the consumer of the shared sets' gradients, runs on — and the leaf work goes behind the attention
    stage's last chunk on the same stream (measured against the decoder branch's stream, three interleaved pairs of 100 updates on
    one box: median 10.52-10.54 vs 10.73-10.74 ms per update)."""
    streams = [s for s in (streams or ()) if s is not None and s.cuda_stream != main.cuda_stream]
    if not streams:
        return main, main, main
    sa = streams[0]
    sg = streams[1] if len(streams) > 1 else streams[0]
    return sa, sg, sa


def usable(state_in, tokens, n_env, text, capturing_ok=True, text_attention="f32"):
    """Can the pipelined block take this call?  Training-size sequences (more than one step) of at most 8 environments on the GPU,
    float32 state / text tensors, map tokens [B, I, 256], the float32 instruction attention (MODEL.TEXT_ATTENTION = "fp8" is not
    wired into the block: the update takes the staged route)."""
    B = state_in.shape[0]
    return (text_attention == "f32" and state_in.is_cuda and state_in.dtype == torch.float32 and n_env <= MAX_BATCH and B % n_env == 0 and B // n_env > 1
            and tokens.dim() == 3 and tokens.shape[2] == 256 and all(t.dtype in (torch.float32, torch.bfloat16) for t in text[:2]))


def chunk_plan(T, want):
    """Time steps per chunk: `want` chunks of equal length when T divides, else the largest divisor count below it (chunks of
    unequal length would only complicate the plan: T = 64 in the bench, DAgger batches are padded to their longest episode)."""
    k = max(1, min(int(want), T))
    while T % k:
        k -= 1
    return k, T // k


class _ChainCounters:
    """The device-side counters of one chained pass: 3 K int32 words zeroed on the current stream, [arrivals in | arrivals out | gate
    words] per chunk.  The producing recurrence adds `in_target` arrivals to word k when chunk k's outputs are complete; the stage's
    first product of chunk k waits for them (its gate launch reports in word 2 K + k) and its last product's workgroups add
    `out_target` arrivals to word K + k, which the consuming recurrence waits for at the first step of chunk k (csrc/wsmg_rnn.hip
    chain_wait / chain_signal).  No other code computes an address into the tensor: one wrong by a word is a missed wait."""

    def __init__(self, K, dev, in_target, out_target):
        self.words = torch.zeros(3 * K, device=dev, dtype=torch.int32)
        self.K, self.base, self.in_target = K, self.words.data_ptr(), int(in_target)
        self.head = (None, 0, ctypes.c_void_p(self.base))      # (in counters, in target, out counters) of the producer's whole-sequence launch
        self.tail = (ctypes.c_void_p(self.base + 4 * K), int(out_target), None)      # ... and of the consumer's

    def wait(self, k):        # `wait` of the stage's first product of chunk k (see _rg): producer chunk k's counter, its target, the gate word
        return self.base + 4 * k, self.in_target, self.base + 4 * (2 * self.K + k)

    def signal(self, k):      # `signal` of its last product
        return self.base + 4 * (self.K + k)


def _workspaces(cell, entry, dev, T, Tc):
    """The workspaces of one pass's recurrence launches (entry: cell.fwd or cell.bwd) -> (owned, own_chunks, pick); pick(role, whole):
    the workspace for a launch of `role` on the current stream, of a chunk or (chained) of the whole sequence.  Launches run on
    workspaces this module owns (no clear in front of every launch); a HIP-graph capture bakes the launch-unique tags in, so replays
    need the clearing form."""
    owned = not torch.cuda.is_current_stream_capturing()
    own_chunks = owned and entry[1] is not None      # (no owned LSTM form: its chunk launches clear a fresh workspace)
    nbytes = cell.workspace_bytes(Tc)

    def pick(role, whole):
        if whole or own_chunks:
            return _owned_ws(dev, role, cell.workspace_bytes(T) if whole else nbytes)
        return _rnn_workspace(nbytes, dev)
    return owned, own_chunks, pick


class _Stage:
    """The attention stage on rows k * rows .. (k + 1) * rows of the full-batch buffers `b` (a namespace: the forward's buffers; in
    backward what it saved and the gradient buffers).  The two attention kernels are here, the dense layers around them in the
    subclasses' fwd / bwd (k, wait, signal): wait / signal as _rg takes them, None unless chained (`chainable` forms only)."""
    chainable = False

    def __init__(self, b, rows, fail_bit):
        self.b, self.rows, self.fail_bit = b, rows, fail_bit    # (the status bit a chained product's wait reports: the recurrence it waits for)
        self.tsfx, self.ksfx, self.L, self.I, self.C = _sfx(b.text_k), _sfx(b.tokens), b.text_k.shape[1], b.tokens.shape[1], b.tokens.shape[2]

    def alloc_fwd(self):
        pass

    alloc_bwd = begin_fwd = alloc_fwd

    def text_fwd(self, r0):
        b = self.b
        _abi.call("wsmg_attn_shared_fwd" + self.tsfx, _prow(b.q1, r0), _p(b.text_k), _p(b.text_v), _p(b.text_mask), _prow(b.inverse, r0),
                  b.scale, self.rows, self.L, self.C, _prow(b.text_emb, r0), _prow(b.attn_text, r0), _stream())

    def map_fwd(self, r0):
        b = self.b
        _abi.call("wsmg_attn_fwd" + self.ksfx, _prow(b.qf, r0), _prow(b.tokens, r0), _prow(b.tokens, r0), None, b.scale, self.rows, self.I,
                  self.C, _prow(b.map_emb, r0), _prow(b.att_map, r0), _stream())

    def map_bwd(self, r0, dmap):
        b = self.b
        _abi.call("wsmg_attn_bwd" + self.ksfx, _prow(b.qf, r0), _prow(b.tokens, r0), _prow(b.tokens, r0), _prow(b.att_map, r0), dmap,
                  None if b.datt is None else _prow(b.datt, r0), b.scale, self.rows, self.I, self.C, _prow(b.dqf, r0), _prow(b.dtokens, r0),
                  _prow(b.dtokens, r0), _stream())

    def text_bwd(self, r0):
        b = self.b
        _abi.call("wsmg_attn_shared_bwd" + self.tsfx, _prow(b.q1, r0), _p(b.text_k), _p(b.text_v), _prow(b.attn_text, r0), _prow(b.dtext, r0),
                  None, _prow(b.inverse, r0), b.scale, self.rows, self.L, self.C, _prow(b.dq1, r0), _prow(b.dl, r0), _stream())


class _RowsStage(_Stage):
    """Every dense layer of the stage is ONE launch (csrc/wsmg_rows_gemm.hip): bias, the concatenation, the ReLU and its mask, the
    split of d(cat) into its three parts and the accumulate-intos (beta = 1, in place) ride in the epilogues / operand segments —
    7 launches per chunk forward and backward instead of 9 + 4 pre-fills / 9 + a threshold_backward, each ~4 us."""
    chainable = True
    saves = ("map_emb",)

    def alloc_bwd(self):
        self.b.dmap_all = torch.empty_like(self.b.dtext)

    def fwd(self, k, wait, signal):
        b, M, r0 = self.b, self.rows, k * self.rows
        _rg([b.y1r], b.wq1, False, [b.q1], r0, M, bias=b.bq1, wait=wait, fail_bit=self.fail_bit)
        self.text_fwd(r0)
        _rg([b.text_emb], b.wq2, False, [b.q2], r0, M, bias=b.bq2)
        _rg([b.q2], b.wk2, True, [b.qf], r0, M)
        self.map_fwd(r0)
        _rg([b.y1r, b.text_emb, b.map_emb], b.wc, False, [b.xc], r0, M, bias=b.bc, relu=True)
        _rg([b.xc], b.w_ih2, False, [b.gi2], r0, M, bias=b.b_ih2, signal=signal)

    def bwd(self, k, wait, signal):
        b, M, r0 = self.b, self.rows, k * self.rows
        _rg([b.dgi2r], b.w_ih2, True, [b.dxc], r0, M, mask=b.xc, wait=wait, fail_bit=self.fail_bit)
        _rg([b.dxc], b.wc, True, [b.dstate_r, b.dtext, b.dmap_all], r0, M)
        self.map_bwd(r0, _prow(b.dmap_all, r0))
        _rg([b.dqf], b.wk2, False, [b.dq2], r0, M)
        _rg([b.dq2], b.wq2, True, [b.dtext], r0, M, cin_segs=[b.dtext])
        self.text_bwd(r0)
        _rg([b.dq1], b.wq1, True, [b.dstate_r], r0, M, cin_segs=[b.dstate_r], signal=signal)

    def concat(self):      # cat(state, text_embedding, map_embedding) for dW of second_state_compress: only ever operand segments here
        return torch.cat([self.b.y1r, self.b.text_emb, self.b.map_emb], dim=1)


class _LibStage(_Stage):
    """The dense layers on the GEMM library.  Projection outputs start as their bias rows and are accumulated into: `addmm` with a 1-D
    bias takes hipBLASLt's bias-epilogue route, whose heuristic picks ONE 256 x 128 macro-tile for a 128-row chunk — 64 us for a
    33-MFLOP product."""
    saves = ("x",)

    def alloc_fwd(self):
        self.b.x = torch.empty(self.b.y1r.shape[0], self.b.wc.shape[1], device=self.b.xc.device, dtype=torch.float32)

    def begin_fwd(self):
        for out, bias in ((self.b.q1, self.b.bq1), (self.b.q2, self.b.bq2), (self.b.xc, self.b.bc), (self.b.gi2, self.b.b_ih2)):
            out.copy_(bias.expand_as(out))

    def alloc_bwd(self):
        self.wc_parts, self.wk2t = self.b.wc.split((self.b.y1r.shape[1], self.C, self.C), dim=1), self.b.wk2.t()

    def fwd(self, k, wait, signal):
        b, r0, r1 = self.b, k * self.rows, (k + 1) * self.rows
        b.q1[r0:r1].addmm_(b.y1r[r0:r1], b.wq1.t())
        self.text_fwd(r0)
        b.q2[r0:r1].addmm_(b.text_emb[r0:r1], b.wq2.t())
        torch.mm(b.q2[r0:r1], b.wk2, out=b.qf[r0:r1])
        self.map_fwd(r0)
        torch.cat([b.y1r[r0:r1], b.text_emb[r0:r1], b.map_emb[r0:r1]], dim=1, out=b.x[r0:r1])
        b.xc[r0:r1].addmm_(b.x[r0:r1], b.wc.t())
        torch.relu_(b.xc[r0:r1])
        b.gi2[r0:r1].addmm_(b.xc[r0:r1], b.w_ih2.t())

    def bwd(self, k, wait, signal):
        b, r0, r1 = self.b, k * self.rows, (k + 1) * self.rows
        # ReLU of second_state_compress: d(pre-activation) = d(xc) where xc > 0
        dxc_k, dq2_k = b.dxc[r0:r1], b.dq2[r0:r1]
        torch.ops.aten.threshold_backward.grad_input(torch.mm(b.dgi2r[r0:r1], b.w_ih2), b.xc[r0:r1], 0.0, grad_input=dxc_k)
        dstate_a, dtext_a, dmap = [torch.mm(dxc_k, w) for w in self.wc_parts]
        self.map_bwd(r0, _p(dmap))
        torch.mm(b.dqf[r0:r1], self.wk2t, out=dq2_k)
        torch.addmm(dtext_a, dq2_k, b.wq2, out=b.dtext[r0:r1])
        self.text_bwd(r0)
        torch.addmm(dstate_a, b.dq1[r0:r1], b.wq1, out=b.dstate_r[r0:r1])

    def concat(self):
        return self.b.x


def _pipeline(names, main, streams, order, chain, dev, producer, stage, consumer, begin=None):
    """Enqueues "producer recurrence -> stage chunks -> consumer recurrence" over the chunks `order` (ascending in forward, descending
    in backward) on streams = (producer's, stage's, consumer's); names: their `_ops.mark` names.  producer / consumer (k, link=None)
    launch chunk k or, with a chain link, the whole sequence; stage (k, wait, signal); begin: runs on the stage's stream in front of
    its chunks.  Chunk k of each waits for chunk k of the one before it: through one event per chunk and edge, or, with chain =
    (arrivals per chunk of a recurrence launch, of the stage's last product), on the device — each recurrence is ONE whole-sequence
    launch that waits on _ChainCounters: no chunk prologues (W_hh into registers: ~10 us, 16 times per update), no launch gaps, no
    events; a waiter is enqueued after its producers.  With the stage on `main` (K = 1) there is one stream and nothing to order.
    The side streams fork from `main` once, behind what is queued on it so far (the buffers' earlier users, the counters' zeroing);
    joining them is the caller's.  Enqueue order: stream by stream — the dependencies are events or counters, so the GPU sees the
    same pipeline as with a chunk-by-chunk order, and the host changes its current stream twice instead of eight times (it has
    < 1.5 ms of lead over the GPU in this part of an update).  -> the counter tensor (the caller keeps it alive) or None."""
    multi = streams[1] is not main
    cnt = _ChainCounters(len(order), dev, *chain) if chain else None
    if multi:
        # ONE event record on `main` (stream.wait_stream(main) records one per call, and a record between two dependent kernels costs
        # the recording stream ~3 us: tools/exp/event_cost.hip)
        e = torch.cuda.Event()
        e.record(main)
        for st in streams:
            if st is not main:
                st.wait_event(e)
    evented = multi and cnt is None

    def run(st, name, launch, waits=None, record=False, link=None, first=None):
        done = {}
        with (contextlib.nullcontext() if st is main else torch.cuda.stream(st)):
            if first:
                first()
            if link:
                launch(0, link)
                _ops.mark(name)
                return done
            for k in order:
                if waits:
                    st.wait_event(waits[k])
                launch(k)
                _ops.mark("%s.%d" % (name, k))
                if record:
                    done[k] = torch.cuda.Event()
                    done[k].record(st)
        return done

    ev = run(streams[0], names[0], producer, record=evented, link=cnt and cnt.head)
    chunk = (lambda k: stage(k, cnt.wait(k), cnt.signal(k))) if cnt else (lambda k: stage(k, None, None))
    ev = run(streams[1], names[1], chunk, ev, evented, first=begin)
    run(streams[2], names[2], consumer, ev, link=cnt and cnt.tail)
    return cnt and cnt.words


_SAVED = ("state_in", "tokens", "text_k", "text_v", "inverse", "m", "h01", "h02", "w_ih1", "w_hh1", "wq1", "wq2", "wk2", "wc", "w_ih2", "w_hh2",
          "gi1", "y1", "sv1", "y2", "sv2", "q1", "text_emb", "attn_text", "q2", "qf", "att_map", "xc")


def _save(ctx, b, names):
    """save_for_backward of the named buffers of `b`, a list (sv1, sv2) item by item -> the layout `_load` names them by again."""
    vals = [getattr(b, n) for n in names]
    ctx.save_for_backward(*[t for v in vals for t in (v if isinstance(v, list) else [v])])
    return [(n, len(v) if isinstance(v, list) else None) for n, v in zip(names, vals)]


def _load(ctx, layout):
    it = iter(ctx.saved_tensors)
    return SimpleNamespace(**{n: next(it) if c is None else [next(it) for _ in range(c)] for n, c in layout})


class _RecurrentBlock(torch.autograd.Function):
    @staticmethod
    def forward(ctx, cfg, state_in, tokens, text_k, text_v, text_mask, inverse, masks, h01, h02,
                w_ih1, b_ih1, w_hh1, b_hh1, wq1, bq1, wq2, bq2, wk, bk, wc, bc, w_ih2, b_ih2, w_hh2, b_hh2):
        N, scale, text_ev, cell = cfg["N"], cfg["scale"], cfg["text_ready"], cfg["cell"]   # cell: ops.GRU or ops.LSTM (ops/rnn.py)
        B, H, G, dev = state_in.shape[0], w_hh1.shape[1], cell.G, state_in.device
        T = B // N
        assert w_hh1.shape[0] == G * H and w_hh2.shape[0] == G * H
        K, Tc = chunk_plan(T, cfg["chunks"])
        main = torch.cuda.current_stream()
        sa, sg, _ = _roles(cfg["streams"] if K > 1 else None, main)
        multi = sa is not main
        K, Tc = (K, Tc) if multi else (1, T)
        rows = Tc * N
        I, C, L = tokens.shape[1], tokens.shape[2], text_k.shape[1]
        E = functools.partial(torch.empty, device=dev, dtype=torch.float32)
        # full-batch buffers (main stream's pool; every other stream is joined into main before this function returns, and they
        # live on as saved tensors until the backward pass).  h01 / h02 are copies: the caller overwrites rnn_hidden_states in place
        # (reference contract); an LSTM's is [h; c]
        b = SimpleNamespace(
            state_in=state_in, tokens=tokens, text_k=text_k, text_v=text_v, text_mask=text_mask, inverse=inverse, m=masks.reshape(T, N),
            scale=scale, w_ih1=w_ih1, w_hh1=w_hh1, wq1=wq1, bq1=bq1, wq2=wq2, bq2=bq2, wk2=wk.reshape(wk.shape[0], -1), wc=wc, bc=bc,
            w_ih2=w_ih2, b_ih2=b_ih2, w_hh2=w_hh2, gi1=torch.addmm(b_ih1, state_in, w_ih1.t()), y1=E(T, N, H), y2=E(T, N, H),
            sv1=cell.new_saves(T, N, H, dev), sv2=cell.new_saves(T, N, H, dev), q1=E(B, wq1.shape[0]), text_emb=E(B, C),
            attn_text=E(B, L), q2=E(B, wq2.shape[0]), qf=E(B, C), map_emb=E(B, C), att_map=E(B, I), xc=E(B, wc.shape[0]), gi2=E(B, G * H),
            h01=h01.clone(), h02=h02.clone())
        b.y1r = b.y1.view(B, H)
        # the kernels' outputs of the final rows below h (an LSTM's c_T: the final c is save_c[T - 1] as well), one per recurrence
        tails = [E(cell.state_rows - 1, N, H) for _ in range(2)]
        form = _RowsStage if rows_gemm_ok(H, C, wc.shape[0], G) and wq1.shape[0] % 256 == 0 and wq2.shape[0] % 256 == 0 else _LibStage
        stage = form(b, rows, cell.fwd_bit)
        stage.alloc_fwd()
        # (wsmgmap.parallel holds its buckets until this block's backward has queued its kernels: see _launch_ready there)
        _core.chain_in_flight = bool(multi and any(ctx.needs_input_grad))
        if text_ev is not None:
            sa.wait_event(text_ev)
        owned, own_chunks, ws = _workspaces(cell, cell.fwd, dev, T, Tc)

        def rnn(gi, w_hh, b_hh, h0, y, sv, tail, role, k, link=None):
            # chunk k of a recurrence (it starts from what step k Tc - 1 left), or, with a chain link, the whole sequence
            cell.launch_fwd(gi, w_hh, b_hh, cell.rows(h0), b.m, y, tail, sv, k * Tc, T if link else Tc, ws(role, link),
                            own_chunks, link and (Tc, *link))

        chain = multi and stage.chainable and owned and _sw.recurrent_chain and K > 1
        _pipeline(("f.g1", "f.at", "f.g2"), main, (main, sa, sg), range(K),
                  chain and (cell.chain_workgroups(), _abi.lib().wsmg_rows_gemm_workgroups(rows, G * H)), dev,
                  functools.partial(rnn, b.gi1.view(T, N, G * H), w_hh1, b_hh1, b.h01, b.y1, b.sv1, tails[0], "f1"), stage.fwd,
                  functools.partial(rnn, b.gi2.view(T, N, G * H), w_hh2, b_hh2, b.h02, b.y2, b.sv2, tails[1], "f2"), stage.begin_fwd)
        if multi:
            main.wait_stream(sg)
            main.wait_stream(sa)
        ctx.form, ctx.chain, ctx.cell, ctx.layout = form, chain, cell, _save(ctx, b, _SAVED + form.saves)
        ctx.cfg, ctx.streams = (N, K, Tc, scale, cfg["sink"], tuple(wk.shape)), cfg["streams"]
        ctx.params = (w_ih1, b_ih1, w_hh1, b_hh1, wq1, bq1, wq2, bq2, wk, bk, wc, bc, w_ih2, b_ih2, w_hh2, b_hh2)
        h1n, h2n = cell.final_state(b.y1, b.sv1), cell.final_state(b.y2, b.sv2)      # habitat's layout: [h] or [h; c]
        ctx.mark_non_differentiable(h1n, h2n)
        ctx.set_materialize_grads(False)
        return b.y2.view(B, H), b.att_map, h1n, h2n

    @staticmethod
    def backward(ctx, dy2, datt, _dh1, _dh2):
        cell, params, b = ctx.cell, ctx.params, _load(ctx, ctx.layout)
        N, K, Tc, b.scale, sink, wk_shape = ctx.cfg
        T, _, H = b.y1.shape
        G, B, dev, U = cell.G, T * N, b.y1.device, b.text_k.shape[0]
        main = torch.cuda.current_stream()
        # Side streams only when this pass SETS the gradients of leaf parameters that nothing but this block uses: the parameter gradients are
        # produced on the leaf stream, so they must not pass through autograd's AccumulateGrad — it runs on the main stream right after this function
        # returns and, whenever it does not simply keep the tensor (an existing .grad to add to; a tensor it decides to copy), launches a kernel there
        # that reads a gradient the leaf stream has not written yet (seen as one wrong weight gradient in 8 runs of two ranks sharing a GPU)..  In that
        # mode this function ASSIGNS p.grad itself, runs the parameters' post-accumulate hooks (wsmgmap.parallel.GradAllReducer's bucket hooks) and
        # returns None for them. A stock DistributedDataParallel wrap hooks the AccumulateGrad nodes instead: there the block stays on one stream.
        own = [p for p in params if p is not None and p.requires_grad]
        # (a parameter with a tensor hook — `register_hook`, which AccumulateGrad's input would have run — keeps the one-stream,
        #  through-autograd form: assigning .grad here would silently skip it.  These parameters have no consumer outside this
        #  block — `is_leaf and grad is None` at entry is the whole contract: nothing else can add to them in this pass)
        multi = (K > 1 and _post_hooks_visible()
                 and all(p.is_leaf and p.grad is None and not getattr(p, "_backward_hooks", None) for p in own))
        if multi and torch.distributed.is_available() and torch.distributed.is_initialized():
            multi = all(getattr(p, "_wsmg_reducer", False) for p in own)
        sa, sg, sl = _roles(ctx.streams if multi else None, main)
        multi = sa is not main
        if multi:
            try:
                _join_side_at_end(main, sl, strict=True)      # raises outside a backward pass (torch.autograd.grad of a test)
                if sl not in _ops._leaf_streams:              # (ops.reset_pass_state re-joins it if a pass died before its callbacks)
                    _ops._leaf_streams.append(sl)
            except RuntimeError:
                multi = False
        if not multi:
            sa = sg = sl = main
            K, Tc = 1, T
        rows = Tc * N
        E = functools.partial(torch.empty, device=dev, dtype=torch.float32)
        # full-batch gradient buffers (an LSTM's one gate gradient is both the gradient of gi and of W_hh h + b_hh: dgh is dgi; its state gradients are [dh; dc])
        b.dy2 = torch.zeros(T, N, H, device=dev, dtype=torch.float32) if dy2 is None else dy2.contiguous().float().view(T, N, H)
        b.datt = None if datt is None else datt.contiguous().float()
        b.dgi2, b.dgi1 = E(T, N, G * H), E(T, N, G * H)
        b.dgh2, b.dgh1 = (torch.empty_like(b.dgi2), torch.empty_like(b.dgi1)) if cell.own_dgh else (b.dgi2, b.dgi1)
        b.dxc, b.dqf, b.dq2, b.dq1 = E(B, b.wc.shape[0]), E(B, b.qf.shape[1]), E(B, b.wq2.shape[0]), E(B, b.wq1.shape[0])
        b.dtext, b.dl, b.dstate, b.dtokens = E(B, b.qf.shape[1]), E(B, b.text_k.shape[1]), E(T, N, H), torch.empty_like(b.tokens)
        b.dh01, b.dh02 = E(*b.h01.shape), E(*b.h02.shape)
        b.carry2, b.carry1 = [E(*b.h02.shape) for _ in range(2)], [E(*b.h01.shape) for _ in range(2)]
        b.y1r, b.dstate_r, b.dgi2r = b.y1.view(B, H), b.dstate.view(B, H), b.dgi2.view(B, G * H)
        stage = ctx.form(b, rows, cell.bwd_bit)
        stage.alloc_bwd()
        if multi:
            # the buffers are allocated from the main stream's pool and used on the others: they must not be handed to a later main-stream allocation
            # while a side stream still works on them — a reference is held until the pass's final callbacks, which run after the leaf stream has been
            # joined into main (cheaper than ~50 record_stream calls, and legal under graph capture) — and so do the tensors SAVED by the forward
            # pass: autograd drops them the moment this function returns, long before the leaf stream's GEMMs have read x, xc, q2, text_emb, y1, y2,
            # ... (seen as one wrong weight gradient in ~8 runs of two ranks sharing a GPU, where the leaf stream starts late)..  `b` names them all
            # (and the chain's counters, below)
            keep = [b]
            torch.autograd.Variable._execution_engine.queue_callback(keep.clear)
        owned, own_chunks, ws = _workspaces(cell, cell.bwd, dev, T, Tc)

        def rnn_bwd(dy, w_hh, h0, y, sv, dgi, dgh, dh0_out, carry, role, k, link=None):
            # as `rnn` in forward; chunk k takes the gradient of its final state from chunk k + 1 and leaves that of its first
            # state to chunk k - 1 (two buffers in turn); the whole-sequence launch (k = 0) has neither
            last = link or k == K - 1
            cell.launch_bwd(dy, None if last else cell.rows(carry[(k + 1) & 1]), w_hh, cell.rows(h0), b.m, y, sv, dgi, dgh,
                            cell.rows(dh0_out if k == 0 else carry[k & 1]), k * Tc, T if link else Tc, ws(role, link), own_chunks,
                            link and (Tc, *link))

        chain = multi and stage.chainable and owned and ctx.chain and K > 1
        b.cnt = _pipeline(("b.g2", "b.at", "b.g1"), main, (sg, sa, main), range(K - 1, -1, -1),
                          chain and (cell.chain_workgroups(), _abi.lib().wsmg_rows_gemm_workgroups(rows, H)), dev,
                          functools.partial(rnn_bwd, b.dy2, b.w_hh2, b.h02, b.y2, b.sv2, b.dgi2, b.dgh2, b.dh02, b.carry2, "b2"), stage.bwd,
                          functools.partial(rnn_bwd, b.dstate, b.w_hh1, b.h01, b.y1, b.sv1, b.dgi1, b.dgh1, b.dh01, b.carry1, "b1"))
        g2, gh2, g1, gh1 = b.dgi2r, b.dgh2.view(B, G * H), b.dgi1.view(B, G * H), b.dgh1.view(B, G * H)
        d_state_in = torch.mm(g1, b.w_ih1) if ctx.needs_input_grad[1] else None
        # gradients of the shared instruction sets (they feed the instruction branch's backward, on ITS stream): after the last
        # attention chunk on the attention stream, joined into main below — by then recurrence 1's last chunk has long hidden them
        with torch.cuda.stream(sa):
            member = torch.nn.functional.one_hot(b.inverse, U).to(torch.float32).t()            # [U, B]
            dk = torch.matmul((member.unsqueeze(2) * b.dl.unsqueeze(0)).transpose(1, 2), b.q1).to(b.text_k.dtype)
            dv = torch.matmul((member.unsqueeze(2) * b.attn_text.unsqueeze(0)).transpose(1, 2), b.dtext).to(b.text_v.dtype)
        if multi:
            ekv = torch.cuda.Event()
            ekv.record(sa)
            sl.wait_stream(main)
            sl.wait_stream(sg)
        # parameter gradients: full-batch GEMMs and column sums, off the chain
        with torch.cuda.stream(sl):
            # the seven bias gradients (column sums) in one launch (torch: a reduction kernel + a memset each); an LSTM's
            # db_hh = db_ih = colsum(dgates), two tensors of their own
            db_ih2, db_hh2, dbc, dbq2, dbq1, db_hh1, db_ih1 = _ops.colsum_multi([g2, gh2, b.dxc, b.dq2, b.dq1, gh1, g1])
            dw_ih2 = g2.t() @ b.xc
            dw_hh2 = cell.hidden_weight_grads(b.dgh2, b.h02, b.y2, b.m)      # dgh^T (mask * h_prev): an LSTM's h_prev is the h row of [h; c]
            dwc = b.dxc.t() @ stage.concat()
            dwk = (b.q2.t() @ b.dqf).reshape(wk_shape)
            # (the key projection's bias adds the same number to every token's logit: it cancels in the softmax, gradient exactly 0)
            dbk = torch.zeros(wk_shape[0], device=dev, dtype=torch.float32) if params[9] is not None else None
            dwq2 = b.dq2.t() @ b.text_emb
            dwq1 = b.dq1.t() @ b.y1r
            dw_hh1 = cell.hidden_weight_grads(b.dgh1, b.h01, b.y1, b.m)
            dw_ih1 = g1.t() @ b.state_in
        pgrads = [dw_ih1, db_ih1, dw_hh1, db_hh1, dwq1, dbq1, dwq2, dbq2, dwk, dbk, dwc, dbc, dw_ih2, db_ih2, dw_hh2, db_hh2]
        _core.chain_in_flight = False      # every kernel of this block's backward is queued: the gradient exchange may issue buckets again
        if multi:
            main.wait_event(ekv)
            for i, p in enumerate(params):
                if p is None or not p.requires_grad or pgrads[i] is None:
                    continue
                p._wsmg_grad_stream = sl           # wsmgmap.parallel.GradAllReducer packs this gradient behind that stream
                p.grad = pgrads[i]
                for hook in list((getattr(p, "_post_accumulate_grad_hooks", None) or {}).values()):
                    hook(p)
            pgrads = [None] * len(pgrads)
        # the map tokens' gradient: parked for the token mean's backward, which merges its broadcast row and the producing
        # convolution's ReLU mask into it in one pass (ops.TokenGradSink), or returned
        if sink is not None:
            sink.park(b.dtokens)
        return (None, d_state_in, b.dtokens if sink is None else None, dk, dv, None, None, None, b.dh01, b.dh02, *pgrads)


def recurrent_block(state_in, tokens, text, masks, h01, h02, net, n_env, chunks=4, sink=None, text_ready=None, streams=None):
    """-> (x [B, H] = the second recurrence's outputs, att_map [B, I], h1_n, h2_n: [1, N, H] each, [2, N, H] = [h; c] for an LSTM).
    state_in [B, in] (rows time-major, B = T * n_env); tokens [B, I, 256] map tokens (keys == values, the key projection
    `net.text_map_k_layer` folded into the query); text = (keys [U, L, 256], values [U, L, 256], pad mask uint8 [U, L], inverse
    int64 [B]) of the U unique instructions; masks [B, 1]; h01 / h02 [N, H] (GRU) or [2, N, H] (LSTM: habitat's [h; c]); net: the
    MGMapNet whose layers these are (core_cell(net) must not be None); text_ready: an event after which `text` is complete
    (recorded on the instruction branch's stream), or None when the caller's stream already waited; streams: up to two helper
    streams that are idle while the block runs (see _roles), None = one stream."""
    cell = core_cell(net)
    if cell is None:
        raise _abi.WsmgError("recurrent_block: these state encoders take the staged route (an LSTM needs hidden 512 and the kernels)")
    r1, r2 = net.state_encoder.rnn, net.second_state_encoder.rnn
    tk, tv, tm, inv = text
    cfg = dict(N=int(n_env), chunks=int(chunks), scale=float(net._scale_f), sink=sink, text_ready=text_ready, streams=tuple(streams or ()),
               cell=_ops.LSTM if cell == "LSTM" else _ops.GRU)
    return _RecurrentBlock.apply(
        cfg, state_in.contiguous(), tokens.contiguous(), tk, tv, tm, inv, masks.reshape(-1).float().contiguous(), h01, h02,
        r1.weight_ih_l0, r1.bias_ih_l0, r1.weight_hh_l0, r1.bias_hh_l0,
        net.state_text_q_layer.weight, net.state_text_q_layer.bias, net.text_map_q_layer.weight, net.text_map_q_layer.bias,
        net.text_map_k_layer.weight, net.text_map_k_layer.bias, net.second_state_compress[0].weight, net.second_state_compress[0].bias,
        r2.weight_ih_l0, r2.bias_ih_l0, r2.weight_hh_l0, r2.bias_hh_l0)

