"""GPU tests, round 4 (VERDICT r03 "Next round" + ADVICE r03): feeder epochs / oversize batches, the data-parallel exchange beside
the persistent RNN kernels over RCCL, and the parity of the kernels added this round (each next to its section below)."""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(autouse=True)
def _aux_losses_off():
    from wsmgmap.common.aux_losses import AuxLosses
    AuxLosses.deactivate()
    AuxLosses.clear()
    yield
    AuxLosses.deactivate()
    AuxLosses.clear()


class _Store:
    """picklable in-memory record store (stands in for the reference's LMDB)"""
    def __init__(self, blobs):
        self.blobs = blobs

    def __call__(self, i):
        return self.blobs[i]


# ----------------------------------------------------------------------------- feeder (ADVICE r03, medium x 2)
def test_feeder_ring_reshuffles_every_epoch_and_survives_oversize_batches():
    """(1) The ring's decode workers are re-seeded per epoch (a fresh base seed per iterator, as DataLoader draws one:
    dagger_trainer.py:116-119,585-594), so the batch order differs from epoch to epoch; an explicit seed reproduces a run.
    (2) A batch that does not fit the ring slot arrives anyway (its own shared block), with the same values."""
    from oracle import data_cases as dc
    from wsmgmap.data import TrajectoryDataset, DeviceFeeder, pack_record
    lengths = (dc.DATASET_LENGTHS * 3)[:64]
    store = _Store([pack_record(*dc.episode(1000 + i, n)) for i, n in enumerate(lengths)])
    mk = lambda: TrajectoryDataset(store, len(store.blobs), batch_size=2, rank=0, world_size=1)  # noqa: E731

    def epoch(fd):
        order, vals = [], {}
        for ob, prev, masks, corr, wts in fd:
            firsts = prev.view(-1, 2, 2)[0, :, 0].cpu().tolist()
            order += firsts
            for n, f in enumerate(firsts):
                vals[f] = float(ob["progress"].view(-1, 2, 1)[:, n].sum())
        return order, vals

    fd = DeviceFeeder(mk(), 2, "cuda", num_workers=2, prefetch=2)
    o1, v1 = epoch(fd)
    o2, v2 = epoch(fd)
    assert fd.epoch == 2 and sorted(o1) == sorted(o2) and o1 != o2, "the same batch order in two epochs"
    a, _ = epoch(DeviceFeeder(mk(), 2, "cuda", num_workers=2, prefetch=2, seed=9))
    b, _ = epoch(DeviceFeeder(mk(), 2, "cuda", num_workers=2, prefetch=2, seed=9))
    assert a == b
    fs = DeviceFeeder(mk(), 2, "cuda", num_workers=2, prefetch=2, seed=9)
    e1, _ = epoch(fs)
    e2, _ = epoch(fs)
    assert e1 == a and e2 != e1
    # oversize: slots of 4 KiB hold only the shortest batches
    small = DeviceFeeder(mk(), 2, "cuda", num_workers=2, prefetch=2, seed=9, slot_bytes=4096)
    c, vc = epoch(small)
    _, va = epoch(DeviceFeeder(mk(), 2, "cuda", num_workers=2, prefetch=2, seed=9))
    assert small.oversize_batches > 0 and c == a and vc == va


# ----------------------------------------------------------------------------- the pipelined recurrent core
def _one_update(pol, obs, prev, masks, weights, N, chunks):
    """forward + DAgger loss + backward with the recurrent core staged (chunks = 0) or pipelined; -> (pred, loss, att, h, grads)."""
    import bench
    from wsmgmap.common.aux_losses import AuxLosses
    pol.net.recurrent_chunks = chunks
    for p in pol.parameters():
        p.grad = None
    AuxLosses.activate()
    AuxLosses.clear()
    h = torch.zeros(2, N, 512, device="cuda")
    o = dict(obs)
    pred, aux = pol(o, h, prev, masks, weights)
    loss = bench.dagger_loss(pred, aux, o["waypoint"], weights)
    loss.backward()
    torch.cuda.synchronize()
    AuxLosses.deactivate()
    grads = {k: (None if p.grad is None else p.grad.detach().clone()) for k, p in pol.named_parameters()}
    return pred.detach().clone(), float(loss), pol.net.att_map_t_m.detach().clone(), h.clone(), grads


@pytest.mark.parametrize("mode,T,N", [("bf16", 64, 8), ("f32", 16, 8), ("bf16", 12, 3)])
def test_pipelined_recurrent_core_matches_the_staged_route(mode, T, N):
    """mg_map_policy.py:220-249 of the reference — GRU 1 -> text attention -> map attention -> second_state_compress -> GRU 2 — as one
    autograd node pipelined over 4 time chunks on three streams (wsmgmap/recurrent.py) against the stage-after-stage route of
    rounds 1-3, on the bench workload (T = 64 x N = 8, bf16) and two smaller shapes: action logits, loss, the map attention row, the
    carried hidden states and EVERY parameter gradient.  The kernels and the float32 GEMMs are the same row for row; the only
    freedom is the GEMM library's kernel choice for 128-row chunks vs 512 rows (float32 rounding): 2e-5 of the largest element."""
    import bench
    import test_gpu_round2 as r2
    from wsmgmap import ops
    pol = r2._train_mode(r2._policy(num_proc=1, compute_dtype=mode, state=r2._default_state()))
    obs, prev, masks, weights = bench.synth_batch(T, N, torch.device("cuda"), 77)
    masks = masks.clone()
    masks.view(T, N)[T // 2 + 1, N - 1] = 0          # an episode restart inside a chunk
    a = _one_update(pol, obs, prev, masks, weights, N, 0)
    b = _one_update(pol, obs, prev, masks, weights, N, 4)
    c = _one_update(pol, obs, prev, masks, weights, N, 4)
    ops.check_rnn_status()

    def close(x, y, name, tol=2e-5):
        assert x.shape == y.shape, name
        d = float((x.double() - y.double()).abs().max())
        assert d <= tol * max(1e-6, float(y.double().abs().max())), (name, d, float(y.abs().max()))
    close(b[0], a[0], "pred")
    assert abs(a[1] - b[1]) <= 2e-6 * max(1.0, abs(a[1]))
    close(b[2], a[2], "att_map_t_m")
    close(b[3], a[3], "rnn_hidden_states")
    assert set(k for k, g in a[4].items() if g is not None) == set(k for k, g in b[4].items() if g is not None)
    core = ("net.state_encoder.", "net.second_state_encoder.", "net.state_text_q_layer.", "net.text_map_q_layer.", "net.text_map_k_layer.",
            "net.second_state_compress.", "action_distribution.", "prog_pred.")
    from util import NULL_GRAD
    for k, g in a[4].items():
        if g is None or k in NULL_GRAD:     # (gradients that are identically zero in exact arithmetic: rounding noise on both sides)
            continue
        if mode == "f32" or k.startswith(core):
            close(b[4][k], g, k, tol=5e-5)
        else:
            # bf16 map stack / instruction branch behind it: a 1e-6 difference in the map tokens' gradient flips bf16 roundings on
            # the way down, and the deepest layers see it amplified (measured 0.9 % of the largest element on the first
            # convolution's weight): direction and size of the tensor are what is held
            x, y = b[4][k].double().flatten(), g.double().flatten()
            if float(y.norm()) > 0:
                cos = float((x @ y) / (x.norm() * y.norm()))
                assert cos >= 0.9999, (k, cos)
            close(b[4][k], g, k, tol=3e-2)
    # the pipelined route is repeatable bit for bit (streams and chunk order change no arithmetic)
    assert torch.equal(b[0], c[0]) and b[1] == c[1]
    for k, g in b[4].items():
        if g is not None:
            assert torch.equal(g, c[4][k]), k


def test_recurrent_block_alone_vs_float64_autograd():
    """The block as an operator: against the same formulas in float64 torch autograd (GRU as explicit steps), values and all gradients,
    with chunk counts 1, 2 and 4 agreeing with each other."""
    from wsmgmap import recurrent
    from wsmgmap.config import default_model_config
    from wsmgmap.models.mg_map_policy import MGMapNet
    torch.manual_seed(3)
    T, N, I, U, L = 8, 4, 36, 3, 11
    B = T * N
    net = MGMapNet(None, default_model_config(num_proc=1)).cuda()
    state_in = torch.randn(B, 640, device="cuda") * 0.5
    tokens = torch.randn(B, I, 256, device="cuda") * 0.5
    tk, tv = torch.randn(U, L, 256, device="cuda"), torch.randn(U, L, 256, device="cuda")
    tmask = torch.zeros(U, L, dtype=torch.uint8, device="cuda")
    tmask[1, 7:] = 1
    inverse = torch.randint(0, U, (B,), device="cuda")
    masks = torch.ones(T, N, device="cuda")
    masks[0] = 0
    masks[5, 2] = 0
    h01, h02 = torch.randn(N, 512, device="cuda") * 0.3, torch.randn(N, 512, device="cuda") * 0.3
    gy, ga = torch.randn(B, 512, device="cuda"), torch.randn(B, I, device="cuda") * 0.1
    names = ["state_encoder.rnn.weight_ih_l0", "state_encoder.rnn.bias_ih_l0", "state_encoder.rnn.weight_hh_l0", "state_encoder.rnn.bias_hh_l0",
             "state_text_q_layer.weight", "state_text_q_layer.bias", "text_map_q_layer.weight", "text_map_q_layer.bias", "text_map_k_layer.weight",
             "second_state_compress.0.weight", "second_state_compress.0.bias", "second_state_encoder.rnn.weight_ih_l0",
             "second_state_encoder.rnn.bias_ih_l0", "second_state_encoder.rnn.weight_hh_l0", "second_state_encoder.rnn.bias_hh_l0"]
    P = dict(net.named_parameters())

    def run(chunks):
        for n in names:
            P[n].grad = None
        ins = [t.clone().requires_grad_(True) for t in (state_in, tokens, tk, tv, h01, h02)]
        x, att, h1n, h2n = recurrent.recurrent_block(ins[0], ins[1], (ins[2], ins[3], tmask, inverse), masks.view(B, 1), ins[4], ins[5],
                                                     net, N, chunks=chunks)
        ((x * gy).sum() + (att * ga).sum()).backward()
        torch.cuda.synchronize()
        return [x.detach(), att.detach(), h1n, h2n] + [t.grad for t in ins] + [P[n].grad.clone() for n in names]

    def gru64(x, rnn, h, m):
        wi, bi, wh, bh = [t.detach().double() for t in (rnn.weight_ih_l0, rnn.bias_ih_l0, rnn.weight_hh_l0, rnn.bias_hh_l0)]
        ws = [t.requires_grad_(True) for t in (wi, bi, wh, bh)]
        ys = []
        for t in range(T):
            h = h * m[t].unsqueeze(-1)
            gi, gh = x[t] @ ws[0].t() + ws[1], h @ ws[2].t() + ws[3]
            ir, iz, inn = gi.chunk(3, 1)
            hr, hz, hn = gh.chunk(3, 1)
            r, z = torch.sigmoid(ir + hr), torch.sigmoid(iz + hz)
            n = torch.tanh(inn + r * hn)
            h = (1 - z) * n + z * h
            ys.append(h)
        return torch.stack(ys), ws

    ins64 = [t.double().clone().requires_grad_(True) for t in (state_in, tokens, tk, tv, h01, h02)]
    d = lambda n: P[n].detach().double().requires_grad_(True)    # noqa: E731
    wq1, bq1, wq2, bq2, wk, wc, bc = (d(n) for n in names[4:11])
    m64 = masks.double()
    y1, ws1 = gru64(ins64[0].view(T, N, -1), net.state_encoder.rnn, ins64[4], m64)
    state = y1.reshape(B, 512)
    sc = net._scale_f

    def attn(q, k, v, mask):
        logits = torch.einsum("bc,bic->bi", q, k)
        if mask is not None:
            logits = logits - mask.double() * 1e8
        a = torch.softmax(logits * sc, dim=1)
        return torch.einsum("bi,bic->bc", a, v), a
    te, _ = attn(state @ wq1.t() + bq1, ins64[2][inverse], ins64[3][inverse], tmask[inverse])
    q2 = te @ wq2.t() + bq2
    keys = torch.einsum("oc,bic->bio", wk.reshape(256, 256), ins64[1])       # the k = 1 Conv1d key projection (bias cancels)
    me, att64 = attn(q2, keys, ins64[1], None)
    xc = torch.relu(torch.cat([state, te, me], 1) @ wc.t() + bc)
    y2, ws2 = gru64(xc.view(T, N, -1), net.second_state_encoder.rnn, ins64[5], m64)
    ((y2.reshape(B, 512) * gy.double()).sum() + (att64 * ga.double()).sum()).backward()
    ref = [y2.reshape(B, 512).detach(), att64.detach(), y1[-1:].detach(), y2[-1:].detach()] + [t.grad for t in ins64] + \
          [ws1[0].grad, ws1[1].grad, ws1[2].grad, ws1[3].grad, wq1.grad, bq1.grad, wq2.grad, bq2.grad, wk.grad, wc.grad, bc.grad,
           ws2[0].grad, ws2[1].grad, ws2[2].grad, ws2[3].grad]
    outs = {c: run(c) for c in (1, 2, 4)}
    for c, got in outs.items():
        assert len(got) == len(ref)
        for i, (g, r) in enumerate(zip(got, ref)):
            err = float((g.double() - r).abs().max())
            assert err <= 3e-5 * max(1e-3, float(r.abs().max())), (c, i, err, float(r.abs().max()))
    for i, (g1, g4) in enumerate(zip(outs[1], outs[4])):
        assert float((g1 - g4).abs().max()) <= 1e-5 * max(1e-3, float(g1.abs().max())), i


# ----------------------------------------------------------------------------- data-parallel launch path
def _free_port():
    import socket
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _dp_soak_worker(port, q, queues, updates):
    """One rank over RCCL on this box's GPU: `updates` teacher-forcing updates (bf16, T = 16 x N = 8, the pipelined recurrent core on
    its three streams, decoder and instruction side streams, multi-tensor Adam) with the gradient exchange, then the same from the
    same state without it."""
    if queues:
        os.environ["GPU_MAX_HW_QUEUES"] = str(queues)       # before the HIP runtime starts in this process
    else:
        os.environ.pop("GPU_MAX_HW_QUEUES", None)
    for p in (ROOT, os.path.join(ROOT, "ws-mgmap_amd"), os.path.join(ROOT, "tests")):
        if p not in sys.path:
            sys.path.insert(0, p)
    try:
        import torch.distributed as dist
        import bench
        import test_gpu_round2 as r2
        from wsmgmap import ops
        from wsmgmap.common.aux_losses import AuxLosses
        from wsmgmap.optim import Adam
        from wsmgmap.parallel import GradAllReducer
        torch.cuda.set_device(0)
        os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
        dist.init_process_group("nccl", rank=0, world_size=1, device_id=torch.device("cuda", 0))
        T_, N = 16, 8
        state = r2._default_state()
        obs, prev, masks, weights = bench.synth_batch(T_, N, torch.device("cuda"), 5)
        AuxLosses.activate()

        def run(exchange):
            pol = r2._train_mode(r2._policy(num_proc=1, compute_dtype="bf16", state=state))
            assert pol.net.recurrent_chunks == 4
            opt = Adam(pol.parameters(), lr=2.5e-4)
            red = GradAllReducer(pol.parameters(), bucket_bytes=4 << 20, single_rank_exchange=True) if exchange else None
            if red:
                red.broadcast_parameters(pol)
            else:
                # under an initialised process group the pipelined core keeps its chunked, leaf-stream backward only for parameters
                # whose gradient-ready hook is GradAllReducer's (a stock DDP wrap hooks AccumulateGrad instead): the comparison run
                # must take the same route — full-batch GEMMs round differently from four 128-row chunks, in the sixth digit
                for p_ in pol.parameters():
                    p_._wsmg_reducer = True
            losses = []
            for _ in range(updates):
                opt.zero_grad(set_to_none=True)
                AuxLosses.clear()
                o = dict(obs)
                pred, aux = pol(o, torch.zeros(2, N, 512, device="cuda"), prev, masks, weights)
                loss = bench.dagger_loss(pred, aux, o["waypoint"], weights)
                loss.backward()
                if red:
                    red.finish()
                opt.step()
                losses.append(loss.detach())
            torch.cuda.synchronize()
            if red:
                red.check()
            ops.check_rnn_status()          # raises on any persistent-RNN timeout of the run
            return [float(x) for x in losses], (red.stats() if red else None)
        with_x, stats = run(True)
        without, _ = run(False)
        q.put(("ok", dict(with_exchange=with_x, without=without, stats=stats, queues=os.environ.get("GPU_MAX_HW_QUEUES"))))
        dist.destroy_process_group()
    except Exception as e:  # pragma: no cover
        import traceback
        q.put(("error", traceback.format_exc() + repr(e)))


@pytest.mark.parametrize("queues", [0, 8], ids=["hwq_default4", "hwq8"])
def test_data_parallel_soak_over_rccl_beside_the_persistent_kernels(queues):
    """The N > 1 launch path as far as a 1-GPU box can take it (common_trainer.py:35-38,60-66 of the reference): 50 updates with the
    whole gradient exchange going through RCCL (one-rank communicator: its kernels, its streams, the bucket hooks inside backward)
    WHILE the pipelined recurrent core runs up to three persistent kernels on three streams and the decoder / instruction branches
    run on theirs — with HIP's default 4 hardware queues and with GPU_MAX_HW_QUEUES=8 (what bench.py sets for --gpus N).  The
    persistent kernels are ordinary (non-cooperative) launches that rely on their 32 workgroups being co-resident: zero timeouts,
    and the loss sequence equal BIT FOR BIT to the same 50 updates without the exchange (world = 1: averaging changes nothing)."""
    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    p = ctx.Process(target=_dp_soak_worker, args=(_free_port(), q, queues, 50))
    p.start()
    status, info = q.get(timeout=900)
    p.join(timeout=120)
    assert status == "ok", info
    assert info["queues"] == (str(queues) if queues else None)
    assert len(info["with_exchange"]) == 50 and info["with_exchange"] == info["without"], \
        [(i, a, b) for i, (a, b) in enumerate(zip(info["with_exchange"], info["without"])) if a != b][:5]
    assert info["with_exchange"][-1] < info["with_exchange"][0]          # it trained
    assert info["stats"]["updates"] == 50


def test_rnn_timeout_in_a_data_parallel_run_names_the_likely_cause():
    """a persistent-RNN timeout seen by GradAllReducer.finish() is agreed on by the ranks (gradients zeroed) and
    raised at the next finish() as GradExchangeError WITH the likely cause in a data-parallel run — the persistent kernels'
    workgroups not co-resident beside the collective's kernels — and the switches that fall back to one persistent kernel at a
    time.  One-rank gloo group in this process; the timeout is forced with the spin-limit hook."""
    import torch.distributed as dist
    from wsmgmap import _abi, ops
    from wsmgmap.parallel import GradAllReducer, GradExchangeError
    torch.cuda.synchronize()
    ops.check_rnn_status()
    dist.init_process_group("gloo", init_method="tcp://127.0.0.1:%d" % _free_port(), rank=0, world_size=1)
    L = _abi.lib()
    try:
        g = torch.Generator().manual_seed(3)
        gi = torch.randn(6, 4, 1536, generator=g).cuda()
        w = torch.nn.Parameter((torch.randn(1536, 512, generator=g) * 0.04).cuda())
        b, h0, m = torch.zeros(1536).cuda(), torch.randn(4, 512, generator=g).cuda(), torch.ones(6, 4).cuda()
        red = GradAllReducer([w], single_rank_exchange=True)
        ops.masked_gru(gi, w, b, h0, m).sum().backward()
        red.finish()                                   # discovery pass, clean
        w.grad = None
        L.wsmg_rnn_debug_spin_limit(1)
        ops.masked_gru(gi, w, b, h0, m).sum().backward()
        torch.cuda.synchronize()
        L.wsmg_rnn_debug_spin_limit(0)
        red.finish()                                   # sees the timeout, takes part in the exchange, zeroes the gradients
        torch.cuda.synchronize()
        assert float(w.grad.abs().max()) == 0.0
        with pytest.raises(GradExchangeError) as ei:
            red.check()
        msg = str(ei.value)
        assert "timed out" in msg and "co-resident" in msg and "recurrent_chunks" in msg and "WSMG_DECODER_STREAMS" in msg, msg
    finally:
        L.wsmg_rnn_debug_spin_limit(0)
        torch.cuda.synchronize()
        L.wsmg_rnn_status(1)
        dist.destroy_process_group()


# ----------------------------------------------------------------------------- instruction dedup in one launch
@pytest.mark.parametrize("dtype", [torch.float32, torch.int64])
def test_instruction_dedup_in_one_launch_matches_torch_unique(dtype):
    """csrc/wsmg_dedup.hip against torch.unique(dim=0): the same SET of distinct rows, inverse reconstructs the input exactly,
    rows in order of first appearance, lengths = non-zero tokens; cases: the teacher-forcing pattern (N rows repeated over T),
    all rows distinct, all rows equal, rows that differ in the last token only, B = 1, a wide batch (B = 2400)."""
    from wsmgmap.models.encoders.instruction_encoder import InstructionEncoder
    g = torch.Generator().manual_seed(11)

    def rows(n, L=200, length=80):
        t = torch.zeros(n, L, dtype=torch.int64)
        t[:, :length] = torch.randint(1, 2504, (n, length), generator=g)
        return t
    base = rows(8)
    last = rows(1).repeat(6, 1)
    last[:, 79] = torch.arange(1, 7)
    cases = [base.repeat(64, 1), rows(300), rows(1).repeat(77, 1), last, rows(1), torch.cat([rows(40, length=37), rows(5)]).repeat(53, 1)[:2400],
             torch.cat([rows(3, length=200), torch.zeros(2, 200, dtype=torch.int64)])]
    for t in cases:
        tok = t.to(dtype).cuda()
        uniq, inverse, len_host, len_dev = InstructionEncoder._dedup_fused(tok)
        torch.cuda.synchronize()
        ref_u, ref_inv = torch.unique(t, dim=0, return_inverse=True)
        assert uniq.shape[0] == ref_u.shape[0]
        assert torch.equal(uniq.cpu()[inverse.cpu()], t)                           # exact reconstruction
        assert set(map(tuple, uniq.cpu().tolist())) == set(map(tuple, ref_u.tolist()))
        first = [int((inverse.cpu() == u).nonzero()[0]) for u in range(uniq.shape[0])]
        assert first == sorted(first)                                              # order of first appearance
        assert torch.equal(len_host, (uniq.cpu() != 0).sum(1)) and torch.equal(len_dev.cpu(), len_host)


def test_feeder_streams_a_recoded_cache_bit_identically():
    """the same episodes stored the reference's way (zlib(msgpack_numpy)) and recoded (raw, uncompressed) come
    out of DeviceFeeder — worker processes, shared-memory ring, device collate — as bit-identical batches, in the same order."""
    from oracle import data_cases as dc
    from wsmgmap.data import DeviceFeeder, TrajectoryDataset, pack_record, recode_record
    lengths = (dc.DATASET_LENGTHS * 2)[:32]
    blobs = [pack_record(*dc.episode(2000 + i, n)) for i, n in enumerate(lengths)]
    raws = [recode_record(b) for b in blobs]

    def run(store):
        ds = TrajectoryDataset(_Store(store), len(store), batch_size=4, rank=0, world_size=1)
        out = []
        for ob, prev, masks, corr, wts in DeviceFeeder(ds, 4, "cuda", num_workers=2, prefetch=2, seed=3):
            out.append(({k: v.cpu() for k, v in ob.items()}, prev.cpu(), masks.cpu(), corr.cpu(), wts.cpu()))
        return out
    a, b = run(blobs), run(raws)
    assert len(a) == len(b) and len(a) > 0
    for (oa, *ra), (ob_, *rb) in zip(a, b):
        assert list(oa) == list(ob_) and all(torch.equal(oa[k], ob_[k]) for k in oa)
        assert all(torch.equal(x, y) for x, y in zip(ra, rb))


# ----------------------------------------------------------------------------- small-channel 3 x 3 weight gradients out of the LDS window
@pytest.mark.parametrize("shape", [
    (130, 24, 64, 64),          # conv_original_size1: 64 co x 64 ci, two waves per tile pair (V222), ragged image ranges
    (115, 24, 256, 64),         # conv_original_size0: four input-channel tiles
    (120, (24, 23), 192, 64),   # conv_original_size2: three input-channel tiles, a row length whose padded rows leave a partial k-step
    (131, 24, 32, 128),         # map_classified_linear: 128 co x 32 ci (V412)
    (67, 48, 32, 32),           # the classifier's 32 -> 32 layer at 48 x 48: eight waves on one tile pair (V118)
    (33, (47, 43), 32, 96),     # V118 with three output-channel tiles and a ragged image
    (259, 16, 32, 32),          # narrowest rows the window kernels take
], ids=["orig1", "orig0", "orig2", "classified", "cls48", "cls-ragged", "w16"])
def test_small_channel_window_weight_gradients_3x3(shape):
    """wsmg_conv_win3_wgrad.hip, round-4 tile shapes (pixel-split tile pairs whose partial sums meet in LDS): the atomic form and the
    slab form against a float64 weight gradient of the same bf16 operands and against the generic kernel (window kernels off);
    the slab form is bit-identical over repeated launches."""
    import ctypes
    import torch.nn.functional as F
    from wsmgmap import _abi, ops
    B, H, Cin, Cout = shape
    H, W = H if isinstance(H, tuple) else (H, H)
    torch.manual_seed(B + Cin)
    x = torch.relu(torch.randn(B, H, W, Cin, device="cuda")).bfloat16()
    gy = (torch.randn(B, H, W, Cout, device="cuda") * 0.1).bfloat16()
    P = lambda t: ctypes.c_void_p(t.data_ptr())   # noqa: E731
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    assert _abi.lib().wsmg_conv_debug_win3_tile(1) in (0, 1, 256, 512)
    ns, fl = ctypes.c_int(0), ctypes.c_longlong(0)
    dims = (B, H, W, Cin, Cout, 3, 3, 1, 1, H, W)
    _abi.call("wsmg_conv2d_bwd_weight_bf16_plan", *dims, ctypes.cast(ctypes.byref(ns), ctypes.c_void_p), ctypes.cast(ctypes.byref(fl), ctypes.c_void_p))
    assert 1 <= ns.value <= 256, f"{ns.value} slabs: the layer did not take the window kernel's plan"
    import conv_route_util as cr
    r = cr.route(cr.BWD_WEIGHT, dims)
    assert (r["kind"], r["nsplit"]) == ("WGRAD_WIN3", ns.value), r

    def atomic(tile):
        prev = _abi.lib().wsmg_conv_debug_win3_tile(tile)
        try:
            assert cr.route(cr.BWD_WEIGHT, dims)["kind"] == ("WGRAD_WIN3" if tile else "WGRAD")      # tile 0: window kernels off
            dw = torch.zeros(Cout, 3, 3, Cin, device="cuda")
            _abi.call("wsmg_conv2d_bwd_weight_bf16", P(x), P(gy), P(dw), *dims, st)
            torch.cuda.synchronize()
            return dw
        finally:
            _abi.lib().wsmg_conv_debug_win3_tile(prev)
    dw = atomic(1)
    w = torch.zeros(Cout, Cin, 3, 3, device="cuda", dtype=torch.float64, requires_grad=True)
    F.conv2d(x.permute(0, 3, 1, 2).double(), w, padding=1).backward(gy.permute(0, 3, 1, 2).double())
    ref = w.grad.permute(0, 2, 3, 1)
    scale = float(ref.abs().max())
    assert float((dw.double() - ref).abs().max()) <= 2e-5 * scale, float((dw.double() - ref).abs().max()) / scale
    assert float((dw - atomic(0)).abs().max()) <= 2e-5 * scale
    slabs = [ops._weight_grad("_bf16", x, gy, dims, 0.0, Cin) for _ in range(3)]      # [Cout, Cin, 3, 3]
    torch.cuda.synchronize()
    assert torch.equal(slabs[0], slabs[1]) and torch.equal(slabs[0], slabs[2])
    assert float((slabs[0].permute(0, 2, 3, 1).double() - ref).abs().max()) <= 2e-5 * scale


# ----------------------------------------------------------------------------- stride-2 window weight gradients (k5 64->128, k7 256->64)
@pytest.mark.parametrize("geom", [
    (37, 50, 64, 128, 5, 1),     # MapEncoder.cnn[3]: 8 waves, 5 kernel-row roles, 3 tiles of 8 x 24 pixels per image
    (3, 50, 64, 128, 5, 1),      # fewer tiles than tile groups
    (45, 24, 256, 64, 7, 3),     # MapDecoder conv1: 4 waves, 7 x 4 roles (kernel row x 64-channel chunk), one 12 x 12 tile per image
    (2, 24, 256, 64, 7, 3),
], ids=["enc3", "enc3-few", "stem", "stem-few"])
def test_stride2_window_weight_gradients(geom):
    """wsmg_conv_s2_wgrad.hip against the float64 weight gradient of the same bf16 operands: the atomic form, and the slab form
    (bit-identical over repeated launches), with post-ReLU inputs and a gradient that is zero on a band of rows (tile edges)."""
    import ctypes
    from wsmgmap import _abi, ops
    B, H, Cin, Cout, K, pad = geom
    OH = (H + 2 * pad - K) // 2 + 1
    g = torch.Generator(device="cuda"); g.manual_seed(B * 13 + K)
    x = torch.relu(torch.randn(B, H, H, Cin, device="cuda", generator=g)).bfloat16()
    dy = (torch.randn(B, OH, OH, Cout, device="cuda", generator=g) * 0.1)
    dy[:, OH // 2] = 0
    dy = dy.bfloat16()
    dims = (B, H, H, Cin, Cout, K, K, 2, pad, OH, OH)
    ns, fl = ctypes.c_int(0), ctypes.c_longlong(0)
    _abi.call("wsmg_conv2d_bwd_weight_bf16_plan", *dims, ctypes.cast(ctypes.byref(ns), ctypes.c_void_p), ctypes.cast(ctypes.byref(fl), ctypes.c_void_p))
    assert ns.value % 8 == 0 and ns.value <= 48, f"{ns.value} slabs: not the stride-2 window kernel's plan"
    import conv_route_util as cr
    r = cr.route(cr.BWD_WEIGHT, dims)
    assert (r["kind"], r["nsplit"]) == ("WGRAD_S2WIN", ns.value), r
    want = torch.nn.grad.conv2d_weight(x.double().permute(0, 3, 1, 2), (Cout, Cin, K, K), dy.double().permute(0, 3, 1, 2), stride=2, padding=pad)
    scale = float(want.abs().max())
    dw = torch.zeros(Cout, K, K, Cin, device="cuda")
    _abi.call("wsmg_conv2d_bwd_weight_bf16", ops._p(x), ops._p(dy), ops._p(dw), *dims, ops._stream())
    torch.cuda.synchronize()
    err = float((dw.permute(0, 3, 1, 2).double() - want).abs().max())
    assert err <= 2e-5 * scale, err / scale
    slabs = [ops._weight_grad("_bf16", x, dy, dims, 0.0, Cin) for _ in range(3)]
    torch.cuda.synchronize()
    assert torch.equal(slabs[0], slabs[1]) and torch.equal(slabs[0], slabs[2])
    assert float((slabs[0].double() - want).abs().max()) <= 2e-5 * scale


# ----------------------------------------------------------------------------- feeder route: ego map as channels-last bf16; input readiness
def test_collate_emits_the_ego_map_as_channels_last_bf16_bit_identically():
    """DeviceCollator(ego_map_nhwc_bf16=True) writes `rgb_ego_map` padded, episode-interleaved, channels-last
    and bf16 in ONE pass (wsmg_collate_pad_nhwc_bf16); the values are those of the float32 collate followed by the policy's NCHW
    float32 -> NHWC bf16 conversion, bit for bit (float16 -> float32 -> bf16 either way), the padding steps hold bf16(1.0), every
    other sensor is untouched — and the policy takes the tensor as it is (no layout / dtype launch)."""
    import test_gpu_round2 as r2
    from wsmgmap import ops
    from wsmgmap.data import DeviceCollator
    rng = np.random.RandomState(5)
    lengths, C, E = [7, 3, 5], 64, 10
    batch = []
    for n in lengths:
        obs = {"instruction": rng.randint(0, 27, size=(n, 6)).astype(np.int64),
               "rgb_ego_map": (rng.randn(n, C, E, E) * 3).astype(np.float16),
               "progress": rng.rand(n, 1).astype(np.float32)}
        batch.append((obs, rng.randn(n, 2).astype(np.float32), rng.randn(n, 2).astype(np.float32), torch.ones(n)))
    ref_obs, *ref_rest = DeviceCollator("cuda")(batch)
    new_obs, *new_rest = DeviceCollator("cuda", ego_map_nhwc_bf16=True)(batch)
    torch.cuda.synchronize()
    for a, b in zip(ref_rest, new_rest):
        assert torch.equal(a, b)
    assert torch.equal(ref_obs["instruction"], new_obs["instruction"]) and torch.equal(ref_obs["progress"], new_obs["progress"])
    ego = new_obs["rgb_ego_map"]
    T, N = max(lengths), len(lengths)
    assert ego.dtype == torch.bfloat16 and tuple(ego.shape) == (T * N, C, E, E) and ego.permute(0, 2, 3, 1).is_contiguous()
    want = ops.to_nhwc(ref_obs["rgb_ego_map"].contiguous(), C, dtype=torch.bfloat16)          # [T*N, E, E, C]
    assert torch.equal(ego.permute(0, 2, 3, 1), want)
    pad_rows = [t * N + n for n, ln in enumerate(lengths) for t in range(ln, T)]
    assert pad_rows and bool((ego[pad_rows].float() == 1.0).all())
    # the policy reads it in place
    pol = r2._policy(num_proc=1, compute_dtype="bf16", state=r2._default_state())
    x = pol.net._ego_to_nhwc(ego)
    assert x.data_ptr() == ego.data_ptr() and x.dtype == torch.bfloat16 and tuple(x.shape) == (T * N, E, E, C)
    # and the tokens carry their readiness event
    assert ops.inputs_ready_event(new_obs["instruction"]) is not None


def test_early_instruction_dedup_changes_no_result(monkeypatch):
    """ops.mark_inputs_ready: with the tokens marked complete, the instruction dedup and its host read-back run on a stream that
    does not wait for the previous update (wsmgmap/ops/core.py); losses, logits and every gradient of three consecutive updates are
    bit-identical to the route that waits, and the persistent kernels' status stays clean."""
    import bench
    import test_gpu_round2 as r2
    from wsmgmap import debug, ops
    from wsmgmap.optim import Adam
    T, N = 16, 4

    def run(early):
        monkeypatch.setattr(debug.sw, "early_dedup", early)
        torch.manual_seed(3)
        pol = r2._train_mode(r2._policy(num_proc=1, compute_dtype="bf16", state=r2._default_state()))
        opt = Adam(pol.parameters(), lr=2.5e-4)
        obs, prev, masks, weights = bench.synth_batch(T, N, torch.device("cuda"), 91)
        ops.mark_inputs_ready(obs["instruction"])
        out = []
        for _ in range(3):
            a = _one_update(pol, obs, prev, masks, weights, N, 4)
            opt.step()
            out.append(a)
        ops.check_rnn_status()
        return out, getattr(pol.net, "_early_stream", None) is not None
    (a, used_a), (b, used_b) = run(True), run(False)
    assert used_a and not used_b
    for x, y in zip(a, b):
        assert torch.equal(x[0], y[0]) and x[1] == y[1]
        for k, g in x[4].items():
            assert (g is None) == (y[4][k] is None) and (g is None or torch.equal(g, y[4][k])), k


def test_cls_tail_poisons_the_loss_row_of_an_out_of_range_label():
    """the reference's F.cross_entropy (policy.py:61-66) faults on a label outside [0, classes); the fused classifier tail
    returns NaN for that sample's loss row — and only for that one — instead of a finite number computed from a padded channel."""
    import torch.nn as nn
    from wsmgmap import ops
    B, H, classes = 4, 48, 27
    g = torch.Generator(device="cuda"); g.manual_seed(11)
    y2 = (torch.randn(B, H, H, 32, device="cuda", generator=g) * 1.5).to(torch.bfloat16)
    bn, conv = nn.BatchNorm2d(32).cuda().train(), nn.Conv2d(32, classes, 1).cuda()
    gt = torch.randint(0, classes, (B, 100, 100), device="cuda", generator=g).float()
    gt[1, 50, 50] = float(classes)       # one past the last class
    gt[3, 0, 0] = -1.0
    st = torch.zeros(ops.BN_SLABS, 2, 32, device="cuda", dtype=torch.float64)
    f = y2.double().reshape(-1, 32)
    st[0, 0], st[0, 1] = f.sum(0), (f * f).sum(0)
    _, _, ce = ops.cls_tail(y2, st, bn, conv, gt)
    torch.cuda.synchronize()
    assert torch.isnan(ce).tolist() == [False, True, False, True], ce


def test_collate_hands_over_the_instruction_dedup():
    """DeviceCollator computes the instruction dedup of the padded, time-major batch on the HOST (plan_batch, in the decode worker) and
    attaches it to the token tensor (ops.attach_instruction_dedup): it equals what the device kernel + read-back compute — distinct rows
    in order of first appearance, inverse map, lengths — and the policy's forward pass, which then launches no dedup kernel and reads
    nothing back, gives bit-identical logits, loss and gradients."""
    import bench
    import test_gpu_round2 as r2
    from wsmgmap import ops
    from wsmgmap.data import DeviceCollator
    from wsmgmap.models.encoders.instruction_encoder import InstructionEncoder
    rng = np.random.RandomState(9)
    lengths, L = [7, 3, 5, 7], 12
    instr = [np.concatenate([rng.randint(1, 27, size=rng.randint(3, L)), np.zeros(L, np.int64)])[:L].astype(np.int64) for _ in lengths]
    instr[3] = instr[0].copy()                                  # two episodes with the same instruction
    batch = []
    for n, tok in zip(lengths, instr):
        obs = {"instruction": np.repeat(tok[None], n, 0), "progress": rng.rand(n, 1).astype(np.float32)}
        batch.append((obs, rng.randn(n, 2).astype(np.float32), rng.randn(n, 2).astype(np.float32), torch.ones(n)))
    obs, *_ = DeviceCollator("cuda")(batch)
    torch.cuda.synchronize()
    dd = ops.attached_instruction_dedup(obs["instruction"])
    assert dd is not None and "instruction_dedup" not in obs
    ref = InstructionEncoder._dedup_fused(obs["instruction"].contiguous())
    torch.cuda.synchronize()
    assert torch.equal(dd[0], ref[0]) and torch.equal(dd[1], ref[1])
    assert torch.equal(dd[2], ref[2].cpu()) and torch.equal(dd[3].cpu(), ref[3].cpu())
    assert dd[0].shape[0] == 4          # three distinct instructions + the all-ones padding row
    # in the policy: same update with and without the attached dedup
    T, N = 16, 4
    pol = r2._train_mode(r2._policy(num_proc=1, compute_dtype="bf16", state=r2._default_state()))
    o, prev, masks, weights = bench.synth_batch(T, N, torch.device("cuda"), 93)
    a = _one_update(pol, o, prev, masks, weights, N, 4)
    ops.attach_instruction_dedup(o["instruction"], pol.net.instruction_encoder.dedup(o["instruction"]))
    b = _one_update(pol, o, prev, masks, weights, N, 4)
    assert torch.equal(a[0], b[0]) and a[1] == b[1]
    for k, g in a[4].items():
        assert (g is None) == (b[4][k] is None) and (g is None or torch.equal(g, b[4][k])), k
