"""GPU tests, round 5 (VERDICT r04 "Next round" + ADVICE r04): the recurrent core's dense layers as one launch each, the persistent
kernels beside pinned compute units, the gradient exchange on a policy stream, the race-free early dense inputs, the mixed-tile
window convolution."""
import math
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


# ----------------------------------------------------------------------------- wsmg_rows_gemm_f32
@pytest.mark.parametrize("M", [128, 64, 37, 512])
def test_rows_gemm_matches_float64(M):
    """csrc/wsmg_rows_gemm.hip against the reference's lines in float64 (mg_map_policy.py:229-245: Linear layers over a
    concatenation, ReLU; and their backward products): both weight layouts, one and three operand / output segments, bias,
    accumulate-into (in place), ReLU, the ReLU-backward mask; row counts that are not multiples of the 32-row tile; rows addressed
    at an offset inside full-batch tensors, as wsmgmap/recurrent.py calls it.  Deterministic bit for bit."""
    from wsmgmap import recurrent
    g = torch.Generator(device="cuda").manual_seed(5 + M)
    r0 = 32                       # the chunk starts at row 32 of the full-batch tensors
    Bf = r0 + M + 7
    rnd = lambda *s: torch.randn(*s, device="cuda", generator=g)  # noqa: E731

    def close(got, want, name):
        d = float((got.double() - want).abs().max())
        assert d <= 2e-6 * max(1.0, float(want.abs().max())), (name, d)

    # forward form: xc = relu(cat(y1, text, map) @ wc^T + bc)  (second_state_compress)
    y1, text, mp = rnd(Bf, 512), rnd(Bf, 256), rnd(Bf, 256)
    wc, bc = rnd(512, 1024) * 0.05, rnd(512)
    xc = torch.full((Bf, 512), float("nan"), device="cuda")
    recurrent._rg([y1, text, mp], wc, False, [xc], r0, M, bias=bc, relu=True)
    want = torch.relu(torch.cat([y1, text, mp], 1).double() @ wc.double().t() + bc.double())[r0:r0 + M]
    close(xc[r0:r0 + M], want, "compress")
    assert torch.isnan(xc[:r0]).all() and torch.isnan(xc[r0 + M:]).all()          # rows outside the chunk untouched
    xc2 = torch.empty_like(xc)
    recurrent._rg([y1, text, mp], wc, False, [xc2], r0, M, bias=bc, relu=True)
    assert torch.equal(xc[r0:r0 + M], xc2[r0:r0 + M])
    # plain NT with bias (state_text_q_layer) and the GRU input projection's width
    wq, bq = rnd(256, 512) * 0.05, rnd(256)
    q1 = torch.empty(Bf, 256, device="cuda")
    recurrent._rg([y1], wq, False, [q1], r0, M, bias=bq)
    close(q1[r0:r0 + M], (y1.double() @ wq.double().t() + bq.double())[r0:r0 + M], "q1")
    wih, bih = rnd(1536, 512) * 0.05, rnd(1536)
    gi = torch.empty(Bf, 1536, device="cuda")
    xcv = torch.relu(rnd(Bf, 512))
    recurrent._rg([xcv], wih, False, [gi], r0, M, bias=bih)
    close(gi[r0:r0 + M], (xcv.double() @ wih.double().t() + bih.double())[r0:r0 + M], "gi2")
    # backward forms: d(pre-activation) = (dgi @ w_ih) where xc > 0; d(cat) = dxc @ wc split into its three parts; accumulate-into
    dgi = rnd(Bf, 1536)
    dxc = torch.empty(Bf, 512, device="cuda")
    recurrent._rg([dgi], wih, True, [dxc], r0, M, mask=xcv)
    want = ((dgi.double() @ wih.double()) * (xcv > 0).double())[r0:r0 + M]
    close(dxc[r0:r0 + M], want, "dxc")
    ds, dt, dm = torch.zeros(Bf, 512, device="cuda"), torch.zeros(Bf, 256, device="cuda"), torch.zeros(Bf, 256, device="cuda")
    recurrent._rg([dxc], wc, True, [ds, dt, dm], r0, M)
    want = (dxc.double() @ wc.double())[r0:r0 + M]
    close(ds[r0:r0 + M], want[:, :512], "dstate")
    close(dt[r0:r0 + M], want[:, 512:768], "dtext")
    close(dm[r0:r0 + M], want[:, 768:], "dmap")
    dq = rnd(Bf, 256)
    before = ds.clone()
    recurrent._rg([dq], wq, True, [ds], r0, M, cin_segs=[ds])                   # in place: ds += dq @ wq
    close(ds[r0:r0 + M], (before.double() + dq.double() @ wq.double())[r0:r0 + M], "accumulate")
    assert torch.equal(ds[:r0], before[:r0])


def test_rows_gemm_refuses_shapes_it_does_not_take():
    from wsmgmap import _abi, recurrent
    a, w, c = torch.zeros(8, 40, device="cuda"), torch.zeros(32, 40, device="cuda"), torch.zeros(8, 32, device="cuda")
    with pytest.raises(_abi.WsmgError):
        recurrent._rg([a], w, False, [c], 0, 8)          # K = 40 is not a multiple of 32


@pytest.mark.parametrize("chunks", [4, 8])
def test_recurrent_core_rows_gemm_route_matches_the_gemm_library_route(chunks, monkeypatch):
    """The pipelined recurrent core with its dense layers on wsmg_rows_gemm_f32 (round 5) against the same core on the GEMM library
    (round 4), bench workload, 4 and 8 time chunks: logits, loss, attention row, hidden states and every parameter gradient of the
    core within float32 summation-order noise (2e-5 / 5e-5 of the largest element); bit-identical run to run."""
    import bench
    import test_gpu_round2 as r2
    import test_gpu_round4 as r4
    from wsmgmap import debug, ops
    pol = r2._train_mode(r2._policy(num_proc=1, compute_dtype="bf16", state=r2._default_state()))
    T, N = 64, 8
    obs, prev, masks, weights = bench.synth_batch(T, N, torch.device("cuda"), 78)
    masks = masks.clone()
    masks.view(T, N)[T // 2 + 1, N - 1] = 0
    monkeypatch.setattr(debug.sw, "rows_gemm", False)
    a = r4._one_update(pol, obs, prev, masks, weights, N, chunks)
    monkeypatch.setattr(debug.sw, "rows_gemm", True)
    b = r4._one_update(pol, obs, prev, masks, weights, N, chunks)
    c = r4._one_update(pol, obs, prev, masks, weights, N, chunks)
    ops.check_rnn_status()

    def close(x, y, name, tol=2e-5):
        d = float((x.double() - y.double()).abs().max())
        assert d <= tol * max(1e-6, float(y.double().abs().max())), (name, d, float(y.abs().max()))
    close(b[0], a[0], "pred")
    assert abs(a[1] - b[1]) <= 2e-6 * max(1.0, abs(a[1]))
    close(b[2], a[2], "att_map_t_m")
    close(b[3], a[3], "rnn_hidden_states")
    core = ("net.state_encoder.", "net.second_state_encoder.", "net.state_text_q_layer.", "net.text_map_q_layer.", "net.text_map_k_layer.",
            "net.second_state_compress.", "action_distribution.", "prog_pred.")
    from util import NULL_GRAD
    for k, g in a[4].items():
        if g is None or k in NULL_GRAD:
            continue
        if k.startswith(core):
            close(b[4][k], g, k, tol=5e-5)
        else:
            x, y = b[4][k].double().flatten(), g.double().flatten()
            if float(y.norm()) > 0:
                assert float((x @ y) / (x.norm() * y.norm())) >= 0.9999, k
    assert torch.equal(b[0], c[0]) and b[1] == c[1]
    for k, g in b[4].items():
        if g is not None:
            assert torch.equal(g, c[4][k]), k


# ----------------------------------------------------------------------------- co-residency beside pinned compute units
@pytest.mark.parametrize("pinned", [16, 32])
def test_persistent_kernels_beside_pinned_compute_units(pinned):
    """What an 8-rank RCCL ring with 8-16 channels does to the rest of the GPU, on a box with one: a dummy persistent kernel holds
    `pinned` WHOLE compute units (1 024 threads + 160 KB of LDS each, so nothing else fits on them) while the update runs — the
    pipelined recurrent core's up to three persistent GRU kernels (32 co-resident workgroups each, ordinary launches), the
    instruction LSTM (16), the decoder / instruction side streams.  Zero RNN timeouts, and the 12 losses equal bit for bit those of
    the same updates on the free GPU.  Reference: the data-parallel launch of common_trainer.py:35-38,60-66."""
    import bench
    import test_gpu_round2 as r2
    from wsmgmap import _abi, ops
    from wsmgmap.common.aux_losses import AuxLosses
    from wsmgmap.optim import Adam
    T_, N = 16, 8
    state = r2._default_state()
    obs, prev, masks, weights = bench.synth_batch(T_, N, torch.device("cuda"), 6)

    def run(n_updates):
        pol = r2._train_mode(r2._policy(num_proc=1, compute_dtype="bf16", state=state))
        assert pol.net.recurrent_chunks >= 4
        opt = Adam(pol.parameters(), lr=2.5e-4)
        AuxLosses.activate()
        losses = []
        for _ in range(n_updates):
            opt.zero_grad(set_to_none=True)
            AuxLosses.clear()
            o = dict(obs)
            pred, aux = pol(o, torch.zeros(2, N, 512, device="cuda"), prev, masks, weights)
            loss = bench.dagger_loss(pred, aux, o["waypoint"], weights)
            loss.backward()
            opt.step()
            losses.append(loss.detach())
        torch.cuda.synchronize()
        AuxLosses.deactivate()
        ops.check_rnn_status()
        return [float(x) for x in losses]

    free = run(12)
    stop = torch.zeros(1, dtype=torch.int32, device="cuda")
    arrived = torch.zeros(1, dtype=torch.int32, device="cuda")
    occ, flip = torch.cuda.Stream(), torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(occ):
        _abi.call("wsmg_debug_occupy", pinned, 160 * 1024, 8000, ops._p(stop), ops._p(arrived), ops._stream())
    try:
        import time
        t0 = time.time()
        with torch.cuda.stream(flip):
            while int(arrived.cpu()) < pinned and time.time() - t0 < 5:
                time.sleep(0.01)
            assert int(arrived.cpu()) == pinned, "the occupying workgroups did not all start"
        held = run(12)
        with torch.cuda.stream(flip):
            still = int(arrived.cpu())          # (the kernel is still resident: it only leaves on the flag or after 8 s)
    finally:
        with torch.cuda.stream(flip):
            stop.fill_(1)
        torch.cuda.synchronize()
    assert still == pinned
    assert held == free, [(i, a, b) for i, (a, b) in enumerate(zip(held, free)) if a != b][:4]
    assert held[-1] < held[0]


# ----------------------------------------------------------------------------- gradient exchange on a policy stream
def _xs_worker(port, q, updates):
    for p in (ROOT, os.path.join(ROOT, "ws-mgmap_amd"), os.path.join(ROOT, "tests")):
        if p not in sys.path:
            sys.path.insert(0, p)
    try:
        os.environ["GPU_MAX_HW_QUEUES"] = "8"
        import torch.distributed as dist
        import bench
        import test_gpu_round2 as r2
        from wsmgmap import debug, ops
        from wsmgmap.common.aux_losses import AuxLosses
        from wsmgmap.optim import Adam
        from wsmgmap.parallel import GradAllReducer
        torch.cuda.set_device(0)
        os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
        dist.init_process_group("nccl", rank=0, world_size=1, device_id=torch.device("cuda", 0))
        T_, N = 16, 8
        state = r2._default_state()
        obs, prev, masks, weights = bench.synth_batch(T_, N, torch.device("cuda"), 5)
        ops.mark_inputs_ready(obs["instruction"])
        AuxLosses.activate()

        def run(xs):
            pol = r2._train_mode(r2._policy(num_proc=1, compute_dtype="bf16", state=state))
            opt = Adam(pol.parameters(), lr=2.5e-4)
            red = GradAllReducer(pol.parameters(), bucket_bytes=4 << 20, single_rank_exchange=True, exchange_stream=xs)
            red.broadcast_parameters(pol)
            losses = []
            for _ in range(updates):
                opt.zero_grad(set_to_none=True)
                AuxLosses.clear()
                o = dict(obs)
                pred, aux = pol(o, torch.zeros(2, N, 512, device="cuda"), prev, masks, weights)
                loss = bench.dagger_loss(pred, aux, o["waypoint"], weights)
                loss.backward()
                red.finish()
                opt.step()
                losses.append(loss.detach())
            torch.cuda.synchronize()
            ops.check_rnn_status()
            red.check()
            return [float(x) for x in losses], red.stats(), bool(debug.sw.early_dedup_dp)
        hook, _, early0 = run(None)
        xs, st, early1 = run("instruction")
        dist.destroy_process_group()
        q.put(("ok", dict(hook=hook, xs=xs, stats=st, early=(early0, early1))))
    except Exception as e:  # noqa: BLE001
        import traceback
        q.put(("error", traceback.format_exc() + repr(e)))


def test_gradient_exchange_on_the_instruction_stream_over_rccl():
    """VERDICT r04 item 3a.  `GradAllReducer(exchange_stream="instruction")`: the buckets are packed and all-reduced (synchronous RCCL
    collectives: they run on the caller's current stream, no internal stream) on the policy's own instruction-branch stream, the
    compute streams never wait for a bucket, the early instruction dedup stays on under the process group — and the 30 losses equal,
    bit for bit, those of the round-2 form (hook-stream pack + asynchronous collective).  One-rank RCCL communicator: what a 1-GPU box
    can host of common_trainer.py:60-66."""
    import socket
    import torch.multiprocessing as mp
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    p = ctx.Process(target=_xs_worker, args=(port, q, 30))
    p.start()
    status, info = q.get(timeout=900)
    p.join(timeout=120)
    assert status == "ok", info
    assert info["early"] == (False, True)
    assert len(info["xs"]) == 30 and info["xs"] == info["hook"], [(i, a, b) for i, (a, b) in enumerate(zip(info["xs"], info["hook"])) if a != b][:4]
    assert info["xs"][-1] < info["xs"][0] and info["stats"]["updates"] == 30


# ----------------------------------------------------------------------------- early dense inputs
def test_update_from_raw_depth_does_not_take_the_early_dense_route():
    """the rgb / depth dense inputs ran on the instruction stream behind `entry` only, while the depth embedding is
    written on the main stream after it.  Now the side stream waits for an event recorded behind the encoders and the early route
    needs BOTH cached feature sets: a grad-enabled forward from raw depth (the frozen ResNet50 runs on main) gives the same logits
    as the same forward with the features cached first."""
    import bench
    import test_gpu_round2 as r2
    from wsmgmap.common.aux_losses import AuxLosses
    pol = r2._train_mode(r2._policy(num_proc=1, compute_dtype="bf16", state=r2._default_state()))
    T, N = 4, 2
    obs, prev, masks, weights = bench.synth_batch(T, N, torch.device("cuda"), 9)
    g = torch.Generator(device="cuda").manual_seed(1)
    depth = torch.rand(T * N, 256, 256, 1, device="cuda", generator=g)
    with torch.no_grad():
        feats = pol.net.depth_encoder.visual_encoder({"depth": depth})
    outs = []
    for use_raw in (False, True, True):
        o = dict(obs)
        if use_raw:
            del o["depth_features"]
            o["depth"] = depth
        else:
            o["depth_features"] = feats
        AuxLosses.activate()
        AuxLosses.clear()
        pred, aux = pol(o, torch.zeros(2, N, 512, device="cuda"), prev, masks, weights)
        (pred.sum() + aux).backward()
        torch.cuda.synchronize()
        outs.append(pred.detach().clone())
        for p in pol.parameters():
            p.grad = None
    # (the frozen ResNet50 runs on stock float32 convolutions, which are not bit-reproducible from call to call: one unit in the last
    #  place of the logits was seen between two identical forwards; a read-before-write shows as a difference in the first digits)
    scale = max(1e-3, float(outs[0].abs().max()))
    assert float((outs[1] - outs[2]).abs().max()) <= 1e-5 * scale
    d = float((outs[0] - outs[1]).abs().max())
    assert d <= 1e-4 * scale, (d, scale)


# ----------------------------------------------------------------------------- two tile sizes in one launch
@pytest.mark.parametrize("Cin,Cout,B", [(128, 256, 512), (256, 128, 512), (256, 64, 512), (256, 256, 300)])
def test_mixed_tile_window_convolution_is_bit_identical_to_one_tile_size(Cin, Cout, B):
    """csrc/wsmg_conv_win3.hip, round 5: whole rounds of 512- / 256-pixel tiles and the remainder as half-size tiles in ONE launch
    (map_encoder.py:26,94-112 / mg_map_policy.py:89-100 layers at 24 x 24).  A tile's size changes which workgroup computes a pixel,
    not how: forward and backward-data outputs and the BatchNorm sums' inputs equal the single-tile-size launch bit for bit."""
    from wsmgmap import _abi, ops
    g = torch.Generator(device="cuda").manual_seed(Cin + Cout)
    H = 24
    x = torch.relu(torch.randn(B, H, H, Cin, device="cuda", generator=g)).to(torch.bfloat16)
    w = (torch.randn(Cout, 3, 3, Cin, device="cuda", generator=g) * 0.05).to(torch.bfloat16)
    dy = torch.randn(B, H, H, Cout, device="cuda", generator=g).to(torch.bfloat16)
    wi = w.permute(3, 1, 2, 0).contiguous()
    args = (B, H, H, Cin, Cout, 3, 3, 1, 1, H, H)
    P, st = ops._p, ops._stream
    outs = {}
    for mt in (512, 256, 1):       # 1 = the shape's own choice, which takes the mixed launch where it pays
        old = _abi.lib().wsmg_conv_debug_win3_tile(mt)
        try:
            y = torch.empty(B, H, H, Cout, device="cuda", dtype=torch.bfloat16)
            dx = torch.empty_like(x)
            _abi.call("wsmg_conv2d_fwd_bf16", P(x), P(w), None, P(y), 0, *args, st())
            _abi.call("wsmg_conv2d_bwd_data_bf16", P(dy), P(wi), P(dx), 0, *args, st())
            torch.cuda.synchronize()
            outs[mt] = (y, dx)
        finally:
            _abi.lib().wsmg_conv_debug_win3_tile(old)
    for mt in (512, 256):
        assert torch.equal(outs[1][0], outs[mt][0]) and torch.equal(outs[1][1], outs[mt][1]), mt


# ----------------------------------------------------------------------------- configs[4] in one launch
def test_fp8_shared_attention_in_one_launch_equals_the_three_launch_route(monkeypatch):
    """VERDICT r04 item 4 / BASELINE configs[4] (`_attn`, mg_map_policy.py:173-178, e4m3 storage): wsmg_attn_fp8_mfma_fused — maxima
    behind a grid barrier, quantisation on the fly, ranked row scan, attention — against the round-3 route (maxima launch, quantise +
    group launch, attention launch): context and weights BIT FOR BIT, at configs[4]'s size, at the update path's (512 rows over 8
    sets: the barrier's largest grid), with ragged lengths and an uneven row-to-set map, with the caller's scales (no barrier),
    and over repeated launches of alternating shapes on one stream (the arrival counter's bookkeeping).  Larger batches fall back."""
    from wsmgmap import debug, ops
    import importlib
    att = importlib.import_module("wsmgmap.ops.attention")
    g = torch.Generator(device="cuda").manual_seed(21)

    def case(B, U, L, scales=None):
        q = torch.randn(B, 256, device="cuda", generator=g)
        k = torch.randn(U, L, 256, device="cuda", generator=g) * 1.7
        v = torch.randn(U, L, 256, device="cuda", generator=g) * 0.6
        inv = torch.randint(0, U, (B,), device="cuda", generator=g)
        inv[: min(B, U)] = torch.arange(min(B, U), device="cuda")
        lens = torch.randint(1, L + 1, (U,), device="cuda", generator=g).to(torch.int32)
        monkeypatch.setattr(debug.sw, "fp8_fused", False)
        o3, a3 = ops.attention_fp8_shared(q, k, v, lens, inv, 1 / 16, scales=scales)
        n3 = att.last_fp8_shared_launches
        monkeypatch.setattr(debug.sw, "fp8_fused", True)
        o1, a1 = ops.attention_fp8_shared(q, k, v, lens, inv, 1 / 16, scales=scales)
        n1 = att.last_fp8_shared_launches
        torch.cuda.synchronize()
        return (o3, a3, n3), (o1, a1, n1)

    for rep in range(3):
        for B, U, L, scales, fused in ((64, 8, 160, None, True), (512, 8, 80, None, True), (37, 5, 200, None, True), (3, 3, 33, None, True),
                                       (64, 8, 160, (0.01, 0.02, 0.005), True), (4096, 64, 160, (0.01, 0.02, 0.005), True),
                                       (4096, 64, 160, None, False)):
            (o3, a3, n3), (o1, a1, n1) = case(B, U, L, scales)
            assert n1 == (1 if fused else 3) and n3 == (2 if scales else 3), (B, U, L, n1, n3)
            assert torch.equal(a1, a3), (B, U, L, rep, float((a1 - a3).abs().max()))
            assert torch.equal(o1, o3), (B, U, L, rep, float((o1 - o3).abs().max()))
            assert torch.isfinite(o1).all()


def test_fp8_one_launch_attention_reproduces_the_reference_golden_g5f():
    """The fused launch against golden g5f — the reference's own `_attn` on e4m3-representable inputs at configs[4]'s size."""
    import numpy as np
    from oracle import cases
    from util import golden
    from wsmgmap import ops
    import importlib
    att = importlib.import_module("wsmgmap.ops.attention")
    c = cases.attn_fp8_inputs()
    g = golden("g5f_attn_fp8.npz")
    q, k, v = (torch.from_numpy(c[n]).cuda() for n in ("q", "k", "v"))
    out, attn = ops.attention_fp8_shared(q, k, v, torch.from_numpy(c["lengths"]).cuda(), torch.from_numpy(c["inverse"]).cuda(), 1.0 / 16,
                                         scales=(c["q_scale"], c["k_scale"], c["v_scale"]))
    assert att.last_fp8_shared_launches == 1
    ea = float(np.abs(attn.cpu().numpy() - g["attn"]).max())
    eo = float(np.abs(out.cpu().numpy() - g["out"]).max() / np.abs(g["out"]).max())
    assert ea <= 3e-5 and eo <= 6e-5, (ea, eo)


# ----------------------------------------------------------------------------- the chained recurrent core
@pytest.mark.parametrize("chunks,T,N", [(4, 64, 8), (8, 64, 8), (4, 12, 3)])
def test_chained_recurrent_core_is_bit_identical_to_the_chunk_launch_route(chunks, T, N, monkeypatch):
    """Round 5: each recurrence of the pipelined core as ONE whole-sequence launch, chained to the attention stage's kernels on the
    other streams by per-chunk arrival counters (device-side waits: csrc/wsmg_rnn.hip chain_wait, wsmg_rows_gemm_f32's wait / signal)
    instead of K launches per recurrence ordered by events (mg_map_policy.py:220-249).  Same kernels, same arithmetic in the same
    order: logits, loss, attention row, hidden states and every gradient are equal BIT FOR BIT, three times in a row (a missed
    wait would read a chunk before it is written)."""
    import bench
    import test_gpu_round2 as r2
    import test_gpu_round4 as r4
    from wsmgmap import debug, ops
    pol = r2._train_mode(r2._policy(num_proc=1, compute_dtype="bf16", state=r2._default_state()))
    obs, prev, masks, weights = bench.synth_batch(T, N, torch.device("cuda"), 79)
    masks = masks.clone()
    masks.view(T, N)[T // 2 + 1, N - 1] = 0
    monkeypatch.setattr(debug.sw, "recurrent_chain", False)
    a = r4._one_update(pol, obs, prev, masks, weights, N, chunks)
    monkeypatch.setattr(debug.sw, "recurrent_chain", True)
    for rep in range(3):
        b = r4._one_update(pol, obs, prev, masks, weights, N, chunks)
        ops.check_rnn_status()
        assert torch.equal(a[0], b[0]) and a[1] == b[1], rep
        assert torch.equal(a[2], b[2]) and torch.equal(a[3], b[3]), rep
        for k, g in a[4].items():
            if g is not None:
                assert torch.equal(g, b[4][k]), (rep, k)


# ----------------------------------------------------------------------------- sparse ego map through the device collate
def test_sparse_ego_map_collates_bit_identically_to_the_dense_record():
    """a recoded record with the sparse ego map (codec.sparse_pack_ego: presence bits + packed non-zeros, 0.4-0.6 x
    the PCIe bytes of the float16 map of dagger_trainer.py:336-343) goes through DeviceCollator(ego_map_nhwc_bf16=True) — one expansion
    kernel, wsmg_collate_ego_sparse_nhwc_bf16 — to the SAME padded channels-last bf16 tensor, bit for bit, as the dense record through
    wsmg_collate_pad_nhwc_bf16 (ragged batch, the 200-step cap, a fully empty and a fully dense step, -0.0); every other sensor is
    untouched; a float32 collator refuses the sparse record instead of guessing."""
    from wsmgmap import _abi
    from wsmgmap.data import DeviceCollator, pack_record_raw, unpack_record
    rng = np.random.RandomState(8)
    lengths, C, E = [9, 203, 4], 64, 10
    dense, sparse = [], []
    for n in lengths:
        ego = np.maximum(rng.randn(n, C, E, E), 0.6).astype(np.float16) - np.float16(0.6)
        ego[0] = 0
        ego[1] = (rng.randn(C, E, E) + 3).astype(np.float16)
        ego[2, 7, 3, 3] = np.float16(-0.0)
        obs = {"instruction": rng.randint(0, 27, size=(n, 6)).astype(np.int64), "rgb_ego_map": ego,
               "progress": rng.rand(n, 1).astype(np.float32)}
        rec = (obs, rng.randn(n, 2).astype(np.float32), rng.randn(n, 2).astype(np.float32))
        dense.append(rec + (torch.ones(n),))
        o2, p2, a2 = unpack_record(pack_record_raw(*rec, sparse_ego=True))
        sparse.append(({k: np.asarray(v) for k, v in o2.items()}, np.asarray(p2), np.asarray(a2), torch.ones(n)))
    want_obs, *want_rest = DeviceCollator("cuda", ego_map_nhwc_bf16=True)(dense)
    got_obs, *got_rest = DeviceCollator("cuda", ego_map_nhwc_bf16=True)(sparse)
    torch.cuda.synchronize()
    for a, b in zip(want_rest, got_rest):
        assert torch.equal(a, b)
    assert set(want_obs) == set(got_obs)
    for k in want_obs:
        assert want_obs[k].dtype == got_obs[k].dtype and want_obs[k].shape == got_obs[k].shape, k
        assert torch.equal(want_obs[k].contiguous().view(torch.int16) if want_obs[k].dtype == torch.bfloat16 else want_obs[k],
                           got_obs[k].contiguous().view(torch.int16) if got_obs[k].dtype == torch.bfloat16 else got_obs[k]), k
    ego = got_obs["rgb_ego_map"]
    assert ego.dtype == torch.bfloat16 and ego.permute(0, 2, 3, 1).is_contiguous() and ego.shape[0] == 200 * 3
    with pytest.raises(_abi.WsmgError):
        DeviceCollator("cuda")(sparse)


# ----------------------------------------------------------------------------- map retrieval: one launch through LDS
@pytest.mark.parametrize("B,E,C,G", [(4, 100, 64, 240), (3, 200, 40, 480), (5, 33, 8, 64), (2, 50, 128, 120), (2, 24, 168, 24)],
                         ids=["e100_c64", "e200_c40", "e33_c8", "e50_c128", "e24_c168_g_eq_e"])
def test_map_retrieve_lds_tiles_equal_crop_then_rotate(B, E, C, G):
    """wsmg_map_retrieve_tiled (round 5: ops.map_retrieve's default) against wsmg_map_retrieve — map_crop_kernel then
    rotate_nhwc_kernel (rgb_mapping.py:57-70), the launches which test_map_sequence_vs_oracle pins to the oracle at the G2 geometry and
    tests/test_gpu_map_edges.py at these edges (dense map, axis headings, agents beyond the border, odd E, odd G, G == E, cfg4; all
    three forms of the retrieve against float64) — bit for bit on a DENSE global map (every tap
    carries weight): headings on and between the axes (0, +-pi/4, +-pi/2, pi, random), agents in the centre, at and beyond the map
    border (taps outside the global map), ego sizes that are not multiples of the 8-pixel tile, G == E; one map holds an infinity
    and a NaN (a tap with weight 0 still propagates them the same way), one trial has an infinite gps (the tile geometry does not fit
    the box: the kernel's register route).  Wide maps go as channel slices of <= 40 (C = 64: 2 x 32, 128: 4 x 32, 168: 6 x 28)."""
    from wsmgmap import ops
    g = torch.Generator(device="cuda").manual_seed(17)
    gm = torch.randn(B, G, G, C, device="cuda", generator=g)
    gm[0, G // 2, G // 2, 0] = float("inf")
    gm[0, G // 2 + 3, G // 2 - 2, C - 1] = float("nan")
    half = G * 0.12 / 2
    fixed = [0.0, math.pi / 4, -math.pi / 4, math.pi / 2, -math.pi / 2, math.pi, 3.0, -1.3]
    for trial in range(6):
        compass = torch.tensor([fixed[(trial * B + b) % len(fixed)] for b in range(B)], device="cuda") if trial < 3 else \
            torch.rand(B, device="cuda", generator=g) * 6.28 - 3.14
        reach = [0.0, 0.5, 1.0, 1.4, 0.97, 1.0][trial]
        gps = (torch.rand(B, 2, device="cuda", generator=g) * 2 - 1) * half * reach
        if trial == 5:
            gps[B - 1, 0] = float("inf")
        two = ops.map_retrieve(gm, gps, compass, E, 0.12, fused=False)
        lds = ops.map_retrieve(gm, gps, compass, E, 0.12, fused="tiled")
        same = (lds == two) | (lds.isnan() & two.isnan())
        assert bool(same.all()), f"trial {trial}: {int((~same).sum())} of {same.numel()} elements differ"
        assert torch.equal(lds.view(torch.int32)[~two.isnan()], two.view(torch.int32)[~two.isnan()])   # signed zeros included


# ----------------------------------------------------------------------------- feeder: a ring that outlives the epoch
class _BlobStore:
    def __init__(self, blobs):
        self.blobs = blobs

    def __call__(self, i):
        return self.blobs[i]


def test_persistent_feeder_ring_serves_epoch_after_epoch_from_the_same_processes():
    """DeviceFeeder(persistent=True): the worker processes, the shared slots and their page-locking are built once; every epoch
    delivers exactly what a fresh feeder with the same seed delivers (order and values: common_trainer / dagger_trainer.py:585-594's
    loader re-seeds per epoch, so does this); an epoch abandoned half way takes the ring down and the next one rebuilds it;
    close() is idempotent."""
    from oracle import data_cases as dc
    from wsmgmap.data import TrajectoryDataset, DeviceFeeder, pack_record
    lengths = (dc.DATASET_LENGTHS * 3)[:48]
    store = _BlobStore([pack_record(*dc.episode(2000 + i, n)) for i, n in enumerate(lengths)])
    mk = lambda: TrajectoryDataset(store, len(store.blobs), batch_size=2, rank=0, world_size=1)  # noqa: E731

    def epoch(fd, stop_after=None):
        seen = []
        for n, (ob, prev, masks, corr, wts) in enumerate(fd):
            seen.append((prev.view(-1, 2, 2)[0, :, 0].cpu().tolist(), float(ob["progress"].sum()), float(ob["rgb_ego_map"].float().abs().sum())))
            if stop_after is not None and n + 1 >= stop_after:
                break
        return seen

    fresh = DeviceFeeder(mk(), 2, "cuda", num_workers=2, prefetch=2, seed=9)
    want = [epoch(fresh) for _ in range(3)]
    assert fresh.ring_opens == 3 and fresh._ring is None
    fd = DeviceFeeder(mk(), 2, "cuda", num_workers=2, prefetch=2, seed=9, persistent=True)
    got = [epoch(fd)]
    pids = [p.pid for p in fd._ring["procs"]]
    got += [epoch(fd), epoch(fd)]
    assert got == want
    assert fd.ring_opens == 1 and [p.pid for p in fd._ring["procs"]] == pids and all(p.is_alive() for p in fd._ring["procs"])
    procs = fd._ring["procs"]
    part = epoch(fd, stop_after=2)                      # abandoned: the generator is closed with batches in flight
    assert len(part) == 2 and fd._ring is None
    for p in procs:
        p.join(timeout=10)
        assert not p.is_alive()
    again = epoch(fd)                                   # epoch counter went on: this is epoch 4 of seed 9
    flat = lambda ep: sorted(x for a in ep for x in a[0])  # noqa: E731  (the episodes of an epoch, however they were paired into batches)
    assert fd.ring_opens == 2 and len(again) == len(want[0]) and flat(again) == flat(want[0])
    fd.close()
    fd.close()
    assert fd._ring is None


# ----------------------------------------------------------------------------- a chained product must not starve what it waits for
def test_chained_product_waits_with_one_workgroup_not_with_its_whole_grid():
    """The first product of a chunk of the chained recurrent core waits, on the device, for a counter that a kernel on ANOTHER stream
    advances (wsmgmap/recurrent.py, csrc/wsmg_rnn.hip chain_signal).  That producer may need whole CUs — the persistent recurrences
    need all 32 of their workgroups resident at once — so the wait must not hold the chip.  Here the producer stream is enqueued
    first, as the product code does (a waiter behind its producer in host order cannot deadlock even where two streams share a
    hardware queue), but its work starts late: a 30 ms delay kernel, then 256 whole-CU workgroups (wsmg_debug_occupy: 1 024 threads
    + 160 KB of LDS each), then the counter.  The waiting product — 768 workgroups of 16 waves: every wave slot of the GPU if they
    all spun — is on the GPU long before that.  With the wait inside the product the whole-CU kernel could not start until the
    product's spin timed out (round 5's first form: this test failed with a timeout); with the one-workgroup gate launch in front of the
    product (round 5; round 6: its verdict in the caller's word, and the whole-grid form is gone) it runs, the counter moves, the product follows — no timeout, the same numbers as unchained."""
    from wsmgmap import _abi, ops, recurrent
    g = torch.Generator(device="cuda").manual_seed(3)
    M, K, N = 128, 1536, 1536
    a = torch.randn(M, K, device="cuda", generator=g)
    w = torch.randn(K, N, device="cuda", generator=g) * 0.05      # [K, N]: the backward form (w_is_kn)
    mask = torch.rand(M, N, device="cuda", generator=g)
    want = torch.zeros(M, N, device="cuda")
    recurrent._rg([a], w, True, [want], 0, M, mask=mask)
    ops.check_rnn_status()
    cnt = torch.zeros(1, dtype=torch.int32, device="cuda")
    gate = torch.full((1,), 7, dtype=torch.int32, device="cuda")      # (round 6: the gate's verdict travels through the CALLER's word)
    stop = torch.zeros(1, dtype=torch.int32, device="cuda")
    arrived = torch.zeros(1, dtype=torch.int32, device="cuda")
    got = torch.zeros(M, N, device="cuda")
    s_wait, s_prod = torch.cuda.Stream(), torch.cuda.Stream()
    torch.cuda.synchronize()
    import time
    t0 = time.time()
    with torch.cuda.stream(s_prod):
        torch.cuda._sleep(60_000_000)          # ~30 ms: the producer's kernels reach the GPU after the waiter has settled in
        _abi.call("wsmg_debug_occupy", 256, 160 * 1024, 20, ops._p(stop), ops._p(arrived), ops._stream())   # 256 whole CUs for 20 ms
        cnt.fill_(1)
    with torch.cuda.stream(s_wait):
        recurrent._rg([a], w, True, [got], 0, M, mask=mask, wait=(cnt.data_ptr(), 1, gate.data_ptr()), fail_bit=2)
    torch.cuda.synchronize()
    dt = time.time() - t0
    assert int(arrived) == 256, "the whole-CU workgroups did not all get a CU"
    ops.check_rnn_status()                 # raises if the wait timed out
    assert torch.equal(got, want) and int(gate) == 0
    assert dt < 1.0, f"{dt:.2f} s: the producer only ran after the waiter's spin gave up"
