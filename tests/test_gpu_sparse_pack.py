"""The sparse form of the ego map written on the device (wsmg_ego_sparse_pack / ops.ego_sparse_pack / SparseEgoRecorder) against the
host codec: `codec.sparse_pack_ego` of the map cast to float16 by NumPy is the yardstick, and every output is compared bit for bit."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

C = 64
CONTENTS = ("zero", "dense", "relu30", "first", "last")


def _row(kind, H, W, rng):
    """One float32 row [H, W, 64] (channels-last)."""
    if kind == "zero":
        return np.zeros((H, W, C), dtype=np.float32)
    if kind == "dense":
        return (rng.rand(H, W, C) + 0.5).astype(np.float32) * np.where(rng.rand(H, W, C) < 0.5, -1, 1).astype(np.float32)
    if kind == "relu30":                               # post-ReLU: P(z > 0.52) = 0.30
        return np.maximum(rng.randn(H, W, C) - 0.52, 0).astype(np.float32)
    x = np.zeros((H, W, C), dtype=np.float32)
    if kind == "first":
        x[0, 0, 0] = 0.75
    else:
        x[H - 1, W - 1, C - 1] = -2.5
    return x


def _want(x_nchw):
    """The yardstick: the host codec on the float16 map; T = the rows of the call."""
    from wsmgmap.data import sparse_pack_ego
    with np.errstate(over="ignore"):
        return sparse_pack_ego(x_nchw.cpu().numpy().astype(np.float16))


def _host(out):
    bits, off, nnz, vals = out
    torch.cuda.synchronize()
    return bits.cpu().numpy(), off.cpu().numpy(), nnz.cpu().numpy(), vals.cpu().numpy()


def _assert_equal(out, want, note=""):
    bits, off, nnz, vals = _host(out)
    B = bits.shape[0]
    base = want["rgb_ego_map__base"]
    assert bits.dtype == np.uint8 and off.dtype == np.uint32 and nnz.dtype == np.int64 and vals.dtype == np.float16
    assert bits.shape == want["rgb_ego_map__bits"].shape and off.shape == want["rgb_ego_map__off"].shape
    assert vals.shape == (B, bits.shape[1] * C)
    assert np.array_equal(nnz, np.diff(base)), note
    assert np.array_equal(bits, want["rgb_ego_map__bits"]), note
    assert np.array_equal(off, want["rgb_ego_map__off"]), note
    for b in range(B):
        got = vals[b, :int(nnz[b])].view(np.uint16)
        assert np.array_equal(got, want["rgb_ego_map__vals"][base[b]:base[b + 1]].view(np.uint16)), (note, b)


def _map(kinds, H, W, seed):
    """The rows as `observations['rgb_ego_map']` holds them: [B, 64, H, W] over channels-last memory."""
    rng = np.random.RandomState(seed)
    nhwc = torch.from_numpy(np.stack([_row(k, H, W, rng) for k in kinds])).cuda()
    return nhwc.permute(0, 3, 1, 2)


@pytest.mark.parametrize("B,H,W", [(1, 1, 1), (3, 5, 7), (2, 31, 33), (2, 25, 41)])
def test_pack_is_the_codec_bit_for_bit(B, H, W):
    """Every row content next to every other one in the same call: call k holds contents k, k + 1, ... of CONTENTS.  1023 pixels:
    one short of a trip of the scan workgroup; 1025: one past it (the carried prefix); 35 and 1: fewer pixels than a workgroup's 64."""
    from wsmgmap import ops
    for k in range(len(CONTENTS)):
        kinds = [CONTENTS[(k + b) % len(CONTENTS)] for b in range(B)]
        x = _map(kinds, H, W, seed=100 * H + k)
        _assert_equal(ops.ego_sparse_pack(x), _want(x), note=kinds)


def test_pack_at_the_rollout_size():
    from wsmgmap import ops
    x = _map(["relu30", "last"], 100, 100, seed=7)
    want = _want(x)
    share = want["rgb_ego_map__base"][1] / (100 * 100 * C)
    assert 0.25 < share < 0.35                       # the content is what the case says it is
    _assert_equal(ops.ego_sparse_pack(x), want)


def test_values_that_decide_the_cast():
    """float32 -> float16 as NumPy casts: round to nearest even, overflow to inf, subnormals kept; present iff the float16 bit pattern
    is not 0.  The expected patterns are written out, and the yardstick is held to them too."""
    from wsmgmap import ops
    cases = [(1e-9, None), (-1e-9, 0x8000), (-0.0, 0x8000), (3e-6, 0x0032), (65504.0, 0x7BFF), (65520.0, 0x7C00), (1e6, 0x7C00),
             (1 + 2.0 ** -11, 0x3C00), (1 + 3 * 2.0 ** -11, 0x3C02), (-65520.0, 0xFC00), (2.0 ** -25, None), (1.5 * 2.0 ** -25, 0x0001),
             (0.0, None)]
    H, W = 2, 3
    x = np.zeros((1, H, W, C), dtype=np.float32)
    x[0, 0, 0, :len(cases)] = [v for v, _ in cases]                 # first pixel, channels 0 ..
    x[0, H - 1, W - 1, C - len(cases):] = [v for v, _ in cases]     # last pixel, channels .. 63
    xd = torch.from_numpy(x).cuda()
    out = ops.ego_sparse_pack(xd)
    want = _want(xd.permute(0, 3, 1, 2))
    _assert_equal(out, want)
    bits, off, nnz, vals = _host(out)
    word = sum(1 << c for c, (_, h) in enumerate(cases) if h is not None)
    pattern = [h for _, h in cases if h is not None]
    words = bits.reshape(H * W, 8).view("<u8").reshape(-1)
    assert int(words[0]) == word and int(words[-1]) == word << (C - len(cases)) and not words[1:-1].any()
    assert int(nnz[0]) == 2 * len(pattern)
    assert list(off[0]) == [0] + [len(pattern)] * (H * W - 1)
    assert list(vals[0, :int(nnz[0])].view(np.uint16)) == pattern + pattern


def test_channels_last_view_and_plain_nhwc_agree_and_runs_repeat():
    from wsmgmap import ops
    rng = np.random.RandomState(11)
    E = 12
    nhwc = torch.from_numpy(np.stack([_row("relu30", E, E, rng), _row("dense", E, E, rng)])).cuda()
    view = torch.empty(2, C, E, E, device="cuda").contiguous(memory_format=torch.channels_last)
    view.copy_(nhwc.permute(0, 3, 1, 2))
    assert not view.is_contiguous() and view.permute(0, 2, 3, 1).is_contiguous()
    a, b, again = _host(ops.ego_sparse_pack(nhwc)), _host(ops.ego_sparse_pack(view)), _host(ops.ego_sparse_pack(nhwc))
    _assert_equal(ops.ego_sparse_pack(view), _want(view))
    for other in (b, again):
        for k in range(3):
            assert np.array_equal(a[k], other[k])
        for r in range(2):
            n = int(a[2][r])
            assert np.array_equal(a[3][r, :n].view(np.uint16), other[3][r, :n].view(np.uint16))


def test_wrapper_refuses_what_the_format_does_not_cover():
    from wsmgmap import _abi, ops
    for bad in (torch.zeros(2, 5, 7, 40, device="cuda"),                                   # C = 40: stays on the dense route
                torch.zeros(2, 5, 7, C, device="cuda", dtype=torch.float16),
                torch.zeros(2, 5, 7, C),                                                    # a CPU tensor
                torch.zeros(2, C, 5, 7, device="cuda"),                                     # NCHW memory
                torch.zeros(2, 5, 7, 2 * C, device="cuda")[..., ::2]):                      # strided channels
        with pytest.raises(_abi.WsmgError):
            ops.ego_sparse_pack(bad)


def test_recorded_steps_collate_like_the_host_route():
    """Rollout steps through SparseEgoRecorder, a subsample of them taken and written as a record, against the host route for the same
    maps (dense float16 copy, pack_record_raw(sparse_ego=True)): the same bytes on disk and, through
    DeviceCollator(ego_map_nhwc_bf16=True), the same tensors."""
    from wsmgmap.data import DeviceCollator, SparseEgoRecorder, pack_record_raw, unpack_record
    rng = np.random.RandomState(21)
    T, N, E, idx = 5, 2, 10, [1, 3, 4]
    rec = SparseEgoRecorder(N, "cuda")
    dense = [[] for _ in range(N)]
    for t in range(T):
        kinds = [("zero", "relu30"), ("relu30", "dense"), ("relu30", "first"), ("last", "relu30"), ("dense", "zero")][t]
        nhwc = torch.from_numpy(np.stack([_row(k, E, E, rng) for k in kinds])).cuda()
        ego = nhwc.permute(0, 3, 1, 2)                  # as the mapping module leaves observations['rgb_ego_map']
        rec.append(ego)
        for n in range(N):
            dense[n].append(ego[n].cpu().numpy().astype(np.float16))
    extra = torch.from_numpy(_row("relu30", E, E, rng)[None]).cuda()
    rec.append(extra, rows=[1])                         # environment 0 is paused: the batch holds environment 1 alone
    dense[1].append(extra[0].permute(2, 0, 1).cpu().numpy().astype(np.float16))
    assert rec.steps(0) == T and rec.steps(1) == T + 1 and len(rec) == 2 * T + 1
    got_batch, want_batch = [], []
    for n, steps in ((0, idx), (1, None)):
        sel = idx if steps is not None else list(range(T + 1))
        k = len(sel)
        other = {"instruction": rng.randint(0, 27, size=(k, 6)).astype(np.int64), "progress": rng.rand(k, 1).astype(np.float32)}
        prev, oracle = rng.randn(k, 2).astype(np.float32), rng.randn(k, 2).astype(np.float32)
        got = pack_record_raw({**other, **rec.take(n, steps)}, prev, oracle)
        want = pack_record_raw({**other, "rgb_ego_map": np.stack(dense[n])[sel]}, prev, oracle, sparse_ego=True)
        assert got == want, n
        for blob, batch in ((got, got_batch), (want, want_batch)):
            o, p, a = unpack_record(blob)
            batch.append(({k_: np.asarray(v) for k_, v in o.items()}, np.asarray(p), np.asarray(a), torch.ones(k)))
    rec.reset(0)
    assert rec.steps(0) == 0 and len(rec) == T + 1
    got_obs, *got_rest = DeviceCollator("cuda", ego_map_nhwc_bf16=True)(got_batch)
    want_obs, *want_rest = DeviceCollator("cuda", ego_map_nhwc_bf16=True)(want_batch)
    torch.cuda.synchronize()
    for a, b in zip(want_rest, got_rest):
        assert torch.equal(a, b)
    assert set(want_obs) == set(got_obs)
    as_bits = lambda v: v.contiguous().view(torch.int16) if v.dtype == torch.bfloat16 else v   # noqa: E731
    for k in want_obs:
        assert torch.equal(as_bits(want_obs[k]), as_bits(got_obs[k])), k
    ego = got_obs["rgb_ego_map"]
    assert ego.dtype == torch.bfloat16 and ego.shape == ((T + 1) * N, C, E, E)
