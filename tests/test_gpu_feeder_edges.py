"""The four kernels every update reads its inputs through, at their edges and against references that are not the project's own:
collate_pad_kernel<DT, V>, collate_pad_nhwc_bf16_kernel, collate_ego_sparse_nhwc_bf16_kernel (csrc/wsmg_collate.hip) and
instruction_dedup_kernel<T> (csrc/wsmg_dedup.hip).  Cases and references: tests/feeder_cases.py (held to their own conditions by
tests/test_feeder_cases_cpu.py).  Every comparison is exact: int32 views of float32 outputs and int16 views of bf16 outputs, so that
-0.0 and NaN compare by their bits; integers for the dedup.

Two entry points.  Through DeviceCollator (both ego_map_nhwc_bf16 settings) wherever it can express the case: plan_batch, pack_batch, the
pointer table and the launch arguments are then under test too.  Directly through _abi.call for everything, because only there can the
output buffer carry a guard: it is allocated with one extra row, filled with a sentinel before the launch and found intact after it
(a store past HW or past row T N - 1 shows), each launch is repeated on the same inputs, and a further launch goes into a buffer of
NaN patterns so that an element nobody writes cannot pass by luck.  The direct calls also reach what the collator never asks for: a
pad value of 0 on an observation, an episode of length 0, C = 128 and 192."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import feeder_cases as fc

pytestmark = pytest.mark.gpu

SENTINEL = {torch.int32: 0x7FC0DEAD, torch.int16: 0xDEAD - (1 << 16)}      # in no reference (asserted)
NAN_FILL = {torch.int32: 0x7FC00001, torch.int16: 0x7FC1}                  # NaN patterns no conversion produces
P = lambda t: ctypes.c_void_p(t.data_ptr())                                 # noqa: E731


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _bits(t):
    t = t.contiguous()
    return t.view(torch.int32) if t.dtype == torch.float32 else t.view(torch.int16) if t.dtype == torch.bfloat16 else t


def _table(arrs):
    """The arrays on the device, one allocation each (16-byte aligned: asserted), and the table of their addresses."""
    keep = [torch.from_numpy(np.ascontiguousarray(a).reshape(-1).view(np.uint8)).cuda() for a in arrs]
    assert all(k.data_ptr() % 16 == 0 for k in keep)
    return keep, torch.tensor([k.data_ptr() for k in keep], dtype=torch.int64).cuda()


def _guarded(rows, row_elems, dtype, fill):
    return torch.full((rows + 1, row_elems), fill, dtype=dtype, device="cuda")


def _check(buf, want, fill, note):
    """buf [rows + 1, row_elems] after a launch: the rows equal the reference, the guard row is as it was filled."""
    torch.cuda.synchronize()
    rows = buf.shape[0] - 1
    want = _bits(want).reshape(rows, -1)
    assert not bool((want == fill).any()), note
    got = buf[:rows].cpu()
    assert torch.equal(got, want), f"{note}: {_differences(got, want)}"
    assert bool((buf[rows] == fill).all()), f"{note}: a store past the last row"


def _differences(got, want, most=12):
    """Where two [rows, row_elems] pattern tensors differ: the count and the first few (row, element, got, want)."""
    where = (got != want).nonzero()
    mask = 0xFFFF if got.dtype == torch.int16 else 0xFFFFFFFF
    some = [f"[{int(r)}, {int(e)}] {int(got[r, e]) & mask:#x} for {int(want[r, e]) & mask:#x}" for r, e in where[:most]]
    return f"{len(where)} of {got.numel()} elements differ: " + "; ".join(some)


def _three_launches(launch, rows, row_elems, dtype, want, note):
    """Sentinel-filled buffer; the same again (equal results); then a buffer of NaN patterns."""
    first = _guarded(rows, row_elems, dtype, SENTINEL[dtype])
    launch(first)
    _check(first, want, SENTINEL[dtype], note)
    again = _guarded(rows, row_elems, dtype, SENTINEL[dtype])
    launch(again)
    torch.cuda.synchronize()
    assert torch.equal(first, again), f"{note}: two launches differ"
    nan = _guarded(rows, row_elems, dtype, NAN_FILL[dtype])
    launch(nan)
    _check(nan, want, NAN_FILL[dtype], f"{note} (into NaN patterns)")


@functools.lru_cache(maxsize=None)
def _stride_ref(i):
    """The grid-stride cases' references, built once for the module and left unchanged."""
    c = fc.stride_pad_cases()[i]
    return _bits(fc.collate_ref(c.eps, c.lengths, c.T, 1.0))


# ------------------------------------------------------------------------------------------------------- collate_pad_kernel<DT, V>
def _pad_launcher(c):
    from wsmgmap import _abi
    keep, ptrs = _table(c.eps)
    lens = torch.tensor(c.lengths, dtype=torch.int32).cuda()

    def launch(buf, pad):
        _abi.call("wsmg_collate_pad", P(ptrs), P(lens), c.N, c.T, c.elems, fc.DT_CODE[c.dtype], float(pad), P(buf), _stream())
        return keep
    return launch


@pytest.mark.parametrize("zero_length", [False, True], ids=["ragged", "len0"])
@pytest.mark.parametrize("form", range(len(fc.SMALL_FORMS)), ids=[f[0] for f in fc.SMALL_FORMS])
def test_collate_pad_converts_every_dtype_in_both_vector_widths(form, zero_length):
    """Every source dtype in the 4-element and the 1-element form, its value set at both ends of every episode, pad 1 and pad 0;
    with an episode of length 0 whose (valid) pointer is never read and whose rows are all pad."""
    c = fc.small_pad_cases(zero_length)[form]
    launch = _pad_launcher(c)
    for pad in fc.PADS:
        want = fc.collate_ref(c.eps, c.lengths, c.T, pad)
        _three_launches(lambda buf: launch(buf, pad), c.T * c.N, c.elems, torch.int32, want, (c.name, pad))


@pytest.mark.parametrize("i", [0, 1], ids=["f16.v4", "f32.v1"])
def test_collate_pad_grid_stride_trips(i):
    """More work items than 16384 x 256: the second trip's `i / per_row` and `row * elems + e` in 64-bit arithmetic."""
    c = fc.stride_pad_cases()[i]
    assert c.work_items > fc.GRID_CAP_ITEMS
    launch = _pad_launcher(c)
    first = _guarded(c.T * c.N, c.elems, torch.int32, SENTINEL[torch.int32])
    launch(first, 1.0)
    _check(first, _stride_ref(i), SENTINEL[torch.int32], c.name)
    nan = _guarded(c.T * c.N, c.elems, torch.int32, NAN_FILL[torch.int32])
    launch(nan, 1.0)
    torch.cuda.synchronize()
    assert torch.equal(first[:-1], nan[:-1]) and bool((nan[-1] == NAN_FILL[torch.int32]).all()), c.name


def _collate(batch, nhwc=False):
    from wsmgmap.data import DeviceCollator
    out = DeviceCollator("cuda", ego_map_nhwc_bf16=nhwc)(batch)
    torch.cuda.synchronize()
    return out


def _check_actions(out, batch, lengths, T):
    """prev_actions, oracle actions and weights: float32 sources, 2 and 1 elements per row (V = 1), pad 0; and the masks."""
    obs, prev, masks, corr, wts = out
    N = len(batch)
    for got, k, shape in ((prev, 1, (T * N, 2)), (corr, 2, (T, N, 2)), (wts, 3, (T, N))):
        assert got.dtype == torch.float32 and got.shape == shape and got.is_contiguous()
        assert torch.equal(_bits(got).cpu().reshape(-1), _bits(fc.collate_ref([b[k] for b in batch], lengths, T, 0.0)).reshape(-1))
    assert torch.equal(masks.cpu(), torch.cat([torch.zeros(1, N), torch.ones(T - 1, N)]).view(-1, 1))


def test_collator_float32_route_on_every_dtype():
    cases = fc.small_pad_cases()
    batch = fc.batch_of(cases)
    T, N, lengths = cases[0].T, cases[0].N, cases[0].lengths
    out = _collate(batch)
    again = _collate(batch)
    assert set(out[0]) == {c.name for c in cases}
    for c in cases:
        got = out[0][c.name]
        assert got.dtype == torch.float32 and got.shape == (T * N,) + c.shape and got.is_contiguous()
        assert torch.equal(_bits(got).cpu(), _bits(fc.collate_ref(c.eps, lengths, T, 1.0)).reshape(got.shape)), c.name
        assert torch.equal(_bits(got), _bits(again[0][c.name])), c.name
    _check_actions(out, batch, lengths, T)


@pytest.mark.parametrize("i", [0, 1], ids=["f16.v4", "f32.v1"])
def test_collator_grid_stride_trips(i):
    c = fc.stride_pad_cases()[i]
    batch = fc.batch_of([c])
    out = _collate(batch)
    got = out[0][c.name]
    assert got.dtype == torch.float32 and got.shape == (c.T * c.N,) + c.shape and got.is_contiguous()
    assert torch.equal(_bits(got).cpu(), _stride_ref(i).reshape(got.shape)), c.name
    _check_actions(out, batch, c.lengths, c.T)


# ---------------------------------------------------------------------------------------------------- collate_pad_nhwc_bf16_kernel
NHWC_IDS = [f"C{C}.{H}x{W}" for C, H, W in fc.NHWC_SHAPES]


@pytest.mark.parametrize("i", range(len(fc.NHWC_SHAPES)), ids=NHWC_IDS)
def test_collate_nhwc_bf16_channel_and_pixel_tiles(i):
    """One, two and three channel tiles; a partial pixel tile alone (HW = 4, 20, 60), none (64, 128), full and partial (100)."""
    from wsmgmap import _abi
    c = fc.nhwc_cases()[i]
    C, H, W = c.shape
    keep, ptrs = _table(c.eps)
    lens = torch.tensor(c.lengths, dtype=torch.int32).cuda()
    for pad in fc.PADS:
        want = fc.collate_ref(c.eps, c.lengths, c.T, pad, "nhwc_bf16")
        assert want.shape == (c.T, c.N, H * W, C)
        _three_launches(lambda buf: _abi.call("wsmg_collate_pad_nhwc_bf16", P(ptrs), P(lens), c.N, c.T, C, H * W, float(pad), P(buf), _stream()),
                        c.T * c.N, H * W * C, torch.int16, want, (c.name, pad))


@pytest.mark.parametrize("i", range(len(fc.NHWC_SHAPES)), ids=NHWC_IDS)
def test_collator_ego_map_in_both_settings(i):
    """`rgb_ego_map` through DeviceCollator: channels-last bf16 with ego_map_nhwc_bf16, float32 NCHW without."""
    c = fc.nhwc_cases()[i]
    C, H, W = c.shape
    batch = fc.batch_of([c], names=["rgb_ego_map"])
    out = _collate(batch, nhwc=True)
    got = out[0]["rgb_ego_map"]
    assert got.dtype == torch.bfloat16 and got.shape == (c.T * c.N, C, H, W)
    nhwc = got.permute(0, 2, 3, 1)
    assert nhwc.is_contiguous()                                                   # channels-last memory under the NCHW shape
    want = fc.collate_ref(c.eps, c.lengths, c.T, 1.0, "nhwc_bf16")
    assert torch.equal(nhwc.view(torch.int16).cpu().reshape(want.shape), want), c.name
    assert torch.equal(nhwc.view(torch.int16), _collate(batch, nhwc=True)[0]["rgb_ego_map"].permute(0, 2, 3, 1).view(torch.int16))
    _check_actions(out, batch, c.lengths, c.T)
    plain = _collate(batch, nhwc=False)[0]["rgb_ego_map"]
    assert plain.dtype == torch.float32 and plain.shape == (c.T * c.N, C, H, W) and plain.is_contiguous()
    assert torch.equal(_bits(plain).cpu(), _bits(fc.collate_ref(c.eps, c.lengths, c.T, 1.0)).reshape(plain.shape)), c.name
    # the route the channels-last kernel replaces, on the device: the float32 collate, then torch's NCHW float32 -> NHWC bf16 pass
    # (this is what fixes the reference's pattern for a NaN: feeder_cases._bf16_bits)
    route = plain.permute(0, 2, 3, 1).contiguous().bfloat16().view(torch.int16)
    assert torch.equal(route, nhwc.view(torch.int16)), f"{c.name}: {_differences(route.cpu().reshape(c.T * c.N, -1), want.reshape(c.T * c.N, -1))}"


# --------------------------------------------------------------------------------------------- collate_ego_sparse_nhwc_bf16_kernel
SPARSE_IDS = [f"{H}x{W}" for H, W in fc.SPARSE_SHAPES]


@functools.lru_cache(maxsize=None)
def _sparse_ref(i, pad):
    c = fc.sparse_cases()[i]
    return fc.sparse_collate_ref(c.records, c.lengths, c.T, pad)


@pytest.mark.parametrize("i", range(len(fc.SPARSE_SHAPES)), ids=SPARSE_IDS)
def test_sparse_expansion_at_every_pixel_count(i):
    """HW = 1, 15, 49, 135 (groups of four pixels that straddle HW), 64 and 100; presence words 0, 1, 1 << 63 and all ones; a stored
    -0.0; an episode whose last live step is followed by its pad rows."""
    from wsmgmap import _abi
    c = fc.sparse_cases()[i]
    tables = [_table([np.asarray(r["rgb_ego_map__" + k]) for r in c.records]) for k in ("bits", "off", "base", "vals")]
    lens = torch.tensor(c.lengths, dtype=torch.int32).cuda()
    for pad in fc.PADS:
        want = _sparse_ref(i, pad)
        assert (int(want[5, 0, 0, 5]) & 0xFFFF) == 0x8000                          # the stored -0.0 keeps its sign
        _three_launches(lambda buf: _abi.call("wsmg_collate_ego_sparse_nhwc_bf16", *(P(t[1]) for t in tables), P(lens), c.N, c.T, 64, c.HW,
                                              float(pad), P(buf), _stream()),
                        c.T * c.N, c.HW * 64, torch.int16, want, (c.name, pad))


@pytest.mark.parametrize("i", range(len(fc.SPARSE_SHAPES)), ids=SPARSE_IDS)
def test_collator_expands_the_sparse_record(i):
    from wsmgmap import _abi
    from wsmgmap.data import DeviceCollator
    c = fc.sparse_cases()[i]
    batch = fc.sparse_batch(c)
    out = _collate(batch, nhwc=True)
    assert set(out[0]) == {"rgb_ego_map"}
    got = out[0]["rgb_ego_map"]
    assert got.dtype == torch.bfloat16 and got.shape == (c.T * c.N, 64, c.H, c.W)
    nhwc = got.permute(0, 2, 3, 1)
    assert nhwc.is_contiguous()
    want = _sparse_ref(i, 1.0)
    assert torch.equal(nhwc.view(torch.int16).cpu().reshape(want.shape), want), c.name
    assert torch.equal(nhwc.view(torch.int16), _collate(batch, nhwc=True)[0]["rgb_ego_map"].permute(0, 2, 3, 1).view(torch.int16))
    _check_actions(out, batch, c.lengths, c.T)
    with pytest.raises(_abi.WsmgError, match="ego_map_nhwc_bf16=True"):           # the float32 route has no sparse form
        DeviceCollator("cuda")(batch)
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------- instruction_dedup_kernel<T>
DEDUP = [(name, dt) for name, _, dts in fc.dedup_cases() for dt in dts]


@functools.lru_cache(maxsize=None)
def _dedup_case(name):
    tok = next(t for n, t, _ in fc.dedup_cases() if n == name)
    return tok, fc.dedup_ref(tok)


def _dedup_direct(tok, fill=-7):
    """wsmg_instruction_dedup into sentinel-filled buffers with a guard row each: (uniq [B + 1, L], inverse [B + 1], meta [2 + B + 1])."""
    from wsmgmap import _abi
    B, L = tok.shape
    uniq = torch.full((B + 1, L), fill, dtype=torch.int64, device="cuda")
    inverse = torch.full((B + 1,), fill, dtype=torch.int64, device="cuda")
    meta = torch.full((2 + B + 1,), fill, dtype=torch.int64, device="cuda")
    _abi.call("wsmg_instruction_dedup", P(tok), int(tok.dtype == torch.float32), B, L, P(uniq), P(inverse), P(meta), _stream())
    torch.cuda.synchronize()
    return uniq.cpu(), inverse.cpu(), meta.cpu()


@pytest.mark.parametrize("name,dtype", DEDUP, ids=[f"{n}.{d}" for n, d in DEDUP])
def test_dedup_at_its_row_count_length_and_hash_edges(name, dtype):
    """B around the 1024-row chunk of the rank scan and at the 4096-row limit, L = 1 and around the 64-lane hash stride, rows that differ
    at token 64 or at the last token only, zero rows, and (int64) different rows with the same 64-bit hash."""
    from wsmgmap.models.encoders.instruction_encoder import InstructionEncoder
    tok_np, (ref_u, ref_inv, ref_len) = _dedup_case(name)
    B, L = tok_np.shape
    U = len(ref_u)
    tokens = torch.from_numpy(tok_np)
    tok = tokens.to(getattr(torch, dtype)).cuda()
    uniq, inverse, len_host, len_dev = InstructionEncoder._dedup_fused(tok)
    torch.cuda.synchronize()
    assert uniq.dtype == inverse.dtype == len_host.dtype == len_dev.dtype == torch.int64
    assert uniq.shape == (U, L) and inverse.shape == (B,) and len_host.shape == (U,) and not len_host.is_cuda
    assert torch.equal(uniq.cpu(), torch.from_numpy(ref_u))
    assert torch.equal(inverse.cpu(), torch.from_numpy(ref_inv))
    assert torch.equal(len_host, torch.from_numpy(ref_len)) and torch.equal(len_dev.cpu(), len_host)
    assert torch.equal(uniq[inverse].cpu(), tokens)
    # the same launch into guarded buffers: meta[0], meta[1], nothing written past row U - 1 of uniq, past inverse[B - 1] or meta[1 + U]
    for _ in range(2):
        u, inv, meta = _dedup_direct(tok)
        assert int(meta[0]) == U and int(meta[1]) == int(ref_len.max())
        assert torch.equal(meta[2:2 + U], len_host) and bool((meta[2 + U:] == -7).all())
        assert torch.equal(u[:U], uniq.cpu()) and bool((u[U:] == -7).all())
        assert torch.equal(inv[:B], inverse.cpu()) and int(inv[B]) == -7


def test_colliding_rows_stay_two_instructions():
    name = next(n for n, _ in DEDUP if "collisions" in n)
    tok_np, (ref_u, ref_inv, _) = _dedup_case(name)
    a1, b1, a2, b2 = fc.collision_rows()
    assert fc.row_hash(a1) == fc.row_hash(b1) and fc.row_hash(a2) == fc.row_hash(b2)
    u, inv, meta = _dedup_direct(torch.from_numpy(tok_np).cuda())
    U = int(meta[0])
    assert U == len(ref_u) == 5
    for a, b in ((a1, b1), (a2, b2)):
        ia = [int(inv[r]) for r in range(len(tok_np)) if np.array_equal(tok_np[r], a)]
        ib = [int(inv[r]) for r in range(len(tok_np)) if np.array_equal(tok_np[r], b)]
        assert len(set(ia)) == 1 and len(set(ib)) == 1 and ia[0] != ib[0]
        assert np.array_equal(u[ia[0]].numpy(), a) and np.array_equal(u[ib[0]].numpy(), b)
    assert torch.equal(inv[:-1], torch.from_numpy(ref_inv))


# ------------------------------------------------------------------------------------------------------------------------ refusals
def test_launchers_refuse_what_the_kernels_do_not_cover():
    """WSMG_EINVAL, nothing queued, the output buffer untouched."""
    from wsmgmap import _abi
    c = fc.nhwc_cases()[0]
    keep, ptrs = _table(c.eps + c.eps)
    lens = torch.tensor(c.lengths + c.lengths, dtype=torch.int32).cuda()
    out = torch.full((4096,), SENTINEL[torch.int32], dtype=torch.int32, device="cuda")
    refused = [
        ("wsmg_collate_pad_nhwc_bf16", (P(ptrs), P(lens), c.N, c.T, 96, 4, 1.0, P(out), _stream())),           # C = 96
        ("wsmg_collate_pad_nhwc_bf16", (P(ptrs), P(lens), c.N, c.T, 64, 6, 1.0, P(out), _stream())),           # HW = 6
        ("wsmg_collate_pad_nhwc_bf16", (P(ptrs), P(lens), 2, 32768, 64, 4, 1.0, P(out), _stream())),           # T N = 65536
        ("wsmg_collate_ego_sparse_nhwc_bf16", (P(ptrs), P(ptrs), P(ptrs), P(ptrs), P(lens), c.N, c.T, 128, 4, 1.0, P(out), _stream())),   # C = 128
        ("wsmg_collate_ego_sparse_nhwc_bf16", (P(ptrs), P(ptrs), P(ptrs), P(ptrs), P(lens), 2, 32768, 64, 4, 1.0, P(out), _stream())),   # T N = 65536
        ("wsmg_collate_pad", (P(ptrs), P(lens), c.N, c.T, 4, 4, 1.0, P(out), _stream())),                      # an unknown dtype code
        ("wsmg_collate_pad", (P(ptrs), P(lens), c.N, c.T, 4, -1, 1.0, P(out), _stream())),
        ("wsmg_instruction_dedup", (P(out), 0, fc.DD_MAX_ROWS + 1, 1, P(out), P(out), P(out), _stream())),     # B = 4097
    ]
    for name, args in refused:
        with pytest.raises(_abi.WsmgError, match="WSMG_EINVAL"):
            _abi.call(name, *args)
    torch.cuda.synchronize()
    assert bool((out == SENTINEL[torch.int32]).all())
    del keep
