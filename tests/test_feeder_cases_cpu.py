"""tests/feeder_cases.py held to its own conditions, without a GPU: every case sits on the path its name claims, the references agree
with the project's host forms and with each other, and no source the collate kernels would be handed is misaligned — so that
test_gpu_feeder_edges.py cannot pass vacuously."""
import numpy as np
import torch

import feeder_cases as fc


def _bits(t):
    return t.contiguous().view(torch.int32) if t.dtype == torch.float32 else t


def test_grid_stride_cases_exceed_the_capped_grid_and_the_others_do_not():
    stride = fc.stride_pad_cases()
    assert {(c.dtype, c.V) for c in stride} == {(np.dtype(np.float16), 4), (np.dtype(np.float32), 1)}
    for c in stride:
        assert c.work_items > fc.GRID_CAP_ITEMS, c.name
        assert c.work_items < 2 * fc.GRID_CAP_ITEMS, c.name            # two trips for the first threads, one for the last
    assert stride[0].shape == (64, 100, 100) and (stride[0].T, stride[0].N) == (9, 3) and stride[0].work_items == 4_320_000
    assert stride[1].elems == 300001 and (stride[1].T, stride[1].N) == (5, 3) and stride[1].work_items == 4_500_015
    for c in fc.small_pad_cases() + fc.small_pad_cases(True):
        assert c.work_items <= fc.GRID_CAP_ITEMS and not c.stride, c.name
        assert c.V == (4 if c.elems % 4 == 0 else 1)
    assert {(c.dtype, c.V) for c in fc.small_pad_cases()} == {(np.dtype(d), v) for d in (np.float16, np.uint8, np.int64, np.float32) for v in (4, 1)}
    assert {(c.dtype, c.V) for c in fc.small_pad_cases(True)} == {(c.dtype, c.V) for c in fc.small_pad_cases()}


def test_lengths_are_ragged_everywhere():
    groups = [fc.small_pad_cases(), fc.small_pad_cases(True), fc.stride_pad_cases(), fc.nhwc_cases(), fc.sparse_cases()]
    for c in [c for g in groups for c in g]:
        assert max(c.lengths) == c.T and 1 in c.lengths, c.name
        assert any(1 < n < c.T for n in c.lengths) or 0 in c.lengths, c.name     # beside the episode of length 1, another with pad rows
    assert all(0 in c.lengths for c in fc.small_pad_cases(True)) and not any(0 in c.lengths for c in fc.small_pad_cases())
    for c in fc.sparse_cases():                                          # a live step followed by pad rows of the same episode
        assert any(0 < n < c.T for n in c.lengths)


def test_every_value_of_the_sets_is_in_its_cases():
    for c in fc.small_pad_cases() + fc.small_pad_cases(True) + fc.nhwc_cases():
        raw = lambda a: a.view({2: np.uint16, 1: np.uint8, 8: np.int64, 4: np.uint32}[a.dtype.itemsize])   # noqa: E731
        live = np.concatenate([raw(e[:n].reshape(-1)) for e, n in zip(c.eps, c.lengths)])
        assert set(raw(fc.value_set(c.dtype)).tolist()) <= set(live.tolist()), c.name
    f16 = set(fc.F16_VALUES)
    assert {0x0000, 0x8000, 0x0001, 0x7BFF, 0x7C00, 0xFC00, 0x7E00} <= f16
    assert {0, 255} <= set(fc.U8_VALUES)
    assert any(v < 0 for v in fc.I64_VALUES) and 2 ** 24 in fc.I64_VALUES and any(v > 2 ** 24 for v in fc.I64_VALUES)
    assert any(float(np.float32(v)) != v for v in fc.I64_VALUES)           # some value is not a float32: the conversion has to round


def test_the_bf16_ties_are_ties_in_both_directions():
    moved = set()
    for pattern, up in fc.BF16_TIES:
        f32 = int(np.array([pattern], dtype=np.uint16).view(np.float16).astype(np.float32).view(np.uint32)[0])
        assert f32 & 0xFFFF == 0x8000, hex(pattern)                        # exactly half way between two bf16 values
        assert ((f32 >> 16) & 1) == up                                     # the odd neighbour moves up, the even one stays
        got = int(fc.convert(np.array([pattern], dtype=np.uint16).view(np.float16).reshape(1, 1, 1, 1), "nhwc_bf16").reshape(-1)[0]) & 0xFFFF
        assert got == (f32 >> 16) + up, hex(pattern)
        moved.add(up)
    assert moved == {0, 1}
    for pattern in fc.BF16_NEAR_TIES:
        f32 = int(np.array([pattern], dtype=np.uint16).view(np.float16).astype(np.float32).view(np.uint32)[0])
        assert f32 & 0xFFFF not in (0, 0x8000)


def test_nhwc_cases_cover_the_tiles_they_name():
    assert [c.shape for c in fc.nhwc_cases()] == fc.NHWC_SHAPES
    tiles = [fc.nhwc_tiles(c.shape[0], c.shape[1] * c.shape[2]) for c in fc.nhwc_cases()]
    assert [c.shape[1] * c.shape[2] for c in fc.nhwc_cases()] == [4, 64, 100, 60, 128, 20]
    assert {t[0] for t in tiles} == {1, 2, 3}
    assert any(full == 0 and part for _, full, part in tiles)              # a partial pixel tile alone
    assert any(full and not part for _, full, part in tiles)               # no partial tile
    assert any(full and part for _, full, part in tiles)                   # full tiles and a partial one
    assert any(ct > 1 and full == 0 for ct, full, _ in tiles) and any(ct > 1 and full > 1 for ct, full, _ in tiles)
    for c in fc.nhwc_cases():
        assert c.shape[0] % 64 == 0 and (c.shape[1] * c.shape[2]) % 4 == 0 and c.T * c.N <= 65535


def test_plan_batch_places_every_episode_of_every_sensor_on_16_bytes():
    """The kernels' 8- and 16-byte loads rest on this (and on the allocator's alignment of the staged buffer itself): no case of
    test_gpu_feeder_edges.py that goes through DeviceCollator hands a kernel a misaligned source."""
    from wsmgmap.data.collate import plan_batch
    batches = [fc.batch_of(fc.small_pad_cases())] + [fc.batch_of([c]) for c in fc.stride_pad_cases() + fc.nhwc_cases()]
    batches += [fc.sparse_batch(c) for c in fc.sparse_cases()]
    for batch in batches:
        plan, meta = plan_batch(batch)
        arrs = [a for _, eps, _ in plan for a in eps]
        assert len(meta["offsets"]) == len(arrs) == len(meta["sensors"]) * meta["N"]
        end = 0
        for o, a in zip(meta["offsets"], arrs):
            assert o % 16 == 0 and o >= end
            end = o + a.nbytes
        assert end <= meta["total"]
        assert meta["lengths"] == [len(b[1]) for b in batch] and meta["T"] == max(meta["lengths"])


def test_collision_pairs_differ_as_rows_and_share_their_hash():
    a1, b1, a2, b2 = fc.collision_rows()
    for (a, b), (l1, l2) in zip(((a1, b1), (a2, b2)), fc.COLLISION_PAIRS):
        assert a.dtype == b.dtype == np.int64 and a.shape == b.shape == (fc.COLLISION_L,)
        assert np.flatnonzero(a != b).tolist() == [l1, l2]
        assert fc.row_hash(a) == fc.row_hash(b)
    assert all(l < fc.HASH_LANES for l in fc.COLLISION_PAIRS[0])
    assert fc.COLLISION_PAIRS[1][0] < fc.HASH_LANES <= fc.COLLISION_PAIRS[1][1]
    assert len({fc.row_hash(r) for r in (a1, a2)}) == 2
    # the restated hash against the same sum in wrapping int64 arithmetic
    mult = torch.tensor([fc._signed(fc.hash_mult(l)) for l in range(fc.COLLISION_L)], dtype=torch.int64)
    for r in (a1, b1, a2, b2):
        assert int((torch.from_numpy(r) * mult).sum()) & fc.M64 == fc.row_hash(r)
    name, tok, dtypes = fc.dedup_cases()[-1]
    assert "collisions" in name and dtypes == ("int64",)
    where = {k: [i for i, r in enumerate(tok) if np.array_equal(r, v)] for k, v in (("a1", a1), ("b1", b1), ("a2", a2), ("b2", b2))}
    assert all(len(v) == 2 for v in where.values())
    for a, b in (("a1", "b1"), ("a2", "b2")):
        assert all(abs(i - j) > 1 for i in where[a] for j in where[b])      # the colliding rows are not adjacent


def test_dedup_cases_are_what_they_are_named():
    cases = {name: (tok, dtypes) for name, tok, dtypes in fc.dedup_cases()}
    shapes = {tok.shape for tok, _ in cases.values()}
    assert {(1, 1), (5, 63), (5, 64), (5, 65), (1023, 8), (1024, 8), (1025, 8), (4096, 200)} <= shapes
    for name, (tok, dtypes) in cases.items():
        assert tok.dtype == np.int64 and tok.shape[0] <= fc.DD_MAX_ROWS
        if "float32" in dtypes:
            assert np.abs(tok).max() < 2 ** 24, name
    count = lambda name: len(fc.dedup_ref(cases[name][0])[0])      # noqa: E731
    assert count("B4096.L200.8rows") == 8 and count("B4096.L200.equal") == 1 and count("B4096.L200.distinct") == 4096
    for B in (1023, 1024, 1025):
        tok = cases[f"B{B}.L8"][0]
        _, inverse, _ = fc.dedup_ref(tok)
        assert int(inverse[B - 1]) == int(inverse.max()) and (inverse == inverse[B - 1]).sum() == 1     # the last row ranks last, alone
    assert int(fc.dedup_ref(cases["B1025.L8"][0])[1][1024]) > 0                  # a representative in the scan's second chunk
    for name, col in (("B6.L130.token64", 64), ("B6.L200.last", 199), ("B5.L63", 62), ("B5.L64", 63), ("B5.L65", 64)):
        tok = cases[name][0]
        differ = np.flatnonzero((tok != tok[0]).any(axis=0)).tolist()
        assert col in differ and (differ == [col] or name.startswith("B5")), name
        assert 1 < count(name) < len(tok)
    tok = cases["B5.L20.zeros"][0]
    _, _, lengths = fc.dedup_ref(tok)
    assert lengths.tolist() == [20, 0, 14, 19] and tok[2, 19] != 0              # a length counts non-zeros: it is not the last one's index


def test_dedup_reference_against_torch_unique():
    for name, tok, _ in fc.dedup_cases():
        uniq, inverse, lengths = fc.dedup_ref(tok)
        ref_u = torch.unique(torch.from_numpy(tok), dim=0)
        assert set(map(bytes, uniq)) == set(map(bytes, ref_u.numpy())) and len(uniq) == ref_u.shape[0], name
        assert np.array_equal(uniq[inverse], tok), name
        first = [int(np.flatnonzero(inverse == u)[0]) for u in range(len(uniq))]
        assert first == sorted(first), name
        assert np.array_equal(lengths, (uniq != 0).sum(1)), name


def test_sparse_cases_hold_the_words_they_claim():
    for c in fc.sparse_cases():
        words = [w for rec in c.records for w in fc.presence_words(rec)]
        assert {0, 1 << 63, 1, fc.M64} <= set(words), c.name
        per_step = np.diff(np.asarray(c.records[0]["rgb_ego_map__base"]))
        assert 0 in per_step and c.HW * 64 in per_step, c.name              # a step with no non-zero, a fully dense step
        # the one stored -0.0: sparse_pack_ego keeps it as present (step 5 of episode 0, pixel 0, channel 5: the pixel's only value)
        rec = c.records[0]
        assert np.asarray(c.dense[0]).view(np.uint16)[5, 5, 0, 0] == 0x8000
        assert fc.presence_words(rec)[5 * c.HW] == 1 << 5
        assert int(np.asarray(rec["rgb_ego_map__vals"]).view(np.uint16)[int(rec["rgb_ego_map__base"][5])]) == 0x8000
        assert [tuple(int(x) for x in r["rgb_ego_map__shape"]) for r in c.records] == [(64, c.H, c.W)] * c.N
    assert [c.HW for c in fc.sparse_cases()] == [1, 15, 49, 64, 100, 135]
    assert any(c.HW % 4 for c in fc.sparse_cases()) and any(c.HW < 16 for c in fc.sparse_cases())


def test_sparse_reference_against_the_dense_reference():
    for c in fc.sparse_cases():
        for pad in fc.PADS:
            want = fc.collate_ref(c.dense, c.lengths, c.T, pad, "nhwc_bf16")
            got = fc.sparse_collate_ref(c.records, c.lengths, c.T, pad)
            assert got.dtype == torch.int16 and got.shape == (c.T, c.N, c.HW, 64)
            assert torch.equal(got, want), (c.name, pad)
        assert (want[5, 0, 0, 5] & 0xFFFF) == 0x8000                         # the reference carries the sign of the stored -0.0


def test_collate_reference_against_the_host_route():
    """collate_fn (the reference's semantics, dtypes as stored) followed by `.float()`: pad 1.0 on observations, 0 on actions and weights."""
    from wsmgmap.data.collate import collate_fn
    cases = fc.small_pad_cases()
    batch = fc.batch_of(cases)
    obs, prev, masks, corr, wts = collate_fn(batch)
    T, N, lengths = cases[0].T, cases[0].N, cases[0].lengths
    for c in cases:
        want = fc.collate_ref(c.eps, lengths, T, 1.0)
        assert want.dtype == torch.float32 and want.shape == (T, N) + c.shape
        assert torch.equal(_bits(obs[c.name].float()), _bits(want.reshape(T * N, *c.shape))), c.name
        assert torch.equal(want[2, 1], torch.ones(c.shape)) and torch.equal(fc.collate_ref(c.eps, lengths, T, 0.0)[2, 1], torch.zeros(c.shape))
    for got, k in ((prev.view(T, N, 2), 1), (corr, 2), (wts, 3)):
        assert torch.equal(_bits(got.float()), _bits(fc.collate_ref([b[k] for b in batch], lengths, T, 0.0)))
    assert torch.equal(masks.view(T, N), torch.cat([torch.zeros(1, N), torch.ones(T - 1, N)]))


def test_written_out_bf16_rounding_is_torchs_on_every_float16_pattern():
    """The route's conversion is `.float().bfloat16()`; the reference writes the second rounding out (feeder_cases._bf16_bits) because
    torch's CPU conversion writes a NaN as 0xFFFF where its device conversion writes 0x7FC0.  Every other pattern: equal."""
    f16 = torch.from_numpy(np.arange(65536, dtype=np.int64).astype(np.uint16).view(np.float16))
    f32 = f16.float()
    ours, torchs = fc._bf16_bits(f32), f32.bfloat16().view(torch.int16)
    nan = torch.isnan(f32)
    assert int(nan.sum()) == 2 * 1023
    assert torch.equal(ours[~nan], torchs[~nan])
    assert bool((ours[nan] == fc.BF16_NAN).all())
    assert bool(((torchs[nan] & 0x7F80) == 0x7F80).all() and ((torchs[nan] & 0x7F) != 0).all())      # torch's are NaNs too, of some pattern
    assert int(fc.pad_value(1.0, "nhwc_bf16")) == 0x3F80 and int(fc.pad_value(0.0, "nhwc_bf16")) == 0


def test_bf16_reference_is_the_float32_reference_rounded_and_permuted():
    c = fc.nhwc_cases()[3]
    C, H, W = c.shape
    f32 = fc.collate_ref(c.eps, c.lengths, c.T, 1.0).permute(0, 1, 3, 4, 2).contiguous()      # [T, N, H, W, C]
    want = f32.bfloat16().view(torch.int16).reshape(c.T, c.N, H * W, C)
    got = fc.collate_ref(c.eps, c.lengths, c.T, 1.0, "nhwc_bf16")
    nan = torch.isnan(f32).reshape(got.shape)
    assert 0 < int(nan.sum()) < 64 and torch.equal(got[~nan], want[~nan]) and bool((got[nan] == fc.BF16_NAN).all())
