"""Cases and references shared by test_feeder_cases_cpu.py and test_gpu_feeder_edges.py: the four device kernels every update reads
its inputs through — collate_pad_kernel<DT, V>, collate_pad_nhwc_bf16_kernel, collate_ego_sparse_nhwc_bf16_kernel
(csrc/wsmg_collate.hip) and instruction_dedup_kernel<T> (csrc/wsmg_dedup.hip).  Nothing here touches a GPU: numpy and torch on the
CPU only.  Every comparison made with these references is exact (bit for bit, integer for integer): there is no tolerance.

The references are written out here and are not the project's own host forms:
  collate_ref         ref[t, n] = src_n[t] converted as the route converts it (`.float()`; or NCHW -> NHWC, `.float().bfloat16()`) for
                      t < length_n, else the pad value.  bf16 results are int16 bit patterns, so -0.0 and NaN compare exactly; the
                      float32 -> bf16 rounding is written out (_bf16_bits: equal to torch's on every input but NaN, which becomes 0x7FC0 as on the device).
  sparse_collate_ref  the same tensor from bits / off / base / vals, pixel by pixel in numpy (not codec.sparse_expand_ego).
  dedup_ref           a dictionary over row.tobytes(): distinct rows in order of first appearance, inverse, non-zero tokens per row.
  row_hash            the dedup kernel's hash in Python integers modulo 2^64; colliding_row builds a different row with the same hash.
test_feeder_cases_cpu.py holds them against collate_fn, torch.unique and each other, and every case to the path its name claims.

The paths (csrc/wsmg_collate.hip): collate_pad_kernel takes V = 4 elements per work item when elems % 4 == 0, else V = 1; its grid is
capped at GRID_CAP_ITEMS = 16384 x 256 work items, beyond which the grid-stride loop makes further trips.  The NHWC kernel walks
64-channel x 64-pixel tiles (C % 64 == 0, HW % 4 == 0); the sparse expansion gives a wave 16 pixels in groups of 4."""
import functools
import types

import numpy as np
import torch

GRID_CAP_ITEMS = 16384 * 256
DT_CODE = {np.dtype(np.float16): 0, np.dtype(np.uint8): 1, np.dtype(np.int64): 2, np.dtype(np.float32): 3}   # the ABI's src_dtype
PADS = (1.0, 0.0)
DD_CHUNK, DD_MAX_ROWS = 1024, 4096         # the dedup kernel's rank-scan chunk and its row limit

# float16 bit patterns: +-0, the smallest subnormal (both signs), the largest subnormal, the smallest normal, +-65504, +-inf, NaN
F16_SPECIAL = [0x0000, 0x8000, 0x0001, 0x8001, 0x03FF, 0x0400, 0x7BFF, 0xFBFF, 0x7C00, 0xFC00, 0x7E00]
# float16 values half way between two bf16 neighbours (low three mantissa bits 100): (pattern, +1 if round-to-nearest-even moves the
# bf16 magnitude up, 0 if it stays), and their neighbours one float16 ulp to either side, which are no ties
BF16_TIES = [(0x3C04, 0), (0x3C0C, 1), (0xBC04, 0), (0xBC0C, 1), (0x4234, 0), (0x423C, 1)]
BF16_NEAR_TIES = [0x3C03, 0x3C05, 0x3C0B, 0x3C0D]
F16_VALUES = F16_SPECIAL + [p for p, _ in BF16_TIES] + BF16_NEAR_TIES
U8_VALUES = [0, 255, 1, 128]
I64_VALUES = [-1, -2, -(2 ** 24), -(2 ** 24) - 1, 2 ** 24, 2 ** 24 + 1, 2 ** 24 + 2, 2 ** 24 + 3, 2 ** 31, 2 ** 40 + 1, -(2 ** 53) - 1,
              2 ** 62 + 2 ** 38, 2 ** 63 - 1, -(2 ** 63)]
F32_BITS = [0x00000000, 0x80000000, 0x00000001, 0x7F7FFFFF, 0x7F800000, 0xFF800000, 0x7FC00000, 0x3F800001]


# ---------------------------------------------------------------------------------------------------------------- collate: references
BF16_NAN = 0x7FC0


def _bf16_bits(t):
    """`t.bfloat16()` of a float32 tensor as int16 patterns, with the rounding written out on the float32 bits: round to nearest, ties
    to even (add 0x7FFF plus the lowest kept bit, keep the upper half); a NaN becomes the quiet NaN 0x7FC0.  torch's `.bfloat16()` on
    the CPU is not used for the values themselves because of that one input: its tensor conversion there writes 0xFFFF for a NaN,
    while the route the kernels are documented to equal bit for bit — wsmg_collate_pad, then torch's float32 -> bf16 conversion ON
    THE DEVICE — gives 0x7FC0 (test_gpu_feeder_edges.py compares the two on the device, NaN included).  test_feeder_cases_cpu.py
    holds this form to `.float().bfloat16()` on every one of the 65536 float16 patterns, NaNs apart."""
    assert t.dtype == torch.float32
    u = t.contiguous().view(torch.int32).to(torch.int64) & 0xFFFFFFFF
    r = ((u + 0x7FFF + ((u >> 16) & 1)) >> 16) & 0xFFFF
    r = torch.where(torch.isnan(t), torch.full_like(r, BF16_NAN), r)
    return torch.where(r >= 0x8000, r - 0x10000, r).to(torch.int16)


def convert(a, route):
    """The steps of one episode as the route converts them: float32 [steps, ...], or int16 patterns [steps, HW, C] of channels-last bf16."""
    t = torch.from_numpy(np.ascontiguousarray(a))
    if route == "f32":
        return t.float()
    assert route == "nhwc_bf16" and t.dim() == 4
    return _bf16_bits(t.float().permute(0, 2, 3, 1)).reshape(t.shape[0], t.shape[2] * t.shape[3], t.shape[1])


def pad_value(pad, route):
    v = torch.tensor(float(pad), dtype=torch.float32)
    return v if route == "f32" else _bf16_bits(v)


def collate_ref(eps, lengths, T, pad, route="f32"):
    """[T, N, ...]: element (t, n) is episode n's step t, converted, when t < lengths[n], else the pad value."""
    N = len(eps)
    rows = [convert(e[:lengths[n]], route) for n, e in enumerate(eps)]
    out = torch.empty((T, N) + tuple(rows[0].shape[1:]), dtype=rows[0].dtype)
    padv = pad_value(pad, route)
    for t in range(T):
        for n in range(N):
            if t < lengths[n]:
                out[t, n] = rows[n][t]
            else:
                out[t, n] = padv
    return out


def sparse_collate_ref(records, lengths, T, pad):
    """int16 [T, N, HW, 64] from the sparse record form: channel c of pixel p of step t is present iff bit c % 8 of byte c / 8 of
    bits[t, p] is set; the present values of a pixel are consecutive in vals from base[t] + off[t, p], in channel order."""
    N = len(records)
    HW = records[0]["rgb_ego_map__bits"].shape[1]
    out = np.full((T, N, HW, 64), int(pad_value(pad, "nhwc_bf16")), dtype=np.int16)
    for n, rec in enumerate(records):
        bits, off = np.asarray(rec["rgb_ego_map__bits"]), np.asarray(rec["rgb_ego_map__off"])
        base = np.asarray(rec["rgb_ego_map__base"])
        vals = _bf16_bits(torch.from_numpy(np.ascontiguousarray(rec["rgb_ego_map__vals"])).float()).numpy()
        for t in range(lengths[n]):
            for p in range(HW):
                k = int(base[t]) + int(off[t, p])
                for c in range(64):
                    if (int(bits[t, p, c // 8]) >> (c % 8)) & 1:
                        out[t, n, p, c] = vals[k]
                        k += 1
                    else:
                        out[t, n, p, c] = 0
    return torch.from_numpy(out)


def presence_words(rec):
    """The 8-byte presence word of every (step, pixel) as Python integers."""
    b = np.asarray(rec["rgb_ego_map__bits"])
    return [int.from_bytes(bytes(b[t, p]), "little") for t in range(b.shape[0]) for p in range(b.shape[1])]


# ------------------------------------------------------------------------------------------------------------------- collate: cases
def _fill(dtype, n, rng):
    """n values of a source dtype with its value set at both ends (the first and the last work items of an episode)."""
    dtype = np.dtype(dtype)
    if dtype == np.float16:
        a, sp = rng.standard_normal(n).astype(np.float16).view(np.uint16), np.array(F16_VALUES, dtype=np.uint16)
    elif dtype == np.uint8:
        a, sp = rng.randint(0, 256, size=n).astype(np.uint8), np.array(U8_VALUES, dtype=np.uint8)
    elif dtype == np.int64:
        a, sp = rng.randint(-2 ** 40, 2 ** 40, size=n).astype(np.int64), np.array(I64_VALUES, dtype=np.int64)
    else:
        a, sp = rng.standard_normal(n).astype(np.float32).view(np.uint32), np.array(F32_BITS, dtype=np.uint32)
    m = min(n, len(sp))
    a[:m] = sp[:m]
    a[n - m:] = sp[:m][::-1]
    return a.view(dtype)


def value_set(dtype):
    dtype = np.dtype(dtype)
    return {np.dtype(np.float16): np.array(F16_VALUES, dtype=np.uint16).view(np.float16), np.dtype(np.uint8): np.array(U8_VALUES, dtype=np.uint8),
            np.dtype(np.int64): np.array(I64_VALUES, dtype=np.int64), np.dtype(np.float32): np.array(F32_BITS, dtype=np.uint32).view(np.float32)}[dtype]


def _pad_case(name, dtype, shape, lengths, seed, stride=False):
    """A sensor of one batch.  An episode of length 0 still owns one (never read) step, so that its pointer is valid."""
    rng = np.random.RandomState(seed)
    elems = int(np.prod(shape, dtype=np.int64))
    eps = [_fill(dtype, max(n, 1) * elems, rng).reshape((max(n, 1),) + tuple(shape)) for n in lengths]
    T, V = max(lengths), 4 if elems % 4 == 0 else 1
    return types.SimpleNamespace(name=name, dtype=np.dtype(dtype), shape=tuple(shape), lengths=list(lengths), T=T, N=len(lengths), eps=eps,
                                 elems=elems, V=V, work_items=T * len(lengths) * (elems // V), stride=stride)


RAGGED = (6, 1, 3, 6)                 # a full-length episode, one of length 1, one with pad rows
RAGGED_ZERO = (6, 1, 0, 3)            # and one of length 0: every row of it is pad
SMALL_FORMS = [("f16.v4", np.float16, (3, 4, 4)), ("f16.v1", np.float16, (5, 7)), ("u8.v4", np.uint8, (3, 4, 4)), ("u8.v1", np.uint8, (5, 7)),
               ("i64.v4", np.int64, (3, 4, 4)), ("i64.v1", np.int64, (5, 7)), ("f32.v4", np.float32, (3, 4, 4)), ("f32.v1", np.float32, (5, 7))]


@functools.lru_cache(maxsize=None)
def small_pad_cases(zero_length=False):
    """One case per source dtype and vector width; with zero_length, the same forms in a batch that has an episode of length 0."""
    lengths = RAGGED_ZERO if zero_length else RAGGED
    return [_pad_case(name + (".len0" if zero_length else ""), dt, shape, lengths, 31 + i) for i, (name, dt, shape) in enumerate(SMALL_FORMS)]


@functools.lru_cache(maxsize=None)
def stride_pad_cases():
    """More work items than the capped grid has threads: the grid-stride loop's second trip, in both vector widths."""
    return [_pad_case("f16.v4.stride", np.float16, (64, 100, 100), (9, 1, 5), 41, stride=True),
            _pad_case("f32.v1.stride", np.float32, (300001,), (5, 1, 3), 42, stride=True)]


NHWC_SHAPES = [(64, 2, 2), (64, 8, 8), (64, 10, 10), (128, 6, 10), (128, 8, 16), (192, 5, 4)]
NHWC_LENGTHS = (4, 1, 2)


def nhwc_tiles(C, HW):
    """(channel tiles, full pixel tiles, pixels of the partial tile) of collate_pad_nhwc_bf16_kernel's grid."""
    return C // 64, HW // 64, HW % 64


@functools.lru_cache(maxsize=None)
def nhwc_cases():
    return [_pad_case(f"nhwc.C{C}.{H}x{W}", np.float16, (C, H, W), NHWC_LENGTHS, 51 + i) for i, (C, H, W) in enumerate(NHWC_SHAPES)]


def batch_of(cases, seed=7, names=None):
    """The cases as the sensors of ONE batch for collate_fn / plan_batch / DeviceCollator: [(obs, prev_actions, oracle_actions, weights)].
    names: the sensors' names when they are not the cases' (the collator takes the channels-last route for `rgb_ego_map` only)."""
    rng = np.random.RandomState(seed)
    lengths = cases[0].lengths
    names = names or [c.name for c in cases]
    assert all(c.lengths == lengths for c in cases) and min(lengths) > 0
    return [({k: c.eps[n][:L] for k, c in zip(names, cases)}, rng.standard_normal((L, 2)).astype(np.float32), rng.standard_normal((L, 2)).astype(np.float32),
             rng.rand(L).astype(np.float32)) for n, L in enumerate(lengths)]


# ------------------------------------------------------------------------------------------------------------ sparse ego map: cases
SPARSE_SHAPES = [(1, 1), (3, 5), (7, 7), (8, 8), (10, 10), (9, 15)]
SPARSE_KINDS = [("zero", "dense", "c63", "all64", "c0", "negzero", "relu30"), ("relu30",), ("dense", "zero", "negzero")]


def _sparse_step(kind, HW, rng):
    """One step, channels-last float16 [HW, 64].  c63 / all64 / c0: the pixel the name describes is the last / the middle / the first
    one and the others are post-ReLU noise; negzero: the first pixel holds exactly one stored value, -0.0 in channel 5."""
    relu = lambda: np.maximum(rng.standard_normal((HW, 64)) - 0.52, 0).astype(np.float16)   # noqa: E731  (30 % non-zeros)
    if kind == "zero":
        return np.zeros((HW, 64), dtype=np.float16)
    if kind == "dense":
        x = ((rng.rand(HW, 64) + 0.5) * np.where(rng.rand(HW, 64) < 0.5, -1, 1)).astype(np.float16)
        sp = np.array([p for p in F16_VALUES if p & 0x7FFF], dtype=np.uint16).view(np.float16)   # every value of the set that is stored
        x[0, :len(sp)] = sp
        x[HW - 1, 64 - len(sp):] = sp
        return x
    x = relu()
    if kind == "c63":
        x[HW - 1] = 0
        x[HW - 1, 63] = -2.5
    elif kind == "all64":
        x[HW // 2] = (rng.rand(64) + 0.5).astype(np.float16)
    elif kind == "c0":
        x[0] = 0
        x[0, 0] = 0.75
    elif kind == "negzero":
        x[0] = 0
        x[0, 5] = -0.0
    return x


@functools.lru_cache(maxsize=None)
def sparse_cases():
    """Per shape: dense float16 episodes [len, 64, H, W] and their records (codec.sparse_pack_ego, pinned by test_gpu_sparse_pack.py)."""
    from wsmgmap.data import sparse_pack_ego
    out = []
    for i, (H, W) in enumerate(SPARSE_SHAPES):
        rng = np.random.RandomState(61 + i)
        dense = [np.ascontiguousarray(np.stack([_sparse_step(k, H * W, rng) for k in kinds]).reshape(len(kinds), H, W, 64).transpose(0, 3, 1, 2))
                 for kinds in SPARSE_KINDS]
        lengths = [len(k) for k in SPARSE_KINDS]
        out.append(types.SimpleNamespace(name=f"sparse.{H}x{W}", H=H, W=W, HW=H * W, lengths=lengths, T=max(lengths), N=len(lengths), dense=dense,
                                         records=[sparse_pack_ego(d) for d in dense]))
    return out


def sparse_batch(case, seed=9):
    rng = np.random.RandomState(seed)
    return [(dict(rec), rng.standard_normal((L, 2)).astype(np.float32), rng.standard_normal((L, 2)).astype(np.float32), rng.rand(L).astype(np.float32))
            for rec, L in zip(case.records, case.lengths)]


# ----------------------------------------------------------------------------------------------------------------------------- dedup
def dedup_ref(tokens):
    """int64 [B, L] -> (distinct rows [U, L] in order of first appearance, inverse [B], non-zero tokens per distinct row [U])."""
    tokens = np.ascontiguousarray(tokens, dtype=np.int64)
    seen, uniq, inverse = {}, [], []
    for row in tokens:
        key = row.tobytes()
        if key not in seen:
            seen[key] = len(uniq)
            uniq.append(row)
        inverse.append(seen[key])
    u = np.stack(uniq)
    return u, np.array(inverse, dtype=np.int64), np.count_nonzero(u, axis=1).astype(np.int64)


M64 = (1 << 64) - 1
HASH_LANES = 64


def hash_mult(l):
    return (((l + 1) * 0x9E3779B97F4A7C15) & M64) | 1


def row_hash(row):
    """h = sum over l of tok_l * m_l modulo 2^64 (every addition of the kernel is modulo 2^64: the order of its lanes does not matter)."""
    return sum((int(t) & M64) * hash_mult(l) for l, t in enumerate(row)) & M64


def _signed(v):
    v &= M64
    return v - (1 << 64) if v >> 63 else v


def colliding_row(row, l1, l2):
    """`row` with tok[l1] += 1 and tok[l2] += d, d = -m_l1 / m_l2 modulo 2^64 (m_l2 is odd, hence invertible): another row, the same hash."""
    d = (-hash_mult(l1) * pow(hash_mult(l2), -1, 1 << 64)) & M64
    out = [int(t) for t in row]
    out[l1] = _signed(out[l1] + 1)
    out[l2] = _signed(out[l2] + d)
    return np.array(out, dtype=np.int64)


COLLISION_L = 100
COLLISION_PAIRS = ((3, 40), (10, 70))       # inside the first 64 tokens; across the 64-lane stride of the hash loop


def _rows(rng, n, L, length=None):
    t = np.zeros((n, L), dtype=np.int64)
    length = L if length is None else length
    t[:, :length] = rng.randint(1, 2504, size=(n, length))
    return t


def collision_rows():
    """(A1, B1, A2, B2): A1 / B1 collide at tokens 3 and 40, A2 / B2 at tokens 10 and 70."""
    rng = np.random.RandomState(77)
    a1, a2 = _rows(rng, 2, COLLISION_L, 80)
    return a1, colliding_row(a1, *COLLISION_PAIRS[0]), a2, colliding_row(a2, *COLLISION_PAIRS[1])


@functools.lru_cache(maxsize=None)
def dedup_cases():
    """[(name, int64 tokens [B, L], dtypes the case runs in)].  float32 cases hold tokens below 2^24 only."""
    rng = np.random.RandomState(71)
    both, cases = ("int64", "float32"), []
    cases.append(("B1.L1", np.array([[5]], dtype=np.int64), both))
    for L in (63, 64, 65):                    # around the 64-lane stride of the hash loop; row 3 differs from row 0 at token L - 1 only
        r = _rows(rng, 3, L)
        t = np.stack([r[0], r[1], r[0], r[0], r[1]])
        t[3, L - 1] += 1
        cases.append((f"B5.L{L}", t, both))
    for B in (DD_CHUNK - 1, DD_CHUNK, DD_CHUNK + 1):      # every fifth row repeats the row three before it; the last row is distinct
        t = _rows(rng, B, 8)
        for b in range(5, B, 5):
            t[b] = t[b - 3]
        cases.append((f"B{B}.L8", t, both))
    B, L = DD_MAX_ROWS, 200
    cases.append((f"B{B}.L{L}.8rows", np.tile(_rows(rng, 8, L, 80), (B // 8, 1)), both))
    cases.append((f"B{B}.L{L}.equal", np.tile(_rows(rng, 1, L, 80), (B, 1)), both))
    distinct = _rows(rng, B, L, 80)
    distinct[:, 0] = 1 + np.arange(B)         # distinct by construction
    cases.append((f"B{B}.L{L}.distinct", distinct, both))
    t = np.tile(_rows(rng, 1, 130), (6, 1))    # rows equal except at token 64: the first token of a lane's second trip
    t[1, 64], t[3, 64], t[4, 64] = 2600, 2601, 2600
    cases.append(("B6.L130.token64", t, both))
    t = np.tile(_rows(rng, 1, 200), (6, 1))    # rows equal except at token L - 1
    t[2, 199], t[3, 199], t[5, 199] = 2600, 2601, 2600
    cases.append(("B6.L200.last", t, both))
    t = _rows(rng, 5, 20)                      # a row of zeros (length 0) beside rows with interior zeros (length = non-zeros)
    t[1] = 0
    t[2, 3:9] = 0
    t[3, 0] = 0
    t[4] = t[2]
    cases.append(("B5.L20.zeros", t, both))
    a1, b1, a2, b2 = collision_rows()           # equal hashes, different rows: not adjacent, each twice
    z = _rows(rng, 1, COLLISION_L, 80)[0]
    cases.append((f"B11.L{COLLISION_L}.collisions", np.stack([a1, a2, z, b1, b2, z, a1, a2, z, b1, b2]), ("int64",)))
    return cases
