"""The grouped column gather (csrc/wsmg_rollout_gather.hip, ops.gather_columns) and the storage's fused minibatches against
`index_select` on the same GPU tensors.  A gather has no rounding: every comparison is of bits (rollout_util.same_bits for float32,
ppo_util.same_bytes, its like, for the other dtypes).  No test hands the GPU an index outside [0, N)."""
import ctypes

import pytest
import torch

import ppo_util as pu
import rollout_util as ru

pytestmark = pytest.mark.gpu

SENTINEL = 85          # 0x55 in every byte of a guard row


def _guarded(fields, rows, n):
    """(out, whole): per field a [rows_f, n, ...] view in front of one guard row, all bytes SENTINEL."""
    whole = []
    for f, r in zip(fields, rows):
        shape = (r + 1, n) + tuple(f.shape[2:])
        nbytes = torch.Size(shape).numel() * f.element_size()
        whole.append(torch.full((nbytes,), SENTINEL, dtype=torch.uint8, device=f.device).view(f.dtype).view(shape))
    return [w[:r] for w, r in zip(whole, rows)], whole


def _untouched(t):
    return bool((t.contiguous().view(torch.uint8) == SENTINEL).all())


@pytest.mark.parametrize("n_kind", ["one", "two", "all"])
@pytest.mark.parametrize("N", [1, 3, 8])
@pytest.mark.parametrize("R", [1, 2, 5])
def test_case_table_against_index_select(R, N, n_kind):
    """Every width of the table in ONE call: both unit sizes, the index_select route of the odd uint8 row, three dtypes."""
    from wsmgmap import ops
    n = {"one": 1, "two": min(2, N), "all": N}[n_kind]
    fields = pu.gather_fields(R, N, device="cuda")
    ind = pu.perm_prefix(N, n, device="cuda")
    got = ops.gather_columns(fields, ind)
    for name, g, w in zip(pu.WIDTHS, got, pu.gather_ref(fields, ind)):
        assert pu.same_bytes(g, w), name


def test_runs_end_inside_rows_and_between_rows():
    """rows = 5, n = 3 of 16 384-byte rows: 7.5 workgroup runs, so runs end inside a row, and (2 rows = 1 run) between rows."""
    from wsmgmap import ops
    R, N, n = 5, 8, 3
    (f,) = pu.gather_fields(R, N, names=("w16384",), device="cuda")
    assert R * n * 16384 > 7 * pu.GATHER_RUN_BYTES and (R * n * 16384) % pu.GATHER_RUN_BYTES != 0
    ind = pu.perm_prefix(N, n, device="cuda")
    (got,) = ops.gather_columns([f], ind)
    assert ru.same_bits(got, f.index_select(1, ind))


def test_first_rows_of_a_longer_source_and_the_guard_rows_survive():
    """Sources with rows + 1 rows give their first `rows`; a hidden-state field with rows = layers = 2 rides beside rows = 5 fields;
    nothing is written behind a destination's end."""
    from wsmgmap import ops
    R, N, n = 5, 8, 3
    names = ("w4", "w12", "w16", "w140", "w2048", "i32x6", "f16x10")
    fields = pu.gather_fields(R + 1, N, names=names, device="cuda") + pu.gather_fields(2, N, names=("w2048",), seed=1, device="cuda")
    rows = [R] * len(names) + [2]
    ind = pu.perm_prefix(N, n, device="cuda")
    out, whole = _guarded(fields, rows, n)
    got = ops.gather_columns(fields, ind, rows=rows, out=out)
    for k, (g, o, w, wh, r) in enumerate(zip(got, out, pu.gather_ref(fields, ind, rows), whole, rows)):
        assert g is o and pu.same_bytes(g, w), k
        assert _untouched(wh[r:]), k


def test_more_fields_than_one_launch_holds():
    from wsmgmap import ops
    R, N, n = 2, 3, 2
    k = pu.GATHER_MAX_FIELDS + 1
    assert ops.GATHER_MAX_FIELDS == pu.GATHER_MAX_FIELDS
    fields = [pu.gather_fields(R, N, names=(("w4", "w8", "w16")[i % 3],), seed=i, device="cuda")[0] for i in range(k)]
    ind = pu.perm_prefix(N, n, device="cuda")
    for i, (g, w) in enumerate(zip(ops.gather_columns(fields, ind), pu.gather_ref(fields, ind))):
        assert pu.same_bytes(g, w), i


def test_misaligned_base_of_a_wide_row_takes_the_4_byte_path():
    from wsmgmap import ops
    R, N, n, W = 5, 8, 3, 64
    g = torch.Generator(); g.manual_seed(3)
    base = torch.randn(R * N * W + 4, generator=g).cuda()
    f = base[1:1 + R * N * W].view(R, N, W)
    assert f.is_contiguous() and f.data_ptr() % 16 == 4 and (W * 4) % 16 == 0
    ind = pu.perm_prefix(N, n, device="cuda")
    (got,) = ops.gather_columns([f], ind)
    assert ru.same_bits(got, f.index_select(1, ind))
    # and a misaligned DESTINATION of an aligned source
    obase = torch.zeros(R * n * W + 4, device="cuda")
    o = obase[1:1 + R * n * W].view(R, n, W)
    aligned = f.clone()
    assert aligned.data_ptr() % 16 == 0 and o.data_ptr() % 16 == 4
    ops.gather_columns([aligned], ind, out=[o])
    assert ru.same_bits(o, f.index_select(1, ind)) and float(obase[0]) == 0.0 and float(obase[-1]) == 0.0


def test_nothing_is_allocated_with_out_and_a_second_call_gives_the_same_bits():
    from wsmgmap import ops
    R, N, n = 5, 8, 3
    fields = pu.gather_fields(R, N, device="cuda")
    ind = pu.perm_prefix(N, n, device="cuda")
    out = [torch.empty((R, n) + tuple(f.shape[2:]), dtype=f.dtype, device="cuda") for f in fields]
    ops.gather_columns(fields, ind, out=out)           # (the first call loads the library)
    first = [o.clone() for o in out]
    for o in out:
        o.view(torch.uint8).fill_(SENTINEL)
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated()
    got = ops.gather_columns(fields, ind, out=out)
    assert torch.cuda.memory_allocated() == before
    assert all(g is o for g, o in zip(got, out))
    for name, a, b in zip(pu.WIDTHS, first, out):
        assert pu.same_bytes(a, b), name


def test_a_captured_gather_follows_the_index_list_it_is_replayed_with():
    from wsmgmap import ops
    R, N, n = 5, 8, 3
    names = ("w4", "w12", "w140", "w2048")
    fields = pu.gather_fields(R, N, names=names, device="cuda")
    ind = pu.perm_prefix(N, n, device="cuda")
    out = [torch.zeros((R, n) + tuple(f.shape[2:]), dtype=f.dtype, device="cuda") for f in fields]
    ops.gather_columns(fields, ind, out=out)
    torch.cuda.synchronize()
    graph, side = torch.cuda.CUDAGraph(), torch.cuda.Stream()
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            ops.gather_columns(fields, ind, out=out)
    other = pu.perm_prefix(N, n, seed=5, device="cuda")
    assert not torch.equal(other, ind)
    ind.copy_(other)
    graph.replay()
    torch.cuda.synchronize()
    for name, o, w in zip(names, out, pu.gather_ref(fields, other)):
        assert pu.same_bytes(o, w), name


def _launch(dst, src, rows, row_bytes, ind_ptr, n, N, n_fields=None):
    """The launcher itself, through the binding: its return code."""
    from wsmgmap import _abi
    k = len(dst)
    arr = lambda ty, v: (ty * max(k, 1))(*v)       # noqa: E731
    return _abi.lib().wsmg_rollout_gather(arr(ctypes.c_void_p, dst), arr(ctypes.c_void_p, src), arr(ctypes.c_longlong, rows),
                                          arr(ctypes.c_longlong, row_bytes), k if n_fields is None else n_fields,
                                          ctypes.c_void_p(ind_ptr), n, N, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))


def test_launcher_refusals_write_nothing():
    """Every WSMG_EINVAL condition, each beside a valid first field: nothing is enqueued, the valid field's destination included."""
    R, N, n = 2, 3, 2
    src = torch.randn(R, N, 4, device="cuda")
    dst = torch.full((R, n, 4), 7.0, device="cuda")
    ind = torch.tensor([2, 0], device="cuda")
    s, d, i = src.data_ptr(), dst.data_ptr(), ind.data_ptr()
    ok = ([d], [s], [R], [16])
    EINVAL = -1
    bad = {
        "n < 1": (*ok, i, 0, N),
        "N < 1": (*ok, i, n, 0),
        "null ind": (*ok, 0, n, N),
        "negative rows": ([d, d], [s, s], [R, -1], [16, 16], i, n, N),
        "row_bytes 0": ([d, d], [s, s], [R, R], [16, 0], i, n, N),
        "row_bytes 6": ([d, d], [s, s], [R, R], [16, 6], i, n, N),
        "negative row_bytes": ([d, d], [s, s], [R, R], [16, -4], i, n, N),
        "misaligned src": ([d, d], [s, s + 2], [R, R], [16, 4], i, n, N),
        "misaligned dst": ([d, d + 1], [s, s], [R, R], [16, 4], i, n, N),
        "null src with rows": ([d, d], [s, 0], [R, R], [16, 16], i, n, N),
        "null dst with rows": ([d, 0], [s, s], [R, R], [16, 16], i, n, N),
        "negative n_fields": (*ok, i, n, N, -1),
    }
    for name, args in bad.items():
        assert _launch(*args) == EINVAL, name
    torch.cuda.synchronize()
    assert bool((dst == 7.0).all())
    # a field with rows == 0 (null bases allowed) owns no workgroup; the field beside it is copied
    assert _launch([0, d], [0, s], [0, R], [16, 16], i, n, N) == 0
    assert _launch([], [], [], [], i, n, N) == 0
    torch.cuda.synchronize()
    assert ru.same_bits(dst, src.index_select(1, ind))


def test_wrapper_refusals_name_the_operand():
    from wsmgmap import _abi, ops
    f = torch.zeros(2, 3, 4, device="cuda")
    ind = torch.tensor([1, 0], device="cuda")
    with pytest.raises(_abi.WsmgError, match=r"fields\[0\] is on cuda:0, ind on cpu"):
        ops.gather_columns([f], ind.cpu())
    with pytest.raises(_abi.WsmgError, match=r"fields\[1\] is not contiguous"):
        ops.gather_columns([f, torch.zeros(2, 4, 3, device="cuda").transpose(1, 2)], ind)
    with pytest.raises(_abi.WsmgError, match=r"out\[0\] must be"):
        ops.gather_columns([f], ind, out=[torch.zeros(2, 3, 4, device="cuda")])
    with pytest.raises(_abi.WsmgError, match=r"out\[0\] must be"):
        ops.gather_columns([f], ind, out=[torch.zeros(2, 2, 4)])
    with pytest.raises(_abi.WsmgError, match=r"out\[0\] is not contiguous"):
        ops.gather_columns([f], ind, out=[torch.zeros(2, 4, 2, device="cuda").transpose(1, 2)])


# -- the storage ---------------------------------------------------------------------------------------------------------------------
def _pair(T, N, steps):
    from wsmgmap.rollout import RolloutStorage
    shapes = {"x": ((3,), torch.float32), "tokens": ((5,), torch.uint8), "grid": ((6, 4), torch.float16)}
    pair = []
    for fused in (True, False):
        st = RolloutStorage(T, N, shapes, 2, 8, num_recurrent_layers=2, fused=fused).to("cuda")
        pu.fill_storage(st, steps)
        st.compute_returns(torch.linspace(-1.0, 1.0, N, device="cuda").view(N, 1), True, 0.99, 0.95)
        pair.append(st)
    return pair


@pytest.mark.parametrize("reuse", [False, True], ids=["fresh", "reuse_buffers"])
@pytest.mark.parametrize("T,N,steps,nmb", [(4, 2, 4, 1), (5, 4, 3, 2), (3, 5, 3, 2)], ids=["T4N2", "partial_3_of_5", "one_env_left_out"])
def test_fused_minibatches_are_the_stock_minibatches(T, N, steps, nmb, reuse):
    fused, stock = _pair(T, N, steps)
    assert ru.same_bits(fused.returns, stock.returns)
    adv_f, adv_s = fused.get_advantages(False), stock.get_advantages(False)      # (the raw form: the same bits on both routes)
    assert ru.same_bits(adv_f, adv_s)
    torch.manual_seed(31)
    want = [b for b in stock.recurrent_generator(adv_s, nmb)]
    torch.manual_seed(31)
    count, ptrs, kept = 0, [], []
    for got, ref in zip(fused.recurrent_generator(adv_f, nmb, reuse_buffers=reuse), want):
        count += 1
        kept.append(got)       # (alive, so that a fresh minibatch cannot land where a freed one was)
        assert len(got) == len(ref) == 9 and list(got[0]) == list(ref[0])
        per = N // nmb
        assert tuple(got[1].shape) == (2, per, 8) and tuple(got[2].shape) == (steps * per, 2)
        for k in ref[0]:
            assert pu.same_bytes(got[0][k], ref[0][k]), k
        for i, (a, b) in enumerate(zip(got[1:], ref[1:]), 1):
            assert pu.same_bytes(a, b), i
        ptrs.append([t.data_ptr() for t in list(got[0].values()) + list(got[1:])])
    assert count == nmb == len(want)
    if nmb > 1:
        shared = [a == b for a, b in zip(ptrs[0], ptrs[1])]
        assert all(shared) if reuse else not any(shared)
    if reuse:
        assert fused._staging is not None and fused.to("cuda")._staging is None
