"""The write side of the sparse ego map, host part (no GPU needed): the step selection of `wsmgmap.data.recorder` against
`codec.sparse_pack_ego` on the dense map, records written from the selected arrays against `pack_record_raw(..., sparse_ego=True)`,
and the refusals of the packing entry point before anything is enqueued."""
import numpy as np
import pytest

C, H, W, T = 64, 5, 7, 9


def _dense(seed=3):
    """float16 [T, 64, H, W]: post-ReLU steps of ~30 % non-zeros, with an all-zero step (4), an all-non-zero step (6) and -0.0."""
    rng = np.random.RandomState(seed)
    ego = (np.maximum(rng.randn(T, C, H, W), 0.52) - 0.52).astype(np.float16)
    ego[4] = 0
    ego[6] = (rng.randn(C, H, W) + 4).astype(np.float16)
    ego[2, 5, 1, 2] = np.float16(-0.0)
    return ego


def _pieces(ego):
    """Every step packed on its own by the codec: what SparseEgoRecorder stores per step."""
    from wsmgmap.data import sparse_pack_ego
    out = []
    for t in range(ego.shape[0]):
        one = sparse_pack_ego(ego[t:t + 1])
        out.append((one["rgb_ego_map__bits"][0], one["rgb_ego_map__off"][0], one["rgb_ego_map__vals"]))
    return out


def _same(got, want):
    assert list(got) == list(want)                       # the same keys in the same order
    for k in want:
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, k
        assert got[k].tobytes() == want[k].tobytes(), k


@pytest.mark.parametrize("idx", [list(range(T)), [0], list(range(2, T, 3)), [3, 4, 5], [4], [7, 1, 1], []],
                         ids=["all", "first", "range_2_T_3", "around_empty_step", "empty_step_alone", "unordered_repeat", "none"])
def test_selected_steps_equal_the_codec_on_the_dense_selection(idx):
    from wsmgmap.data import select_steps, sparse_pack_ego
    ego = _dense()
    got = select_steps(_pieces(ego), idx, (C, H, W))
    _same(got, sparse_pack_ego(ego[idx]))


def test_record_of_taken_arrays_is_the_sparse_record_of_the_dense_map():
    from wsmgmap.data import densify, pack_record_raw, select_steps, unpack_record
    ego = _dense(5)
    rng = np.random.RandomState(6)
    idx = list(range(2, T, 3))
    n = len(idx)
    other = {"instruction": rng.randint(0, 27, size=(n, 6)).astype(np.int64), "progress": rng.rand(n, 1).astype(np.float32)}
    prev, oracle = rng.randn(n, 2).astype(np.float32), rng.randn(n, 2).astype(np.float32)
    taken = select_steps(_pieces(ego), idx, (C, H, W))
    blob = pack_record_raw({**other, **taken}, prev, oracle)
    want = pack_record_raw({**other, "rgb_ego_map": ego[idx]}, prev, oracle, sparse_ego=True)
    assert blob == want
    obs, p2, o2 = unpack_record(blob)
    back = densify(obs)
    assert back["rgb_ego_map"].dtype == np.float16
    assert back["rgb_ego_map"].view(np.uint16).tobytes() == np.ascontiguousarray(ego[idx]).view(np.uint16).tobytes()
    assert np.array_equal(p2, prev) and np.array_equal(o2, oracle) and np.array_equal(back["instruction"], other["instruction"])


def test_ego_sparse_pack_abi_refuses_before_enqueuing():
    """wsmg_ego_sparse_pack returns WSMG_EINVAL — with no device in the machine, so before any launch — for a channel count other
    than 64, an empty map, a map whose offsets would not fit 32 bits, and null pointers."""
    import ctypes
    from wsmgmap import _abi
    L = _abi.lib()
    assert "wsmg_ego_sparse_pack" in _abi.exported_names()
    buf = (ctypes.c_uint64 * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    for B, Cc, HW in ((1, 40, 4), (1, 32, 4), (1, 128, 4), (1, 64, 0), (1, 64, -3), (0, 64, 4), (1, 64, 1 << 26)):
        assert L.wsmg_ego_sparse_pack(p, B, Cc, HW, p, p, p, p, None) == -1, (B, Cc, HW)
    for hole in range(5):
        args = [p] * 5
        args[hole] = None
        assert L.wsmg_ego_sparse_pack(args[0], 1, 64, 4, args[1], args[2], args[3], args[4], None) == -1, hole


def test_recorder_and_wrapper_refuse_the_cpu():
    import torch
    from wsmgmap import _abi, ops
    from wsmgmap.data import SparseEgoRecorder
    with pytest.raises(_abi.WsmgError):
        ops.ego_sparse_pack(torch.zeros(1, 2, 2, 64))
    with pytest.raises(_abi.WsmgError):
        SparseEgoRecorder(2, "cpu")
