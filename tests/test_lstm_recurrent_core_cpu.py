"""CPU: the C ABI of the chained LSTM state-encoder launches (wsmg_lstm_state_fwd_chain / _bwd_chain, the pipelined recurrent
core's form for rnn_type "LSTM"): exported, declared as their _SIG entries say, and refusing every unsupported argument with
WSMG_EINVAL before anything is enqueued (the launches themselves are tested on the GPU, tests/test_gpu_lstm_recurrent_core.py)."""
import ctypes

import pytest

EINVAL = -1
NAMES = ("wsmg_lstm_state_fwd_chain", "wsmg_lstm_state_bwd_chain", "wsmg_lstm_state_chain_workgroups")


@pytest.mark.parametrize("name", NAMES)
def test_chain_symbols_are_exported_and_match_the_header(name):
    """(Every argument against the header's declaration: tests/test_abi_cpu.py.)"""
    from wsmgmap import _abi
    L = _abi.lib()
    assert hasattr(L, name) and name in _abi.exported_names()
    assert getattr(L, name).restype is ctypes.c_int
    assert len(_abi._SIG[name]) == {NAMES[0]: 19, NAMES[1]: 20, NAMES[2]: 0}[name]
    assert _abi.lib().wsmg_abi_version() == 1


def test_chain_workgroups_is_the_grid_of_the_lstm_kernels():
    from wsmgmap import _abi
    L = _abi.lib()
    assert L.wsmg_lstm_state_chain_workgroups() == 32 == L.wsmg_gru_chain_workgroups()
    assert L.wsmg_rows_gemm_supported(4 * 512) == 1       # the LSTM core's dxc product (K = 4 H)


class _Dummy:
    """128-byte-aligned dummy addresses: never dereferenced, because every case below is refused before anything is enqueued."""
    base = 1 << 20

    def __init__(self):
        self.k = 0

    def __call__(self):
        self.k += 1
        return ctypes.c_void_p(self.base + 4096 * self.k)


def _fwd(L, **over):
    d = _Dummy()
    a = dict(gi=d(), w_hh=d(), b_hh=d(), h0=d(), c0=d(), masks=d(), T=8, N=4, hidden=512, y=d(), c_T=d(), save_gates=d(),
             save_c=d(), sync_ws=d(), steps_per_chunk=2, in_count=None, in_target=0, out_count=None, stream=None)
    a.update(over)
    return L.wsmg_lstm_state_fwd_chain(*a.values())


def _bwd(L, **over):
    d = _Dummy()
    a = dict(dy=d(), dhT=None, dcT=None, w_hh=d(), c0=d(), masks=d(), save_gates=d(), save_c=d(), T=8, N=4, hidden=512,
             dgates=d(), dh0=d(), dc0=d(), sync_ws=d(), steps_per_chunk=2, in_count=None, in_target=0, out_count=None, stream=None)
    a.update(over)
    return L.wsmg_lstm_state_bwd_chain(*a.values())


REFUSALS = [dict(steps_per_chunk=0), dict(steps_per_chunk=-2), dict(steps_per_chunk=3), dict(T=10, steps_per_chunk=4),
            dict(hidden=256), dict(hidden=128), dict(N=9), dict(N=0), dict(T=1024, steps_per_chunk=1), dict(T=0),
            dict(sync_ws=ctypes.c_void_p((1 << 20) + 64))]
FWD_NEEDS = ("gi", "w_hh", "b_hh", "h0", "c0", "masks", "y", "c_T", "save_gates", "save_c", "sync_ws")
BWD_NEEDS = ("dy", "w_hh", "c0", "masks", "save_gates", "save_c", "dgates", "dh0", "dc0", "sync_ws")


@pytest.mark.parametrize("over", REFUSALS, ids=lambda o: ",".join(f"{k}={v}" for k, v in o.items()))
def test_chain_entry_points_refuse_unsupported_shapes(over):
    from wsmgmap import _abi
    L = _abi.lib()
    assert _fwd(L, **over) == EINVAL
    assert _bwd(L, **over) == EINVAL


def test_chain_entry_points_refuse_null_pointers_they_need():
    from wsmgmap import _abi
    L = _abi.lib()
    for n in FWD_NEEDS:
        assert _fwd(L, **{n: None}) == EINVAL, n
    for n in BWD_NEEDS:
        assert _bwd(L, **{n: None}) == EINVAL, n
    # the plain entry points take the same checks (Tc = 0: no chaining)
    assert L.wsmg_lstm_state_fwd(*[None] * 6, 8, 4, 512, *[None] * 5, None) == EINVAL
    assert L.wsmg_lstm_state_bwd(*[None] * 8, 8, 4, 512, *[None] * 4, None) == EINVAL
