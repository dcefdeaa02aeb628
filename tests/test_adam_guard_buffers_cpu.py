"""CPU: the host side of the BatchNorm roll-back of a skipped guarded step (wsmgmap.optim.Adam(skip_nonfinite=True,
guard_buffers=module), wsmg_copy_multi_guarded): the entry point is exported, declared as its _SIG entry says, and refuses every
unsupported argument with WSMG_EINVAL before anything is enqueued (no GPU is present here, so a launch would be an error of its
own); the constructor's checks; and a construction without the option holds nothing of it.  The kernel and the optimizer's device
side are tested in tests/test_gpu_adam_guard_buffers.py."""
import ctypes

import pytest
import torch

EINVAL = -1
NAME = "wsmg_copy_multi_guarded"
A, B, G = 1 << 20, 2 << 20, 3 << 20        # dummy addresses: never dereferenced, every call below is refused


def _descs(*rows):
    from wsmgmap import _abi
    d = (_abi.CopyDesc * len(rows))()
    for x, (dst, src, nbytes) in zip(d, rows):
        x.dst, x.src, x.bytes = dst, src, nbytes
    return d


def test_entry_point_is_exported_declared_and_bound():
    """(The declaration's own words — a WsmgCopyDesc list, a count, a float guard record, the stream: tests/test_abi_cpu.py.)"""
    from wsmgmap import _abi
    assert _abi._SIG[NAME] == [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p]
    L = _abi.lib()
    assert NAME in _abi.exported_names() and hasattr(L, NAME)
    assert L.wsmg_abi_version() == 1


REFUSED = {
    "null-descs": lambda d: (None, 1, G),
    "null-guard": lambda d: (d, 1, None),
    "n-zero": lambda d: (d, 0, G),
    "n-negative": lambda d: (d, -1, G),
}


@pytest.mark.parametrize("case", sorted(REFUSED))
def test_rejected_call_arguments_return_einval(case):
    from wsmgmap import _abi
    d = _descs((A, B, 16))
    descs, n, guard = REFUSED[case](d)
    descs = None if descs is None else ctypes.cast(descs, ctypes.c_void_p)
    assert _abi.lib().wsmg_copy_multi_guarded(descs, n, None if guard is None else ctypes.c_void_p(guard), None) == EINVAL


@pytest.mark.parametrize("at", [0, 1, 49, 99], ids=lambda a: f"desc{a}")
@pytest.mark.parametrize("bad", [(None, B, 16), (A, None, 16), (A, B, -1), (None, None, 1)],
                         ids=["null-dst", "null-src", "negative-bytes", "null-both"])
def test_a_rejected_descriptor_anywhere_in_the_list_returns_einval(bad, at):
    """The bad descriptor in the first launch's table, at its edge and in the third launch's (48 per launch): refused before
    the first launch, so the good descriptors in front of it are never enqueued."""
    from wsmgmap import _abi
    rows = [(A + 64 * i, B + 64 * i, 16) for i in range(100)]
    rows[at] = bad
    d = _descs(*rows)
    assert _abi.lib().wsmg_copy_multi_guarded(ctypes.cast(d, ctypes.c_void_p), len(rows), ctypes.c_void_p(G), None) == EINVAL


def _param(n=5):
    return torch.nn.Parameter(torch.zeros(n))


def test_guard_buffers_needs_skip_nonfinite():
    from wsmgmap import optim
    m = torch.nn.BatchNorm1d(5)
    with pytest.raises(ValueError):
        optim.Adam([_param()], guard_buffers=m)
    with pytest.raises(ValueError):
        optim.Adam([_param()], max_grad_norm=1.0, guard_buffers=m)      # clipping alone never skips
    opt = optim.Adam([_param()], skip_nonfinite=True, guard_buffers=m)
    assert opt._guard_buffers is m and opt._snap is None                 # nothing is allocated before the first snapshot


def test_default_construction_holds_no_snapshot_state():
    from wsmgmap import _abi, optim
    for kw in ({}, dict(skip_nonfinite=True), dict(max_grad_norm=1.0)):
        opt = optim.Adam([_param()], lr=1e-3, **kw)
        assert opt._guard_buffers is None
        assert opt._snap is None and opt._snap_save is None and opt._snap_restore is None
        assert opt._snap_slots is None and opt._snap_bufs is None and opt._snap_ptrs is None
        assert opt._snap_fresh is False
        opt.zero_grad()                                                  # takes no snapshot, needs none
        assert opt._snap is None and opt._snap_fresh is False
        with pytest.raises(_abi.WsmgError):
            opt.snapshot_buffers()


def test_unsupported_modules_are_refused_at_the_first_snapshot_by_name():
    """No device here: a module without tracked statistics and one whose buffers are CPU tensors are both refused before any
    call into the library, the second by the buffer's qualified name."""
    from wsmgmap import _abi, optim
    none = torch.nn.Sequential(torch.nn.Linear(5, 5), torch.nn.BatchNorm1d(5, track_running_stats=False))
    opt = optim.Adam(none.parameters(), skip_nonfinite=True, guard_buffers=none)
    with pytest.raises(_abi.WsmgError, match="no BatchNorm"):
        opt.zero_grad()
    cpu = torch.nn.Sequential(torch.nn.Linear(5, 5), torch.nn.BatchNorm1d(5))
    opt = optim.Adam(cpu.parameters(), skip_nonfinite=True, guard_buffers=cpu)
    with pytest.raises(_abi.WsmgError, match=r"1\.running_mean"):
        opt.snapshot_buffers()
    assert opt._snap is None and opt._snap_fresh is False
    sd = opt.state_dict()
    assert set(sd) == {"state", "param_groups"} and "guard_buffers" not in sd["param_groups"][0]
