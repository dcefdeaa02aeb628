"""CPU: the host side of wsmgmap.optim.Adam(hyper_on_device=True) — the hyper-parameters read from a device record so that a step
captured in a HIP graph follows schedules: the two entry points in the header and the binding, the constructor's and the
`max_grad_norm` setter's refusals, and a default construction that is the object it was.  The kernels, `sync_hyper()` and the graph
replay are tested in tests/test_gpu_adam_hyper.py."""
import pytest
import torch

NAMES = ("wsmg_adam_step_multi_hyper", "wsmg_grad_norm_multi_hyper")


def _param(n=5):
    return torch.nn.Parameter(torch.zeros(n))


def test_entry_points_are_declared_bound_and_exported():
    """(Their declarations against the binding, and the record's layout documented next to the guard record's: tests/test_abi_cpu.py.)"""
    from wsmgmap import _abi
    L = _abi.lib()
    for name in NAMES:
        assert name in _abi.exported_names() and hasattr(L, name)
    assert len(getattr(L, NAMES[0]).argtypes) == 6 and len(getattr(L, NAMES[1]).argtypes) == 9
    assert L.wsmg_abi_version() == 1


def test_hyper_on_device_needs_a_step_count_on_the_device():
    from wsmgmap import optim
    with pytest.raises(ValueError, match="capturable"):
        optim.Adam([_param()], hyper_on_device=True)
    for kw in (dict(capturable=True), dict(max_grad_norm=1.0), dict(skip_nonfinite=True)):
        opt = optim.Adam([_param()], hyper_on_device=True, **kw)
        # CPU parameters: nothing to allocate on (step() refuses them), and nothing to synchronise
        assert opt._hyper is None and opt._hyper_stage is None and opt.hyper_record is None and opt.sync_hyper() is False
        with pytest.raises(ValueError, match="add_param_group"):
            opt.add_param_group({"params": [_param()]})


def test_max_grad_norm_is_a_validated_property():
    from wsmgmap import optim
    opt = optim.Adam([_param()], max_grad_norm=2.0)
    assert opt.max_grad_norm == 2.0
    opt.max_grad_norm = 0.5
    assert opt.max_grad_norm == 0.5 and isinstance(opt.max_grad_norm, float)
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            opt.max_grad_norm = bad
        assert opt.max_grad_norm == 0.5
    with pytest.raises(ValueError, match="on or off"):      # clipping off: another path than the one a graph captured
        opt.max_grad_norm = None
    for kw in (dict(), dict(skip_nonfinite=True)):
        off = optim.Adam([_param()], **kw)
        assert off.max_grad_norm is None
        off.max_grad_norm = None                             # no change
        with pytest.raises(ValueError, match="on or off"):
            off.max_grad_norm = 1.0
        assert off.max_grad_norm is None


def test_default_construction_is_the_object_it_was():
    """No flag: not a tensor more on the object than before (the guard's and the snapshot's slots stay None), sync_hyper() is a no-op
    that returns False, add_param_group works, and the state_dict has torch.optim.Adam's keys only."""
    from wsmgmap import optim
    opt = optim.Adam([_param()], lr=1e-3)
    assert opt._hyper_on_device is False and opt.sync_hyper() is False and opt.hyper_record is None
    held = {k: v for k, v in vars(opt).items() if torch.is_tensor(v)}
    assert not held, f"a default Adam holds tensors: {sorted(held)}"
    for k in ("_hyper", "_hyper_stage", "_hyper_mirror", "_hyper_event", "_guard", "_guard_step", "_partials", "_snap"):
        assert getattr(opt, k) is None, k
    opt.add_param_group({"params": [_param()], "lr": 5e-4})
    assert len(opt.param_groups) == 2 and opt.param_groups[1]["lr"] == 5e-4
    ref = torch.optim.Adam([_param()], lr=1e-3).state_dict()
    assert set(opt.state_dict()["param_groups"][0]) <= set(ref["param_groups"][0])
    flagged = optim.Adam([_param()], lr=1e-3, capturable=True, hyper_on_device=True)
    assert set(flagged.state_dict()) == set(ref) and set(flagged.state_dict()["param_groups"][0]) <= set(ref["param_groups"][0])
