"""CPU: the host side of the guarded Adam step (wsmgmap.optim.Adam(max_grad_norm=..., skip_nonfinite=...)): constructor
validation, no device state for a default construction, torch.optim.Adam's state_dict layout with the options on, and the two
entry points in the header and the binding.  The kernels are tested in tests/test_gpu_adam_guard.py."""
import pytest
import torch

NAMES = ("wsmg_grad_norm_multi", "wsmg_adam_step_multi_guarded")


def _param(n=5):
    return torch.nn.Parameter(torch.zeros(n))


@pytest.mark.parametrize("bad", [0.0, -1.0, float("nan"), float("inf"), -float("inf")])
def test_invalid_max_grad_norm_is_refused_at_construction(bad):
    from wsmgmap import optim
    with pytest.raises(ValueError):
        optim.Adam([_param()], max_grad_norm=bad)
    with pytest.raises(ValueError):
        optim.Adam([_param()], max_grad_norm=bad, skip_nonfinite=True)


def test_valid_options_construct_and_defaults_hold_no_guard_state():
    """The defaults are the object of before: not guarded, no guard record, no step count on the device, no workspace.  With an
    option on (CPU parameters here: nothing to allocate on) the properties answer without a device."""
    from wsmgmap import _abi, optim
    opt = optim.Adam([_param()], lr=1e-3)
    assert opt._guarded is False and opt._guard is None and opt._guard_step is None and opt._partials is None
    assert opt.grad_norm is None and opt.skipped_steps == 0
    for kw in (dict(max_grad_norm=1.0), dict(skip_nonfinite=True), dict(max_grad_norm=0.5, skip_nonfinite=True)):
        g = optim.Adam([_param()], lr=1e-3, **kw)
        assert g._guarded is True and g.skipped_steps == 0 and g.grad_norm is None
        p = g.param_groups[0]["params"][0]
        p.grad = torch.ones(5)
        with pytest.raises(_abi.WsmgError):      # no CPU path, guarded or not
            g.step()
    with pytest.raises(_abi.WsmgError):
        optim.global_grad_norm([_param()])       # no gradients at all
    p = _param()
    p.grad = torch.ones(5)
    with pytest.raises(_abi.WsmgError):
        optim.global_grad_norm([p])              # a CPU gradient


def test_state_dict_layout_is_torch_adams_with_the_options_on():
    from wsmgmap import optim
    tp = _param()
    tp.grad = torch.ones(5)
    ref_opt = torch.optim.Adam([tp], lr=1e-3)
    for _ in range(3):
        ref_opt.step()
    ref = ref_opt.state_dict()
    opt = optim.Adam([_param()], lr=1e-3, max_grad_norm=1.0, skip_nonfinite=True)
    opt.load_state_dict(ref)
    mine = opt.state_dict()
    assert mine["state"].keys() == ref["state"].keys()
    for k in ref["state"]:
        assert set(mine["state"][k]) == set(ref["state"][k]) == {"step", "exp_avg", "exp_avg_sq"}
        step = mine["state"][k]["step"]
        assert isinstance(step, torch.Tensor) and step.dtype == torch.float32 and step.dim() == 0 and float(step) == 3.0
        assert torch.equal(mine["state"][k]["exp_avg"], ref["state"][k]["exp_avg"])
    assert set(mine["param_groups"][0]) <= set(ref["param_groups"][0])
    torch.optim.Adam([_param()], lr=1e-3).load_state_dict(mine)     # and torch's optimizer takes it back


def test_entry_points_are_declared_bound_and_exported():
    """(Their declarations against the binding: tests/test_abi_cpu.py.)"""
    from wsmgmap import _abi
    L = _abi.lib()
    for name in NAMES:
        assert name in _abi.exported_names() and hasattr(L, name)
    assert L.wsmg_abi_version() == 1
