"""CPU: the host side of the per-tensor gradient report — wsmgmap.optim.Adam(grad_report=True), `grad_report()`, `last_skipped()`,
wsmgmap.optim.grad_stats — the two entry points in the header and the binding, the constructor's refusals, and a default construction
that holds nothing new.  The kernels, the latch and the graph replay are tested in tests/test_gpu_adam_grad_report.py."""
import pytest
import torch

NAMES = ("wsmg_grad_report_multi", "wsmg_grad_stats_multi")


def _param(n=5):
    return torch.nn.Parameter(torch.zeros(n))


def test_entry_points_are_declared_bound_and_exported():
    """(Their declarations against the binding: tests/test_abi_cpu.py.)"""
    from wsmgmap import _abi
    L = _abi.lib()
    for name in NAMES:
        assert name in _abi.exported_names() and hasattr(L, name)
    assert len(getattr(L, NAMES[0]).argtypes) == 11 and len(getattr(L, NAMES[1]).argtypes) == 8
    assert L.wsmg_abi_version() == 1


def test_grad_report_needs_the_guarded_step():
    from wsmgmap import optim
    with pytest.raises(ValueError, match="guarded step"):
        optim.Adam([_param()], grad_report=True)
    with pytest.raises(ValueError, match="guarded step"):
        optim.Adam([_param()], capturable=True, grad_report=True)


@pytest.mark.parametrize("kw", [dict(skip_nonfinite=True), dict(max_grad_norm=1.0), dict(max_grad_norm=1.0, skip_nonfinite=True),
                                dict(skip_nonfinite=True, hyper_on_device=True)], ids=["skip", "clip", "clip+skip", "skip+hyper"])
def test_cpu_parameters_construct_answer_empty_and_refuse_to_step(kw):
    from wsmgmap import _abi, optim
    ps = [_param(), _param(3)]
    opt = optim.Adam(ps, grad_report=True, **kw)
    assert opt._report is None and opt._latch is None and opt._scan is None          # nothing to allocate on
    assert opt.grad_report() == [] and opt.grad_report(["a", "b"]) == [] and opt.last_skipped() is None
    for p in ps:
        p.grad = torch.ones_like(p)
    with pytest.raises(_abi.WsmgError):
        opt.step()
    with pytest.raises(ValueError, match="add_param_group"):
        opt.add_param_group({"params": [_param()]})


def test_default_construction_holds_no_report_state():
    from wsmgmap import optim
    for kw in (dict(), dict(skip_nonfinite=True), dict(capturable=True)):
        opt = optim.Adam([_param()], lr=1e-3, **kw)
        assert opt._grad_report is False
        for k in ("_report", "_latch", "_scan"):
            assert getattr(opt, k) is None, k
        assert opt.grad_report() == [] and opt.last_skipped() is None
        assert not {k: v for k, v in vars(opt).items() if torch.is_tensor(v)}
        opt.add_param_group({"params": [_param()]})          # still allowed without the flag
        assert len(opt.param_groups) == 2


def test_state_dict_layout_is_torch_adams_with_the_option_on():
    from wsmgmap import optim
    ref = torch.optim.Adam([_param()], lr=1e-3).state_dict()
    opt = optim.Adam([_param()], lr=1e-3, skip_nonfinite=True, grad_report=True)
    sd = opt.state_dict()
    assert set(sd) == set(ref) and set(sd["param_groups"][0]) <= set(ref["param_groups"][0])
    assert sd["state"] == {} and sd["param_groups"][0]["params"] == [0]
    opt.load_state_dict(sd)                                  # re-creates the guard's tables where there is a device: none here
    assert opt._report is None and opt.last_skipped() is None


def test_names_follow_param_groups_order():
    from wsmgmap import optim
    lin = torch.nn.Linear(3, 2)
    extra = _param()
    opt = optim.Adam([{"params": [lin.bias, extra]}, {"params": [lin.weight]}], skip_nonfinite=True, grad_report=True)
    assert opt._report_names(None) == ["group0.param0", "group0.param1", "group1.param0"]
    assert opt._report_names(lin) == ["bias", "group0.param1", "weight"]              # by identity; a stranger keeps its default
    assert opt._report_names(("b", "x", "w")) == ["b", "x", "w"]
    with pytest.raises(ValueError):
        opt._report_names(["only-one"])


def test_grad_stats_refuses_cpu_or_absent_gradients():
    from wsmgmap import _abi, optim
    p = _param()
    with pytest.raises(_abi.WsmgError, match="no parameter has a gradient"):
        optim.grad_stats([p])
    p.grad = torch.ones(5)
    with pytest.raises(_abi.WsmgError, match="CUDA"):
        optim.grad_stats([p, _param()])
    table = torch.tensor([[0x3f800000, 0x40000000, 3, -1]], dtype=torch.int32)
    assert optim.stats_as_float(table).tolist() == [[1.0, 2.0]]
    assert optim._stats_rows(table, ["w"]) == [optim.GradStat(0, "w", 1.0, 2.0, 3, 0xffffffff)]
