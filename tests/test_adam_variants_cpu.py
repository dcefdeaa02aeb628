"""CPU: the host side of wsmgmap.optim.Adam(amsgrad=True / maximize=True) and wsmgmap.optim.AdamW: construction, the validation that
stays (amsgrad=True over CPU parameters is refused at construction), torch.optim.Adam's / torch.optim.AdamW's state_dict layout in
both directions (CPU parameters: nothing is stepped here, the torch optimizers do the stepping), the flags each group steps with, and the four `_ext` entry points and three flag values in the
header and the binding.  The kernels are tested in tests/test_gpu_adam_variants.py."""
import copy
import ctypes
import inspect
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("wsmg_adam_step_multi_ext", "wsmg_adam_step_multi_dev_ext", "wsmg_adam_step_multi_guarded_ext", "wsmg_adam_step_multi_hyper_ext")
TORCH_HAS_DECOUPLED = "decoupled_weight_decay" in inspect.signature(torch.optim.Adam.__init__).parameters


def _param(n=5):
    return torch.nn.Parameter(torch.zeros(n))


def _stepped(cls, **kw):
    """state_dict() of a torch optimizer after three steps on one CPU parameter."""
    p = _param()
    opt = cls([p], lr=1e-3, **kw)
    for k in range(3):
        p.grad = torch.full((5,), 1.0 if k == 0 else 1e-3)    # one large gradient, then small ones: exp_avg_sq decays below its maximum
        opt.step()
    return opt.state_dict()


# ----------------------------------------------------------------------------- construction (these raise on the parent commit)
def test_the_variants_construct_and_report_their_flags():
    """maximize and AdamW construct over CPU parameters, as a plain Adam does (stepping them raises: no CPU path).  amsgrad=True is
    the device's: over CPU parameters it is refused at construction, by name (tests/test_host_cpu.py pins the ValueError); its
    construction over CUDA parameters is in tests/test_gpu_adam_variants.py."""
    from wsmgmap import optim
    m = optim.Adam([_param()], maximize=True)
    w = optim.AdamW([_param()])
    both = optim.AdamW([_param()], maximize=True, weight_decay=0.1)
    plain = optim.Adam([_param()], weight_decay=0.1)
    assert (optim.FLAG_AMSGRAD, optim.FLAG_MAXIMIZE, optim.FLAG_DECOUPLED_WD) == (1, 2, 4)
    assert [o._flags(o.param_groups[0]) for o in (plain, m, w, both)] == [0, 2, 4, 6]
    assert plain._flags({"amsgrad": True}) == 1 and both._flags({"amsgrad": True, "maximize": True}) == 7
    assert m.param_groups[0]["maximize"] is True and m.param_groups[0]["amsgrad"] is False
    assert w.param_groups[0]["weight_decay"] == 1e-2 == torch.optim.AdamW([_param()]).param_groups[0]["weight_decay"]
    assert isinstance(w, optim.Adam) and isinstance(w, torch.optim.Optimizer)
    assert both.param_groups[0]["weight_decay"] == 0.1
    for cls in (optim.Adam, optim.AdamW):
        with pytest.raises(ValueError, match="amsgrad=True.*CUDA parameters"):
            cls([_param()], amsgrad=True)
    with pytest.raises(ValueError, match="amsgrad=True.*CUDA parameters"):
        w.add_param_group({"params": [_param()], "amsgrad": True})
    assert len(w.param_groups) == 1
    # the state is lazy, like the moments: nothing before the first step
    assert len(m.state) == 0 and len(w.state) == 0
    # a plain construction holds what it held: no device state, not guarded
    assert plain._guard is None and plain._hyper is None and plain._guarded is False


def test_variants_combine_with_every_other_option_at_construction():
    from wsmgmap import optim
    net = torch.nn.BatchNorm1d(5)
    opt = optim.AdamW(net.parameters(), maximize=True, capturable=True, max_grad_norm=1.0, skip_nonfinite=True,
                      guard_buffers=net, hyper_on_device=True, grad_report=True)
    assert opt._flags(opt.param_groups[0]) == 6 and opt._guarded and opt._capturable and opt._hyper_on_device and opt._grad_report
    with pytest.raises(ValueError):                       # add_param_group's rules stay
        opt.add_param_group({"params": [_param()]})
    free = optim.AdamW([_param()], maximize=True)
    free.add_param_group({"params": [_param()], "maximize": False, "weight_decay": 0.0})
    assert [free._flags(g) for g in free.param_groups] == [6, 4]


def test_adam_takes_decoupled_weight_decay_where_torch_does():
    """torch.optim.Adam has the keyword in this torch or it has not: with it, ours takes it and `param_groups` carries it as torch's
    do; without it, ours refuses it by name and AdamW is the decoupled form all the same."""
    from wsmgmap import optim
    w = optim.AdamW([_param()])
    assert w._flags(w.param_groups[0]) == 4
    with pytest.raises(TypeError):
        optim.AdamW([_param()], decoupled_weight_decay=False)
    if TORCH_HAS_DECOUPLED:
        opt = optim.Adam([_param()], weight_decay=0.1, decoupled_weight_decay=True)
        assert opt.param_groups[0]["decoupled_weight_decay"] is True and opt._flags(opt.param_groups[0]) == 4
        assert optim.Adam([_param()], weight_decay=0.1).param_groups[0]["decoupled_weight_decay"] is False
        assert w.param_groups[0]["decoupled_weight_decay"] is True
    else:
        with pytest.raises(ValueError, match="decoupled_weight_decay"):
            optim.Adam([_param()], weight_decay=0.1, decoupled_weight_decay=True)
        assert "decoupled_weight_decay" not in w.param_groups[0]


@pytest.mark.parametrize("cls", ["Adam", "AdamW"])
@pytest.mark.parametrize("bad", [dict(lr=-1.0), dict(eps=-1e-8), dict(weight_decay=-0.1), dict(betas=(1.0, 0.999)), dict(betas=(0.9, -0.1)),
                                 dict(max_grad_norm=0.0), dict(max_grad_norm=float("nan")), dict(guard_buffers=torch.nn.BatchNorm1d(5)),
                                 dict(hyper_on_device=True), dict(grad_report=True)],
                         ids=["lr", "eps", "weight_decay", "beta1", "beta2", "max_grad_norm-0", "max_grad_norm-nan", "guard_buffers-alone",
                              "hyper-alone", "report-alone"])
def test_invalid_arguments_still_raise_with_the_variants_on(cls, bad):
    from wsmgmap import optim
    with pytest.raises(ValueError):
        getattr(optim, cls)([_param()], maximize=True, **bad)


def test_no_cpu_path_for_the_variants_either():
    from wsmgmap import _abi, optim
    for make in (lambda p: optim.Adam([p], maximize=True), lambda p: optim.AdamW([p]),
                 lambda p: optim.AdamW([p], maximize=True, max_grad_norm=1.0)):
        p = _param()
        p.grad = torch.ones(5)
        opt = make(p)
        with pytest.raises(_abi.WsmgError):
            opt.step()
        assert len(opt.state) == 0                        # refused before any state was made


# ----------------------------------------------------------------------------- state_dict, both ways
@pytest.mark.parametrize("name,kw", [("Adam", dict(amsgrad=True)), ("Adam", dict(amsgrad=True, maximize=True, weight_decay=0.1)),
                                     ("AdamW", {}), ("AdamW", dict(amsgrad=True))],
                         ids=["adam-amsgrad", "adam-amsgrad-maximize-wd", "adamw", "adamw-amsgrad"])
def test_state_dict_round_trips_with_torchs_optimizer(name, kw):
    """torch -> wsmgmap -> torch: three steps of the torch optimizer, loaded into ours (constructed with OTHER flags: the loaded
    param_groups carry them, as in torch — amsgrad too, which only a construction over CPU parameters refuses), saved again and
    loaded into a fresh torch optimizer, whose next step then equals the uninterrupted torch optimizer's bit for bit."""
    from wsmgmap import optim
    tcls = getattr(torch.optim, name)
    ref = _stepped(tcls, **kw)
    opt = getattr(optim, name)([_param()], lr=0.5)
    opt.load_state_dict(ref)
    mine = opt.state_dict()
    want_keys = {"step", "exp_avg", "exp_avg_sq"} | ({"max_exp_avg_sq"} if kw.get("amsgrad") else set())
    assert mine["state"].keys() == ref["state"].keys()
    for k in ref["state"]:
        assert set(mine["state"][k]) == set(ref["state"][k]) == want_keys
        step = mine["state"][k]["step"]
        assert isinstance(step, torch.Tensor) and step.dtype == torch.float32 and step.dim() == 0 and float(step) == 3.0
        for key in want_keys - {"step"}:
            assert torch.equal(mine["state"][k][key], ref["state"][k][key]), key
    if kw.get("amsgrad"):                                 # the inputs did exercise the maximum: v fell below it
        st = ref["state"][0]
        assert bool((st["max_exp_avg_sq"] > st["exp_avg_sq"]).all())
    group = mine["param_groups"][0]
    assert set(group) <= set(ref["param_groups"][0])
    for key in ("lr", "betas", "eps", "weight_decay", "amsgrad", "maximize"):
        assert group[key] == ref["param_groups"][0][key], key
    want_flags = ((1 if kw.get("amsgrad") else 0) | (2 if kw.get("maximize") else 0) | (4 if name == "AdamW" else 0))
    assert opt._flags(opt.param_groups[0]) == want_flags
    # and back: a fresh torch optimizer continues from our state_dict exactly as the original does
    pa, pb = _param(), _param()
    oa, ob = tcls([pa], lr=0.5), tcls([pb], lr=0.5)
    oa.load_state_dict(copy.deepcopy(ref))        # (load_state_dict adopts the tensors it is given: each optimizer its own)
    ob.load_state_dict(copy.deepcopy(mine))
    for p, o in ((pa, oa), (pb, ob)):
        p.grad = torch.full((5,), 0.25)
        o.step()
    assert torch.equal(pa, pb) and float(ob.state[pb]["step"]) == 4.0
    for key in want_keys - {"step"}:
        assert torch.equal(oa.state[pa][key], ob.state[pb][key]), key


def test_fresh_state_dict_of_each_variant_loads_into_torch():
    """wsmgmap -> torch without a step: the param_groups alone (no state yet) are ones torch's classes accept and step with."""
    from wsmgmap import optim
    for name, kw in (("Adam", dict(maximize=True)), ("AdamW", dict(maximize=True))):
        sd = getattr(optim, name)([_param()], lr=2e-3, **kw).state_dict()
        p = _param()
        t = getattr(torch.optim, name)([p], lr=0.5)
        t.load_state_dict(sd)
        assert t.param_groups[0]["lr"] == 2e-3 and t.param_groups[0]["maximize"] is True and t.param_groups[0]["amsgrad"] is False
        p.grad = torch.ones(5)
        t.step()
        assert bool((p > 0).all())                        # maximized: the parameter moved along the gradient


# ----------------------------------------------------------------------------- header and binding
def test_header_declares_the_ext_entry_points_and_the_flag_values():
    from wsmgmap import _abi
    header = open(os.path.join(ROOT, "include", "wsmgmap.h")).read()
    consts = {k: int(v) for k, v in re.findall(r"\b(WSMG_ADAM_[A-Z_]+)\s*=\s*(\d+)", header)}
    assert consts == {"WSMG_ADAM_AMSGRAD": 1, "WSMG_ADAM_MAXIMIZE": 2, "WSMG_ADAM_DECOUPLED_WD": 4}
    sig, restype, structs = _abi.parse_header(header)
    P, I, F, D = ctypes.c_void_p, ctypes.c_int, ctypes.c_float, ctypes.c_double
    want = {"wsmg_adam_step_multi_ext": [P, I, P, I, F, F, F, F, F, D, D, P],
            "wsmg_adam_step_multi_dev_ext": [P, I, P, I, F, F, F, F, F, P, P],
            "wsmg_adam_step_multi_guarded_ext": [P, I, P, I, F, F, F, F, F, P, P, P],
            "wsmg_adam_step_multi_hyper_ext": [P, I, P, I, P, P, P, P]}
    assert set(want) == set(NAMES)
    L = _abi.lib()
    for name in NAMES:
        assert sig[name] == want[name] and restype[name] is I, name
        # the binding of every new name comes from the header: what the loaded function carries is the parse
        fn = getattr(L, name)
        assert list(fn.argtypes) == sig[name] == _abi._SIG[name] and fn.restype is restype[name]
        assert name in _abi.exported_names()
        # each mirrors the entry point without `_ext`: its arguments with (max_exp_avg_sq, flags) behind (descs, n)
        base = sig[name[:-len("_ext")]]
        assert sig[name] == base[:2] + [P, I] + base[2:], name
    # WsmgAdamDesc keeps its layout: the fifth pointer travels beside it
    assert [n for n, _ in structs["WsmgAdamDesc"]] == ["param", "grad", "exp_avg", "exp_avg_sq", "n"]
