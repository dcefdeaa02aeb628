"""CPU: the policy-gradient surface without a GPU — the float64 yardstick of tests/pg_util.py against the project's own
DiagGaussian, the four new entry points' names and refusals, `BasePolicy.evaluate_actions` / `get_value` on their composed (CPU)
route, and the branch coverage of the PPO test rows.  The kernels are tested on the GPU (tests/test_gpu_pg_heads.py)."""
import ctypes

import pytest
import torch
import torch.nn as nn

import pg_util as pu

EINVAL = -1
NEW = ("wsmg_eval_heads_fwd", "wsmg_eval_heads_bwd", "wsmg_ppo_loss_fwd", "wsmg_ppo_loss_bwd")


# ----------------------------------------------------------------------------- 1. the yardstick against DiagGaussian
@pytest.mark.parametrize("shape", [(5, 512, 2), (3, 8, 4), (1, 4, 1)], ids=["B5_K512_A2", "B3_K8_A4", "B1_K4_A1"])
def test_oracle_agrees_with_the_projects_diag_gaussian_in_float64(shape):
    from wsmgmap.common.distributions import DiagGaussian
    from wsmgmap.models.policy import CriticHead
    B, K, A = shape
    (x, wm, bm, ls, wc, bc, action), _ = pu.eval_inputs(B, K, A)
    ad, critic = DiagGaussian(K, A).double(), CriticHead(K).double()
    with torch.no_grad():
        for p, v in ((ad.fc_mean.weight, wm), (ad.fc_mean.bias, bm), (ad.logstd._bias, ls), (critic.fc.weight, wc), (critic.fc.bias, bc)):
            p.copy_(v.double())
    dist = ad(x.double())
    value, logp, entropy, mean = pu.eval_heads_ref(x, wm, bm, ls, wc, bc, action)
    assert value.dtype == logp.dtype == entropy.dtype == torch.float64
    assert tuple(value.shape) == (B, 1) and tuple(logp.shape) == (B,) and entropy.dim() == 0
    close = lambda a, b: torch.allclose(a, b, rtol=1e-13, atol=1e-13)      # noqa: E731
    assert close(logp, dist.log_probs(action.double())) and close(entropy, dist.entropy().mean())
    assert close(value, critic(x.double())) and close(mean, dist.mean)
    # ... and with the closed forms the kernels are written from
    lsd, d = ls.double().view(1, A), action.double() - mean
    half_log_2pi = 0.5 * torch.log(torch.tensor(2 * torch.pi, dtype=torch.float64))
    assert close(logp, (-(d * d) / (2 * torch.exp(2 * lsd)) - lsd - half_log_2pi).sum(-1))
    assert close(entropy, (0.5 + half_log_2pi + lsd).sum())


def test_ppo_rows_sit_on_every_branch():
    """Every size the GPU test uses from 255 rows up holds every branch combination; the rows are off every tie and clamp edge."""
    for B in (255, 256, 257, 2049):
        (logp, old_logp, adv, value, old_value, ret), _ = pu.ppo_inputs(B)
        ratio = torch.exp(logp.double() - old_logp.double())
        clip = pu.f32_scalar(pu.CLIP)
        lo, hi = 1 - clip, 1 + clip
        for side in (ratio < lo, (ratio > lo) & (ratio < hi) & (ratio != 1), ratio == 1, ratio > hi):
            for sgn in (adv > 0, adv < 0, adv == 0):
                assert int((side & sgn).sum()) > 0
        assert float(torch.minimum((ratio - lo).abs(), (ratio - hi).abs()).min()) > 1e-2
        dv = value.double() - old_value.double()
        vc = old_value.double() + dv.clamp(-clip, clip)
        l1, l2 = (value.double() - ret.double()) ** 2, (vc - ret.double()) ** 2
        inside = dv.abs() < clip
        assert int(inside.sum()) > 0 and int((~inside & (l1 > l2)).sum()) > 0 and int((~inside & (l2 > l1)).sum()) > 0
        assert float((dv.abs() - clip).abs().min()) > 1e-2 and float((l1 - l2)[~inside].abs().min()) > 1e-2


# ----------------------------------------------------------------------------- 2. names
def test_new_entry_points_and_operators_are_exported():
    from wsmgmap import _abi, ops
    from wsmgmap.ops import heads
    lib = _abi.lib()
    for name in NEW:
        assert name in _abi.exported_names() and hasattr(lib, name), name
        assert getattr(lib, name).restype is ctypes.c_int
    for name in ("eval_heads", "ppo_loss", "eval_heads_ok"):
        assert getattr(ops, name) is getattr(heads, name)


def test_policy_has_habitats_two_methods():
    from wsmgmap.models.policy import BasePolicy, CMAPolicy
    assert callable(BasePolicy.evaluate_actions) and callable(BasePolicy.get_value) and CMAPolicy is BasePolicy


# ----------------------------------------------------------------------------- 3. refusals through the C ABI, no device needed
_BUF = (ctypes.c_uint64 * 64)()
_P = ctypes.cast(_BUF, ctypes.c_void_p)      # host memory that is never dereferenced: every case must be refused before a launch

_ARGS = {
    "wsmg_eval_heads_fwd": dict(x=_P, wm=_P, bm=_P, logstd=_P, wc=_P, bc=_P, action=_P, B=4, K=512, A=2, value=_P, logp=_P, mean=_P,
                                entropy=_P, stream=None),
    "wsmg_eval_heads_bwd": dict(x=_P, wm=_P, wc=_P, logstd=_P, action=_P, mean=_P, dvalue=_P, dlogp=_P, dentropy=_P, B=4, K=512, A=2,
                                dx=_P, dwm=_P, dbm=_P, dlogstd=_P, dwc=_P, dbc=_P, stream=None),
    "wsmg_ppo_loss_fwd": dict(logp=_P, old_logp=_P, adv=_P, value=_P, old_value=_P, ret=_P, mask=_P, entropy=_P, clip=0.2, value_coef=0.5,
                              entropy_coef=0.01, clipped_value=1, B=8, out5=_P, nsel=_P, stream=None),
    "wsmg_ppo_loss_bwd": dict(logp=_P, old_logp=_P, adv=_P, value=_P, old_value=_P, ret=_P, mask=_P, nsel=_P, dloss=_P, clip=0.2,
                              value_coef=0.5, entropy_coef=0.01, clipped_value=1, B=8, dlogp=_P, dvalue=_P, dentropy=_P, stream=None),
}
_OPTIONAL = {"dvalue", "dlogp", "dentropy", "mask", "stream"}      # may be null


def _refusals():
    out = []
    for name, args in _ARGS.items():
        sizes = [("B", 0), ("B", -1)]
        sizes += [("A", 0), ("A", 5), ("K", 6), ("K", 0)] if "A" in args else [("B", (1 << 20) + 1)]
        out += [(name, k, v) for k, v in sizes]
        out += [(name, k, None) for k, v in args.items() if v is _P and k not in _OPTIONAL]
    return out


@pytest.mark.parametrize("name,key,bad", _refusals(), ids=lambda v: "null" if v is None else str(v))
def test_new_entry_points_refuse_bad_sizes_and_null_pointers(name, key, bad):
    from wsmgmap import _abi
    lib = _abi.lib()
    args = dict(_ARGS[name])
    assert len(args) == len(_abi._SIG[name])
    args[key] = bad
    assert getattr(lib, name)(*args.values()) == EINVAL


def test_header_parameter_names_are_the_ones_the_refusal_table_uses():
    """The table above is keyed by the header's parameter names, in the header's order: a reordered declaration fails here."""
    import os
    import re
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "wsmgmap.h")).read()
    for name, args in _ARGS.items():
        params = re.search(r"^int %s\(([^()]*)\);" % name, header, re.M).group(1)
        assert [p.split()[-1].lstrip("*") for p in params.split(",")] == list(args), name


# ----------------------------------------------------------------------------- 4. the composed route of the two methods
class _FeatureNet(nn.Module):
    """Stands in for MGMapNet: hands back the features it is given."""

    def forward(self, observations, rnn_hidden_states, prev_actions, masks):
        return observations["features"], rnn_hidden_states, None


def _head_only_policy(K, A, dtype):
    from wsmgmap.common.distributions import DiagGaussian
    from wsmgmap.models.policy import BasePolicy, CriticHead
    pol = BasePolicy.__new__(BasePolicy)
    nn.Module.__init__(pol)
    pol.net, pol.action_distribution, pol.critic, pol.prog_pred, pol.prog = _FeatureNet(), DiagGaussian(K, A), CriticHead(K), nn.Linear(K, 1), None
    return pol.to(dtype)


@pytest.mark.parametrize("shape", [(5, 512, 2), (4, 6, 2), (3, 16, 5)], ids=["B5_K512_A2", "K6", "A5"])
def test_composed_route_of_evaluate_actions_and_get_value_matches_the_oracle(shape):
    """On CPU tensors (and for K % 4 != 0 or A > 4 anywhere) the methods compose DiagGaussian + CriticHead: float64 modules against
    the oracle, shapes as `act()` returns them, nothing registered with AuxLosses, `prog` untouched, the flags of the net reset."""
    from wsmgmap.common.aux_losses import AuxLosses
    B, K, A = shape
    (x, wm, bm, ls, wc, bc, action), grads = pu.eval_inputs(B, K, A)
    pol = _head_only_policy(K, A, torch.float64)
    ad = pol.action_distribution
    with torch.no_grad():
        for p, v in ((ad.fc_mean.weight, wm), (ad.fc_mean.bias, bm), (ad.logstd._bias, ls), (pol.critic.fc.weight, wc), (pol.critic.fc.bias, bc)):
            p.copy_(v.double())
    AuxLosses.deactivate()
    AuxLosses.clear()
    h = torch.zeros(2, B, 8, dtype=torch.float64)
    obs = {"features": x.double()}
    value, logp, entropy, h_out = pol.evaluate_actions(obs, h, None, None, action.double())
    ref = pu.eval_heads_run((x, wm, bm, ls, wc, bc, action), grads, torch.float64)
    assert tuple(value.shape) == (B, 1) and tuple(logp.shape) == (B,) and entropy.dim() == 0 and h_out is h
    close = lambda a, b: torch.allclose(a, b, rtol=1e-12, atol=1e-13)      # noqa: E731
    assert close(value, ref["value"]) and close(logp, ref["logp"]) and close(entropy, ref["entropy"])
    sum((o * g.double()).sum() for o, g in zip((value, logp, entropy), grads)).backward()
    assert close(ad.logstd._bias.grad, ref["dlogstd"]) and close(pol.critic.fc.weight.grad, ref["dwc"])
    assert close(ad.fc_mean.weight.grad, ref["dwm"]) and tuple(ad.logstd._bias.grad.shape) == (A, 1)
    assert close(pol.get_value(obs, h, None, None), ref["value"])
    assert not AuxLosses._entries and pol.prog is None
    assert pol.net.skip_pred_map_nchw is False and pol.net._gt_semantic_map is None and pol.net._cls_tail_allowed is False


def test_operators_refuse_cpu_tensors_and_misfitting_shapes():
    from wsmgmap import _abi, ops
    (x, wm, bm, ls, wc, bc, action), _ = pu.eval_inputs(3, 8, 2)
    fc, cr = nn.Linear(8, 2), nn.Linear(8, 1)
    with pytest.raises(_abi.WsmgError, match="GPU tensors"):
        ops.eval_heads(x, fc, ls, cr, action)
    rows, ent = pu.ppo_inputs(4)
    with pytest.raises(_abi.WsmgError, match="GPU tensors"):
        ops.ppo_loss(rows[0], rows[1], rows[2], rows[3], rows[4], rows[5], ent, 0.2, 0.5, 0.01)
    assert not ops.eval_heads_ok(x, 2) and not ops.eval_heads_ok(x.double(), 2)
