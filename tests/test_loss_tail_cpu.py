"""CPU: the float64 yardstick of the update's loss tail (oracle/tail_ref.py) and the refusals of its entry points.

1. every tail_ref function, in float64, equals the inline reference expressions of the three existing direct tests
   (test_gpu_round3.py: heads / aux / dagger, test_gpu_round2.py: path_kl, test_gpu_kernels.py: cross_entropy_nhwc) at their shapes;
2. for every long-sum case of test_gpu_loss_tail.py the same function evaluated in float32 on the CPU stays inside that case's bar
   against float64: the bar is one the reference arithmetic itself meets (the figures are printed, and recorded beside the bar in
   loss_tail_cases.long_sum_bar);
3. the C ABI refuses what the kernels cannot take with WSMG_EINVAL before anything is queued.
The kernels themselves are tested on the GPU (tests/test_gpu_loss_tail.py)."""
import ctypes

import pytest
import torch
import torch.nn.functional as F

from loss_tail_cases import AUX_L, DAGGER_CASES, DAGGER_IDS, aux_inputs, aux_terms, dagger_inputs, long_sum_bar
from oracle import tail_ref

EINVAL = -1


def _close(a, b):
    return torch.allclose(a, b, rtol=1e-12, atol=1e-14, equal_nan=True)


# ----------------------------------------------------------------------------- 1. the yardstick against the inline references
@pytest.mark.parametrize("shape", [(64, 8, 512, 2), (5, 3, 512, 2), (1, 1, 256, 3), (7, 2, 640, 4)], ids=["bench", "ragged", "b1", "a4"])
def test_heads_aux_and_dagger_yardsticks_equal_the_inline_reference(shape):
    T_, N, K, A = shape
    B = T_ * N
    g = torch.Generator(); g.manual_seed(B * 31 + K)
    rnd = lambda *s: torch.randn(*s, generator=g)      # noqa: E731
    feats = rnd(B, K)
    fc, pp = torch.nn.Linear(K, A), torch.nn.Linear(K, 1)
    progress, wp = torch.rand(B, 1, generator=g), rnd(B, A + 1)
    weights = torch.rand(T_, N, generator=g) + 0.1
    if T_ > 2:
        weights[T_ - 2:, 0] = 0.0
    ce, kl = torch.rand(B, generator=g), torch.rand(B, generator=g)
    mask = (weights > 0).view(-1)
    if (~mask).any():
        kl = kl.masked_fill(~mask, float("nan"))
    alphas = (0.1, 0.5, 1.0)
    # the inline reference of test_update_heads_aux_reduce_and_dagger_loss_match_the_reference_lines
    xd = feats.double()
    pred = F.linear(xd, fc.weight.double(), fc.bias.double())
    prog = torch.tanh(F.linear(xd, pp.weight.double(), pp.bias.double()))
    prows = F.mse_loss(prog, progress.double(), reduction="none").mean(-1)
    aux = sum(a * torch.masked_select(l.double(), mask).mean() for a, l in zip(alphas, (ce, kl, prows)))
    logits = torch.tanh(pred).view(T_, N, -1)
    al = F.mse_loss(logits, wp[:, :A].double().view(T_, N, -1), reduction="none").sum(dim=2)
    action = ((weights.double() * al).sum(0) / weights.double().sum(0)).mean()
    loss = action + aux
    # the yardstick
    pred_y, prog_y, prows_y = tail_ref.update_heads(feats, fc.weight, fc.bias, pp.weight, pp.bias, progress)
    aux_y = tail_ref.aux_reduce([ce, kl, prows_y], alphas, mask)
    loss_y, action_y = tail_ref.dagger_loss(pred_y, aux_y, wp, weights)
    for name, a_, b_ in (("pred", pred_y, pred), ("prog", prog_y, prog), ("prog_rows", prows_y, prows), ("aux", aux_y, aux),
                         ("action", action_y, action), ("loss", loss_y, loss)):
        assert a_.dtype == torch.float64 and a_.shape == b_.shape and torch.isfinite(a_).all(), name
        assert _close(a_, b_), name
    assert tail_ref.update_heads(feats, fc.weight, fc.bias, pp.weight, pp.bias, None)[2] is None
    assert _close(tail_ref.dagger_loss(pred_y, None, wp, weights)[0], action)


@pytest.mark.parametrize("geom", [(8, 100, 24), (3, 196, 49), (5, 57, 10)], ids=["E100", "E196", "odd"])
def test_path_kl_yardstick_equals_the_inline_reference(geom):
    B, E, S = geom
    torch.manual_seed(E)
    dis = (torch.rand(B, E, E) * 50).contiguous()
    dis[0, :5] = 0.0
    att = torch.softmax(torch.randn(B, S * S) * 2, dim=1)
    # the inline reference of test_path_kl_matches_torch_formula
    d = dis.double()
    lo, hi = d.min(), d.max()
    tg = F.interpolate(((hi - d) / (hi - lo)).unsqueeze(1), size=[S, S], mode="area").squeeze(1)
    tg = F.softmax(tg.reshape(B, -1) / 0.07, dim=1)
    ref = F.kl_div(torch.log(att.double()), tg, reduction="none").mean(-1)
    got = tail_ref.path_kl(dis, att, S, 0.07)
    assert got.dtype == torch.float64 and _close(got, ref) and _close(tail_ref.path_kl_target(dis, S, 0.07), tg)


def test_ce_nhwc_yardstick_equals_the_inline_reference_and_poisons_out_of_range_rows():
    torch.manual_seed(2)
    B, S, C = 3, 10, 27
    logits = torch.randn(B, S, S, 32) * 3
    logits[..., C:] = 0
    target = torch.randint(0, C, (B, S, S))
    # the inline reference of test_cross_entropy_nhwc
    ref = F.cross_entropy(logits.double()[..., :C].permute(0, 3, 1, 2), target, reduction="none")
    got = tail_ref.ce_nhwc(logits, target, C)
    assert got.dtype == torch.float64 and got.shape == ref.shape and _close(got, ref)
    # labels outside [0, classes): NaN rows, -100 among them; every other row as before
    bad = target.clone()
    where = [(0, 0, 0), (0, 3, 4), (1, 9, 9), (2, 0, 5), (2, 5, 5), (2, 9, 0)]
    for pos, lab in zip(where, (-1, -100, C, 31, 32, 2 ** 40)):
        bad[pos] = lab
    x = logits.clone().requires_grad_(True)
    got = tail_ref.ce_nhwc(x, bad, C)
    hit = torch.zeros_like(target, dtype=torch.bool)
    for pos in where:
        hit[pos] = True
    assert torch.equal(torch.isnan(got), hit) and _close(got[~hit], ref[~hit])
    got[~hit].sum().backward()
    assert torch.isfinite(x.grad).all() and float(x.grad[hit].abs().max()) == 0.0 and float(x.grad[..., C:].abs().max()) == 0.0


# ----------------------------------------------------------------------------- 2. the long-sum bars against the reference in float32
def _rel(a, b, floor):
    return float((a.double() - b).abs().max()) / max(float(b.abs().max()), floor)


@pytest.mark.parametrize("case", DAGGER_CASES, ids=DAGGER_IDS)
def test_dagger_bar_is_met_by_the_reference_in_float32(case):
    T_, N, A, ld = case
    pred, wp, weights = dagger_inputs(*case)
    out = {}
    for dt in (torch.float64, torch.float32):
        p = pred.clone().requires_grad_(True)
        loss, action = tail_ref.dagger_loss(p, torch.tensor(0.25), wp, weights, dtype=dt)
        loss.backward()
        assert loss.dtype == dt
        out[dt] = (loss.detach(), action.detach(), p.grad)
    bar = long_sum_bar(T_)
    e_loss = _rel(out[torch.float32][0], out[torch.float64][0], 1.0)
    e_act = _rel(out[torch.float32][1], out[torch.float64][1], 1.0)
    e_grad = _rel(out[torch.float32][2], out[torch.float64][2].double(), 0.0)
    print(f"dagger {case}: bar {bar:.2e}, float32 reference: loss {e_loss:.2e}, action {e_act:.2e}, d pred {e_grad:.2e}")
    assert torch.isfinite(out[torch.float64][0]) and torch.isfinite(out[torch.float64][2]).all()
    assert e_loss <= bar and e_act <= bar and e_grad <= bar


@pytest.mark.parametrize("L", AUX_L)
def test_aux_reduce_bar_is_met_by_the_reference_in_float32(L):
    B = 4099
    rows, alphas, mask = aux_inputs(B, L)
    out = {}
    for dt in (torch.float64, torch.float32):
        rs = [r.clone().requires_grad_(True) for r in rows]
        v = tail_ref.aux_reduce(rs, alphas, mask, dtype=dt)
        v.backward()
        out[dt] = (v.detach(), torch.stack([r.grad for r in rs]))
    bar = long_sum_bar(aux_terms(B))
    e_val = _rel(out[torch.float32][0], out[torch.float64][0], 1.0)
    e_grad = _rel(out[torch.float32][1], out[torch.float64][1].double(), 0.0)
    print(f"aux_reduce B={B} L={L}: bar {bar:.2e}, float32 reference: value {e_val:.2e}, d rows {e_grad:.2e}")
    assert torch.isfinite(out[torch.float64][0]) and torch.isfinite(out[torch.float64][1]).all()
    assert e_val <= bar and e_grad <= bar


# ----------------------------------------------------------------------------- 3. refusals through the C ABI
_BUF = (ctypes.c_uint64 * 64)()
_P = ctypes.cast(_BUF, ctypes.c_void_p)      # host memory that is never dereferenced: every case must be refused before a launch


def _dagger(**over):
    a = dict(pred=_P, waypoint=_P, ld_waypoint=3, weights=_P, aux=None, T=4, N=2, A=2, out2=_P, den=_P, stream=None)
    a.update(over)
    return "wsmg_dagger_loss_fwd", a


def _aux(**over):
    a = dict(rows=_P, alpha=_P, L=3, mask=_P, B=8, out2=_P, stream=None)
    a.update(over)
    return "wsmg_aux_reduce_fwd", a


def _heads(**over):
    a = dict(x=_P, wm=_P, bm=_P, wp=_P, bp=_P, progress=_P, B=4, K=512, A=2, pred=_P, prog=_P, prog_rows=_P, stream=None)
    a.update(over)
    return "wsmg_update_heads_fwd", a


def _kl(**over):
    a = dict(dis=_P, lo=_P, hi=_P, att=_P, B=2, H=12, W=16, S=4, tau=0.07, target=_P, kl=_P, stream=None)
    a.update(over)
    return "wsmg_path_kl_fwd", a


@pytest.mark.parametrize("entry", [_dagger(N=257), _dagger(ld_waypoint=1), _aux(L=5), _heads(A=5), _heads(K=510), _kl(S=13), _kl(S=14, H=16, W=13),
                                   _kl(tau=0.0)],
                         ids=["dagger_N=257", "dagger_ld_waypoint<A", "aux_L=5", "heads_A=5", "heads_K=510", "path_kl_S>H", "path_kl_S>W",
                              "path_kl_tau=0"])
def test_loss_tail_entry_points_refuse_invalid_arguments(entry):
    from wsmgmap import _abi
    try:
        lib = _abi.lib()
    except _abi.WsmgError as e:          # the library needs a GPU runtime this machine cannot load
        pytest.skip(str(e)[:120])
    name, args = entry
    assert len(args) == len(_abi._SIG[name])
    assert getattr(lib, name)(*args.values()) == EINVAL
