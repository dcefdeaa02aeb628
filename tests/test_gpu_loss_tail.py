"""GPU: the chain of small float32 kernels that ends every update in the scalar loss — update_heads, aux_reduce, dagger_loss
(csrc/wsmg_heads.hip), path_kl (csrc/wsmg_loss.hip), ce_nhwc (csrc/wsmg_loss.hip) — beyond the bench shape and on bad batches:
the second chunk of the DAgger loss, the optional-gradient branches and the ragged last workgroup of the heads' backward, empty
and single-row selections of the auxiliary reduction, non-square and degenerate geometries of the contrastive monitor's KL,
extreme logits and out-of-range labels of the unfused cross-entropy.

Everything goes through wsmgmap.ops and is compared with oracle/tail_ref.py evaluated in float64 on the host on the same
float32 (or bf16-valued) inputs.  The bars are the existing direct tests' (2e-6 heads / aux / dagger, 2e-5 path_kl, the
cross-entropy's 2e-6 * (1 + |ref|), 2e-6 / 1e-2 of max |grad|) except where a sum gets longer: loss_tail_cases.long_sum_bar,
which test_loss_tail_cpu.py shows the reference's own float32 evaluation to meet.  NaN masks are compared with torch.equal;
nothing that is compared goes through nan_to_num."""
import pytest
import torch

from loss_tail_cases import AUX_B, AUX_L, DAGGER_CASES, DAGGER_DEAD, DAGGER_IDS, aux_inputs, aux_terms, dagger_inputs, long_sum_bar
from oracle import tail_ref

pytestmark = pytest.mark.gpu


def _err(got, ref):
    return float((got.detach().double().cpu() - ref.detach()).abs().max())


# ----------------------------------------------------------------------------- dagger_loss
def _dagger_fused(pred, wp, weights, aux_value=0.25):
    from wsmgmap import ops
    p = pred.cuda().requires_grad_(True)
    aux = torch.tensor(aux_value, device="cuda", requires_grad=True)
    loss, action = ops.dagger_loss(p, aux, wp.cuda(), weights.cuda())
    loss.backward()
    torch.cuda.synchronize()
    return loss.detach().cpu(), action.detach().cpu(), p.grad.cpu(), aux.grad.cpu()


def _dagger_ref(pred, wp, weights, aux_value=0.25):
    p = pred.clone().requires_grad_(True)
    loss, action = tail_ref.dagger_loss(p, torch.tensor(aux_value), wp, weights)
    loss.backward()
    return loss.detach(), action.detach(), p.grad


@pytest.mark.parametrize("case", DAGGER_CASES, ids=DAGGER_IDS)
def test_dagger_loss_beyond_one_chunk(case):
    """Value, action loss and d pred over more than DL_CHUNK = 2048 rows (and at exactly 2048), N at its limit of 256, one
    episode; the same bits in two runs."""
    T_, N, A, ld = case
    pred, wp, weights = dagger_inputs(*case)
    loss, action, dpred, daux = _dagger_fused(pred, wp, weights)
    loss2, action2, dpred2, _ = _dagger_fused(pred, wp, weights)
    rl, ra, rg = _dagger_ref(pred, wp, weights)
    bar = long_sum_bar(T_)
    e_l, e_a, e_g = _err(loss, rl), _err(action, ra), _err(dpred, rg)
    print(f"dagger {case}: bar {bar:.2e}  loss {e_l / max(1.0, abs(float(rl))):.2e}  action {e_a / max(1.0, abs(float(ra))):.2e}  "
          f"d pred {e_g / float(rg.abs().max()):.2e}")
    assert torch.isfinite(loss) and torch.isfinite(action) and torch.isfinite(dpred).all()
    assert e_l <= bar * max(1.0, abs(float(rl))) and e_a <= bar * max(1.0, abs(float(ra)))
    assert e_g <= bar * float(rg.abs().max())
    assert float(daux) == 1.0
    assert float(dpred.view(T_, N, A)[T_ - 2:, 0].abs().max()) == 0.0, "a step of weight 0 received a gradient"
    assert torch.equal(loss, loss2) and torch.equal(action, action2) and torch.equal(dpred, dpred2), "dagger_loss is not repeatable"


def test_dagger_loss_of_an_episode_without_weight_is_nan_where_the_reference_is():
    """An episode whose weights are all zero is 0 / 0 in the reference: loss and action loss NaN, d pred NaN on exactly that
    episode's rows and within the bar everywhere else."""
    T_, N, A, ld, dead = DAGGER_DEAD
    pred, wp, weights = dagger_inputs(T_, N, A, ld, dead=dead)
    loss, action, dpred, _ = _dagger_fused(pred, wp, weights)
    rl, ra, rg = _dagger_ref(pred, wp, weights)
    assert torch.isnan(rl) and torch.isnan(ra) and torch.isnan(loss) and torch.isnan(action)
    want = torch.zeros(T_, N, A, dtype=torch.bool)
    want[:, dead] = True
    assert torch.equal(torch.isnan(rg).view(T_, N, A), want)
    assert torch.equal(torch.isnan(dpred).view(T_, N, A), want)
    ok = ~want.view(T_ * N, A)
    bar = long_sum_bar(T_)
    assert torch.isfinite(dpred[ok]).all()
    assert _err(dpred[ok], rg[ok]) <= bar * float(rg[ok].abs().max())


# ----------------------------------------------------------------------------- update_heads
def _heads_inputs(B, K, A):
    g = torch.Generator(); g.manual_seed(B * 31 + K + A)
    x = torch.randn(B, K, generator=g)
    fc, pp = torch.nn.Linear(K, A), torch.nn.Linear(K, 1)
    with torch.no_grad():
        for p in (fc.weight, fc.bias, pp.weight, pp.bias):
            p.copy_((torch.rand(p.shape, generator=g) * 2 - 1) / K ** 0.5)
    progress = torch.rand(B, 1, generator=g)
    # upstream gradients of pred, prog and the progress rows.  One sign each, and the sign of d prog that of the rows' term
    # (prog - progress is negative on most rows): the bias gradients are sums over the B rows, and a sum that cancels to a
    # fraction of its terms cannot be held to 2e-6 of its own size in float32 by anything, the reference's lines included.
    gs = (torch.rand(B, A, generator=g) + 0.5, -(torch.rand(B, 1, generator=g) + 0.5), torch.rand(B, generator=g) + 0.5)
    return x, fc, pp, progress, gs


_FORMS = {   # which outputs the loss uses: (pred, prog directly, progress rows)
    "pred_only": (True, False, False), "prog_only": (False, True, False), "rows_only": (False, False, True), "all_three": (True, True, True)}


def _heads_loss(form, outs, gs):
    return sum((o * g.to(o)).sum() for use, o, g in zip(_FORMS[form], outs, gs) if use)


@pytest.mark.parametrize("form", list(_FORMS))
@pytest.mark.parametrize("shape", [(3, 260, 1), (5, 516, 4), (33, 256, 2)], ids=["B3_K260_A1", "B5_K516_A4", "B33_K256_A2"])
def test_update_heads_optional_gradients_and_ragged_workgroups(shape, form):
    """update_heads_bwd_kernel with a gradient missing (`set_materialize_grads(False)`: only pred used -> d prog and d rows are
    null; prog used directly -> the d prog branch; only the progress rows), all of them together, K % 8 != 0 (the last
    workgroup's 8 feature columns are half dead) and B % 4 != 0 (a forward workgroup with idle waves).  All five parameter
    gradients and d x; what the reference leaves at exactly zero is exactly zero."""
    import copy
    from wsmgmap import ops
    B, K, A = shape
    x, fc, pp, progress, gs = _heads_inputs(B, K, A)
    # fused
    xg = x.cuda().requires_grad_(True)
    fcg, ppg = copy.deepcopy(fc).cuda(), copy.deepcopy(pp).cuda()
    outs = ops.update_heads(xg, fcg, ppg, progress.cuda())
    _heads_loss(form, outs, [g.cuda() for g in gs]).backward()
    torch.cuda.synchronize()
    got_g = [xg.grad, fcg.weight.grad, fcg.bias.grad, ppg.weight.grad, ppg.bias.grad]
    # reference
    leaves = [t.detach().clone().requires_grad_(True) for t in (x, fc.weight, fc.bias, pp.weight, pp.bias)]
    refs = tail_ref.update_heads(*leaves, progress)
    _heads_loss(form, refs, gs).backward()
    for name, o, r in zip(("pred", "prog", "prog_rows"), outs, refs):
        assert o.shape == r.shape and torch.isfinite(o).all(), name
        assert _err(o, r) <= 2e-6 * max(1.0, float(r.detach().abs().max())), (name, _err(o, r))
    for name, got, leaf in zip(("dx", "dWm", "dbm", "dWp", "dbp"), got_g, leaves):
        assert got is not None and got.shape == leaf.shape and torch.isfinite(got).all(), name
        ref = leaf.grad if leaf.grad is not None else torch.zeros_like(leaf)
        if float(ref.abs().max()) == 0.0:
            assert float(got.abs().max()) == 0.0, f"{name}: the reference leaves it at exactly zero"
        else:
            assert _err(got, ref) <= 2e-6 * max(float(ref.abs().max()), 1e-3), (name, _err(got, ref))


def test_update_heads_without_progress_returns_no_rows():
    from wsmgmap import ops
    B, K, A = 5, 516, 4
    x, fc, pp, _, gs = _heads_inputs(B, K, A)
    xg = x.cuda().requires_grad_(True)
    pred, prog, rows = ops.update_heads(xg, fc.cuda(), pp.cuda(), None)
    assert rows is None
    ((pred * gs[0].cuda()).sum() + (prog * gs[1].cuda()).sum()).backward()
    leaves = [t.detach().cpu().clone().requires_grad_(True) for t in (x, fc.weight, fc.bias, pp.weight, pp.bias)]
    rp, rg, rr = tail_ref.update_heads(*leaves, None)
    assert rr is None
    ((rp * gs[0]).sum() + (rg * gs[1]).sum()).backward()
    assert _err(pred, rp) <= 2e-6 * max(1.0, float(rp.detach().abs().max())) and _err(prog, rg) <= 2e-6
    for name, got, leaf in zip(("dx", "dWm", "dbm", "dWp", "dbp"), (xg.grad, fc.weight.grad, fc.bias.grad, pp.weight.grad, pp.bias.grad), leaves):
        assert _err(got, leaf.grad) <= 2e-6 * max(float(leaf.grad.abs().max()), 1e-3), name


def test_update_heads_is_repeatable_to_the_bit():
    """B % 32 != 0 (row groups of unequal length), K % 8 != 0 (a half-dead last column workgroup) and the widest A through the
    column-owned backward, all three outputs used: two runs give the same bits in every output and every gradient."""
    import copy
    from wsmgmap import ops
    B, K, A = 33, 516, 4
    x, fc, pp, progress, gs = _heads_inputs(B, K, A)

    def run():
        xg = x.cuda().requires_grad_(True)
        fcg, ppg = copy.deepcopy(fc).cuda(), copy.deepcopy(pp).cuda()
        outs = ops.update_heads(xg, fcg, ppg, progress.cuda())
        _heads_loss("all_three", outs, [g.cuda() for g in gs]).backward()
        torch.cuda.synchronize()
        named = dict(zip(("pred", "prog", "prog_rows"), (o.detach() for o in outs)))
        named.update(dx=xg.grad, dWm=fcg.weight.grad, dbm=fcg.bias.grad, dWp=ppg.weight.grad, dbp=ppg.bias.grad)
        return named

    a, b = run(), run()
    assert len(a) == 8
    for k in a:
        assert a[k] is not None and torch.isfinite(a[k]).all(), k
        assert torch.equal(a[k], b[k]), k


# ----------------------------------------------------------------------------- aux_reduce
def _aux_both(rows, alphas, mask):
    from wsmgmap import ops
    rg = [r.cuda().requires_grad_(True) for r in rows]
    v = ops.aux_reduce(rg, alphas, mask.cuda())
    v.backward()
    torch.cuda.synchronize()
    rr = [r.clone().requires_grad_(True) for r in rows]
    w = tail_ref.aux_reduce(rr, alphas, mask)
    w.backward()
    return v.detach().cpu(), torch.stack([r.grad.cpu() for r in rg]), w.detach(), torch.stack([r.grad for r in rr])


@pytest.mark.parametrize("L", AUX_L)
@pytest.mark.parametrize("B", AUX_B)
def test_aux_reduce_sizes_and_selections(B, L):
    """One row, one short of / one past a pass of the 256 threads, 17 passes; one and four loss vectors; a random selection, a
    single selected row and an empty one (NaN, with all-zero gradients, as `masked_select(...).mean()`); NaN planted in the
    unselected rows stays out of the value and of the gradients."""
    bar = long_sum_bar(aux_terms(B))
    for kind in ("random", "one"):
        rows, alphas, mask = aux_inputs(B, L, kind)
        v, g, rv, rg = _aux_both(rows, alphas, mask)
        assert torch.isfinite(rv) and torch.isfinite(rg).all()
        assert torch.isfinite(v) and torch.isfinite(g).all(), kind
        assert _err(v, rv) <= bar * max(1.0, abs(float(rv))), (kind, _err(v, rv))
        assert _err(g, rg) <= bar * float(rg.abs().max()), (kind, _err(g, rg))
        assert float(g[:, ~mask].abs().sum()) == 0.0, kind
    rows, alphas, mask = aux_inputs(B, L, "empty")
    v, g, rv, rg = _aux_both(rows, alphas, mask)
    assert torch.isnan(rv) and float(rg.abs().max()) == 0.0
    assert torch.isnan(v) and float(g.abs().max()) == 0.0


# ----------------------------------------------------------------------------- cross_entropy_nhwc
_CE_SHAPES = {"rows257": (1, 257, 1), "rows3x10x10": (3, 10, 10)}


def _ce_both(logits, target, classes, gl):
    """logits: float32 or bf16 CPU tensor [..., 32] -> (loss, d logits) of the kernel and of the yardstick on the same values."""
    from wsmgmap import ops
    x = logits.cuda().requires_grad_(True)
    loss = ops.cross_entropy_nhwc(x, target.cuda(), classes)
    (loss * gl.cuda()).sum().backward()
    torch.cuda.synchronize()
    xr = logits.double().requires_grad_(True)
    ref = tail_ref.ce_nhwc(xr, target, classes)
    ok = ~torch.isnan(ref)
    (ref[ok] * gl.double()[ok]).sum().backward()
    return loss.detach().cpu(), x.grad.float().cpu(), ref.detach(), xr.grad


@pytest.mark.parametrize("dt", ["f32", "bf16"])
@pytest.mark.parametrize("shape", list(_CE_SHAPES))
@pytest.mark.parametrize("classes", [1, 27, 32])
def test_cross_entropy_nhwc_extreme_logits(classes, shape, dt):
    """Logits drawn from +-1e4 with one constant row: only the maximum subtraction keeps expf from overflowing.  One class, the
    reference's 27, and 32 (no padded channel); a second workgroup with a ragged tail (257 rows)."""
    dims = _CE_SHAPES[shape]
    g = torch.Generator(); g.manual_seed(classes * 1000 + dims[1])
    logits = (torch.rand(*dims, 32, generator=g) * 2 - 1) * 1e4
    logits[0, 1] = 3700.0
    logits[..., classes:] = 0
    if dt == "bf16":
        logits = logits.bfloat16()
    target = torch.randint(0, classes, dims, generator=g)
    gl = torch.randn(*dims, generator=g)
    loss, grad, ref, rgrad = _ce_both(logits, target, classes, gl)
    assert torch.isfinite(ref).all() and torch.isfinite(loss).all() and torch.isfinite(grad).all()
    e_l, e_g = _err(loss, ref), _err(grad, rgrad)
    print(f"ce extreme classes={classes} {shape} {dt}: loss err {e_l:.3e} (|ref| max {float(ref.abs().max()):.3e}), grad err {e_g:.3e}")
    assert e_l <= 2e-6 * (1 + float(ref.abs().max()))
    tol = 2e-6 if dt == "f32" else 1e-2
    if classes > 1:
        assert e_g <= tol * float(rgrad.abs().max())
    else:
        assert float(rgrad.abs().max()) == 0.0 and float(grad.abs().max()) == 0.0      # softmax of one class - onehot = 0
    if classes < 32:
        assert float(grad[..., classes:].abs().max()) == 0.0


@pytest.mark.parametrize("dt", ["f32", "bf16"])
@pytest.mark.parametrize("shape", list(_CE_SHAPES))
@pytest.mark.parametrize("classes", [1, 27, 32])
def test_cross_entropy_nhwc_poisons_the_row_of_an_out_of_range_label(classes, shape, dt):
    """The contract shared with cls_tail: a label outside [0, classes) — negative, -100 (no ignore_index), `classes`, a padded
    channel's index, 32, or 2^40 (whose low 32 bits are 0, a valid label) — makes that row's loss NaN and its whole 32-wide
    gradient row NaN; every other row is as without it, padded channels at exactly 0.

    Before the guard in ce_nhwc_fwd/bwd_kernel these rows came out finite: the bare log-sum-exp for a label that matches no
    channel, log-sum-exp minus a padded channel's logit for classes <= label < 32, and class 0's loss for 2^40."""
    dims = _CE_SHAPES[shape]
    g = torch.Generator(); g.manual_seed(classes * 1000 + dims[1] + 1)
    logits = torch.randn(*dims, 32, generator=g) * 3
    logits[..., classes:] = 0
    if dt == "bf16":
        logits = logits.bfloat16()
    target = torch.randint(0, classes, dims, generator=g)
    labels = [-1, -100, classes] + ([31] if classes < 32 else []) + [32, 2 ** 40]
    n = target.numel()
    at = [0, 7, 99, n // 2, n - 2, n - 1][:len(labels)]        # first and last rows included; 256 (the second workgroup) is n - 1 of 257
    flat = target.view(-1)
    hit = torch.zeros(n, dtype=torch.bool)
    for i, lab in zip(at, labels):
        flat[i] = lab
        hit[i] = True
    hit = hit.view(dims)
    gl = torch.randn(*dims, generator=g)
    loss, grad, ref, rgrad = _ce_both(logits, target, classes, gl)
    assert torch.equal(torch.isnan(ref), hit)
    print(f"ce labels classes={classes} {shape} {dt}: loss rows of the out-of-range labels {labels}: {loss[hit].tolist()}")
    assert torch.equal(torch.isnan(loss), hit), f"out-of-range labels {labels} gave loss rows {loss[hit].tolist()}"
    assert torch.equal(torch.isnan(grad), hit.unsqueeze(-1).expand(*dims, 32)), "d logits: NaN on exactly the whole rows of the out-of-range labels"
    ok = ~hit
    assert _err(loss[ok], ref[ok]) <= 2e-6 * (1 + float(ref[ok].abs().max()))
    tol = 2e-6 if dt == "f32" else 1e-2
    if classes > 1:
        assert _err(grad[ok], rgrad[ok]) <= tol * float(rgrad[ok].abs().max())
    else:
        assert float(grad[ok].abs().max()) == 0.0
    if classes < 32:
        assert float(grad[ok][:, classes:].abs().max()) == 0.0


# ----------------------------------------------------------------------------- path_kl
def _kl_both(dis, att, S, tau, g):
    from wsmgmap import ops
    a = att.cuda().requires_grad_(True)
    kl = ops.path_kl(dis.cuda(), a, S, tau)
    kl.backward(g.cuda())
    torch.cuda.synchronize()
    ar = att.clone().requires_grad_(True)
    ref = tail_ref.path_kl(dis, ar, S, tau)
    ref.backward(g.double())
    return kl.detach().cpu(), a.grad.cpu(), ref.detach(), ar.grad


def _att(B, n, g):
    if n == 1:
        return torch.rand(B, 1, generator=g) * 0.8 + 0.1      # (a one-bin row: softmax would make it exactly 1 and the loss 0)
    return torch.softmax(torch.randn(B, n, generator=g) * 2, dim=1)


@pytest.mark.parametrize("geom", [(3, 40, 24, 8), (2, 24, 40, 8), (2, 12, 12, 12), (4, 9, 7, 1), (1, 57, 31, 10)],
                         ids=["H40_W24", "H24_W40", "one_pixel_bins", "one_bin", "uneven_bins_both_axes"])
def test_path_kl_on_non_square_and_degenerate_geometries(geom):
    """H != W in both orientations (a transposed H / W in the bin arithmetic passes every square case), one-pixel bins (S = H),
    a single bin (n = 1: 255 threads idle in all three reductions), bins that divide neither axis evenly."""
    B, H, W, S = geom
    g = torch.Generator(); g.manual_seed(H * 100 + W)
    dis = torch.rand(B, H, W, generator=g) * 50
    dis[0, :2] = 0.0
    att = _att(B, S * S, g)
    kl, datt, ref, rgrad = _kl_both(dis, att, S, 0.07, torch.rand(B, generator=g))
    assert torch.isfinite(ref).all() and torch.isfinite(kl).all() and torch.isfinite(datt).all()
    assert _err(kl, ref) <= 2e-5 * max(1.0, float(ref.abs().max())), _err(kl, ref)
    assert _err(datt, rgrad) <= 2e-5 * float(rgrad.abs().max()), _err(datt, rgrad)


def test_path_kl_with_target_bins_that_underflow_to_zero():
    """tau = 0.004 on a map that spans its range from one edge to the other: exp((a_j - a_max) / tau) underflows to exactly 0 in
    float32 for the far bins, and `t * log(t)` is taken as 0 there (xlogy), not as 0 * -inf.  kl and d att finite and within
    the bar; d att exactly 0 where the target is 0."""
    B, H, W, S, tau = 3, 40, 24, 8, 0.004
    g = torch.Generator(); g.manual_seed(4)
    ramp = torch.linspace(0.0, 1.0, H).view(1, H, 1) * 0.5 + torch.linspace(0.0, 1.0, W).view(1, 1, W) * 0.5
    dis = (ramp * 50 + torch.rand(B, H, W, generator=g) * 0.2).contiguous()
    att = _att(B, S * S, g)
    tg32 = tail_ref.path_kl_target(dis, S, tau, dtype=torch.float32)
    zero = tg32 == 0
    assert zero.any() and not zero.all(1).any(), "the float32 target must contain exact zeros"
    # no bin sits at the edge of the underflow (exp(-103.97) is the smallest float32 denormal): which bins are zero does not
    # depend on the last bits of the exponent
    z = torch.log(tail_ref.path_kl_target(dis, S, tau))
    gap = z.max(1, keepdim=True).values - z
    assert not ((gap > 100) & (gap < 108)).any() and torch.equal(gap > 104, zero)
    kl, datt, ref, rgrad = _kl_both(dis, att, S, tau, torch.rand(B, generator=g) + 0.5)
    assert torch.isfinite(kl).all() and torch.isfinite(datt).all()
    assert _err(kl, ref) <= 2e-5 * max(1.0, float(ref.abs().max())), _err(kl, ref)
    assert _err(datt, rgrad) <= 2e-5 * float(rgrad.abs().max()), _err(datt, rgrad)
    assert float(datt[zero].abs().max()) == 0.0


def test_path_kl_of_a_constant_map_is_nan_on_every_row():
    """hi == lo: the reference's normalisation is 0 / 0 and every row of its kl is NaN — not a finite number."""
    B, H, W, S = 3, 12, 16, 4
    g = torch.Generator(); g.manual_seed(5)
    dis = torch.full((B, H, W), 7.5)
    kl, _, ref, _ = _kl_both(dis, _att(B, S * S, g), S, 0.07, torch.ones(B))
    assert torch.isnan(ref).all() and torch.isnan(kl).all()
