"""CPU: the cases, references and bars of tests/norm_cases.py are what tests/test_gpu_norm_edges.py needs them to be.

1. the written-out float64 BatchNorm (+ residual)(+ ReLU) — forward, running statistics, dx, dgamma, dbeta, dres — is F.batch_norm +
   autograd in float64 to 1e-12 on every case with fewer than 100 000 rows, and the written-out GroupNorm is F.group_norm;
2. every case has the block count its name promises, by arithmetic written here (not norm_cases.nblk_of), and the tables hold every
   edge the kernels have: both loops of reduce_partials, the block cap from both sides, more than two trips per thread;
3. at most 1 % of a ReLU case's dy is zeroed because its pre-activation sits near 0, and the inputs are well conditioned;
4. the kernels' formulas in plain float32 on the CPU stay inside every bar;
5. the GroupNorm bar's float32 part stays inside the stage test's allowance, and the group sizes are the ones the table is there for."""
import math

import pytest
import torch
import torch.nn.functional as F

import norm_cases as nc

DT_IDS = ["f32", "bf16"]
MODES = [(False, False), (False, True), (True, False), (True, True)]        # (residual, relu)


def all_bn_cases():
    """(C, rows, bf16, res, relu, seed) of every train-mode case the GPU file builds."""
    out = []
    for bf16 in (False, True):
        for C, e in nc.EDGE_CASES:
            out.append((C, nc.edge_rows(C)[e][0], bf16, True, True, ""))
        for C in nc.CHANNELS:
            B, H, W = nc.MODE_SHAPES[C]
            out += [(C, B * H * W, bf16, res, relu, "") for res, relu in MODES]
        B, H, W = nc.STRIDED_SHAPE
        for C in sorted({s[0] for s in nc.STRIDED}):
            out += [(C, B * H * W, bf16, True, True, ""), (C, B * H * W, bf16, False, True, "")]
    out.append((256, nc.edge_rows(256)["nblk65"][0], True, False, True, ""))         # section d's case without a residual
    return sorted(set(out))


def test_every_case_has_the_block_count_of_its_name():
    for C in nc.CHANNELS:
        rpi = 1024 // C
        for name, (rows, want) in nc.edge_rows(C).items():
            nblk = min(1024, math.ceil(rows / (8 * rpi)))
            assert nblk == want == nc.nblk_of(rows, C), (C, name, rows, nblk, want)
            B, H, W = nc.shape_of(rows)
            assert B * H * W == rows
    r = {e: nc.edge_rows(256)[e][0] for e in nc.SMALL}
    assert [r[e] for e in nc.SMALL] == [2, 3, 4, 5, 31, 33]
    # reduce_partials enters its unrolled loop when b + 3 * 64 < nblk for lane 0: from 193 partials up
    assert all(nc.edge_rows(256)[e][1] <= 192 for e in nc.TAIL_ONLY) and all(nc.edge_rows(256)[e][1] >= 193 for e in nc.UNROLLED)
    for C in (32, 256, 512):
        rpi, rows = 1024 // C, nc.edge_rows(C)["beyond"][0]
        assert nc.edge_rows(C)["cap"][0] == 8192 * rpi == 1024 * 8 * rpi and nc.edge_rows(C)["cap+1"][0] == 8192 * rpi + 1
        trips, tail = divmod(rows, 1024 * rpi * 4)              # whole four-row trips of every thread, rows left for the tail loop
        assert trips >= 4 and 0 < tail < 1024 * rpi * 4 and tail % rpi, (C, rows, trips, tail)
    assert max(C * nc.edge_rows(C)["beyond"][0] for C, _ in nc.EDGE_CASES) <= 16.8e6
    for C, (B, H, W) in nc.MODE_SHAPES.items():
        assert (B * H * W) % (8 * (1024 // C)) and len({B, H, W}) == 3 and nc.nblk_of(B * H * W, C) >= 3
    for C, Ctot, c0 in nc.STRIDED + [nc.MISALIGNED]:
        assert c0 + C <= Ctot and (Ctot - C) % 8 == 0 and Ctot % 8 == 0
    assert all(c0 % 8 == 0 for _, _, c0 in nc.STRIDED) and any(c0 for _, _, c0 in nc.STRIDED) and nc.MISALIGNED[2] % 8 == 4


def _rel(name, got, want, scale=None):
    s = max(float(want.abs().max()), scale or 0.0)
    err = float((got - want).abs().max())
    assert err <= 1e-12 * s, f"{name}: {err:.3e} against {s:.3e}"


@pytest.mark.parametrize("bf16", [False, True], ids=DT_IDS)
def test_written_out_batchnorm_is_torch_float64(bf16):
    n = 0
    for C, rows, b, res, relu, seed in all_bn_cases():
        if b != bf16 or rows >= 100_000:
            continue
        c = nc.bn_case(C, rows, b, res, relu, seed)
        x, g, bt = (c[k].double().requires_grad_(True) for k in ("x", "gamma", "beta"))
        r = c["res"].double().requires_grad_(True) if res else None
        rm, rv = c["rm"].double().clone(), c["rv"].double().clone()
        y = F.batch_norm(x, rm, rv, g, bt, training=True, momentum=nc.MOMENTUM, eps=nc.EPS)
        y = y + r if res else y
        y = F.relu(y) if relu else y
        y.backward(c["dy"].double())
        tag = f"C{C}.rows{rows}.{res}.{relu}"
        _rel(tag + ".y", c["fwd"]["y"], y.detach())
        _rel(tag + ".running_mean", c["fwd"]["running_mean"], rm)
        _rel(tag + ".running_var", c["fwd"]["running_var"], rv)
        # dx cancels to ~0 at two rows: its scale is that of its terms, gamma invstd |dy|
        _rel(tag + ".dx", c["bwd"]["dx"], x.grad, scale=float((c["gamma"].double() * c["fwd"]["invstd"]).max() * c["dy"].abs().max()))
        _rel(tag + ".dgamma", c["bwd"]["dgamma"], g.grad, scale=float(c["dy"].abs().sum(dim=0).max()))
        _rel(tag + ".dbeta", c["bwd"]["dbeta"], bt.grad, scale=float(c["dy"].abs().sum(dim=0).max()))
        if res:
            assert torch.equal(c["bwd"]["dres"], r.grad), tag
        n += 1
    assert n >= 40
    # eval mode: the running statistics, unchanged
    c = nc.bn_case(64, 494, bf16, True, True)
    d = {k: c[k].double() for k in ("x", "gamma", "beta", "res", "rm", "rv")}
    ev = nc.bn_forward_ref(d["x"], d["gamma"], d["beta"], d["res"], True, d["rm"], d["rv"], train=False)
    want = F.relu(F.batch_norm(d["x"], d["rm"].clone(), d["rv"].clone(), d["gamma"], d["beta"], training=False, eps=nc.EPS) + d["res"])
    _rel("eval.y", ev["y"], want)
    assert ev["running_mean"] is d["rm"] and ev["running_var"] is d["rv"]


def test_relu_cases_zero_at_most_one_percent_of_dy_and_inputs_are_well_conditioned():
    worst = 0.0
    for C, rows, bf16, res, relu, seed in all_bn_cases():
        c = nc.bn_case(C, rows, bf16, res, relu, seed)
        if relu:
            assert c["zeroed"] <= nc.ZEROED_DY_CAP, (C, rows, bf16, res, c["zeroed"])
            worst = max(worst, c["zeroed"])
            if not bf16:
                near = c["fwd"]["pre"].abs() < 1e-3
                assert bool((c["dy"][near] == 0).all()) and abs(float(near.double().mean()) - c["zeroed"]) < 1e-12
        else:
            assert c["zeroed"] == 0.0
        sd = torch.sqrt(c["fwd"]["var"])
        # (a sample of two to five rows can sit closer together than the distribution it is drawn from: |offset| <= 1 = 1.2 sigma)
        assert float(c["fwd"]["var"].min()) >= 0.1 and (rows < 31 or float((c["fwd"]["mean"].abs() / sd).max()) <= 2.0), (C, rows)
    print(f"\nlargest fraction of dy zeroed near pre = 0: {worst:.4f}")
    assert worst > 0.0


@pytest.mark.parametrize("bf16", [False, True], ids=DT_IDS)
def test_float32_formulas_stay_inside_the_batchnorm_bars(bf16):
    worst = {}
    for C, rows, b, res, relu, seed in all_bn_cases():
        if b != bf16 or rows >= 100_000:
            continue
        c = nc.bn_case(C, rows, b, res, relu, seed)
        m, bars = nc.bn_float32_model(c, bf16, res, relu), nc.bn_bars(c, bf16)
        for name in ("y", "dx", "dgamma", "dbeta"):
            ref = c["fwd"]["y"] if name == "y" else c["bwd"][name]
            rt, at = bars[name]
            ratio = float(((m[name].double() - ref).abs() / (at + rt * ref.abs())).max())
            assert ratio <= 1.0, (C, rows, res, relu, name, ratio)
            worst[name] = max(worst.get(name, 0.0), ratio)
        if res:
            assert torch.equal(m["dres"].double(), c["bwd"]["dres"])
    print(f"\nfloat32 on the CPU, {DT_IDS[bf16]}: worst error / bar " + ", ".join(f"{k} {v:.3f}" for k, v in worst.items()))


def test_slab_split_adds_up_and_has_empty_slabs():
    x = nc.bn_case(32, 561, True, False, True)["x"].double()
    for nslab in nc.NSLABS:
        s = nc.slab_split(x, nslab, f"t{nslab}")
        assert s.shape == (nslab, 2, 32)
        assert float((s[:, 0].sum(dim=0) - x.sum(dim=0)).abs().max()) <= 1e-10 and float((s[:, 1].sum(dim=0) - (x * x).sum(dim=0)).abs().max()) <= 1e-9
        empty = int((s.abs().sum(dim=(1, 2)) == 0).sum())
        assert (empty >= 1) == (nslab >= 4), (nslab, empty)
        if nslab > 1:
            assert len({float(v) for v in s[:, 1, 0]}) > min(nslab, 8) // 2        # uneven: the slabs differ


def test_channel_sum_inputs():
    for rows in (2, 33):
        x = nc.sum_input(64, rows, False, "pm1").double()
        assert set(x.sum(dim=0).tolist()) <= {0.0, 1.0, -1.0} and (rows % 2 == 0) == bool((x.sum(dim=0) == 0).all())
    x = nc.sum_input(32, 33, True, "zero_col")
    assert bool((x[:, 5] == 0).all()) and bool((x[:, 4] != 0).any()) and torch.equal(nc.bf_round(x), x)
    ref = torch.tensor([0.0, 1.0, -8.0], dtype=torch.float64)
    assert nc.sum_bar(ref).tolist() == [8 * 2.0 ** -23, 8 * 2.0 ** -23, 8 * 2.0 ** -23]


@pytest.mark.parametrize("bf16", [False, True], ids=DT_IDS)
def test_written_out_groupnorm_is_torch_float64_and_its_bar_is_inside_the_stage_bar(bf16):
    sizes = set()
    for C, G in nc.GN_CG:
        for shape in nc.GN_SHAPES:
            for res, relu in MODES:
                inp = nc.gn_inputs(C, G, shape, bf16, res)
                x, g, b = inp["x"].double(), inp["gamma"].double(), inp["beta"].double()
                r = inp["res"].double() if res else None
                ref = nc.gn_ref(x, g, b, G, nc.EPS, r, relu)
                # (torch.group_norm: F.group_norm is the same function behind a check that refuses B H W = 1)
                want = torch.group_norm(x.permute(0, 3, 1, 2).contiguous(), G, g, b, nc.EPS, False).permute(0, 2, 3, 1)
                want = want + r if res else want
                want = F.relu(want) if relu else want
                n = shape[1] * shape[2] * (C // G)
                if n == 1:      # variance 0: beta (+ res), exactly
                    exact = b.expand_as(x) + (r if res else 0.0)
                    assert torch.equal(ref["y"], F.relu(exact) if relu else exact)
                assert float((ref["y"] - want).abs().max()) <= 1e-12 * max(1.0, float(want.abs().max())), (C, G, shape)
                bar, f32_part = nc.gn_bar(inp, ref, G, nc.EPS)
                assert float(f32_part.max()) <= nc.GN_STAGE_BAR and float(bar.min()) >= 0.0, (C, G, shape, float(f32_part.max()))
                sizes.add(n)
    # groups of one element, of fewer than a wave, of fewer than 256, of no multiple of 256; C / G no power of two
    assert 1 in sizes and {3, 5} <= sizes and any(64 < n < 256 for n in sizes) and any(n > 256 and n % 256 for n in sizes)
    assert any((C // G) & (C // G - 1) for C, G in nc.GN_CG)
