"""CPU: the cases, the model and the bars of tests/cls_tail_cases.py are what tests/test_gpu_cls_tail_edges.py needs them to be.

1. every case builds: the exact cases meet the builder's conditions (no rounding point rounds, float32 partial sums exact, products
   within 2^10), the ce cases have integer logits spanning +-6, a loss bar under 1e-4 max|ce| and backward bars under half of every
   patch's contribution — a case that does not is an error, never a skip;
2. the model with rounding off is torch autograd in float64, sample by sample, and its labels are F.interpolate's;
3. patch counts, per and the finish kernel's group bounds are what the case names promise, by arithmetic written here;
4. a single wrong label moves a loss row by more than ten times its bar;
5. five fault models — the last patch of a sample dropped, sy and sx swapped, the label's row bound taken from Wg, the finish
   kernel's tail samples skipped, the BatchNorm constants of channel c ^ 1 — are each rejected by the GPU test's own comparison
   functions on at least one case."""
import pytest
import torch
import torch.nn.functional as F

import cls_tail_cases as cc


def test_every_case_builds_and_meets_the_builders_conditions():
    for name in cc.EXACT_CASES:
        c = cc.case(name, "exact")
        B, H, W, Hg, Wg, classes = c["geom"]
        w = c["want"]
        assert w["sem"].shape == (B, H, W, 32) and w["pooled"].shape == (B, H // 2, W // 2, 32) and w["part"].shape == (B, cc.PART)
        assert w["dw6"].shape == (classes, 32) and w["db6"].shape == (classes,)
        assert float(w["sem"][..., classes:].float().abs().sum()) == 0.0 and float(w["dbn"].float().abs().max()) > 0.0
        # every sample has data of its own: no two records agree
        assert len({tuple(r.tolist()) for r in w["part"]}) == B
        # without d pooled (and without a loss) every gradient is an exact zero
        z = c["want_nodp"]
        assert all(float(z[k].float().abs().max()) == 0.0 for k in ("dbn", "part", "dgamma", "dbeta", "dw6", "db6"))
        assert torch.equal(z["sem"], w["sem"]) and torch.equal(z["pooled"], w["pooled"])
    for name in cc.CE_CASES:
        c = cc.case(name, "ce")
        ce_max = float(c["ce64"].abs().max())
        assert c["ce_bar"] <= 1e-4 * ce_max and c["ce_bar"] >= 8.0 * float((c["ce32"].double() - c["ce64"]).abs().max())
        assert all(bool((v >= 0).all()) for v in c["bars"].values())
    k = cc.constants()
    pairs = {(float(k["scale"][i]), float(k["shift"][i]), float(k["invstd"][i]), float(k["mean"][i])) for i in range(32)}
    assert len(pairs) == 32 and all(float(k["scale"][i]) != float(k["scale"][i ^ 1]) for i in range(32))
    assert len({tuple(r.tolist()) for r in k["w6"]}) == 32 and set(k["w6"].flatten().tolist()) == {-1.0, 0.0, 1.0}
    assert set((k["invstd"] * k["gamma"]).tolist()) == {0.5, 1.0, 2.0} and torch.equal(k["beta"] - k["mean"] * k["scale"], k["shift"])


@pytest.mark.parametrize("kind", ["exact", "ce"])
def test_model_with_rounding_off_is_torch_autograd_in_float64(kind):
    for name in (cc.EXACT_CASES if kind == "exact" else cc.CE_CASES):
        inp = cc.case(name, kind)["inp"]
        B, H, W, Hg, Wg, classes = cc.GEOMETRIES[name]
        m = cc.model(inp, False, ce=kind == "ce")
        if kind == "ce":
            want = F.interpolate(inp["gt"].unsqueeze(1), size=(H, W)).squeeze(1).long()
            assert torch.equal(cc.labels_of(inp["gt"], H, W), want), name
            labs = set(inp["gt"].flatten().tolist())
            assert labs <= set(map(float, range(classes))) and len(labs) >= min(classes, 8), name
            if classes > 1:     # neighbouring source cells differ nearly everywhere
                g = inp["gt"]
                assert float((g[:, :, 1:] != g[:, :, :-1]).double().mean()) >= 0.7 * (1 - 1 / classes), name
        tot = {k: 0.0 for k in ("gamma", "beta", "w6", "b6")}
        for b in range(B):
            y2 = inp["y2"][b:b + 1].clone()
            p = {k: inp[k].clone().requires_grad_(True) for k in ("gamma", "beta", "w6", "b6")}
            bn = ((y2 - inp["mean"]) * inp["invstd"] * p["gamma"] + p["beta"]).permute(0, 3, 1, 2)       # NCHW, as the reference
            bn.retain_grad()
            logits = F.conv2d(torch.relu(bn), p["w6"].view(classes, 32, 1, 1), p["b6"])
            pooled = F.avg_pool2d(logits, 2)
            loss = (pooled * inp["dpooled"][b:b + 1, ..., :classes].permute(0, 3, 1, 2)).sum()
            if kind == "ce":
                target = F.interpolate(inp["gt"][b:b + 1].unsqueeze(1), size=(H, W)).squeeze(1).long()
                ce = F.cross_entropy(logits, target, reduction="none").mean([1, 2])
                loss = loss + (ce * inp["g_rows"][b:b + 1]).sum()
                assert abs(float(ce.detach()) - float(m["ce"][b])) <= 1e-12 * max(1.0, abs(float(ce.detach()))), name
            loss.backward()
            for got, ref, what in ((m["sem"][b, ..., :classes], logits[0].permute(1, 2, 0), "sem"),
                                   (m["pooled"][b, ..., :classes], pooled[0].permute(1, 2, 0), "pooled"),
                                   (m["dbn"][b], bn.grad[0].permute(1, 2, 0), "dbn"),
                                   (m["part"][b, 0:32], p["beta"].grad, "sum dy"), (m["part"][b, 32:64], p["gamma"].grad, "sum dy xhat"),
                                   (m["part"][b, 64:64 + 32 * 32].view(32, 32)[:classes], p["w6"].grad, "dW"),
                                   (m["part"][b, 64 + 32 * 32:][:classes], p["b6"].grad, "db")):
                s = max(1.0, float(ref.detach().abs().max()))
                assert float((got - ref.detach()).abs().max()) <= 1e-12 * s, (name, b, what)
            for k2 in tot:
                tot[k2] = tot[k2] + p[k2].grad
        for got, ref, what in ((m["dgamma"], tot["gamma"], "dgamma"), (m["dbeta"], tot["beta"], "dbeta"), (m["dw6"][:classes], tot["w6"], "dw6"),
                               (m["db6"][:classes], tot["b6"], "db6")):
            assert float((got - ref).abs().max()) <= 1e-12 * max(1.0, float(ref.abs().max())), (name, what)
        assert float(m["part"][:, 64:64 + 32 * 32].view(B, 32, 32)[:, classes:].abs().sum()) == 0.0


def test_patch_counts_and_sample_groups_are_what_the_names_promise():
    for name, (B, H, W, Hg, Wg, classes) in cc.GEOMETRIES.items():
        assert H % 2 == 0 and W % 16 == 0 and 1 <= classes <= 32
        assert (H // 2) * (W // 16) == cc.PATCHES[name], name
    counts = sorted({cc.PATCHES[n] for n in cc.GEOMETRIES})
    assert counts == [1, 7, 9, 15, 17]
    # a ragged last trip of `for (p = wave; p < npatch; p += 8)`: some waves run one patch more than others
    assert sum(1 for n in cc.GEOMETRIES if cc.PATCHES[n] % 8 and cc.PATCHES[n] > 8) >= 4
    g = cc.GEOMETRIES
    assert (g["nine_tall"][2] // 16, g["nine_3x3"][2] // 16) == (1, 3)                          # 9 patches two ways
    ratios = {n: (g[n][3] / g[n][1], g[n][4] / g[n][2]) for n in g}
    assert any(a > 1 and b > 1 and a != b for a, b in ratios.values())                          # down-scaling, a ratio per axis
    assert any(a < 1 or b < 1 for a, b in ratios.values()) and (1.0, 1.0) in ratios.values()     # up-scaling; the identity
    assert any(a != int(a) and 1 / a != int(1 / a) for a, _ in ratios.values())                  # a non-integer ratio
    assert all(g[n][3] != g[n][4] for n in ("one_patch", "seven_in_a_row", "nine_tall", "nine_3x3", "fifteen"))
    assert {g[n][5] for n in g} >= {1, 4, 5, 8, 17, 27, 32}
    for name, (B, per) in cc.BATCHES.items():
        assert cc.GEOMETRIES[name][0] == B and (B + 15) // 16 == per == cc.group_bounds(B)[0]
        groups = [(grp * per, min(grp * per + per, B)) for grp in range(16)]
        assert groups == cc.group_bounds(B)[1]
        assert sorted(b for b0, b1 in groups for b in range(b0, b1)) == list(range(B))
    size = lambda B: [max(b1 - b0, 0) for b0, b1 in cc.group_bounds(B)[1]]
    assert size(16) == [1] * 16 and size(17) == [2] * 8 + [1] + [0] * 7 and size(128) == [8] * 16 and size(130) == [9] * 14 + [4, 0]
    assert cc.finish_tail_samples(128) == [] and len(cc.finish_tail_samples(16)) == 16 and len(cc.finish_tail_samples(17)) == 17
    assert cc.finish_tail_samples(130) == [9 * grp + 8 for grp in range(14)] + [126, 127, 128, 129]


def test_one_wrong_label_moves_a_loss_row_far_beyond_its_bar():
    for name in cc.CE_CASES:
        c = cc.case(name, "ce")
        B, H, W, Hg, Wg, classes = c["geom"]
        if classes == 1:
            assert c["ce_bar"] == 0.0 and float(c["ce64"].abs().max()) == 0.0       # the soft-max over one class: the loss is 0
            continue
        assert 1.0 / (H * W) > 10.0 * c["ce_bar"], (name, c["ce_bar"])
        # and on the data: the label of one pixel moved to a class whose (integer) logit differs there
        inp = c["inp"]
        m = cc.model(inp, True, ce=True)
        lg = m["logits"][0, 0, 0, :classes]
        t = int(cc.labels_of(inp["gt"], H, W)[0, 0, 0])
        other = next(k for k in range(classes) if float(lg[k]) != float(lg[t]))
        assert abs(float(lg[other] - lg[t])) / (H * W) > 10.0 * c["ce_bar"]


def _as_kernel_output(m, classes, ce):
    out = cc.outputs_of(m, classes)
    if not ce:
        out.pop("ce", None)
    return out


@pytest.mark.parametrize("mut", cc.MUTATIONS)
def test_the_comparison_rejects_each_fault_model_on_some_case(mut):
    caught = []
    for kind, names, cmp in (("exact", cc.EXACT_CASES, None), ("ce", cc.CE_CASES, None)):
        for name in names:
            c = cc.case(name, kind)
            classes = c["geom"][5]
            bad = _as_kernel_output(cc.model(c["inp"], True, ce=kind == "ce", mut=mut), classes, kind == "ce")
            good = _as_kernel_output(cc.model(c["inp"], True, ce=kind == "ce"), classes, kind == "ce")
            if kind == "exact":
                assert cc.compare_exact(good, c["want"]) == [], name
                fails = cc.compare_exact(bad, c["want"])
            else:
                assert cc.compare_ce(c, good) == [], name
                fails = cc.compare_ce(c, bad)
            if fails:
                caught.append((kind, name, fails[0]))
    print(f"\n{mut}: rejected on {len(caught)} cases: " + ", ".join(f"{k}.{n}" for k, n, _ in caught))
    assert caught, mut
    kinds = {k for k, _, _ in caught}
    names = {n for _, n, _ in caught}
    if mut == "drop_last_patch":            # every case has a last patch: every case must see it, in its reduced outputs too
        assert len(caught) == len(cc.EXACT_CASES) + len(cc.CE_CASES)
        for name in cc.CE_CASES:
            c = cc.case(name, "ce")
            bad = _as_kernel_output(cc.model(c["inp"], True, ce=True, mut=mut), c["geom"][5], True)
            bad.update({k: c["want"][k] for k in ("sem", "pooled", "dbn")})       # the reductions alone
            bad["ce"] = c["ce64"].float()
            assert any(f.split(":")[0] in ("part",) + cc.REDUCED for f in cc.compare_ce(c, bad)), name
    if mut in ("swap_sy_sx", "row_bound_from_Wg"):
        assert kinds == {"ce"} and "nine_3x3" in names and "nine_tall" in names
    if mut == "skip_finish_tail":
        assert {"B16", "B17", "B130"} <= names and "B128" not in names
    if mut == "bn_of_c_xor_1":
        assert len(caught) == len(cc.EXACT_CASES) + len(cc.CE_CASES)
