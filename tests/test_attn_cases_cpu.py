"""CPU: the cases, references, bars and fault models of tests/attn_cases.py are what tests/test_gpu_attn_edges.py needs them to be.

1. the float64 reference is oracle.policy_ref.attn's formula (compared with it and with golden g5_attn.npz on the old 160-token case);
2. the tables hold every limit they are named after with a neighbour on each side, and the inputs have the logits their kind promises;
3. the same formula in plain float32 on the CPU stays inside every derived bar (the worst ratio of error to bar is printed per output);
4. every fault model — the formula with one defect — exceeds the bar of a named case of each kernel form it can apply to by a factor
   of at least 10.  Together 3 and 4 hold the bars' constants from both sides.

A guard of csrc/wsmg_attn.hip and the fault model that stands for its removal (FAULT_CASES names the case that then fails on the GPU):
  `i0 + u < I` of a load, `if (i >= I) break`, `lane < 8 && i0 + lane < I`       last_token_dropped (a guard off by one)
  `mask[...]` read for the tokens of a ragged trip                                tail_mask_ignored
  `corr = expf(m - mx)` applied to acc and ssum                                   no_rescale
  `lg[i] - mx`, `d[u] - mx`, `lg[i] - M`                                          no_max_subtraction
  the token-to-lane mapping of dots8 / halve8                                     tokens_swapped_in_logits
  `-INFINITY` for the tokens past I of a ragged trip                              tail_token_weighs_one
  `m = -INFINITY` of a wave without tokens, `f = expf(wm[w] - M)` = 0 for it      empty_wave_weighs_one
  `dattn ? dattn[...] : 0.f`                                                      dattn_ignored
  the 256-thread stride of `s += ab[i] * da[i]`, the sum of wsum[] over all waves s_first_sweep_only"""
import numpy as np
import pytest
import torch

import attn_cases as ac
from oracle import cases, policy_ref
from util import golden

DT_IDS = ["f32", "bf16"]

# fault -> form -> the (I, kind, mask) at which it must be gross
FAULT_CASES = {
    "last_token_dropped": {"generic": (5, "peak_last", "none"), "same": (9, "peak_last", "none")},
    "tail_mask_ignored": {"generic": (5, "peak_last", "prefix_I-1"), "same": (9, "peak_last", "prefix_I-1")},
    "no_rescale": {"same": (257, "ascending", "none")},
    "no_max_subtraction": {"generic": (17, "shifted+200", "none"), "same": (129, "shifted-200", "none")},
    "tokens_swapped_in_logits": {"same": (9, "lane_tagged", "none")},
    "empty_wave_weighs_one": {"same": (7, "shifted-200", "none")},
    "tail_token_weighs_one": {"same": (7, "shifted-200", "none")},
    "dattn_ignored": {"generic": (5, "plain", "none"), "same": (9, "plain", "none")},
    "s_first_sweep_only": {"generic": (17, "peak_last", "none"), "same": (129, "peak_last", "none")},
}


def test_reference_is_the_oracles_formula_and_reproduces_golden_g5():
    g = golden("g5_attn.npz")
    q, k, v, m = cases.attn_inputs()
    B, _, I = k.shape
    for mask, key in ((ac.T(m), "out"), (None, "out_nomask")):
        inp = {"form": "generic", "I": I, "kind": "plain", "bf16": False, "shared": None, "B": B, "U": B, "q": ac.T(q),
               "k": ac.T(k).permute(0, 2, 1).contiguous(), "v": ac.T(v).permute(0, 2, 1).contiguous(), "inverse": torch.arange(B),
               "mask": mask, "dout": torch.ones(B, 256), "dattn": torch.zeros(B, I)}
        ref = ac.reference(inp)
        o, a = policy_ref.attn(ac.T(q).double(), ac.T(k).double(), ac.T(v).double(), mask)
        assert ref["out"].dtype == torch.float64 and o.dtype == torch.float64
        assert float((ref["out"] - o).abs().max()) <= 1e-13 and float((ref["attn"] - a).abs().max()) <= 1e-14
        np.testing.assert_allclose(ref["out"].numpy(), g[key], rtol=1e-5, atol=1e-6)
        if mask is not None:
            np.testing.assert_allclose(ref["attn"].numpy(), g["attn"], rtol=1e-5, atol=1e-7)
        # the written-out formula of evaluate() is the same function, gradients included
        got = ac.evaluate(inp)
        for n in ("dq", "dk", "dv", "dlogits"):
            r = ref["grads"]["both"][n]
            assert float((got[n] - r).abs().max()) <= 1e-12 * (1 + float(r.abs().max())), n


def test_tables_straddle_every_limit_they_are_named_after():
    for form, limits in (("generic", (4, 16, 256, 2560)), ("same", (8, 128, 256, 2560))):
        have = set(ac.COUNTS[form])
        for n in limits:
            if n == 256 and form == "same":      # the 1024-thread stride of its last loop is 4 x 256: 136 below, 257 above
                assert any(128 < c < 256 for c in have) and 257 in have
                continue
            assert n in have and n - 1 in have or n == 2560, (form, n)
            assert n + 1 in have or n == 2560, (form, n)           # 2561 is refused: REFUSED_I
        assert ac.AMAX_I in have and ac.AMAX_I - 1 not in have and max(have) == ac.AMAX_I and ac.REFUSED_I == ac.AMAX_I + 1
        assert any(ac.AMAX_I > c > ac.sweep(form) for c in have)            # 2560 has an accepted neighbour below: 2304
        assert 1 in have and min(c for c in have if c > 1) < ac.FORMS[form]["trip"]      # below one trip
        assert 2304 in have
    # 136 = 128 + 8: the second sweep of the keys-are-values kernels has exactly one wave with tokens
    assert 136 in ac.COUNTS["same"] and 136 % 8 == 0 and 136 % 128 == 8
    for name, (U, inv) in ac.SHARED.items():
        assert max(inv) < U
    assert ac.SHARED["u1"][0] == 1 and len(ac.SHARED["b1"][1]) == 1
    assert 1 not in ac.SHARED["unused_set"][1] and set(ac.SHARED["set_of_every_row"][1]) == {1}
    assert ac.SHARED["unsorted"][1] != sorted(ac.SHARED["unsorted"][1])
    for form in ac.FORMS:
        for I in ac.COUNTS[form]:
            got = ac.combos(form, I)
            assert {k for k, _ in got} == set(ac.KINDS) | {"grid"}
            for k in ac.KINDS:       # every kind meets every mask that fits, at the large counts too
                assert [m for kk, m in got if kk == k] == [m for m in ac.MASKS if ac.applies(form, I, m)]
                assert ac.combos(form, I, k) == [c for c in got if c[0] == k]
            if I > ac.sweep(form):
                assert {m for _, m in got} == set(ac.MASKS) | {"full_row"}


@pytest.mark.parametrize("form", list(ac.FORMS))
def test_inputs_have_the_logits_their_kind_promises(form):
    trip, waves = ac.FORMS[form]["trip"], ac.FORMS[form]["waves"]
    for bf16 in (False, True):
        for I in (17, 257) if form == "generic" else (129, 257):
            l = {k: ac.reference(ac.inputs(form, I, k, "none", bf16))["logits"] for k in ac.KINDS}
            span = l["plain"].max(dim=1).values - l["plain"].min(dim=1).values
            assert float(span.min()) >= 20.0, float(span.min())                     # scaled logits span several tens
            asc = l["ascending"]
            want = min(I - 1.0, 80.0)                                               # about 1 per token, up to a span of about 80
            assert abs(float((asc[:, -1] - asc[:, 0]).min()) - want) <= 0.5 and abs(float((asc[:, -1] - asc[:, 0]).max()) - want) <= 0.5
            for w in range(min(waves, I // trip)):                                  # every trip of a wave raises its running maximum
                tops = torch.stack([asc[:, i0:i0 + trip].max(dim=1).values for i0 in range(w * trip, I, trip * waves)], dim=1)
                assert bool((tops[:, 1:] > tops[:, :-1]).all())
            assert bool((asc.argmax(dim=1) == I - 1).all())
            for kind, p in (("peak_last", I - 1), ("peak_first", 0)):
                rest = torch.cat([l[kind][:, :p], l[kind][:, p + 1:]], dim=1).max(dim=1).values
                assert float((l[kind][:, p] - rest).min()) >= 30.0
            for kind, t in (("shifted+200", 200.0), ("shifted-200", -200.0)):
                assert float((l[kind].mean(dim=1) - t).abs().max()) <= 10.0 and float((l[kind] - t).abs().max()) <= 40.0
            tag = l["lane_tagged"][:, :8]
            assert float((tag[:, 1:] - tag[:, :-1]).min()) >= 2.0                   # the 8 tokens of a trip: distinct by e^2 at least
            v = ac.inputs(form, I, "lane_tagged", "none", bf16)["v"][:, :8].double()
            assert float((v[:, 1:] - v[:, :-1]).abs().sum(dim=2).min()) > 1.0
    inp = ac.inputs(form, 17 if form == "generic" else 129, "grid", "full_row", False)
    for n in ("q", "k", "v"):
        assert torch.equal(inp[n], inp[n].round()) and float(inp[n].abs().max()) <= 2.0 and torch.equal(ac.bf_round(inp[n]), inp[n])
    assert bool(inp["mask"][-1].all()) and not bool(inp["mask"][:-1].all(dim=1).any())
    a = ac.reference(inp)["attn"]
    assert bool(torch.isfinite(a).all()) and float((a.sum(dim=1) - 1).abs().max()) <= 1e-14 and float(a[-1].min()) > 0.0
    for name in ac.SHARED:                                       # shared sets: some row's set is masked altogether
        sh = ac.inputs("generic", 17, "grid", "full_row", False, name)
        assert bool(sh["mask"][sh["inverse"]].all(dim=1).any())
    if form == "same":      # the folded query is exact in float32: the product in float32 equals the product in float64
        p = ac.inputs(form, 9, "plain", "none", False)
        assert torch.equal((p["q0"].float() @ p["W"].float()).double(), p["q0"] @ p["W"]) and torch.equal(p["q"].double(), p["q0"] @ p["W"])
    sc = ac.inputs(form, 257, "plain", "scattered", False)       # the scattered mask hides the largest raw logit of every row
    d = torch.einsum("bc,bic->bi", sc["q"].double(), sc["k"].double())
    assert bool(sc["mask"][torch.arange(sc["B"]), d.argmax(dim=1)].all()) and 0.2 < float(sc["mask"].float().mean()) < 0.5


COUNT_GROUPS = [(f, g) for f in ac.FORMS for g in ("small", ) + tuple(I for I in ac.COUNTS[f] if I >= ac.LARGE)]


@pytest.mark.parametrize("bf16", [False, True], ids=DT_IDS)
@pytest.mark.parametrize("form,group", COUNT_GROUPS, ids=[f"{f}-{g}" for f, g in COUNT_GROUPS])
def test_float32_evaluation_stays_inside_every_bar(form, group, bf16):
    """The formula in float32 (torch on the CPU: another summation order, the same roundings per operation) at every case of the
    per-row tables (the counts below 2304 together, 2304 and 2560 each alone); the worst ratio of error to bar per output is printed,
    and none exceeds 1."""
    worst = {}
    for I in [c for c in ac.COUNTS[form] if c < ac.LARGE] if group == "small" else [group]:
        for kind, mask in ac.combos(form, I):
            inp = ac.inputs(form, I, kind, mask, bf16)
            ref = ac.reference(inp)
            modes = ("both", "dout", "dattn") if (kind, mask) in (("plain", "none"), ("grid", "full_row")) else ("both",)
            for mode in modes:
                r = ac.worst_ratios(ac.evaluate(inp, torch.float32, mode=mode), inp, ref, mode)
                for n, x in r.items():
                    if x > worst.get(n, (0.0,))[0]:
                        worst[n] = (x, f"I={I} {kind} {mask} {mode}")
    for n, (x, where) in sorted(worst.items()):
        print(f"float32 on the CPU, {form} {group} {DT_IDS[bf16]} {n}: worst error / bar {x:.3f} at {where}")
    assert all(x <= 1.0 for x, _ in worst.values()), worst


def test_shared_set_float32_evaluation_stays_inside_its_bars():
    """The shared-set bars (the rows' bars summed per set): float32 autograd through a gather of the sets."""
    worst = {}
    for name in ac.SHARED:
        for I in (5, 257):
            for kind, mask in (("plain", "scattered"), ("ascending", "none"), ("grid", "full_row")):
                inp = ac.inputs("generic", I, kind, mask, False, name)
                ref = ac.reference(inp)
                q, k, v = (inp[n].clone().requires_grad_(True) for n in ("q", "k", "v"))
                d = torch.einsum("bc,bic->bi", q, k[inp["inverse"]])
                if inp["mask"] is not None:
                    d = torch.where(inp["mask"][inp["inverse"]], d - torch.tensor(1e8), d)
                a = torch.softmax(d * ac.SCALE, dim=1)
                out = torch.einsum("bi,bic->bc", a, v[inp["inverse"]])
                ((out * inp["dout"]).sum() + (a * inp["dattn"]).sum()).backward()
                got = {"out": out.detach(), "attn": a.detach(), "dq": q.grad, "dk": k.grad, "dv": v.grad}
                for n, x in ac.worst_ratios(got, inp, ref).items():
                    worst[n] = max(worst.get(n, 0.0), x)
                used = set(inp["inverse"].tolist())
                for u in set(range(inp["U"])) - used:
                    assert float(ref["grads"]["both"]["dk"][u].abs().max()) == 0.0 and float(ref["grads"]["both"]["dv"][u].abs().max()) == 0.0
    print("float32 on the CPU, shared sets: worst error / bar", {n: round(x, 3) for n, x in worst.items()})
    assert all(x <= 1.0 for x in worst.values()), worst


@pytest.mark.parametrize("fault", list(ac.FAULTS))
def test_every_fault_model_is_gross_at_its_named_case(fault):
    """The formula with one defect, in float64, against the bars: at least 10 times the bar of some output that the GPU test of that
    form compares (attn_cases.COMPARED: not dlogits, which only the shared entry points return), for each form the defect can apply
    to and in both dtypes.  Without the defect the same evaluation is inside the bars by many orders."""
    assert set(FAULT_CASES[fault]) == set(ac.FAULTS[fault])
    for form, (I, kind, mask) in FAULT_CASES[fault].items():
        assert I in ac.COUNTS[form] and (kind, mask) in ac.combos(form, I)
        for bf16 in (False, True):
            inp = ac.inputs(form, I, kind, mask, bf16)
            ref = ac.reference(inp)
            clean = ac.worst_ratios(ac.evaluate(inp), inp, ref)
            bad = {n: x for n, x in ac.worst_ratios(ac.evaluate(inp, fault=fault), inp, ref).items() if n in ac.COMPARED[form]}
            assert set(bad) == set(ac.COMPARED[form])
            name = max(bad, key=bad.get)
            print(f"fault {fault}, {form} {DT_IDS[bf16]} I={I} {kind} {mask}: {name} at {bad[name]:.3g} x its bar "
                  f"(without the defect {max(clean.values()):.2g})")
            # (bf16: evaluate() rounds dk, dv, dx to bf16, half an ulp = at most 2^-8 of the value: up to the whole BF16_EPS term)
            assert max(clean.values()) <= (1.0 if bf16 else 1e-6), clean
            assert bad[name] >= 10.0, bad
