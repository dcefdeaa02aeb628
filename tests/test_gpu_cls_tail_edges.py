"""GPU: the fused classifier tail (csrc/wsmg_cls_tail.hip) at the edges of its patch loop, of its label arithmetic, of its class
masks and of cls_tail_finish_kernel's sample groups.  wsmg_cls_tail_fwd_bf16 and wsmg_cls_tail_bwd_bf16 are called directly, so mean,
invstd, gamma and beta are inputs and the per-sample records part[B][1120] can be read back.  Cases, the float64 model, the bars and
the comparison functions are those of tests/cls_tail_cases.py (checked on the CPU by tests/test_cls_tail_cases_cpu.py, which also
shows that the comparisons reject a dropped patch, swapped resize scales, a row bound from Wg, skipped tail samples and the
BatchNorm constants of a neighbouring channel).  Every comparison prints what it measured beside its bar (profiles/cls_tail_edges.txt).

Exact path (no ground truth): inputs on which no rounding point of the kernel rounds and every float32 sum is exact, so sem, pooled,
dbn, the records and dgamma / dbeta / dw6 / db6 must equal the float64 model element for element; padded channels are zero, rows of
dw6 / db6 from `classes` on stay untouched, two launches agree, and without d pooled every gradient is an exact, written zero.
Cross-entropy path: sem and pooled still exact (integer logits); ce_rows against the float64 loss within
max(8 max|float32 torch - float64|, 1e-6 max|ce|); the backward against the model with the kernel's rounding points, per output
within 4 max|model in float32 - model in float64| + n 2^-24 sum|terms|."""
import ctypes

import pytest
import torch

import cls_tail_cases as cc

pytestmark = pytest.mark.gpu

NAN = float("nan")


def P(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def S():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def run(c, ce, dp=True):
    """One forward and one backward call on case c; every output starts as NaN.  -> the outputs of cls_tail_cases.OUT_KEYS (+ ce),
    dw6 / db6 as the whole poisoned [32, 32] / [32] buffers."""
    from wsmgmap import _abi
    B, H, W, Hg, Wg, classes = c["geom"]
    inp = c["inp"]
    bf = torch.bfloat16
    y2 = inp["y2"].to(bf).cuda()
    par = {k: inp[k].float().cuda() for k in ("gamma", "beta", "mean", "invstd", "w6", "b6")}
    gt = inp["gt"].float().cuda() if ce else None
    g_rows = inp["g_rows"].float().cuda() if ce else None
    dpooled = inp["dpooled"].to(bf).cuda() if dp else None
    if not ce:
        Hg = Wg = 0
    sem = torch.full((B, H, W, 32), NAN, dtype=bf, device="cuda")
    pooled = torch.full((B, H // 2, W // 2, 32), NAN, dtype=bf, device="cuda")
    ce_rows = torch.full((B,), NAN, device="cuda") if ce else None
    head = (P(y2), P(par["gamma"]), P(par["beta"]), P(par["mean"]), P(par["invstd"]), P(par["w6"]), P(par["b6"]), classes, P(gt), Hg, Wg)
    _abi.call("wsmg_cls_tail_fwd_bf16", *head, B, H, W, P(sem), P(pooled), P(ce_rows), S())
    nws = int(_abi.lib().wsmg_cls_tail_workspace_floats(B))
    assert nws == B * cc.PART
    dbn = torch.full((B, H, W, 32), NAN, dtype=bf, device="cuda")
    ws = torch.full((nws,), NAN, device="cuda")
    dgamma, dbeta, db6 = (torch.full((32,), NAN, device="cuda") for _ in range(3))
    dw6 = torch.full((32, 32), NAN, device="cuda")
    _abi.call("wsmg_cls_tail_bwd_bf16", *head, P(g_rows), P(dpooled), B, H, W, P(dbn), P(ws), nws, P(dgamma), P(dbeta), P(dw6), P(db6), S())
    torch.cuda.synchronize()
    out = dict(sem=sem, pooled=pooled, dbn=dbn, part=ws.view(B, cc.PART), dgamma=dgamma, dbeta=dbeta, dw6_buf=dw6, db6_buf=db6,
               dw6=dw6[:classes], db6=db6[:classes])
    if ce:
        out["ce"] = ce_rows
    return {k: v.cpu() for k, v in out.items()}


def check_padding(name, c, out):
    classes = c["geom"][5]
    if classes < 32:
        assert float(out["sem"][..., classes:].float().abs().max()) == 0.0, f"{name}: sem beyond class {classes}"
        assert float(out["pooled"][..., classes:].float().abs().max()) == 0.0, f"{name}: pooled beyond class {classes}"
        assert bool(torch.isnan(out["dw6_buf"][classes:]).all()) and bool(torch.isnan(out["db6_buf"][classes:]).all()), \
            f"{name}: rows of dw6 / db6 from {classes} on were written"


def same_bits(a, b):
    return all(torch.equal(torch.nan_to_num(a[k].float(), nan=12345.0), torch.nan_to_num(b[k].float(), nan=12345.0)) for k in a)


@pytest.mark.parametrize("name", cc.EXACT_CASES)
def test_exact_inputs_give_the_float64_model_bit_for_bit(name):
    c = cc.case(name, "exact")
    out = run(c, ce=False)
    report = []
    fails = cc.compare_exact(out, c["want"], report)
    print("\n" + "\n".join(f"exact.{name}.{line}" for line in report))
    assert not fails, f"{name}: " + "; ".join(fails)
    check_padding(name, c, out)
    assert same_bits(out, run(c, ce=False)), f"{name}: two launches differ"


@pytest.mark.parametrize("name", cc.EXACT_CASES)
def test_without_d_pooled_every_gradient_is_a_written_zero(name):
    c = cc.case(name, "exact")
    out = run(c, ce=False, dp=False)
    report = []
    fails = cc.compare_exact(out, c["want_nodp"], report)
    print("\n" + "\n".join(f"nodp.{name}.{line}" for line in report))
    assert not fails, f"{name}: " + "; ".join(fails)
    for k in ("dbn", "part", "dgamma", "dbeta", "dw6", "db6"):
        assert not bool(torch.isnan(out[k].float()).any()) and float(out[k].float().abs().max()) == 0.0, f"{name}: {k}"
    check_padding(name, c, out)


@pytest.mark.parametrize("name", cc.CE_CASES)
def test_cross_entropy_path_against_the_model_with_the_kernels_rounding_points(name):
    c = cc.case(name, "ce")
    out = run(c, ce=True)
    report = []
    fails = cc.compare_ce(c, out, report)
    print("\n" + "\n".join(f"ce.{name}.{line}" for line in report))
    assert not fails, f"{name}: " + "; ".join(fails)
    check_padding(name, c, out)
    assert same_bits(out, run(c, ce=True)), f"{name}: two launches differ"
