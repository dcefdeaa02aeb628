#!/usr/bin/env python3
"""GPU-box tool: SHA-256 of every output of the attention family (csrc/wsmg_attn*.hip) on fixed inputs — the listing two builds of
the library must share when a change claims to leave their bits alone.

    python3 tools/attn_bits.py [--out FILE]                    (WSMG_LIB=<other build>/libwsmgmap.so for the other side)

Inputs come from CPU generators with fixed seeds; every entry point of the four files is called.
Single-query forms (B = 3; I = 1, 7, 8, 9, 33, 129, 257, 2560: 8 | 9 straddle one trip, 129 opens the second trip of the 16-wave kernels,
2560 is the LDS limit; float32 and bf16; no mask, a scattered mask, a mask with one fully masked row): forward and backward with one
tensor (k == v, dk == dv), two tensors, and two tensors with one gradient buffer (k != v, dk == dv), dattn given and NULL; the shared-set
entry points over U = 2 sets of which one is unused, with dlogits.
e4m3 forms (L = 1, 33, 160, 224): the row, split and backward kernels at B = 3, scale fixed and computed on the device; prep, MFMA
forward, fused forward and MFMA backward at B = 5 over U = 2; the two quantise entry points at n = 4 and n = 1028.
One `name shape sha256` line per tensor; the digest is of the tensor's bytes after a copy to the host."""
import argparse
import hashlib
import importlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "ws-mgmap_amd"))
import torch  # noqa: E402

from wsmgmap import _abi  # noqa: E402

A = importlib.import_module("wsmgmap.ops.attention")     # (the package's `attention` attribute is the function of that name)

P, S = A._p, A._stream
C, SCALE = 256, 1.0 / 16
COUNTS = [1, 7, 8, 9, 33, 129, 257, 2560]
F8_COUNTS = [1, 33, 160, 224]
LINES = []


def emit(name, t):
    h = t.detach().contiguous().cpu()
    h = h.view(torch.int16) if h.dtype == torch.bfloat16 else h
    LINES.append(f"{name} {tuple(h.shape)} {hashlib.sha256(h.numpy().tobytes()).hexdigest()}")


def gen(*seed):
    g = torch.Generator()
    g.manual_seed(sum(s * 1009 ** i for i, s in enumerate(seed)) + 29)
    return g


def empty(*shape, dtype=torch.float32):
    return torch.full(shape, float("nan"), device="cuda", dtype=dtype) if dtype.is_floating_point else torch.zeros(shape, device="cuda", dtype=dtype)


def masks(rows, I, g):
    scattered = torch.rand(rows, I, generator=g) < 0.3
    scattered[:, 0] = False
    full = scattered.clone()
    full[rows - 1] = True
    return {"nomask": None, "scattered": scattered.to(torch.uint8).cuda(), "fullrow": full.to(torch.uint8).cuda()}


def single_query(I, dtype):
    B, U = 3, 2
    sfx = "_bf16" if dtype == torch.bfloat16 else ""
    g = gen(1, I, len(sfx))
    q, dout = torch.randn(B, C, generator=g).cuda(), torch.randn(B, C, generator=g).cuda()
    dattn = (torch.randn(B, I, generator=g) * 0.1).cuda()
    k = torch.randn(B, I, C, generator=g).to(dtype).cuda()
    v = torch.randn(B, I, C, generator=g).to(dtype).cuda()
    k2 = k.clone()                                    # equal values, another tensor
    inv = torch.ones(B, dtype=torch.int64).cuda()     # every row uses set 1: set 0 is unused
    tag0 = f"I{I}.{'bf16' if sfx else 'f32'}"
    for mname, m in masks(B, I, g).items():
        for form, kk, vv in (("one", k, k), ("two", k, v), ("two_eq", k, k2)):
            tag = f"{tag0}.{mname}.{form}"
            out, attn = empty(B, C), empty(B, I)
            _abi.call("wsmg_attn_fwd" + sfx, P(q), P(kk), P(vv), P(m), SCALE, B, I, C, P(out), P(attn), S())
            emit(f"attn_fwd.{tag}.out", out)
            emit(f"attn_fwd.{tag}.attn", attn)
            for gname, ga in (("dattn", dattn), ("null", None)):
                grads = (("dx",),) if form == "one" else (("dk", "dv"), ("dkv",))          # dkv: one gradient buffer for two tensors
                for names in grads:
                    dq = empty(B, C)
                    bufs = [empty(B, I, C, dtype=dtype) for _ in names]
                    _abi.call("wsmg_attn_bwd" + sfx, P(q), P(kk), P(vv), P(attn), P(dout), P(ga), SCALE, B, I, C, P(dq), P(bufs[0]), P(bufs[-1]), S())
                    for n, t in zip(("dq",) + names, [dq] + bufs):
                        emit(f"attn_bwd.{tag}.{gname}.{'+'.join(names)}.{n}", t)
    ks, vs = k[:U].contiguous(), v[:U].contiguous()
    for mname, m in masks(U, I, g).items():
        tag = f"{tag0}.{mname}"
        out, attn = empty(B, C), empty(B, I)
        _abi.call("wsmg_attn_shared_fwd" + sfx, P(q), P(ks), P(vs), P(m), P(inv), SCALE, B, I, C, P(out), P(attn), S())
        emit(f"attn_shared_fwd.{tag}.out", out)
        emit(f"attn_shared_fwd.{tag}.attn", attn)
        for gname, ga in (("dattn", dattn), ("null", None)):
            dq, dl = empty(B, C), empty(B, I)
            _abi.call("wsmg_attn_shared_bwd" + sfx, P(q), P(ks), P(vs), P(attn), P(dout), P(ga), P(inv), SCALE, B, I, C, P(dq), P(dl), S())
            emit(f"attn_shared_bwd.{tag}.{gname}.dq", dq)
            emit(f"attn_shared_bwd.{tag}.{gname}.dlogits", dl)


def quantise(n):
    x = (torch.randn(n, generator=gen(2, n)) * 3).cuda()
    x[0] = 1e6                                       # saturates
    sc = torch.tensor([0.0173], device="cuda")
    y = empty(n, dtype=torch.uint8)
    _abi.call("wsmg_quantize_e4m3", P(x), n, 1.0 / 0.0173, P(y), S())
    emit(f"quantize_e4m3.n{n}", y)
    y = empty(n, dtype=torch.uint8)
    _abi.call("wsmg_quantize_e4m3_dev", P(x), n, P(sc), P(y), S())
    emit(f"quantize_e4m3_dev.n{n}", y)


def fp8_rows(L):
    """wsmg_quantize_e4m3_dev, wsmg_attn_fp8_row_fwd, wsmg_attn_fp8_fold + wsmg_attn_fp8_fwd (split), wsmg_attn_fp8_bwd at B = 3"""
    B = 3
    g = gen(3, L)
    q, dout = torch.randn(B, C, generator=g).cuda(), torch.randn(B, C, generator=g).cuda()
    w = (torch.randn(C, C, generator=g) / 16).cuda()
    x = torch.randn(B, L, C, generator=g).cuda()
    dattn = (torch.randn(B, L, generator=g) * 0.1).cuda()
    lengths = torch.tensor([L, max(1, L // 2), max(1, L - 1)], dtype=torch.int32).cuda()
    for sname, xs in (("fixed", torch.tensor([0.011], device="cuda")), ("device", (x.abs().amax() / 448.0).clamp_min(1e-30).reshape(1))):
        tag = f"L{L}.{sname}"
        codes = empty(B, L, C, dtype=torch.uint8)
        _abi.call("wsmg_quantize_e4m3_dev", P(x), x.numel(), P(xs), P(codes), S())
        emit(f"attn_fp8.{tag}.codes", codes)
        qf, out, attn = empty(B, C), empty(B, C), empty(B, L)
        _abi.call("wsmg_attn_fp8_row_fwd", P(q), P(w), P(codes), P(xs), P(lengths), SCALE, B, L, C, P(qf), P(out), P(attn), S())
        for n, t in (("qf", qf), ("out", out), ("attn", attn)):
            emit(f"attn_fp8_row_fwd.{tag}.{n}", t)
        qf2 = A._fp8_fold(q, w, False)
        ws, ticket = A._fp8_scratch(B, L, q.device)
        out2, attn2 = empty(B, C), empty(B, L)
        _abi.call("wsmg_attn_fp8_fwd", P(qf2), P(codes), P(xs), P(lengths), SCALE, B, L, C, P(out2), P(attn2), P(ws), P(ticket), S())
        for n, t in (("qf", qf2), ("out", out2), ("attn", attn2)):
            emit(f"attn_fp8_fwd.{tag}.{n}", t)
        for gname, ga in (("dattn", dattn), ("null", None)):
            dqf, dx = empty(B, C), empty(B, L, C)
            _abi.call("wsmg_attn_fp8_bwd", P(qf), P(codes), P(xs), P(attn), P(dout), P(ga), SCALE, B, L, C, P(dqf), P(dx), S())
            emit(f"attn_fp8_bwd.{tag}.{gname}.dqf", dqf)
            emit(f"attn_fp8_bwd.{tag}.{gname}.dx", dx)
            emit(f"attn_fp8_fold.{tag}.{gname}.dq", A._fp8_fold(dqf, w, True))


def fp8_shared(L):
    """wsmg_attn_fp8_prep + wsmg_attn_fp8_mfma_fwd, wsmg_attn_fp8_mfma_fused, wsmg_attn_fp8_mfma_bwd at B = 5 over U = 2"""
    B, U = 5, 2
    g = gen(4, L)
    q, dout = torch.randn(B, C, generator=g).cuda(), torch.randn(B, C, generator=g).cuda()
    ks, vs = torch.randn(U, L, C, generator=g).cuda(), torch.randn(U, L, C, generator=g).cuda()
    dattn = (torch.randn(B, L, generator=g) * 0.1).cuda()
    inverse = torch.tensor([1, 0, 1, 1, 0]).cuda()
    lengths = torch.tensor([L, max(1, L - 3)], dtype=torch.int32).cuda()
    for sname, scales in (("fixed", (0.012, 0.011, 0.013)), ("device", None)):
        tag = f"L{L}.{sname}"
        args = A._fp8_shared_args(q, ks, vs, lengths, inverse, scales)
        out, attn, saved = A._fp8_shared_staged(*args, SCALE)
        for n, t in zip(("out", "attn", "q_codes", "k_codes", "v_codes", "scales", "set_start"), (out, attn) + saved[:4] + saved[5:]):
            emit(f"attn_fp8_mfma_fwd.{tag}.{n}", t)
        # (row_ids orders the rows inside a set arbitrarily: listed sorted per set)
        start = saved[5].tolist()
        emit(f"attn_fp8_mfma_fwd.{tag}.row_ids", torch.cat([saved[4][a:b].sort().values for a, b in zip(start, start[1:])]))
        fo, fa = A._attention_fp8_shared_nograd(q, ks, vs, lengths, inverse, SCALE, scales)
        assert A.last_fp8_shared_launches == 1
        emit(f"attn_fp8_mfma_fused.{tag}.out", fo)
        emit(f"attn_fp8_mfma_fused.{tag}.attn", fa)
        qc, kc, vc, sc, order, start_t = saved
        for gname, go, ga in (("both", dout, dattn), ("dout", dout, None), ("dattn", None, dattn)):
            dq, dk, dv, dl = empty(B, C), empty(U, L, C), empty(U, L, C), empty(B, L)
            _abi.call("wsmg_attn_fp8_mfma_bwd", P(qc), P(sc[0:1]), P(kc), P(sc[1:2]), P(vc), P(sc[2:3]), P(order), P(start_t), P(args[4]), P(attn),
                      P(go), P(ga), SCALE, B, U, L, C, P(dq), P(dk), P(dv), P(dl), S())
            for n, t in (("dq", dq), ("dk", dk), ("dv", dv), ("dl", dl)):
                emit(f"attn_fp8_mfma_bwd.{tag}.{gname}.{n}", t)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    for I in COUNTS:
        for dtype in (torch.float32, torch.bfloat16):
            single_query(I, dtype)
    for n in (4, 1028):
        quantise(n)
    for L in F8_COUNTS:
        fp8_rows(L)
        fp8_shared(L)
    torch.cuda.synchronize()
    text = "\n".join(LINES)
    print(text)
    print(f"# {len(LINES)} tensors, sha256 of all lines: {hashlib.sha256(text.encode()).hexdigest()}")
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
