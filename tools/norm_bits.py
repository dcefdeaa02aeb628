#!/usr/bin/env python3
"""GPU-box tool: SHA-256 of every output of every entry point of csrc/wsmg_norm.hip on fixed inputs — the listing two builds of the
library must share when a change claims to leave their bits alone.

    python3 tools/norm_bits.py [--out FILE]                    (WSMG_LIB=<other build>/libwsmgmap.so for the other side)

Shapes are those of tests/norm_cases.py, the smallest on both sides of each loop bound, nothing of workload size:
  edges    edge_rows(C) at rows2, rpi+1, 8rpi+1, nblk65, nblk257 and cap, C = 32, 256, 512: residual + ReLU, train, float32 and bf16,
           backward through wsmg_bn_act_bwd[_bf16]; the channel sums of x on the same rows
  modes    MODE_SHAPES over residual x ReLU, both types: train and eval forward, backward through wsmg_bn_act_bwd_ld[_bf16] with ld = C
           and, for bf16, through wsmg_bn_act_bwd_ld_bf16_lo
  strided  STRIDED: dy a channel slice of a wider tensor, both types, with and without residual
  slabs    NSLABS 1, 64, 65, 257 at C = 32 and 256: wsmg_bn_act_fwd_bf16_pre and wsmg_bn_stats_finalize (+ wsmg_bn_bwd_apply_bf16)
  gn       GN_CG x GN_SHAPES, float32 and bf16 input, residual + ReLU and plain
Inputs come from CPU generators with fixed seeds; every output buffer is filled with NaN before its call, and a NaN left in one ends
the run.  The tensors: y, save_mean, save_invstd, both running statistics, the slabs after the call, dx, dres, dx_lo, dgamma, dbeta, the
channel sums.  One `name shape sha256`
line per tensor; the digest is of the tensor's bytes after a copy to the host.  One process, no children."""
import argparse
import ctypes
import hashlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "ws-mgmap_amd"), ROOT, os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)
import torch  # noqa: E402

import norm_cases as nc  # noqa: E402
from wsmgmap import _abi  # noqa: E402

LINES = []
NAN = float("nan")
EDGES = ["rows2", "rpi+1", "8rpi+1", "nblk65", "nblk257", "cap"]
MODES = [(False, False), (False, True), (True, False), (True, True)]        # (residual, relu)
F32, BF16 = torch.float32, torch.bfloat16


def emit(name, t):
    h = t.detach().contiguous().cpu()
    if bool(torch.isnan(h).any()):
        raise SystemExit(f"{name}: an element was left unwritten (NaN)")
    if h.dtype == BF16:
        h = h.view(torch.int16)
    LINES.append(f"{name} {tuple(h.shape)} {hashlib.sha256(h.numpy().tobytes()).hexdigest()}")


def gen(*seed):
    g = torch.Generator()
    g.manual_seed(sum(int(s) * 1009 ** i for i, s in enumerate(seed)) + 29)
    return g


def P(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def S():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def nan(shape, dt=F32):
    return torch.full(shape, NAN, dtype=dt, device="cuda")


def sfx(dt):
    return "_bf16" if dt == BF16 else ""


def workspace(rows, C):
    return torch.empty(max(int(_abi.lib().wsmg_channel_reduce_workspace_bytes(rows, C)) // 8, 1), dtype=torch.float64, device="cuda")


def ok(rc, what):
    if rc != 0:
        raise SystemExit(f"{what}: return code {rc}")


def inputs(rows, C, dt, res, seed, wide=None):
    """x, res, dy [rows, C] of type dt (dy a slice of [rows, Ctot] for wide = (Ctot, c0)), gamma, beta, running statistics."""
    g = gen(rows, C, int(dt == BF16), int(res), seed)
    x = (torch.rand(rows, C, generator=g) * 6 - 3 + (torch.rand(1, C, generator=g) * 4 - 2)).to(dt).cuda()
    r = (torch.rand(rows, C, generator=g) * 4 - 2).to(dt).cuda() if res else None
    Ctot, c0 = wide or (C, 0)
    dyw = (torch.rand(rows, Ctot, generator=g) * 4 - 2).to(dt).cuda()
    par = dict(gamma=(torch.rand(C, generator=g) * 0.5 + 0.5).cuda(), beta=(torch.rand(C, generator=g) - 0.5).cuda(),
               rm=(torch.rand(C, generator=g) * 0.4 - 0.2).cuda(), rv=(torch.rand(C, generator=g) * 0.5 + 0.5).cuda())
    return x, r, dyw[:, c0:c0 + C], Ctot, par


def forward(name, x, r, par, dt, relu, train):
    rows, C = x.shape
    y, mean, invstd = nan((rows, C), dt), nan((C,)), nan((C,))
    rm, rv = par["rm"].clone(), par["rv"].clone()
    ws = workspace(rows, C)
    ok(getattr(_abi.lib(), "wsmg_bn_act_fwd" + sfx(dt))(P(x), P(r), P(par["gamma"]), P(par["beta"]), P(rm), P(rv), nc.MOMENTUM, nc.EPS,
                                                        int(train), int(relu), rows, C, P(y), P(mean), P(invstd), P(ws), ws.numel() * 8, S()), name)
    for n, t in (("y", y), ("save_mean", mean), ("save_invstd", invstd), ("running_mean", rm), ("running_var", rv)):
        emit(f"{name}.{n}", t)
    return y, mean, invstd


def backward(name, entry, dy, ld, x, y, r, par, mean, invstd, dt, relu):
    """entry: "" (wsmg_bn_act_bwd), "_ld", or "_ld_lo" (bf16).  y is handed over only where the forward keeps it (residual + ReLU)."""
    rows, C = x.shape
    dx, dres = nan((rows, C), dt), (nan((rows, C), dt) if r is not None else None)
    lo = nan((rows, C), dt) if entry == "_ld_lo" else None
    dg, db = nan((C,)), nan((C,))
    ws = workspace(rows, C)
    kept = y if (relu and r is not None) else None
    head = (P(dy),) + ((ld,) if entry else ()) + (P(x), P(kept), P(par["gamma"]), P(par["beta"]), P(mean), P(invstd), int(relu), rows, C, P(dx))
    tail = (P(dres), P(dg), P(db), P(ws), ws.numel() * 8, S())
    fn = {"": "wsmg_bn_act_bwd" + sfx(dt), "_ld": "wsmg_bn_act_bwd_ld" + sfx(dt), "_ld_lo": "wsmg_bn_act_bwd_ld_bf16_lo"}[entry]
    ok(getattr(_abi.lib(), fn)(*head, *((P(lo),) if lo is not None else ()), *tail), name)
    for n, t in (("dx", dx), ("dres", dres), ("dx_lo", lo), ("dgamma", dg), ("dbeta", db)):
        if t is not None:
            emit(f"{name}.{n}", t)


def channel_sum(name, x, dt):
    rows, C = x.shape
    out, ws = nan((C,)), workspace(rows, C)
    ok(getattr(_abi.lib(), "wsmg_channel_sum" + sfx(dt))(P(x), rows, C, P(out), P(ws), ws.numel() * 8, S()), name)
    emit(f"{name}.sum", out)


def edges():
    for C in (32, 256, 512):
        for edge in EDGES:
            rows = nc.edge_rows(C)[edge][0]
            for dt in (F32, BF16):
                name = f"edge.C{C}.{edge}.{'bf16' if dt == BF16 else 'f32'}"
                x, r, dy, ld, par = inputs(rows, C, dt, True, 1)
                y, mean, invstd = forward(name + ".fwd", x, r, par, dt, True, True)
                backward(name + ".bwd", "", dy, ld, x, y, r, par, mean, invstd, dt, True)
                channel_sum(name, x, dt)


def modes():
    for C, (B, H, W) in nc.MODE_SHAPES.items():
        rows = B * H * W
        for res, relu in MODES:
            for dt in (F32, BF16):
                name = f"mode.C{C}.res{int(res)}.relu{int(relu)}.{'bf16' if dt == BF16 else 'f32'}"
                x, r, dy, ld, par = inputs(rows, C, dt, res, 2)
                forward(name + ".eval", x, r, par, dt, relu, False)
                y, mean, invstd = forward(name + ".train", x, r, par, dt, relu, True)
                backward(name + ".bwd_ld", "_ld", dy, ld, x, y, r, par, mean, invstd, dt, relu)
                if dt == BF16:
                    backward(name + ".bwd_lo", "_ld_lo", dy, ld, x, y, r, par, mean, invstd, dt, relu)


def strided():
    B, H, W = nc.STRIDED_SHAPE
    for C, Ctot, c0 in nc.STRIDED:
        for res in (False, True):
            for dt in (F32, BF16):
                name = f"strided.C{C}of{Ctot}at{c0}.res{int(res)}.{'bf16' if dt == BF16 else 'f32'}"
                x, r, dy, ld, par = inputs(B * H * W, C, dt, res, 3, wide=(Ctot, c0))
                y, mean, invstd = forward(name + ".fwd", x, r, par, dt, True, True)
                backward(name + ".bwd_ld", "_ld", dy, ld, x, y, r, par, mean, invstd, dt, True)
                if dt == BF16:
                    backward(name + ".bwd_lo", "_ld_lo", dy, ld, x, y, r, par, mean, invstd, dt, True)


def slabs():
    L = _abi.lib()
    for C in (32, 256):
        B, H, W = nc.MODE_SHAPES[C]
        rows = B * H * W
        for nslab in [n for n in nc.NSLABS if n in (1, 64, 65, 257)]:
            name = f"slabs.C{C}.n{nslab}"
            x, r, dy, _, par = inputs(rows, C, BF16, True, 4)
            split = nc.slab_split(x.double().cpu(), nslab, f"normbits.{C}.{nslab}")
            for form in ("pre", "finalize"):
                st = split.cuda()
                mean, invstd, rm, rv = nan((C,)), nan((C,)), par["rm"].clone(), par["rv"].clone()
                if form == "pre":
                    y = nan((rows, C), BF16)
                    ok(L.wsmg_bn_act_fwd_bf16_pre(P(x), P(r), P(par["gamma"]), P(par["beta"]), P(rm), P(rv), nc.MOMENTUM, nc.EPS, 1, rows, C,
                                                  P(y), P(mean), P(invstd), P(st), nslab, S()), name)
                    emit(f"{name}.pre.y", y)
                else:
                    ok(L.wsmg_bn_stats_finalize(P(st), nslab, C, rows, nc.MOMENTUM, nc.EPS, P(rm), P(rv), P(mean), P(invstd), S()), name)
                    dx = nan((rows, C), BF16)
                    ok(L.wsmg_bn_bwd_apply_bf16(P(dy), P(x), P(par["gamma"]), P(mean), P(invstd), P(par["beta"]), P(par["rv"]), rows, C,
                                                P(dx), S()), name)      # any two float32 vectors serve as the supplied sums
                    emit(f"{name}.finalize.bwd_apply.dx", dx)
                if int((st != 0).sum()) or bool(torch.signbit(st).any()):
                    raise SystemExit(f"{name}.{form}: the slabs did not come back exactly 0.0")
                for n, t in (("save_mean", mean), ("save_invstd", invstd), ("running_mean", rm), ("running_var", rv), ("slabs_after", st)):
                    emit(f"{name}.{form}.{n}", t)


def group_norm():
    L = _abi.lib()
    for C, G in nc.GN_CG:
        for B, H, W in nc.GN_SHAPES:
            for dt in (F32, BF16):
                for res, relu in ((False, False), (True, True)):
                    g = gen(C, G, B, H, W, int(dt == BF16), 5)
                    x = (torch.rand(B, H, W, C, generator=g) * 6 - 3 + (torch.rand(1, 1, 1, C, generator=g) * 4 - 2)).to(dt).cuda()
                    r = (torch.rand(B, H, W, C, generator=g) * 4 - 2).to(BF16).cuda() if res else None
                    gam, bet = (torch.rand(C, generator=g) * 0.5 + 0.5).cuda(), (torch.rand(C, generator=g) - 0.5).cuda()
                    y = nan((B, H, W, C), BF16)
                    name = f"gn.C{C}G{G}.{B}x{H}x{W}.{'bf16' if dt == BF16 else 'f32'}.res{int(res)}relu{int(relu)}"
                    ok(L.wsmg_group_norm_nhwc_bf16(P(x), int(dt == F32), P(r), P(gam), P(bet), B, H * W, C, G, nc.EPS, int(relu), P(y), S()), name)
                    emit(name + ".y", y)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    for fn in (edges, modes, strided, slabs, group_norm):
        fn()
    torch.cuda.synchronize()
    text = "\n".join(LINES)
    print(text)
    print(f"# {len(LINES)} tensors, sha256 of all lines: {hashlib.sha256(text.encode()).hexdigest()}")
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
