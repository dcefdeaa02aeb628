#!/usr/bin/env python3
"""GPU-box tool: SHA-256 of the slab workspace and of the reduced OIHW dW of the SLAB form of every weight-gradient kernel on fixed
inputs — the listing two builds of the library must share when a change claims to leave the family's bits alone.

    python3 tools/wgrad_bits.py [--out FILE]                    (WSMG_LIB=<other build>/libwsmgmap.so for the other side)

Through wsmg_conv2d_bwd_weight[_bf16]_plan / _slabs / wsmg_weight_grad_reduce_oihw.  Cases are the smallest on both sides of each
plan bound, nothing of workload size:
  s2win    tests/test_gpu_round4.py test_stride2_window_weight_gradients: enc3-few, stem-few, and enc3 with more tiles than groups
  win3     test_small_channel_window_weight_gradients_3x3: w16, cls-ragged, and one case per tile variant (V421, V222, V412 at the route's
           pixel bound; V118 is w16's)
  generic  every WGRAD form of tests/test_gpu_kernel_instances.py (conv_wgrad_bf16_kernel<TC, TU, 1, UPT>)
  f32      conv_wgrad_kernel<false> (the one DB compiled): a short last split
  stem     the k8 s2 p3 stem (conv_win_wgrad_kernel), LAST: B = 2 at 100 x 100 (40 tiles, 40 groups, whole blocks), then the two with
           fewer tiles than groups: B = 1 at 100 x 100 (20 tiles, 24 groups) and B = 1 at 36 x 36 (4 tiles, 8 groups, every block
           over the right and bottom edges); --only stem.b1-36 runs the cases whose names begin so
Inputs come from oracle/detfill.py (x post-ReLU, dy zero on a band of rows).  The workspace and dW are filled with NaN before each call,
and a NaN left in either ends the run (lines are printed as they are made: what came before it stands).  The atomic form is not
bit-reproducible and is not listed.  One `name shape sha256` line per tensor; the digest is of the bytes after a copy to the host.  One
process, no children."""
import argparse
import ctypes
import hashlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "ws-mgmap_amd"), ROOT, os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)
import torch  # noqa: E402

import conv_route_util as cr  # noqa: E402
from oracle import detfill as df  # noqa: E402
from test_gpu_kernel_instances import WGRAD  # noqa: E402
from wsmgmap import _abi  # noqa: E402

LINES = []
# (name, B, Cin, Cout, k, stride, pad, H, W, route family)
S2WIN = [("s2win.enc3-few", 3, 64, 128, 5, 2, 1, 50, 50, "WGRAD_S2WIN"), ("s2win.stem-few", 2, 256, 64, 7, 2, 3, 24, 24, "WGRAD_S2WIN"),
         ("s2win.enc3-more", 17, 64, 128, 5, 2, 1, 50, 50, "WGRAD_S2WIN")]          # 51 tiles, 48 groups
WIN3 = [("win3.w16", 259, 32, 32, 3, 1, 1, 16, 16, "WGRAD_WIN3"), ("win3.cls-ragged", 33, 32, 96, 3, 1, 1, 47, 43, "WGRAD_WIN3"),
        ("win3.v421", 114, 64, 128, 3, 1, 1, 24, 24, "WGRAD_WIN3"), ("win3.v222", 114, 64, 64, 3, 1, 1, 24, 24, "WGRAD_WIN3"),
        ("win3.v412", 114, 32, 128, 3, 1, 1, 24, 24, "WGRAD_WIN3")]      # B = 114: the fewest 24 x 24 images the route sends to the window
GENERIC = [("generic." + c[0],) + c[2:] + ("WGRAD",) for c in WGRAD]
STEM = [("stem.b2-100", 2, 64, 64, 8, 2, 3, 100, 100, "WGRAD_STEM_WIN"), ("stem.b1-100", 1, 64, 64, 8, 2, 3, 100, 100, "WGRAD_STEM_WIN"),
        ("stem.b1-36", 1, 64, 64, 8, 2, 3, 36, 36, "WGRAD_STEM_WIN")]
F32 = [("f32.k3_c32", 3, 32, 64, 3, 1, 1, 13, 17, None)]


def emit(name, t):
    h = t.detach().contiguous().cpu()
    if bool(torch.isnan(h).any()):
        raise SystemExit(f"{name}: {int(torch.isnan(h).sum())} of {h.numel()} elements were left unwritten (NaN)")
    LINES.append(f"{name} {tuple(h.shape)} {hashlib.sha256(h.numpy().tobytes()).hexdigest()}")
    print(LINES[-1], flush=True)


def P(t):
    return ctypes.c_void_p(t.data_ptr())


def case(name, B, Cin, Cout, k, s, p, H, W, family):
    sfx = "" if family is None else "_bf16"
    dims = cr.dims(B, Cin, Cout, k, s, p, H, W)
    OH, OW = dims[-2:]
    x = torch.relu(torch.from_numpy(df.uniform(f"wgbits.{name}.x", (B, H, W, Cin), 4.0)))
    dy = torch.from_numpy(df.uniform(f"wgbits.{name}.dy", (B, OH, OW, Cout), 0.4)).clone()
    dy[:, OH // 2] = 0
    if family is not None:
        x, dy = x.to(torch.bfloat16), dy.to(torch.bfloat16)
        kind = cr.route(cr.BWD_WEIGHT, dims)["kind"]
        if kind != family:
            raise SystemExit(f"{name}: routed to {kind}, not {family}")
    x, dy = x.cuda(), dy.cuda()
    ns, fl = ctypes.c_int(0), ctypes.c_longlong(0)
    _abi.call("wsmg_conv2d_bwd_weight" + sfx + "_plan", *dims, ctypes.cast(ctypes.byref(ns), ctypes.c_void_p),
              ctypes.cast(ctypes.byref(fl), ctypes.c_void_p))
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    ws = torch.full((ns.value, Cout, k, k, Cin), float("nan"), device="cuda")
    assert ws.numel() == fl.value, (name, ns.value, fl.value)
    _abi.call("wsmg_conv2d_bwd_weight" + sfx + "_slabs", P(x), P(dy), P(ws), ns.value, fl.value, *dims, st)
    emit(name + ".slabs", ws)
    dw = torch.full((Cout, Cin, k, k), float("nan"), device="cuda")
    _abi.call("wsmg_weight_grad_reduce_oihw", P(ws), ns.value, Cout, Cin, k, k, Cin, P(dw), st)
    emit(name + ".dw", dw)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--only", default="")
    a = ap.parse_args()
    try:
        for c in S2WIN + WIN3 + GENERIC + F32 + STEM:
            if c[0].startswith(a.only):
                case(*c)
        torch.cuda.synchronize()
    finally:
        text = "\n".join(LINES)
        print(f"# {len(LINES)} tensors, sha256 of all lines: {hashlib.sha256(text.encode()).hexdigest()}")
        if a.out:
            with open(a.out, "w") as f:
                f.write(text + "\n")


if __name__ == "__main__":
    main()
