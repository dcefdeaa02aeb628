#!/usr/bin/env python3
"""GPU-box tool: the entry points of csrc/wsmg_norm.hip at the shapes one bench update calls them with.

    python3 tools/time_norm.py --record FILE        one update of bench.py's workload with wsmgmap._abi.call wrapped: every distinct
                                                    (entry point, rows, C, ReLU, residual, kept y, dy stride, slabs) and its count -> FILE
    python3 tools/time_norm.py --shapes FILE        each of them alone: median microseconds per call over --rounds rounds of --calls
                                                    calls between HIP events      (WSMG_LIB=<other build>/libwsmgmap.so for the other side)

Under `rocprofv3 --kernel-trace --stats` the second form gives the kernels' own durations.  Inputs are uniform random numbers, outputs
are not looked at: tools/norm_bits.py and the tests do that."""
import argparse
import ctypes
import json
import os
import runpy
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "ws-mgmap_amd"))
import torch  # noqa: E402

from wsmgmap import _abi  # noqa: E402


def describe(name, a):
    """The arguments of a wsmg_norm.hip entry point that decide what its kernels do, or None for any other entry point."""
    has = lambda i: a[i] is not None      # noqa: E731
    if name == "wsmg_bn_act_fwd_bf16_pre":
        return dict(rows=a[9], C=a[10], relu=a[8], res=has(1), nslab=a[15])
    if name in ("wsmg_bn_act_fwd", "wsmg_bn_act_fwd_bf16"):
        return dict(rows=a[10], C=a[11], relu=a[9], res=has(1), train=a[8])
    if name in ("wsmg_bn_act_bwd_ld", "wsmg_bn_act_bwd_ld_bf16"):
        return dict(rows=a[9], C=a[10], relu=a[8], res=has(12), kept=has(3), ld=a[1])
    if name == "wsmg_bn_act_bwd_ld_bf16_lo":
        return dict(rows=a[9], C=a[10], relu=a[8], res=has(13), kept=has(3), ld=a[1])
    if name == "wsmg_bn_stats_finalize":
        return dict(rows=a[3], C=a[2], nslab=a[1])
    if name == "wsmg_bn_bwd_apply_bf16":
        return dict(rows=a[7], C=a[8])
    if name in ("wsmg_channel_sum", "wsmg_channel_sum_bf16"):
        return dict(rows=a[1], C=a[2])
    return None


def record(path):
    seen, real = {}, _abi.call

    def wrapped(name, *a):
        d = describe(name, a)
        if d is not None:
            key = json.dumps(dict(entry=name, **d), sort_keys=True)
            seen[key] = seen.get(key, 0) + 1
        return real(name, *a)
    _abi.call = wrapped
    sys.argv = ["bench.py", "--gpus", "1", "--steps", "1", "--warmup", "0", "--no-cpu-baseline", "--no-f32", "--no-other-configs", "--prewarm-s", "0"]
    try:
        runpy.run_path(os.path.join(ROOT, "bench.py"), run_name="__main__")
    except SystemExit:
        pass
    with open(path, "w") as f:
        for key, n in sorted(seen.items()):
            f.write(json.dumps(dict(json.loads(key), calls_seen=n), sort_keys=True) + "\n")
    print(f"{len(seen)} distinct calls -> {path}")


def P(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def closure(s):
    """A function that makes the call s describes once, on buffers allocated here."""
    L, entry, rows, C = _abi.lib(), s["entry"], s["rows"], s["C"]
    dt = torch.bfloat16 if ("bf16" in entry) else torch.float32
    g = torch.Generator().manual_seed(7)
    act = lambda cols=C: (torch.rand(rows, cols, generator=g) * 4 - 2).to(dt).cuda()      # noqa: E731
    vec = lambda: (torch.rand(C, generator=g) * 0.5 + 0.5).cuda()                        # noqa: E731
    x, out, out2, out3 = act(), act(), act(), act()
    gamma, beta, mean, invstd, rm, rv, v1, v2 = (vec() for _ in range(8))
    ws = torch.empty(max(int(L.wsmg_channel_reduce_workspace_bytes(rows, C)) // 8, 1), dtype=torch.float64, device="cuda")
    st = lambda: ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)                # noqa: E731
    res = act() if s.get("res") else None
    if entry == "wsmg_bn_act_fwd_bf16_pre":
        slabs = torch.zeros(s["nslab"], 2, C, dtype=torch.float64, device="cuda")

        def call():      # the slabs come back zeroed, and zeros take as long to reduce as any sums
            return L.wsmg_bn_act_fwd_bf16_pre(P(x), P(res), P(gamma), P(beta), P(rm), P(rv), 0.1, 1e-5, s["relu"], rows, C, P(out), P(mean),
                                              P(invstd), P(slabs), s["nslab"], st())
    elif entry.startswith("wsmg_bn_act_fwd"):
        def call():
            return getattr(L, entry)(P(x), P(res), P(gamma), P(beta), P(rm), P(rv), 0.1, 1e-5, s["train"], s["relu"], rows, C, P(out), P(mean),
                                     P(invstd), P(ws), ws.numel() * 8, st())
    elif entry.startswith("wsmg_bn_act_bwd_ld"):
        wide = act(s["ld"])
        kept = act() if s["kept"] else None
        lo = (P(out3),) if entry.endswith("_lo") else ()

        def call():
            return getattr(L, entry)(P(wide), s["ld"], P(x), P(kept), P(gamma), P(beta), P(mean), P(invstd), s["relu"], rows, C, P(out), *lo,
                                     P(out2) if s["res"] else None, P(v1), P(v2), P(ws), ws.numel() * 8, st())
    elif entry == "wsmg_bn_stats_finalize":
        slabs = torch.zeros(s["nslab"], 2, C, dtype=torch.float64, device="cuda")

        def call():
            return L.wsmg_bn_stats_finalize(P(slabs), s["nslab"], C, rows, 0.1, 1e-5, P(rm), P(rv), P(mean), P(invstd), st())
    elif entry == "wsmg_bn_bwd_apply_bf16":
        def call():
            return L.wsmg_bn_bwd_apply_bf16(P(out2), P(x), P(gamma), P(mean), P(invstd), P(v1), P(v2), rows, C, P(out), st())
    else:
        def call():
            return getattr(L, entry)(P(x), rows, C, P(v1), P(ws), ws.numel() * 8, st())
    return call


def time_shapes(path, rounds, calls):
    shapes = [json.loads(line) for line in open(path)]
    for s in shapes:
        call = closure(s)
        assert call() == 0, s
        torch.cuda.synchronize()
        us = []
        for _ in range(rounds):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(calls):
                call()
            b.record()
            torch.cuda.synchronize()
            us.append(a.elapsed_time(b) * 1000.0 / calls)
        print(json.dumps(dict(s, us_median=round(statistics.median(us), 2), us_min=round(min(us), 2), us_max=round(max(us), 2)), sort_keys=True))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--record", default=None)
    ap.add_argument("--shapes", default=None)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--calls", type=int, default=20)
    a = ap.parse_args()
    if a.record:
        record(a.record)
    if a.shapes:
        time_shapes(a.shapes, a.rounds, a.calls)
