#!/usr/bin/env python3
"""GPU-box tool: a rollout's returns and advantages, the one launch against the torch loop.

    python3 tools/time_gae_returns.py [--rounds 7] [--calls 20] [--out FILE]

Both arms are `RolloutStorage.compute_returns(next_value, use_gae=True, 0.99, 0.95)` + `get_advantages()` on the same inserted data at
(T, N) = (128, 8) (the bench's N) and (128, 64): fused = the storage's one launch (ops.gae_returns, csrc/wsmg_pg_rollout.hip), stock = a
storage built with `fused=False`, the Python loop over T of habitat-baselines' `compute_returns` in torch operators followed by the
mean / std expression.  The arms are interleaved round by round; a round is `calls` calls between two HIP events, host-paced.  A third
figure is the kernel's own time: `calls` launches captured into one HIP graph and replayed, per launch (no host in between).  Prints
the median, minimum and maximum per arm over the rounds."""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "ws-mgmap_amd"))
import torch  # noqa: E402

from wsmgmap.rollout import RolloutStorage  # noqa: E402

SHAPES = ((128, 8), (128, 64))
GAMMA, TAU = 0.99, 0.95


def storages(T, N):
    g = torch.Generator(); g.manual_seed(T * 1000 + N)
    out = [RolloutStorage(T, N, {"x": ((1,), torch.float32)}, 2, 4, fused=f).to("cuda") for f in (True, False)]
    for _ in range(T):
        row = ({"x": torch.zeros(N, 1)}, torch.zeros(1, N, 4), torch.zeros(N, 2), torch.randn(N, generator=g), torch.randn(N, 1, generator=g),
               torch.randn(N, 1, generator=g), (torch.rand(N, 1, generator=g) >= 0.05).float())
        for st in out:
            st.insert(*row)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lines = [f"compute_returns(GAE, {GAMMA}, {TAU}) + get_advantages(); {a.rounds} interleaved rounds of {a.calls} calls, us per call "
             "between HIP events (host-paced); kernel: the same launch replayed from one captured graph, us per launch"]
    for T, N in SHAPES:
        fused, stock = storages(T, N)
        nv = torch.linspace(-1.0, 1.0, N, device="cuda").view(N, 1)

        def call(st):
            st.compute_returns(nv, True, GAMMA, TAU)
            return st.get_advantages()

        af, as_ = call(fused), call(stock)
        torch.cuda.synchronize()
        same = torch.equal(fused.returns, stock.returns)
        diff = float((af - as_).abs().max())
        for st in (fused, stock):
            for _ in range(3):
                call(st)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            for _ in range(a.calls):
                call(fused)
        arms = (("fused", lambda: [call(fused) for _ in range(a.calls)]), ("stock", lambda: [call(stock) for _ in range(a.calls)]),
                ("kernel", graph.replay))
        times = {name: [] for name, _ in arms}
        for _ in range(a.rounds):
            for name, fn in arms:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                fn()
                e1.record()
                torch.cuda.synchronize()
                times[name].append(e0.elapsed_time(e1) * 1e3 / a.calls)
        lines.append(f"T = {T}, N = {N}: returns bit-identical between the arms: {same}; normalised advantages differ by at most {diff:.2e}")
        for name, _ in arms:
            t = times[name]
            lines.append(f"  {name:6s}  median {statistics.median(t):9.1f}   min {min(t):9.1f}   max {max(t):9.1f}")
    text = "\n".join(lines)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
