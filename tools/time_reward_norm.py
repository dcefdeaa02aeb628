#!/usr/bin/env python3
"""GPU-box tool: what normalising a rollout's rewards costs in front of its returns and advantages.

    python3 tools/time_reward_norm.py [--rounds 7] [--calls 20] [--out FILE]

Three arms on the same inserted data at (T, N) = (64, 8) (the bench's shape) and (128, 64), GAE, gamma 0.99, tau 0.95:
  fused   ops.normalized_gae_returns: normaliser + returns + advantages, ONE launch (wsmg_gae_returns_normalized)
  parent  ops.gae_returns on the raw rewards: the launch `compute_returns` was before there was a normaliser (wsmg_gae_returns)
  stock   RewardNormalizer.normalize_stock (the float64 torch loop over the steps, on the GPU) followed by that launch
The arms are interleaved round by round; a round is `calls` calls between two HIP events, host-paced.  `fused graph` / `parent graph`
are the same launches captured `calls` times into one HIP graph and replayed: per launch, no host in between.  The normaliser's
statistics keep advancing over the calls (that is its work); every arm writes into preallocated tensors.  Prints the median,
minimum and maximum per arm over the rounds, and the fused launch's added microseconds over the parent's."""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "ws-mgmap_amd"))
import torch  # noqa: E402

from wsmgmap import ops  # noqa: E402
from wsmgmap.rollout import RewardNormalizer  # noqa: E402

SHAPES = ((64, 8), (128, 64))
GAMMA, TAU = 0.99, 0.95


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lines = [f"normaliser + returns (GAE, {GAMMA}, {TAU}) + advantages; {a.rounds} interleaved rounds of {a.calls} calls, us per call between "
             "HIP events (host-paced); graph: the same launch replayed from one captured graph, us per launch"]
    for T, N in SHAPES:
        g = torch.Generator(); g.manual_seed(T * 1000 + N)
        rewards = (3.0 * torch.randn(T, N, 1, generator=g)).cuda()
        value_preds = torch.randn(T + 1, N, 1, generator=g).cuda()
        masks = (torch.rand(T + 1, N, 1, generator=g) >= 0.05).float().cuda()
        nv = torch.linspace(-1.0, 1.0, N, device="cuda").view(N, 1)
        mk = lambda *s, dt=torch.float32: torch.zeros(*s, device="cuda", dtype=dt)      # noqa: E731
        outs = {k: (mk(T + 1, N, 1), mk(T, N, 1), mk(T, N, 1), mk(2, dt=torch.float64)) for k in ("fused", "parent", "stock")}
        rnorm = {k: mk(T, N, 1) for k in ("fused", "stock")}
        nz = {k: RewardNormalizer(N, GAMMA).to("cuda") for k in ("fused", "stock")}

        def fused():
            z = nz["fused"]
            ops.normalized_gae_returns(rewards, value_preds, masks, nv, GAMMA, TAU, z.state, z.gamma, z.clip, z.eps, rewards_out=rnorm["fused"],
                                       out=outs["fused"])

        def parent():
            ops.gae_returns(rewards, value_preds, masks, nv, GAMMA, TAU, out=outs["parent"])

        def stock():
            nz["stock"].normalize_stock(rewards, masks, 0, rnorm["stock"])
            ops.gae_returns(rnorm["stock"], value_preds, masks, nv, GAMMA, TAU, out=outs["stock"])

        for fn in (fused, parent, stock):
            for _ in range(3):
                fn()
        torch.cuda.synchronize()
        graphs = {}
        for name, fn in (("fused graph", fused), ("parent graph", parent)):
            graphs[name] = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graphs[name]):
                for _ in range(a.calls):
                    fn()
        arms = (("fused", lambda: [fused() for _ in range(a.calls)]), ("parent", lambda: [parent() for _ in range(a.calls)]),
                ("stock", lambda: [stock() for _ in range(a.calls)]), ("fused graph", graphs["fused graph"].replay),
                ("parent graph", graphs["parent graph"].replay))
        times = {name: [] for name, _ in arms}
        for _ in range(a.rounds):
            for name, fn in arms:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                fn()
                e1.record()
                torch.cuda.synchronize()
                times[name].append(e0.elapsed_time(e1) * 1e3 / a.calls)
        lines.append(f"T = {T}, N = {N}: statistics after the run: fused count {float(nz['fused'].count):.4f} var {float(nz['fused'].var):.6f}; "
                     f"stock count {float(nz['stock'].count):.4f} var {float(nz['stock'].var):.6f}")
        for name, _ in arms:
            t = times[name]
            lines.append(f"  {name:12s}  median {statistics.median(t):9.1f}   min {min(t):9.1f}   max {max(t):9.1f}")
        med = {k: statistics.median(v) for k, v in times.items()}
        lines.append(f"  fused - parent: {med['fused'] - med['parent']:+.1f} us host-paced, {med['fused graph'] - med['parent graph']:+.1f} us per "
                     "replayed launch")
    text = "\n".join(lines)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
