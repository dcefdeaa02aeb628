#!/usr/bin/env python3
"""GPU-box tool: what one rollout step pays to get its ego map into the trajectory cache's sparse form, two routes in one process —

    host    the dense float32 map to the host (`.cpu()`, as the trainer's hook does), `astype(float16)`, `codec.sparse_pack_ego`
    device  `SparseEgoRecorder.append`: packed by wsmg_ego_sparse_pack, then the presence bits, the offsets and the non-zero values only

on maps the rollout path produces (frozen RGB encoder -> BEV operator -> global map -> retrieval) from synthetic RGB-D frames at
BASELINE configs[0]'s sizes, B environments walking for a few steps so that the global map fills.  Per step: wall time around the
whole route, HIP events around its device work (the copy; the kernels and the copies), bytes that crossed PCIe, the non-zero share.
`--reps` interleaved repetitions (host, device, host, ...), medians over all steps.  Both routes are checked to give the same arrays.

    python3 tools/bench_sparse_pack.py [--B 8] [--steps 12] [--reps 5] [--out FILE]
"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "ws-mgmap_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np
import torch

from bench_act_helpers import _Box, obs_of
from wsmgmap.config import default_model_config
from wsmgmap.data import SparseEgoRecorder, sparse_pack_ego
from wsmgmap.models.policy import BasePolicy


def rollout_maps(B, steps, seed=0):
    """`steps` consecutive `observations['rgb_ego_map']` tensors [B, 64, E, E] of B environments (fresh frames, a short walk)."""
    gen = torch.Generator(device="cuda")
    gen.manual_seed(seed)
    torch.manual_seed(seed)
    pol = BasePolicy(None, _Box(), default_model_config(num_proc=B, compute_dtype="bf16")).cuda().eval()
    maps = []
    gps = (torch.rand(B, 2, device="cuda", generator=gen) - 0.5) * 2
    compass = (torch.rand(B, 1, device="cuda", generator=gen) - 0.5) * 6.28
    with torch.no_grad():
        for t in range(steps):
            obs = obs_of(B, 256, gen)
            gps = gps + (torch.rand(B, 2, device="cuda", generator=gen) - 0.5) * 0.5
            compass = compass + (torch.rand(B, 1, device="cuda", generator=gen) - 0.5) * 0.5
            obs["gps"], obs["compass"] = gps, compass
            masks = torch.full((B, 1), 0.0 if t == 0 else 1.0, device="cuda")
            _, proj = pol.net.rgb_encoder(obs)
            pol.net.rgb_mapping_module(proj, obs, masks)
            maps.append(obs["rgb_ego_map"].float().clone(memory_format=torch.preserve_format))
    torch.cuda.synchronize()
    return maps


def host_route(ego):
    """-> (sparse arrays of the step's B rows, ms of device work, ms of wall time by stage)."""
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0 = time.perf_counter()
    s.record()
    o = ego.cpu()
    e.record()
    t1 = time.perf_counter()
    h = o.numpy().astype(np.float16)
    t2 = time.perf_counter()
    arrays = sparse_pack_ego(h)
    t3 = time.perf_counter()
    e.synchronize()
    return arrays, s.elapsed_time(e), ((t1 - t0) * 1e3, (t2 - t1) * 1e3, (t3 - t2) * 1e3)


def device_route(rec, ego):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0 = time.perf_counter()
    s.record()
    rec.append(ego)
    e.record()
    t1 = time.perf_counter()
    e.synchronize()
    return s.elapsed_time(e), (t1 - t0) * 1e3


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--B", type=int, default=8)
    ap.add_argument("--steps", type=int, default=12)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_sparse_pack.py measures on the GPU: no device here")
    maps = rollout_maps(a.B, a.steps)
    B, C, E, _ = maps[0].shape
    assert maps[0].permute(0, 2, 3, 1).is_contiguous(), "the rollout's ego map is channels-last in memory"
    rec = SparseEgoRecorder(B, "cuda")
    for ego in maps[:2]:                         # warm both routes: code objects, pinned staging, NumPy's buffers
        host_route(ego)
        device_route(rec, ego)
    for i in range(B):
        rec.reset(i)
    host_wall, host_dev, host_stage, dev_wall, dev_dev, rep_lines = [], [], [], [], [], []
    share, dev_bytes = [], []
    for r in range(a.reps):
        hw, dw = [], []
        for t, ego in enumerate(maps):
            arrays, ms_dev, stages = host_route(ego)
            hw.append(sum(stages)); host_dev.append(ms_dev); host_stage.append(stages)
            if r == 0:
                share.append(float(arrays["rgb_ego_map__base"][-1]) / ego.numel())
        for t, ego in enumerate(maps):
            before = rec.bytes_to_host
            ms_dev, ms_wall = device_route(rec, ego)
            dw.append(ms_wall); dev_dev.append(ms_dev)
            if r == 0:
                dev_bytes.append(rec.bytes_to_host - before)
        if r == 0:                               # the two routes agree: environment 0's steps against the host codec
            want = sparse_pack_ego(np.stack([m[0].cpu().numpy().astype(np.float16) for m in maps]))
            got = rec.take(0)
            assert all(got[k].tobytes() == want[k].tobytes() for k in want), "device and host routes differ"
        for i in range(B):
            rec.reset(i)
        host_wall += hw; dev_wall += dw
        rep_lines.append(f"  repetition {r}: host route {statistics.median(hw):.3f} ms, device route {statistics.median(dw):.3f} ms (medians of {len(maps)} steps)")
    med = statistics.median
    dense_bytes = B * C * E * E * 4
    lines = [
        f"ego map -> sparse cache form, per rollout step: B = {B}, C = {C}, E = {E}; {len(maps)} rollout maps x {a.reps} interleaved repetitions",
        f"non-zero share of the float16 map: median {med(share):.3f} (min {min(share):.3f}, max {max(share):.3f} over the walk)",
        f"host route   (.cpu() float32 -> astype(float16) -> sparse_pack_ego): wall median {med(host_wall):.3f} ms per step "
        f"(copy {med(s[0] for s in host_stage):.3f}, cast {med(s[1] for s in host_stage):.3f}, pack {med(s[2] for s in host_stage):.3f}); "
        f"device work (the copy, HIP events) {med(host_dev):.3f} ms; {dense_bytes / 1e6:.2f} MB over PCIe per step",
        f"device route (SparseEgoRecorder.append): wall median {med(dev_wall):.3f} ms per step; device work (3 kernels + copies, HIP "
        f"events, includes the host's wait for the counters) {med(dev_dev):.3f} ms; {med(dev_bytes) / 1e6:.2f} MB over PCIe per step "
        f"(min {min(dev_bytes) / 1e6:.2f}, max {max(dev_bytes) / 1e6:.2f})",
        f"ratio device / host: wall {med(dev_wall) / med(host_wall):.3f}, PCIe bytes {med(dev_bytes) / dense_bytes:.3f}",
        f"of the host route, what the rollout pays today without the offline recode (copy + cast): {med(s[0] + s[1] for s in host_stage):.3f} ms",
    ] + rep_lines
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
