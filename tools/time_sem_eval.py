#!/usr/bin/env python3
"""GPU-box tool: what scoring the semantic-map head costs per update at the bench shape — `SemanticMapMeter.update` (one kernel
launch + the mask's compare) against the stock route on the same tensors (`to_nchw` + `argmax` + `F.interpolate` + `bincount`) —
the two arms interleaved, HIP events around blocks of calls, medians over the rounds; and that the two arms count the same matrix.

    python3 tools/time_sem_eval.py [--B 512] [--rounds 7] [--calls 50] [--out FILE]
"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "ws-mgmap_amd"))
import torch
import torch.nn.functional as F

from wsmgmap import ops
from wsmgmap.metrics import SemanticMapMeter

CLASSES, SIDE, E = 27, 48, 100


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=512)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    B = a.B
    g = torch.Generator(device="cuda").manual_seed(0)
    logits = torch.randn(B, SIDE, SIDE, 32, device="cuda", generator=g).bfloat16()
    gt = torch.randint(0, CLASSES, (B, E, E), device="cuda", generator=g).float()
    weights = torch.ones(B, 1, device="cuda")
    weights[-1] = 0.0

    class Net:
        sem_logits_nhwc = logits
    obs = {"gt_semantic_map": gt}
    meter = SemanticMapMeter()
    stock_conf = torch.zeros(CLASSES * CLASSES, device="cuda", dtype=torch.int64)

    def kernel_arm():
        meter.update(Net, obs, weights)

    def stock_arm():
        pred = ops.to_nchw(logits, CLASSES).argmax(1)                                    # what `pred_sem_map` would be scored from
        label = F.interpolate(gt.unsqueeze(1), size=(SIDE, SIDE)).squeeze(1).long()
        on = (weights > 0).view(-1, 1, 1).expand_as(label)
        stock_conf.add_(torch.bincount((label * CLASSES + pred)[on], minlength=CLASSES * CLASSES))

    arms = {"meter.update (wsmg_sem_confusion_bf16)": kernel_arm, "stock (to_nchw + argmax + interpolate + bincount)": stock_arm}
    for fn in arms.values():
        for _ in range(5):
            fn()
    torch.cuda.synchronize()
    meter.reset()
    stock_conf.zero_()
    per = {k: [] for k in arms}
    for _ in range(a.rounds):
        for name, fn in arms.items():                                                    # interleaved: one block of each per round
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            for _ in range(a.calls):
                fn()
            e.record()
            e.synchronize()
            per[name].append(s.elapsed_time(e) * 1e3 / a.calls)
    same = bool(torch.equal(meter.confusion.view(-1), stock_conf))
    mb = (logits.numel() * 2 + B * SIDE * SIDE * 4) / 1e6
    lines = [f"semantic-map scoring per call, B = {B}: logits [{B}, {SIDE}, {SIDE}, 32] bf16, ground truth [{B}, {E}, {E}] float32, "
             f"one row masked out; {a.rounds} interleaved rounds of {a.calls} calls between HIP events (host-paced where launches dominate)"]
    for name, v in per.items():
        lines.append(f"  {name:58s} median {statistics.median(v):8.1f} us  [min {min(v):.1f}, max {max(v):.1f}]")
    lines.append(f"  bytes the kernel must read: {mb:.1f} MB (logits + the gathered labels)")
    lines.append(f"  both arms count the same matrix over the timed calls: {same} ({int(meter.confusion.sum())} pixels)")
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")
    return 0 if same else 1


if __name__ == "__main__":
    sys.exit(main())
