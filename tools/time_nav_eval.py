#!/usr/bin/env python3
"""GPU-box tool: what scoring the waypoint attention, the action mean and the progress head costs per update at the bench shape —
`NavigationMeter.update` (wsmg_nav_rows + wsmg_nav_accumulate + the mask's compare) against the stock route on the same tensors
(area `F.interpolate` + `argmin` / `argmax` + the distance, mass and entropy arithmetic + `tanh` + the stop compare, already without
the reference target's `aminmax`, normalisation and softmax) —
the two arms interleaved, HIP events around blocks of calls, medians over the rounds; each launch of the meter alone; and that the
two arms agree on the integer scores.

    python3 tools/time_nav_eval.py [--B 512] [--rounds 7] [--calls 50] [--out FILE]
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
from wsmgmap.metrics import NavigationMeter

S, E, A, THR = 24, 100, 2, 0.8


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=512)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    B = a.B
    g = torch.Generator(device="cuda").manual_seed(0)
    att = torch.softmax(2.0 * torch.randn(B, S * S, device="cuda", generator=g), 1)
    # integer-valued and < 2^24 / 36: every window sum is exact in float32 in any order, and two cells hardly ever tie
    dis = torch.randint(0, 400000, (B, E, E), device="cuda", generator=g).float()
    pred = torch.randn(B, A, device="cuda", generator=g)
    waypoint = torch.rand(B, 3, device="cuda", generator=g) * 2 - 1
    prog, progress = torch.rand(B, 1, device="cuda", generator=g), torch.rand(B, 1, device="cuda", generator=g)
    weights = torch.ones(B, 1, device="cuda")
    weights[-1] = 0.0

    class Net:
        att_map_t_m = att

    class Pol:
        net = Net
    Pol.prog = prog
    obs = {"gt_path": dis, "waypoint": waypoint, "progress": progress}
    meter = NavigationMeter(stop_threshold=THR)
    stock = torch.zeros(8, device="cuda", dtype=torch.int64)          # rows, hits at 0 / 1 / 2, the stop confusion

    def meter_arm():
        meter.update(Pol, obs, pred, weights)

    def rows_arm():
        ops.nav_rows(att, dis, S, pred, waypoint, prog, progress, meter._mask, THR, out=meter.rows)

    def fold_arm():
        ops.nav_accumulate(meter.rows, meter.counts, meter.sums)

    def stock_arm():
        on = (weights > 0).view(-1)
        target = F.interpolate(dis.unsqueeze(1), size=[S, S], mode="area").reshape(B, -1).argmin(1)
        peak = att.argmax(1)
        dy, dx = (peak // S - target // S).abs(), (peak % S - target % S).abs()
        cheb = torch.maximum(dy, dx)
        cells = torch.arange(S * S, device="cuda")
        near = ((cells // S)[None] - (target // S)[:, None]).abs().le(1) & ((cells % S)[None] - (target % S)[:, None]).abs().le(1)
        mass = (att.double() * near).sum(1)[on].sum()
        entropy = (-torch.special.xlogy(att.double(), att.double())).sum(1)[on].sum()
        e = torch.tanh(pred.double()) - waypoint[:, :A].double()
        sq = (e * e).sum(1)[on].sum()
        d = (prog.double() - progress.double()).view(-1)[on]
        code = (2 * (progress >= THR).long() + (prog >= THR).long()).view(-1)[on]
        stock.add_(torch.cat([on.sum().view(1), torch.stack([(cheb[on] <= k).sum() for k in range(3)]), torch.bincount(code, minlength=4)]))
        return mass, entropy, sq, d.abs().sum(), torch.sqrt((dy * dy + dx * dx).double())[on].sum()

    arms = {"meter.update (nav_rows + nav_accumulate + mask)": meter_arm, "  ops.nav_rows alone": rows_arm,
            "  ops.nav_accumulate alone": fold_arm, "stock (interpolate + argmin / argmax + arithmetic)": stock_arm}
    for fn in arms.values():
        for _ in range(5):
            fn()
    torch.cuda.synchronize()
    meter.reset()
    stock.zero_()
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
    # the timed calls of the fold arm re-added the last record: compare one fresh update of each arm instead
    meter.reset()
    stock.zero_()
    meter_arm()
    stock_arm()
    c = meter.counts.cpu().tolist()
    N = ops.NAV_N
    mine = [c[N["att"]], c[N["hit0"]], c[N["hit0"] + 1], c[N["hit0"] + 2]] + c[N["stop"]:N["stop"] + 4]
    same = mine == stock.cpu().tolist()
    mb = (dis.numel() + att.numel() * 2 + B * (A + 3 + 2)) * 4 / 1e6 + B * ops.NAV_ROW * 8 * 2 / 1e6
    lines = [f"attention / action / progress scoring per call, B = {B}: attention [{B}, {S * S}], gt_path [{B}, {E}, {E}], pred [{B}, {A}], "
             f"one row masked out; {a.rounds} interleaved rounds of {a.calls} calls between HIP events (host-paced where launches dominate)"]
    for name, v in per.items():
        lines.append(f"  {name:58s} median {statistics.median(v):8.1f} us  [min {min(v):.1f}, max {max(v):.1f}]")
    lines.append(f"  bytes the two kernels move: {mb:.1f} MB")
    lines.append(f"  both arms agree on rows, hits at 0 / 1 / 2 and the stop confusion of one update: {same} ({mine})")
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")
    return 0 if same else 1


if __name__ == "__main__":
    sys.exit(main())
