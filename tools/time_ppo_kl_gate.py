#!/usr/bin/env python3
"""GPU-box tool: what the KL gate of `wsmgmap.ppo.PPO(target_kl=...)` costs when it never closes.

    python3 tools/time_ppo_kl_gate.py [--rounds 9] [--out FILE]

(a) one `PPO.update` (ppo_epoch 2 x 2 minibatches) on the tests' T = 4 policy with target_kl=None against target_kl=inf: the same
    steps, to the bit (tests/test_gpu_ppo_kl.py); the gated arm drops the per-minibatch `torch.stack` + add of the five figures and
    adds the BatchNorm snapshot and its guarded restore (`guard_buffers`), which an early stop needs.  Device launches per update are
    counted with torch.profiler where it works.
(b) `ops.ppo_loss` forward at B = 512, ungated against gated (limit inf), 200 calls between two HIP events.

tools/time_ppo_update.py's method: the arms interleaved round by round, host-paced, between HIP events; median, minimum and maximum
over the rounds.  Run it in two processes and keep both."""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "ws-mgmap_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)
import torch  # noqa: E402

from time_ppo_update import rounds_of  # noqa: E402


def launches(fn):
    """Device kernels one call of fn launches, or None where the profiler gives no device events."""
    try:
        from torch.profiler import ProfilerActivity, profile
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        n = sum(1 for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA and "emcpy" not in e.name
                and "emset" not in e.name)
        return n or None
    except Exception:       # noqa: BLE001  (a box without the tracer: the times below do not depend on it)
        return None


def report(lines, arms, times, unit):
    for name, _ in arms:
        t = times[name]
        lines.append(f"  {name:24s}  median {statistics.median(t):10.2f}   min {min(t):10.2f}   max {max(t):10.2f}   {unit}")


def update_part(a, lines):
    import ppo_util as pu
    from wsmgmap.ppo import PPO
    hyper = dict(clip_param=0.2, ppo_epoch=2, num_mini_batch=2, value_loss_coef=0.5, entropy_coef=0.01)
    fused, _ = pu.policy_storages()
    agents = {name: PPO(pu.build_policy(), lr=2.5e-4, eps=1e-5, max_grad_norm=0.5, target_kl=t, **hyper)
              for name, t in (("target_kl=None", None), ("target_kl=inf", float("inf")))}
    arms = tuple((name, (lambda ag=ag: ag.update(fused))) for name, ag in agents.items())
    for _, fn in arms:
        fn()
    torch.cuda.synchronize()
    times = rounds_of(arms, a.rounds, 1)
    lines.append("(a) one PPO.update of the tests' T = 4 policy, N = 4, ppo_epoch 2 x 2 minibatches, us per update")
    report(lines, arms, times, "us")
    counts = {name: launches(fn) for name, fn in arms}
    lines.append("  device kernels per update (torch.profiler): " + ", ".join(f"{k} {v if v is not None else 'not counted'}"
                                                                              for k, v in counts.items()))


def loss_part(a, lines):
    from wsmgmap import ops
    B, calls = 512, 200
    g = torch.Generator(device="cuda"); g.manual_seed(5)
    rows = [torch.randn(B, device="cuda", generator=g) for _ in range(6)]
    ent = torch.randn(1, device="cuda", generator=g)
    gate, sums = torch.zeros(ops.KL_GATE, device="cuda"), torch.zeros(5, device="cuda")

    def run(**kw):
        with torch.no_grad():
            for _ in range(calls):
                ops.ppo_loss(rows[0], rows[1], rows[2], rows[3], rows[4], rows[5], ent, 0.2, 0.5, 0.01, **kw)

    arms = (("ppo_loss", run), ("ppo_loss gated", lambda: run(gate=gate, sums=sums, kl_limit=float("inf"))))
    for _, fn in arms:
        fn()
    torch.cuda.synchronize()
    times = rounds_of(arms, a.rounds, calls)
    lines.append(f"(b) ops.ppo_loss forward at B = {B}, {calls} calls between the events (host-paced: launch and Python included), us per call")
    report(lines, arms, times, "us")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lines = [f"{a.rounds} interleaved rounds between HIP events (host-paced); pid {os.getpid()}"]
    update_part(a, lines)
    loss_part(a, lines)
    text = "\n".join(lines)
    print(text)
    if a.out:
        with open(a.out, "a") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
