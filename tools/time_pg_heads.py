#!/usr/bin/env python3
"""GPU-box tool: the policy-gradient heads + PPO loss, forward + backward, fused against the stock-torch composition.

    python3 tools/time_pg_heads.py [--rounds 7] [--calls 50] [--out FILE]

Both arms evaluate the same arithmetic on the same inputs at B = 512, K = 512, A = 2 (the update's row count): critic, diagonal
Gaussian log-probability and entropy, the clipped-surrogate loss, and the backward down to the features and the five head
parameters.  fused: ops.eval_heads + ops.ppo_loss (4 launches and the seed of autograd); stock: DiagGaussian + CriticHead + the
loss written in torch operators, clip fraction and approximate KL included.  The arms are interleaved round by round; a round
is `calls` forward + backward passes between two HIP events, host-paced (neither arm is captured into a graph).  Prints the
median, minimum and maximum per arm over the rounds."""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "ws-mgmap_amd"))
import torch  # noqa: E402

from wsmgmap import ops  # noqa: E402
from wsmgmap.common.distributions import DiagGaussian  # noqa: E402
from wsmgmap.models.policy import CriticHead  # noqa: E402

B, K, A = 512, 512, 2
CLIP, VALUE_COEF, ENTROPY_COEF = 0.2, 0.5, 0.01


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    torch.manual_seed(0)
    dev = "cuda"
    x = torch.randn(B, K, device=dev, requires_grad=True)
    ad, critic = DiagGaussian(K, A).to(dev), CriticHead(K).to(dev)
    with torch.no_grad():
        ad.logstd._bias.uniform_(-0.5, 0.5)
        action = ad(x).sample()
        old_logp = ad(x).log_probs(action) + 0.2 * torch.randn(B, device=dev)
        old_value = critic(x).view(-1) + 0.3 * torch.randn(B, device=dev)
    adv, ret = torch.randn(B, device=dev), torch.randn(B, device=dev)
    params = [x, ad.fc_mean.weight, ad.fc_mean.bias, ad.logstd._bias, critic.fc.weight, critic.fc.bias]

    def fused():
        value, logp, entropy = ops.eval_heads(x, ad.fc_mean, ad.logstd._bias, critic.fc, action)
        out = ops.ppo_loss(logp, old_logp, adv, value, old_value, ret, entropy, CLIP, VALUE_COEF, ENTROPY_COEF)
        return out[0], out[3], out[4]

    def stock():
        dist = ad(x)
        value = critic(x).view(-1)
        logp = dist.log_probs(action)
        entropy = dist.entropy().mean()
        ratio = torch.exp(logp - old_logp)
        action_loss = -torch.min(ratio * adv, torch.clamp(ratio, 1.0 - CLIP, 1.0 + CLIP) * adv).mean()
        vc = old_value + (value - old_value).clamp(-CLIP, CLIP)
        value_loss = 0.5 * torch.max((value - ret).pow(2), (vc - ret).pow(2)).mean()
        with torch.no_grad():      # the two diagnostics the fused forward also writes
            clip_frac = ((ratio - 1.0).abs() > CLIP).float().mean()
            approx_kl = (old_logp - logp).mean()
        return value_loss * VALUE_COEF + action_loss - entropy * ENTROPY_COEF, clip_frac, approx_kl

    def step(fn):
        for p in params:
            p.grad = None
        loss, clip_frac, approx_kl = fn()
        loss.backward()
        return loss

    lf = float(step(fused).detach())
    gf = [p.grad.clone() for p in params]
    ls = float(step(stock).detach())
    worst = max(float((g - p.grad).abs().max()) / (float(p.grad.abs().max()) + 1e-30) for g, p in zip(gf, params))
    for fn in (fused, stock):
        for _ in range(10):
            step(fn)
    torch.cuda.synchronize()
    times = {"fused": [], "stock": []}
    for _ in range(a.rounds):
        for name, fn in (("fused", fused), ("stock", stock)):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.calls):
                step(fn)
            e1.record()
            torch.cuda.synchronize()
            times[name].append(e0.elapsed_time(e1) * 1e3 / a.calls)
    lines = [f"policy-gradient heads + PPO loss, forward + backward, B = {B}, K = {K}, A = {A}; {a.rounds} interleaved rounds of {a.calls} calls, "
             "us per call between HIP events (host-paced)",
             f"  loss: fused {lf:.7f}  stock {ls:.7f};  worst gradient difference / max |gradient| over the six tensors: {worst:.2e}"]
    for name in ("fused", "stock"):
        t = times[name]
        lines.append(f"  {name:5s}  median {statistics.median(t):8.1f}   min {min(t):8.1f}   max {max(t):8.1f}")
    text = "\n".join(lines)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
