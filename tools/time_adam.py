#!/usr/bin/env python3
"""GPU-box tool: one optimizer step over the policy's live parameters (102 tensors), GPU time between HIP events and host time
per step, arms interleaved over --rounds rounds of --steps steps:

    torch-foreach, torch-fused   torch.optim.Adam (multi-tensor default / fused=True)
    wsmg                         wsmgmap.optim.Adam, the unguarded step (3 launches)
    wsmg-dev                     wsmgmap.optim.Adam(capturable=True): the step count on the device (the form a HIP graph captures)
    wsmg-dev-hyper               the same with hyper_on_device=True: lr, betas, eps, weight_decay read from the device record
    wsmg-guarded-hyper           wsmg-guarded with hyper_on_device=True (max_grad_norm read from the record too)
    wsmg-guarded                 wsmgmap.optim.Adam(max_grad_norm=..., skip_nonfinite=True): norm launches + finalize + guarded step
    wsmg-guarded-buffers         the same with guard_buffers=policy: snapshot_buffers() (what zero_grad() adds) + the step with the
                                 conditional roll-back of the BatchNorm statistics behind it (steps taken: the roll-back returns at once)
    wsmg-guarded-report          wsmg-guarded with grad_report=True: the per-tensor report and its latch behind the norm (steps taken:
                                 the latch's launch returns at once)
    clip+wsmg                    torch.nn.utils.clip_grad_norm_ in front of the unguarded step (what the guard replaces)
    wsmg-amsgrad                 wsmgmap.optim.Adam(amsgrad=True): a fifth array, max_exp_avg_sq, read and written (nine streamed arrays
                                 against seven)
    wsmg-adamw-amsgrad           wsmgmap.optim.AdamW(amsgrad=True, weight_decay=1e-2): the same with the decoupled decay
    wsmg-maximize                wsmgmap.optim.Adam(maximize=True): the plain step's arrays through the kernels that take the options

WSMG_LIB=<another build of libwsmgmap.so> times that library's unguarded step (an older build has no guarded arm: --arms wsmg)."""
import argparse
import os, sys
import time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "ws-mgmap_amd"))
import torch
import bench
from wsmgmap.common.aux_losses import AuxLosses
from wsmgmap.config import default_model_config
from wsmgmap.models.policy import BasePolicy
from wsmgmap.optim import Adam as WsmgAdam, AdamW as WsmgAdamW
ap = argparse.ArgumentParser()
ap.add_argument("--arms", default="torch-foreach,torch-fused,wsmg,wsmg-guarded,clip+wsmg")
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--steps", type=int, default=20)
args = ap.parse_args()
T, N = 8, 8
dev = torch.device("cuda:0")
torch.manual_seed(0)
policy = BasePolicy(None, bench._Box(), default_model_config(num_proc=1, gpu_id=0, compute_dtype="bf16"))
policy.net.instruction_encoder.embedding_layer.weight.requires_grad_(False)
policy = policy.to(dev); policy.train(); policy.net.depth_encoder.eval(); policy.net.rgb_encoder.eval()
obs, prev, masks, weights = bench.synth_batch(T, N, dev, 1000)
AuxLosses.activate(); AuxLosses.clear()
o = dict(obs)
pred, aux = policy(o, torch.zeros(policy.net.num_recurrent_layers, N, 512, device=dev), prev, masks, weights)
bench.dagger_loss(pred, aux, o["waypoint"], weights).backward()
live = [p for p in policy.parameters() if p.grad is not None]
print("live parameter tensors:", len(live), "floats:", sum(p.numel() for p in live), "library:", os.environ.get("WSMG_LIB", "(built)"))
norm = float(torch.linalg.vector_norm(torch.stack([p.grad.norm() for p in live])))     # the clip arms clip at half of it
arms = {}
for name in args.arms.split(","):
    if name == "torch-foreach":
        opt = torch.optim.Adam(policy.parameters(), lr=1e-6)
    elif name == "torch-fused":
        opt = torch.optim.Adam(policy.parameters(), lr=1e-6, fused=True)
    elif name in ("wsmg", "clip+wsmg"):
        opt = WsmgAdam(policy.parameters(), lr=1e-6)
    elif name in ("wsmg-dev", "wsmg-dev-hyper"):
        opt = WsmgAdam(policy.parameters(), lr=1e-6, capturable=True, **({"hyper_on_device": True} if name.endswith("-hyper") else {}))
    elif name == "wsmg-amsgrad":
        opt = WsmgAdam(policy.parameters(), lr=1e-6, amsgrad=True)
    elif name == "wsmg-adamw-amsgrad":
        opt = WsmgAdamW(policy.parameters(), lr=1e-6, amsgrad=True, weight_decay=1e-2)
    elif name == "wsmg-maximize":
        opt = WsmgAdam(policy.parameters(), lr=1e-6, maximize=True)
    elif name == "wsmg-guarded":
        opt = WsmgAdam(policy.parameters(), lr=1e-6, max_grad_norm=0.5 * norm, skip_nonfinite=True)
    elif name == "wsmg-guarded-hyper":
        opt = WsmgAdam(policy.parameters(), lr=1e-6, max_grad_norm=0.5 * norm, skip_nonfinite=True, hyper_on_device=True)
    elif name == "wsmg-guarded-report":
        opt = WsmgAdam(policy.parameters(), lr=1e-6, max_grad_norm=0.5 * norm, skip_nonfinite=True, grad_report=True)
    elif name == "wsmg-guarded-buffers":
        opt = WsmgAdam(policy.parameters(), lr=1e-6, max_grad_norm=0.5 * norm, skip_nonfinite=True, guard_buffers=policy)
    else:
        raise SystemExit("unknown arm " + name)
    if name == "clip+wsmg":
        saved = [p.grad.clone() for p in live]

        def step(opt=opt, saved=saved):
            torch.nn.utils.clip_grad_norm_(live, 0.5 * norm)
            opt.step()
            torch._foreach_copy_([p.grad for p in live], saved)      # clip_grad_norm_ scaled them in place (this copy is timed too)
    elif name == "wsmg-guarded-buffers":
        def step(opt=opt):
            opt.snapshot_buffers()
            opt.step()
    else:
        step = opt.step
    for _ in range(3): step()
    arms[name] = step
torch.cuda.synchronize()
for r in range(args.rounds):
    for name, step in arms.items():
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        t0 = time.perf_counter()
        for _ in range(args.steps): step()
        host = time.perf_counter() - t0
        b.record(); torch.cuda.synchronize()
        print(f"round {r} Adam {name}: {a.elapsed_time(b) / args.steps * 1e3:.0f} us per step between events, "
              f"host {host / args.steps * 1e6:.0f} us per step")
