#!/usr/bin/env python3
"""GPU-box tool: one bf16 configs[1] update (T = 64 x N = 8, the bench's synthetic batch and optimizer) per instruction encoder
setting — the default bidirectional LSTM, GRU bidirectional 128, LSTM / GRU unidirectional 256 — timed with HIP events over
`--steps` updates after `--warmup`.  Not a bench.py leg: the bench line measures the default configuration only."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "ws-mgmap_amd"))
import torch  # noqa: E402

import bench  # noqa: E402


def leg(cell, bidir, hidden, steps, warmup, T=64, N=8):
    from wsmgmap import ops
    from wsmgmap.common.aux_losses import AuxLosses
    from wsmgmap.config import default_model_config
    from wsmgmap.models.policy import BasePolicy
    from wsmgmap.optim import Adam
    torch.manual_seed(0)
    mc = default_model_config(num_proc=1, compute_dtype="bf16")
    mc.INSTRUCTION_ENCODER.rnn_type, mc.INSTRUCTION_ENCODER.bidirectional, mc.INSTRUCTION_ENCODER.hidden_size = cell, bidir, hidden
    pol = BasePolicy(None, bench._Box(), mc)
    pol.net.instruction_encoder.embedding_layer.weight.requires_grad_(False)
    pol = pol.cuda()
    pol.train()
    pol.net.depth_encoder.eval()
    pol.net.rgb_encoder.eval()
    opt = Adam(pol.parameters(), lr=2.5e-4)
    obs, prev, masks, weights = bench.synth_batch(T, N, "cuda", 1000)
    ops.mark_inputs_ready(obs["instruction"])
    AuxLosses.activate()

    def update():
        opt.zero_grad(set_to_none=True)
        AuxLosses.clear()
        h0 = torch.zeros(pol.net.num_recurrent_layers, N, 512, device="cuda")
        o = dict(obs)
        pred, aux = pol(o, h0, prev, masks, weights)
        loss = bench.dagger_loss(pred, aux, o["waypoint"], weights)
        loss.backward()
        opt.step()
        return loss
    for _ in range(warmup):
        update()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(steps):
        loss = update()
    b.record()
    torch.cuda.synchronize()
    pol.check_status()
    AuxLosses.deactivate()
    return a.elapsed_time(b) / steps, float(loss)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=10)
    args = ap.parse_args()
    for cell, bidir, hidden in (("LSTM", True, 128), ("GRU", True, 128), ("LSTM", False, 256), ("GRU", False, 256)):
        ms, loss = leg(cell, bidir, hidden, args.steps, args.warmup)
        print(f"instruction {cell} bidirectional={bidir} hidden={hidden}: {ms:.2f} ms per bf16 update (T=64 N=8), loss {loss:.5f}",
              flush=True)
