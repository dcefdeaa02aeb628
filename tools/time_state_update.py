#!/usr/bin/env python3
"""GPU-box tool: one bf16 configs[1] update (T = 64 x N = 8, the bench's synthetic batch and optimizer) per arm — state encoders
(MODEL.STATE_ENCODER.rnn_type) GRU or LSTM x net.recurrent_chunks 0 (the staged route) or 4 (the pipelined recurrent core) — timed
with HIP events over `--steps` updates after `--warmup`.  Each arm's line names the route its updates took: "core" when the
pipelined block (wsmgmap.recurrent.recurrent_block) ran in every update, else "staged".  Not a bench.py leg: the bench line measures
the default configuration only."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "ws-mgmap_amd"))
import torch  # noqa: E402

import bench  # noqa: E402

ARMS = {"gru0": ("GRU", 0), "gru4": ("GRU", 4), "lstm0": ("LSTM", 0), "lstm4": ("LSTM", 4)}


def leg(rnn_type, chunks, steps, warmup, T=64, N=8):
    from wsmgmap import debug, ops, recurrent
    from wsmgmap.common.aux_losses import AuxLosses
    from wsmgmap.config import default_model_config
    from wsmgmap.models.policy import BasePolicy
    from wsmgmap.optim import Adam
    torch.manual_seed(0)
    mc = default_model_config(num_proc=1, compute_dtype="bf16")
    mc.STATE_ENCODER.rnn_type = rnn_type
    pol = BasePolicy(None, bench._Box(), mc)
    pol.net.instruction_encoder.embedding_layer.weight.requires_grad_(False)
    pol = pol.cuda()
    pol.train()
    pol.net.depth_encoder.eval()
    pol.net.rgb_encoder.eval()
    pol.net.recurrent_chunks = chunks
    opt = Adam(pol.parameters(), lr=2.5e-4)
    obs, prev, masks, weights = bench.synth_batch(T, N, "cuda", 1000)
    ops.mark_inputs_ready(obs["instruction"])
    AuxLosses.activate()
    calls = [0]
    block = recurrent.recurrent_block

    def counted(*a, **k):
        calls[0] += 1
        return block(*a, **k)

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
    recurrent.recurrent_block = counted
    try:
        for _ in range(warmup):
            update()
        torch.cuda.synchronize()
        calls[0] = 0
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(steps):
            loss = update()
        b.record()
        torch.cuda.synchronize()
    finally:
        recurrent.recurrent_block = block
    pol.check_status()
    AuxLosses.deactivate()
    route = ("core, chained" if debug.sw.recurrent_chain else "core, chunk launches") if calls[0] == steps else \
        "staged" if calls[0] == 0 else f"mixed ({calls[0]} of {steps} through the core)"
    return a.elapsed_time(b) / steps, float(loss), route


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--arms", default="gru0,gru4,lstm0,lstm4", help="comma-separated subset of " + ", ".join(ARMS))
    ap.add_argument("--tag", default="", help="a label printed on every line (e.g. the commit)")
    args = ap.parse_args()
    for name in args.arms.split(","):
        rnn_type, chunks = ARMS[name]
        ms, loss, route = leg(rnn_type, chunks, args.steps, args.warmup)
        print(f"{args.tag}state {rnn_type} recurrent_chunks={chunks}: {ms:.3f} ms per bf16 update (T=64 N=8, {args.steps} updates), "
              f"route {route}, loss {loss:.5f}", flush=True)
