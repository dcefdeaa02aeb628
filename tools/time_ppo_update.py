#!/usr/bin/env python3
"""GPU-box tool: a PPO minibatch as one grouped gather launch against the `index_select` route, and one `PPO.update` for context.

    python3 tools/time_ppo_update.py [--rounds 7] [--passes 3] [--parts a,b,c] [--out FILE]

(a) `RolloutStorage.recurrent_generator(advantages, 2)` at (T, N) = (128, 8) with the update path's eight observation keys
    (oracle/cases.update_inputs' shapes; the ego map is 2.56 MB per step and environment): fused = one `ops.gather_columns` launch per
    minibatch into fresh tensors, reuse = the same into the storage's staging buffers (`reuse_buffers=True`, what `PPO.update` passes),
    stock = a `fused=False` storage, an `index_select` + allocation per field behind a host copy of the index list.
(b) the same with no observation keys: the eight non-observation fields, 4 to 4 096 bytes per row — launches, not bytes.
(c) one `PPO.update` (ppo_epoch 2 x 2 minibatches) on the tests' T = 4 policy against tests/ppo_util.py's written-out loop on a
    `fused=False` storage: context only, the net's forward and backward dominate both.

The arms are interleaved round by round; a round is `passes` passes of the generator (2 minibatches each) between two HIP events,
host-paced, reported in us per minibatch with the median, minimum and maximum over the rounds.  For (a) the bytes a minibatch moves
(read + written) over the median time are set beside the 6.29 TB/s a float4 copy reaches on this part."""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "ws-mgmap_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)
import torch  # noqa: E402

from wsmgmap.rollout import RolloutStorage  # noqa: E402

T, N, NMB = 128, 8, 2
COPY_RATE = 6.29e12


def storages(with_obs):
    shapes = {}
    if with_obs:
        from oracle import cases
        obs, _, _, _ = cases.update_inputs(1, 2, tag="time")
        shapes = {k: (tuple(v.shape[1:]), torch.from_numpy(v).dtype) for k, v in obs.items()}
    g = torch.Generator(device="cuda"); g.manual_seed(1)
    pair = []
    for fused in (True, False):
        st = RolloutStorage(T, N, shapes, 2, 512, 2, fused=fused).to("cuda")
        for name in st._TENSORS:
            getattr(st, name).normal_(generator=g)
        for v in st.observations.values():
            v.normal_(generator=g)
        st.masks.fill_(1.0)
        st.step = T
        pair.append(st)
    for name in pair[0]._TENSORS:
        getattr(pair[1], name).copy_(getattr(pair[0], name))
    for k, v in pair[0].observations.items():
        pair[1].observations[k].copy_(v)
    for st in pair:
        st.compute_returns(torch.zeros(N, 1, device="cuda"), True, 0.99, 0.95)
    return pair


def minibatch_bytes(st):
    per = N // NMB
    fields = list(st.observations.values()) + [st.actions, st.prev_actions, st.value_preds, st.returns, st.masks, st.action_log_probs,
                                                st.rewards]                    # (rewards: the size of the advantages)
    moved = sum(t[0, 0].numel() * t.element_size() for t in fields) * T * per
    moved += st.recurrent_hidden_states[0, :, 0].numel() * 4 * per
    return 2 * moved, len(fields) + 1


def rounds_of(arms, rounds, per_round):
    times = {name: [] for name, _ in arms}
    for _ in range(rounds):
        for name, fn in arms:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            times[name].append(e0.elapsed_time(e1) * 1e3 / per_round)
    return times


def gather_part(tag, with_obs, a, lines):
    fused, stock = storages(with_obs)
    adv = [st.get_advantages(False) for st in (fused, stock)]

    def passes(st, ad, **kw):
        for _ in range(a.passes):
            for _batch in st.recurrent_generator(ad, NMB, **kw):
                pass

    torch.manual_seed(3)
    x = list(fused.recurrent_generator(adv[0], NMB))
    torch.manual_seed(3)
    y = list(stock.recurrent_generator(adv[1], NMB))
    same = all(torch.equal(p, q) for b, c in zip(x, y) for p, q in zip(list(b[0].values()) + list(b[1:]), list(c[0].values()) + list(c[1:])))
    del x, y
    arms = (("fused", lambda: passes(fused, adv[0])), ("reuse", lambda: passes(fused, adv[0], reuse_buffers=True)),
            ("stock", lambda: passes(stock, adv[1])))
    for _, fn in arms:
        fn()
    torch.cuda.synchronize()
    times = rounds_of(arms, a.rounds, a.passes * NMB)
    moved, nfields = minibatch_bytes(fused)
    lines.append(f"({tag}) T = {T}, N = {N}, {NMB} minibatches, {nfields} fields, {moved / 1e6:.3f} MB read + written per minibatch; "
                 f"fused and stock minibatches equal: {same}")
    for name, _ in arms:
        t = times[name]
        med = statistics.median(t)
        lines.append(f"  {name:6s}  median {med:10.1f}   min {min(t):10.1f}   max {max(t):10.1f}   {moved / (med * 1e-6) / 1e12:6.3f} TB/s "
                     f"({100 * moved / (med * 1e-6) / COPY_RATE:5.1f} % of the float4 copy rate)")


def update_part(a, lines):
    import ppo_util as pu
    from wsmgmap.optim import Adam
    from wsmgmap.ppo import PPO
    hyper = dict(clip_param=0.2, ppo_epoch=2, num_mini_batch=2, value_loss_coef=0.5, entropy_coef=0.01)
    fused, stock = pu.policy_storages()
    pol_a, pol_b = pu.build_policy(), pu.build_policy()
    agent = PPO(pol_a, lr=2.5e-4, eps=1e-5, max_grad_norm=0.5, **hyper)
    opt = Adam([p for p in pol_b.parameters() if p.requires_grad], lr=2.5e-4, eps=1e-5, max_grad_norm=0.5)
    arms = (("PPO.update", lambda: agent.update(fused)),
            ("written-out loop", lambda: pu.written_out_update(pol_b, stock, opt, max_grad_norm=0.5, **hyper)))
    for _, fn in arms:
        fn()
    torch.cuda.synchronize()
    times = rounds_of(arms, a.rounds, 1)
    lines.append("(c) one update of the tests' T = 4 policy, N = 4, ppo_epoch 2 x 2 minibatches, us per update (both end in one read-back)")
    for name, _ in arms:
        t = times[name]
        lines.append(f"  {name:16s}  median {statistics.median(t):10.1f}   min {min(t):10.1f}   max {max(t):10.1f}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--passes", type=int, default=3)
    ap.add_argument("--parts", default="a,b,c")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lines = [f"{a.rounds} interleaved rounds of {a.passes} generator passes, us per minibatch between HIP events (host-paced); pid {os.getpid()}"]
    parts = a.parts.split(",")
    if "a" in parts:
        gather_part("a", True, a, lines)
    if "b" in parts:
        gather_part("b", False, a, lines)
    if "c" in parts:
        update_part(a, lines)
    text = "\n".join(lines)
    print(text)
    if a.out:
        with open(a.out, "a") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
