#!/usr/bin/env python3
"""GPU-box tool: SHA-256 of every output and gradient of the heads family on fixed inputs — the listing two builds of the library
must share when a change claims to leave their bits alone.

    python3 tools/heads_bits.py [--out FILE]                    (WSMG_LIB=<other build>/libwsmgmap.so for the other side)

Inputs come from CPU generators with fixed seeds.  At (B, K, A) = (3, 260, 1), (5, 516, 4), (33, 256, 2), (33, 512, 4):
update_heads in its four gradient forms, eval_heads with all gradients and with one at a time, aux_reduce, dagger_loss, ppo_loss
(masked and unmasked, clipped value loss and plain), act_heads (mode and sampled), linear_rows (plain, tanh, pooled input).
One `name shape sha256` line per tensor; the digest is of the tensor's bytes after a copy to the host."""
import argparse
import copy
import hashlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "ws-mgmap_amd"))
import torch  # noqa: E402

from wsmgmap import ops  # noqa: E402

SHAPES = [(3, 260, 1), (5, 516, 4), (33, 256, 2), (33, 512, 4)]
LINES = []


def emit(name, shape, t):
    h = t.detach().contiguous().cpu()
    LINES.append(f"{name} B{shape[0]}_K{shape[1]}_A{shape[2]} {tuple(h.shape)} {hashlib.sha256(h.numpy().tobytes()).hexdigest()}")


def gen(*seed):
    g = torch.Generator()
    g.manual_seed(sum(s * 1009 ** i for i, s in enumerate(seed)) + 17)
    return g


def linear(K, O, g):
    m = torch.nn.Linear(K, O)
    with torch.no_grad():
        for p in (m.weight, m.bias):
            p.copy_((torch.rand(p.shape, generator=g) * 2 - 1) / K ** 0.5)
    return m


def update_heads(shape):
    B, K, A = shape
    g = gen(1, *shape)
    x, fc, pp = torch.randn(B, K, generator=g), linear(K, A, g), linear(K, 1, g)
    progress = torch.rand(B, 1, generator=g)
    gs = [torch.rand(B, A, generator=g) + 0.5, -(torch.rand(B, 1, generator=g) + 0.5), torch.rand(B, generator=g) + 0.5]
    forms = {"pred_only": (1, 0, 0), "prog_only": (0, 1, 0), "rows_only": (0, 0, 1), "all_three": (1, 1, 1)}
    for form, use in forms.items():
        xg = x.cuda().requires_grad_(True)
        fcg, ppg = copy.deepcopy(fc).cuda(), copy.deepcopy(pp).cuda()
        outs = ops.update_heads(xg, fcg, ppg, progress.cuda())
        sum((o * w.cuda()).sum() for u, o, w in zip(use, outs, gs) if u).backward()
        for n, o in zip(("pred", "prog", "prog_rows"), outs):
            emit(f"update_heads.{form}.{n}", shape, o)
        for n, t in zip(("dx", "dWm", "dbm", "dWp", "dbp"), (xg.grad, fcg.weight.grad, fcg.bias.grad, ppg.weight.grad, ppg.bias.grad)):
            emit(f"update_heads.{form}.{n}", shape, t)


def eval_heads(shape):
    B, K, A = shape
    g = gen(2, *shape)
    x, fc, cr = torch.randn(B, K, generator=g), linear(K, A, g), linear(K, 1, g)
    ls = 0.5 * (torch.rand(A, 1, generator=g) * 2 - 1)
    action = torch.nn.functional.linear(x, fc.weight, fc.bias).detach() + torch.randn(B, A, generator=g) * ls.t().exp()
    gs = [torch.rand(B, 1, generator=g) + 0.5, torch.rand(B, generator=g) + 0.5, torch.tensor(0.75)]
    forms = {"all": (1, 1, 1), "value_only": (1, 0, 0), "logp_only": (0, 1, 0), "entropy_only": (0, 0, 1)}
    for form, use in forms.items():
        xg = x.cuda().requires_grad_(True)
        fcg, crg = copy.deepcopy(fc).cuda(), copy.deepcopy(cr).cuda()
        lsg = ls.cuda().requires_grad_(True)
        outs = ops.eval_heads(xg, fcg, lsg, crg, action.cuda())
        sum((o * w.cuda()).sum() for u, o, w in zip(use, outs, gs) if u).backward()
        for n, o in zip(("value", "logp", "entropy"), outs):
            emit(f"eval_heads.{form}.{n}", shape, o)
        for n, t in zip(("dx", "dWm", "dbm", "dlogstd", "dWc", "dbc"),
                        (xg.grad, fcg.weight.grad, fcg.bias.grad, lsg.grad, crg.weight.grad, crg.bias.grad)):
            emit(f"eval_heads.{form}.{n}", shape, t)


def aux_reduce(shape):
    B = shape[0]
    g = gen(3, *shape)
    rows = [(torch.rand(B, generator=g) + 0.1).cuda().requires_grad_(True) for _ in range(3)]
    mask = torch.rand(B, generator=g) < 0.7
    mask[0] = True
    v = ops.aux_reduce(rows, (1.0, 0.5, 0.25), mask.cuda())
    v.backward()
    emit("aux_reduce.value", shape, v)
    for k, r in enumerate(rows):
        emit(f"aux_reduce.drows{k}", shape, r.grad)


def dagger_loss(shape):
    T_, _, A = shape
    N = 3
    g = gen(4, *shape)
    pred = torch.randn(T_ * N, A, generator=g).cuda().requires_grad_(True)
    wp = torch.rand(T_ * N, A + 1, generator=g) * 2 - 1
    weights = torch.rand(T_, N, generator=g) + 0.25
    aux = torch.tensor(0.25, device="cuda", requires_grad=True)
    loss, action = ops.dagger_loss(pred, aux, wp.cuda(), weights.cuda())
    loss.backward()
    for n, t in (("loss", loss), ("action", action), ("dpred", pred.grad), ("daux", aux.grad)):
        emit(f"dagger_loss.{n}", shape, t)


def ppo_loss(shape):
    B = shape[0] * 37          # more than one pass of the 256 threads at B = 33
    g = gen(5, *shape)
    r = lambda: torch.randn(B, generator=g)      # noqa: E731
    old_logp = -1.0 - r().abs()
    logp0, adv, old_value = old_logp + 0.3 * r(), r(), r()
    value0, ret = old_value + 0.3 * r(), old_value + r()
    mask = torch.rand(B, generator=g) < 0.6
    mask[0] = True
    for form, m, clipped in (("plain", None, True), ("masked", mask, True), ("unclipped_value", None, False)):
        logp, value = logp0.cuda().requires_grad_(True), value0.cuda().requires_grad_(True)
        ent = torch.tensor([1.3], device="cuda", requires_grad=True)
        outs = ops.ppo_loss(logp, old_logp.cuda(), adv.cuda(), value, old_value.cuda(), ret.cuda(), ent, 0.2, 0.5, 0.01,
                            clipped_value=clipped, mask=None if m is None else m.cuda())
        outs[0].backward()
        for n, o in zip(("loss", "action_loss", "value_loss", "clip_frac", "approx_kl"), outs):
            emit(f"ppo_loss.{form}.{n}", shape, o)
        for n, t in (("dlogp", logp.grad), ("dvalue", value.grad), ("dentropy", ent.grad)):
            emit(f"ppo_loss.{form}.{n}", shape, t)


def act_heads(shape):
    B, K, A = shape
    g = gen(6, *shape)
    x = torch.randn(B, K, generator=g).cuda()
    pp, fc, cr = linear(K, 1, g).cuda(), linear(K, A, g).cuda(), linear(K, 1, g).cuda()
    ls = (0.5 * (torch.rand(A, 1, generator=g) * 2 - 1)).cuda()
    noise = torch.randn(B, A, generator=g).cuda()
    for form, nz in (("mode", None), ("sampled", noise)):
        for n, t in zip(("prog", "value", "action", "logp"), ops.act_heads(x, pp, fc, ls, cr, nz)):
            emit(f"act_heads.{form}.{n}", shape, t)


def linear_rows(shape):
    B, K, _ = shape
    g = gen(7, *shape)
    lin = linear(K, 7, g).cuda()
    x = torch.randn(B, K, generator=g).cuda()
    xp = torch.randn(B, K, 3, generator=g).cuda()
    emit("linear_rows.plain", shape, ops.linear_rows(x, lin.weight, lin.bias))
    emit("linear_rows.tanh_nobias", shape, ops.linear_rows(x, lin.weight, None, act="tanh"))
    emit("linear_rows.relu_pool3", shape, ops.linear_rows(xp, lin.weight, lin.bias, act="relu", pool=3))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    for shape in SHAPES:
        for fn in (update_heads, eval_heads, aux_reduce, dagger_loss, ppo_loss, act_heads, linear_rows):
            fn(shape)
    torch.cuda.synchronize()
    text = "\n".join(LINES)
    print(text)
    print(f"# {len(LINES)} tensors, sha256 of all lines: {hashlib.sha256(text.encode()).hexdigest()}")
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
