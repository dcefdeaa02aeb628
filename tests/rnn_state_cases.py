"""Inputs, float64 references and bars shared by test_rnn_state_cases_cpu.py and test_gpu_rnn_state_edges.py: the persistent state-encoder
kernels of csrc/wsmg_rnn.hip (gru_fwd8 / gru_bwd8 / lstm_state_fwd8 / lstm_state_bwd8) on gi DIRECTLY — no input projection in front
of them, no nn.GRU / nn.LSTM behind the reference.  Nothing here touches a GPU.  Inputs are oracle.detfill values under tags of their
own: w_hh at scale sqrt(12 / 512), b_hh 0.2, gi 2.0, h0 / c0 1.0, gy / g_end 2.0.  H = 512 is the only hidden size the kernels take.

References: each recurrence written out in torch, h (and c) multiplied by masks[t] before step t; `gru_ref` / `lstm_ref` run in whatever
dtype they are given.  Gradients by autograd of sum(y gy) [+ sum(h_T g_end_h) + sum(c_T g_end_c)]; the GRU's dgh is the gradient of
W_hh h + b_hh taken where it is formed (retain_grad), not derived from dgi.

Bars: for each case and output ONE number, 4 x the largest error of the same code run in float32 on the CPU against float64 (the 4
covers the kernels' summation order — K split over 16 lanes x 2 wave halves, 32 producers' partial sums — and the device's expf /
tanhf), never below 2^-23 max|ref| (two float32 roundings).  Elementwise the bar is the smaller of that number and the bar the suite
already applies to the quantity (EXISTING): test_gpu_kernels.py::test_masked_gru_persistent_kernel and
test_gpu_lstm_state.py::_kernel_case, where dgi stands for their dx (dx = dgi W_ih: the quantity the kernel itself contributes).
The saved tensors and dgh have no earlier bar.

A case is named for its edge:
  T{T}.N{N}        lengths 1 2 3 4 5 8 9 (BWD_RING = 4: first reuse of a ring slot at T = 5) at N = 1 and 8; N = 2, 7 at T = 5 (6 and 1
                   idle batch slots); T200.N3 (the documented maximum), T64.N7, T1023.N2 (the launcher's limit: the only length at
                   which the tag's 10-bit step field is all ones).  Restarts at t = 0 in the first N // 2 columns and at T // 2 in the
                   last column; dy and g_end given
  T5.N8.alt        the same shape with other values (the workspace-reuse sequence)
  mask.<kind>[.end]  T = 9, N = 4, without / with g_end: none (no restart, h0 != 0), all_t0, every_step (column 1 restarts at every
                   t), consecutive (t = 3, 4, 5 of column 2), same_step (every column at t = 4), last_step (column 0 at t = T - 1;
                   with g_end only: carry * mk_next at the first backward step).  All of them share one set of values
  saturated        T = 4, N = 2: in batch slot 1 one unit per gate has gi = +120 and one -120 at every step, so that the pre-activation
                   stays beyond +-100 whatever W_hh h + b_hh adds (|.| <= 512 x 0.077 x 1 + 0.1 < 20)
  no_dy            LSTM, T = 5, N = 3: the loss reads c_T alone (dy = None in _MaskedRNN.backward, dhT NULL, dcT given)"""
import functools
import math

import torch

from oracle import detfill as df
from util import T as _t

H = 512
GATES = {"GRU": 3, "LSTM": 4}
W_SCALE = math.sqrt(12.0 / H)
BAR_FACTOR = 4.0
FLOOR = 2.0 ** -23
SAT = 120.0
SAT_SLOT = 1                      # the batch slot whose gates are saturated
SAT_UNIT0 = 37                    # gate g: unit SAT_UNIT0 + 2 g has gi = +SAT, unit SAT_UNIT0 + 2 g + 1 has -SAT

LENGTHS = [(T, N) for T in (1, 2, 3, 4, 5, 8, 9) for N in (1, 8)] + [(200, 3), (64, 7), (1023, 2)]
BATCH = [(5, 2), (5, 7)]          # with (5, 1) and (5, 8) of LENGTHS: N in {1, 2, 7, 8} at T = 5
SHAPE_CASES = [f"T{T}.N{N}" for T, N in LENGTHS + BATCH]
MASK_T, MASK_N = 9, 4
MASK_KINDS = ["none", "all_t0", "every_step", "consecutive", "same_step", "last_step"]
MASK_CASES = [f"mask.{k}" for k in MASK_KINDS if k != "last_step"] + [f"mask.{k}.end" for k in MASK_KINDS]
REUSE = ["T5.N8", "T3.N2", "T5.N8.alt", "T9.N1"]      # one workspace, zeroed once, used by these launches in this order
COMMON = SHAPE_CASES + ["T3.N2", "T5.N8.alt"] + MASK_CASES + ["saturated"]
CASES = {"GRU": COMMON, "LSTM": COMMON + ["no_dy"]}
WRAPPER_CASES = {"GRU": ["T1.N1", "T1.N8", "mask.last_step.end"], "LSTM": ["T1.N1", "T1.N8", "mask.last_step.end", "no_dy"]}

# (rtol, atol as a multiple of max|ref|, atol): the bars the suite holds the same quantity to today (see the module docstring)
EXISTING = {
    "GRU": {"y": (1e-5, 0.0, 2e-6), "dgi": (1e-4, 1e-5, 0.0), "dh0": (1e-4, 1e-5, 1e-9), "dw_hh": (1e-4, 2e-5, 1e-9), "db_hh": (1e-4, 2e-5, 1e-9)},
    "LSTM": {"y": (0.0, 0.0, 1e-5), "c_T": (0.0, 0.0, 1e-5), "dgi": (1e-4, 1e-5, 0.0), "dh0": (1e-4, 1e-5, 1e-9), "dc0": (1e-4, 1e-5, 1e-9),
             "dw_hh": (1e-4, 2e-5, 1e-9), "db_hh": (1e-4, 2e-5, 1e-9)},
}
FORWARD = {"GRU": ["y", "r", "z", "n", "ghn"], "LSTM": ["y", "c", "gates", "c_T"]}
BACKWARD = {"GRU": ["dgi", "dgh", "dh0"], "LSTM": ["dgi", "dh0", "dc0"]}
WEIGHT_GRADS = ["dw_hh", "db_hh"]                      # what the autograd wrappers add (one GEMM and one column sum of dgh)


# ----------------------------------------------------------------------------- the recurrences, in the dtype of their arguments
def gru_ref(gi, w_hh, b_hh, h0, masks, gh_out=None):
    """gi [T, N, 3H] (r, z, n), h0 [N, H], masks [T, N] -> y, r, z, n, ghn = W_hn h + b_hn, each [T, N, H].
    gh_out: a list that receives every step's W_hh h + b_hh [N, 3H] with its gradient retained."""
    h, out = h0, [[], [], [], [], []]
    for t, g in enumerate(gi.unbind(0)):        # (unbind: one backward node for all of gi, not a [T, N, 3H] zero fill per step)
        h = h * masks[t].unsqueeze(-1)
        gh = h @ w_hh.t() + b_hh
        if gh_out is not None:
            gh.retain_grad()
            gh_out.append(gh)
        r = torch.sigmoid(g[:, :H] + gh[:, :H])
        z = torch.sigmoid(g[:, H:2 * H] + gh[:, H:2 * H])
        ghn = gh[:, 2 * H:]
        n = torch.tanh(g[:, 2 * H:] + r * ghn)
        h = (1.0 - z) * n + z * h
        for lst, v in zip(out, (h, r, z, n, ghn)):
            lst.append(v)
    return tuple(torch.stack(v) for v in out)


def lstm_ref(gi, w_hh, b_hh, h0, c0, masks):
    """gi [T, N, 4H] (i, f, g, o) -> y [T, N, H], c [T, N, H], gates [T, N, 4H] (post-activation i, f, g, o), c_T [N, H]."""
    h, c, ys, cs, gs = h0, c0, [], [], []
    for t, x in enumerate(gi.unbind(0)):
        m = masks[t].unsqueeze(-1)
        h, c = h * m, c * m
        pre = x + (h @ w_hh.t() + b_hh)
        i, f, o = torch.sigmoid(pre[:, :H]), torch.sigmoid(pre[:, H:2 * H]), torch.sigmoid(pre[:, 3 * H:])
        g = torch.tanh(pre[:, 2 * H:3 * H])
        c = f * c + i * g
        h = o * torch.tanh(c)
        ys.append(h), cs.append(c), gs.append(torch.cat([i, f, g, o], dim=1))
    return torch.stack(ys), torch.stack(cs), torch.stack(gs), c


# ----------------------------------------------------------------------------- case table
def spec(name):
    """{T, N, mask kind, g_end, dy, sat, values tag} of a case name."""
    s = dict(mask="mixed", g_end=True, dy=True, sat=False, tag=name)
    if name.startswith("mask."):
        parts = name.split(".")
        s.update(T=MASK_T, N=MASK_N, mask=parts[1], g_end=len(parts) == 3, tag="mask")
    elif name == "saturated":
        s.update(T=4, N=2, sat=True)
    elif name == "no_dy":
        s.update(T=5, N=3, dy=False)
    else:
        parts = name.split(".")
        s.update(T=int(parts[0][1:]), N=int(parts[1][1:]))
    return s


def masks_of(kind, T, N):
    m = torch.ones(T, N)
    if kind == "mixed":
        m[0, :N // 2] = 0
        if T >= 3:
            m[T // 2, N - 1] = 0
    elif kind == "all_t0":
        m[0, :] = 0
    elif kind == "every_step":
        m[:, 1] = 0
    elif kind == "consecutive":
        m[3:6, 2] = 0
    elif kind == "same_step":
        m[4, :] = 0
    elif kind == "last_step":
        m[T - 1, 0] = 0
    else:
        assert kind == "none", kind
    return m


def weights(cell):
    G = GATES[cell]
    return _t(df.uniform(f"rnnedge.{cell}.w_hh", (G * H, H), W_SCALE)), _t(df.uniform(f"rnnedge.{cell}.b_hh", (G * H,), 0.2))


def inputs(cell, name):
    """float32 CPU tensors of a case: gi, w_hh, b_hh, state [R, N, H] (h0, or h0 and c0), masks, gy (zeros for no_dy), g_end [R, N, H]
    with `ends` = which of its rows the loss reads."""
    s, G, R = spec(name), GATES[cell], 1 if cell == "GRU" else 2
    Tn, N, tag = s["T"], s["N"], f"rnnedge.{cell}.{s['tag']}"
    w_hh, b_hh = weights(cell)
    gi = _t(df.uniform(tag + ".gi", (Tn, N, G * H), 2.0))
    if s["sat"]:
        for g in range(G):
            gi[:, SAT_SLOT, g * H + SAT_UNIT0 + 2 * g] = SAT
            gi[:, SAT_SLOT, g * H + SAT_UNIT0 + 2 * g + 1] = -SAT
    gy = _t(df.uniform(tag + ".gy", (Tn, N, H), 2.0)) if s["dy"] else torch.zeros(Tn, N, H)
    ends = [s["g_end"] and s["dy"]] + ([s["g_end"]] if R == 2 else [])
    return dict(spec=s, gi=gi, w_hh=w_hh, b_hh=b_hh, state=_t(df.uniform(tag + ".state", (R, N, H), 1.0)), masks=masks_of(s["mask"], Tn, N),
                gy=gy, g_end=_t(df.uniform(tag + ".g_end", (R, N, H), 2.0)), ends=ends)


def evaluate(cell, inp, dtype, weight_grads=False):
    """The recurrence and its gradients in `dtype` on the CPU -> {output name: tensor}: FORWARD + BACKWARD of the cell, and
    WEIGHT_GRADS where asked for (T outer products of 3H x H: most of the time of a long case)."""
    gi, state = (inp[k].to(dtype, copy=True).requires_grad_(True) for k in ("gi", "state"))
    w_hh, b_hh = (inp[k].to(dtype, copy=True).requires_grad_(weight_grads) for k in ("w_hh", "b_hh"))
    masks, gy, g_end = (inp[k].to(dtype) for k in ("masks", "gy", "g_end"))
    if cell == "GRU":
        ghs = []
        y, r, z, n, ghn = gru_ref(gi, w_hh, b_hh, state[0], masks, ghs)
        out = dict(y=y, r=r, z=z, n=n, ghn=ghn)
        ends = [y[-1]]
    else:
        y, c, gates, c_T = lstm_ref(gi, w_hh, b_hh, state[0], state[1], masks)
        out = dict(y=y, c=c, gates=gates, c_T=c_T)
        ends = [y[-1], c_T]
    loss = (y * gy).sum()
    for on, e, g in zip(inp["ends"], ends, g_end):
        if on:
            loss = loss + (e * g).sum()
    loss.backward()
    out = {k: v.detach() for k, v in out.items()}
    out.update(dgi=gi.grad, dh0=state.grad[0])
    if weight_grads:
        out.update(dw_hh=w_hh.grad, db_hh=b_hh.grad)
    if cell == "GRU":
        out["dgh"] = torch.stack([g.grad for g in ghs])
    else:
        out["dc0"] = state.grad[1]
    return out


@functools.lru_cache(maxsize=6)
def case(cell, name):
    """inputs(), the float64 reference `ref`, the float32 CPU evaluation's largest error per output `f32_err`, and `bar`: the
    elementwise float64 bar of every output.  dw_hh and db_hh for the WRAPPER_CASES only."""
    c = inputs(cell, name)
    wg = name in WRAPPER_CASES[cell]
    ref, f32 = evaluate(cell, c, torch.float64, wg), evaluate(cell, c, torch.float32, wg)
    c["ref"] = ref
    c["f32_err"] = {k: float((f32[k].double() - ref[k]).abs().max()) for k in ref}
    c["derived"] = {k: max(BAR_FACTOR * c["f32_err"][k], FLOOR * float(ref[k].abs().max())) for k in ref}
    c["bar"] = {k: bar_of(cell, k, ref[k], c["derived"][k]) for k in ref}
    return c


def existing_bar(cell, out, ref):
    """The elementwise bar the suite already applies to `out`, or None."""
    if out not in EXISTING[cell]:
        return None
    rtol, amax, atol = EXISTING[cell][out]
    return rtol * ref.abs() + (amax * float(ref.abs().max()) + atol)


def bar_of(cell, out, ref, derived):
    old = existing_bar(cell, out, ref)
    new = torch.full_like(ref, derived)
    return new if old is None else torch.minimum(new, old)


def ratio(got, ref, bar):
    """max over elements of |got - ref| / bar (0 / 0 = 0: where the reference is exactly 0 everywhere, so must the kernel be);
    inf for a result that is not finite."""
    got = got.detach().double().cpu().reshape(ref.shape)
    if not bool(torch.isfinite(got).all()):
        return float("inf"), float("nan")
    err = (got - ref).abs()
    q = torch.where(err == 0, torch.zeros_like(err), err / bar)
    return float(q.max()), float(err.max())


def saturated_slots(cell):
    """[(tensor name, column into that tensor's last dimension, the value the gate must take)] of the saturated case, batch slot
    SAT_SLOT, every step.  GRU: r, z in {1, 0}, n in {+1, -1}; LSTM gates: i, f, o in {1, 0}, g in {+1, -1}."""
    out = []
    if cell == "GRU":
        for g, nm in enumerate(("r", "z", "n")):
            lo = -1.0 if nm == "n" else 0.0
            out += [(nm, SAT_UNIT0 + 2 * g, 1.0), (nm, SAT_UNIT0 + 2 * g + 1, lo)]
    else:
        for g in range(4):
            lo = -1.0 if g == 2 else 0.0
            out += [("gates", g * H + SAT_UNIT0 + 2 * g, 1.0), ("gates", g * H + SAT_UNIT0 + 2 * g + 1, lo)]
    return out
