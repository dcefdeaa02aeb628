"""Inputs, float64 references, derived bars and fault models shared by test_attn_cases_cpu.py and test_gpu_attn_edges.py: the four
single-query attention kernels of csrc/wsmg_attn.hip at the token counts, masks and logit placements where hand-written tails,
butterflies and online softmaxes go wrong.  Nothing here touches a GPU.  Inputs are oracle.detfill values under tags of their own;
every reference is oracle.policy_ref.attn's formula evaluated in float64, gradients by float64 autograd, for bf16 from the
bf16-rounded operands.

Forms.  "generic": attn_fwd_kernel / attn_bwd_kernel, 4 tokens per trip, 4 waves, 16 tokens per sweep (distinct k and v; also the
shared-set calls).  "same": attn_same_fwd_kernel / attn_same_bwd_kernel <T, 16>, keys are values, 8 tokens per trip, 16 waves, 128 per
sweep.  C = 256 and scale = 1 / 16 throughout.

Which kind meets which mask.  At every token count every kind meets every mask that fits the count (applies()); the kind "grid"
comes with the mask "full_row" only.  One float64 reference with its bars costs a tenth of a second at 2304 and 2560 tokens, so the
tests take those counts one kind at a time (combos(form, I, kind))."""
import functools
import math

import numpy as np
import torch

from oracle import detfill as df

C = 256
SCALE = 1.0 / 16
U32 = 2.0 ** -24          # unit roundoff of float32
BF16_EPS = 2.0 ** -8      # as tests/test_gpu_kernels.py: the bar of one bf16 rounding
FLOOR = 2.0 ** -120       # a float32 / bf16 result below 2^-126 may be flushed to zero; 2^6 of room for the factor |q|, |g| or |k|
AMAX_I = 2560             # csrc/wsmg_attn.hip: logits kept in LDS
REFUSED_I = AMAX_I + 1
FORMS = {"generic": {"trip": 4, "waves": 4}, "same": {"trip": 8, "waves": 16}}
COUNTS = {"generic": [1, 3, 4, 5, 15, 16, 17, 255, 256, 257, 2304, 2560],
          "same": [1, 7, 8, 9, 127, 128, 129, 136, 257, 2304, 2560]}
SHARED_COUNTS = [1, 5, 17, 257, 2560]
LARGE = 2304              # from here on a test takes one kind at a time (module docstring)
KINDS = ["plain", "ascending", "peak_last", "peak_first", "shifted+200", "shifted-200", "lane_tagged"]
# prefix masks keep the first n tokens (as oracle.cases.attn_inputs' lengths do); "prefix_I-1" is also "the last token of the tail
# masked"; "prefix_I" masks nothing but passes a mask pointer.  "full_row" comes with the kind "grid" only.
MASKS = ["none", "prefix_1", "prefix_I-1", "prefix_I", "scattered", "first_sweep", "one_wave"]
# shared-set index vectors: name -> (U, inverse)
SHARED = {"u1": (1, [0, 0, 0]), "unused_set": (3, [2, 0, 2, 0]), "set_of_every_row": (2, [1, 1, 1]), "unsorted": (3, [2, 0, 1, 0, 2]),
          "b1": (2, [1])}


def sweep(form):
    return FORMS[form]["trip"] * FORMS[form]["waves"]


def rows(I):
    return 3 if I >= 255 else 5


def T(a):
    return torch.from_numpy(np.ascontiguousarray(a))


def bf_round(t):
    return t.to(torch.bfloat16).float()


def applies(form, I, mask):
    """Whether a named mask fits a token count: a row keeps at least one token (only "full_row" masks a whole row)."""
    if mask in ("none", "prefix_I"):
        return True
    if mask in ("prefix_1", "prefix_I-1", "scattered", "full_row"):
        return I >= 2 or mask == "full_row"
    if mask == "first_sweep":
        return I > sweep(form)
    if mask == "one_wave":
        return I >= 16
    raise KeyError(mask)


def combos(form, I, kind=None):
    """The (kind, mask) pairs of a token count: every kind with every mask that fits, then the grid kind with its fully masked row;
    with `kind`, that kind's pairs only."""
    out = [(k, m) for k in KINDS for m in MASKS if applies(form, I, m)] + [("grid", "full_row")]
    return [c for c in out if kind is None or c[0] == kind]


def _grid(tag, shape, scale):
    return np.round(df.uniform(tag, shape, scale).astype(np.float64)) + 0.0


def folded_query(tag, B):
    """(q0 [B, C], W [C, C], b [C], q = q0 W): the folded form's operands on grids — q0 on multiples of 1/32 in [-4, 4], W on
    {-2, ..., 2} / 16 — so that q0 W is exact in float32 in any order (every product a multiple of 2^-9 below 1, every partial sum
    below 2^8: 17 bits) and the kernel sees exactly the query the reference uses.  The key bias b cancels in the softmax."""
    q0 = np.round(df.uniform(tag + ".q0", (B, C), 8.0).astype(np.float64) * 32.0) / 32.0
    W = _grid(tag + ".w", (C, C), 4.0) / 16.0
    b = df.uniform(tag + ".b", (C,), 0.6).astype(np.float64)
    return q0, W, b, q0 @ W


@functools.lru_cache(maxsize=4)
def inputs(form, I, kind, mask, bf16, shared=None):
    """One case.  q [B, C] float32; k, v [U, I, C] float32 (bf16: rounded; form "same": v is k); inverse [B] int64 (per-row forms:
    arange); mask [U, I] bool or None; dout [B, C], dattn [B, I] float32; for the form "same" also q0, W, b of folded_query.

    The scaled logits of set u are placed through the query of the first row that uses it (row 0 for an unused set): adding
    (t / scale) q / |q|^2 to a key raises that row's scaled logit by t.
      plain        k = detfill in [-1, 1), for the form "same" in [-3, 3): scaled logits spanning several tens.  (detfill runs of one
                   stride correlate, so dot products of two runs are larger than independent values would give; the query of the
                   form "same" is a matrix product and correlates less.)
      ascending    small noise (amplitude 2^-6: scaled logits within +-0.2) + t_i = i min(1, 80 / (I - 1)): the running maximum of a
                   wave rises on every trip and the last token dominates
      peak_last / peak_first   plain, and the last token / token 0 lifted 32 above the largest other scaled logit
      shifted+-200 plain, every scaled logit moved by +-200: exp without the maximum subtracted overflows / underflows in float32
      lane_tagged  small noise + t_i = 3 (i mod 8), and for distinct values v_i += (i mod 8) / 2: a permuted token of a trip moves
                   its weight by a factor of e^3 or more
      grid         q, k, v integers in {-2, ..., 2}: every dot product (|d| <= 1024) is exact in float32 in any order, so
                   float32(d - 1e8f) * scale is a defined reference for the fully masked row of the mask "full_row"."""
    B = rows(I)
    inverse = np.arange(B)
    if shared is not None:
        U, inv = SHARED[shared]
        inverse, B = np.asarray(inv), len(inv)
    U = int(inverse.max()) + 1 if shared is None else SHARED[shared][0]
    tag = f"attnedge.{form}.{I}.{kind}" + (f".{shared}" if shared else "")
    extra = {}
    if kind == "grid":
        q = _grid(tag + ".q", (B, C), 4.0)
        if form == "same":
            extra = {"q0": q, "W": np.eye(C), "b": np.zeros(C)}
        k = _grid(tag + ".k", (U, I, C), 4.0)
        v = k if form == "same" else _grid(tag + ".v", (U, I, C), 4.0)
    else:
        if form == "same":
            q0, W, b, q = folded_query(tag, B)
            extra = {"q0": q0, "W": W, "b": b}
        else:
            q = df.uniform(tag + ".q", (B, C), 8.0).astype(np.float64)
        small = kind in ("ascending", "lane_tagged")
        k = df.uniform(tag + ".k", (U, I, C), 2.0 ** -6 if small else (6.0 if form == "same" else 2.0)).astype(np.float64)
        first = [int(np.argmax(inverse == u)) if (inverse == u).any() else 0 for u in range(U)]
        qs = q[first]                                                          # [U, C]
        qhat = qs / (qs * qs).sum(axis=1, keepdims=True)
        t = np.zeros((U, I))
        idx = np.arange(I)
        if kind == "ascending":
            t[:] = idx * min(1.0, 80.0 / max(I - 1, 1))
        elif kind == "lane_tagged":
            t[:] = 3.0 * (idx % 8)
        elif kind.startswith("shifted"):
            t[:] = float(kind[len("shifted"):])
        elif kind in ("peak_last", "peak_first") and I > 1:
            p = I - 1 if kind == "peak_last" else 0
            l = SCALE * np.einsum("uc,uic->ui", qs, k)
            others = np.delete(l, p, axis=1).max(axis=1)
            t[:, p] = others - l[:, p] + 32.0
        k = k + (t / SCALE)[:, :, None] * qhat[:, None, :]
        if form == "same":
            v = k
        else:
            v = df.uniform(tag + ".v", (U, I, C), 2.0).astype(np.float64)
            if kind == "lane_tagged":
                v = v + 0.5 * (idx % 8)[None, :, None]
    q, k = T(q).float(), T(k).float()
    v = k if form == "same" else T(v).float()
    if bf16:
        k = bf_round(k)
        v = k if form == "same" else bf_round(v)
    inv_t = T(inverse).long()
    m = _mask(form, I, mask, tag, q, k, inv_t, U)
    out = {"form": form, "I": I, "kind": kind, "mask_name": mask, "bf16": bf16, "shared": shared, "B": B, "U": U,
           "q": q, "k": k, "v": v, "inverse": inv_t, "mask": m,
           "dout": T(df.uniform(tag + ".go", (B, C), 2.0)), "dattn": T(df.uniform(tag + ".ga", (B, I), 2.0))}
    out.update({n: T(a) for n, a in extra.items()})
    return out


def _mask(form, I, name, tag, q, k, inverse, U):
    """bool [U, I] (True = masked) or None."""
    if name == "none":
        return None
    m = torch.zeros(U, I, dtype=torch.bool)
    if name == "prefix_1":
        m[:, 1:] = True
    elif name == "prefix_I-1":
        m[:, I - 1:] = True
    elif name == "prefix_I":
        pass
    elif name == "first_sweep":
        m[:, :sweep(form)] = True
    elif name == "one_wave":
        m[:, 8:16] = True
    elif name == "scattered":
        # about a third of the tokens, and the token with the largest raw logit of the first row that uses the set; its neighbour stays
        first = [int((inverse == u).nonzero()[0]) if bool((inverse == u).any()) else 0 for u in range(U)]
        d = torch.einsum("uc,uic->ui", q[first].double(), k.double())
        top = d.argmax(dim=1)
        m = T(df.uniform(tag + ".scatter", (U, I), 1.0)) > 0.17
        m[torch.arange(U), top] = True
        m[torch.arange(U), (top + 1) % I] = False
    elif name == "full_row":
        m[:, max(1, I // 2):] = True            # every set a prefix mask ...
        m[int(inverse[-1])] = True              # ... and the last row's set masked altogether (per-row forms: the last row)
    else:
        raise KeyError(name)
    return m


# ----------------------------------------------------------------------------- reference
def logits64(inp, q, k):
    """Scaled logits [B, I] as float64 tensors of the graph of q and k (k: [B, I, C], gathered).  Kind "grid": the model's own float32
    semantics, float32(d - 1e8f) * scale, entered as a constant offset to the exact d (the dot products are exact integers)."""
    d = torch.einsum("bc,bic->bi", q, k)
    if inp["mask"] is None:
        return d, d * SCALE
    mrow = inp["mask"][inp["inverse"]]
    if inp["kind"] == "grid":
        d32 = d.detach().float()
        assert torch.equal(d32.double(), d.detach())
        l32 = torch.where(mrow, d32 - torch.tensor(1e8, dtype=torch.float32), d32)
        return d, (d + (l32.double() - d.detach())) * SCALE
    return d, (d - 1e8 * mrow.double()) * SCALE


def reference(inp):
    """float64: out [B, C], attn [B, I], logits (scaled), and per gradient mode ("dout": dattn absent; "dattn": dout zero; "both") dq
    [B, C], dk, dv [U, I, C] (form "same": dx in both), dlogits [B, I] (the gradient of the raw dot products), by autograd; the
    folded form's dq0, dW, db by the chain rule through q = q0 W (applied explicitly, in float64)."""
    q = inp["q"].double().requires_grad_(True)
    ks = inp["k"].double().requires_grad_(True)
    vs = ks if inp["form"] == "same" else inp["v"].double().requires_grad_(True)
    d, l = logits64(inp, q, ks[inp["inverse"]])
    d.retain_grad()
    a = torch.softmax(l, dim=1)
    out = torch.einsum("bi,bic->bc", a, vs[inp["inverse"]])
    ref = {"out": out.detach(), "attn": a.detach(), "logits": l.detach()}
    grads = {}
    for mode, loss in (("dout", (out * inp["dout"].double()).sum()), ("dattn", (a * inp["dattn"].double()).sum())):
        for t in (q, ks, vs, d):
            t.grad = None
        loss.backward(retain_graph=True)
        z = torch.zeros_like(ks)
        grads[mode] = {"dq": q.grad.clone(), "dk": ks.grad.clone() if ks.grad is not None else z,
                       "dv": vs.grad.clone() if vs.grad is not None else z, "dlogits": d.grad.clone()}
    grads["both"] = {n: grads["dout"][n] + grads["dattn"][n] for n in grads["dout"]}
    for g in grads.values():
        if inp["form"] == "same":
            g["dx"] = g["dk"]
            if "W" in inp:
                g["dq0"] = g["dq"] @ inp["W"].double().t()
                g["dW"] = inp["q0"].double().t() @ g["dq"]
    ref["grads"] = grads
    return ref


# ----------------------------------------------------------------------------- bars
def bars(inp, ref, mode="both"):
    """Elementwise bars {name: float64 tensor} of every output, derived from the operands through the summation trees of the kernels;
    first order in u = 2^-24.  A result is inside its bar where |got - ref| <= bar.

    dot       A 256-channel dot product is 4 products and 3 additions in a lane, then 6 exchange levels, then the multiplication by
              scale: depth 11.  |delta l_i| <= 11 u scale sum_c |q_c k_ic|.
    exponent  l_i - M rounds once, and expf reduces its argument with an error relative to it: 3 u |l_i - M| in all.  So
              eps_i = 11 u scale sum_c |q_c k_ic| + 3 u |l_i - M|.
    tokens    A sum over tokens is sequential inside a wave (n_w = trip ceil(I / sweep) tokens) and then summed across the waves:
              D_tok = n_w + waves.
    weights   a_i = e_i / S.  A perturbed logit moves a_i by the relative eps_i + sum_j a_j eps_j (numerator, denominator); S has
              positive terms, so its summation adds D_S u relative: generic D_S = ceil(I / 256) + 6 + 4 (per thread, wave, block),
              same D_S = D_tok + 4 trips (every trip rescales by corr: one expf at 2 u, its argument, one multiplication) + 88 u
              for the arguments m - mx of the rescales, which telescope to at most the span that float32 exp does not flush; expf, 1 / S
              and the product add 4 u.   rho_i = eps_i + sum_j a_j eps_j + (D_S + 4) u [+ 88 u].   bar(attn_i) = a_i rho_i.
    out       sum_i a_i v_ic with every term off by rho_i and the token sum by D_tok + 2:  sum_i |a_i v_ic| (rho_i + (D_tok + 2) u).
    da        da_i = dattn_i + dout . v_i:  eta_i = 11 u sum_c |g_c v_ic| + u |da_i| (absolute).
    s         s = sum_i a_i da_i:  delta_s = sum_i a_i (|da_i| (rho_i + D_s u) + eta_i), D_s = D_S + 1 generic, D_tok + 2 same.
    dlogits   dl_i = a_i (da_i - s) scale:  delta_i = scale a_i (rho_i |da_i - s| + eta_i + delta_s + 3 u |da_i - s|).
    dq        generic, sum_i dl_i k_ic:  sum_i |k_ic| (delta_i + |dl_i| (D_tok + 1) u).
              same, scale (A - s O) with A = sum a_i da_i x_i, O = sum a_i x_i, which cancel:  scale (delta_A + |s| delta_O + |O| delta_s
              + 3 u (|A| + |s O|)), delta_A = sum_i |a_i x_ic| (|da_i| (rho_i + (D_tok + 2) u) + eta_i), delta_O = sum_i |a_i x_ic| (rho_i
              + (D_tok + 1) u).
    dk, dv    dl_i q_c: delta_i |q_c| + u |dl_i q_c|;  a_i g_c: a_i rho_i |g_c| + u |a_i g_c|;  same, dx = their sum, one rounding more.
              Shared sets: the sum of the rows' bars, plus B u sum_b |term| for the caller's sum over the rows of a set (any order).
    folded    dq0 = dq W^T and dW = q0^T dq are matrix products of the caller: |W| and |q0| carry dq's bar, plus n u sum |terms|
              (n = 256 / B) for a float32 sum in any order.
    bf16      outputs stored as bf16 (dk, dv, dx) add one rounding, BF16_EPS |ref|.  Every bar has the floor 2^-120 (flush to zero)."""
    form, I, u = inp["form"], inp["I"], U32
    trip, waves = FORMS[form]["trip"], FORMS[form]["waves"]
    trips = math.ceil(I / (trip * waves))
    d_tok = trip * trips + waves
    inv = inp["inverse"]
    q, g = inp["q"].double(), inp["dout"].double()
    k, v = inp["k"].double()[inv], inp["v"].double()[inv]
    a, l = ref["attn"], ref["logits"]
    lm = (l - l.max(dim=1, keepdim=True).values).abs()
    eps = 11 * u * SCALE * torch.einsum("bc,bic->bi", q.abs(), k.abs()) + 3 * u * lm
    d_s = d_tok + 4 * trips if form == "same" else math.ceil(I / 256) + 10
    rho = eps + (a * eps).sum(dim=1, keepdim=True) + (d_s + 4) * u + (88 * u if form == "same" else 0.0)
    out = {"attn": a * rho, "out": torch.einsum("bi,bic->bc", a * (rho + (d_tok + 2) * u), v.abs())}
    if mode is not None:
        gr = ref["grads"][mode]
        if mode == "dattn":
            g = torch.zeros_like(g)
        ga = inp["dattn"].double() if mode != "dout" else torch.zeros_like(a)
        da = ga + torch.einsum("bc,bic->bi", g, v)
        eta = 11 * u * torch.einsum("bc,bic->bi", g.abs(), v.abs()) + u * da.abs()
        s = (a * da).sum(dim=1, keepdim=True)
        d_s2 = d_tok + 2 if form == "same" else d_s + 1
        ds = (a * (da.abs() * (rho + d_s2 * u) + eta)).sum(dim=1, keepdim=True)
        dlc = (da - s).abs()
        ddl = SCALE * a * (rho * dlc + eta + ds + 3 * u * dlc)
        dl = gr["dlogits"]
        out["dlogits"] = ddl
        dk_row = ddl.unsqueeze(2) * q.abs().unsqueeze(1) + u * (dl.unsqueeze(2) * q.unsqueeze(1)).abs()
        dv_row = (a * rho).unsqueeze(2) * g.abs().unsqueeze(1) + u * (a.unsqueeze(2) * g.unsqueeze(1)).abs()
        if form == "same":
            ax = a.unsqueeze(2) * v.abs()
            dA = (ax * (da.abs() * (rho + (d_tok + 2) * u) + eta).unsqueeze(2)).sum(dim=1)
            dO = (ax * (rho + (d_tok + 1) * u).unsqueeze(2)).sum(dim=1)
            O = torch.einsum("bi,bic->bc", a, v)
            A = torch.einsum("bi,bic->bc", a * da, v)
            out["dq"] = SCALE * (dA + s.abs() * dO + O.abs() * ds + 3 * u * (A.abs() + (s * O).abs()))
            out["dx"] = dk_row + dv_row + u * gr["dx"].abs()
            if "W" in inp:
                W, q0 = inp["W"].double(), inp["q0"].double()
                out["dq0"] = out["dq"] @ W.abs().t() + C * u * (gr["dq"].abs() @ W.abs().t())
                out["dW"] = q0.abs().t() @ out["dq"] + inp["B"] * u * (q0.abs().t() @ gr["dq"].abs())
        else:
            out["dq"] = torch.einsum("bi,bic->bc", ddl + dl.abs() * (d_tok + 1) * u, k.abs())
            nb = inp["B"] * u if inp["shared"] else 0.0
            for name, row, term in (("dk", dk_row, dl.unsqueeze(2) * q.unsqueeze(1)), ("dv", dv_row, a.unsqueeze(2) * g.unsqueeze(1))):
                out[name] = torch.zeros(inp["U"], I, C, dtype=torch.float64).index_add_(0, inv, row + nb * term.abs())
        if inp["bf16"]:
            for name in ("dk", "dv", "dx"):
                if name in out:
                    out[name] = out[name] + BF16_EPS * gr[name].abs()
    return {n: b + FLOOR for n, b in out.items()}


def ratio(got, ref, bar):
    """max over the elements of |got - ref| / bar; a NaN or an infinity in got counts as infinite."""
    got = torch.as_tensor(got).double()
    if not bool(torch.isfinite(got).all()):
        return float("inf")
    return float(((got - ref).abs() / bar).max())


def worst_ratios(got, inp, ref, mode="both"):
    """{name: ratio} of a result dict (out, attn and the gradients it holds) against the reference under bars()."""
    b = bars(inp, ref, mode)
    want = dict(ref["grads"][mode]) if mode is not None else {}
    want.update(out=ref["out"], attn=ref["attn"])
    return {n: ratio(got[n], want[n], b[n]) for n in got if n in b}


# ----------------------------------------------------------------------------- the formula in float32, and with one defect
# the outputs that tests/test_gpu_attn_edges.py compares for a per-row form (dlogits leaves only the shared entry points)
COMPARED = {"generic": ("out", "attn", "dq", "dk", "dv"), "same": ("out", "attn", "dq", "dx")}
FAULTS = {   # name -> the forms it can apply to
    "last_token_dropped": ("generic", "same"),
    "tail_mask_ignored": ("generic", "same"),
    "no_rescale": ("same",),
    "no_max_subtraction": ("generic", "same"),
    "tokens_swapped_in_logits": ("same",),
    "empty_wave_weighs_one": ("same",),
    "tail_token_weighs_one": ("same",),
    "dattn_ignored": ("generic", "same"),
    "s_first_sweep_only": ("generic", "same"),
}


def evaluate(inp, dtype=torch.float64, fault=None, mode="both"):
    """policy_ref.attn's formula and its backward (the formulas in the header of attn_bwd_kernel) written out in `dtype`, per-row forms
    only, optionally with ONE defect:
      last_token_dropped        token I - 1 gets no weight
      tail_mask_ignored         the tokens of the last, ragged trip are never masked
      no_rescale                the per-wave online softmax of attn_same_fwd_kernel, with acc and ssum NOT multiplied by corr when the
                                running maximum rises
      no_max_subtraction        exp(l) / sum exp(l) in float32
      tokens_swapped_in_logits  tokens 1 and 2 of every trip of 8 trade logits, not values (a mis-mapped lane in dots8)
      empty_wave_weighs_one     a wave that saw no token enters the combination as one token of logit 0 and value 0 (m = 0, ssum = 1
                                instead of m = -inf, ssum = 0)
      tail_token_weighs_one     the zero-filled tokens past I of the last, ragged trip of 8 enter the softmax with logit 0 (and value 0)
                                instead of -inf, inside a wave that does have tokens
      dattn_ignored             da = dout . v alone
      s_first_sweep_only        s summed over the first sweep's tokens only
    Returns {out, attn, dq, dk, dv | dx, dlogits} as float64."""
    form, I = inp["form"], inp["I"]
    trip, waves = FORMS[form]["trip"], FORMS[form]["waves"]
    assert inp["shared"] is None
    q, k, v = inp["q"].to(dtype), inp["k"].to(dtype), inp["v"].to(dtype)
    g, ga = inp["dout"].to(dtype), inp["dattn"].to(dtype)
    if mode == "dattn":
        g = torch.zeros_like(g)
    if mode == "dout" or fault == "dattn_ignored":
        ga = torch.zeros_like(ga)
    d = torch.einsum("bc,bic->bi", q, k)
    if inp["mask"] is not None:
        m = inp["mask"].clone()
        if fault == "tail_mask_ignored":
            m[:, (I - 1) // trip * trip:] = False
        d = torch.where(m, d - 1e8 if dtype == torch.float64 and inp["kind"] != "grid" else (d.float() - torch.tensor(1e8, dtype=torch.float32)).to(dtype), d)
    l = d * SCALE
    if fault == "tokens_swapped_in_logits":
        l = l.clone()
        i1 = torch.arange(1, I - 1, 8)
        l[:, i1], l[:, i1 + 1] = l[:, i1 + 1].clone(), l[:, i1].clone()
    if fault == "last_token_dropped":
        l = l.clone()
        l[:, I - 1] = float("-inf")
    if fault == "tail_token_weighs_one":
        pad = torch.zeros(l.shape[0], -I % trip, dtype=dtype)
        a = torch.softmax(torch.cat([l, pad], dim=1), dim=1)[:, :I]
        out = torch.einsum("bi,bic->bc", a, v)
    elif fault == "no_max_subtraction":
        e = torch.exp(l.float())
        a = (e / e.sum(dim=1, keepdim=True)).to(dtype)
        out = torch.einsum("bi,bic->bc", a, v)
    elif fault in ("no_rescale", "empty_wave_weighs_one"):
        out, a = _online(l, v, trip, waves, fault)
    else:
        a = torch.softmax(l, dim=1)
        out = torch.einsum("bi,bic->bc", a, v)
    da = ga + torch.einsum("bc,bic->bi", g, v)
    w = a * da
    s = (w[:, :trip * waves] if fault == "s_first_sweep_only" else w).sum(dim=1, keepdim=True)
    dl = a * (da - s) * SCALE
    dk = dl.unsqueeze(2) * q.unsqueeze(1)
    dv = a.unsqueeze(2) * g.unsqueeze(1)
    res = {"out": out, "attn": a, "dlogits": dl, "dq": torch.einsum("bi,bic->bc", dl, k)}
    if form == "same":
        res["dx"] = dk + dv
    else:
        res["dk"], res["dv"] = dk, dv
    if inp["bf16"]:
        for n in ("dk", "dv", "dx"):
            if n in res:
                res[n] = bf_round(res[n].float())
    return {n: t.double() for n, t in res.items()}


def _online(l, x, trip, waves, fault):
    """attn_same_fwd_kernel's bookkeeping in l's dtype: per wave a running maximum m, a sum ssum and an accumulator acc over its trips,
    combined through wm / wsum at the end."""
    B, I = l.shape
    ninf = float("-inf")
    wm = torch.full((B, waves), ninf, dtype=l.dtype)
    wsum = torch.zeros(B, waves, dtype=l.dtype)
    part = torch.zeros(B, waves, x.shape[2], dtype=l.dtype)
    for w in range(waves):
        m = torch.full((B, 1), ninf, dtype=l.dtype)
        ssum = torch.zeros(B, 1, dtype=l.dtype)
        acc = torch.zeros(B, x.shape[2], dtype=l.dtype)
        for i0 in range(w * trip, I, trip * waves):
            lt = l[:, i0:min(i0 + trip, I)]
            mx = torch.maximum(m, lt.max(dim=1, keepdim=True).values)
            if fault != "no_rescale":
                corr = torch.exp(m - mx)
                ssum, acc = ssum * corr, acc * corr
            e = torch.exp(lt - mx)
            ssum = ssum + e.sum(dim=1, keepdim=True)
            acc = acc + torch.einsum("bi,bic->bc", e, x[:, i0:i0 + lt.shape[1]])
            m = mx
        if w * trip >= I and fault == "empty_wave_weighs_one":
            m, ssum = torch.zeros_like(m), torch.ones_like(ssum)
        wm[:, w], wsum[:, w], part[:, w] = m[:, 0], ssum[:, 0], acc
    M = wm.max(dim=1, keepdim=True).values
    f = torch.exp(wm - M)
    S = (wsum * f).sum(dim=1, keepdim=True)
    return (part * f.unsqueeze(2)).sum(dim=1) / S, torch.exp(l - M) / S
