"""The yardstick of the attention / action / progress scoring (csrc/wsmg_nav_eval.hip, ops.nav_rows, NavigationMeter.rows_from):
a brute-force row record written independently of `rows_from` — plain Python loops over cells, math.floor / math.ceil for the
area windows, float64 arithmetic (the cell sums alone in float32, one np.float32 addition at a time, row-major) — the input cases
both test files share, and the comparison with its bounds.

Bounds.  Integer fields (states, cells, Chebyshev distance, stop code) are compared for equality, NaN positions must coincide.  A
float field is held to (n + 8) * 2^-52 * sum|terms| with n its term count: S*S for the entropy (terms a log a), 9 for the mass
(terms a), 1 for the distance and the progress fields (the field itself), A for the action fields.  The action's terms are those
of the expression in its inputs, t_j = tanh(pred_j) and w_j: e_j = t_j - w_j cancels, so two correct double-precision tanh that
differ by one ulp of t_j (numpy's and libm's do) differ in e_j by 2^-53 |t_j| however small e_j is, and a bound on |e_j| itself
cannot hold.  |e_j|: |t_j| + |w_j|;  sum e^2 = sum t^2 - 2 t w + w^2: sum_j (|t_j| + |w_j|)^2;  its root: the deviation is
|sum e_j d_j| / root <= sqrt(sum d_j^2), so sqrt(sum_j (|t_j| + |w_j|)^2)."""
import math

import numpy as np
import torch

R = 18
ATT_STATE, ATT_TARGET, ATT_PEAK, ATT_CHEB, ATT_EUCLID, ATT_MASS, ATT_ENTROPY = range(7)
ACT_STATE, ACT_SQ, ACT_L2, ACT_ABS = 7, 8, 9, 10
PROG_STATE, PROG_ABS, PROG_SQ, PROG_STOP = 14, 15, 16, 17
ABSENT, COUNTED, INVALID = 0.0, 1.0, 2.0
INT_FIELDS = (ATT_STATE, ATT_TARGET, ATT_PEAK, ATT_CHEB, ACT_STATE, PROG_STATE, PROG_STOP)
SUM_FIELDS = (3, 4, 5, 6, 8, 9, 10, 11, 12, 13, 15, 16)
GROUP_FIELDS = {ATT_STATE: range(1, 7), ACT_STATE: range(8, 14), PROG_STATE: range(15, 18)}
EPS = 2.0 ** -52
THR = 0.8          # PROG_THRESHOLD of the reference's config


def _np(t):
    return None if t is None else (t.detach().cpu().numpy() if torch.is_tensor(t) else np.asarray(t))


def window(i, L, S):
    return math.floor(i * L / S), math.ceil((i + 1) * L / S)


def brute_cells(dis_row, S):
    """Means of the S x S area windows of one [H, W] map: float32 sums in row-major order, one addition at a time."""
    H, W = dis_row.shape
    out = []
    for cy in range(S):
        y0, y1 = window(cy, H, S)
        for cx in range(S):
            x0, x1 = window(cx, W, S)
            acc = np.float32(0.0)
            for y in range(y0, y1):
                for x in range(x0, x1):
                    acc = np.float32(acc + dis_row[y, x])
            out.append(np.float32(acc / np.float32((y1 - y0) * (x1 - x0))))
    return out


def brute_rows(att=None, dis=None, S=0, pred=None, waypoint=None, prog=None, progress=None, mask=None, stop_threshold=THR, B=None):
    """float64 [B, 18] by loops; every pair may be None."""
    att, dis, pred, waypoint, prog, progress, mask = (_np(t) for t in (att, dis, pred, waypoint, prog, progress, mask))
    for t in (att, pred, prog, mask):
        if t is not None and B is None:
            B = t.shape[0]
    nan = float("nan")
    rows = []
    with np.errstate(all="ignore"):
        for b in range(B):
            row = [nan] * R
            row[ATT_STATE] = row[ACT_STATE] = row[PROG_STATE] = ABSENT
            on = mask is None or bool(mask.reshape(-1)[b])
            if att is not None and on:
                a = [float(v) for v in att[b]]
                if any(v != v or v < 0 for v in a) or bool(np.isnan(dis[b]).any()):
                    row[ATT_STATE] = INVALID
                else:
                    cells = brute_cells(dis[b], S)
                    target, best = 0, math.inf
                    for c, v in enumerate(cells):
                        v = math.inf if v != v else float(v)
                        if v < best:
                            target, best = c, v
                    peak = 0
                    for c, v in enumerate(a):
                        if v > a[peak]:
                            peak = c
                    ty, tx, py, px = target // S, target % S, peak // S, peak % S
                    mass = 0.0
                    for y in range(max(ty - 1, 0), min(ty + 1, S - 1) + 1):
                        for x in range(max(tx - 1, 0), min(tx + 1, S - 1) + 1):
                            mass += a[y * S + x]
                    row[ATT_STATE:ATT_ENTROPY + 1] = [COUNTED, float(target), float(peak), float(max(abs(py - ty), abs(px - tx))),
                                                      math.sqrt((py - ty) ** 2 + (px - tx) ** 2), mass,
                                                      -math.fsum(v * math.log(v) for v in a if v > 0)]
            if pred is not None and on:
                A = pred.shape[1]
                p, w = [float(v) for v in pred[b]], [float(v) for v in waypoint[b, :A]]
                if not all(math.isfinite(v) for v in p + w):
                    row[ACT_STATE] = INVALID
                else:
                    e = [math.tanh(p[j]) - w[j] for j in range(A)]
                    sq = 0.0
                    for v in e:
                        sq += v * v
                    row[ACT_STATE:ACT_ABS + 4] = [COUNTED, sq, math.sqrt(sq)] + [abs(v) for v in e] + [0.0] * (4 - A)
            if prog is not None and on:
                p, q = np.float32(prog.reshape(-1)[b]), np.float32(progress.reshape(-1)[b])
                if not (math.isfinite(p) and math.isfinite(q)):
                    row[PROG_STATE] = INVALID
                else:
                    d = float(p) - float(q)
                    thr = np.float32(stop_threshold)
                    row[PROG_STATE:PROG_STOP + 1] = [COUNTED, abs(d), d * d, float(2 * int(q >= thr) + int(p >= thr))]
            rows.append(row)
    return np.array(rows, np.float64).reshape(B, R)


def bounds(want, att=None, S=0, pred=None, waypoint=None, **_):
    """float64 [B, 18]: the largest |difference| allowed per field against the record `want` (0 for the integer fields)."""
    want = _np(want)
    B = want.shape[0]
    tol = np.zeros((B, R))
    mag = np.abs(np.nan_to_num(want, nan=0.0))
    tol[:, ATT_EUCLID] = 9 * EPS * mag[:, ATT_EUCLID]
    tol[:, ATT_MASS] = 17 * EPS * mag[:, ATT_MASS]
    if att is not None:
        a = _np(att).astype(np.float64)
        with np.errstate(all="ignore"):
            terms = np.where(a > 0, np.abs(a * np.log(np.where(a > 0, a, 1.0))), 0.0).sum(1)
        tol[:, ATT_ENTROPY] = (S * S + 8) * EPS * np.nan_to_num(terms, nan=0.0, posinf=0.0)
    if pred is not None:
        p, w = _np(pred).astype(np.float64), _np(waypoint).astype(np.float64)
        A = p.shape[1]
        with np.errstate(all="ignore"):
            m = np.nan_to_num(np.abs(np.tanh(p)) + np.abs(w[:, :A]), nan=0.0, posinf=0.0)
        tol[:, ACT_SQ] = (A + 8) * EPS * (m * m).sum(1)
        tol[:, ACT_L2] = (A + 8) * EPS * np.sqrt((m * m).sum(1))
        tol[:, ACT_ABS:ACT_ABS + A] = (A + 8) * EPS * m
    for f in (PROG_ABS, PROG_SQ):
        tol[:, f] = 9 * EPS * mag[:, f]
    return tol


def compare(got, want, tol, what=""):
    """Assert the record `got` against `want` within `tol`; -> the largest |difference| / bound over the float fields (0 / 0 = 0)."""
    got, want = _np(got), _np(want)
    assert got.shape == want.shape and got.dtype == np.float64, f"{what}: shape {got.shape} {got.dtype} against {want.shape}"
    assert np.array_equal(np.isnan(got), np.isnan(want)), f"{what}: NaN positions differ\n{got}\n{want}"
    worst = 0.0
    for f in range(R):
        g, w = got[:, f], want[:, f]
        ok = ~np.isnan(w)
        if f in INT_FIELDS:
            assert np.array_equal(g[ok], w[ok]), f"{what}: field {f} differs: {g} against {w}"
            continue
        diff = np.abs(g[ok] - w[ok])
        assert (diff <= tol[ok, f]).all(), f"{what}: field {f} off by {diff.max()} (bound {tol[ok, f]}): {g} against {w}"
        with np.errstate(all="ignore"):
            ratio = np.where(diff > 0, diff / tol[ok, f], 0.0)
        worst = max(worst, float(ratio.max(initial=0.0)))
    return worst


def states(rows):
    rows = _np(rows)
    return [tuple(int(v) for v in r) for r in rows[:, [ATT_STATE, ACT_STATE, PROG_STATE]]]


def brute_totals(rows_list):
    """(counts [13], sums [12]) of the records in order: every sum adds the counted rows one at a time in float64."""
    c, s = [0] * 13, [0.0] * 12
    for rows in rows_list:
        for r in _np(rows):
            for k, st in enumerate((ATT_STATE, ACT_STATE, PROG_STATE)):
                c[(0, 5, 7)[k]] += int(r[st] == COUNTED)
                c[(1, 6, 8)[k]] += int(r[st] == INVALID)
            if r[ATT_STATE] == COUNTED:
                for k in range(3):
                    c[2 + k] += int(r[ATT_CHEB] <= k)
            if r[PROG_STATE] == COUNTED:
                c[9 + int(r[PROG_STOP])] += 1
            for k, f in enumerate(SUM_FIELDS):
                st = PROG_STATE if f >= PROG_STATE else ACT_STATE if f >= ACT_STATE else ATT_STATE
                if r[st] == COUNTED:
                    s[k] += float(r[f])
    return c, s


# ----------------------------------------------------------------------------- the cases
# (H, W, S): windows of 5 and 6; ratio 2.5; non-square and odd; identity; H < S; a map row longer than the kernel's 10 240-float
# band (the cells then read global memory directly)
SHAPES = [(100, 100, 24), (10, 10, 4), (7, 5, 4), (4, 4, 4), (3, 3, 4), (2, 10243, 3)]


def random_case(B, H, W, S, A=2, seed=0, ld=3):
    """dis integer-valued in [0, 50] (every window sum exact in float32), att a softmax row, pred ~ N(0, 1), waypoint [B, ld] in
    [-1, 1), prog and progress in [0, 1)."""
    g = torch.Generator().manual_seed(1000 * seed + 7 * B + H + S)
    return dict(att=torch.softmax(2.0 * torch.randn(B, S * S, generator=g), 1), dis=torch.randint(0, 51, (B, H, W), generator=g).float(),
                S=S, pred=torch.randn(B, A, generator=g), waypoint=torch.rand(B, ld, generator=g) * 2 - 1,
                prog=torch.rand(B, 1, generator=g), progress=torch.rand(B, 1, generator=g))


def _put_target(dis, b, cell, S):
    """Make `cell` the only cell of row b whose window is all zero (every other cell keeps a 50 in its window)."""
    H, W = dis.shape[1:]
    dis[b] = 50.0
    y0, y1 = window(cell // S, H, S)
    x0, x1 = window(cell % S, W, S)
    dis[b, y0:y1, x0:x1] = 0.0


def ties_case():
    """Row 1: two cells with mean exactly 0 (targets 50 and 300: the lower wins); row 3: two equal attention maxima (peaks 77, 401)."""
    c = random_case(5, 100, 100, 24, seed=3)
    _put_target(c["dis"], 1, 300, 24)
    y0, y1 = window(50 // 24, 100, 24)
    x0, x1 = window(50 % 24, 100, 24)
    c["dis"][1, y0:y1, x0:x1] = 0.0
    c["att"][3] *= 0.5
    c["att"][3, 401] = c["att"][3, 77] = 0.25
    return c


def edges_case(S=24, H=100, W=100):
    """Target at the four corners and on the top edge, the attention's peak in the opposite corner / on the opposite edge."""
    c = random_case(5, H, W, S, seed=4)
    last, mid = S - 1, S // 2
    targets = [0, last, last * S, last * S + last, mid]
    peaks = [last * S + last, last * S, last, 0, last * S + mid]
    for b, (t, p) in enumerate(zip(targets, peaks)):
        _put_target(c["dis"], b, t, S)
        c["att"][b] *= 0.1
        c["att"][b, p] = 0.9
    return c, targets, peaks


def invalid_case():
    """One bad value per row, each in one group: NaN in att, a negative att, NaN in dis, Inf in pred, NaN in progress."""
    c = random_case(5, 10, 10, 4, seed=5)
    c["att"][0, 5] = float("nan")
    c["att"][1, 15] = -1e-3
    c["dis"][2, 9, 9] = float("nan")
    c["pred"][3, 1] = float("inf")
    c["progress"][4, 0] = float("nan")
    want = [(2, 1, 1), (2, 1, 1), (2, 1, 1), (1, 2, 1), (1, 1, 2)]
    return c, want


def stop_case():
    """prog x progress over { one float32 ulp below the threshold, the threshold, one ulp above }: nine rows."""
    t = np.float32(THR)
    v = np.array([np.nextafter(t, np.float32(0)), t, np.nextafter(t, np.float32(1))], np.float32)
    prog, progress = np.repeat(v, 3), np.tile(v, 3)
    codes = [2 * int(q >= t) + int(p >= t) for p, q in zip(prog, progress)]
    return dict(prog=torch.from_numpy(prog.copy()), progress=torch.from_numpy(progress.copy())), codes


def group_args(c, groups=("att", "act", "prog")):
    """The keyword arguments of rows_from / brute_rows / ops.nav_rows for the chosen groups of a case."""
    kw = {}
    if "att" in groups:
        kw.update(att=c["att"], dis=c["dis"], S=c["S"])
    if "act" in groups:
        kw.update(pred=c["pred"], waypoint=c["waypoint"])
    if "prog" in groups:
        kw.update(prog=c["prog"], progress=c["progress"])
    return kw
