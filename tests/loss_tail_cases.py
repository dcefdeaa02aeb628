"""Inputs and bars shared by test_loss_tail_cpu.py and test_gpu_loss_tail.py: the cases of the loss tail whose sums are longer
than the bench shape's, so that the CPU file can show that each bar is one the reference arithmetic itself meets in float32."""
import math

import torch

# (T, N, A, ld_waypoint) of ops.dagger_loss.  dagger_loss_fwd_kernel stages DL_CHUNK = 2048 rows at a time, whole steps only
# (tpc = 2048 // N steps per chunk), and adds an episode's terms in step order:
#   (200, 11, 2, 3)   2200 rows, tpc = 186, a second chunk of 14 steps (the trainer's 200-step cap with 11 episodes)
#   (9, 256, 2, 2)    N at the ABI limit, tpc = 8, a second chunk of 1 step
#   (2049, 1, 3, 4)   one episode, a second chunk of a single row
#   (16, 128, 4, 4)   exactly 2048 rows: one full chunk and no second trip
DAGGER_CASES = [(200, 11, 2, 3), (9, 256, 2, 2), (2049, 1, 3, 4), (16, 128, 4, 4)]
DAGGER_IDS = ["T200xN11_two_chunks", "N256_limit", "T2049_one_episode", "exactly_one_chunk"]
DAGGER_DEAD = (200, 11, 2, 3, 4)      # the first case with episode 4 given all-zero weights

AUX_B = [1, 255, 257, 4099]
AUX_L = [1, 4]
AUX_ALPHAS = (0.1, 0.5, 1.0, 0.25)


def long_sum_bar(terms):
    """The bar of a float32 sum of `terms` numbers added one after the other: the existing direct tests' 2e-6 until the
    worst-case bound of the sequential sum, terms * 2^-24 (each of the terms - 1 additions rounds by at most half an ulp of a
    partial sum that is at most the sum of the magnitudes), is larger.  Relative to max(1, |ref|) for a value and to max |grad|
    for a gradient.

    What the reference's own lines give in float32 on the CPU against float64 (oracle/tail_ref.py; measured by
    test_loss_tail_cpu.py, which asserts each one under its bar):
        dagger (200, 11, 2, 3)    bar 1.19e-05   loss 1.2e-08   d pred 1.8e-07
        dagger (9, 256, 2, 2)     bar 2.00e-06   loss 1.0e-09   d pred 8.7e-08
        dagger (2049, 1, 3, 4)    bar 1.22e-04   loss 5.6e-08   d pred 2.3e-07
        dagger (16, 128, 4, 4)    bar 2.00e-06   loss 1.2e-08   d pred 1.9e-07
        aux_reduce B = 4099, L = 1 (17 terms per thread)   bar 2.00e-06   value 1.3e-08   d rows 0.0e+00
        aux_reduce B = 4099, L = 4                         bar 2.00e-06   value 3.1e-08   d rows 1.0e-08
    """
    return max(2e-6, terms * 2.0 ** -24)


def aux_terms(B):
    """Terms one thread of aux_reduce_fwd_kernel adds: it strides the B rows by 256."""
    return math.ceil(B / 256)


def _gen(*key):
    g = torch.Generator()
    g.manual_seed(sum(int(k) * m for k, m in zip(key, (1000003, 10007, 101, 7, 3))) + 17)
    return g


def dagger_inputs(T, N, A, ld, dead=None):
    """CPU float32 (pred [T*N, A], waypoint [T*N, ld], weights [T, N]): weights rand + 0.1 with the trailing steps of two
    episodes zeroed (padded steps); `dead`: an episode whose weights are all zero."""
    g = _gen(T, N, A, ld)
    pred = torch.randn(T * N, A, generator=g)
    waypoint = torch.rand(T * N, ld, generator=g) * 2 - 1
    weights = torch.rand(T, N, generator=g) + 0.1
    weights[T - 2:, 0] = 0.0
    if N > 1:
        weights[T - 5:, N - 1] = 0.0
    if dead is not None:
        weights[:, dead] = 0.0
    return pred, waypoint, weights


def aux_inputs(B, L, kind="random"):
    """CPU (rows: L float32 [B] vectors, alphas, mask [B] bool).  kind: "random" (about 70 % selected, at least one), "empty"
    (nothing selected), "one" (a single row selected).  Every unselected row holds NaN in every other vector, the first included:
    the log of an underflowed attention weight on a padded row, which a masked MEAN drops and a multiplication by zero would not."""
    g = _gen(B, L, 5)
    rows = [torch.rand(B, generator=g) * 2 for _ in range(L)]
    if kind == "random":
        mask = torch.rand(B, generator=g) < 0.7
        mask[B // 2] = True
    elif kind == "empty":
        mask = torch.zeros(B, dtype=torch.bool)
    else:
        mask = torch.zeros(B, dtype=torch.bool)
        mask[(B * 2) // 3] = True
    for k in range(0, L, 2):
        rows[k] = rows[k].masked_fill(~mask, float("nan"))
    return rows, AUX_ALPHAS[:L], mask
