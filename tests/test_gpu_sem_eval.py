"""GPU: scoring the semantic-map head on the device — wsmg_sem_confusion_f32 / _bf16 and wsmg_sem_scores (csrc/wsmg_sem_eval.hip)
through ops.sem_confusion / ops.sem_scores, wsmgmap.metrics.SemanticMapMeter and BasePolicy.semantic_prediction, against the
numpy / torch oracle of tests/sem_eval_util.py.  Counts and predictions are compared by exact equality: the kernel does no
arithmetic on the logits and adds integers.  The scores are one float64 division per figure on exact integers: the host form
(SemanticMapMeter.score_vector) is the truth and the device may differ by 4 ulp of float64 (measured on an MI355X: 0 ulp at every
figure of every matrix below)."""
import copy
import functools

import numpy as np
import pytest
import torch

from oracle import cases
from sem_eval_util import NO_PRED, make_gt, make_logits, oracle, resized_labels, sampled_sources
from util import T, state_dict_values

pytestmark = pytest.mark.gpu

DTYPES = {"f32": torch.float32, "bf16": torch.bfloat16}
# (B, H, W, Hg, Wg, classes): the policy's shape; both scales non-integer, one axis up-sampled, W % 16 != 0, less than a workgroup;
# one pixel; a pixel count that is no multiple of a workgroup's share (1 024 pixels per trip), no padding channels
SHAPES = [(3, 48, 48, 100, 100, 27), (2, 6, 10, 13, 7, 5), (1, 1, 1, 1, 1, 1), (2, 33, 17, 100, 100, 32)]


def _run(logits, gt, classes, **kw):
    from wsmgmap import ops
    conf, ign, pred = ops.sem_confusion(logits.cuda(), None if gt is None else gt.cuda(), classes, want_pred=True,
                                        **{k: (v.cuda() if torch.is_tensor(v) else v) for k, v in kw.items()})
    torch.cuda.synchronize()
    return (None if conf is None else conf.cpu().numpy()), (None if ign is None else ign.cpu().numpy()), pred.cpu().numpy()


def _same(got, want, what=""):
    for g, w, name in zip(got, want, ("confusion", "ignored", "pred")):
        assert g.dtype == w.dtype and g.shape == w.shape and np.array_equal(g, w), f"{what}: {name} differs from the oracle"


# ----------------------------------------------------------------------------- 1. shapes
@pytest.mark.parametrize("dtype", list(DTYPES))
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_shapes_match_the_oracle_exactly(shape, dtype):
    B, H, W, Hg, Wg, classes = shape
    logits, gt = make_logits(B, H, W, classes, DTYPES[dtype], seed=B * H + W), make_gt(B, Hg, Wg, classes, seed=Hg)
    want = oracle(logits, gt, classes)
    assert want[0].sum() == B * H * W and not want[1].any()          # labels uniform in [0, classes): every pixel is counted
    _same(_run(logits, gt, classes), want, str(shape))


# ----------------------------------------------------------------------------- 2. ties and padding
def _four_valued(B, H, W, seed):
    g = torch.Generator().manual_seed(seed)
    vals = torch.tensor([-1.5, 0.0, 0.25, 3.0])
    return vals[torch.randint(0, 4, (B, H, W, 32), generator=g)].to(torch.bfloat16)


def test_ties_go_to_the_lowest_class():
    B, H, W, classes = 2, 20, 24, 27
    logits, gt = _four_valued(B, H, W, 5), make_gt(B, 100, 100, classes, seed=6)
    x = logits.float()[..., :classes]
    tied = ((x == x.max(-1, keepdim=True).values).sum(-1) > 1).float().mean()
    assert tied > 0.9, "the inputs were meant to tie at most pixels"
    want = oracle(logits, gt, classes)
    got = _run(logits, gt, classes)
    _same(got, want)
    assert np.array_equal(got[2], (x == x.max(-1, keepdim=True).values).float().argmax(-1).numpy().astype(np.uint8))


@pytest.mark.parametrize("dtype", list(DTYPES))
@pytest.mark.parametrize("fill", [1e30, float("nan")], ids=["huge", "nan"])
def test_padding_channels_never_win_whatever_they_hold(fill, dtype):
    B, H, W, classes = 2, 20, 24, 27
    logits, gt = make_logits(B, H, W, classes, DTYPES[dtype], seed=11), make_gt(B, 100, 100, classes, seed=12)
    plain = _run(logits, gt, classes)
    padded = logits.clone()
    padded[..., classes:] = fill
    got = _run(padded, gt, classes)
    _same(got, oracle(logits, gt, classes))
    _same(got, plain, "against the run with ordinary padding")
    assert not got[1].any() and got[2].max() < classes


@pytest.mark.parametrize("dtype", list(DTYPES))
def test_signed_zeros_tie_and_infinities_are_ordinary(dtype):
    classes, inf = 27, float("inf")
    rows = torch.full((6, 32), -2.0)
    rows[0, 0], rows[0, 3] = -0.0, 0.0              # -0.0 first: +0.0 is not greater -> class 0
    rows[1, 2], rows[1, 9] = 0.0, -0.0              # +0.0 first -> class 2
    rows[2, 5] = inf                                # +Inf wins
    rows[3, :] = -inf                               # all -Inf -> class 0
    rows[4, 7], rows[4, 20] = inf, inf              # two +Inf tie -> 7
    rows[5, :classes], rows[5, 26] = -inf, -1e30    # a finite value beats -Inf
    logits = rows.view(1, 2, 3, 32).to(DTYPES[dtype])
    gt = torch.zeros(1, 4, 4)
    want = oracle(logits, gt, classes)
    assert want[2].reshape(-1).tolist() == [0, 2, 5, 0, 7, 26]
    _same(_run(logits, gt, classes), want)


# ----------------------------------------------------------------------------- 3. bad pixels
@pytest.mark.parametrize("dtype", list(DTYPES))
def test_bad_labels_and_nan_logits_are_counted_apart(dtype):
    B, H, W, Hg, Wg, classes = 3, 48, 48, 100, 100, 27
    logits, gt = make_logits(B, H, W, classes, DTYPES[dtype], seed=21), make_gt(B, Hg, Wg, classes, seed=22)
    ys, xs = sampled_sources(H, W, Hg, Wg)
    assert len(ys) == H and len(xs) == W
    bad = [-1.0, -0.5, 26.9, 27.0, 1e20, float("nan"), float("inf"), -float("inf")]
    for i, v in enumerate(bad):                     # three sampled positions per value, one in every row of the batch
        for b in range(B):
            gt[b, ys[3 * i + b], xs[40 - 2 * i - b]] = v
    lab = resized_labels(gt, H, W)                  # on the CPU first: the resize really reads every one of them
    for v in bad:
        n = int(np.isnan(lab).sum()) if v != v else int((lab == np.float32(v)).sum())
        assert n >= B, f"the nearest resize does not sample the {v} labels"
    # NaN logits: in channel 0, in the last class, in every channel; one of them on a pixel whose label is invalid as well
    logits[0, 3, 4, 0] = float("nan")
    logits[1, 7, 47, classes - 1] = float("nan")
    logits[2, 47, 0, :] = float("nan")
    by, bx = np.argwhere(np.isnan(lab[0]))[0]
    logits[0, by, bx, 5] = float("nan")
    want = oracle(logits, gt, classes)
    invalid = B * 6                                 # -1, 27, 1e20, NaN, +Inf, -Inf; -0.5 and 26.9 are valid (0 and 26)
    assert want[1].tolist() == [invalid, 3] and int((want[2] == NO_PRED).sum()) == 4
    assert want[0].sum() == B * H * W - invalid - 3 and want[0].sum() >= 0.9 * B * H * W
    _same(_run(logits, gt, classes), want)


# ----------------------------------------------------------------------------- 4. accumulation and the mask
def test_calls_accumulate_and_counts_pass_2_to_32():
    from wsmgmap import ops
    B, H, W, classes = 2, 20, 24, 27
    gt = make_gt(B, 100, 100, classes, seed=32)
    a, b = make_logits(B, H, W, classes, torch.bfloat16, seed=30), make_logits(B, H, W, classes, torch.float32, seed=31)
    wa, wb = oracle(a, gt, classes), oracle(b, gt, classes)
    cell = np.unravel_index(np.argmax(wa[0] + wb[0]), wa[0].shape)
    conf = torch.zeros(classes, classes, dtype=torch.int64, device="cuda")
    ign = torch.zeros(2, dtype=torch.int64, device="cuda")
    conf[cell] = (1 << 32) - 1
    ign[0] = (1 << 32) - 1
    gt_bad = gt.clone()
    gt_bad[:, 0, 0] = -1.0                          # source (0, 0) is always sampled: ignored[0] steps past 2^32 too
    wb = oracle(b, gt_bad, classes)
    r1 = ops.sem_confusion(a.cuda(), gt.cuda(), classes, conf, ign)
    r2 = ops.sem_confusion(b.cuda(), gt_bad.cuda(), classes, conf, ign)
    assert r1[0] is conf and r2[1] is ign and r1[2] is None
    want = wa[0] + wb[0]
    want[cell] += (1 << 32) - 1
    assert (wa[0] + wb[0])[cell] >= 2 and want[cell] > (1 << 32)
    assert np.array_equal(conf.cpu().numpy(), want)
    assert wb[1][0] >= 1 and ign.cpu().tolist() == [(1 << 32) - 1 + int(wa[1][0] + wb[1][0]), 0]


@pytest.mark.parametrize("mask_dtype", [torch.bool, torch.uint8])
def test_row_mask_switches_rows_off(mask_dtype):
    B, H, W, classes = 5, 12, 16, 27
    logits, gt = make_logits(B, H, W, classes, torch.bfloat16, seed=40), make_gt(B, 30, 30, classes, seed=41)
    mask = torch.tensor([1, 0, 1, 1, 0]).to(mask_dtype)
    want = oracle(logits, gt, classes, mask)
    assert want[0].sum() == 3 * H * W and (want[2][1] == NO_PRED).all() and (want[2][0] != NO_PRED).all()
    _same(_run(logits, gt, classes, row_mask=mask), want)


def test_all_rows_off_changes_nothing():
    from wsmgmap import ops
    B, H, W, classes = 3, 12, 16, 27
    logits, gt = make_logits(B, H, W, classes, torch.float32, seed=42), make_gt(B, 30, 30, classes, seed=43)
    conf = torch.randint(0, 1 << 40, (classes, classes), device="cuda")
    ign = torch.tensor([7, 1 << 35], device="cuda")
    before = (conf.clone(), ign.clone())
    _, _, pred = ops.sem_confusion(logits.cuda(), gt.cuda(), classes, conf, ign, row_mask=torch.zeros(B, dtype=torch.bool, device="cuda"),
                                   want_pred=True)
    assert torch.equal(conf, before[0]) and torch.equal(ign, before[1]) and bool((pred == NO_PRED).all())


# ----------------------------------------------------------------------------- 5. scores
def _ulps(got, want):
    """Largest |got - want| in units of float64 ulp(want) over the finite entries; NaN positions must coincide."""
    assert np.array_equal(np.isnan(got), np.isnan(want)), "NaN positions differ"
    ok = ~np.isnan(want)
    return float(np.max(np.abs(got[ok] - want[ok]) / np.spacing(np.abs(want[ok])), initial=0.0))


def test_scores_match_the_host_form_within_4_ulp():
    from wsmgmap import ops
    from wsmgmap.metrics import SemanticMapMeter
    classes = 27
    dense = oracle(make_logits(3, 48, 48, classes, torch.float32, seed=50), make_gt(3, 100, 100, classes, seed=51), classes)[0]
    sparse = dense.copy()
    sparse[[3, 11, 26], :] = 0
    sparse[:, [3, 11, 26]] = 0                       # three classes absent on both sides: NaN IoU, left out of the mean
    g = torch.Generator().manual_seed(52)
    big = torch.randint(0, 1 << 42, (classes, classes), generator=g).numpy()          # every sum < 2^52: exact as doubles
    mats = dict(dense=dense, sparse=sparse, empty=np.zeros((classes, classes), np.int64), big=big,
                small=np.array([[3, 1, 0], [2, 2, 0], [0, 0, 0]], np.int64), one=np.array([[5]], np.int64))
    worst = 0.0
    for name, m in mats.items():
        want = SemanticMapMeter.score_vector(torch.from_numpy(m)).numpy()
        got = ops.sem_scores(torch.from_numpy(m).cuda()).cpu().numpy()
        u = _ulps(got, want)
        print(f"sem_scores[{name}]: worst difference {u} ulp; miou {got[2]!r} pixel accuracy {got[1]!r}")
        worst = max(worst, u)
        assert u <= 4.0, f"{name}: {u} ulp"
        c = m.shape[0]
        assert got[0] == m.sum() and np.array_equal(got[4::3], m.sum(1)) and np.array_equal(got[5::3], m.sum(0)) and got.size == 3 + 3 * c
    assert np.isnan(ops.sem_scores(torch.from_numpy(mats["sparse"]).cuda()).cpu().numpy()[3 + 3 * 11])
    print(f"sem_scores: worst difference over all matrices {worst} ulp")


def test_meter_compute_reset_and_state_dict():
    from wsmgmap.metrics import SemanticMapMeter
    classes = 5
    logits, gt = make_logits(2, 6, 10, classes, torch.bfloat16, seed=60).cuda(), make_gt(2, 13, 7, classes, seed=61)
    gt[0, 0, 0] = float("nan")
    want = oracle(logits, gt, classes)

    class Net:
        sem_logits_nhwc = logits
    meter = SemanticMapMeter(classes=classes)
    meter.update(Net(), {"gt_semantic_map": gt.cuda()})
    out = meter.compute()
    ref = SemanticMapMeter.scores_from(torch.from_numpy(want[0]), torch.from_numpy(want[1]))
    assert out["pixels"] == int(want[0].sum()) and out["ignored_labels"] == int(want[1][0]) >= 1 and out["nan_pixels"] == 0
    assert out["gt_pixels"] == ref["gt_pixels"] and out["pred_pixels"] == ref["pred_pixels"] and len(out["iou"]) == classes
    assert abs(out["miou"] - ref["miou"]) <= 4 * np.spacing(ref["miou"]) and abs(out["pixel_accuracy"] - ref["pixel_accuracy"]) <= 4 * np.spacing(ref["pixel_accuracy"])
    state = meter.state_dict()
    other = SemanticMapMeter(classes=classes)
    other.load_state_dict({k: (v.cpu() if torch.is_tensor(v) else v) for k, v in state.items()})       # a checkpoint read to the host
    other.update(Net(), {"gt_semantic_map": gt.cuda()})
    assert np.array_equal(other.confusion.cpu().numpy(), 2 * want[0]) and other.ignored.cpu().tolist() == (2 * want[1]).tolist()
    meter.reset()
    assert not meter.confusion.any() and not meter.ignored.any() and meter.compute()["pixels"] == 0
    assert np.array_equal(other.confusion.cpu().numpy(), 2 * want[0])           # its own storage


def test_meter_refuses_what_it_cannot_score():
    from wsmgmap import _abi
    from wsmgmap.metrics import SemanticMapMeter

    class Net:
        sem_logits_nhwc = None
    meter = SemanticMapMeter()
    gt = torch.zeros(2, 100, 100, device="cuda")
    with pytest.raises(_abi.WsmgError, match="no forward pass"):
        meter.update(Net(), {"gt_semantic_map": gt})
    Net.sem_logits_nhwc = torch.zeros(2, 48, 48, 32, device="cuda")
    with pytest.raises(_abi.WsmgError, match="no 'gt_semantic_map'"):
        meter.update(Net(), {})
    with pytest.raises(_abi.WsmgError, match="float32"):
        meter.update(Net(), {"gt_semantic_map": gt.long()})
    with pytest.raises(_abi.WsmgError, match="on the GPU"):
        meter.update(Net(), {"gt_semantic_map": gt.cpu()})
    with pytest.raises(_abi.WsmgError, match="3 ground-truth maps for 2 rows"):
        meter.update(Net(), {"gt_semantic_map": torch.zeros(3, 100, 100, device="cuda")})
    with pytest.raises(_abi.WsmgError, match="weights"):
        meter.update(Net(), {"gt_semantic_map": gt}, torch.ones(3, device="cuda"))
    assert not meter.confusion.any() and not meter.ignored.any()


# ----------------------------------------------------------------------------- 6. capture
def test_update_replays_from_a_captured_graph():
    from wsmgmap.metrics import SemanticMapMeter
    B, H, W, classes = 4, 48, 48, 27
    gt = make_gt(B, 100, 100, classes, seed=70)
    batches = [make_logits(B, H, W, classes, torch.bfloat16, seed=71 + i) for i in range(4)]
    weights = torch.tensor([[1.0], [0.0], [0.5], [2.0]])
    wants = [oracle(x, gt, classes, (weights > 0).view(-1)) for x in batches]

    class Net:
        sem_logits_nhwc = batches[0].cuda()
    obs, w = {"gt_semantic_map": gt.cuda()}, weights.cuda()
    meter = SemanticMapMeter()
    meter.update(Net(), obs, w)                                  # the eager warm-up: the mask buffer exists from here on
    mask_ptr = meter._mask.data_ptr()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):                                # one stream, no parallel branches
        meter.update(Net(), obs, w)
    assert meter._mask.data_ptr() == mask_ptr
    meter.reset()
    total = np.zeros((classes, classes), np.int64)
    for x, want in zip(batches[1:], wants[1:]):
        Net.sem_logits_nhwc.copy_(x.cuda())                      # fresh logits into the same storage
        graph.replay()
        total += want[0]
    torch.cuda.synchronize()
    assert np.array_equal(meter.confusion.cpu().numpy(), total) and total.sum() == 3 * 3 * H * W
    assert not meter.ignored.any()


# ----------------------------------------------------------------------------- 7. the policy
class _Box:
    shape = (2,)


Tn, N = 4, 2


@functools.lru_cache(maxsize=None)
def _base(mode):
    """The deterministic-fill T = 4 x N = 2 policy of the update tests in `mode`, NEVER run (every run works on a deep copy)."""
    from wsmgmap.config import default_model_config
    from wsmgmap.models.policy import BasePolicy
    pol = BasePolicy(None, _Box(), default_model_config(num_proc=2, compute_dtype=mode))
    pol.load_state_dict(state_dict_values(), strict=True)
    pol = pol.cuda()
    pol.train()
    pol.net.depth_encoder.eval()
    pol.net.rgb_encoder.eval()
    return pol


def _update(mode, between=None):
    """One teacher-forcing update on a fresh copy; `between(policy, obs, weights)` runs after the forward pass, before the loss."""
    from wsmgmap.common.aux_losses import AuxLosses
    pol = copy.deepcopy(_base(mode))
    obs_np, prev, masks, weights = cases.update_inputs(Tn, N)
    og = {k: T(v).cuda() for k, v in obs_np.items()}
    w = T(weights).cuda()
    AuxLosses.activate()
    AuxLosses.clear()
    try:
        pred, aux = pol(og, torch.zeros(2, N, 512, device="cuda"), T(prev).cuda(), T(masks).cuda(), w)
        extra = between(pol, og, w) if between else None
        loss = (pred ** 2).mean() + aux
        loss.backward()
        torch.cuda.synchronize()
    finally:
        AuxLosses.deactivate()
        AuxLosses.clear()
    grads = {k: p.grad.clone() for k, p in pol.named_parameters() if p.grad is not None}
    return pol, pred.detach().clone(), aux.detach().clone(), grads, extra


@pytest.mark.parametrize("mode", ["bf16", "f32"])
def test_policy_update_is_scored_without_being_touched(mode):
    from wsmgmap.metrics import SemanticMapMeter
    from wsmgmap.models.mg_map_policy import SEM_CLASSES

    def score(pol, og, w):
        meter = SemanticMapMeter()
        meter.update(pol, og, w)
        logits = pol.net.sem_logits_nhwc
        want = oracle(logits, og["gt_semantic_map"], SEM_CLASSES, (w > 0).view(-1))
        assert np.array_equal(meter.confusion.cpu().numpy(), want[0]) and meter.ignored.cpu().tolist() == want[1].tolist()
        assert want[0].sum() > 0
        # the prediction map: every row, mask or not
        sp = pol.semantic_prediction()
        assert sp.dtype == torch.uint8 and tuple(sp.shape) == tuple(logits.shape[:3])
        assert np.array_equal(sp.cpu().numpy(), oracle(logits, None, SEM_CLASSES)[2])
        # a weights row of zeros removes exactly that row's pixels
        w0 = w.clone().view(-1)
        keep = int(torch.nonzero(w0 > 0)[0])
        w0[keep] = 0.0
        less = SemanticMapMeter()
        less.update(pol.net, og, w0.view_as(w))
        one_row = oracle(logits[keep:keep + 1], og["gt_semantic_map"][keep:keep + 1], SEM_CLASSES)
        assert one_row[0].sum() + one_row[1].sum() == logits.shape[1] * logits.shape[2]
        assert np.array_equal(less.confusion.cpu().numpy(), want[0] - one_row[0])
        assert less.ignored.cpu().tolist() == (want[1] - one_row[1]).tolist()
        return meter.compute()

    pol, pred, aux, grads, out = _update(mode, score)
    if mode == "bf16":
        assert pol.net.sem_ce_rows is not None and pol.net.sem_logits_nhwc.dtype == torch.bfloat16        # the fused tail ran
    else:
        assert pol.net.sem_ce_rows is None and pol.net.sem_logits_nhwc.dtype == torch.float32            # the unfused route
    assert tuple(pol.net.sem_logits_nhwc.shape) == (Tn * N, 48, 48, 32)
    assert 0.0 <= out["pixel_accuracy"] <= 1.0 and 0.0 <= out["miou"] <= 1.0 and out["pixels"] > 0
    _, pred0, aux0, grads0, _ = _update(mode)                     # the same update without the meter
    assert torch.equal(pred.view(torch.int32), pred0.view(torch.int32)) and torch.equal(aux.view(torch.int32), aux0.view(torch.int32))
    assert grads.keys() == grads0.keys() and len(grads) > 50
    for k in grads:
        assert torch.equal(grads[k].view(torch.int32), grads0[k].view(torch.int32)), k
