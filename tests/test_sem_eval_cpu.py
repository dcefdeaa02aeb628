"""CPU: the host side of the semantic-map scoring — the three entry points of csrc/wsmg_sem_eval.hip in the header and the binding,
every refused argument (the checks precede the first launch, so no GPU is needed), ops.sem_confusion's refusal of CPU tensors, and
SemanticMapMeter.scores_from, the documented host form of the scores.  The kernels are tested in tests/test_gpu_sem_eval.py."""
import ctypes
import math

import pytest
import torch

EINVAL = -1
NAMES = ("wsmg_sem_confusion_f32", "wsmg_sem_confusion_bf16", "wsmg_sem_scores")

_buf = (ctypes.c_uint64 * 64)()
P = ctypes.cast(_buf, ctypes.c_void_p)      # a non-null host pointer: never dereferenced, every check precedes the launch


def _confusion(L, name, **over):
    """(logits, classes, gt, Hg, Wg, B, H, W, row_mask, confusion, ignored, pred, stream), valid unless overridden."""
    a = dict(logits=P, classes=27, gt=P, Hg=100, Wg=100, B=2, H=48, W=48, row_mask=None, confusion=P, ignored=P, pred=None)
    a.update(over)
    return getattr(L, name)(a["logits"], a["classes"], a["gt"], a["Hg"], a["Wg"], a["B"], a["H"], a["W"], a["row_mask"],
                            a["confusion"], a["ignored"], a["pred"], None)


def test_entry_points_are_declared_bound_and_exported():
    """(Their declarations against the binding: tests/test_abi_cpu.py.)"""
    from wsmgmap import _abi
    L = _abi.lib()
    for name in NAMES:
        assert name in _abi.exported_names() and hasattr(L, name)
        assert list(getattr(L, name).argtypes) == list(_abi._SIG[name]) and getattr(L, name).restype is ctypes.c_int
    assert len(_abi._SIG[NAMES[0]]) == 13 and _abi._SIG[NAMES[1]] == _abi._SIG[NAMES[0]] and len(_abi._SIG[NAMES[2]]) == 4
    assert L.wsmg_abi_version() == 1


@pytest.mark.parametrize("name", NAMES[:2])
@pytest.mark.parametrize("over", [
    dict(logits=None), dict(gt=None), dict(confusion=None), dict(ignored=None),
    dict(gt=None, confusion=None), dict(confusion=None, ignored=None),
    dict(gt=None, confusion=None, ignored=None),                    # the prediction-only use needs a place for the predictions
    dict(classes=0), dict(classes=33), dict(classes=-1),
    dict(B=0), dict(B=-1), dict(H=0), dict(W=0), dict(H=-3), dict(Hg=0), dict(Wg=0), dict(Wg=-1),
    dict(B=1 << 15, H=1 << 8, W=1 << 8),                                # B*H*W = 2^31
    dict(B=46341, H=46341, W=1),                                        # just above 2^31 (and above int32)
], ids=lambda o: ",".join(f"{k}={v}" for k, v in o.items()))
def test_confusion_refuses_bad_arguments_before_any_launch(name, over):
    from wsmgmap import _abi
    assert _confusion(_abi.lib(), name, **over) == EINVAL


def test_scores_refuses_bad_arguments_before_any_launch():
    from wsmgmap import _abi
    L = _abi.lib()
    assert L.wsmg_sem_scores(None, 27, P, None) == EINVAL
    assert L.wsmg_sem_scores(P, 27, None, None) == EINVAL
    assert L.wsmg_sem_scores(P, 0, P, None) == EINVAL
    assert L.wsmg_sem_scores(P, 33, P, None) == EINVAL


def test_ops_refuse_cpu_tensors():
    from wsmgmap import _abi, ops
    logits, gt = torch.zeros(1, 4, 4, 32), torch.zeros(1, 5, 5)
    with pytest.raises(_abi.WsmgError, match="no CPU fallback"):
        ops.sem_confusion(logits, gt, 27)
    with pytest.raises(_abi.WsmgError, match="no CPU fallback"):
        ops.sem_confusion(logits, None, 27, want_pred=True)
    with pytest.raises(_abi.WsmgError, match="no CPU fallback"):
        ops.sem_scores(torch.zeros(27, 27, dtype=torch.int64))
    from wsmgmap.metrics import SemanticMapMeter
    with pytest.raises(_abi.WsmgError, match="no CPU fallback"):
        SemanticMapMeter(device="cpu")


def test_policy_has_the_prediction_method_and_refuses_before_a_forward_pass():
    from wsmgmap import _abi
    from wsmgmap.config import default_model_config
    from wsmgmap.models.policy import BasePolicy

    class Box:
        shape = (2,)
    pol = BasePolicy(None, Box(), default_model_config(num_proc=2))
    with pytest.raises(_abi.WsmgError, match="no forward pass"):
        pol.semantic_prediction()


# ----------------------------------------------------------------------------- scores_from: the host form
def _scores(m):
    from wsmgmap.metrics import SemanticMapMeter
    return SemanticMapMeter.scores_from(torch.tensor(m, dtype=torch.int64))


def test_scores_of_a_diagonal_matrix():
    s = _scores([[5, 0, 0], [0, 7, 0], [0, 0, 1]])
    assert s["pixels"] == 13 and s["pixel_accuracy"] == 1.0 and s["miou"] == 1.0
    assert s["iou"] == [1.0, 1.0, 1.0] and s["gt_pixels"] == [5, 7, 1] and s["pred_pixels"] == [5, 7, 1]
    assert s["ignored_labels"] == 0 and s["nan_pixels"] == 0


def test_scores_by_hand():
    # labels in rows: class 0: TP 3, FN 1 (predicted 1); class 1: TP 2, FN 2 (predicted 0); class 2 never a label, predicted never
    s = _scores([[3, 1, 0], [2, 2, 0], [0, 0, 0]])
    assert s["pixels"] == 8 and s["pixel_accuracy"] == 5 / 8
    assert s["iou"][0] == 3 / 6 and s["iou"][1] == 2 / 5 and math.isnan(s["iou"][2])
    assert s["miou"] == (3 / 6 + 2 / 5) / 2                         # the absent class is left out of the mean
    assert s["gt_pixels"] == [4, 4, 0] and s["pred_pixels"] == [5, 3, 0]


def test_scores_of_a_class_that_is_only_predicted():
    # class 2 is never a label but is predicted once: union 1, IoU 0 — present, and it pulls the mean down
    s = _scores([[1, 0, 1], [0, 1, 0], [0, 0, 0]])
    assert s["iou"] == [0.5, 1.0, 0.0] and s["miou"] == 0.5


def test_scores_of_an_empty_matrix():
    s = _scores([[0, 0], [0, 0]])
    assert s["pixels"] == 0 and math.isnan(s["pixel_accuracy"]) and math.isnan(s["miou"])
    assert all(math.isnan(v) for v in s["iou"]) and s["gt_pixels"] == [0, 0] and s["pred_pixels"] == [0, 0]


def test_scores_with_counts_above_2_to_32():
    big = (1 << 40) + 3
    s = _scores([[big, 1], [2, 1 << 33]])
    assert s["pixels"] == big + 3 + (1 << 33)
    assert s["gt_pixels"] == [big + 1, (1 << 33) + 2] and s["pred_pixels"] == [big + 2, (1 << 33) + 1]
    assert s["iou"][0] == big / (big + 3) and s["iou"][1] == (1 << 33) / ((1 << 33) + 3)
    assert s["pixel_accuracy"] == (big + (1 << 33)) / (big + 3 + (1 << 33))


def test_scores_from_carries_the_ignored_pair_and_refuses_other_matrices():
    from wsmgmap.metrics import SemanticMapMeter
    s = SemanticMapMeter.scores_from(torch.eye(2, dtype=torch.int64), torch.tensor([4, 9]))
    assert s["ignored_labels"] == 4 and s["nan_pixels"] == 9
    with pytest.raises(ValueError):
        SemanticMapMeter.scores_from(torch.zeros(2, 3, dtype=torch.int64))
    with pytest.raises(ValueError):
        SemanticMapMeter.scores_from(torch.zeros(2, 2))
