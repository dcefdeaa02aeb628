"""wsmg_map_fuse_retrieve / wsmg_bev_project without a GPU: the two symbols in the built library and the binding (derived from the header); the
argument checks of ops.map_fuse_retrieve and ops.bev_project, which refuse before any launch; and the property the one-launch
fuse + retrieve leans on, shown on the oracle alone: a fuse step applied twice with the same inputs leaves the map of the first
application, bit for bit (masks in {0, 1}, a map and features of both signs, -0.0 entries)."""
import subprocess

import numpy as np
import pytest
import torch

from oracle import bev_ref
from util import T

NAMES = ("wsmg_map_fuse_retrieve", "wsmg_bev_project")


def test_both_entry_points_are_declared_exported_and_bound():
    """(Their declarations against the binding, and the header's promise of bit-identical results: tests/test_abi_cpu.py.)"""
    from wsmgmap import _abi
    nm = subprocess.run(["nm", "-D", "--defined-only", _abi.LIB_PATH], check=True, capture_output=True, text=True).stdout
    exported = {line.split()[-1] for line in nm.splitlines() if line.strip()}
    for name in NAMES:
        assert name in exported, f"{name} is not exported by {_abi.LIB_PATH}"
        assert name in _abi.exported_names()
    assert len(_abi._SIG[NAMES[0]]) == 12 and len(_abi._SIG[NAMES[1]]) == 17


def _fr_args(B=2, C=8, E=24, G=32, P=2):
    return dict(ego_rot_planes=torch.zeros(B, C, E, E), global_map=torch.zeros(P, G, G, C), gps=torch.zeros(B, 2),
                compass=torch.zeros(B), masks=torch.ones(B), E=E)


@pytest.mark.parametrize("change,match", [
    (dict(gps=torch.zeros(3, 2)), "must match"),
    (dict(masks=torch.ones(1)), "must match"),
    (dict(compass=torch.zeros(5)), "must match"),
    (dict(global_map=torch.zeros(1, 32, 32, 8)), "num_proc"),
    (dict(ego_rot_planes=torch.zeros(2, 6, 24, 24), global_map=torch.zeros(2, 32, 32, 6)), "bev_planes_ok"),
    (dict(ego_rot_planes=torch.zeros(2, 68, 24, 24), global_map=torch.zeros(2, 32, 32, 68)), "bev_planes_ok"),
    (dict(ego_rot_planes=torch.zeros(2, 8, 24, 20)), "rotated planes"),
], ids=["gps_batch", "masks_batch", "compass_batch", "more_rows_than_maps", "c_not_multiple_of_4", "c_above_64", "not_square"])
def test_map_fuse_retrieve_refuses_before_any_launch(monkeypatch, change, match):
    from wsmgmap import _abi, ops
    monkeypatch.setattr(_abi, "call", lambda *a: pytest.fail("a refused call reached the library"))
    with pytest.raises(_abi.WsmgError, match=match):
        ops.map_fuse_retrieve(**{**_fr_args(), **change})


def test_map_fuse_retrieve_refuses_a_plane_that_does_not_fit_lds(monkeypatch):
    from wsmgmap import _abi, ops
    monkeypatch.setattr(_abi, "call", lambda *a: pytest.fail("a refused call reached the library"))
    E = 203                                             # 203 * 203 * 4 > 160 KiB
    assert not ops.bev_planes_ok(8, E) and ops.bev_planes_ok(8, 202)
    planes = torch.zeros(1, 1, 1, 1).expand(1, 8, E, E)
    gm = torch.zeros(1, 1, 1, 1).expand(1, 256, 256, 8)
    with pytest.raises(_abi.WsmgError, match="bev_planes_ok"):
        ops.map_fuse_retrieve(planes, gm, torch.zeros(1, 2), torch.zeros(1), torch.ones(1), E)


@pytest.mark.parametrize("change,match", [
    (dict(feat=torch.zeros(3, 8, 16, 16)), "same batch"),
    (dict(heading=torch.zeros(4)), "same batch"),
    (dict(C=6), "bev_planes_ok"),
    (dict(E=203), "bev_planes_ok"),
    (dict(C=12), "C <= Cf"),
    (dict(feat=torch.zeros(2, 8, 64, 64)), "no larger than the depth"),
], ids=["feat_batch", "heading_batch", "c_not_multiple_of_4", "plane_beyond_lds", "more_map_than_feature_channels", "feat_larger_than_depth"])
def test_bev_project_refuses_before_any_launch(monkeypatch, change, match):
    from wsmgmap import _abi, ops
    monkeypatch.setattr(_abi, "call", lambda *a: pytest.fail("a refused call reached the library"))
    args = dict(depth=torch.zeros(2, 32, 32), feat=torch.zeros(2, 8, 16, 16), heading=torch.zeros(2), sign=-1.0, C=8, E=24)
    with pytest.raises(_abi.WsmgError, match=match):
        ops.bev_project(**{**args, **change})


def test_the_default_route_is_the_measured_one(monkeypatch):
    """With the switch at -1 (as shipped) a one-launch form is taken only where profiles/bev_fuse_retrieve.txt has it measured and
    not slower: map_fuse_retrieve at B = 1 of E = 100, C = 64, G = 240; nothing at B = 8, nothing at a geometry that was not
    measured, bev_project nowhere.  0 and 1 force neither / both."""
    from wsmgmap import debug, ops
    assert dict((n, d) for n, _, d, _, _ in debug._TABLE)["bev_one_launch"] == -1
    monkeypatch.setattr(debug.sw, "bev_one_launch", -1)
    assert ops.bev_one_launch_routes(1, 64, 100, 240) == (False, True)
    assert ops.bev_one_launch_routes(8, 64, 100, 240) == (False, False)
    assert ops.bev_one_launch_routes(32, 40, 200, 480) == (False, False)
    assert ops.bev_one_launch_routes(1, 40, 200, 480) == (False, False)        # not measured: the two launches stay
    assert ops.bev_one_launch_routes(2, 64, 100, 240) == (False, False)
    monkeypatch.setattr(debug.sw, "bev_one_launch", 1)
    assert ops.bev_one_launch_routes(1, 40, 200, 480) == (True, True)
    assert ops.bev_one_launch_routes(8, 64, 100, 240) == (False, True)
    assert ops.bev_one_launch_routes(1, 68, 100, 240) == (False, False)        # bev_planes_ok refuses: no one-launch form
    monkeypatch.setattr(debug.sw, "bev_one_launch", 0)
    assert ops.bev_one_launch_routes(1, 64, 100, 240) == (False, False)


@pytest.mark.parametrize("E,C,G", [(24, 8, 24), (33, 8, 65)], ids=["e24_c8_g24", "e33_c8_g65"])
def test_a_fuse_step_applied_twice_is_the_step_applied_once_on_the_oracle(E, C, G):
    """F(F(g)) == F(g) for F(g) = max(g * m, paste), on bev_ref.MapperRef in float32 and the inputs of the GPU file's signed-zero
    test: sample 0 reset (m = 0), the others kept; the map holds both signs, -0.0 and +0.0.  The one-launch kernel's readers fuse
    values that their owner may already have fused — this is the invariant that makes that exact, independent of the kernel."""
    from test_gpu_map_fuse_retrieve import signed_inputs
    B = 3
    n = B * G * G * C
    i = np.arange(n)
    start = ((i % 977) / 977.0 - 0.5).astype(np.float32)
    start[i % 11 == 0] = 0.0
    start[i % 7 == 0] = -0.0
    start = T(start.reshape(B, G, G, C))
    for step in (2, 3):
        c = signed_inputs(E, C, G, step)
        assert float(c["feat"].min()) < 0 < float(c["feat"].max())
        args = (T(c["feat"]), T(c["depth"]), T(c["gps"]), c["compass"], T(c["masks"]))
        ref = bev_ref.MapperRef(B, G, E, C, 0.12)
        ref.full_global_map = start.clone()
        ref.step(*args)
        once = ref.full_global_map.clone()
        ref.step(*args)
        twice = ref.full_global_map
        assert torch.equal(once.view(torch.int32), twice.view(torch.int32)), int((once.view(torch.int32) != twice.view(torch.int32)).sum())
        assert not torch.equal(once.view(torch.int32), start.view(torch.int32))
        if step == 2:
            assert int((once[0].view(torch.int32) == -2 ** 31).sum()) > 0      # g * 0 kept the sign of the negative entries
