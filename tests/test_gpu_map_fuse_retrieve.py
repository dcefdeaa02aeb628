"""The one-launch forms of the map operator against the launches they replace, bit for bit: wsmg_map_fuse_retrieve (= wsmg_map_fuse_planes
then wsmg_map_retrieve_tiled) and wsmg_bev_project (= wsmg_bev_index then wsmg_bev_scatter_rotate), on the edge sequence of
test_gpu_map_edges.py (windows leaving the map, odd E, odd G, G == E, the six headings, an episode reset), with P > B, with negative
features and signed zeros in the map, on the retrieval tiles' rare route (a gps that is not finite), inside a captured graph and on Mapping.project_feat_to_map's route; and map_fuse_retrieve alone
against the float64 oracle under the edges file's bar.

Why bit identity is the bar: both forms run the expressions of the launches they replace (csrc/wsmg_bev.hip lifts the device
functions).  In wsmg_map_fuse_retrieve a retrieval workgroup may read a map element before or after its owner's store and fuses
what it read itself; that is exact only because the fuse is idempotent per element for masks in {0, 1} (the comment at
map_fuse_retrieve_kernel) — the signed-zero test below is the one that would show a hole in that argument.
"""
import types

import numpy as np
import pytest
import torch

from oracle import bev_ref
from oracle import detfill as df
from util import T
from test_gpu_map_edges import GEOMS, GEOM_IDS, HF, RES, Figures, dev, dmax, floor_depth, gate_case, headings, seq_inputs

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops():
    from wsmgmap import ops as o
    return o


def bits(t):
    return t.contiguous().view(torch.int32)


def same_bits(a, b, what):
    assert a.shape == b.shape, (what, a.shape, b.shape)
    n = int((bits(a) != bits(b)).sum())
    assert n == 0, f"{what}: {n} of {a.numel()} elements differ in their bits"


def fill(shape, signed=False):
    """A deterministic dense map: (i mod 977) / 977 + 0.01 (positive), or centred on 0 with every 7th element -0.0 and every 11th
    +0.0 (`signed`)."""
    n = int(np.prod(shape))
    i = torch.arange(n, device="cuda")
    v = i.remainder(977).float() / 977.0
    if not signed:
        return (v + 0.01).reshape(shape)
    v = v - 0.5
    v[i.remainder(11) == 0] = 0.0
    v[i.remainder(7) == 0] = -0.0
    return v.reshape(shape)


def step_args(c):
    return (dev(c["feat"]), dev(c["depth"][..., 0]), dev(c["gps"]), dev(c["compass"]).reshape(-1).contiguous(),
            dev(c["masks"]).reshape(-1).contiguous())


def two_launches(ops, rotp, gm, gps, compass, masks, E):
    ops.map_fuse(rotp, gm, gps, masks, RES, planes=True)
    return ops.map_retrieve(gm, gps, compass, E, RES)


def signed_inputs(E, C, G, step):
    """Steps 2 (sample 0 reset, reach 0.97) and 3 (reach 1.2) of the edge sequence with features of both signs (not clamped)."""
    B = 3
    c = seq_inputs(f"fr.signed.{E}.{C}.{G}", step, B, E, C, G)
    c["feat"] = df.uniform(f"fr.signed.feat.{E}.{G}.{step}", (B, C, HF, HF), 4.0)
    return c


# ----------------------------------------------------------------------------- 1. the edge sequence, bit for bit
@pytest.mark.parametrize("E,C,G", GEOMS, ids=GEOM_IDS)
def test_fuse_retrieve_equals_the_two_launches_over_the_edge_sequence(ops, E, C, G):
    B = 3
    tag = f"edges.seq.{E}.{C}.{G}"
    gm2, gm1 = fill((B, G, G, C)), fill((B, G, G, C))
    for step in range(4):
        feat, depth, gps, compass, masks = step_args(seq_inputs(tag, step, B, E, C, G))
        rotp = ops.bev_scatter_rotate(feat, ops.bev_index(depth, HF, HF, E), compass, -1.0, C, E)
        ego2 = two_launches(ops, rotp, gm2, gps, compass, masks, E)
        ego1 = ops.map_fuse_retrieve(rotp, gm1, gps, compass, masks, E, RES)
        same_bits(gm1, gm2, f"step {step} global map")
        same_bits(ego1, ego2, f"step {step} ego map")
        if step == 2:       # the reset erased the fill of sample 0 outside the window too, and nothing of the others
            assert float(gm1[0, 0, 0].abs().max()) == 0.0 or float(gm1[0, -1, -1].abs().max()) == 0.0
            assert float(gm1[1].min()) > 0.0
    for name, t in (("global", gm1), ("ego", ego1)):
        nz = float((t != 0).float().mean())
        assert float(t.max()) > 0 and nz > 0.01, (name, nz)


# ----------------------------------------------------------------------------- 2. B = 1 in a map of three slots
@pytest.mark.parametrize("E,C,G", [(33, 8, 64), (100, 64, 240)], ids=["e33_c8_g64", "e100_c64_g240"])
def test_fuse_retrieve_b1_touches_only_its_slot(ops, E, C, G):
    start = fill((3, G, G, C))
    gm2, gm1 = start.clone(), start.clone()
    for step in (1, 2):     # the border, then a reset
        feat, depth, gps, compass, masks = step_args(seq_inputs(f"fr.b1.{E}.{G}", step, 1, E, C, G))
        rotp = ops.bev_scatter_rotate(feat, ops.bev_index(depth, HF, HF, E), compass, -1.0, C, E)
        ego2 = two_launches(ops, rotp, gm2, gps, compass, masks, E)
        ego1 = ops.map_fuse_retrieve(rotp, gm1, gps, compass, masks, E, RES)
        assert ego1.shape == (1, E, E, C)
        same_bits(gm1[:1], gm2[:1], f"step {step} slot 0")
        same_bits(ego1, ego2, f"step {step} ego map")
        same_bits(gm1[1:], start[1:], f"step {step} slots 1-2")
    assert float(ego1.max()) > 0


# ----------------------------------------------------------------------------- 3. negative features, signed zeros
@pytest.mark.parametrize("E,C,G", [(24, 8, 24), (33, 8, 65)], ids=["e24_c8_g24", "e33_c8_g65"])
def test_fuse_retrieve_negative_features_and_signed_zeros(ops, E, C, G):
    """The case that decides the idempotency argument: a map of both signs with -0.0 and +0.0 entries, features of both signs, one
    sample reset (g * 0 is -0.0 for every negative g) and two not."""
    start = fill((3, G, G, C), signed=True)
    gm2, gm1 = start.clone(), start.clone()
    assert int((bits(start) == -2 ** 31).sum()) > 0       # -0.0 is there
    for step in (2, 3):
        feat, depth, gps, compass, masks = step_args(signed_inputs(E, C, G, step))
        rotp = ops.bev_scatter_rotate(feat, ops.bev_index(depth, HF, HF, E), compass, -1.0, C, E)
        assert float(rotp.min()) < 0 < float(rotp.max())
        ego2 = two_launches(ops, rotp, gm2, gps, compass, masks, E)
        ego1 = ops.map_fuse_retrieve(rotp, gm1, gps, compass, masks, E, RES)
        same_bits(gm1, gm2, f"step {step} global map")
        same_bits(ego1, ego2, f"step {step} ego map")
    assert int((bits(gm1[0]) == -2 ** 31).sum()) > 0        # the reset sample holds -0.0 where the map was negative
    assert float(gm1.min()) < 0 < float(gm1.max())


# ----------------------------------------------------------------------------- 3b. the rare route of the retrieval tiles
@pytest.mark.parametrize("E,C,G", [(24, 8, 24), (33, 8, 64)], ids=["e24_c8_g24", "e33_c8_g64"])
def test_fuse_retrieve_rare_route_with_a_non_finite_gps(ops, E, C, G):
    """A retrieval tile whose box does not fit 14 x 14 takes the register route (retrieve_item_seq, here with AsFused / fuse_quad).
    A finite pose never does; a gps coordinate that is not finite does, as in test_map_retrieve_lds_tiles_equal_crop_then_rotate:
    sample 1 has a NaN coordinate (the taps land on map rows 0 and 1 with NaN weights: fuse_quad runs, inside the fuse window at
    G == E; the ego map is NaN), sample 2 an infinite one (every tap is outside the map: zeros), samples 0 (in the
    map's corner, reset at step 2) and 3 (inside the map) finite poses on the usual route beside them.  The fused values of the rare route cannot be seen through the ego map (NaN or no
    tap at all), so what this holds is: the same NaN pattern, the same bits wherever the two launches give a number, and the
    same global map, which no retrieval workgroup may write."""
    start = fill((4, G, G, C), signed=True)
    gm2, gm1 = start.clone(), start.clone()
    for step in (1, 2):
        c = seq_inputs(f"fr.rare.{E}.{G}", step, 4, E, C, G)
        feat, depth, gps, compass, masks = step_args(c)
        gps[1, 0] = float("nan")
        gps[2, 0] = float("inf")
        rotp = ops.bev_scatter_rotate(feat, ops.bev_index(depth, HF, HF, E), compass, -1.0, C, E)
        ego2 = two_launches(ops, rotp, gm2, gps, compass, masks, E)
        ego1 = ops.map_fuse_retrieve(rotp, gm1, gps, compass, masks, E, RES)
        same_bits(gm1, gm2, f"step {step} global map")
        assert torch.equal(ego1.isnan(), ego2.isnan()), f"step {step}: the NaN patterns differ"
        num = ~ego2.isnan()
        assert torch.equal(bits(ego1)[num], bits(ego2)[num]), f"step {step}: ego map"
        assert bool(ego2[1].isnan().any()) and not bool(ego2[[0, 2, 3]].isnan().any())       # the NaN sample's taps were taken
        assert float(ego2[2].abs().max()) == 0.0 and float(ego2[3].abs().max()) > 0
    assert not bool(gm1.isnan().any())


# ----------------------------------------------------------------------------- 4. against the float64 oracle
@pytest.mark.parametrize("E,C,G", GEOMS, ids=GEOM_IDS)
def test_fuse_retrieve_sequence_vs_float64_oracle(ops, E, C, G):
    """map_fuse_retrieve alone over the edge sequence (from an empty map, as the oracle starts) under the edges file's bar:
    |kernel - oracle64| <= K_TOL * d32, d32 the reference's own float32-to-float64 distance.  The figures are those of the
    two-launch route in test_gpu_map_edges.py's table (the results are bit-identical)."""
    B = 3
    tag = f"edges.seq.{E}.{C}.{G}"
    ref64 = bev_ref.MapperRef(B, G, E, C, RES, dtype=torch.float64)
    ref32 = bev_ref.MapperRef(B, G, E, C, RES)
    gm = torch.zeros(B, G, G, C, device="cuda")
    fig = Figures()
    for step in range(4):
        c = seq_inputs(tag, step, B, E, C, G)
        args = (T(c["feat"]), T(c["depth"]), T(c["gps"]), c["compass"], T(c["masks"]))
        ego64, ego32 = ref64.step(*args), ref32.step(*args)
        d_map, d_ego = dmax(ref32.full_global_map, ref64.full_global_map), dmax(ego32, ego64)
        vmax = float(c["feat"].max())
        fig.condition(f"s{step}.global", d_map, G, vmax)
        fig.condition(f"s{step}.ego", d_ego, G, vmax)
        feat, depth, gps, compass, masks = step_args(c)
        rotp = ops.bev_scatter_rotate(feat, ops.bev_index(depth, HF, HF, E), compass, -1.0, C, E)
        ego = ops.map_fuse_retrieve(rotp, gm, gps, compass, masks, E, RES)
        fig.check(f"one_launch.s{step}.global", gm, ref64.full_global_map, d_map)
        fig.check(f"one_launch.s{step}.ego", ego.permute(0, 3, 1, 2), ego64, d_ego)
    assert float(gm.max()) > 0 and float((ego != 0).float().mean()) > 0.01
    fig.done()


# ----------------------------------------------------------------------------- 5. bev_project
def project_cases():
    out = []
    for E in (33, 101):
        for Hf in (64, 100):
            out.append(pytest.param(("gate", E, Hf), id=f"gate_e{E}_f{Hf}"))
    for Cf in (16, 20, 32):        # adaptive-max-pool windows of 2, 3 and 4 feature channels: the other instantiations of the kernel
        out.append(pytest.param(("wide", 33, Cf), id=f"window_cf{Cf}_c8"))
    out.append(pytest.param(("seq", 100, 64, 240), id="seq_e100_c64_g240"))
    out.append(pytest.param(("seq", 200, 40, 480), id="seq_e200_c40_g480"))
    return out


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("case", project_cases())
def test_bev_project_equals_index_then_scatter_rotate(ops, case, B):
    if case[0] == "gate":
        _, E, Hf = case
        C = 8
        c = gate_case(E, Hf, 3)        # (the case is built for three samples: zero rows, ties, an all-invalid sample)
    elif case[0] == "wide":
        _, E, Cf = case
        C, Hf = 8, HF
        c = dict(depth=floor_depth(f"fr.wide.depth.{Cf}", 3, E), feat=df.uniform(f"fr.wide.feat.{Cf}", (3, Cf, HF, HF), 4.0))
    else:
        _, E, C, G = case
        Hf = HF
        c = seq_inputs(f"edges.seq.{E}.{C}.{G}", 0, 3, E, C, G)
    c = {k: c[k][:B] for k in ("depth", "feat")}
    depth, feat = dev(c["depth"][..., 0]).contiguous(), dev(c["feat"]).contiguous()
    heading = dev(headings(1, B)).reshape(-1).contiguous()
    lin = ops.bev_index(depth, Hf, Hf, E)
    want = ops.bev_scatter_rotate(feat, lin, heading, -1.0, C, E)
    got, got_lin = ops.bev_project(depth, feat, heading, -1.0, C, E)
    assert got_lin.dtype == torch.int32 and torch.equal(got_lin, lin)
    same_bits(got, want, "planes")
    got2, none = ops.bev_project(depth, feat, heading, -1.0, C, E, want_index=False)     # lin_idx = NULL
    assert none is None
    same_bits(got2, want, "planes without the index")
    if case[0] != "gate" or B > 1:
        assert float(want.abs().max()) > 0 and int((lin >= 0).sum()) > 0


# ----------------------------------------------------------------------------- 6. graph capture
def test_one_step_replays_in_a_captured_graph(ops):
    """bev_project -> map_fuse_retrieve captured once and replayed twice with the inputs changed in place between the replays
    (the map carries over): after each replay the ego map and the global map equal the eager index / scatter_rotate / fuse /
    retrieve route's."""
    E, C, G, B = 33, 8, 64, 1
    steps = [step_args(seq_inputs("fr.graph", s, B, E, C, G)) for s in (0, 1, 2)]
    static = [t.clone() for t in steps[0]]
    gm1, gm2 = fill((B, G, G, C)), fill((B, G, G, C))
    start = gm1.clone()

    def one(feat, depth, gps, compass, masks):
        rotp, _ = ops.bev_project(depth, feat, compass, -1.0, C, E, want_index=False)
        return ops.map_fuse_retrieve(rotp, gm1, gps, compass, masks, E, RES)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        one(*static)                                       # warm-up outside the capture (first-launch attributes)
    torch.cuda.current_stream().wait_stream(side)
    gm1.copy_(start)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        ego1 = one(*static)
    gm1.copy_(start)                                       # (capturing runs nothing)
    for n, args in enumerate(steps[1:]):
        for s, a in zip(static, args):
            s.copy_(a)
        graph.replay()
        feat, depth, gps, compass, masks = args
        rotp = ops.bev_scatter_rotate(feat, ops.bev_index(depth, HF, HF, E), compass, -1.0, C, E)
        ego2 = two_launches(ops, rotp, gm2, gps, compass, masks, E)
        torch.cuda.synchronize()
        same_bits(ego1, ego2, f"replay {n} ego map")
        same_bits(gm1, gm2, f"replay {n} global map")
    assert float(ego1.max()) > 0


# ----------------------------------------------------------------------------- 7. the policy's route
@pytest.mark.parametrize("B,names", [
    (1, ["wsmg_bev_project", "wsmg_map_fuse_retrieve"]),
    (8, ["wsmg_bev_index_compact", "wsmg_bev_scatter_rotate_compact", "wsmg_map_fuse_retrieve"]),
], ids=["b1_two_launches", "b8_three_launches"])
def test_mapping_route_takes_the_one_launch_forms_and_keeps_the_bits(monkeypatch, B, names):
    from wsmgmap import _abi, debug
    from wsmgmap.common.rgb_mapping import RGBMapping
    E, C, G = 100, 64, 240
    cfg = types.SimpleNamespace(num_proc=B, resolution=RES, egocentric_map_size=E, global_map_size=G, map_depth=C, gpu_id=0)
    calls = []
    real = _abi.call

    def counting(name, *a):
        calls.append(name)
        return real(name, *a)
    monkeypatch.setattr(_abi, "call", counting)
    maps = {route: RGBMapping(cfg).cuda() for route in (0, 1)}
    for step in (1, 2):
        c = seq_inputs(f"fr.route.{B}", step, B, E, C, G)
        egos = {}
        for route in (0, 1):
            monkeypatch.setattr(debug.sw, "bev_one_launch", route)
            obs = dict(depth=dev(c["depth"]), gps=dev(c["gps"]), compass=dev(c["compass"]))
            del calls[:]
            egos[route] = maps[route](dev(c["feat"]), obs, dev(c["masks"]))
            assert obs["rgb_ego_map"] is egos[route]
            if route:
                assert calls == names, calls
            else:
                assert "wsmg_map_fuse_retrieve" not in calls and "wsmg_bev_project" not in calls and len(calls) == 4, calls
        assert egos[0].shape == (B, C, E, E)
        same_bits(egos[1], egos[0], f"step {step} rgb_ego_map")
        same_bits(maps[1].full_global_map, maps[0].full_global_map, f"step {step} full_global_map")
    assert float(egos[1].max()) > 0
