"""The map operator (csrc/wsmg_bev.hip: index, scatter-max, first rotation, paste + translate + max-fuse, crop, final rotation)
against the ORACLE at the edges the G2 sequence does not reach: the ego window leaving the global map, headings whose sampling
coordinates land on pixel centres, odd E, odd G, G == E and the cfg4 geometry.  The kernel-against-kernel tests
(test_bev_scatter_rotate_and_plane_fuse_equal_the_separate_launches, test_map_retrieve_lds_tiles_equal_crop_then_rotate) hold the
fast launches bit for bit to wsmg_bev_rotate / wsmg_map_fuse / wsmg_map_retrieve; this file holds those base launches — and the
fast ones once more — to the reference's arithmetic there.

Float bar.  The yardstick is the reference's own float32 distance from its float64 evaluation of the same case,
`d32 = max|oracle32 - oracle64|` (CPU only, no code under test in it); a kernel is compared with oracle64 and has to stay within
`K_TOL * d32`, per case and tensor — its float32 arithmetic is of ATen's kind in another order, so its distance is of d32's size.
Every case also requires `d32 <= 1e-4 * (grid / 240) * max|values|`: the project's 2e-4 rule (G = 240, |feature| <= 2), scaled.
The integer gate is bit-exact.
"""
import math

import numpy as np
import pytest
import torch

from oracle import bev_ref, cases
from oracle import detfill as df
from util import T

pytestmark = pytest.mark.gpu

HF = 64
RES = 0.12
HEADINGS = [0.0, math.pi / 2, -math.pi / 2, math.pi, math.pi / 4, -1.3]
# (E, C, G): default, cfg4, odd E, odd E and odd G, G == E
GEOMS = [(100, 64, 240), (200, 40, 480), (33, 8, 64), (33, 8, 65), (24, 8, 24)]
GEOM_IDS = ["e100_c64_g240", "e200_c40_g480", "e33_c8_g64", "e33_c8_g65", "e24_c8_g24"]
# k = twice the worst measured ratio `|kernel - oracle64| / d32`, rounded up: 1.99 (the table in the first test's docstring) -> 4.
# A ratio above 4 is a finding about a kernel, not a tolerance: it is explained from the code, never absorbed here.
K_TOL = 4


@pytest.fixture(scope="module")
def ops():
    from wsmgmap import ops as o
    return o


def dev(a):
    return (a if torch.is_tensor(a) else T(a)).cuda()


def headings(first, B):
    """[B, 1] float32: HEADINGS[first + b], cyclically."""
    return torch.tensor([[HEADINGS[(first + b) % len(HEADINGS)]] for b in range(B)], dtype=torch.float32)


def gps_cells(name, B, G, reach, flip=0):
    """gps [B, 2] float32 = (integer cell + 0.25) * 0.12 with |cell| <= reach * G / 2: sample 0 at the full reach (+, -), sample 1
    at (-, drawn) or, with `flip`, (drawn, +), the rest drawn within half the reach (they stay inside the map and fill it).  The quarter keeps every rounding of `grid_cell` a quarter cell away from a tie — asserted
    here, on the CPU: a flipped tie would be an error of a whole cell, and this file tests sampling."""
    r = int(round(reach * G / 2))
    n = np.rint(df.uniform(name, (B, 2), 2.0).astype(np.float64) * r).astype(np.int64)    # in [-r, r]
    n[0] = (r, -r)
    if B > 1:
        n[1, flip] = r if flip else -r
    n[2:] = np.rint(n[2:] * 0.5)
    gps = ((n.astype(np.float32) + np.float32(0.25)) * np.float32(RES)).astype(np.float32)
    cmax, cmin = G * RES / 2, -G * RES / 2
    gs = (cmax - cmin) / G
    t = T(gps)
    for pre in ((cmax - t[:, 0]) / gs, (t[:, 1] - cmin) / gs):     # grid_cell's arguments of round(), float32 as there
        frac = (pre.double() - torch.floor(pre.double())).numpy()
        assert np.all(np.abs(frac - 0.5) >= 0.2), f"{name}: a cell rounding within 0.3 of a tie ({frac})"
    return gps


class Figures:
    """Collects `kernel distance / d32` per case and tensor: printed as measured, asserted together at the end of a test."""

    def __init__(self):
        self.bad = []

    def condition(self, name, d32, grid, vmax):
        lim = 1e-4 * (grid / 240.0) * vmax
        print(f"D32 {name}: d32 {d32:.3e} limit {lim:.3e}")
        if not d32 <= lim:
            self.bad.append(f"{name}: the reference's own d32 {d32:.3e} exceeds 1e-4 * ({grid}/240) * {vmax:.3g} = {lim:.3e}")

    def check(self, name, got, ref64, d32):
        dist = float((got.detach().double().cpu() - ref64).abs().max())
        ratio = dist / d32 if d32 > 0 else (0.0 if dist == 0 else float("inf"))
        print(f"RATIO {name}: kernel {dist:.3e} d32 {d32:.3e} ratio {ratio:.2f}")
        if not dist <= K_TOL * d32:
            self.bad.append(f"{name}: |kernel - oracle64| {dist:.3e} > {K_TOL} * d32 ({d32:.3e}), ratio {ratio:.2f}")

    def done(self):
        assert not self.bad, "\n".join(self.bad)


def dmax(a, b):
    return float((a.double() - b.double()).abs().max())


# ----------------------------------------------------------------------------- (a) fuse + retrieve sequence
REACH = [0.3, 1.0, 0.97, 1.2]      # fraction of the map half-width; the last puts the window partly off the map


def floor_depth(name, B, E):
    """depth_raw [B,256,256,1] (sensor units of 10 m) that fills an E-cell ego map: below the horizon a random depth up to the map's
    far edge (E / 2 cells of 0.12 m) or to where the ray meets 1.45 m under the camera, whichever is nearer — every such source
    passes the height filter and lands inside the map; above the horizon random depths, which the filter drops; 8 zero rows."""
    zmax = E * RES / 2
    yy = (128.0 - np.arange(256)) / 128.0                       # (y - cy) / fy of ComputeSpatialLocs, y = 256 - row
    row_max = np.where(yy < 0, np.minimum(zmax, 1.45 / np.maximum(-yy, 1e-9)), zmax).astype(np.float32)
    depth = (df.uniform(name, (B, 256, 256, 1)) + np.float32(0.5)) * (row_max / np.float32(10))[None, :, None, None]
    depth[:, :8] = 0.0
    return depth.astype(np.float32)


def seq_inputs(tag, step, B, E, C, G):
    depth = floor_depth(f"{tag}.depth.{step}", B, E)
    feat = np.clip(df.uniform(f"{tag}.feat.{step}", (B, C, HF, HF), 4.0) + np.float32(1.5), 0.0, 2.0)   # post-ReLU, clamped to <= 2
    masks = np.ones((B, 1), np.float32)
    if step == 2:
        masks[0] = 0.0
    return dict(depth=depth, feat=feat, gps=gps_cells(f"{tag}.gps.{step}", B, G, REACH[step], flip=1 - step % 2), compass=headings(step * B, B), masks=masks)


@pytest.mark.parametrize("E,C,G", GEOMS, ids=GEOM_IDS)
def test_fuse_retrieve_sequence_vs_float64_oracle_at_the_edges(ops, E, C, G):
    """Four steps of index / scatter-max / rotation / fuse / retrieve, once with the base launches (bev_scatter_max, bev_rotate,
    map_fuse, map_retrieve as crop then rotation) and once on the default route (bev_scatter_rotate, map_fuse on planes, the
    LDS-tiled retrieve): the global map and the ego map after every step against MapperRef in float64.  Headings cycle through
    0, +-pi/2, pi, pi/4, -1.3; the agents reach 0.3, 1.0, 0.97 and 1.2 of the map's half-width; step 2 resets sample 0.

    Measured `|kernel - oracle64| / d32` on an MI355X, worst case (step, trial or batch) of each geometry and tensor; the base and
    the default route give the same figures (they are bit-identical), as do the three forms of the retrieve.  Every check prints
    its figure (`RATIO ...`, shown with -s).

        (E, C, G)        sequence: global map   ego map     retrieve of a dense map
        (100, 64, 240)             1.11         0.97        1.44
        (200, 40, 480)             1.15         1.11        1.00
        (33, 8, 64)                1.55         1.70        1.99
        (33, 8, 65)                1.06         1.02        1.05
        (24, 8, 24)                1.00         1.26        1.14

        E                bev_rotate   bev_scatter_rotate
        24               1.29         1.00
        33               1.00         1.00
        100              1.00         1.07
        200              1.00         1.00

    Worst 1.99 -> K_TOL = 4.  No ratio is above 4: no divergence at these edges.
    """
    B = 3
    tag = f"edges.seq.{E}.{C}.{G}"
    assert ops.bev_planes_ok(C, E)
    ref64 = bev_ref.MapperRef(B, G, E, C, RES, dtype=torch.float64)
    ref32 = bev_ref.MapperRef(B, G, E, C, RES)
    gms = {"base": torch.zeros(B, G, G, C, device="cuda"), "default": torch.zeros(B, G, G, C, device="cuda")}
    fig = Figures()
    for step in range(4):
        c = seq_inputs(tag, step, B, E, C, G)
        args = (T(c["feat"]), T(c["depth"]), T(c["gps"]), c["compass"], T(c["masks"]))
        ego64, ego32 = ref64.step(*args), ref32.step(*args)
        d_map, d_ego = dmax(ref32.full_global_map, ref64.full_global_map), dmax(ego32, ego64)
        vmax = float(c["feat"].max())
        fig.condition(f"s{step}.global", d_map, G, vmax)
        fig.condition(f"s{step}.ego", d_ego, G, vmax)
        feat, gps = dev(c["feat"]), dev(c["gps"])
        compass, masks = dev(c["compass"]).reshape(-1).contiguous(), dev(c["masks"]).reshape(-1).contiguous()
        lin = ops.bev_index(dev(c["depth"][..., 0]), HF, HF, E)
        egos = {}
        rot = ops.bev_rotate(ops.bev_scatter_max(feat, lin, C, E), compass, -1.0)
        ops.map_fuse(rot, gms["base"], gps, masks, RES)
        egos["base"] = ops.map_retrieve(gms["base"], gps, compass, E, RES, fused=False)
        rotp = ops.bev_scatter_rotate(feat, lin, compass, -1.0, C, E)
        ops.map_fuse(rotp, gms["default"], gps, masks, RES, planes=True)
        egos["default"] = ops.map_retrieve(gms["default"], gps, compass, E, RES)
        for route in ("base", "default"):
            fig.check(f"{route}.s{step}.global", gms[route], ref64.full_global_map, d_map)
            fig.check(f"{route}.s{step}.ego", egos[route].permute(0, 3, 1, 2), ego64, d_ego)
    for route in ("base", "default"):       # the sequence is not trivially zero (the oracle gives 3 - 40 % non-zeros on such inputs)
        for name, t in (("global", gms[route]), ("ego", egos[route])):
            nz = float((t != 0).float().mean())
            print(f"NONZERO {route}.{name}: max {float(t.max()):.3f}, non-zero {100 * nz:.1f} %")
            assert float(t.max()) > 0 and nz > 0.01, (route, name, nz)
    fig.done()


# ----------------------------------------------------------------------------- (b) retrieve alone, dense map
@pytest.mark.parametrize("E,C,G", GEOMS, ids=GEOM_IDS)
def test_retrieve_of_a_dense_map_vs_float64_oracle(ops, E, C, G):
    """map_retrieve in its three forms (crop then rotation, the register form, the LDS-tiled default) on a dense normal map — every
    tap carries weight, negative values included (retrieval is linear) — against bev_ref.retrieve in float64: the six headings,
    agents in the centre, on the border and beyond it (reach 0, 1.0, 1.4: taps outside the global map).  Finite inputs only."""
    B = 2
    g = torch.Generator().manual_seed(1000 + E + G)
    gm = torch.randn(B, G, G, C, generator=g)
    gm_dev = gm.cuda()
    vmax = float(gm.abs().max())
    fig = Figures()
    for trial, reach in enumerate((0.0, 1.0, 1.4)):
        gps = gps_cells(f"edges.ret.{E}.{G}.{trial}", B, G, reach)
        compass = headings(trial * B, B)
        want = bev_ref.retrieve(gm, T(gps), compass, E, RES, dtype=torch.float64)
        d32 = dmax(bev_ref.retrieve(gm, T(gps), compass, E, RES), want)
        fig.condition(f"t{trial}", d32, G, vmax)
        for form in (False, True, "tiled"):
            got = ops.map_retrieve(gm_dev, dev(gps), dev(compass).reshape(-1).contiguous(), E, RES, fused=form)
            fig.check(f"t{trial}.fused={form}", got.permute(0, 3, 1, 2), want, d32)
    fig.done()


# ----------------------------------------------------------------------------- (c) the first rotation alone
@pytest.mark.parametrize("E,C", [(24, 8), (33, 8), (100, 64), (200, 40)], ids=["e24", "e33", "e100", "e200"])
def test_first_rotation_vs_float64_oracle(ops, E, C):
    """bev_rotate on dense normal planes, and bev_scatter_rotate on the oracle's own scatter-max planes (project_to_ground),
    against bev_ref.rotate in float64, at the six headings (two batches of three, rotating by -heading as the operator does and by
    +heading).  The grid of this sampling is E wide: the d32 condition scales with E."""
    B = 3
    g = torch.Generator().manual_seed(2000 + E)
    fig = Figures()
    for batch, sign in enumerate((-1.0, 1.0)):
        heading = headings(batch * B, B)
        planes = torch.randn(B, C, E, E, generator=g)
        want = bev_ref.rotate(planes, sign * heading, dtype=torch.float64)
        d32 = dmax(bev_ref.rotate(planes, sign * heading), want)
        fig.condition(f"dense.b{batch}", d32, E, float(planes.abs().max()))
        got = ops.bev_rotate(planes.cuda(), dev(heading).reshape(-1).contiguous(), sign)
        fig.check(f"bev_rotate.b{batch}", got.permute(0, 3, 1, 2), want, d32)

        depth = floor_depth(f"edges.rot.depth.{E}.{batch}", B, E)
        feat = np.clip(df.uniform(f"edges.rot.feat.{E}.{batch}", (B, C, HF, HF), 4.0), 0.0, 2.0)
        proj, lin_ref, inv_ref, *_ = bev_ref.project_to_ground(feat, depth, E)
        want = bev_ref.rotate(T(proj), sign * heading, dtype=torch.float64)
        d32 = dmax(bev_ref.rotate(T(proj), sign * heading), want)
        fig.condition(f"scatter.b{batch}", d32, E, float(feat.max()))
        lin = ops.bev_index(dev(depth[..., 0]), HF, HF, E)
        assert np.array_equal(np.where(lin.cpu().numpy() < 0, 0, lin.cpu().numpy()), lin_ref)
        got = ops.bev_scatter_rotate(dev(feat), lin, dev(heading).reshape(-1).contiguous(), sign, C, E)
        assert float(got.abs().max()) > 0
        fig.check(f"bev_scatter_rotate.b{batch}", got, want, d32)
    fig.done()


# ----------------------------------------------------------------------------- (d) the integer gate at odd E
def gate_case(E, Hf, B):
    return cases.bev_inputs_at(f"edges.gate.e{E}.f{Hf}", E, 8, Hf, B)


@pytest.mark.parametrize("Hf", [64, 100])
@pytest.mark.parametrize("E", [33, 101])
def test_integer_gate_at_odd_ego_sizes_bit_exact(ops, E, Hf):
    """bev_index and bev_scatter_max against bev_ref.project_to_ground where `half = (E - 1) / 2` is an integer — the rintf ties
    then sit on other inputs than at the even sizes of the golden cases — and at the sub-sample ratio 256 / 100 = 2.56 (not a
    power of two): validity flags, linear index and the planes' bits.  Structured depth of cases.bev_inputs (zero rows, depths on
    multiples of the cell, an all-invalid sample) plus depths on odd multiples of half a cell, which are this geometry's ties."""
    c = gate_case(E, Hf, 3)
    proj_ref, lin_ref, inv_ref, x_gp, y_gp, valid = bev_ref.project_to_ground(c["feat"], c["depth"], E)
    # the case does carry ties, on valid sources inside the map (the oracle's own arithmetic, float32)
    z = c["depth"][..., 0].astype(np.float32) * np.float32(10)
    pre = -(z / np.float32(RES)) + np.float32((E - 1) / 2)
    ih = bev_ref.subsample_index(Hf, 256)
    tie = (np.abs(pre - np.floor(pre)) == 0.5) & valid & (y_gp >= 0) & (y_gp < E) & (x_gp >= 0) & (x_gp < E)
    assert int(tie[:, ih[:, None], ih[None, :]].sum()) > 0, "no sub-sampled source on a rounding tie"
    lin = ops.bev_index(dev(c["depth"][..., 0]), Hf, Hf, E)
    lin_h = lin.cpu().numpy()
    got_inv = lin_h < 0
    assert np.array_equal(got_inv, inv_ref), f"{int((got_inv != inv_ref).sum())} validity flags differ"
    assert np.array_equal(np.where(got_inv, 0, lin_h), lin_ref), "linear cell index differs"
    assert got_inv[2].all() and not got_inv[0].all()
    proj = ops.bev_scatter_max(dev(c["feat"]), lin, 8, E).cpu().numpy()
    assert np.array_equal(proj.view(np.uint32), proj_ref.view(np.uint32)), f"scatter-max differs in {int((proj != proj_ref).sum())} cells"


@pytest.mark.parametrize("E,Hf", [(33, 64), (33, 100), (101, 64), (101, 100), (200, 256)],
                         ids=["e33_f64", "e33_f100", "e101_f64", "e101_f100", "e200_f256_sources_at_the_limit"])
def test_compacted_route_equals_the_plain_one_at_odd_ego_sizes(ops, E, Hf):
    """bev_index_compact + bev_scatter_rotate(compact=...) at B = 4 (the batch from which the rollout takes this route) against
    bev_index + bev_scatter_rotate on the same inputs, bit for bit; the index also against the oracle.  (200, 256): Hf * Wf ==
    65536 alone at the packing limit is still taken."""
    assert ops.bev_compact_ok(Hf, Hf, E, 4)
    c = gate_case(E, Hf, 4)
    _, lin_ref, inv_ref, *_ = bev_ref.project_to_ground(c["feat"], c["depth"], E)
    depth, feat = dev(c["depth"][..., 0]), dev(c["feat"])
    lin0 = ops.bev_index(depth, Hf, Hf, E)
    lin, comp = ops.bev_index_compact(depth, Hf, Hf, E)
    assert torch.equal(lin, lin0)
    lin_h = lin.cpu().numpy()
    assert np.array_equal(lin_h < 0, inv_ref) and np.array_equal(np.where(lin_h < 0, 0, lin_h), lin_ref)
    assert int(comp[1].sum()) == int((~inv_ref).sum())
    heading = dev(headings(4, 4)).reshape(-1).contiguous()
    a = ops.bev_scatter_rotate(feat, lin, heading, -1.0, 8, E)
    b = ops.bev_scatter_rotate(feat, lin, heading, -1.0, 8, E, compact=comp)
    assert float(a.abs().max()) > 0
    assert torch.equal(a.view(torch.int32), b.view(torch.int32)), f"{int((a != b).sum())} elements differ"
