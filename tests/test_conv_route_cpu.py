"""CPU: the route of the bf16 conv engine (wsmg_conv_route_bf16, csrc/wsmg_conv_route.hip) is the dispatch the engine had when each pass
decided by an if-cascade of its own.  The query is host arithmetic; without a device the library takes 256 CUs, the MI355X's count, so
every number here is the one a launch on that device uses.  The expected families and tiles were written by reading the cascades of the
commit before the route existed (conv_fwd_bf16_impl, conv_bwd_data_bf16_impl, wgrad_plan_bf16 and the entry points they fell through);
the slab counts were recorded from that commit's wsmg_conv2d_bwd_weight_bf16_plan, built on its own and called without a device."""
import os
import subprocess
import sys

import pytest

import conv_route_util as U
from conv_route_util import BWD_DATA, BWD_WEIGHT, F32, FWD, RELU_Y, SLICE, SPLIT, STATS, dims, route, route_rc

# name, Cin, Cout, k, stride, pad, H: the LAYERS of tools/bench_conv.py, the sixteen conv shapes of an update, at B = 512
LAYERS = [
    ("enc0_k8s2", 64, 64, 8, 2, 3, 100), ("enc3_k5s2", 64, 128, 5, 2, 1, 50), ("enc6_k3", 128, 256, 3, 1, 1, 24),
    ("encoded_lin_k3", 256, 128, 3, 1, 1, 24), ("orig0_k3", 256, 64, 3, 1, 1, 24), ("orig1_k3", 64, 64, 3, 1, 1, 24),
    ("stem_k7s2", 256, 64, 7, 2, 3, 24), ("block_k3_6", 64, 64, 3, 1, 1, 6), ("up0_k3_12", 128, 128, 3, 1, 1, 12),
    ("orig2_k3", 192, 64, 3, 1, 1, 24), ("convT_adj_k4s2", 32, 64, 4, 2, 1, 48), ("cls_k3_48", 32, 32, 3, 1, 1, 48),
    ("classified_k3", 32, 128, 3, 1, 1, 24), ("cated_k3", 256, 256, 3, 1, 1, 24), ("l0_1x1_12", 64, 64, 1, 1, 0, 12),
    ("l1_1x1_6", 64, 64, 1, 1, 0, 6),
]
# name -> (forward, backward-data, weight gradient): (family, 3 x 3 window tile) twice, then (family, nsplit).  The nsplit column is the
# earlier commit's plan call.
I0 = ("IGEMM", 0)
EXPECT = {
    "enc0_k8s2": (("STEM_WIN", 0), I0, ("WGRAD_STEM_WIN", 64)),
    "enc3_k5s2": (I0, I0, ("WGRAD_S2WIN", 48)),
    "enc6_k3": (("WIN3", 512), ("WIN3", 256), ("WGRAD_WIN3", 64)),           # 576 x 2 = 1152 tiles of 512 forward, 576 x 1 backward
    "encoded_lin_k3": (("WIN3", 256), ("WIN3", 512), ("WGRAD_WIN3", 64)),
    "orig0_k3": (("WIN3", 512), ("WIN3", 512), ("WGRAD_WIN3", 64)),          # 64-channel tiles forward (Kc = 256), 128-channel backward
    "orig1_k3": (I0, I0, ("WGRAD_WIN3", 256)),                                # 64 -> 64: Kc < 128 and N < 192
    "stem_k7s2": (I0, I0, ("WGRAD_S2WIN", 16)),
    "block_k3_6": (I0, I0, ("WGRAD", 36)),                                    # 18 432 pixels
    "up0_k3_12": (I0, I0, ("WGRAD", 43)),                                     # 73 728 pixels; rows of 12 < 16 for the window gradient
    "orig2_k3": (("WIN3", 512), ("WIN3", 512), ("WGRAD_WIN3", 74)),
    "convT_adj_k4s2": (I0, ("CONVT_K4S2", 0), ("WGRAD", 192)),
    "cls_k3_48": (("WIN3_K32", 0), ("WIN3_K32", 0), ("WGRAD_WIN3", 256)),
    "classified_k3": (("WIN3_K32", 0), ("WIN3", 256), ("WGRAD_WIN3", 256)),   # backward: Kc = 128, 32-channel tiles
    "cated_k3": (("WIN3", 512), ("WIN3", 512), ("WGRAD_WIN3", 32)),
    "l0_1x1_12": (I0, I0, ("WGRAD", 144)),
    "l1_1x1_6": (I0, I0, ("WGRAD", 36)),
}
GEOM = {name: dims(512, *rest) for name, *rest in LAYERS}


def fam(pass_, geom, needs=0):
    r = route(pass_, geom, needs)
    return r["kind"], r["mt"]


class tile:
    """The tests' tile switch (wsmg_conv_debug_win3_tile) for a block, restored after it."""

    def __init__(self, mt):
        self.mt = mt

    def __enter__(self):
        from wsmgmap import _abi
        self.prev = _abi.lib().wsmg_conv_debug_win3_tile(self.mt)

    def __exit__(self, *exc):
        from wsmgmap import _abi
        _abi.lib().wsmg_conv_debug_win3_tile(self.prev)


@pytest.fixture(autouse=True)
def _by_shape():
    """Every test starts from the default state (tile by shape) and none of the tunes set: the numbers below are the defaults'."""
    assert not [k for k in os.environ if k.startswith(("WSMG_CONV", "WSMG_WGRAD"))]
    with tile(1):
        yield


@pytest.mark.parametrize("name", [n for n, *_ in LAYERS])
def test_workload_layers_take_the_kernels_the_cascades_chose(name):
    fwd, bwd, wg = EXPECT[name]
    g = GEOM[name]
    assert fam(FWD, g) == fwd and fam(BWD_DATA, g) == bwd
    r = route(BWD_WEIGHT, g)
    assert (r["kind"], r["nsplit"]) == wg and U.plan_nsplit(g) == wg[1]
    # a window route chosen by shape says so; the statistics bit moves nothing
    for p, want in ((FWD, fwd), (BWD_DATA, bwd)):
        assert route(p, g)["by_shape"] == (1 if want[0] == "WIN3" else 0)
        assert route(p, g, STATS) == route(p, g)


# the eleven WGRAD geometries of tests/test_gpu_kernel_instances.py (B, Cin, Cout, k, stride, pad, H, W) and the four stride-2 cases of
# tests/test_gpu_round4.py (B, H, Cin, Cout, k, pad); nsplit from the earlier commit's plan call
WGRAD_GEN = [((11, 256, 128, 3, 2, 1, 13, 17), 2), ((7, 128, 128, 5, 1, 2, 11, 9), 2), ((5, 64, 128, 5, 1, 2, 13, 10), 2),
             ((5, 32, 128, 7, 1, 3, 12, 11), 2), ((5, 96, 128, 5, 1, 2, 9, 14), 2), ((3, 64, 32, 8, 1, 3, 14, 17), 2),
             ((5, 128, 64, 1, 1, 0, 13, 9), 2), ((13, 256, 96, 3, 2, 1, 15, 11), 2), ((3, 64, 96, 3, 2, 1, 25, 31), 2),
             ((5, 32, 32, 1, 1, 0, 21, 13), 3), ((5, 96, 64, 3, 2, 1, 19, 23), 2)]
WGRAD_S2 = [((37, 50, 64, 128, 5, 1), 48), ((3, 50, 64, 128, 5, 1), 16), ((45, 24, 256, 64, 7, 3), 16), ((2, 24, 256, 64, 7, 3), 8)]


def test_slab_counts_are_the_recorded_ones():
    for cfg, ns in WGRAD_GEN:
        g = dims(*cfg)
        r = route(BWD_WEIGHT, g)
        assert (r["kind"], r["nsplit"]) == ("WGRAD", ns) and U.plan_nsplit(g) == ns, cfg
        assert r["chunk"] % 64 == 0 and -(-(g[0] * g[9] * g[10]) // r["chunk"]) == ns and r["gx"] >= 1 and r["gy"] >= 1
    for (B, H, Cin, Cout, k, p), ns in WGRAD_S2:
        g = dims(B, Cin, Cout, k, 2, p, H)
        r = route(BWD_WEIGHT, g)
        assert (r["kind"], r["nsplit"]) == ("WGRAD_S2WIN", ns) and U.plan_nsplit(g) == ns, (B, H)


def k3(B, H, W, Cin, Cout):
    return dims(B, Cin, Cout, 3, 1, 1, H, W)


def test_pixel_count_thresholds_of_the_window_kernels():
    # 65 536 pixels: below it no 3 x 3 window kernel at all — seen with a forced tile (by shape the bar is 131 072) and in the weight gradient
    below, at = k3(257, 15, 17, 64, 128), k3(256, 16, 16, 64, 128)
    assert below[0] * 15 * 17 == 65535 and at[0] * 256 == 65536
    with tile(256):
        assert fam(FWD, below) == I0 and fam(BWD_DATA, below) == I0
        assert fam(FWD, at) == ("WIN3", 256) and route(FWD, at)["by_shape"] == 0
        assert fam(BWD_DATA, k3(256, 16, 16, 128, 64)) == ("WIN3", 256)
    assert route(BWD_WEIGHT, below)["kind"] == "WGRAD" and route(BWD_WEIGHT, at)["kind"] == "WGRAD_WIN3"
    assert fam(FWD, at) == I0                       # by shape: under 131 072
    # 131 072 pixels by shape, for the 128-, 64- and 32-channel tiles and the k32 kernel.  131 071 is prime: only maps one pixel wide
    # reach it, whose windows never fit (asserted last); 514 x 15 x 17 = 131 070 is the largest count below the bar with a real map.
    for Cin, Cout, want in ((64, 128, ("WIN3", 256)), (128, 64, ("WIN3", 512)), (64, 32, ("WIN3", 256)), (32, 32, ("WIN3_K32", 0)),
                            (32, 64, ("WIN3_K32", 0)), (32, 128, ("WIN3_K32", 0))):
        assert fam(FWD, k3(514, 15, 17, Cin, Cout)) == I0, (Cin, Cout)
        assert fam(FWD, k3(512, 16, 16, Cin, Cout)) == want, (Cin, Cout)
        assert fam(BWD_DATA, k3(514, 15, 17, Cout, Cin)) == I0 and fam(BWD_DATA, k3(512, 16, 16, Cout, Cin)) == want, (Cin, Cout)
    assert fam(FWD, k3(131071, 1, 1, 64, 128)) == I0 and fam(FWD, k3(131071, 1, 1, 32, 32)) == I0
    # ConvTranspose: 131 072 input pixels
    assert fam(BWD_DATA, dims(512, 32, 64, 4, 2, 1, 32)) == ("CONVT_K4S2", 0)         # 512 x 16 x 16
    assert fam(BWD_DATA, dims(511, 32, 64, 4, 2, 1, 32)) == I0
    assert fam(BWD_DATA, dims(128, 32, 64, 4, 2, 1, 64)) == I0                        # 128 x 32 x 32: a 128-pixel tile's window needs 275 of 256 entries


def test_channel_thresholds_of_the_window_kernels():
    B, H = 512, 16                                                    # 131 072 pixels
    assert fam(FWD, k3(B, H, H, 32, 256)) == I0                       # Kc = 32 outside the k32 kernel's widths: nine k-steps, no window
    assert fam(FWD, k3(B, H, H, 64, 256)) == ("WIN3", 256)
    assert fam(FWD, k3(B, H, H, 32, 192)) == I0 and fam(FWD, k3(B, H, H, 64, 192)) == ("WIN3", 512)    # N = 192 >= 192
    assert fam(FWD, k3(B, H, H, 64, 64)) == I0                        # N = 64 with Kc = 64: one 64-channel tile, 18 k-steps
    assert fam(FWD, k3(B, H, H, 128, 64)) == ("WIN3", 512)
    assert fam(FWD, k3(512, 12, 12, 128, 128)) == I0                  # 73 728 pixels, N = 128
    # 512-pixel tiles from 1024 tiles on (4 rounds over 256 CUs), 256-pixel tiles below
    assert fam(FWD, k3(2046, 16, 16, 64, 128)) == ("WIN3", 256)       # 1023 tiles of 512
    assert fam(FWD, k3(2047, 16, 16, 64, 128)) == ("WIN3", 512)       # 1023.5 -> 1024
    assert fam(FWD, k3(1022, 16, 16, 64, 256)) == ("WIN3", 256) and fam(FWD, k3(1023, 16, 16, 64, 256)) == ("WIN3", 512)


def test_a_window_that_does_not_fit_leaves_the_layer_on_the_implicit_gemm_kernel():
    """wsmg_win3_window_bound(512, 10, 12) = 769 entries against the 768 of six window pieces per wave — over by one, less than a padded
    row of 14 — and 745 at 10 x 13.  The choice by pixel count says 512 for both; the fits test of the kernel's file decides."""
    with tile(512):
        assert fam(FWD, k3(547, 10, 12, 64, 128)) == I0 and fam(BWD_DATA, k3(547, 10, 12, 128, 64)) == I0
        assert fam(FWD, k3(547, 10, 13, 64, 128)) == ("WIN3", 512)
    # the k32 kernel's 512-entry window (256-pixel tiles): 4 x 31 needs 541, 5 x 31 fits; the layer then takes the general window
    # kernel's 256-pixel tile if that fits, else the implicit-GEMM kernel
    assert fam(FWD, k3(1058, 4, 31, 32, 32)) == I0 and fam(FWD, k3(1058, 5, 31, 32, 32)) == ("WIN3_K32", 0)


def test_stem_and_stride2_geometries_one_step_off():
    for B in (3, 512):
        assert fam(FWD, dims(B, 64, 64, 8, 2, 3, 100)) == ("STEM_WIN", 0)
        assert fam(FWD, dims(B, 64, 64, 8, 2, 2, 100)) == I0                                     # pad 2
        assert route(BWD_WEIGHT, dims(B, 64, 64, 8, 2, 3, 100))["kind"] == "WGRAD_STEM_WIN"
        assert route(BWD_WEIGHT, dims(B, 64, 64, 8, 2, 2, 100))["kind"] == "WGRAD"
    assert fam(FWD, dims(512, 64, 128, 8, 2, 3, 100)) == I0 and fam(BWD_DATA, dims(512, 64, 64, 8, 2, 3, 100)) == I0
    for cfg, H_in, H_off in (((64, 128, 5, 2, 1), 50, 48), ((256, 64, 7, 2, 3), 24, 26)):
        assert route(BWD_WEIGHT, dims(512, *cfg, H_in))["kind"] == "WGRAD_S2WIN"
        assert route(BWD_WEIGHT, dims(512, *cfg, H_off))["kind"] == "WGRAD"
    # ConvTranspose with an odd output: H = 2 OH + 1
    g = dims(512, 32, 64, 4, 2, 1, 49)
    assert (g[1], g[9]) == (49, 24) and fam(BWD_DATA, g) == I0
    assert fam(BWD_DATA, dims(512, 32, 64, 4, 2, 1, 48)) == ("CONVT_K4S2", 0)
    assert fam(BWD_DATA, dims(512, 64, 64, 4, 2, 1, 48)) == I0 and fam(BWD_DATA, dims(512, 32, 128, 4, 2, 1, 48)) == I0


def test_needs_bits_move_the_route_as_the_cascades_did():
    stem, cls, convt, cated = GEOM["enc0_k8s2"], GEOM["cls_k3_48"], GEOM["convT_adj_k4s2"], GEOM["cated_k3"]
    assert fam(FWD, stem, SLICE) == I0                                      # a channel-slice output takes the stem off its window kernel
    assert fam(FWD, cls, SLICE) == ("WIN3_K32", 0) and fam(FWD, cated, SLICE) == ("WIN3", 512)      # the 3 x 3 kernels write slices
    for bit in (RELU_Y, SPLIT, RELU_Y | SPLIT):                             # mask / split: the general window kernel, not k32 or ConvTranspose
        assert fam(BWD_DATA, cls, bit) == ("WIN3", 256) and fam(BWD_DATA, convt, bit) == I0
        assert fam(BWD_DATA, cated, bit) == ("WIN3", 512)
    for name in EXPECT:                                                     # float32 or accumulated output: no window kernel
        assert fam(FWD, GEOM[name], F32) == I0 and fam(BWD_DATA, GEOM[name], F32) == I0, name
        assert fam(FWD, GEOM[name], F32 | STATS) == I0


def test_forced_tile_and_off_state():
    cls, convt, cated, enc6 = GEOM["cls_k3_48"], GEOM["convT_adj_k4s2"], GEOM["cated_k3"], GEOM["enc6_k3"]
    for mt in (256, 512):
        with tile(mt):                                                      # a forced tile: general window kernel, by_shape 0; k32 / ConvTranspose off
            assert fam(FWD, cls) == ("WIN3", mt) and fam(BWD_DATA, convt) == I0 and fam(BWD_DATA, enc6) == ("WIN3", mt)
            assert route(FWD, cated)["by_shape"] == 0
            assert route(BWD_WEIGHT, cated)["kind"] == "WGRAD_WIN3"
    with tile(0):
        assert fam(FWD, cls) == I0 and fam(FWD, cated) == I0 and fam(BWD_DATA, convt) == I0
        assert route(BWD_WEIGHT, cated)["kind"] == "WGRAD" and route(BWD_WEIGHT, GEOM["enc0_k8s2"])["kind"] == "WGRAD_STEM_WIN"


def test_query_refuses_before_it_answers():
    g = GEOM["cated_k3"]
    assert route_rc(3, g)[0] == -1 and route_rc(-1, g)[0] == -1
    assert route_rc(FWD, g, RELU_Y)[0] == -1 and route_rc(BWD_DATA, g, SLICE)[0] == -1 and route_rc(BWD_WEIGHT, g, STATS)[0] == -1
    assert route_rc(FWD, g, 32)[0] == -1
    assert route_rc(FWD, g[:9] + (23, 24))[0] == -1                         # OH that is not the convolution's
    assert route_rc(FWD, dims(512, 48, 64, 3, 1, 1, 24))[0] == -1           # channels no multiple of 32
    from wsmgmap import _abi
    assert _abi.lib().wsmg_conv_route_bf16(FWD, *g, 0, None) == -1
    assert len(U.FAMILY) == 9 and sorted(U.FAMILY) == list(range(9)) and U.WORDS == 9 == len(U.FIELDS)


def test_one_tune_in_a_fresh_process():
    """Tunes are read once per process: a child with WSMG_CONV_K32=0 sends the classifier's 32 -> 32 layer to the general window kernel."""
    code = ("import sys; sys.path[:0] = %r\n"
            "import conv_route_util as U\n"
            "g = U.dims(512, 32, 32, 3, 1, 1, 48)\n"
            "print([(U.route(p, g)['kind'], U.route(p, g)['mt'], U.route(p, g)['by_shape']) for p in (U.FWD, U.BWD_DATA)])\n"
            % [os.path.dirname(os.path.abspath(__file__)), os.path.join(U.ROOT, "ws-mgmap_amd"), U.ROOT])
    out = subprocess.run([sys.executable, "-c", code], env={**os.environ, "WSMG_CONV_K32": "0"}, capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    assert out.stdout.strip() == str([("WIN3", 256, 1)] * 2), out.stdout
