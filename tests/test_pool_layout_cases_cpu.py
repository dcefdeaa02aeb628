"""CPU: the cases of tests/pool_layout_cases.py are what tests/test_gpu_pool_layout_edges.py needs them to be.

1. max-pool: every tie-heavy geometry larger than 2 x 3 has at least half of its windows tied and border windows whose first valid tap
   is not tap 0 (some of them tied and won by that tap); the signed input has its -inf element and its all -inf window and nothing
   that is NaN; the tap decoded from ATen's flat index equals the first maximum found by comparing the nine taps;
2. every arithmetic reference is float64;
3. every pool / upsampling geometry differs from the old 3 x 64 x 12 x 12 case in an odd size, H != W or C % 8 != 0, and every transpose
   case takes the kernel its comment names;
4. the derived bars (token-gradient merge, slab reduction) are met by the same arithmetic in float32 on the CPU, and broken by the
   mistakes they are there to catch (another batch row's g; a swapped kh / kw stride)."""
import numpy as np
import pytest
import torch

import pool_layout_cases as pc

GEOM_IDS = [pc.geom_id(g) for g in pc.MAXPOOL_GEOMS]


# ----------------------------------------------------------------------------- 1. max-pool inputs
@pytest.mark.parametrize("geom", [g for g in pc.MAXPOOL_GEOMS if g[1] * g[2] > 6], ids=pc.geom_id)
def test_tie_heavy_input_is_tie_heavy_and_has_contested_border_windows(geom):
    x = pc.maxpool_input(geom, "ties", False)
    st = pc.window_stats(x)
    print(geom, st)
    assert st["tied"] >= 0.5                    # at least half of the windows have a tied maximum
    assert st["border"] >= 1                    # a window whose first valid tap is not tap 0 ...
    assert st["border_won"] >= 1                # ... and one of them tied, with that tap the winner
    assert st["all_zero"] > 0.0


@pytest.mark.parametrize("geom", pc.MAXPOOL_GEOMS, ids=GEOM_IDS)
def test_maxpool_inputs_are_on_their_grids_and_hold_no_nan(geom):
    B, H, W, C = geom
    x = pc.maxpool_input(geom, "ties", False)
    assert torch.equal(x * 4, (x * 4).round()) and float(x.min()) >= 0.0 and float(x.max()) <= 1.0
    assert torch.equal(pc.bf_round(x), x) and torch.equal(pc.maxpool_input(geom, "ties", True), x)      # exact in bf16
    assert not bool(torch.signbit(x[x == 0]).any())
    for bf16 in (False, True):
        s = pc.maxpool_input(geom, "signed", bf16)
        assert not bool(torch.isnan(s).any()) and float(s[torch.isfinite(s)].min()) < 0.0
        assert float(s[0, 0, 0, W - 1]) == pc.NINF
        c = pc.maxpool_case(geom, "signed", bf16)
        n_inf = int((c["y"] == pc.NINF).sum())
        assert n_inf == 1, n_inf                                    # one window is all -inf (at 1 x 1 it is the single element's)
        if pc.pool_out(H) * pc.pool_out(W) > 1:
            assert float(c["y"][B - 1, C - 1, -1, -1]) == pc.NINF and bool(torch.isfinite(c["y"][0, 0]).all())
        if bf16:
            assert torch.equal(pc.bf_round(s), s) and torch.equal(pc.bf_round(c["gy"]), c["gy"])
    g = pc.maxpool_case(geom, "ties", False)["gy"]
    assert torch.equal(g * 4, (g * 4).round()) and float(g.abs().max()) <= 1.0


@pytest.mark.parametrize("bf16", [False, True], ids=["f32", "bf16"])
@pytest.mark.parametrize("kind", pc.MAXPOOL_KINDS)
@pytest.mark.parametrize("geom", pc.MAXPOOL_GEOMS, ids=GEOM_IDS)
def test_maxpool_reference_is_float64_and_its_taps_are_the_first_maximum(geom, kind, bf16):
    B, H, W, C = geom
    c = pc.maxpool_case(geom, kind, bf16)
    OH, OW = pc.pool_out(H), pc.pool_out(W)
    assert c["y"].dtype == torch.float64 and c["dx"].dtype == torch.float64
    assert tuple(c["y"].shape) == (B, C, OH, OW) and tuple(c["dx"].shape) == (B, C, H, W)
    assert bool(torch.isfinite(c["dx"]).all())
    assert c["taps"].dtype == torch.uint8 and tuple(c["taps"].shape) == (B, OH, OW, C)
    assert torch.equal(c["taps"], pc.scan_taps(c["x"]))
    # the gradient is the scatter of gy through those taps: every dx element is the sum of the gy of the windows it won
    want = torch.zeros(B, C, H, W, dtype=torch.float64)
    taps = pc.nchw(c["taps"]).long()
    for oy in range(OH):
        for ox in range(OW):
            iy = 2 * oy - 1 + taps[:, :, oy, ox] // 3
            ix = 2 * ox - 1 + taps[:, :, oy, ox] % 3
            assert int(iy.min()) >= 0 and int(iy.max()) < H and int(ix.min()) >= 0 and int(ix.max()) < W
            want.view(B, C, H * W).scatter_add_(2, (iy * W + ix).unsqueeze(-1), c["gy"][:, :, oy, ox].double().unsqueeze(-1))
    assert torch.equal(want, c["dx"])


# ----------------------------------------------------------------------------- 2. / 3. float64 references, geometries
@pytest.mark.parametrize("op,geom", [("avgpool", g) for g in pc.AVGPOOL_GEOMS] + [("upsample", g) for g in pc.UPSAMPLE_GEOMS],
                         ids=lambda v: v if isinstance(v, str) else pc.geom_id(v))
def test_smooth_references_are_float64(op, geom):
    B, H, W, C = geom
    for bf16 in (False, True):
        c = pc.smooth_case(op, geom, bf16)
        assert c["y"].dtype == torch.float64 and c["dx"].dtype == torch.float64
        oh, ow = (H // 2, W // 2) if op == "avgpool" else (2 * H, 2 * W)
        assert tuple(c["y"].shape) == (B, C, oh, ow) and tuple(c["dx"].shape) == (B, C, H, W)
        assert bool(torch.isfinite(c["y"]).all()) and bool(torch.isfinite(c["dx"]).all())
        if bf16:
            assert torch.equal(pc.bf_round(c["x"]), c["x"]) and torch.equal(pc.bf_round(c["gy"]), c["gy"])


def test_every_pool_geometry_differs_from_the_square_12_x_12_x_64_case():
    assert not pc.differs_from_the_square_case(12, 12, 64)
    geoms = pc.MAXPOOL_GEOMS + pc.AVGPOOL_GEOMS + pc.AVGPOOL_ODD + pc.UPSAMPLE_GEOMS
    for B, H, W, C in geoms:
        assert pc.differs_from_the_square_case(H, W, C), (B, H, W, C)
        assert C % 4 == 0                                  # what the kernels require
    assert len(set(geoms)) == len(geoms)
    for B, H, W, C in pc.AVGPOOL_GEOMS:
        assert H % 2 == 0 and W % 2 == 0
    for B, H, W, C in pc.AVGPOOL_ODD:
        assert H % 2 or W % 2
    hw = [(g[1], g[2]) for g in pc.MAXPOOL_GEOMS]
    assert any(h % 2 and w % 2 == 0 for h, w in hw) and any(h % 2 == 0 and w % 2 for h, w in hw)      # odd in each axis on its own
    assert any(h > w for h, w in hw) and any(h < w for h, w in hw)                                    # both orientations


def test_transpose_cases_take_the_kernel_they_name():
    assert [pc.takes_64_form(cs, h, w, cd) for _, cs, h, w, cd in pc.TO_NHWC_CASES] == pc.TO_NHWC_64_FORM
    assert pc.takes_64_form(64, 100, 100, 64) and not pc.takes_64_form(27, 48, 48, 32)      # the two forms of the older tests
    hw64 = [h * w for (_, cs, h, w, cd), f in zip(pc.TO_NHWC_CASES, pc.TO_NHWC_64_FORM) if f]
    assert any(n < 64 for n in hw64) and any(n % 64 and n % 4 == 0 and n > 4 for n in hw64)
    gen = [(cs, h * w, cd) for (_, cs, h, w, cd), f in zip(pc.TO_NHWC_CASES, pc.TO_NHWC_64_FORM) if not f]
    assert any(cs % 64 == 0 and cs == cd and n % 4 for cs, n, cd in gen)          # 64 channels that fall through
    assert any(cs % 64 == 0 and cd > cs for cs, n, cd in gen)                    # padding from a 64-multiple
    for case in pc.TO_NHWC_CASES:
        B, Cs, H, W, Cd = case
        x, want = pc.to_nhwc_case(case)
        assert tuple(want.shape) == (B, H, W, Cd) and torch.equal(want[..., :Cs], x.permute(0, 2, 3, 1))
        assert Cd == Cs or float(want[..., Cs:].abs().max()) == 0.0
    for case in pc.TO_NCHW_CASES:
        B, Cs, H, W, Cd = case
        for bf16 in (False, True):
            x, want = pc.to_nchw_case(case, bf16)
            assert tuple(want.shape) == (B, Cd, H, W) and Cd <= Cs and want.is_contiguous()
            assert torch.equal(want.permute(0, 2, 3, 1), x[..., :Cd])


# ----------------------------------------------------------------------------- 4. the derived bars
@pytest.mark.parametrize("bf16", [False, True], ids=["f32", "bf16"])
@pytest.mark.parametrize("case", pc.MERGE_CASES, ids=pc.geom_id)
def test_merge_bar_is_met_by_float32_arithmetic_and_broken_by_another_rows_g(case, bf16):
    B, I, C = case
    dx, x, g = pc.merge_inputs(case, bf16)
    assert int((x == 0).sum()) > 0 and int((x < 0).sum()) > 0 and int((x > 0).sum()) > 0
    for relu in (0, 1):
        ref = pc.merge_ref(dx, x, g, relu)
        bar = pc.merge_bar(dx, g, ref, bf16)
        assert ref.dtype == torch.float64 and bar.dtype == torch.float64 and tuple(ref.shape) == (B, I, C)
        # the kernel's line in float32 without the fused multiply-add (one rounding more than the kernel makes)
        got = dx + g.unsqueeze(1) * torch.tensor(1.0 / I, dtype=torch.float32)
        if relu:
            got = torch.where(x > 0, got, torch.zeros_like(got))
        if bf16:
            got = pc.bf_round(got)
        err = (got.double() - ref).abs()
        print(f"merge {case} relu {relu} bf16 {bf16}: max err / bar {float((err / bar.clamp_min(1e-300)).max()):.3f}")
        assert bool((err <= bar).all())
        if relu:
            assert bool((ref[x <= 0] == 0).all())
        if B > 1:       # the broadcast row of the next batch entry is far outside the bar
            wrong = pc.merge_ref(dx, x, g.roll(1, 0), relu)
            assert bool(((wrong - ref).abs() > bar).any())


@pytest.mark.parametrize("case", pc.WEIGHT_CASES, ids=pc.geom_id)
def test_weight_references_pad_with_zero_and_tell_kh_from_kw(case):
    O, I, KH, KW, I_pad = case
    w = pc.weight_param(case)
    ohwi, ihwo = pc.relayout_ref(w, I_pad)
    assert ohwi.shape == (O, KH, KW, I_pad) and ihwo.shape == (I_pad, KH, KW, O)
    assert np.array_equal(ohwi, ihwo.transpose(3, 1, 2, 0))
    if I_pad > I:
        assert not ohwi[..., I:].any() and not ihwo[I:].any()
    for o, i, kh, kw in ((0, 0, 0, 0), (O - 1, I - 1, KH - 1, KW - 1), (O // 2, I // 2, KH // 2, KW // 2)):
        assert ohwi[o, kh, kw, i] == w[o, i, kh, kw] == ihwo[i, kh, kw, o]
    if KH != KW:
        # a kernel that swaps the kh and kw strides reads the parameter as [O][I][KW][KH].  Where one extent is 1 the taps are a line and
        # that is the identity — 1 x 3 and 3 x 1 hold the extents apart (a kh bounded by KW runs off the line) —; 2 x 5 shows the swap
        swapped = w.reshape(O, I, KW, KH).transpose(0, 3, 2, 1)
        assert np.array_equal(swapped, ohwi[..., :I]) == (min(KH, KW) == 1)
    assert any(min(c[2], c[3]) > 1 and c[2] != c[3] for c in pc.WEIGHT_CASES)
    for nsplit in pc.NSPLITS:
        ws = pc.slabs(case, nsplit)
        assert ws.shape == (nsplit, O, KH, KW, I_pad) and (I_pad == I or np.isnan(ws[..., I:]).all())
        ref, bar = pc.reduce_ref(ws, I)
        assert ref.dtype == np.float64 and ref.shape == (O, I, KH, KW) and np.isfinite(ref).all() and (bar > 0).all()
        acc = np.zeros((O, KH, KW, I), np.float32)
        for z in range(nsplit):                                  # a float32 sum in slab order stays inside the bar
            acc = acc + ws[z, ..., :I]
        err = np.abs(acc.transpose(0, 3, 1, 2).astype(np.float64) - ref)
        assert (err <= bar).all()
