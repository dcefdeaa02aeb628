"""wsmgmap.ops.bev — operator 1: RGB-D -> egocentric BEV index / scatter-max / rotation, global-map fuse and retrieve (rollout only,
no autograd).
"""
import ctypes

import torch

from .. import _abi
from ..debug import sw
from .core import _p, _raw_stream, _stream, _req, _f32, _sfx, _workspace, _rows_of, _conv_out, _launch, _zeros_f32, _prelaid, _join_side_at_end, TokenGradSink


# ----------------------------------------------------------------------------- BEV (no autograd: rollout only)
@torch.no_grad()
def bev_index(depth, Hf, Wf, E, depth_scale=10.0, local_scale=0.12):
    """depth [B,Hd,Wd] -> lin_idx int32 [B,Hf*Wf] (-1 = invalid source)."""
    _req(depth)
    _f32(depth)
    B, Hd, Wd = depth.shape
    lin = torch.empty(B, Hf * Wf, device=depth.device, dtype=torch.int32)
    _abi.call("wsmg_bev_index", _p(depth), B, Hd, Wd, float(depth_scale), Hf, Wf, E, float(local_scale), _p(lin), _stream())
    return lin


def bev_compact_ok(Hf, Wf, E, B=None):
    """Shapes the compacted-source route takes (source and cell ids are packed into 16 bits each).  Not below 4 frames: there the
    operator is four launches' latency (cfg1: 40 us), the scatter is not paced by its list, and the compaction adds 3 us to the index.
    Not both products at 65536 together: source 65535 on cell 65535 would pack to 0xffffffff, the list's "no entry" word."""
    fits = Hf * Wf <= 65536 and E * E <= 65536 and not (Hf * Wf == 65536 and E * E == 65536)
    return fits and sw.bev_compact and (B is None or B >= 4)


@torch.no_grad()
def bev_index_compact(depth, Hf, Wf, E, depth_scale=10.0, local_scale=0.12):
    """bev_index + the list of valid sources: -> (lin_idx int32 [B,Hf*Wf], (clist uint32-as-int32 [B,Hf*Wf], cnt int32 [B,nblk]))."""
    _req(depth)
    _f32(depth)
    B, Hd, Wd = depth.shape
    per = Hf * Wf
    lin = torch.empty(B, per, device=depth.device, dtype=torch.int32)
    clist = torch.empty(B, per, device=depth.device, dtype=torch.int32)
    cnt = torch.empty(B, (per + 8191) // 8192, device=depth.device, dtype=torch.int32)
    _abi.call("wsmg_bev_index_compact", _p(depth), B, Hd, Wd, float(depth_scale), Hf, Wf, E, float(local_scale), _p(lin), _p(clist), _p(cnt),
              _stream())
    return lin, (clist, cnt)


@torch.no_grad()
def bev_scatter_max(feat, lin, C, E):
    """feat [B,Cf,Hf,Wf] NCHW -> [B,C,E,E] NCHW planes."""
    _req(feat, lin)
    _f32(feat)
    B, Cf, Hf, Wf = feat.shape
    out = torch.empty(B, C, E, E, device=feat.device, dtype=torch.float32)
    _abi.call("wsmg_bev_scatter_max", _p(feat), _p(lin), B, Cf, Hf, Wf, C, E, _p(out), _stream())
    return out


@torch.no_grad()
def bev_rotate(planes, heading, sign):
    """planes [B,C,E,E] -> rotated NHWC [B,E,E,C]."""
    _req(planes, heading)
    B, C, E, _ = planes.shape
    out = torch.empty(B, E, E, C, device=planes.device, dtype=torch.float32)
    _abi.call("wsmg_bev_rotate", _p(planes), _p(heading), float(sign), B, C, E, _p(out), _stream())
    return out


@torch.no_grad()
def bev_scatter_rotate(feat, lin, heading, sign, C, E, compact=None):
    """bev_scatter_max + bev_rotate in one launch; the rotated map stays in NCHW planes [B,C,E,E] (for map_fuse(..., planes=True)).
    compact: bev_index_compact's (clist, cnt) — the scatter then walks the valid sources only (same planes bit for bit)."""
    _req(feat, lin, heading)
    _f32(feat, heading)
    B, Cf, Hf, Wf = feat.shape
    out = torch.empty(B, C, E, E, device=feat.device, dtype=torch.float32)
    if compact is not None:
        _abi.call("wsmg_bev_scatter_rotate_compact", _p(feat), _p(compact[0]), _p(compact[1]), _p(heading), float(sign), B, Cf, Hf, Wf, C, E,
                  _p(out), _stream())
        return out
    _abi.call("wsmg_bev_scatter_rotate", _p(feat), _p(lin), _p(heading), float(sign), B, Cf, Hf, Wf, C, E, _p(out), _stream())
    return out


def bev_planes_ok(C, E):
    """Shapes the one-launch scatter + rotation and the plane-consuming fuse take."""
    return C % 4 == 0 and C <= 64 and E > 1 and E * E * 4 <= 160 * 1024


@torch.no_grad()
def _check_global_map(global_map, B, C, *f32s):
    """The kernels index global_map[b] for b < B: the reference slices `full_global_map[:bs]` (rgb_mapping.py:43) and
    fails with a shape error when the batch has more rows than num_proc — here that would be an out-of-bounds access."""
    _f32(global_map, *f32s)
    if global_map.dim() != 4 or global_map.shape[1] != global_map.shape[2]:
        raise _abi.WsmgError(f"full_global_map must be [num_proc, G, G, C], got {tuple(global_map.shape)}")
    if global_map.shape[0] < B:
        raise _abi.WsmgError(f"batch of {B} rows but full_global_map holds {global_map.shape[0]} maps (num_proc): "
                             "construct the policy with RGBMAPPING.num_proc >= the rollout batch")
    if global_map.shape[3] != C:
        raise _abi.WsmgError(f"full_global_map has {global_map.shape[3]} channels, the ego map {C}")


def map_fuse(ego_rot, global_map, gps, masks, resolution=0.12, planes=False):
    """planes: ego_rot is [B,C,E,E] (bev_scatter_rotate's output) instead of NHWC [B,E,E,C]; same result bit for bit."""
    _req(ego_rot, global_map, gps, masks)
    if planes:
        B, C, E, _ = ego_rot.shape
    else:
        B, E, _, C = ego_rot.shape
    _check_global_map(global_map, B, C, ego_rot, gps, masks)
    if gps.shape[0] != B or masks.numel() != B:
        raise _abi.WsmgError("map_fuse: gps [B,2] and masks [B] must match the ego maps' batch")
    G = global_map.shape[1]
    _abi.call("wsmg_map_fuse_planes" if planes else "wsmg_map_fuse", _p(ego_rot), _p(global_map), _p(gps), _p(masks), B, C, E, G,
              float(resolution), _stream())


@torch.no_grad()
def map_retrieve(global_map, gps, compass, E, resolution=0.12, fused=None):
    """fused: crop + rotation in one launch, bit-identical to the two.  "tiled" (the default): the LDS-staged launch
    (wsmg_map_retrieve_tiled); True: the register form (16 gathers per item — 11 us at B = 1 but 311 vs 219 us at cfg4);
    False: crop and rotation as two launches through a scratch map."""
    _req(global_map, gps, compass)
    B = gps.shape[0]
    _check_global_map(global_map, B, global_map.shape[3] if global_map.dim() == 4 else -1, gps, compass)
    if compass.numel() != B:
        raise _abi.WsmgError("map_retrieve: compass [B] must match gps [B,2]")
    G, C = global_map.shape[1], global_map.shape[3]
    out = torch.empty(B, E, E, C, device=gps.device, dtype=torch.float32)
    if fused is None:
        fused = "tiled"
    if fused == "tiled":
        _abi.call("wsmg_map_retrieve_tiled", _p(global_map), _p(gps), _p(compass), B, C, E, G, float(resolution), _p(out), _stream())
        return out
    if fused:
        _abi.call("wsmg_map_retrieve_fused", _p(global_map), _p(gps), _p(compass), B, C, E, G, float(resolution), _p(out), _stream())
        return out
    scratch = torch.empty(B, E, E, C, device=gps.device, dtype=torch.float32)
    _abi.call("wsmg_map_retrieve", _p(global_map), _p(gps), _p(compass), B, C, E, G, float(resolution), _p(scratch), _p(out), _stream())
    return out


def bev_one_launch_routes(B, C, E, G):
    """(project, fuse_retrieve): which of the two one-launch forms Mapping.project_feat_to_map takes for a batch of B frames of a
    [C,E,E] ego map in a G x G global map.  debug.sw.bev_one_launch = 0 / 1 forces neither / both wherever the shapes allow; -1
    follows the interleaved A/B of profiles/bev_fuse_retrieve.txt: a form is the default only at a configuration where it was
    measured and its median was not slower than the launches it replaces.  bev_project is a small-batch form: from 4 frames on the
    compacted index route stays."""
    if not bev_planes_ok(C, E) or sw.bev_one_launch == 0:
        return False, False
    small = B < 4
    if sw.bev_one_launch > 0:
        return small, True
    return small and _PROJECT_DEFAULT, _fuse_retrieve_default(B, C, E, G)


# profiles/bev_fuse_retrieve.txt: bev_project is slower than index + scatter_rotate at every measured configuration (B = 1: every
# plane workgroup pays the index arithmetic of all sources), so no batch takes it by default; map_fuse_retrieve wins where the step is
# launch latency (B = 1 at E = 100, C = 64, G = 240: cfg1 and the native configuration) and loses once the tiles' recomputed paste
# is real work (B = 8 and cfg4).  Nothing else was measured — batches of 2 and 3, B = 1 at another geometry — and what was not
# measured keeps the two launches.
_PROJECT_DEFAULT = False
_FUSE_RETRIEVE_MEASURED_FASTER = {(1, 64, 100, 240)}          # (B, C, E, G)


def _fuse_retrieve_default(B, C, E, G):
    return (B, C, E, G) in _FUSE_RETRIEVE_MEASURED_FASTER


@torch.no_grad()
def map_fuse_retrieve(ego_rot_planes, global_map, gps, compass, masks, E, resolution=0.12):
    """map_fuse(planes=True) + map_retrieve (the tiled form) in ONE launch (wsmg_map_fuse_retrieve): global_map [P,G,G,C] is updated
    in place, -> ego map NHWC [B,E,E,C]; both bit for bit what the two calls leave, for masks in {0, 1} and finite features (finite
    ego_rot_planes).  Outside that contract — a mask that is neither 0 nor 1, an infinite plane value on a reset step — the result
    depends on the order in which workgroups run and is not repeatable; the two calls are.  ego_rot_planes [B,C,E,E] is
    bev_scatter_rotate's / bev_project's output."""
    if ego_rot_planes.dim() != 4 or ego_rot_planes.shape[2] != E or ego_rot_planes.shape[3] != E:
        raise _abi.WsmgError(f"map_fuse_retrieve: rotated planes [B,C,{E},{E}] expected, got {tuple(ego_rot_planes.shape)}")
    B, C = ego_rot_planes.shape[:2]
    _check_global_map(global_map, B, C, ego_rot_planes, gps, compass, masks)
    if gps.shape[0] != B or masks.numel() != B or compass.numel() != B:
        raise _abi.WsmgError("map_fuse_retrieve: gps [B,2], compass [B] and masks [B] must match the ego maps' batch")
    if not bev_planes_ok(C, E):
        raise _abi.WsmgError(f"map_fuse_retrieve: needs C % 4 == 0, C <= 64 and E * E * 4 <= 160 KiB (bev_planes_ok), got C = {C}, E = {E}")
    G = global_map.shape[1]
    if G < E:
        raise _abi.WsmgError(f"map_fuse_retrieve: the global map ({G}) is smaller than the ego map ({E})")
    _req(ego_rot_planes, global_map, gps, compass, masks)
    out = torch.empty(B, E, E, C, device=gps.device, dtype=torch.float32)
    _abi.call("wsmg_map_fuse_retrieve", _p(ego_rot_planes), _p(global_map), _p(gps), _p(compass), _p(masks), B, C, E, G, float(resolution),
              _p(out), _stream())
    return out


@torch.no_grad()
def bev_project(depth, feat, heading, sign, C, E, depth_scale=10.0, local_scale=0.12, want_index=True):
    """bev_index + bev_scatter_rotate in ONE launch (wsmg_bev_project; meant for batches below 4): depth [B,Hd,Wd], feat
    [B,Cf,Hf,Wf] NCHW, heading [B] -> (rotated planes [B,C,E,E], lin_idx int32 [B,Hf*Wf] or None without want_index), both bit for
    bit what the two calls give."""
    _f32(depth, feat, heading)
    if depth.dim() != 3 or feat.dim() != 4:
        raise _abi.WsmgError(f"bev_project: depth [B,Hd,Wd] and feat [B,Cf,Hf,Wf] expected, got {tuple(depth.shape)}, {tuple(feat.shape)}")
    B, Hd, Wd = depth.shape
    _, Cf, Hf, Wf = feat.shape
    if feat.shape[0] != B or heading.numel() != B:
        raise _abi.WsmgError("bev_project: depth, feat and heading must have the same batch")
    if not bev_planes_ok(C, E):
        raise _abi.WsmgError(f"bev_project: needs C % 4 == 0, C <= 64 and E * E * 4 <= 160 KiB (bev_planes_ok), got C = {C}, E = {E}")
    if C > Cf or Hf > Hd or Wf > Wd:
        raise _abi.WsmgError(f"bev_project: C <= Cf and a feature map no larger than the depth image expected, got C = {C}, feat {tuple(feat.shape)}, depth {tuple(depth.shape)}")
    _req(depth, feat, heading)
    lin = torch.empty(B, Hf * Wf, device=depth.device, dtype=torch.int32) if want_index else None
    out = torch.empty(B, C, E, E, device=feat.device, dtype=torch.float32)
    _abi.call("wsmg_bev_project", _p(depth), _p(feat), _p(heading), float(sign), B, Hd, Wd, float(depth_scale), Cf, Hf, Wf, C, E,
              float(local_scale), _p(lin) if want_index else None, _p(out), _stream())
    return out, lin


def ego_channels_last_dims(ego):
    """(B, H, W, C) of an ego map that is channels-last in memory: `observations['rgb_ego_map']` as the mapping module leaves it
    ([B,C,H,W]: map_retrieve's NHWC tensor, permuted) or a plain contiguous NHWC tensor [B,H,W,C]; anything else raises."""
    if not torch.is_tensor(ego) or not ego.is_cuda:
        raise _abi.WsmgError("wsmgmap operators need GPU tensors: the HIP path is the only path (no CPU fallback)")
    if ego.dim() != 4:
        raise _abi.WsmgError(f"ego map: [B,C,H,W] over channels-last memory or NHWC [B,H,W,C] expected, got {tuple(ego.shape)}")
    if ego.shape[1] == 64 and ego.permute(0, 2, 3, 1).is_contiguous():
        B, C, H, W = ego.shape
    elif ego.is_contiguous():
        B, H, W, C = ego.shape
    else:
        raise _abi.WsmgError(f"ego map: must be channels-last in memory, got shape {tuple(ego.shape)} strides {ego.stride()}")
    return int(B), int(H), int(W), int(C)


@torch.no_grad()
def ego_sparse_pack(ego):
    """One rollout step of the ego map -> the sparse record form of wsmgmap/data/codec.py, packed on the device:
    (bits uint8 [B,H*W,8], off uint32 [B,H*W], nnz int64 [B], vals float16 [B,H*W*64]); row b's values are vals[b, :nnz[b]],
    the rest of its region is not written.  ego: float32, channels-last in memory (`ego_channels_last_dims`).  Bit for bit what
    codec.sparse_pack_ego makes of the float16 map, row by row.  The format is defined for 64 channels only."""
    B, H, W, C = ego_channels_last_dims(ego)
    _f32(ego)
    HW = H * W
    if C != 64:
        raise _abi.WsmgError(f"ego_sparse_pack: the sparse ego map is defined for 64 channels, got {C} (other maps are stored dense)")
    if B <= 0 or HW <= 0:
        raise _abi.WsmgError(f"ego_sparse_pack: empty map {tuple(ego.shape)}")
    bits = torch.empty(B, HW, 8, device=ego.device, dtype=torch.uint8)
    off = torch.empty(B, HW, device=ego.device, dtype=torch.uint32)
    nnz = torch.empty(B, device=ego.device, dtype=torch.int64)
    vals = torch.empty(B, HW * 64, device=ego.device, dtype=torch.float16)
    _abi.call("wsmg_ego_sparse_pack", _p(ego), B, C, HW, _p(bits), _p(off), _p(nnz), _p(vals), _stream())
    return bits, off, nnz, vals
