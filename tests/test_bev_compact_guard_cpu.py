"""The compacted-source route of the BEV scatter (csrc/wsmg_bev.hip, bev_index_compact_kernel) packs (source << 16) | cell and keeps
0xffffffff for "no entry": source 65535 on cell 65535 would be that word.  The shape where both ids reach 65535 (Hf * Wf == 65536
together with E * E == 65536) is refused — by the route's predicate and by the entry points, before anything is enqueued (no GPU
needed: the argument check precedes every launch); either product alone at the limit is still taken (cfg4 has Hf * Wf == 65536)."""
import ctypes

EINVAL = -1


def test_compact_predicate_refuses_both_ids_at_the_limit():
    from wsmgmap import ops
    from wsmgmap.debug import sw
    assert sw.bev_compact
    assert not ops.bev_compact_ok(256, 256, 256)
    assert not ops.bev_compact_ok(256, 256, 256, 8)
    assert ops.bev_compact_ok(256, 256, 200) and ops.bev_compact_ok(256, 256, 200, 4)      # cfg4: sources alone at the limit
    assert ops.bev_compact_ok(224, 224, 256) and ops.bev_compact_ok(255, 256, 256)          # cells alone at the limit
    assert not ops.bev_compact_ok(256, 257, 200) and not ops.bev_compact_ok(224, 224, 257)  # beyond 16 bits, as before


def test_compact_entry_points_refuse_both_ids_at_the_limit_before_enqueuing():
    from wsmgmap import _abi
    L = _abi.lib()
    buf = (ctypes.c_uint64 * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    # wsmg_bev_index_compact(depth, B, Hd, Wd, depth_scale, Hf, Wf, E, local_scale, lin, clist, cnt, stream)
    assert L.wsmg_bev_index_compact(p, 4, 256, 256, 10.0, 256, 256, 256, 0.12, p, p, p, None) == EINVAL
    assert L.wsmg_bev_index_compact(p, 4, 512, 512, 10.0, 512, 128, 256, 0.12, p, p, p, None) == EINVAL
    # wsmg_bev_scatter_rotate_compact(feat, clist, cnt, heading, sign, B, Cf, Hf, Wf, C, E, out, stream)
    assert L.wsmg_bev_scatter_rotate_compact(p, p, p, p, -1.0, 4, 8, 256, 256, 8, 256, p, None) == EINVAL
    assert L.wsmg_bev_scatter_rotate_compact(p, p, p, p, -1.0, 4, 8, 128, 512, 8, 256, p, None) == EINVAL
    # the refusals that were there before stay: an id beyond 16 bits, a missing list
    assert L.wsmg_bev_index_compact(p, 4, 512, 512, 10.0, 257, 256, 200, 0.12, p, p, p, None) == EINVAL
    assert L.wsmg_bev_index_compact(p, 4, 256, 256, 10.0, 64, 64, 257, 0.12, p, p, p, None) == EINVAL
    assert L.wsmg_bev_scatter_rotate_compact(p, None, p, p, -1.0, 4, 8, 256, 256, 8, 200, p, None) == EINVAL
