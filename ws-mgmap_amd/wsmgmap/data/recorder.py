"""The write side of the sparse ego map: rollout steps packed on the device, kept per running episode on the host.

A DAgger rollout stores every step's observations until the episode ends and then writes one record (dagger_trainer.py:301-343).  The
ego map is 89 % of those bytes, and it is already on the GPU in the layout the sparse form of `codec.py` is defined in.
`SparseEgoRecorder.append` packs a step there (`ops.ego_sparse_pack`: presence bits, per-pixel offsets, the non-zero float16 values)
and brings to the host exactly what the record will hold; `take` hands back the five `rgb_ego_map__*` arrays of an episode — or of a
subsample of its steps — for `codec.pack_record_raw`.  They are, bit for bit, what `codec.sparse_pack_ego` returns for the dense
float16 map of those steps, so the feeder reads such records like recoded ones (tools/recode_cache.py --sparse-ego).

Steps are stored independently of each other: selecting some of them is a host concatenation plus a cumulative sum (`select_steps`).
"""
import numpy as np
import torch

from .. import _abi
from .codec import SPARSE_EGO


def select_steps(pieces, steps, shape):
    """The five sparse arrays of the steps `steps` (indices into `pieces`, in that order) of one episode.  pieces[t] = (bits uint8
    [H*W, C/8], off uint32 [H*W], vals float16 [nnz_t]) of step t, as `codec.sparse_pack_ego` makes them of a one-step map; shape =
    (C, H, W).  Equal to `sparse_pack_ego(dense[steps])`: bits and off are per step already, `__base` is the running sum of the
    selected steps' counts."""
    C, H, W = (int(x) for x in shape)
    steps = [int(t) for t in steps]
    T, HW = len(steps), H * W
    bits = np.empty((T, HW, C // 8), dtype=np.uint8)
    off = np.empty((T, HW), dtype=np.uint32)
    base = np.zeros(T + 1, dtype=np.int64)
    vals = []
    for j, t in enumerate(steps):
        b, o, v = pieces[t]
        bits[j] = np.asarray(b).reshape(HW, C // 8)
        off[j] = np.asarray(o).reshape(HW)
        base[j + 1] = base[j] + v.size
        vals.append(np.asarray(v, dtype=np.float16).reshape(-1))
    vals = np.concatenate(vals) if vals else np.empty(0, dtype=np.float16)
    return {SPARSE_EGO + "__bits": bits, SPARSE_EGO + "__off": off, SPARSE_EGO + "__base": base,
            SPARSE_EGO + "__vals": np.ascontiguousarray(vals), SPARSE_EGO + "__shape": np.array([C, H, W], dtype=np.int64)}


class SparseEgoRecorder:
    """Packed ego-map steps of `num_envs` running episodes.

        rec = SparseEgoRecorder(envs.num_envs, device)
        rec.append(observations["rgb_ego_map"])            # after policy.act / update_map, once per rollout step
        ...
        arrays = rec.take(i, range(24, rec.steps(i), step_num))     # episode i has ended
        blob = codec.pack_record_raw({**other_obs, **arrays}, prev_actions, oracle_actions)
        rec.reset(i)
    """

    def __init__(self, num_envs, device="cuda"):
        self.num_envs = int(num_envs)
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise _abi.WsmgError("SparseEgoRecorder packs on the GPU: the HIP path is the only path (codec.sparse_pack_ego is the host form)")
        self.shape = None                       # (C, H, W), fixed by the first step
        self._steps = [[] for _ in range(self.num_envs)]
        self._pinned = None
        self.bytes_to_host = 0                  # device-to-host bytes so far (counters, bits, offsets, values)

    def _staging(self, nbytes):
        if self._pinned is None or self._pinned.numel() < nbytes:
            self._pinned = torch.empty(int(nbytes * 1.25) + 4096, dtype=torch.uint8).pin_memory()
        return self._pinned

    def __len__(self):
        """Stored steps over all environments."""
        return sum(len(s) for s in self._steps)

    def steps(self, i):
        return len(self._steps[i])

    def reset(self, i):
        """Drop environment i's steps (its episode was written, or abandoned)."""
        self._steps[i] = []

    @torch.no_grad()
    def append(self, ego, rows=None):
        """Pack one step.  ego: the step's `rgb_ego_map` on the device (see `ops.ego_sparse_pack`); rows: the environment of each of
        its rows (default: row b is environment b, all of them present).  Synchronises the current stream twice: once to read the B
        counters, once for the copies, which carry each row's bits, offsets and exactly nnz values through pinned staging."""
        from ..ops import ego_channels_last_dims, ego_sparse_pack
        _, H, W, C = ego_channels_last_dims(ego)
        bits, off, nnz, vals = ego_sparse_pack(ego)
        B, HW = off.shape
        rows = list(range(B)) if rows is None else [int(r) for r in rows]
        if len(rows) != B or len(set(rows)) != B or min(rows) < 0 or max(rows) >= self.num_envs:
            raise _abi.WsmgError(f"SparseEgoRecorder.append: {B} map rows for environments {rows} of {self.num_envs}")
        shape = (C, H, W)
        if self.shape is None:
            self.shape = shape
        elif shape != self.shape:
            raise _abi.WsmgError(f"SparseEgoRecorder.append: map of shape {shape} after steps of shape {self.shape}")
        stream = torch.cuda.current_stream(self.device)
        # staging layout: counters | bits | offsets | values of row 0, row 1, ... (capacity for a fully dense step is not needed: the
        # values' size is known once the counters are here)
        head = 8 * B
        stage = self._staging(head + B * HW * 12)
        n_host = stage[:head].view(torch.int64)
        n_host.copy_(nnz, non_blocking=True)
        stream.synchronize()
        counts = n_host.tolist()
        total = head + B * HW * 12 + 2 * sum(counts)
        if stage.numel() < total:
            stage = self._staging(total)
        b_host = stage[head:head + B * HW * 8].view(B, HW, 8)
        o_host = stage[head + B * HW * 8:head + B * HW * 12].view(torch.uint32).view(B, HW)
        b_host.copy_(bits, non_blocking=True)
        o_host.copy_(off, non_blocking=True)
        at, v_host = head + B * HW * 12, []
        for b, n in enumerate(counts):
            v = stage[at:at + 2 * n].view(torch.float16)
            if n:
                v.copy_(vals[b, :n], non_blocking=True)
            v_host.append(v)
            at += 2 * n
        stream.synchronize()
        self.bytes_to_host += total
        b_np, o_np = b_host.numpy(), o_host.numpy()
        for b, env in enumerate(rows):          # the staging is reused by the next step: every piece is copied out of it
            self._steps[env].append((b_np[b].copy(), o_np[b].copy(), v_host[b].numpy().copy()))

    def take(self, i, steps=None):
        """The `rgb_ego_map__bits / __off / __base / __vals / __shape` arrays of environment i's stored steps, or of the steps
        `steps` of them (an index list, as the trainer's `range(24, len(ep), step_num)`), for `codec.pack_record_raw`."""
        if self.shape is None:
            raise _abi.WsmgError("SparseEgoRecorder.take before the first append: the map's shape is not known yet")
        n = len(self._steps[i])
        return select_steps(self._steps[i], range(n) if steps is None else steps, self.shape)
