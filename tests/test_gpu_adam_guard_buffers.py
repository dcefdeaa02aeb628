"""GPU: a skipped guarded Adam step also rolls back the BatchNorm running statistics its forward pass wrote
(csrc/wsmg_small.hip: copy_multi_guarded_kernel behind wsmg_copy_multi_guarded; wsmgmap.optim.Adam(skip_nonfinite=True,
guard_buffers=module): snapshot in zero_grad(), conditional restore in step()).

Everything here is compared BITWISE: the kernel copies bytes (against numpy), and a rolled-back policy must be the policy that never
saw the poisoned batch — the same launches on the same values, so there is no tolerance to choose.  NaN and Inf are ordinary
floating-point data; nothing here faults."""
import copy
import ctypes
import functools

import numpy as np
import pytest
import torch

from adam_util import _bits, _ptr, _stream
from oracle import cases
from util import T, state_dict_values

pytestmark = pytest.mark.gpu

LR = 2.5e-4


def _same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(_bits(a), _bits(b))


def _bn_buffers(module):
    """{name: tensor}: running_mean, running_var, num_batches_tracked of every BatchNorm layer below module."""
    out = {}
    for mname, m in module.named_modules():
        if isinstance(m, torch.nn.modules.batchnorm._BatchNorm) and m.track_running_stats:
            for b in ("running_mean", "running_var", "num_batches_tracked"):
                out[f"{mname}.{b}"] = getattr(m, b)
    return out


def _record(tensors):
    return {k: _bits(v).clone() for k, v in tensors.items()}


def _unchanged(tensors, rec):
    return [k for k, v in tensors.items() if not torch.equal(_bits(v), rec[k])]


# ----------------------------------------------------------------------------- 1. the kernel against numpy
SIZES = [1, 3, 15, 16, 17, 4096, 4096 + 5]
OFFS = [0, 1, 4, 8]                    # bytes past a 16-byte boundary: every (dst, src) pairing, aligned and not
PAD = 64                               # guard bytes on both sides of every destination (and source)
BIG = 2 * 16384 + 5                    # more than one 16 KB workgroup of one copy, dst and src sharing a misalignment of 1
NAN_WORDS = np.array([0x7fc00001, 0xffffffff, 0x7f800001, 0xffc12345], np.uint32)   # quiet / signalling NaNs with payloads


@functools.lru_cache(maxsize=None)
def _arena():
    """(rows, src bytes, dst bytes): rows = [(dst offset, src offset, bytes)] into two byte arenas, one slot per descriptor —
    PAD guard bytes, the misalignment, the payload, PAD guard bytes, slots on 16-byte boundaries.  Random bytes (seeded), NaN bit
    patterns at the head of every source of 16 bytes or more.  Computed once, never written."""
    rng = np.random.default_rng(20261018)
    shapes = [(n, do, so) for n in SIZES for do in OFFS for so in OFFS] + [(BIG, 1, 1)]
    rows, at = [], 0
    for n, do, so in shapes:
        rows.append((at + PAD + do, at + PAD + so, n))
        at += (PAD + 16 + n + PAD + 15) // 16 * 16
    src = rng.integers(0, 256, at, dtype=np.uint8)
    dst = rng.integers(0, 256, at, dtype=np.uint8)
    for _, so, n in rows:
        if n >= 16:
            src[so:so + 16] = NAN_WORDS.view(np.uint8)
    src.setflags(write=False)
    dst.setflags(write=False)
    return rows, src, dst


@pytest.mark.parametrize("flag", [0.0, 1.0], ids=["taken", "skipped"])
def test_guarded_copy_matches_numpy_bitwise(flag):
    """Lists of 1, 48 (one launch's table), 49 and all 113 + 1 descriptors (three launches; the last one an int64 tensor):
    with guard[2] = 0 not one byte of the destination arena changes; with guard[2] = 1 every destination equals its source and
    every other byte of the arena — the 64 guard bytes around each destination among them — is unchanged.  The guard record and
    the floats around it are only read."""
    from wsmgmap import _abi
    from wsmgmap.optim import ADAM_MAX
    rows, src_np, dst_np = _arena()
    assert ADAM_MAX == 48 and len(rows) > 2 * ADAM_MAX
    src = torch.from_numpy(src_np.copy()).cuda()
    pristine = torch.from_numpy(dst_np.copy()).cuda()
    dst = torch.empty_like(pristine)
    assert src.data_ptr() % 16 == 0 and dst.data_ptr() % 16 == 0
    i64_src = torch.tensor([2 ** 62 + 1, -7, 2 ** 53 + 1, 0, -2 ** 63], dtype=torch.int64, device="cuda")
    i64_dst = torch.empty_like(i64_src)
    record = torch.tensor([-7.0, -7.0, -7.0, -7.0, 1.25, float("nan"), flag, 3.0, -7.0, -7.0, -7.0, -7.0], device="cuda")
    record_before = _bits(record).clone()
    guard = _ptr(record[4:])
    descs = (_abi.CopyDesc * (len(rows) + 1))()
    for d, (do, so, n) in zip(descs, rows):
        d.dst, d.src, d.bytes = dst.data_ptr() + do, src.data_ptr() + so, n
    descs[len(rows)].dst, descs[len(rows)].src, descs[len(rows)].bytes = i64_dst.data_ptr(), i64_src.data_ptr(), 40
    for count in (1, ADAM_MAX, ADAM_MAX + 1, len(rows) + 1):
        dst.copy_(pristine)
        i64_dst.fill_(11)
        _abi.call("wsmg_copy_multi_guarded", ctypes.cast(descs, ctypes.c_void_p), count, guard, _stream())
        torch.cuda.synchronize()
        want = dst_np.copy()
        if flag:
            for do, so, n in rows[:count]:
                want[do:do + n] = src_np[so:so + n]
        got = dst.cpu().numpy()
        bad = np.flatnonzero(got != want)
        assert bad.size == 0, f"{count} descriptors, guard[2] = {flag}: {bad.size} bytes differ, first at arena offset {int(bad[0])}"
        if flag and count > len(rows):
            assert torch.equal(i64_dst, i64_src)
        else:
            assert bool((i64_dst == 11).all())
        assert torch.equal(_bits(record), record_before), "the guard record was written"
    assert np.array_equal(src.cpu().numpy(), src_np)


# ----------------------------------------------------------------------------- the policy of test_gpu_adam_guard.py's update test
class _Box:
    shape = (2,)


@functools.lru_cache(maxsize=None)
def _base():
    """(policy, inputs): the T = 4 x N = 2 float32 policy on the device, NEVER run — every test works on deep copies — and its
    update batch."""
    from wsmgmap.config import default_model_config
    from wsmgmap.models.policy import BasePolicy
    obs_np, prev, masks, weights = cases.update_inputs(4, 2, n_tok=(80, 37), tag="adam")
    policy = BasePolicy(None, _Box(), default_model_config(num_proc=2, compute_dtype="f32"))
    policy.load_state_dict(state_dict_values(), strict=True)
    policy.net.instruction_encoder.embedding_layer.weight.requires_grad_(False)
    policy = policy.cuda()
    policy.train(); policy.net.depth_encoder.eval(); policy.net.rgb_encoder.eval()
    obs = {k: T(v).cuda() for k, v in obs_np.items()}
    return policy, (obs, T(prev).cuda(), T(masks).cuda(), T(weights).cuda())


def _policy_and_adam(**kw):
    from wsmgmap import optim
    policy = copy.deepcopy(_base()[0])
    if kw.pop("protect", False):
        kw["guard_buffers"] = policy
    return policy, optim.Adam(policy.parameters(), lr=LR, skip_nonfinite=True, **kw)


def _update(policy, opt, obs=None):
    """One update as the reference's _update_agent orders it: zero_grad, forward, loss, backward, step -> (logits, loss)."""
    from wsmgmap.common.aux_losses import AuxLosses
    base_obs, prev, masks, weights = _base()[1]
    opt.zero_grad()
    AuxLosses.activate(); AuxLosses.clear()
    pred, aux = policy(dict(base_obs if obs is None else obs), torch.zeros(2, 2, 512, device="cuda"), prev, masks, weights)
    loss = (pred ** 2).mean() + aux
    loss.backward()
    AuxLosses.deactivate()
    opt.step()
    return pred.detach().clone(), loss.detach().clone()


def _poisoned_obs():
    obs = dict(_base()[1][0])
    ego = obs["rgb_ego_map"].clone()
    ego[3, 5, 40, 41] = float("nan")            # one element of one row of the T x N batch
    obs["rgb_ego_map"] = ego
    return obs


def _moments(policy, opt):
    out = {}
    for name, p in policy.named_parameters():
        st = opt.state.get(p, {})
        for k in ("exp_avg", "exp_avg_sq"):
            if k in st:
                out[f"{name}.{k}"] = st[k]
    return out


# ----------------------------------------------------------------------------- 2. end to end (fails without the feature)
def test_poisoned_update_leaves_the_policy_as_it_was():
    """A NaN in one row of rgb_ego_map reaches the map stack's BatchNorm statistics in the forward pass and every gradient in the
    backward.  With guard_buffers the skipped update leaves every BatchNorm buffer (num_batches_tracked included), parameter and
    moment bit-equal to what it was; without it (the control) running means are non-finite.  The next clean update is then, bit
    for bit, the first clean update of a copy that never saw the poisoned batch."""
    policy, opt = _policy_and_adam(protect=True)
    bufs, params = _bn_buffers(policy), dict(policy.named_parameters())
    assert len(bufs) == 3 * 63 and not any(k.endswith("_scale") for k in bufs)
    buf_rec, par_rec = _record(bufs), _record(params)
    state_rec = _record({k: v for k, v in policy.state_dict().items() if k not in bufs and k not in params})
    _update(policy, opt, _poisoned_obs())
    torch.cuda.synchronize()
    assert opt.skipped_steps == 1 and not np.isfinite(float(opt.grad_norm))
    assert _unchanged(bufs, buf_rec) == [], "a skipped update left BatchNorm statistics changed"
    assert _unchanged(params, par_rec) == [], "a skipped update wrote a parameter"
    moments = _moments(policy, opt)
    assert len(moments) > 2 * 96 and all(not bool(m.view(torch.int32).any()) for m in moments.values()), "a moment was written"
    assert _unchanged({k: v for k, v in policy.state_dict().items() if k in state_rec}, state_rec) == []   # (_scale: never touched)

    control, copt = _policy_and_adam()
    _update(control, copt, _poisoned_obs())
    torch.cuda.synchronize()
    cbufs = _bn_buffers(control)
    poisoned = [k for k, v in cbufs.items() if k.endswith("running_mean") and not bool(torch.isfinite(v).all())]
    print(f"control: {len(poisoned)} non-finite running means, e.g. {poisoned[:3]}")
    assert copt.skipped_steps == 1 and poisoned, "the poison did not reach the statistics: the test shows nothing"
    assert any(not torch.equal(_bits(v), buf_rec[k]) for k, v in cbufs.items() if k.endswith("num_batches_tracked"))

    fresh, fopt = _policy_and_adam(protect=True)
    got = _update(policy, opt)
    want = _update(fresh, fopt)
    torch.cuda.synchronize()
    assert opt.skipped_steps == 1 and fopt.skipped_steps == 0
    assert _same(got[0], want[0]), "logits differ from the policy that never saw the poisoned batch"
    assert _same(got[1], want[1]) and np.isfinite(float(got[1])), "loss differs"
    fparams, fbufs = dict(fresh.named_parameters()), _bn_buffers(fresh)
    assert [k for k in params if not _same(params[k], fparams[k])] == []
    assert [k for k in bufs if not _same(bufs[k], fbufs[k])] == []
    assert any(not torch.equal(_bits(v), par_rec[k]) for k, v in params.items()), "the clean update did not step"
    assert {float(st["step"]) for st in opt.state_dict()["state"].values()} == {1.0}       # attempted 2, skipped 1


# ----------------------------------------------------------------------------- 3. a clean step is not disturbed
def test_clean_update_is_the_same_with_and_without_guard_buffers():
    a, aopt = _policy_and_adam(protect=True)
    b, bopt = _policy_and_adam()
    before = _record(_bn_buffers(a))
    la, lb = _update(a, aopt), _update(b, bopt)
    torch.cuda.synchronize()
    assert aopt.skipped_steps == 0 == bopt.skipped_steps
    assert _same(la[0], lb[0]) and _same(la[1], lb[1])
    pa, pb = dict(a.named_parameters()), dict(b.named_parameters())
    assert [k for k in pa if not _same(pa[k], pb[k])] == []
    ba, bb = _bn_buffers(a), _bn_buffers(b)
    assert [k for k in ba if not _same(ba[k], bb[k])] == []
    ma, mb = _moments(a, aopt), _moments(b, bopt)
    assert ma.keys() == mb.keys() and [k for k in ma if not _same(ma[k], mb[k])] == []
    train = [k for k in ba if k.endswith("num_batches_tracked") and ".rgb_encoder." not in k and ".depth_encoder." not in k]
    stepped = [k for k in train if int(ba[k]) == int(before[k]) + 1]
    frozen = [k for k in ba if k.endswith("num_batches_tracked") and k not in train]
    print(f"{len(stepped)} of {len(train)} train-mode counters advanced by one, {len(frozen)} frozen")
    assert "net.map_encoder.cnn.1.num_batches_tracked" in stepped and "net.map_classfier.1.num_batches_tracked" in stepped
    assert all(int(ba[k]) in (int(before[k]), int(before[k]) + 1) for k in train)
    assert all(int(ba[k]) == int(before[k]) for k in frozen)
    assert any(not torch.equal(_bits(ba[k]), before[k]) for k in ba if k.endswith("running_mean"))


# ----------------------------------------------------------------------------- 4. inside a HIP graph
def _small(seed=0):
    torch.manual_seed(seed)
    return torch.nn.Sequential(torch.nn.Linear(8, 8), torch.nn.BatchNorm1d(8)).cuda().train()


def _small_update(m, opt, x):
    opt.zero_grad(set_to_none=True)
    m(x).pow(2).mean().backward()
    opt.step()


def _small_state(m):
    return {**dict(m.named_parameters()), **dict(m.named_buffers())}


def test_snapshot_and_roll_back_replay_in_a_graph():
    """zero_grad (the snapshot), stock torch forward and backward, and the guarded step (norm, finalize, Adam, conditional restore)
    captured once on a side stream after one eager update; replayed with a clean input, one holding an Inf, and a clean one."""
    from wsmgmap import _abi, optim
    m = _small()
    twin, lazy_m = copy.deepcopy(m), copy.deepcopy(m)
    opt = optim.Adam(m.parameters(), lr=1e-2, skip_nonfinite=True, guard_buffers=m)
    topt = optim.Adam(twin.parameters(), lr=1e-2, skip_nonfinite=True, guard_buffers=twin)
    lazy = optim.Adam(lazy_m.parameters(), lr=1e-2, skip_nonfinite=True, guard_buffers=lazy_m)
    g = torch.Generator().manual_seed(1)
    xs = [torch.randn(4, 8, generator=g).cuda() for _ in range(3)]
    bad = xs[1].clone()
    bad[2, 3] = float("inf")
    x = xs[0].clone()                          # the graph's static input
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        _small_update(m, opt, x)               # eager: moments, snapshot storage and first launches exist before the capture
        _small_update(twin, topt, x)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    assert [k for k, v in _small_state(m).items() if not _same(v, _small_state(twin)[k])] == []
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        with pytest.raises(_abi.WsmgError):    # the snapshot's allocation is never made under capture
            lazy.zero_grad()
        _small_update(m, opt, x)
    opt.note_replayed_steps(-1)                # the capture ran the host bookkeeping once and executed nothing
    torch.cuda.synchronize()
    after = []
    for k, inp in enumerate((xs[1], bad, xs[2])):
        x.copy_(inp)
        graph.replay()
        opt.note_replayed_steps(1)
        torch.cuda.synchronize()
        after.append(_record(_small_state(m)))
        assert opt.skipped_steps == (0 if k == 0 else 1)
    state = _small_state(m)
    assert [k for k in state if not torch.equal(after[1][k], after[0][k])] == [], "the skipped replay changed the module"
    assert int(state["1.num_batches_tracked"]) == 3
    with torch.cuda.stream(side):
        _small_update(twin, topt, xs[1])
        _small_update(twin, topt, xs[2])
    torch.cuda.synchronize()
    tstate = _small_state(twin)
    assert [k for k in state if not _same(state[k], tstate[k])] == [], "replays differ from two clean eager updates"
    assert float(opt._guard_step) == 3.0 == float(topt._guard_step) and topt.skipped_steps == 0
    assert bool(torch.isfinite(state["1.running_mean"]).all()) and bool(torch.isfinite(state["1.running_var"]).all())


# ----------------------------------------------------------------------------- 5. a stale snapshot is refused
def test_step_without_a_fresh_snapshot_raises_and_writes_nothing():
    from wsmgmap import _abi, optim
    m = _small(seed=3)
    opt = optim.Adam(m.parameters(), lr=1e-2, skip_nonfinite=True, guard_buffers=m)
    g = torch.Generator().manual_seed(4)
    x = torch.randn(4, 8, generator=g).cuda()
    with pytest.raises(_abi.WsmgError):        # never snapshotted at all
        m(x).pow(2).mean().backward()
        opt.step()
    assert opt.state_dict()["state"] == {}
    _small_update(m, opt, x)
    for p in m.parameters():                   # gradients zeroed some other way: no snapshot
        p.grad = None
    m(x).pow(2).mean().backward()
    torch.cuda.synchronize()
    rec, skipped, count = _record(_small_state(m)), opt.skipped_steps, float(opt._guard_step)
    guard_rec = _bits(opt._guard).clone()
    with pytest.raises(_abi.WsmgError, match="snapshot"):
        opt.step()
    torch.cuda.synchronize()
    assert _unchanged(_small_state(m), rec) == []
    assert opt.skipped_steps == skipped == 0 and float(opt._guard_step) == count == 1.0
    assert torch.equal(_bits(opt._guard), guard_rec)
    assert {float(st["step"]) for st in opt.state_dict()["state"].values()} == {1.0}
    opt.snapshot_buffers()                     # the explicit form; the statistics of the forward above are then kept
    opt.step()
    torch.cuda.synchronize()
    assert float(opt._guard_step) == 2.0 and _unchanged(dict(m.named_parameters()), rec) != []
    assert int(m[1].num_batches_tracked) == 3
