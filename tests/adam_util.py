"""Shared helpers of the GPU tests of the Adam step and its guard (tests/test_gpu_adam_guard.py, test_gpu_adam_hyper.py,
test_gpu_adam_grad_report.py, test_gpu_adam_guard_buffers.py).

The tensor set: sizes around the 4-element vector and the 4 096-element workgroup, once 16-byte aligned and once as views one float
off, then ragged small sizes up to 50 tensors (the table of 48 spills into a second launch); values from oracle.detfill under a tag
of the test file's, so each file keeps its own numbers."""
import ctypes
import functools

import numpy as np
import torch

from oracle import detfill as df
from util import T

SIZES = [1, 3, 4, 4095, 4096, 4097, 8193]
ALL_SIZES = SIZES + SIZES + [5 + 7 * i for i in range(50 - 2 * len(SIZES))]
CHUNK = 4096
TOTAL_BLOCKS = sum((n + CHUNK - 1) // CHUNK for n in ALL_SIZES)


def _fill(name, off, n):
    """(offset in floats from a 16-byte boundary, (p, g, m, v)) of one tensor — read-only arrays."""
    vals = [df.uniform(f"{name}.{what}", (n,), sc) for what, sc in (("p", 2.0), ("g", 0.2), ("m", 0.02))]
    vals.append(np.abs(df.uniform(f"{name}.v", (n,), 0.002)))
    for a in vals:
        a.setflags(write=False)
    return off, tuple(vals)


@functools.lru_cache(maxsize=None)
def _values(tag):
    """[(offset in floats from a 16-byte boundary, (p, g, m, v))] of ALL_SIZES — computed once per tag, never written."""
    return [_fill(f"{tag}.{i}", 1 if len(SIZES) <= i < 2 * len(SIZES) else 0, n) for i, n in enumerate(ALL_SIZES)]


class DevSet:
    """The tensors on the device, each a view into a zeroed buffer with 8 floats of slack: .views[i] = [p, g, m, v].  fresh: zero
    moments; gscale: the gradients times it; values: a list as _values returns it (default: _values(tag))."""

    def __init__(self, tag, fresh=False, gscale=None, values=None):
        self.values = _values(tag) if values is None else values
        self.bufs, self.views = [], []
        for off, (p, g, m, v) in self.values:
            if fresh:
                m, v = np.zeros_like(m), np.zeros_like(v)
            row = []
            for k, a in enumerate((p, g, m, v)):
                buf = torch.zeros(a.size + 8, device="cuda")
                assert buf.data_ptr() % 16 == 0
                view = buf[off:off + a.size]
                src = T(a)
                view.copy_(src * gscale if (k == 1 and gscale is not None) else src)
                row.append(view)
                self.bufs.append((off, a.size, buf))
            assert row[0].data_ptr() % 16 == 4 * off
            self.views.append(row)

    def descs(self):
        from wsmgmap.optim import _AdamDesc
        d = (_AdamDesc * len(self.views))()
        for x, (p, g, m, v) in zip(d, self.views):
            x.param, x.grad, x.exp_avg, x.exp_avg_sq, x.n = p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), p.numel()
        return d

    def params(self):
        out = []
        for p, g, _, _ in self.views:
            q = torch.nn.Parameter(p)
            assert q.data_ptr() == p.data_ptr()
            q.grad = g
            out.append(q)
        return out

    def slack_untouched(self):
        return all(bool((buf[:off] == 0).all()) and bool((buf[off + n:] == 0).all()) for off, n, buf in self.bufs)

    def grads_unchanged(self):
        return all(torch.equal(row[1].cpu().view(torch.int32), T(vals[1]).view(torch.int32))
                   for row, (_, vals) in zip(self.views, self.values))


def _bits(t):
    t = t.detach().contiguous()
    return t.view(torch.int64) if t.element_size() == 8 else t.view(torch.int32)


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _ptr(t, byte_offset=0):
    return ctypes.c_void_p(t.data_ptr() + byte_offset)


def _norm64(values):
    return float(torch.linalg.vector_norm(torch.cat([T(g).double() for _, (_, g, _, _) in values])))
