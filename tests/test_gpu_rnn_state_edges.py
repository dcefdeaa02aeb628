"""GPU: the persistent state-encoder kernels of csrc/wsmg_rnn.hip (gru_fwd8 / gru_bwd8 / lstm_state_fwd8 / lstm_state_bwd8) against
float64 at their launch edges, driven through the cell descriptions ops.GRU / ops.LSTM on gi directly: no input projection whose
float32 error could hide the kernel's.  Inputs, references and bars are those of tests/rnn_state_cases.py (checked on the CPU by
tests/test_rnn_state_cases_cpu.py): every bar is 4 x the error of the same formula in float32 on the CPU, and never looser than the
bar test_masked_gru_persistent_kernel / test_gpu_lstm_state._kernel_case apply to the same quantity.  Every comparison prints
`name: err / bar`; the module prints the worst ratio per cell and output at its end (profiles/rnn_state_edges.txt).

What is pinned, and what held it before:
a. every case      y, every saved tensor (r, z, n, W_hn h + b_hn; gates, c), the LSTM's c_T, dgi, the GRU's dgh, dh0 / dc0 — lengths
                   around BWD_RING = 4, the documented maximum 200 and the launcher's limit 1023; 1, 2, 7, 8 batch slots; restarts at
                   every step, at consecutive steps, in every column at once, at the last step under a final-state gradient, none at
                   all; saturated gates; a loss that reads c_T alone.  Outputs start as NaN and are one time step longer than the
                   launch: the extra row must stay NaN, every row of the launch must be written.  Two launches are bit-identical
                   — before: four (T, N) GRU cases and the LSTM's through the module's float32 addmm at 10 to 30 times these bars;
                   dhT, the saved tensors and dgh against no reference at all
b. wrappers        ops.masked_gru / ops.masked_lstm (autograd) on the length-1, last_step and no-dy cases, dW_hh and db_hh included
c. workspace reuse one workspace zeroed once, then (5, 8), (3, 2), another (5, 8), (9, 1) forward and backward without a clear:
                   the GRU's _owned entry points and both cells' _chain entry points with no counters — before: route against route,
                   bit for bit, at one T and N
d. refusals        N = 9, T = 0, T = 1024, hidden = 256, a workspace 64 bytes off its alignment, steps_per_chunk 0 and not dividing T:
                   WSMG_EINVAL, nothing written, no status bit — before: the instruction RNN's only"""
import pytest
import torch

import rnn_state_cases as rc

pytestmark = pytest.mark.gpu

H = rc.H
EINVAL = -1
NAN = float("nan")
CELLS = ["GRU", "LSTM"]
WORST = {}                # (cell, output) -> (worst error / bar, where)
SAVED = {"GRU": ["r", "z", "n", "ghn"], "LSTM": ["gates", "c"]}      # the order of cell.new_saves


@pytest.fixture(scope="module")
def ops():
    from wsmgmap import ops as o
    yield o
    for (cell, n), (x, where) in sorted(WORST.items()):
        print(f"\nworst measured error / bar, {cell} {n}: {x:.3f} at {where}", end="")
    print()


def nan(*shape):
    return torch.full(shape, NAN, device="cuda")


def close(name, got, ref, bar, key):
    q, err = rc.ratio(got, ref, bar)
    print(f"{name}: {err:.3e} / {float(bar.max()):.3e} (ref max {float(ref.abs().max()):.3e}), error / bar {q:.3f}")
    if q > WORST.get(key, (-1.0,))[0]:
        WORST[key] = (q, name)
    assert q <= 1.0, f"{name}: max abs err {err:.3e}, {q:.3f} x its bar {float(bar.max()):.3e}"


def device_inputs(c):
    return {k: c[k].cuda() for k in ("gi", "w_hh", "b_hh", "state", "masks", "gy", "g_end")}


def run(ops, cell_name, c, d, ws=None, owned=False, chain_steps=None):
    """One forward and one backward launch of case c (d = device_inputs(c)) into NaN-filled outputs one time step longer than the
    launch.  ws None: a fresh workspace and the clearing entry points.  -> {output name: tensor}, the extra rows included."""
    cell = getattr(ops, cell_name)
    Tn, N, R, G = c["spec"]["T"], c["spec"]["N"], cell.state_rows, cell.G
    chain = None if chain_steps is None else (chain_steps, None, 0, None)
    y, tail = nan(Tn + 1, N, H), nan(max(R - 1, 1), N, H)
    saves = [nan(Tn + 1, N, w * H) for w in cell.save_widths]
    w = ws if ws is not None else ops._rnn_workspace(cell.workspace_bytes(Tn), y.device)
    cell.launch_fwd(d["gi"], d["w_hh"], d["b_hh"], cell.rows(d["state"]), d["masks"], y, tail, saves, 0, Tn, w, owned=owned, chain=chain)
    dgi = nan(Tn + 1, N, G * H)
    dgh = nan(Tn + 1, N, G * H) if cell.own_dgh else dgi
    d0 = nan(R, N, H)
    d_end = [ops._prow(d["g_end"], k) if on else None for k, on in enumerate(c["ends"])]
    w = ws if ws is not None else ops._rnn_workspace(cell.workspace_bytes(Tn), y.device)
    cell.launch_bwd(d["gy"], d_end if any(c["ends"]) else None, d["w_hh"], cell.rows(d["state"]), d["masks"], y, saves, dgi, dgh, cell.rows(d0),
                    0, Tn, w, owned=owned, chain=chain)
    torch.cuda.synchronize()
    ops.check_rnn_status()
    out = dict(zip(SAVED[cell_name], saves), y=y, dgi=dgi, dh0=d0[0])
    if cell.own_dgh:
        out["dgh"] = dgh
    else:
        out.update(c_T=tail[0], dc0=d0[1])
    return out


def check(name, cell_name, c, out):
    """The extra row still NaN, every row of the launch finite and within its bar of float64."""
    Tn = c["spec"]["T"]
    for k in rc.FORWARD[cell_name] + rc.BACKWARD[cell_name]:
        got = out[k]
        if got.shape[0] == Tn + 1 and got.dim() == 3:
            assert bool(torch.isnan(got[Tn]).all()), f"{name}.{k}: the row after the launch was written"
            got = got[:Tn]
        assert bool(torch.isfinite(got).all()), f"{name}.{k}: not every element of the launch was written"
        close(f"{name}.{k}", got, c["ref"][k], c["bar"][k], (cell_name, k))


# ----------------------------------------------------------------------------- a. every case, through the clearing entry points
@pytest.mark.parametrize("cell_name,name", [(cell, n) for cell in CELLS for n in rc.CASES[cell]])
def test_state_kernels_against_float64(ops, cell_name, name):
    c = rc.case(cell_name, name)
    d = device_inputs(c)
    out = run(ops, cell_name, c, d)
    check(f"{cell_name}.{name}", cell_name, c, out)
    again = run(ops, cell_name, c, d)
    for k, v in out.items():
        assert torch.equal(v.view(torch.int32), again[k].view(torch.int32)), f"{cell_name}.{name}.{k}: two launches differ"
    if name == "saturated":
        for nm, col, val in rc.saturated_slots(cell_name):
            got = out[nm][:c["spec"]["T"], rc.SAT_SLOT, col].double().cpu()
            assert float((got - val).abs().max()) <= 2.0 ** -23, f"{cell_name}.saturated.{nm}[{col}]: {got.tolist()} is not {val}"


# ----------------------------------------------------------------------------- b. the autograd wrappers
@pytest.mark.parametrize("cell_name,name", [(cell, n) for cell in CELLS for n in rc.WRAPPER_CASES[cell]])
def test_autograd_wrappers_against_float64(ops, cell_name, name):
    c = rc.case(cell_name, name)
    d = device_inputs(c)
    gi, w_hh, b_hh, state = (d[k].clone().requires_grad_(True) for k in ("gi", "w_hh", "b_hh", "state"))
    if cell_name == "GRU":
        y = ops.masked_gru(gi, w_hh, b_hh, state[0], d["masks"])
        ends, got = [y[-1]], {}
    else:
        y, c_T = ops.masked_lstm(gi, w_hh, b_hh, state[0], state[1], d["masks"])
        ends, got = [y[-1], c_T], {"c_T": c_T}
    loss = (y * d["gy"]).sum() if c["spec"]["dy"] else 0.0
    for on, e, g in zip(c["ends"], ends, d["g_end"]):
        if on:
            loss = loss + (e * g).sum()
    loss.backward()
    torch.cuda.synchronize()
    ops.check_rnn_status()
    got.update(y=y, dgi=gi.grad, dh0=state.grad[0], dw_hh=w_hh.grad, db_hh=b_hh.grad)
    if cell_name == "LSTM":
        got["dc0"] = state.grad[1]
    for k, v in got.items():
        close(f"wrapper.{cell_name}.{name}.{k}", v, c["ref"][k], c["bar"][k], (cell_name, "wrapper " + k))


# ----------------------------------------------------------------------------- c. one workspace, never cleared between launches
@pytest.mark.parametrize("cell_name,route", [("GRU", "owned"), ("GRU", "chain"), ("LSTM", "chain")])
def test_one_workspace_serves_launches_of_other_lengths_and_batches(ops, cell_name, route):
    cell = getattr(ops, cell_name)
    ws = torch.zeros((int(cell.workspace_bytes(9)) + 3) // 4, device="cuda")
    assert ws.data_ptr() % 128 == 0
    for i, name in enumerate(rc.REUSE):
        c = rc.case(cell_name, name)
        Tn = c["spec"]["T"]
        assert int(cell.workspace_bytes(Tn)) <= ws.numel() * 4
        steps = None if route == "owned" else (1 if i % 2 else Tn)      # chunks of the whole launch, and of one step
        out = run(ops, cell_name, c, device_inputs(c), ws=ws, owned=route == "owned", chain_steps=steps)
        check(f"reuse.{route}.{cell_name}.{i}.{name}", cell_name, c, out)


# ----------------------------------------------------------------------------- d. refusals
def _refusal_args(ops, cell_name):
    """Tensors for a (T = 4, N = 3) launch that would be taken; every output NaN."""
    cell = getattr(ops, cell_name)
    Tn, N, R, G = 4, 3, cell.state_rows, cell.G
    z = lambda *s: torch.zeros(*s, device="cuda")       # noqa: E731
    a = dict(gi=z(Tn, N, G * H), w_hh=z(G * H, H), b_hh=z(G * H), state=z(R, N, H), masks=torch.ones(Tn, N, device="cuda"), gy=z(Tn, N, H),
             y=nan(Tn, N, H), tail=nan(max(R - 1, 1), N, H), saves=[nan(Tn, N, w * H) for w in cell.save_widths], dgi=nan(Tn, N, G * H),
             d0=nan(R, N, H), ws=torch.zeros((int(cell.workspace_bytes(1024)) + 3) // 4 + 32, device="cuda"))
    a["dgh"] = nan(Tn, N, G * H) if cell.own_dgh else a["dgi"]
    return a


def _launch(ops, cell_name, a, rcs, T=4, N=3, hidden=H, ws_off=0, owned=False, chain_steps=None):
    """Forward and backward through the cell description with the sizes the kernels are told overridden; the entry points' return
    codes go to rcs (wsmgmap._abi.call is replaced by the caller)."""
    cell = getattr(ops, cell_name)
    chain = None if chain_steps is None else (chain_steps, None, 0, None)
    y = a["y"].view(-1)[:4 * N * hidden].view(4, N, hidden) if (N, hidden) != (3, H) else a["y"]       # launch_* read N and hidden off y
    ws = a["ws"][ws_off // 4:]
    cell.launch_fwd(a["gi"], a["w_hh"], a["b_hh"], cell.rows(a["state"]), a["masks"], y, a["tail"], a["saves"], 0, T, ws, owned=owned, chain=chain)
    cell.launch_bwd(a["gy"], None, a["w_hh"], cell.rows(a["state"]), a["masks"], y, a["saves"], a["dgi"], a["dgh"], cell.rows(a["d0"]), 0, T, ws,
                    owned=owned, chain=chain)
    assert len(rcs) >= 2
    return rcs[-2:]


@pytest.mark.parametrize("cell_name", CELLS)
def test_state_kernels_refuse_bad_launches_before_anything_is_queued(ops, monkeypatch, cell_name):
    from wsmgmap import _abi
    cell = getattr(ops, cell_name)
    names, rcs = [], []

    def call(name, *args):
        names.append(name)
        rcs.append(getattr(_abi.lib(), name)(*args))
    monkeypatch.setattr(_abi, "call", call)
    a = _refusal_args(ops, cell_name)
    # N = 9 and hidden = 256 are told to the kernels through y's shape: a y of as many elements (9 x 512 > 3 x 512 needs its own)
    wide = dict(a, y=nan(4, 9, H))

    def untouched(what):
        torch.cuda.synchronize()
        for k in ("y", "tail", "dgi", "dgh", "d0"):
            assert bool(torch.isnan(a[k]).all()), f"{cell_name}, {what}: the refused launch wrote {k}"
        assert bool(torch.isnan(wide["y"]).all()) and all(bool(torch.isnan(t).all()) for t in a["saves"]), (cell_name, what)
        assert int(_abi.lib().wsmg_rnn_status(0)) == 0, (cell_name, what)
    routes = [dict()] + ([dict(owned=True)] if cell.fwd[1] else []) + [dict(chain_steps=2)]
    for route in routes:
        want = [cell.fwd[2 if "chain_steps" in route else 1 if route else 0], cell.bwd[2 if "chain_steps" in route else 1 if route else 0]]
        for what, args, kw in [("N = 9", wide, dict(N=9)), ("T = 0", a, dict(T=0)), ("T = 1024", a, dict(T=1024)),
                               ("hidden = 256", a, dict(hidden=256)), ("workspace + 64 bytes", a, dict(ws_off=64))]:
            if "chain_steps" in route and what == "T = 1024":
                kw = dict(kw, chain_steps=1024)             # a chunk length that divides T: the refusal is the length's
            got = _launch(ops, cell_name, args, rcs, **dict(route, **kw))
            assert names[-2:] == want and got == [EINVAL, EINVAL], (cell_name, route, what, names[-2:], got)
            untouched(what)
    for what, steps in [("steps_per_chunk = 0", 0), ("steps_per_chunk = 3 does not divide T = 4", 3)]:
        got = _launch(ops, cell_name, a, rcs, chain_steps=steps)
        assert names[-2:] == [cell.fwd[2], cell.bwd[2]] and got == [EINVAL, EINVAL], (cell_name, what, got)
        untouched(what)
    assert int((a["ws"] != 0).sum()) == 0, "a refused launch cleared or wrote its workspace"
    # and the same tensors are taken when nothing is wrong: the refusals above are the arguments', not the harness's
    assert _launch(ops, cell_name, a, rcs) == [0, 0] and _launch(ops, cell_name, a, rcs, chain_steps=2) == [0, 0]
    torch.cuda.synchronize()
    assert all(bool(torch.isfinite(a[k]).all()) for k in ("y", "dgi", "dgh", "d0")) and int(_abi.lib().wsmg_rnn_status(0)) == 0
