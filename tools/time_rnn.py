#!/usr/bin/env python3
"""GPU-box tool: per-kernel time of the persistent GRU / LSTM-state / bi-LSTM / instruction GRU-LSTM launches, and of the
stock routes of the LSTM state encoder and of the instruction encoders for contrast (HIP events, no other load)."""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "ws-mgmap_amd"))
import torch
from wsmgmap import ops, _abi
L = _abi.lib(); P = ops._p; st = ops._stream
T, N, H = int(os.environ.get("T", "64")), 8, 512
torch.manual_seed(0)
gi = torch.randn(T, N, 3 * H, device="cuda"); whh = torch.randn(3 * H, H, device="cuda") * 0.04
bhh = torch.randn(3 * H, device="cuda") * 0.1; h0 = torch.randn(N, H, device="cuda")
masks = torch.ones(T, N, device="cuda"); masks[0] = 0
y = torch.empty(T, N, H, device="cuda"); saves = [torch.empty(T, N, H, device="cuda") for _ in range(4)]
gy = torch.randn(T, N, H, device="cuda")
dgi = torch.empty(T, N, 3 * H, device="cuda"); dgh = torch.empty_like(dgi); dh0 = torch.empty(N, H, device="cuda")
ws = ops._rnn_workspace(L.wsmg_gru_workspace_bytes(T), gi.device)
def fwd(): _abi.call("wsmg_gru_fwd", P(gi), P(whh), P(bhh), P(h0), P(masks), T, N, H, P(y), *[P(s) for s in saves], P(ws), st())
def bwd(): _abi.call("wsmg_gru_bwd", P(gy), None, P(whh), P(h0), P(masks), P(y), *[P(s) for s in saves], T, N, H, P(dgi), P(dgh), P(dh0), P(ws), st())
def timeit(f, reps=20):
    for _ in range(3): f()
    torch.cuda.synchronize()
    a = torch.cuda.Event(enable_timing=True); b = torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps): f()
    b.record(); torch.cuda.synchronize()
    return a.elapsed_time(b) / reps * 1e3
tf, tb = timeit(fwd), timeit(bwd)
print(f"GRU T={T} N={N}: fwd {tf:.1f} us ({tf / T:.2f} us/step)  bwd {tb:.1f} us ({tb / T:.2f} us/step)")
# LSTM state encoder (STATE_ENCODER.rnn_type = "LSTM"): the persistent kernel pair on the same sequence, then the stock route
sgi = torch.randn(T, N, 4 * H, device="cuda"); swhh = torch.randn(4 * H, H, device="cuda") * 0.04
sbhh = torch.randn(4 * H, device="cuda") * 0.1; c0 = torch.randn(N, H, device="cuda")
sy = torch.empty(T, N, H, device="cuda"); scT = torch.empty(N, H, device="cuda")
ssg = torch.empty(T, N, 4 * H, device="cuda"); ssc = torch.empty(T, N, H, device="cuda")
sdg = torch.empty(T, N, 4 * H, device="cuda"); sdh0 = torch.empty(N, H, device="cuda"); sdc0 = torch.empty(N, H, device="cuda")
sws = ops._rnn_workspace(L.wsmg_lstm_state_workspace_bytes(T), gi.device)
def sfwd(): _abi.call("wsmg_lstm_state_fwd", P(sgi), P(swhh), P(sbhh), P(h0), P(c0), P(masks), T, N, H, P(sy), P(scT), P(ssg), P(ssc), P(sws), st())
def sbwd(): _abi.call("wsmg_lstm_state_bwd", P(gy), None, None, P(swhh), P(c0), P(masks), P(ssg), P(ssc), T, N, H, P(sdg), P(sdh0), P(sdc0), P(sws), st())
tsf, tsb = timeit(sfwd), timeit(sbwd)
print(f"LSTM state T={T} N={N}: fwd {tsf:.1f} us ({tsf / T:.2f} us/step)  bwd {tsb:.1f} us ({tsb / T:.2f} us/step)")
from wsmgmap.models.rnn_state_encoder import RNNStateEncoder
enc = RNNStateEncoder(640, H, rnn_type="LSTM").cuda()
sx = torch.randn(T * N, 640, device="cuda", requires_grad=True); shc = torch.randn(2, N, H, device="cuda")
smk = masks.reshape(-1, 1); sgy = gy.reshape(T * N, H)
def kf(): enc(sx, shc, smk)
def kfb(): (enc(sx, shc, smk)[0] * sgy).sum().backward()
def stf(): enc.forward_stock(sx, shc, smk)
def stfb(): (enc.forward_stock(sx, shc, smk)[0] * sgy).sum().backward()
tkf, tkfb, tstf, tstfb = timeit(kf), timeit(kfb), timeit(stf), timeit(stfb)
print(f"LSTM state module T={T} N={N} (in 640): kernel route fwd {tkf:.1f} us  fwd+bwd {tkfb:.1f} us | "
      f"stock nn.LSTM route (forward_stock) fwd {tstf:.1f} us  fwd+bwd {tstfb:.1f} us")
U, Lt = 8, int(os.environ.get("L", "80"))
lgi = torch.randn(U, Lt, 2, 512, device="cuda", requires_grad=True); lw = torch.randn(2, 512, 128, device="cuda") * 0.08
lb = torch.randn(2, 512, device="cuda") * 0.1; lens = torch.full((U,), Lt, device="cuda", dtype=torch.int32)
lgy = torch.randn(U, Lt, 256, device="cuda")
def lf():
    return ops.bilstm(lgi, lw, lb, lens)
tlf = timeit(lf)
def lfb():
    o = ops.bilstm(lgi, lw, lb, lens); (o * lgy).sum().backward()
tlfb = timeit(lfb)
print(f"LSTM L={Lt} U={U}: fwd (op) {tlf:.1f} us  fwd+bwd (op) {tlfb:.1f} us")
# instruction encoders (INSTRUCTION_ENCODER.rnn_type / .bidirectional / .hidden_size): per row and U in (1, 8), the kernel pair
# alone (wsmg_instr_rnn_fwd / _bwd; the default bi-LSTM through the same entry points) and the stock packed MIOpen route
from wsmgmap.models.encoders.instruction_encoder import InstructionEncoder
from wsmgmap.config import default_model_config
for cell, D, Hh in (("LSTM", 2, 128), ("GRU", 2, 128), ("LSTM", 1, 256), ("GRU", 1, 256)):
    G, code = (4 if cell == "LSTM" else 3), ops.CELLS[cell]
    for U in (1, 8):
        igi = torch.randn(U, Lt, D, G * Hh, device="cuda"); iw = torch.randn(D, G * Hh, Hh, device="cuda") * Hh ** -0.5
        ib = torch.randn(D, G * Hh, device="cuda") * 0.1; ilen = torch.full((U,), Lt, device="cuda", dtype=torch.int32)
        iout = torch.empty(U, Lt, D * Hh, device="cuda"); isg = torch.empty(D, U, Lt, 4, Hh, device="cuda")
        isc = torch.empty(D, U, Lt, Hh, device="cuda"); idgi = torch.empty_like(igi); idgh = torch.empty_like(igi)
        iws = ops._rnn_workspace(L.wsmg_instr_rnn_workspace_bytes(code, Hh, D, Lt), igi.device)
        def ifwd(): _abi.call("wsmg_instr_rnn_fwd", code, P(igi), P(iw), P(ib), P(ilen), U, Lt, Hh, D, P(iout), P(isg), P(isc), P(iws), st())
        def ibwd(): _abi.call("wsmg_instr_rnn_bwd", code, P(iout), P(iw), P(ilen), P(iout), P(isg), P(isc), U, Lt, Hh, D, P(idgi), P(idgh), P(iws), st())
        tif, tib = timeit(ifwd), timeit(ibwd)
        cfg = default_model_config().INSTRUCTION_ENCODER
        cfg.rnn_type, cfg.bidirectional, cfg.hidden_size = cell, D == 2, Hh
        enc = InstructionEncoder(cfg).cuda()
        tok = torch.randint(1, 2504, (U, Lt), device="cuda")
        dd = enc.dedup(tok, reuse=False)
        egy = torch.randn(U, Lt, 256, device="cuda")
        def kr(): (enc.encode_unique(tok, dedup=dd)[0] * egy).sum().backward()
        def sr(): (enc.encode_unique(tok, stock=True, dedup=dd)[0] * egy).sum().backward()
        tk, ts = timeit(kr), timeit(sr)
        print(f"instr {cell} dirs={D} H={Hh} U={U} L={Lt}: kernel fwd {tif:.1f} us ({tif / Lt:.2f} us/step)  bwd {tib:.1f} us "
              f"({tib / Lt:.2f} us/step) | encoder fwd+bwd: kernel route {tk:.1f} us, stock packed route {ts:.1f} us")
