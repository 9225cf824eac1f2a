#!/usr/bin/env python3
"""BBFRAME -> TS parser bank timing: S streams x F BBFRAMEs of 8PSK 3/4 normal frames (kbch 48408) per call,
frames resident in HBM.  Prints one JSON line: packets/s, frames/s, GB/s moved (read DFL/8 + write 188 per 188) against HBM.
--ma: the same frames through the mode-adaptation mode (CCM sizes, SIS, no ISSY / NPD: the same bytes in and out, so the two figures
compare like with like; MA_ISSY=2|3 and MA_NPD=1 in the environment add the fields, payload then from tests/ma_ref.py)."""
import json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import numpy as np
import torch
import __graft_entry__ as g
import orc_bbts as B

pkg = g.load_package()
eng = pkg.Engine(0)
S = int(os.environ.get('STREAMS', '4096'))
F = int(os.environ.get('FRAMES', '4'))
KBCH = int(os.environ.get('KBCH', '48408'))
fb = KBCH // 8
D = fb - 10
rng = np.random.default_rng(0)
nfr = 4 * F
pk = B.ts_packets(nfr * D // 188 + 2, rng)
fr = torch.from_numpy(B.bbframes_from_ts(pk, KBCH, nfr)).cuda()
bank = pkg.BbTsParserBank(eng, S, KBCH, F)
MA = '--ma' in sys.argv
if MA:
    issy, npd = int(os.environ.get('MA_ISSY', '0')), int(os.environ.get('MA_NPD', '0'))
    if issy or npd:
        import ma_ref as M
        ts = M.make_ts(nfr * D // 188 + 2, rng, null_runs=False)
        st, _ = M.slot_stream(ts, issy, bool(npd))
        fr = torch.from_numpy(np.stack([f for f, _ in M.frames_of_stream(st, M.slot_len(issy, npd), [KBCH], sis=True, issyi=issy > 0, npd=bool(npd))][:nfr])).cuda()
    bank.set_mode_adaptation(True, issy_bytes=issy)
calls = [[fr[k * F:(k + 1) * F].reshape(-1).clone() for _ in range(S)] for k in range(4)]
outs = [torch.zeros(F * fb + 376, dtype=torch.uint8, device='cuda') for _ in range(S)]
if MA:
    # argument arrays built once (8 output slots per stream: building them in Python per call would cost more than the kernels)
    import ctypes as C
    pout = (C.c_void_p * (8 * S))(*[outs[i // 8].data_ptr() if i % 8 == 0 else None for i in range(8 * S)])
    pin = [(C.c_void_p * S)(*[t.data_ptr() for t in calls[k]]) for k in range(4)]
    cnt, nbuf, need = (C.c_int * S)(*[F] * S), (C.c_int * (8 * S))(), (C.c_int * (8 * S))()

    def run(k):
        eng._check(bank.lib.dvbs2gpu_bbts_process_ma_batch(bank.h, pin[k], None, cnt, pout, F * fb + 376, nbuf, need, eng._stream()))
        return np.frombuffer(nbuf, np.int32)[::8].tolist()
else:
    run = lambda k: bank.process_batch(calls[k], outs)
for k in range(4):
    nb = run(k)
torch.cuda.synchronize()
reps = int(os.environ.get('REPS', '5'))
t0 = time.perf_counter()
tot = 0
for r in range(reps):
    for k in range(4):
        tot += sum(run(k))
torch.cuda.synchronize()
dt = (time.perf_counter() - t0) / (4 * reps)
# check: the packets of the last call against the transmitted ones for stream 0 (stream state wrapped around the 4 calls: resync'd by SYNCD)
o = outs[0][:nb[0]].cpu().numpy().reshape(-1, 188)
assert np.all(o[:, 0] == 0x47)
print(json.dumps({'mode': 'mode adaptation' if MA else 'reference', 'streams': S, 'frames_per_call': F, 'kbch': KBCH, 'ms_per_call': round(dt * 1e3, 3),
                  'frames_per_s': round(S * F / dt), 'ts_packets_per_s': round(tot / 188 / (4 * reps) / dt),
                  'GB_per_s_read_plus_write': round((S * F * D + tot / (4 * reps)) / dt / 1e9, 1), 'includes': 'host arg upload + sync per call'}))
