#!/usr/bin/env python3
"""TS monitor bank timing: 4096 streams x 309 packets per call -- the TS of the headline step, 8 BBFRAMEs of
58192 bits per stream -- resident in HBM as the packetiser left it.  Three calls are timed in alternation in one process:
  bbts          dvbs2gpu_bbts_process_batch, the existing call that produces these bytes (the scale);
  monitor       dvbs2gpu_tsmon_process_batch without output buffers (statistics and PID table);
  monitor_pass3 the same with a pass list of three PIDs per stream and the passing packets compacted into output buffers.
Each time is a host clock around one synchronous call (argument upload and read-back included), median of REPS rounds after a
warm-up round.  Two sets of buffers alternate, so a call's input was last touched two calls ago (2 x 240 MB of TS: more than the
256 MB Infinity Cache holds).  Bytes are counted from the shapes: what the call must read and write, headers at the 64-byte
granularity of a memory access.  Writes one JSON object to --out (default profiles/tsmon_bench.json) and prints it."""
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import numpy as np
import torch
import __graft_entry__ as g
import orc_bbts as B
import tsmon_ref as T

HBM_MEASURED = 6.29e12          # bytes/s, a float4 copy on this part (the figure the other profiles are held against)
S = int(os.environ.get('STREAMS', '4096'))
REPS = int(os.environ.get('REPS', '10'))
KBCH, F, PATTERNS = 58192, 8, 16
out_path = sys.argv[sys.argv.index('--out') + 1] if '--out' in sys.argv else os.path.join(ROOT, 'profiles', 'tsmon_bench.json')

pkg = g.load_package()
eng = pkg.Engine(0)
fb = KBCH // 8
npk = F * (fb - 10) // 188                                          # 309
PIDS = [0, 0x11, 0x100, 0x101, 0x102, 0x200, 0x201, 0x1FFE]
sel = torch.arange(S, device='cuda') % PATTERNS
frames = []
for k in range(2):
    pats = [B.bbframes_from_ts(T.make_mux(np.random.default_rng(100 * k + p), npk + 2, PIDS)[0], KBCH, F).reshape(-1) for p in range(PATTERNS)]
    frames.append(torch.from_numpy(np.stack(pats)).cuda()[sel].contiguous())
cap = F * fb + 376
ts = [torch.zeros((S, cap), dtype=torch.uint8, device='cuda') for _ in range(2)]
MAXP = npk + 2                                                     # a call that completes a carried packet brings one more
passed = torch.zeros((S, MAXP * 188), dtype=torch.uint8, device='cuda')
bank = pkg.BbTsParserBank(eng, S, KBCH, F)
mon, monf = pkg.TsMonitorBank(eng, S, MAXP), pkg.TsMonitorBank(eng, S, MAXP)
for i in range(S):
    monf.set_filter(i, mode=1, pids=[0x100, 0x101, 0x200])


def ptrs(t):
    return (C.c_void_p * S)(*[t[i].data_ptr() for i in range(S)])


p_fr, p_ts, p_pass = [ptrs(t) for t in frames], [ptrs(t) for t in ts], ptrs(passed)
cnt = (C.c_int * S)(*[F] * S)
nb = [(C.c_int * S)(), (C.c_int * S)()]
nbp = (C.c_int * S)()
lib, st = eng.lib, eng._stream()


def run(name, k):
    if name == 'bbts':
        eng._check(lib.dvbs2gpu_bbts_process_batch(bank.h, p_fr[k], cnt, p_ts[k], cap, nb[k], st))
    elif name == 'monitor':
        eng._check(lib.dvbs2gpu_tsmon_process_batch(mon.h, p_ts[k], nb[k], None, 0, None, st))
    else:
        eng._check(lib.dvbs2gpu_tsmon_process_batch(monf.h, p_ts[k], nb[k], p_pass, MAXP * 188, nbp, st))


names = ('bbts', 'monitor', 'monitor_pass3')
times = {n: [] for n in names}
for r in range(REPS + 1):                                           # round 0 warms up
    for name in names:
        for k in range(2):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            run(name, k)
            torch.cuda.synchronize()
            if r:
                times[name].append(time.perf_counter() - t0)
packets = sum(nb[1]) // 188
assert packets >= S * (npk - 1), packets
# the device bank against the model on the last call of one stream (the patterns start afresh every call: the model too)
m = T.Monitor()
m.set_filter(mode=1, pids=[0x100, 0x101, 0x200])
want = m.process(ts[1][5, :nb[1][5]].cpu().numpy())
assert nbp[5] == want.size and np.array_equal(passed[5, :nbp[5]].cpu().numpy(), want)
pass_bytes = sum(nbp)
ts_bytes = sum(nb[1])
bytes_moved = {'bbts': S * F * fb + ts_bytes,                       # BBFRAMEs read, TS written
               'monitor': packets * 64 + packets * 1,               # one 64-byte access per header, the touched state bytes at most
               'monitor_pass3': 2 * packets * 64 + 2 * pass_bytes}  # headers twice (sizes first, then the copy), passing packets read and written
res = {'streams': S, 'packets_per_stream_call': npk, 'ts_bytes_per_call': ts_bytes, 'passed_bytes_per_call': pass_bytes, 'reps': REPS,
       'timing': 'host clock around one synchronous call, argument upload and read-back included; median / min of 2 x reps calls',
       'hbm_bytes_per_s_reference': HBM_MEASURED}
for n in names:
    med = float(np.median(times[n]))
    res[n] = {'ms_per_call': round(med * 1e3, 3), 'min_ms': round(min(times[n]) * 1e3, 3), 'max_ms': round(max(times[n]) * 1e3, 3),
              'bytes_read_plus_written': int(bytes_moved[n]), 'GB_per_s': round(bytes_moved[n] / med / 1e9, 1),
              'fraction_of_hbm': round(bytes_moved[n] / med / HBM_MEASURED, 4)}
res['monitor_over_bbts'] = round(res['monitor']['ms_per_call'] / res['bbts']['ms_per_call'], 3)
res['monitor_pass3_over_bbts'] = round(res['monitor_pass3']['ms_per_call'] / res['bbts']['ms_per_call'], 3)
os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
with open(out_path, 'w') as f:
    json.dump(res, f, indent=1)
    f.write('\n')
print(json.dumps(res))
