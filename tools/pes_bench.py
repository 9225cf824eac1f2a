#!/usr/bin/env python3
"""PES bank timing: 4096 streams x 309 packets per call -- the TS of the headline step -- resident in HBM, each
stream a multiplex with two watched elementary PIDs whose PES packets start every 8 to 12 packets, with PTS that follow the packet
position at 90000 ticks (27 MHz) per packet.  Two calls are timed in alternation in one process:
  pes       dvbs2gpu_pes_process_batch, both PIDs watched, the rate set;
  monitor   dvbs2gpu_tsmon_process_batch without output buffers on the same buffers (the scale; existing code).
Each time is a host clock around one synchronous call (argument upload and read-back included), median of 2 x REPS calls after a
warm-up round.  Two sets of buffers alternate, so a call's input was last touched two calls ago (2 x 238 MB of TS: more than the
256 MB Infinity Cache holds).  Bytes are counted from the shapes: one 64-byte access per packet, for the PES bank 20 bytes more per
start, read twice, a 48-byte row per start and the call record of a stream (1552 bytes) written and copied to the host; for the
monitor its 48 bytes.  Writes one JSON object to --out (default profiles/pes_bench.json) and prints it."""
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
import pes_ref as P

HBM_MEASURED = 6.29e12          # bytes/s, a float4 copy on this part (the figure the other profiles are held against)
S = int(os.environ.get('STREAMS', '4096'))
REPS = int(os.environ.get('REPS', '10'))
NPK, PATTERNS = 309, 16
out_path = sys.argv[sys.argv.index('--out') + 1] if '--out' in sys.argv else os.path.join(ROOT, 'profiles', 'pes_bench.json')
PES_PIDS = [0x200, 0x201]
TPP = 90000
RECORD = 1552


def mux(rng, k):
    """buffer set k of one pattern: 309 packets, the two PIDs in turn, on each a start every 4 to 6 of its packets (8 to 12 of the stream's); the counters and the PTS of set 1 go on where set 0 ended (its last PES packet does not: the first closing of a call is a mismatch)"""
    out = P.null_packets(NPK)
    for j, pid in enumerate(PES_PIDS):
        slots = list(range(j, NPK, 2))                               # every second packet belongs to the PID
        left, cc = 0, (k * len(range(j, NPK, 2))) & 15
        for at in slots:
            pos = k * NPK + at
            if left == 0:
                left = int(rng.integers(4, 7))
                out[at] = P.pes_packet(pid, cc, 0xE0 + j, pts=pos * TPP // 300, declared=left * 184 - 6)
            else:
                out[at] = P.body_packet(pid, cc)
            left, cc = left - 1, (cc + 1) & 15
    return out.reshape(-1)


pkg = g.load_package()
eng = pkg.Engine(0)
sel = torch.arange(S, device='cuda') % PATTERNS
host = [np.stack([mux(np.random.default_rng(100 * k + p), k) for p in range(PATTERNS)]) for k in range(2)]
ts = [torch.from_numpy(h).cuda()[sel].contiguous() for h in host]
bank, mon = pkg.PesBank(eng, S, NPK, 128), pkg.TsMonitorBank(eng, S, NPK)
for i in range(S):
    bank.set_watch(i, 0, PES_PIDS[0]), bank.set_watch(i, 1, PES_PIDS[1])
    bank.set_rate(i, TPP << 24)


def ptrs(t):
    return (C.c_void_p * S)(*[t[i].data_ptr() for i in range(S)])


p_ts = [ptrs(t) for t in ts]
nb = (C.c_int * S)(*[NPK * 188] * S)
orows = (C.c_int * S)()
lib, st = eng.lib, eng._stream()


def run(name, k):
    if name == 'pes':
        eng._check(lib.dvbs2gpu_pes_process_batch(bank.h, p_ts[k], nb, orows, st))
    else:
        eng._check(lib.dvbs2gpu_tsmon_process_batch(mon.h, p_ts[k], nb, None, 0, None, st))


names = ('pes', 'monitor')
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
# the device bank against the model on one stream: the same calls in the same order
m = P.Pes(128)
m.set_watch(0, PES_PIDS[0]), m.set_watch(1, PES_PIDS[1])
m.set_rate(TPP << 24)
for r in range(REPS + 1):
    for k in range(2):
        m.process(host[k][5].reshape(-1, 188))
assert bank.stats(5) == m.stats() and bank.row_table(5) == m.table and bank.stream_stats(5) == m.stream_stats() and m.stats()['closed_ok'] > 0, (bank.stats(5), m.stats())
packets, starts = S * NPK, S * int(orows[5])
bytes_moved = {'pes': packets * 64 + starts * (2 * 20 + 48) + S * RECORD * 2, 'monitor': packets * 64 + packets + S * 48 * 2}
res = {'streams': S, 'packets_per_stream_call': NPK, 'starts_per_stream_call': int(orows[5]), 'ts_bytes_per_call': packets * 188, 'reps': REPS,
       'call_record_bytes_per_stream': {'pes': RECORD, 'monitor': 48},
       'timing': 'host clock around one synchronous call, argument upload and read-back included; median / min of 2 x reps calls',
       'hbm_bytes_per_s_reference': HBM_MEASURED}
for n in names:
    med = float(np.median(times[n]))
    res[n] = {'ms_per_call': round(med * 1e3, 3), 'min_ms': round(min(times[n]) * 1e3, 3), 'max_ms': round(max(times[n]) * 1e3, 3),
              'bytes_touched': int(bytes_moved[n]), 'GB_per_s': round(bytes_moved[n] / med / 1e9, 1), 'fraction_of_hbm': round(bytes_moved[n] / med / HBM_MEASURED, 4)}
res['pes_over_monitor'] = round(res['pes']['ms_per_call'] / res['monitor']['ms_per_call'], 3)
os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
with open(out_path, 'w') as f:
    json.dump(res, f, indent=1)
    f.write('\n')
print(json.dumps(res))
