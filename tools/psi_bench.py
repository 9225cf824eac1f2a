#!/usr/bin/env python3
"""PSI section bank timing: 4096 streams x 309 packets per call -- the TS of the headline step -- resident in HBM, each
stream a multiplex with a PAT and two PMTs at a plausible share of the packets (one PAT and one of each PMT per 100 packets, the
rest elementary-stream packets and null packets; the two buffer sets carry the same tables, a steady multiplex: after the warm-up no
section is CHANGED and no section byte crosses to the host).  Three calls are timed in alternation in one process:
  psi_rows      dvbs2gpu_psi_process_batch without output buffers (rows and counters), PAT and both PMT PIDs watched;
  psi_deliver1  the same with output buffers and deliver mode 1 (valid changed sections only);
  monitor       dvbs2gpu_tsmon_process_batch without output buffers on the same buffers (the scale; existing code).
Each time is a host clock around one synchronous call (argument upload and read-back included), median of REPS rounds after a
warm-up round.  Two sets of buffers alternate, so a call's input was last touched two calls ago (2 x 238 MB of TS: more than the
256 MB Infinity Cache holds).  Bytes are counted from the shapes: what a call must touch, one 64-byte access per packet plus the
watched packets' payloads.  Writes one JSON object to --out (default profiles/psi_bench.json) and prints it."""
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
import psi_ref as P

HBM_MEASURED = 6.29e12          # bytes/s, a float4 copy on this part (the figure the other profiles are held against)
S = int(os.environ.get('STREAMS', '4096'))
REPS = int(os.environ.get('REPS', '10'))
NPK, PATTERNS = 309, 16
out_path = sys.argv[sys.argv.index('--out') + 1] if '--out' in sys.argv else os.path.join(ROOT, 'profiles', 'psi_bench.json')
PMT_PIDS = [0x100, 0x101]


def mux(seed, tsid):
    rng = np.random.default_rng(seed)
    zp, zm = P.Packetiser(0, int(rng.integers(16))), [P.Packetiser(p, int(rng.integers(16))) for p in PMT_PIDS]
    pat = P.pat(tsid, [(0, 0x10), (1, PMT_PIDS[0]), (2, PMT_PIDS[1])])
    pmts = [P.pmt(1, 0x200, [(0x1b, 0x200), (0x0f, 0x201), (0x06, 0x202)], es_info=b'\x0a\x04eng\x00'), P.pmt(2, 0x210, [(0x02, 0x210), (0x04, 0x211)], program_info=bytes(190))]
    parts, cc = [], 0
    while sum(len(p) for p in parts) < NPK:
        psi = [zp.lay([pat]), zm[0].lay([pmts[0]]), zm[1].lay([pmts[1]])]      # the second PMT spans two packets
        es = P.filler(0x200, 88, rng, cc)
        cc += 88
        null = np.tile(P.packet(0x1FFF, 0), (8, 1))
        parts += [psi[0], es[:30], psi[1], es[30:60], null, psi[2], es[60:]]
    return np.concatenate(parts)[:NPK]


pkg = g.load_package()
eng = pkg.Engine(0)
sel = torch.arange(S, device='cuda') % PATTERNS
ts = [torch.from_numpy(np.stack([mux(100 * k + p, p + 1).reshape(-1) for p in range(PATTERNS)])).cuda()[sel].contiguous() for k in range(2)]
out = torch.zeros((S, 4096), dtype=torch.uint8, device='cuda')
rows_bank, del_bank = pkg.PsiBank(eng, S, NPK, 64), pkg.PsiBank(eng, S, NPK, 64)
mon = pkg.TsMonitorBank(eng, S, NPK)
for i in range(S):
    for b in (rows_bank, del_bank):
        b.set_watch(i, 1, PMT_PIDS[0], 2), b.set_watch(i, 2, PMT_PIDS[1], 2)
    del_bank.set_deliver(i, 1)


def ptrs(t):
    return (C.c_void_p * S)(*[t[i].data_ptr() for i in range(S)])


p_ts, p_out = [ptrs(t) for t in ts], ptrs(out)
nb = (C.c_int * S)(*[NPK * 188] * S)
ob, orows = (C.c_int * S)(), (C.c_int * S)()
lib, st = eng.lib, eng._stream()


def run(name, k):
    if name == 'psi_rows':
        eng._check(lib.dvbs2gpu_psi_process_batch(rows_bank.h, p_ts[k], nb, None, 0, None, orows, st))
    elif name == 'psi_deliver1':
        eng._check(lib.dvbs2gpu_psi_process_batch(del_bank.h, p_ts[k], nb, p_out, 4096, ob, orows, st))
    else:
        eng._check(lib.dvbs2gpu_tsmon_process_batch(mon.h, p_ts[k], nb, None, 0, None, st))


names = ('psi_rows', 'psi_deliver1', 'monitor')
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
# the device bank against the model on one stream: the same calls in the same order (the buffers alternate, the continuity counters
# start again with every buffer: the model sees that too)
m = P.Assembler()
m.set_watch(1, PMT_PIDS[0], 2), m.set_watch(2, PMT_PIDS[1], 2)
host = [t[5].cpu().numpy() for t in ts]
for r in range(REPS + 1):
    for k in range(2):
        m.process(host[k], deliver=False)
assert rows_bank.stats(5) == m.stats() and rows_bank.section_table(5) == m.table and m.stats()['sections'] > 0, (rows_bank.stats(5), m.stats())
watched = int(sum(np.isin((h[:NPK * 188].reshape(-1, 188)[:, 1].astype(int) & 0x1f) << 8 | h[:NPK * 188].reshape(-1, 188)[:, 2], [0] + PMT_PIDS).sum() for h in host)) // 2
packets = S * NPK
touch = packets * 64 + S * watched * 188                            # one access per packet, the watched packets whole
bytes_moved = {'psi_rows': touch, 'psi_deliver1': touch + int(sum(ob)) * 2, 'monitor': packets * 64 + packets}
res = {'streams': S, 'packets_per_stream_call': NPK, 'watched_packets_per_stream_call': watched, 'sections_per_stream_call': int(orows[5]),
       'ts_bytes_per_call': packets * 188, 'delivered_bytes_last_call': int(sum(ob)), 'reps': REPS,
       'timing': 'host clock around one synchronous call, argument upload and read-back included; median / min of 2 x reps calls',
       'hbm_bytes_per_s_reference': HBM_MEASURED}
for n in names:
    med = float(np.median(times[n]))
    res[n] = {'ms_per_call': round(med * 1e3, 3), 'min_ms': round(min(times[n]) * 1e3, 3), 'max_ms': round(max(times[n]) * 1e3, 3),
              'bytes_touched': int(bytes_moved[n]), 'GB_per_s': round(bytes_moved[n] / med / 1e9, 1), 'fraction_of_hbm': round(bytes_moved[n] / med / HBM_MEASURED, 4)}
res['psi_rows_over_monitor'] = round(res['psi_rows']['ms_per_call'] / res['monitor']['ms_per_call'], 3)
res['psi_deliver1_over_monitor'] = round(res['psi_deliver1']['ms_per_call'] / res['monitor']['ms_per_call'], 3)
os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
with open(out_path, 'w') as f:
    json.dump(res, f, indent=1)
    f.write('\n')
print(json.dumps(res))
