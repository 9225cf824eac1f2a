#!/usr/bin/env python3
"""T2-MI bank timing: 4096 streams x 309 packets per call -- the TS of the headline step -- resident in HBM, each
stream a T2-MI feed: one PID carries about 95 % of the packets as T2-MI packets with BBFRAMEs of about 6.7 KB of one PLP, the rest
are null packets.  Four calls are timed in alternation in one process:
  t2mi        dvbs2gpu_t2mi_process_batch with an output buffer per stream: the BBFRAMEs are delivered;
  t2mi_rows   the same call without output buffers: rows and counters only (a bank of its own);
  monitor     dvbs2gpu_tsmon_process_batch without output buffers on the same buffers (the header scan's scale);
  bbts        dvbs2gpu_bbts_process_batch on 8 frames of 7274 bytes per stream, the same byte count (the yardstick: a packetiser
              that reads the bytes and writes about as many).
Each time is a host clock around one synchronous call (argument upload and read-back included), median of 2 x REPS calls after a
warm-up round.  Two sets of buffers alternate, so a call's input was last touched two calls ago (2 x 238 MB of TS: more than the
256 MB Infinity Cache holds); set 1 goes on where set 0 ended, so a T2-MI packet is carried from call to call.  Bytes are counted
from the shapes: the T2-MI bank reads every TS byte of the PID once for the CRC and the BBFRAME bytes once more for the copy, writes
the BBFRAME bytes, 6 bytes per packet, 52 bytes per row and a 64-byte call record per (stream, slot), four of which go to the host.
Writes one JSON object to --out (default profiles/t2mi_bench.json) and prints it."""
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
import t2mi_ref as T

HBM_MEASURED = 6.29e12          # bytes/s, a float4 copy on this part (the figure the other profiles are held against)
S = int(os.environ.get('STREAMS', '4096'))
REPS = int(os.environ.get('REPS', '10'))
NPK, PATTERNS = 309, 16
KBCH, F = 58192, 8
PID, PLP = 0x1000, 1
out_path = sys.argv[sys.argv.index('--out') + 1] if '--out' in sys.argv else os.path.join(ROOT, 'profiles', 't2mi_bench.json')


def feed(rng):
    """2 x 309 packets: a null packet in every 20th place, the T2-MI feed in the others"""
    z, count, pk = T.Packetiser(PID), int(rng.integers(256)), []
    n_t2 = 2 * NPK - len(range(0, 2 * NPK, 20))
    while sum(len(p) for p in pk) < (n_t2 + 1) * 184:
        count = (count + 1) & 255
        pk.append(T.bb_packet(count, PLP, bytes(rng.integers(0, 256, int(rng.integers(6500, 6900)), dtype=np.uint8)), frame_idx=count))
    t2 = z.lay(pk)[:n_t2]
    out = np.zeros((2 * NPK, 188), np.uint8)
    out[:, 0], out[:, 1], out[:, 2], out[:, 3] = 0x47, 0x1F, 0xFF, 0x10
    out[[i for i in range(2 * NPK) if i % 20]] = t2
    return out


pkg = g.load_package()
eng = pkg.Engine(0)
sel = torch.arange(S, device='cuda') % PATTERNS
feeds = [feed(np.random.default_rng(100 + p)) for p in range(PATTERNS)]
host = [np.stack([f[k * NPK:(k + 1) * NPK].reshape(-1) for f in feeds]) for k in range(2)]
ts = [torch.from_numpy(h).cuda()[sel].contiguous() for h in host]
frames = [torch.from_numpy(np.stack([B.bbframes_from_ts(f[k * (NPK - 2):k * (NPK - 2) + NPK + 2], KBCH, F).reshape(-1) for f in feeds])).cuda()[sel].contiguous()
          for k in range(2)]
cap = NPK * 188
bb_out = torch.zeros((S, cap), dtype=torch.uint8, device='cuda')
ts_out = torch.zeros((S, F * KBCH // 8 + 376), dtype=torch.uint8, device='cuda')
bank, rows_bank = pkg.T2miBank(eng, S, NPK, 64), pkg.T2miBank(eng, S, NPK, 64)
mon, bbts = pkg.TsMonitorBank(eng, S, NPK), pkg.BbTsParserBank(eng, S, KBCH, F)
for i in range(S):
    bank.set_watch(i, 0, PID, PLP), rows_bank.set_watch(i, 0, PID, PLP)


def ptrs(t):
    return (C.c_void_p * S)(*[t[i].data_ptr() for i in range(S)])


p_ts, p_fr, p_tso = [ptrs(t) for t in ts], [ptrs(t) for t in frames], ptrs(ts_out)
p_bb = (C.c_void_p * (4 * S))(*[bb_out[i // 4].data_ptr() if i % 4 == 0 else None for i in range(4 * S)])
nb = (C.c_int * S)(*[NPK * 188] * S)
cnt = (C.c_int * S)(*[F] * S)
ob, orows, onb = (C.c_int * (4 * S))(), (C.c_int * (4 * S))(), (C.c_int * S)()
lib, st = eng.lib, eng._stream()


def run(name, k):
    if name == 't2mi':
        eng._check(lib.dvbs2gpu_t2mi_process_batch(bank.h, p_ts[k], nb, p_bb, cap, ob, orows, st))
    elif name == 't2mi_rows':
        eng._check(lib.dvbs2gpu_t2mi_process_batch(rows_bank.h, p_ts[k], nb, None, 0, None, orows, st))
    elif name == 'monitor':
        eng._check(lib.dvbs2gpu_tsmon_process_batch(mon.h, p_ts[k], nb, None, 0, None, st))
    else:
        eng._check(lib.dvbs2gpu_bbts_process_batch(bbts.h, p_fr[k], cnt, p_tso, ts_out.shape[1], onb, st))


names = ('t2mi', 't2mi_rows', 'monitor', 'bbts')
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
m = T.T2mi()
m.set_watch(0, PID, PLP)
for r in range(REPS + 1):
    for k in range(2):
        want = m.process(host[k][5].reshape(-1, 188))[0]
assert bank.stats(5) == m.stats() and bank.row_table(5, 0) == m.table(0) and bank.frame_bytes(5, 0) == m.frame_bytes(0), (bank.stats(5), m.stats())
assert np.array_equal(bb_out[5, :want.size].cpu().numpy(), want) and m.stats()['bbframes_delivered'] > 10 * REPS and m.stats()['crc_errors'] == 0
per_two_calls = {k: v / (REPS + 1) for k, v in m.stats().items()}
packets, t2_packets = S * NPK, S * per_two_calls['packets'] / 2
delivered, rows = S * per_two_calls['bytes_delivered'] / 2, S * per_two_calls['t2mi_packets'] / 2
record = 64 * 4
bytes_moved = {'t2mi': packets * 64 + t2_packets * 188 + 2 * delivered + t2_packets * 6 * 2 + rows * 52 + S * record * 2,
               't2mi_rows': packets * 64 + t2_packets * 188 + t2_packets * 6 + rows * 52 + S * record * 2,
               'monitor': packets * 64 + packets + S * 48 * 2, 'bbts': 2 * S * F * KBCH // 8}
res = {'streams': S, 'packets_per_stream_call': NPK, 't2mi_ts_packets_per_stream_call': per_two_calls['packets'] / 2,
       't2mi_packets_per_stream_call': per_two_calls['t2mi_packets'] / 2, 'bbframe_bytes_per_stream_call': per_two_calls['bytes_delivered'] / 2,
       'ts_bytes_per_call': packets * 188, 'reps': REPS, 'call_record_bytes_per_stream': {'t2mi': record, 'monitor': 48},
       'timing': 'host clock around one synchronous call, argument upload and read-back included; median / min of 2 x reps calls',
       'hbm_bytes_per_s_reference': HBM_MEASURED}
for n in names:
    med = float(np.median(times[n]))
    res[n] = {'ms_per_call': round(med * 1e3, 3), 'min_ms': round(min(times[n]) * 1e3, 3), 'max_ms': round(max(times[n]) * 1e3, 3),
              'bytes_touched': int(bytes_moved[n]), 'GB_per_s': round(bytes_moved[n] / med / 1e9, 1), 'fraction_of_hbm': round(bytes_moved[n] / med / HBM_MEASURED, 4)}
for n in ('t2mi', 't2mi_rows'):
    res[n + '_over_bbts'] = round(res[n]['ms_per_call'] / res['bbts']['ms_per_call'], 3)
    res[n + '_over_monitor'] = round(res[n]['ms_per_call'] / res['monitor']['ms_per_call'], 3)
os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
with open(out_path, 'w') as f:
    json.dump(res, f, indent=1)
    f.write('\n')
print(json.dumps(res))
