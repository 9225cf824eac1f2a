#!/usr/bin/env python3
"""ULE bank timing: 4096 streams x 309 packets per call -- the TS of the headline step -- resident in HBM, each
stream a ULE feed: one PID carries 95 % of the packets as SNDUs with UDP/IPv4 datagrams of 1300 to 1472 bytes to one NPA address
(D = 0) watched by one slot, the rest are null packets.  Four calls are timed in alternation in one process:
  ule         dvbs2gpu_ule_process_batch with an output buffer per stream: the datagrams are delivered;
  ule_rows    the same call without output buffers: rows and counters only (a bank of its own);
  mpe         dvbs2gpu_mpe_process_batch with an output buffer per stream on an MPE feed of the same datagrams, cut to the same byte
              count (tools/mpe_bench.py's feed): the bank that shares phases A to C and the commit's shape with this one, the yardstick;
  monitor     dvbs2gpu_tsmon_process_batch without output buffers on the ULE buffers (the header scan's scale).
Each time is a host clock around one synchronous call (argument upload and read-back included), median of 2 x REPS = 20 calls after
a warm-up round; min and max are the run-to-run spread that the ule / mpe ratio is held against.  Two sets of buffers alternate, so a
call's input was last touched several calls ago; set 1 goes on where set 0 ended, so an SNDU is carried from call to call.  Bytes
are counted from the shapes: the ULE bank reads 64 bytes of every packet for the header, every TS byte of the PID once for the CRC
and the datagram bytes once more for the copy, writes the datagram bytes, 6 bytes per packet (read again by the commit kernel), 64
bytes per row and an 88-byte call record per (stream, slot), four of which go to the host.  ONLY=<name> runs one call alone, for a
kernel trace.  Writes one JSON object to --out (default profiles/ule_bench.json) and prints it."""
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
import mpe_ref as P
import ule_ref as R

HBM_MEASURED = 6.29e12          # bytes/s, a float4 copy on this part (the figure the other profiles are held against)
S = int(os.environ.get('STREAMS', '4096'))
REPS = int(os.environ.get('REPS', '10'))
NPK, PATTERNS = 309, 16
PID = 0x1000
NPA = bytes.fromhex('01005e000105')
out_path = sys.argv[sys.argv.index('--out') + 1] if '--out' in sys.argv else os.path.join(ROOT, 'profiles', 'ule_bench.json')


def with_nulls(pid_packets):
    """2 x 309 packets: a null packet in every 20th place, the PID's packets in the others"""
    out = np.zeros((2 * NPK, 188), np.uint8)
    out[:, 0], out[:, 1], out[:, 2], out[:, 3] = 0x47, 0x1F, 0xFF, 0x10
    out[[i for i in range(2 * NPK) if i % 20]] = pid_packets
    return out


N_PID = 2 * NPK - len(range(0, 2 * NPK, 20))


def datagrams(rng):
    out = []
    while sum(len(d) + 16 for d in out) < (N_PID + 1) * 184:
        n = int(rng.integers(1300, 1473))
        out.append(P.ipv4(P.udp(int(rng.integers(1024, 65536)), 5004, bytes(rng.integers(0, 256, n - 28, dtype=np.uint8)))))
    return out


def ule_feed(dgrams):
    return with_nulls(R.Packetiser(PID).lay([R.sndu(0x0800, d, npa=NPA) for d in dgrams])[:N_PID])


def mpe_feed(dgrams):
    return with_nulls(P.Packetiser(PID).lay([P.section(d, mac=NPA) for d in dgrams])[:N_PID])


pkg = g.load_package()
eng = pkg.Engine(0)
sel = torch.arange(S, device='cuda') % PATTERNS


def resident(feeds):
    host = [np.stack([f[k * NPK:(k + 1) * NPK].reshape(-1) for f in feeds]) for k in range(2)]
    return host, [torch.from_numpy(h).cuda()[sel].contiguous() for h in host]


sent = [datagrams(np.random.default_rng(100 + p)) for p in range(PATTERNS)]
host, ts = resident([ule_feed(d) for d in sent])
host_mpe, ts_mpe = resident([mpe_feed(d) for d in sent])
cap = NPK * 188
ip_out = torch.zeros((S, cap), dtype=torch.uint8, device='cuda')
mpe_out = torch.zeros((S, cap), dtype=torch.uint8, device='cuda')
bank, rows_bank, mpe = pkg.UleBank(eng, S, NPK, 64), pkg.UleBank(eng, S, NPK, 64), pkg.MpeBank(eng, S, NPK, 64)
mon = pkg.TsMonitorBank(eng, S, NPK)
for i in range(S):
    bank.set_watch(i, 0, PID, NPA, b'\xff' * 6), rows_bank.set_watch(i, 0, PID, NPA, b'\xff' * 6), mpe.set_watch(i, 0, PID, NPA, b'\xff' * 6)


def ptrs(t):
    return (C.c_void_p * S)(*[t[i].data_ptr() for i in range(S)])


def slot0(t):
    return (C.c_void_p * (4 * S))(*[t[i // 4].data_ptr() if i % 4 == 0 else None for i in range(4 * S)])


p_ts, p_mpe = [ptrs(t) for t in ts], [ptrs(t) for t in ts_mpe]
p_ip, p_mo = slot0(ip_out), slot0(mpe_out)
nb = (C.c_int * S)(*[NPK * 188] * S)
ob, orows = (C.c_int * (4 * S))(), (C.c_int * (4 * S))()
lib, st = eng.lib, eng._stream()


def run(name, k):
    if name == 'ule':
        eng._check(lib.dvbs2gpu_ule_process_batch(bank.h, p_ts[k], nb, p_ip, cap, ob, orows, st))
    elif name == 'ule_rows':
        eng._check(lib.dvbs2gpu_ule_process_batch(rows_bank.h, p_ts[k], nb, None, 0, None, orows, st))
    elif name == 'monitor':
        eng._check(lib.dvbs2gpu_tsmon_process_batch(mon.h, p_ts[k], nb, None, 0, None, st))
    else:
        eng._check(lib.dvbs2gpu_mpe_process_batch(mpe.h, p_mpe[k], nb, p_mo, cap, ob, orows, st))


names = ('ule', 'ule_rows', 'mpe', 'monitor')
only = os.environ.get('ONLY')                                      # one call alone, for a kernel trace
times = {n: [] for n in names}
for r in range(REPS + 1):                                           # round 0 warms up
    for name in names if not only else (only,):
        for k in range(2):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            run(name, k)
            torch.cuda.synchronize()
            if r:
                times[name].append(time.perf_counter() - t0)
if only:
    print(json.dumps({only: {'ms_per_call': round(float(np.median(times[only])) * 1e3, 3)}}))
    sys.exit(0)
# the device banks against the models on one stream: the same calls in the same order
m, mm = R.Ule(), P.Mpe()
m.set_watch(0, PID, NPA, b'\xff' * 6), mm.set_watch(0, PID, NPA, b'\xff' * 6)
for r in range(REPS + 1):
    for k in range(2):
        want = m.process(host[k][5].reshape(-1, 188))[0]
        want_mpe = mm.process(host_mpe[k][5].reshape(-1, 188))[0]
assert bank.stats(5) == m.stats() and bank.row_table(5, 0) == m.table(0), (bank.stats(5), m.stats())
assert np.array_equal(ip_out[5, :want.size].cpu().numpy(), want) and m.stats()['datagrams_delivered'] > 70 * REPS and m.stats()['crc_errors'] == 0
assert mpe.stats(5) == mm.stats() and np.array_equal(mpe_out[5, :want_mpe.size].cpu().numpy(), want_mpe) and mm.stats()['crc_errors'] == 0
per_two_calls = {k: v / (REPS + 1) for k, v in m.stats().items()}
packets, pid_packets = S * NPK, S * per_two_calls['packets'] / 2
delivered, rows = S * per_two_calls['bytes_delivered'] / 2, S * per_two_calls['sndus'] / 2
record = 88 * 4
bytes_moved = {'ule': packets * 64 + pid_packets * 188 + 2 * delivered + pid_packets * 6 * 2 + rows * 64 + S * record * 2,
               'ule_rows': packets * 64 + pid_packets * 188 + pid_packets * 6 + rows * 64 + S * record * 2,
               'monitor': packets * 64 + packets + S * 48 * 2}
res = {'streams': S, 'packets_per_stream_call': NPK, 'ule_ts_packets_per_stream_call': per_two_calls['packets'] / 2,
       'sndus_per_stream_call': per_two_calls['sndus'] / 2, 'datagram_bytes_per_stream_call': per_two_calls['bytes_delivered'] / 2,
       'mpe_datagram_bytes_per_stream_call': mm.stats()['bytes_delivered'] / (REPS + 1) / 2,
       'ts_bytes_per_call': packets * 188, 'reps': REPS, 'call_record_bytes_per_stream': {'ule': record, 'mpe': 84 * 4, 'monitor': 48},
       'timing': 'host clock around one synchronous call, argument upload and read-back included; median / min / max of 2 x reps calls',
       'hbm_bytes_per_s_reference': HBM_MEASURED}
for n in names:
    med = float(np.median(times[n]))
    res[n] = {'ms_per_call': round(med * 1e3, 3), 'min_ms': round(min(times[n]) * 1e3, 3), 'max_ms': round(max(times[n]) * 1e3, 3)}
    if n in bytes_moved:
        res[n].update(bytes_touched=int(bytes_moved[n]), GB_per_s=round(bytes_moved[n] / med / 1e9, 1), fraction_of_hbm=round(bytes_moved[n] / med / HBM_MEASURED, 4))
for n in ('ule', 'ule_rows'):
    res[n + '_over_monitor'] = round(res[n]['ms_per_call'] / res['monitor']['ms_per_call'], 3)
    res[n + '_over_mpe'] = round(res[n]['ms_per_call'] / res['mpe']['ms_per_call'], 3)
res['ule_minus_mpe_ms'] = round(res['ule']['ms_per_call'] - res['mpe']['ms_per_call'], 3)
res['mpe_spread_ms'] = round(res['mpe']['max_ms'] - res['mpe']['min_ms'], 3)
os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
with open(out_path, 'w') as f:
    json.dump(res, f, indent=1)
    f.write('\n')
print(json.dumps(res))
