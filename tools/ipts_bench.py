#!/usr/bin/env python3
"""IP-TS bank timing: 4096 streams x 309 packets per call -- the TS of the headline step -- resident in HBM, each
stream an MPE feed as in tools/mpe_bench.py (one PID carries 95 % of the packets, the rest are null packets) whose datagrams are
UDP/RTP to one multicast group and port with 7 inner TS packets each, 1356 bytes.  Per call two library calls are timed, in the same
run and one behind the other as a user chains them:
  mpe     dvbs2gpu_mpe_process_batch with an output buffer per stream: the call that produces the datagrams (the yardstick: it touches
          the same bytes once with a CRC);
  ipts    dvbs2gpu_ipts_process_batch on the views of that call's row tables, with an output buffer per stream: UDP checksum, RTP
          rules and the inner TS laid out.
Each time is a pair of device events around one synchronous call (argument upload and read-back included), median of 2 x REPS calls
after a warm-up round; the host clock around the same call is kept beside it.  The views (one table pointer and row count per stream,
read through dvbs2gpu_mpe_get_row_table_device) are built between the two calls, outside both windows.  Two sets of buffers alternate;
set 1 goes on where set 0 ended, in the MPE sections and in the RTP sequence numbers, and the IP-TS bank is reset before every pair so
that set 0 is not late behind set 1.  Bytes are counted from the shapes: the IP-TS bank reads 8 bytes of every input row and 128 of
its datagram's head, every UDP byte once for the checksum and the TS bytes once more for the copy, writes the TS bytes, 40 bytes per
row (read twice again) and a 272-byte call record per stream, which goes to the host.  Writes one JSON object to --out (default
profiles/ipts_bench.json) and prints it."""
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
import ipts_ref as I
import mpe_ref as R

HBM_MEASURED = 6.29e12          # bytes/s, a float4 copy on this part (the figure the other profiles are held against)
S = int(os.environ.get('STREAMS', '4096'))
REPS = int(os.environ.get('REPS', '10'))
NPK, PATTERNS, MAX_ROWS = 309, 16, 64
PID, PORT = 0x1000, 5004
MAC = bytes.fromhex('01005e000105')
out_path = sys.argv[sys.argv.index('--out') + 1] if '--out' in sys.argv else os.path.join(ROOT, 'profiles', 'ipts_bench.json')
N_PID = 2 * NPK - len(range(0, 2 * NPK, 20))


def feed(rng, seed):
    """2 x 309 packets: a null packet in every 20th place, the PID's packets in the others, sections of RTP datagrams in sequence"""
    secs, seq = [], int(rng.integers(0, 65536))
    while sum(len(s) for s in secs) < (N_PID + 1) * 184:
        seq = (seq + 1) & 0xFFFF
        secs.append(R.section(I.datagram(I.rtp(I.ts_packets(7, 0x100, 7 * len(secs), seed), seq=seq, timestamp=3003 * len(secs)), dport=PORT), mac=MAC))
    out = np.zeros((2 * NPK, 188), np.uint8)
    out[:, 0], out[:, 1], out[:, 2], out[:, 3] = 0x47, 0x1F, 0xFF, 0x10
    out[[i for i in range(2 * NPK) if i % 20]] = R.Packetiser(PID).lay(secs)[:N_PID]
    return out


pkg = g.load_package()
eng = pkg.Engine(0)
sel = torch.arange(S, device='cuda') % PATTERNS
feeds = [feed(np.random.default_rng(100 + p), p) for p in range(PATTERNS)]
host = [np.stack([f[k * NPK:(k + 1) * NPK].reshape(-1) for f in feeds]) for k in range(2)]
ts = [torch.from_numpy(h).cuda()[sel].contiguous() for h in host]
cap = NPK * 188
ip_out = torch.zeros((S, cap), dtype=torch.uint8, device='cuda')
ts_out = torch.zeros((S, cap), dtype=torch.uint8, device='cuda')
mpe, bank = pkg.MpeBank(eng, S, NPK, MAX_ROWS), pkg.IpTsBank(eng, S, MAX_ROWS)
for i in range(S):
    mpe.set_watch(i, 0, PID, MAC, b'\xff' * 6), bank.set_flow(i, 0, 4, I.V4_DST, PORT)
p_ts = [(C.c_void_p * S)(*[t[i].data_ptr() for i in range(S)]) for t in ts]
slot0 = lambda t: (C.c_void_p * (4 * S))(*[t[i // 4].data_ptr() if i % 4 == 0 else None for i in range(4 * S)])
p_ip, p_out = slot0(ip_out), slot0(ts_out)
nb = (C.c_int * S)(*[NPK * 188] * S)
ob, orows, tb, trows = (C.c_int * (4 * S))(), (C.c_int * (4 * S))(), (C.c_int * (4 * S))(), (C.c_int * S)()
views = (pkg.IptsView * S)()
lib, st = eng.lib, eng._stream()
Row = pkg.MpeRow
ip_ptr = [ip_out[i].data_ptr() for i in range(S)]


def build_views():
    p, n = C.c_void_p(), C.c_int()
    for i in range(S):
        eng._check(lib.dvbs2gpu_mpe_get_row_table_device(mpe.h, i, 0, C.byref(p), C.byref(n)))
        views[i] = pkg.IptsView(ip_ptr[i] if n.value else None, p.value, C.sizeof(Row), Row.offset.offset, Row.bytes.offset, 0, n.value, 0)


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e-3, time.perf_counter() - t0


times = {'mpe': [], 'ipts': []}
clock = {'mpe': [], 'ipts': []}
for r in range(REPS + 1):                                           # round 0 warms up
    bank.reset()
    for k in range(2):
        a = timed(lambda: eng._check(lib.dvbs2gpu_mpe_process_batch(mpe.h, p_ts[k], nb, p_ip, cap, ob, orows, st)))
        build_views()
        b = timed(lambda: eng._check(lib.dvbs2gpu_ipts_process_batch(bank.h, views, p_out, cap, tb, trows, st)))
        if r:
            times['mpe'].append(a[0]), times['ipts'].append(b[0]), clock['mpe'].append(a[1]), clock['ipts'].append(b[1])
# the device banks against the models on one stream: the same calls in the same order
m, m2 = R.Mpe(), I.Stream()
m.set_watch(0, PID, MAC, b'\xff' * 6), m2.set_flow(0, 4, I.V4_DST, PORT)
for r in range(REPS + 1):
    m2.reset()
    for k in range(2):
        ip_want = m.process(host[k][5].reshape(-1, 188))[0]
        ts_want = m2.process(ip_want, [(x['offset'], x['bytes']) for x in m.table(0)])[0]
assert mpe.stats(5) == m.stats() and bank.stats(5) == m2.stats() and bank.row_table(5) == m2.table, (bank.stats(5), m2.stats())
assert np.array_equal(ts_out[5, :ts_want.size].cpu().numpy(), ts_want) and m2.stats()['ts'] > 35 and m2.stats()['late'] == 0 and m2.stats()['bad_checksum'] == 0
per_call = {k: v / 2 for k, v in m2.stats().items()}
rows, udp, inner = S * per_call['rows'], S * per_call['ts'] * (1356 - 20), S * per_call['bytes_delivered']
moved = rows * (8 + 128 + 3 * 40) + udp + 2 * inner + S * 272 * 2
res = {'streams': S, 'packets_per_stream_call': NPK, 'rows_per_stream_call': per_call['rows'], 'ts_rows_per_stream_call': per_call['ts'],
       'inner_ts_bytes_per_stream_call': per_call['bytes_delivered'], 'ts_bytes_per_call': S * NPK * 188, 'reps': REPS,
       'timing': 'device events around one synchronous call, argument upload and read-back included; median / min of 2 x reps calls; host_clock_ms: the host clock around the same calls',
       'hbm_bytes_per_s_reference': HBM_MEASURED}
for n in ('mpe', 'ipts'):
    med = float(np.median(times[n]))
    res[n] = {'ms_per_call': round(med * 1e3, 3), 'min_ms': round(min(times[n]) * 1e3, 3), 'max_ms': round(max(times[n]) * 1e3, 3),
              'host_clock_ms': round(float(np.median(clock[n])) * 1e3, 3)}
res['ipts'].update(bytes_touched=int(moved), GB_per_s=round(moved / float(np.median(times['ipts'])) / 1e9, 1))
res['ipts_over_mpe'] = round(res['ipts']['ms_per_call'] / res['mpe']['ms_per_call'], 3)
os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
with open(out_path, 'w') as f:
    json.dump(res, f, indent=1)
    f.write('\n')
print(json.dumps(res))
