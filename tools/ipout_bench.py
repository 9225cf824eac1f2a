#!/usr/bin/env python3
"""IP output bank timing: 4096 streams x 309 packets per call -- the TS of the headline step -- resident in HBM, each
stream a mux of four PIDs in random order.  Per round four library calls are timed, in the same run and one behind the other:
  mon     dvbs2gpu_tsmon_process_batch with a pass-all filter and an output buffer per stream: the nearest existing kernel that reads
          and writes every byte once (the yardstick);
  ipout   dvbs2gpu_ipout_process_batch, one pass-all RTP flow per stream, P = 7, IPv4, no flush: 309 = 44 x 7 + 1, so what a slot
          holds walks through 0 .. 6 from call to call;
  ipts    dvbs2gpu_ipts_process_batch on the views of that call's row tables: the call that reads the result back;
  ipout4  dvbs2gpu_ipout_process_batch of a second bank with four flows per stream, each one of the four PIDs.
Each time is a pair of device events around one synchronous call (argument upload and read-back included), median, min and max of REPS
calls after a warm-up round; the host clock around the same call is kept beside it.  The views are built between the calls, outside
the windows.  Bytes are counted from the shapes: the output bank reads every TS byte once (the scan's header dwords and the sum's
second pass over a packet come from cache lines the copy fetches), writes the datagram bytes, 24 bytes per row, 2 bytes per passing
packet twice (the index list) and a 40-byte call record per stream, which goes to the host.  Writes one JSON object to --out (default
profiles/ipout_bench.json) and prints it."""
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
import ipout_cases as K
import ipout_ref as R
import ipts_ref as I

HBM_MEASURED = 6.29e12          # bytes/s, a float4 copy on this part (the figure the other profiles are held against)
S = int(os.environ.get('STREAMS', '4096'))
REPS = int(os.environ.get('REPS', '20'))
NPK, PATTERNS, P = 309, 16, 7
PIDS = (0x100, 0x101, 0x102, 0x103)
out_path = sys.argv[sys.argv.index('--out') + 1] if '--out' in sys.argv else os.path.join(ROOT, 'profiles', 'ipout_bench.json')

pkg = g.load_package()
eng = pkg.Engine(0)
sel = torch.arange(S, device='cuda') % PATTERNS
host = np.stack([K.packets([PIDS[i] for i in np.random.default_rng(50 + p).integers(0, 4, NPK)], seed=p) for p in range(PATTERNS)])
ts = torch.from_numpy(host).cuda()[sel].contiguous()
one = K.flow(4, R.RTP_MODE, P, port=5004)
four = [K.flow(4, R.RTP_MODE, P, port=5010 + k, pid_mode=1, pids=(PIDS[k],)) for k in range(4)]
cap1, cap4 = (NPK + 6) // P * (40 + 188 * P) + 64, (NPK // 2) // P * (40 + 188 * P) + 2048
mon_out = torch.zeros((S, NPK * 188), dtype=torch.uint8, device='cuda')
ip_out = torch.zeros((S, cap1), dtype=torch.uint8, device='cuda')
ip4_out = torch.zeros((S * 4, cap4), dtype=torch.uint8, device='cuda')
ts_out = torch.zeros((S, (NPK + 6) * 188), dtype=torch.uint8, device='cuda')
mon, bank, bank4, back = pkg.TsMonitorBank(eng, S, NPK), pkg.IpOutBank(eng, S, NPK), pkg.IpOutBank(eng, S, NPK), pkg.IpTsBank(eng, S, 64)
for i in range(S):
    mon.set_filter(i, 0)
    bank.set_flow(i, 0, **one), bank.set_rate(i, K.RATE), bank4.set_rate(i, K.RATE)
    back.set_flow(i, 0, 4, one['dst'], one['dst_port'])
    for k in range(4):
        bank4.set_flow(i, k, **four[k])
p_ts = (C.c_void_p * S)(*[ts[i].data_ptr() for i in range(S)])
p_mon = (C.c_void_p * S)(*[mon_out[i].data_ptr() for i in range(S)])
slot0 = lambda t: (C.c_void_p * (4 * S))(*[t[i // 4].data_ptr() if i % 4 == 0 else None for i in range(4 * S)])
p_ip, p_back = slot0(ip_out), slot0(ts_out)
p_ip4 = (C.c_void_p * (4 * S))(*[ip4_out[i].data_ptr() for i in range(4 * S)])
nb = (C.c_int * S)(*[NPK * 188] * S)
mb, ob, orows, ob4, tb, trows = (C.c_int * S)(), (C.c_int * (4 * S))(), (C.c_int * (4 * S))(), (C.c_int * (4 * S))(), (C.c_int * (4 * S))(), (C.c_int * S)()
views = (pkg.IptsView * S)()
lib, st = eng.lib, eng._stream()
Row = pkg.IpoutRow
ip_ptr = [ip_out[i].data_ptr() for i in range(S)]


def build_views():
    p, n = C.c_void_p(), C.c_int()
    for i in range(S):
        eng._check(lib.dvbs2gpu_ipout_get_row_table_device(bank.h, i, 0, C.byref(p), C.byref(n)))
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


names = ('mon', 'ipout', 'ipts', 'ipout4')
times, clock = {n: [] for n in names}, {n: [] for n in names}
for r in range(REPS + 1):                                           # round 0 warms up
    got = {}
    got['mon'] = timed(lambda: eng._check(lib.dvbs2gpu_tsmon_process_batch(mon.h, p_ts, nb, p_mon, NPK * 188, mb, st)))
    got['ipout'] = timed(lambda: eng._check(lib.dvbs2gpu_ipout_process_batch(bank.h, p_ts, nb, p_ip, cap1, ob, orows, 0, st)))
    build_views()
    got['ipts'] = timed(lambda: eng._check(lib.dvbs2gpu_ipts_process_batch(back.h, views, p_back, ts_out.shape[1], tb, trows, st)))
    got['ipout4'] = timed(lambda: eng._check(lib.dvbs2gpu_ipout_process_batch(bank4.h, p_ts, nb, p_ip4, cap4, ob4, None, 0, st)))
    for n in names:
        if r:
            times[n].append(got[n][0]), clock[n].append(got[n][1])
# the device banks against the models on one stream: the same calls in the same order
m, m4, mb_ = R.Stream(), R.Stream(), I.Stream()
m.set_flow(0, **one), m.set_rate(K.RATE), m4.set_rate(K.RATE), mb_.set_flow(0, 4, one['dst'], one['dst_port'])
for k in range(4):
    m4.set_flow(k, **four[k])
for r in range(REPS + 1):
    want = m.process(host[5])[0]
    want4 = m4.process(host[5])
    ts_want = mb_.process(np.frombuffer(want, np.uint8), [(x['offset'], x['bytes']) for x in m.table[0]])[0]
assert bank.stats(5) == m.stats() and bank.row_table(5, 0) == m.table[0] and ip_out[5, :len(want)].cpu().numpy().tobytes() == want
assert bank4.stats(5) == m4.stats() and all(ip4_out[20 + k, :len(want4[k])].cpu().numpy().tobytes() == want4[k] for k in range(4))
assert back.stats(5) == mb_.stats() and back.row_table(5) == mb_.table and np.array_equal(ts_out[5, :ts_want.size].cpu().numpy(), ts_want)
assert mb_.stats()['lost'] == 0 and mb_.stats()['bad_checksum'] == 0 and mb_.stats()['late'] == 0 and mb_.stats()['ts'] == m.stats()['datagrams'] > 40 * REPS
per_call = {k: v / (REPS + 1) for k, v in m.stats().items()}
moved = S * (NPK * 188 + per_call['bytes_delivered'] + 24 * per_call['datagrams'] + 4 * NPK + 40 * 2)
res = {'streams': S, 'packets_per_stream_call': NPK, 'packets_per_datagram': P, 'datagrams_per_stream_call': per_call['datagrams'],
       'datagram_bytes_per_stream_call': per_call['bytes_delivered'], 'ts_bytes_per_call': S * NPK * 188, 'reps': REPS,
       'timing': 'device events around one synchronous call, argument upload and read-back included; median / min / max of reps calls; host_clock_ms: the host clock around the same calls',
       'hbm_bytes_per_s_reference': HBM_MEASURED}
for n in names:
    med = float(np.median(times[n]))
    res[n] = {'ms_per_call': round(med * 1e3, 3), 'min_ms': round(min(times[n]) * 1e3, 3), 'max_ms': round(max(times[n]) * 1e3, 3),
              'host_clock_ms': round(float(np.median(clock[n])) * 1e3, 3)}
res['ipout'].update(bytes_touched=int(moved), GB_per_s=round(moved / float(np.median(times['ipout'])) / 1e9, 1))
res['ipout_over_mon'] = round(res['ipout']['ms_per_call'] / res['mon']['ms_per_call'], 3)
res['ipout_over_ipts'] = round(res['ipout']['ms_per_call'] / res['ipts']['ms_per_call'], 3)
res['ipout4_over_ipout'] = round(res['ipout4']['ms_per_call'] / res['ipout']['ms_per_call'], 3)
os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
with open(out_path, 'w') as f:
    json.dump(res, f, indent=1)
    f.write('\n')
print(json.dumps(res))
