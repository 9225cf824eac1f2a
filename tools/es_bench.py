#!/usr/bin/env python3
"""ES bank timing: 4096 streams x 309 packets per call -- the TS of the headline step -- resident in HBM, every packet
on one of two watched video PIDs (H.264 and MPEG-2 elementary streams of tests/es_cases.py) whose PES packets start every 8 to 12
packets of the stream.  Three calls are timed in alternation in one process:
  es        dvbs2gpu_es_process_batch, both PIDs watched: every payload byte is read;
  pes       dvbs2gpu_pes_process_batch on the same buffers, both PIDs watched (existing code: headers only);
  monitor   dvbs2gpu_tsmon_process_batch with a pass-all filter and output buffers on the same buffers (existing code: every byte is
            read once and written once).
Each time is a host clock around one synchronous call (argument upload and read-back included), median of 2 x REPS calls after a
warm-up round.  Two sets of buffers alternate, so a call's input was last touched two calls ago (2 x 238 MB of TS: more than the
256 MB Infinity Cache holds).  Bytes are counted from the shapes: the ES bank reads every packet once (188 bytes), a 48-byte row per
row and the call record of a stream (1680 bytes) written and copied to the host; the compacting monitor reads and writes 188 bytes
per packet.  ONLY=es (pes, monitor) times one of them alone, for a kernel trace.  Writes one JSON object to --out (default
profiles/es_bench.json) and prints it."""
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
import es_cases as K
import es_ref as E
import pes_ref as P

HBM_MEASURED = 6.29e12          # bytes/s, a float4 copy on this part (the figure the other profiles are held against)
HBM_NOMINAL = 8e12
S = int(os.environ.get('STREAMS', '4096'))
REPS = int(os.environ.get('REPS', '10'))
ONLY = os.environ.get('ONLY', '')
NPK, PATTERNS = 309, 16
out_path = sys.argv[sys.argv.index('--out') + 1] if '--out' in sys.argv else os.path.join(ROOT, 'profiles', 'es_bench.json')
WATCHES = [(0x200, E.H264), (0x201, E.MPEG2)]
RECORD = {'es': 1680, 'pes': 1552, 'monitor': 48}


def pictures(rng, codec, nbytes):
    """an elementary stream of pictures of about a PES packet's size (1 to 3 slices of 150 to 700 bytes; the builders' default is far
    smaller: theirs is a test of rows, this one of bytes), a sequence header or SPS every sixth"""
    out, n = b'', 0
    while len(out) < nbytes:
        first, slices = n % 6 == 0, int(rng.integers(1, 4))
        if codec == E.MPEG2:
            out += K.mpeg2_picture(rng, 1 if first else 2 + n % 2, n & 1023, slices, seq=first, gop=first, size=(150, 700))
        else:
            out += K.h264_picture(rng, K.H264_I if first else (K.H264_P, K.H264_B)[n % 2], idr=first, slices=slices, sps=first, sei=n % 4 == 0, size=(150, 700))
        n += 1
    return out


def mux(rng, k):
    """buffer set k of one pattern: 309 packets, the two PIDs in turn, on each a PES packet of 4 to 6 full TS packets after the other (a
    start every 8 to 12 packets of the stream); the counters of set 1 go on where set 0 ended"""
    out = P.null_packets(NPK)
    for j, (pid, codec) in enumerate(WATCHES):
        slots = list(range(j, NPK, 2))                               # every second packet belongs to the PID
        es, at_es = pictures(rng, codec, len(slots) * 184), 0
        left, cc, pts = 0, (k * len(slots)) & 15, 90000 + k * 3600 * 40
        for at in slots:
            if left == 0:
                left, pts = int(rng.integers(4, 7)), pts + 3600
                hd = K.head(pts)
                out[at] = K.pkt(pid, cc, hd + es[at_es:at_es + 184 - len(hd)], pusi=1)
                at_es += 184 - len(hd)
            else:
                out[at] = K.pkt(pid, cc, es[at_es:at_es + 184])
                at_es += 184
            left, cc = left - 1, (cc + 1) & 15
    return out.reshape(-1)


pkg = g.load_package()
eng = pkg.Engine(0)
sel = torch.arange(S, device='cuda') % PATTERNS
host = [np.stack([mux(np.random.default_rng(100 * k + p), k) for p in range(PATTERNS)]) for k in range(2)]
ts = [torch.from_numpy(h).cuda()[sel].contiguous() for h in host]
passed = torch.zeros((S, NPK * 188), dtype=torch.uint8, device='cuda')
bank, pes, mon = pkg.EsBank(eng, S, NPK, 256), pkg.PesBank(eng, S, NPK, 128), pkg.TsMonitorBank(eng, S, NPK)
for i in range(S):
    for slot, (pid, codec) in enumerate(WATCHES):
        bank.set_watch(i, slot, pid, codec), pes.set_watch(i, slot, pid)


def ptrs(t):
    return (C.c_void_p * S)(*[t[i].data_ptr() for i in range(S)])


p_ts, p_out = [ptrs(t) for t in ts], ptrs(passed)
nb = (C.c_int * S)(*[NPK * 188] * S)
orows, onb = (C.c_int * S)(), (C.c_int * S)()
lib, st = eng.lib, eng._stream()


def run(name, k):
    if name == 'es':
        eng._check(lib.dvbs2gpu_es_process_batch(bank.h, p_ts[k], nb, orows, st))
    elif name == 'pes':
        eng._check(lib.dvbs2gpu_pes_process_batch(pes.h, p_ts[k], nb, None, st))
    else:
        eng._check(lib.dvbs2gpu_tsmon_process_batch(mon.h, p_ts[k], nb, p_out, NPK * 188, onb, st))


names = tuple(n for n in ('es', 'pes', 'monitor') if not ONLY or n == ONLY)
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
packets = S * NPK
res = {'streams': S, 'packets_per_stream_call': NPK, 'ts_bytes_per_call': packets * 188, 'reps': REPS, 'call_record_bytes_per_stream': RECORD,
       'timing': 'host clock around one synchronous call, argument upload and read-back included; median / min of 2 x reps calls',
       'hbm_bytes_per_s_reference': HBM_MEASURED, 'hbm_bytes_per_s_nominal': HBM_NOMINAL}
rows = 0
if 'es' in names:
    # the device bank against the model on one stream: the same calls in the same order
    m = E.Es(256)
    for slot, (pid, codec) in enumerate(WATCHES):
        m.set_watch(slot, pid, codec)
    for r in range(REPS + 1):
        for k in range(2):
            m.process(host[k][5].reshape(-1, 188))
    assert bank.stats(5) == m.stats() and bank.rows(5) == m.table and bank.stream_stats(5) == m.stream_stats() and m.stats()['pictures'] > 0, (bank.stats(5), m.stats())
    rows = int(orows[5])
    res.update(rows_per_stream_call=rows, pictures_per_stream=m.stats()['pictures'] // (2 * (REPS + 1)), codes_per_stream=m.stats()['codes'] // (2 * (REPS + 1)))
if 'monitor' in names:
    assert all(v == NPK * 188 for v in onb)
bytes_moved = {'es': packets * 188 + S * rows * 48 + S * RECORD['es'] * 2, 'pes': packets * 64 + S * RECORD['pes'] * 2, 'monitor': packets * 188 * 2 + S * 48 * 2}
for n in names:
    med = float(np.median(times[n]))
    res[n] = {'ms_per_call': round(med * 1e3, 3), 'min_ms': round(min(times[n]) * 1e3, 3), 'max_ms': round(max(times[n]) * 1e3, 3),
              'bytes_touched': int(bytes_moved[n]), 'GB_per_s': round(bytes_moved[n] / med / 1e9, 1), 'fraction_of_hbm': round(bytes_moved[n] / med / HBM_MEASURED, 4),
              'fraction_of_nominal_8TBps': round(bytes_moved[n] / med / HBM_NOMINAL, 4)}
if len(names) == 3:
    res['es_over_monitor'] = round(res['es']['ms_per_call'] / res['monitor']['ms_per_call'], 3)
    res['es_over_pes'] = round(res['es']['ms_per_call'] / res['pes']['ms_per_call'], 3)
    res['ts_read_once_ms_at_8TBps'] = round(packets * 188 / HBM_NOMINAL * 1e3, 4)
if not ONLY:
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, 'w') as f:
        json.dump(res, f, indent=1)
        f.write('\n')
print(json.dumps(res))
