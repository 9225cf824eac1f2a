#!/usr/bin/env python3
"""Audio bank timing: 4096 streams x 309 packets per call -- the TS of the headline step -- resident in HBM, every
packet on one of four watched audio PIDs (MPEG-1 layer II at 192 kbit/s, ADTS frames of 250 to 400 bytes, AC-3 at 192 kbit/s and
E-AC-3 frames of 768 bytes, built by tests/aud_cases.py with filler full of false sync words).  Four calls are timed in alternation in
one process:
  aud_aligned    dvbs2gpu_aud_process_batch on a PES-aligned feed: every PES packet holds whole frames (3 to 5 TS packets each), so
                 every start acquires or continues the chain and the speculative walks hold;
  aud_unaligned  the same frames in PES packets of 1000 payload bytes, cut anywhere: the first start of a call acquires, every other
                 one finds the chain inside a frame, and one lane per PID walks the call's frames one after the other;
  es             dvbs2gpu_es_process_batch on the aligned buffers, the four PIDs watched as H.264 (existing code: every payload byte
                 is scanned for start codes);
  pes            dvbs2gpu_pes_process_batch on the aligned buffers (existing code: headers only).
Each time is a host clock around one synchronous call (argument upload and read-back included), median of 2 x REPS calls after a
warm-up round.  Two sets of buffers alternate per feed, so a call's input was last touched several calls ago (4 x 238 MB of TS: more
than the 256 MB Infinity Cache holds).  Bytes are counted from the shapes: the audio bank reads every packet's header and the bytes
of the frame headers, but a 188-byte packet is two or three cache lines, so the packets count whole; a 48-byte row per row and the
call record of a stream (1296 bytes) written and copied to the host.  ONLY=aud_aligned (...) times one of them alone, for a kernel
trace.  Writes one JSON object to --out (default profiles/aud_bench.json) and prints it."""
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
import aud_cases as K
import aud_ref as A
import pes_ref as P

HBM_MEASURED = 6.29e12          # bytes/s, a float4 copy on this part (the figure the other profiles are held against)
HBM_NOMINAL = 8e12
S = int(os.environ.get('STREAMS', '4096'))
REPS = int(os.environ.get('REPS', '10'))
ONLY = os.environ.get('ONLY', '')
NPK, PATTERNS = 309, 16
out_path = sys.argv[sys.argv.index('--out') + 1] if '--out' in sys.argv else os.path.join(ROOT, 'profiles', 'aud_bench.json')
WATCHES = [(0x200, A.MPA), (0x201, A.ADTS), (0x202, A.AC3), (0x203, A.AC3)]
RECORD = {'aud': 1296, 'es': 1680, 'pes': 1552}


def frames_of(rng, j, nbytes):
    out, n = [], 0
    while n < nbytes:
        f = (K.mpa_frame(rng, bri=10, sri=1, pad=0) if j == 0 else K.adts_frame(rng, int(rng.integers(250, 400))) if j == 1 else
             K.ac3_frame(rng, fscod=0, frmsizecod=20) if j == 2 else K.eac3_frame(rng, frmsiz=383))
        out.append(f)
        n += len(f)
    return out


def mux(rng, k, aligned):
    """buffer set k of one pattern: 309 packets, the four PIDs in turn; on each, PES packets of whole frames (aligned) or of 1000 bytes
    of the frames' bytes, the first of which begins with a frame (unaligned)"""
    out = P.null_packets(NPK)
    for j, (pid, codec) in enumerate(WATCHES):
        slots = list(range(j, NPK, len(WATCHES)))
        fr = frames_of(rng, j, len(slots) * 184)
        ln = K.Line(pid, cc=8 * k, pts=90000 + k * 3600 * 40)         # (77 or 78 packets per PID: a set never continues the other's counter, so a
                                                                      # call begins with a reset and its first start, which begins with a frame, acquires)
        if aligned:
            per, at = max(1, 900 // len(fr[0])), 0
            while len(ln.out) < len(slots):
                ln.pes(b''.join(fr[at:at + per]))
                at += per
        else:
            es, at = b''.join(fr), 0
            while len(ln.out) < len(slots):
                ln.pes(es[at:at + 1000])
                at += 1000
        out[slots] = ln.take()[:len(slots)]
    return out.reshape(-1)


pkg = g.load_package()
eng = pkg.Engine(0)
sel = torch.arange(S, device='cuda') % PATTERNS
FEEDS = ('aligned', 'unaligned')
host = {f: [np.stack([mux(np.random.default_rng(100 * k + p), k, f == 'aligned') for p in range(PATTERNS)]) for k in range(2)] for f in FEEDS}
ts = {f: [torch.from_numpy(h).cuda()[sel].contiguous() for h in host[f]] for f in FEEDS}
aud = {f: pkg.AudBank(eng, S, NPK, 256) for f in FEEDS}
es, pes = pkg.EsBank(eng, S, NPK, 256), pkg.PesBank(eng, S, NPK, 128)
for i in range(S):
    for slot, (pid, codec) in enumerate(WATCHES):
        aud['aligned'].set_watch(i, slot, pid, codec), aud['unaligned'].set_watch(i, slot, pid, codec), es.set_watch(i, slot, pid, pkg.EsBank.H264), pes.set_watch(i, slot, pid)


def ptrs(t):
    return (C.c_void_p * S)(*[t[i].data_ptr() for i in range(S)])


p_ts = {f: [ptrs(t) for t in ts[f]] for f in FEEDS}
nb = (C.c_int * S)(*[NPK * 188] * S)
orows = {n: (C.c_int * S)() for n in ('aud_aligned', 'aud_unaligned', 'es')}
lib, st = eng.lib, eng._stream()


def run(name, k):
    if name.startswith('aud_'):
        eng._check(lib.dvbs2gpu_aud_process_batch(aud[name[4:]].h, p_ts[name[4:]][k], nb, orows[name], st))
    elif name == 'es':
        eng._check(lib.dvbs2gpu_es_process_batch(es.h, p_ts['aligned'][k], nb, orows['es'], st))
    else:
        eng._check(lib.dvbs2gpu_pes_process_batch(pes.h, p_ts['aligned'][k], nb, None, st))


ALL = ('aud_aligned', 'aud_unaligned', 'es', 'pes')
names = tuple(n for n in ALL if not ONLY or n == ONLY)
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
rows = {n: 0 for n in ALL}
for f in FEEDS:
    if 'aud_' + f not in names:
        continue
    # the device bank against the model on one stream: the same calls in the same order
    m = K.model(256, [(slot, pid, codec) for slot, (pid, codec) in enumerate(WATCHES)])
    for r in range(REPS + 1):
        for k in range(2):
            m.process(host[f][k][5].reshape(-1, 188))
    bank = aud[f]
    assert bank.stats(5) == m.stats() and bank.rows(5) == m.table and bank.stream_stats(5) == m.stream_stats() and m.stats()['frames'] > 0, (bank.stats(5), m.stats())
    calls = 2 * (REPS + 1)
    rows['aud_' + f] = int(orows['aud_' + f][5])
    res['feed_' + f] = {'rows_per_stream_call': rows['aud_' + f], 'frames_per_stream_call': m.stats()['frames'] // calls, 'pes_starts_per_stream_call': m.stats()['pes_starts'] // calls,
                        'acquisitions_per_stream_call': m.stats()['acquisitions'] / calls, 'unaligned_starts_per_stream_call': m.stats()['unaligned_starts'] / calls,
                        'sync_losses': m.stats()['sync_losses']}
if 'es' in names:
    rows['es'] = int(orows['es'][5])
bytes_moved = {n: packets * 188 + S * rows[n] * 48 + S * RECORD['aud'] * 2 for n in ('aud_aligned', 'aud_unaligned')}
bytes_moved.update(es=packets * 188 + S * rows['es'] * 48 + S * RECORD['es'] * 2, pes=packets * 64 + S * RECORD['pes'] * 2)
for n in names:
    med = float(np.median(times[n]))
    res[n] = {'ms_per_call': round(med * 1e3, 3), 'min_ms': round(min(times[n]) * 1e3, 3), 'max_ms': round(max(times[n]) * 1e3, 3),
              'bytes_touched': int(bytes_moved[n]), 'GB_per_s': round(bytes_moved[n] / med / 1e9, 1), 'fraction_of_hbm': round(bytes_moved[n] / med / HBM_MEASURED, 4),
              'fraction_of_nominal_8TBps': round(bytes_moved[n] / med / HBM_NOMINAL, 4)}
if len(names) == len(ALL):
    res['aud_aligned_over_es'] = round(res['aud_aligned']['ms_per_call'] / res['es']['ms_per_call'], 3)
    res['aud_aligned_over_pes'] = round(res['aud_aligned']['ms_per_call'] / res['pes']['ms_per_call'], 3)
    res['aud_unaligned_over_aligned'] = round(res['aud_unaligned']['ms_per_call'] / res['aud_aligned']['ms_per_call'], 3)
    res['aud_unaligned_over_es'] = round(res['aud_unaligned']['ms_per_call'] / res['es']['ms_per_call'], 3)
    res['ts_read_once_ms_at_8TBps'] = round(packets * 188 / HBM_NOMINAL * 1e3, 4)
if not ONLY:
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, 'w') as f:
        json.dump(res, f, indent=1)
        f.write('\n')
print(json.dumps(res))
