#!/usr/bin/env python3
"""BBFRAME -> TS parser bank timing: S streams x F BBFRAMEs of 8PSK 3/4 normal frames (kbch 48408) per call,
frames resident in HBM.  Prints one JSON line: packets/s, frames/s, GB/s moved (read DFL/8 + write 188 per 188) against HBM.
--ma: the same frames through the mode-adaptation mode (CCM sizes, SIS, no ISSY / NPD: the same bytes in and out, so the two figures
compare like with like; MA_ISSY=2|3 and MA_NPD=1 in the environment add the fields, payload then from tests/ma_ref.py; MA_GSE=1 switches
GSE decapsulation on for these TS-only frames; MA_HEM=1 feeds DVB-T2 high-efficiency-mode frames of the same data-field size instead, from
tests/hem_ref.py, with dvbs2gpu_bbts_ma_set_t2_hem on: MA_NPD adds the DNP byte, MA_ISSY != 0 the ISSY field in the header).
--gse: well-formed GSE data fields instead (the transmitter of tests/test_gpu_gse.py: 45 % of the packets complete PDUs of 40-1500 bytes,
20 % START packets of PDUs cut into 2-5 fragments of 40-1400 bytes, the rest their continuations; 64 different streams repeated over the
bank), for 4096, 64 and 1 streams x 8 frames per call, the device path and the forced host path (dvbs2gpu_bbts_set_gse_path) timed in
alternation in one process; one JSON line per bank size.
--ma --gse: adds to each of those lines the mode-adaptation bank with GSE on (dvbs2gpu_bbts_ma_set_gse): the same packet mix as two
ISIs per stream (two independent packet sequences per pattern, their frames sent in turn, both selected), timed in the same
alternation; and the host bank (dvbs2gpu_bbts_create_host, one stream: its ms per call is for ONE stream's call)."""
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


def gse_bench():
    import ctypes as C
    import test_gpu_gse as T
    kbch, F, P = int(os.environ.get('KBCH', '48408')), 8, 64
    fb = kbch // 8
    pats = []
    for p in range(P):
        pk, _ = T.transmitter(np.random.default_rng(p), 4 * F * (fb - 10))
        fr = T.pack_frames(pk, kbch)[:4 * F]
        assert len(fr) == 4 * F
        pats.append(torch.from_numpy(fr).cuda())
    ma_pats = []
    for p in range(P if MA_GSE else 0):
        two = []
        for j, isi in enumerate((5, 200)):                      # half the frames per ISI, multistream headers
            pk, _ = T.transmitter(np.random.default_rng(1000 * (j + 1) + p), 2 * F * (fb - 10))
            fr = T.pack_frames(pk, kbch)[:2 * F].copy()
            assert len(fr) == 2 * F
            fr[:, 0] &= 0xDF
            fr[:, 1] = isi
            for f in fr:
                f[9] = B.crc8(f[:9])
            two.append(fr)
        ma_pats.append(torch.from_numpy(np.stack([two[f % 2][f // 2] for f in range(4 * F)])).cuda())
    cap = F * fb + 376 + 3 * 7000          # three open reassemblies of this traffic hold at most 5 x 1400 bytes each
    for S in [int(x) for x in os.environ.get('STREAMS', '4096,64,1').split(',')]:
        outs = torch.zeros((S, cap), dtype=torch.uint8, device='cuda')
        pout = (C.c_void_p * S)(*[outs[i].data_ptr() for i in range(S)])
        pin = [(C.c_void_p * S)(*[pats[i % P][k * F:(k + 1) * F].data_ptr() for i in range(S)]) for k in range(4)]
        cnt, nb = (C.c_int * S)(*[F] * S), (C.c_int * S)()
        banks = {}
        for name, mode in (('device', 0), ('host', 1)):
            banks[name] = pkg.BbTsParserBank(eng, S, kbch, F)
            banks[name].set_gse_path(mode)
        names = ('device', 'host') + (('ma',) if MA_GSE else ())
        if MA_GSE:
            banks['ma'] = pkg.BbTsParserBank(eng, S, kbch, F)
            banks['ma'].set_mode_adaptation(True)
            for i in range(S):
                banks['ma'].select_isi(i, (5, 200))
            banks['ma'].ma_set_gse(True)
            outs2 = torch.zeros((S, 2, cap), dtype=torch.uint8, device='cuda')
            pout2 = (C.c_void_p * (8 * S))(*[outs2[i // 8, i % 8].data_ptr() if i % 8 < 2 else None for i in range(8 * S)])
            pin2 = [(C.c_void_p * S)(*[ma_pats[i % P][k * F:(k + 1) * F].data_ptr() for i in range(S)]) for k in range(4)]
            nb2, need2 = (C.c_int * (8 * S))(), (C.c_int * (8 * S))()

        def run(name, k):
            if name == 'ma':
                eng._check(banks[name].lib.dvbs2gpu_bbts_process_ma_batch(banks[name].h, pin2[k], None, cnt, pout2, cap, nb2, need2, eng._stream()))
                return int(np.frombuffer(nb2, np.int32).sum())
            eng._check(banks[name].lib.dvbs2gpu_bbts_process_batch(banks[name].h, pin[k], cnt, pout, cap, nb, eng._stream()))
            return sum(nb)
        res = {k: [] for k in names}
        pdus = {}
        reps = int(os.environ.get('REPS', '5'))
        for r in range(reps + 1):                       # round 0 warms up (and allocates the device path's GSE storage)
            for name in names:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                tot = sum(run(name, k) for k in range(4))
                torch.cuda.synchronize()
                if r:
                    res[name].append(((time.perf_counter() - t0) / 4, tot / 4))
        line = {'mode': 'gse', 'streams': S, 'frames_per_call': F, 'kbch': kbch}
        for name in ('device', 'host'):
            st = [banks[name].gse_stats(i) for i in range(min(S, P))]
            per_call = sum(x['complete_pdus'] + x['reassembled_pdus'] for x in st) / len(st) * S / (4 * (reps + 1))
            dt = float(np.median([a for a, _ in res[name]]))
            line[name] = {'ms_per_call': round(dt * 1e3, 3), 'min_ms': round(min(a for a, _ in res[name]) * 1e3, 3), 'pdus_per_s': round(per_call / dt),
                          'GB_per_s_read_plus_write': round((S * F * fb + res[name][0][1]) / dt / 1e9, 2),
                          'host_fallback_calls': sum(x['host_fallback_calls'] for x in st)}
        line['host_over_device'] = round(line['host']['ms_per_call'] / line['device']['ms_per_call'], 1)
        if MA_GSE:
            st = [banks['ma'].ma_gse_stats(i, j) for i in range(min(S, P)) for j in range(2)]
            per_call = sum(x['complete_pdus'] + x['reassembled_pdus'] for x in st) / (len(st) / 2) * S / (4 * (reps + 1))
            dt = float(np.median([a for a, _ in res['ma']]))
            line['ma'] = {'ms_per_call': round(dt * 1e3, 3), 'min_ms': round(min(a for a, _ in res['ma']) * 1e3, 3), 'max_ms': round(max(a for a, _ in res['ma']) * 1e3, 3),
                          'pdus_per_s': round(per_call / dt), 'GB_per_s_read_plus_write': round((S * F * fb + res['ma'][0][1]) / dt / 1e9, 2),
                          'host_fallback_calls': sum(x['host_fallback_calls'] for x in st) // 2}
            line['device']['max_ms'] = round(max(a for a, _ in res['device']) * 1e3, 3)
            line['ma_over_device'] = round(line['ma']['ms_per_call'] / line['device']['ms_per_call'], 2)
            hb = pkg.BbTsParserBank.host(kbch, F)
            hb.set_mode_adaptation(True)
            hb.select_isi(0, (5, 200))
            hb.ma_set_gse(True)
            hcalls = [[f for f in ma_pats[0][k * F:(k + 1) * F].cpu().numpy()] for k in range(4)]
            ht = []
            for r in range(reps + 1):
                t0 = time.perf_counter()
                for k in range(4):
                    hb.ma_work(hcalls[k], cap=cap)
                ht.append((time.perf_counter() - t0) / 4)
            line['ma_host_bank_ms_per_stream_call'] = round(float(np.median(ht[1:])) * 1e3, 3)
        line['includes'] = 'host arg upload + sync per call'
        print(json.dumps(line), flush=True)


MA_GSE = '--ma' in sys.argv and '--gse' in sys.argv
if '--gse' in sys.argv:
    gse_bench()
    sys.exit(0)
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
MA, hem = '--ma' in sys.argv, False
if MA:
    issy, npd = int(os.environ.get('MA_ISSY', '0')), int(os.environ.get('MA_NPD', '0'))
    hem = os.environ.get('MA_HEM') == '1'
    if hem:
        import hem_ref as H
        ts = H.make_ts(nfr * D // 187 + 2, rng, null_runs=False)
        fr = torch.from_numpy(np.stack(H.frames_of_stream(H.slot_stream(ts, bool(npd)), H.slot_len(npd), [D], sis=True, issyi=issy > 0, npd=bool(npd),
                                                            frame_bytes=fb)[:nfr])).cuda()
        issy = 0
    elif issy or npd:
        import ma_ref as M
        ts = M.make_ts(nfr * D // 188 + 2, rng, null_runs=False)
        st, _ = M.slot_stream(ts, issy, bool(npd))
        fr = torch.from_numpy(np.stack([f for f, _ in M.frames_of_stream(st, M.slot_len(issy, npd), [KBCH], sis=True, issyi=issy > 0, npd=bool(npd))][:nfr])).cuda()
    bank.set_mode_adaptation(True, issy_bytes=issy)
    if os.environ.get('MA_GSE') == '1':             # the TS-only call of a bank that has GSE switched on (no GSE frame ever comes)
        bank.ma_set_gse(True)
    if hem:
        bank.ma_set_t2_hem(True)
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
print(json.dumps({'mode': ('mode adaptation, T2 HEM' if hem else 'mode adaptation') if MA else 'reference', 'streams': S, 'frames_per_call': F, 'kbch': KBCH, 'ms_per_call': round(dt * 1e3, 3),
                  'frames_per_s': round(S * F / dt), 'ts_packets_per_s': round(tot / 188 / (4 * reps) / dt),
                  'GB_per_s_read_plus_write': round((S * F * D + tot / (4 * reps)) / dt / 1e9, 1), 'includes': 'host arg upload + sync per call'}))
