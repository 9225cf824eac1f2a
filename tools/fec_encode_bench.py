"""What the FEC encoder and the channel-error count cost beside the decoder: F frames of rate 3/4 normal (the headline's code) and F of rate 8/9 short, random
BBFRAMEs made on the device, encoded, sent through an AWGN channel on the device (BPSK LLRs as tests/orc.py::bits_to_llr makes them), then per call and code
    fec_encode_batch (with its LLR output), fec_channel_ber_batch (on the decoder's LLRs, BBFRAMEs and corrections), fec_decode_batch (the headline's forced 50
    sweeps, and early exit with a limit of 25)
timed with device events: `--warmup` untimed calls, `--runs` timed ones, median and spread (min, max).  Also: the bytes each call has to move (encode: kbch / 8
read and N / 8 written per frame, N more with the LLR output; BER: N + kbch / 8 read) as a fraction of the 8 TB/s of HBM, and the ratio to the forced decode.
Prints one JSON line; --out also writes it to a file.
    python tools/fec_encode_bench.py [--frames 32768] [--runs 5] [--warmup 1] [--snr-db 6.0] [--snr-db-short 9.0] [--out profiles/fec_encode_bench.json]"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as g  # noqa: E402

HBM_BYTES_PER_S = 8e12


def timed(fn, warmup, runs):
    for _ in range(warmup):
        fn()
    ms = []
    for _ in range(runs):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b))
    return {'median_ms': round(float(np.median(ms)), 3), 'min_ms': round(min(ms), 3), 'max_ms': round(max(ms), 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--frames', type=int, default=32768)
    ap.add_argument('--runs', type=int, default=5)
    ap.add_argument('--warmup', type=int, default=1)
    ap.add_argument('--snr-db', type=float, default=6.0, help='1 / sigma^2 of the channel for the normal code')
    ap.add_argument('--snr-db-short', type=float, default=9.0, help='... for the short code (rate 8/9 does not decode at 6 dB)')
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    pkg = g.load_package()
    eng = pkg.Engine(0)
    F = a.frames
    res = {'frames': F, 'runs': a.runs, 'warmup': a.warmup, 'codes': []}
    for rate, short in ((6, False), (9, True)):
        fi = pkg.fec_info(rate, short)
        N, kb = fi['ldpc_n'], fi['kbch'] // 8
        gen = torch.Generator(device='cuda').manual_seed(100 + rate)
        bb = torch.randint(0, 256, (F, kb), dtype=torch.uint8, device='cuda', generator=gen)
        code = torch.empty((F, N // 8), dtype=torch.uint8, device='cuda')
        llr = torch.empty((F, N), dtype=torch.int8, device='cuda')
        eng.fec_encode(bb, rate, short, amplitude=1, out=code, llr=llr)
        # the channel: y = +-1 + sigma n, LLR = round(2 y / sigma^2) clipped (bits_to_llr with its default scale), a slice of frames at a time
        snr_db = a.snr_db_short if short else a.snr_db
        sigma = 10 ** (-snr_db / 20.0)
        for k in range(0, F, 1024):
            y = llr[k:k + 1024].float()
            y += sigma * torch.randn(y.shape, device='cuda', generator=gen)
            llr[k:k + 1024] = torch.clamp(torch.round(y * (2.0 / (sigma * sigma))), -127, 127).to(torch.int8)
        clean = torch.empty_like(llr)
        out = torch.empty((F, kb), dtype=torch.uint8, device='cuda')
        trials = torch.empty(F, dtype=torch.int32, device='cuda')
        corr = torch.empty(F, dtype=torch.int32, device='cuda')
        r = {'rate': rate, 'short': int(short), 'snr_db': snr_db}
        r['fec_decode_forced_50'] = timed(lambda: eng.fec_decode(llr, rate, short, max_trials=50, force=True, out=out, trials=trials, corr=corr), a.warmup, a.runs)
        r['fec_decode_limit_25'] = timed(lambda: eng.fec_decode(llr, rate, short, max_trials=25, out=out, trials=trials, corr=corr), a.warmup, a.runs)
        r['frames_equal_to_sent'] = int((out == bb).all(dim=1).sum())
        r['fec_encode'] = timed(lambda: eng.fec_encode(bb, rate, short, out=code), a.warmup, a.runs)
        r['fec_encode_with_llr'] = timed(lambda: eng.fec_encode(bb, rate, short, amplitude=20, out=code, llr=clean), a.warmup, a.runs)
        ber = []
        r['fec_channel_ber'] = timed(lambda: ber.append(eng.channel_ber(llr, out, rate, short, corrections=corr)), a.warmup, a.runs)
        err, cnt = ber[-1]
        ok = err >= 0
        r['channel_ber'] = float(err[ok].sum()) / max(float(cnt[ok].sum()), 1.0)
        r['frames_without_ber'] = int((~ok).sum())
        moved = {'fec_encode': F * (kb + N // 8), 'fec_encode_with_llr': F * (kb + N // 8 + N), 'fec_channel_ber': F * (N + kb)}
        for k, nbytes in moved.items():
            r[k]['bytes_moved'] = nbytes
            r[k]['fraction_of_hbm_peak'] = round(nbytes / (r[k]['median_ms'] * 1e-3) / HBM_BYTES_PER_S, 4)
            r[k]['ratio_to_forced_decode'] = round(r[k]['median_ms'] / r['fec_decode_forced_50']['median_ms'], 4)
            r[k]['ratio_to_decode_limit_25'] = round(r[k]['median_ms'] / r['fec_decode_limit_25']['median_ms'], 4)
        res['codes'].append(r)
        del bb, code, llr, clean, out
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
