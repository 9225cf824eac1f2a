"""What the modulator costs: S streams x F frames of 8PSK 3/4 normal frames (the headline's MODCOD), random BBFRAMEs made on the device, then per call
    fec_encode, pl_frame, pulse_shape, channel (AWGN and a carrier offset) one by one on buffers of their own, and modulate (the same four in one call)
timed with device events: `--warmup` untimed calls, `--runs` timed ones, median and spread (min, max).  Beside each stage: the bytes it has to move (encode:
kbch / 8 read and N / 8 written per frame; framing: N / 8 read and 8 bytes per symbol written; shaping: 8 bytes per symbol read and 16 written; channel: 16 bytes
per symbol read and written) and the time those bytes take at the 8 TB/s of HBM.  Beside the total: the 0.13 s the CPU transmitter of the tests needs for one
stream's block, times S.  Prints one JSON line; --out also writes it to a file.
    python tools/s2_tx_bench.py [--streams 4096] [--frames 8] [--runs 5] [--warmup 1] [--out profiles/s2_tx_bench.json]"""
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
CPU_TRANSMITTER_S_PER_BLOCK = 0.13


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
    ap.add_argument('--streams', type=int, default=4096)
    ap.add_argument('--frames', type=int, default=8)
    ap.add_argument('--runs', type=int, default=5)
    ap.add_argument('--warmup', type=int, default=1)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    pkg = g.load_package()
    eng = pkg.Engine(0)
    S, F = a.streams, a.frames
    modcod, rate, short = 14, 6, False
    pls = [modcod << 2] * F
    sz = pkg.s2_tx_sizes(pls)
    fi = pkg.fec_info(rate, short)
    N, kb = fi['ldpc_n'], fi['kbch'] // 8
    nsym = sz['symbols']
    gen = torch.Generator(device='cuda').manual_seed(14)
    bb = torch.randint(0, 256, (F * S, kb), dtype=torch.uint8, device='cuda', generator=gen)       # frame-major: [frame][stream][kbch / 8]
    code = torch.empty((F * S, N // 8), dtype=torch.uint8, device='cuda')
    sym = torch.empty((S, nsym), dtype=torch.complex64, device='cuda')
    iq = torch.empty((S, 2 * nsym), dtype=torch.complex64, device='cuda')
    off = [f * S * (N // 8) for f in range(F)]
    stride = [N // 8] * F
    chan = dict(esn0_db=10.0, cfo=1e-3, phase0=0.0, seed=1)
    res = {'streams': S, 'frames_per_stream': F, 'modcod': modcod, 'symbols_per_stream': nsym, 'runs': a.runs, 'warmup': a.warmup, 'stages': {}}
    st = res['stages']
    st['fec_encode'] = timed(lambda: eng.fec_encode(bb, rate, short, out=code), a.warmup, a.runs)
    st['pl_frame'] = timed(lambda: eng.pl_frame(code.view(-1), pls, nstreams=S, code_off=off, code_stride=stride, out=sym), a.warmup, a.runs)
    st['pulse_shape'] = timed(lambda: eng.pulse_shape(sym, 0.35, 0.3, False, out=iq), a.warmup, a.runs)
    st['channel'] = timed(lambda: eng.channel(iq, **chan), a.warmup, a.runs)
    res['modulate'] = timed(lambda: eng.modulate(bb.view(-1), pls, S, rolloff=0.35, timing=0.3, out=iq, **chan), a.warmup, a.runs)
    moved = {'fec_encode': S * F * (kb + N // 8), 'pl_frame': S * (F * (N // 8) + 8 * nsym), 'pulse_shape': S * 24 * nsym, 'channel': S * 32 * nsym}
    for k, nbytes in moved.items():
        st[k]['bytes_moved'] = nbytes
        st[k]['ms_at_hbm_peak'] = round(nbytes / HBM_BYTES_PER_S * 1e3, 3)
        st[k]['fraction_of_hbm_peak'] = round(nbytes / (st[k]['median_ms'] * 1e-3) / HBM_BYTES_PER_S, 4)
    res['stages_sum_median_ms'] = round(sum(v['median_ms'] for v in st.values()), 3)
    res['modulate']['bytes_moved'] = sum(moved.values())
    res['modulate']['ms_at_hbm_peak'] = round(sum(moved.values()) / HBM_BYTES_PER_S * 1e3, 3)
    res['modulate']['msym_per_s'] = round(S * nsym / (res['modulate']['median_ms'] * 1e-3) / 1e6, 1)
    res['cpu_transmitter_s_per_block'] = CPU_TRANSMITTER_S_PER_BLOCK
    res['cpu_transmitter_s_for_all_streams'] = round(CPU_TRANSMITTER_S_PER_BLOCK * S, 1)
    res['speedup_over_cpu_transmitter'] = round(CPU_TRANSMITTER_S_PER_BLOCK * S / (res['modulate']['median_ms'] * 1e-3), 1)
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
