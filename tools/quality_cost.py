"""What the signal-quality estimate costs on the headline workload: N streams of 8PSK 3/4 normal frames, F frames per stream and step, the
throughput mode, the decoder at a forced iteration count (bench.py's 50 by default; 0: its trial limit), steps timed with quality off and on
(same handles, same input, the two settings alternated twice).  Prints one JSON line with the ms per step of each.
    python tools/quality_cost.py [--streams 4096] [--frames 8] [--steps 5] [--warmup 2] [--force-iters 50] [--esn0 11]"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import __graft_entry__ as g  # noqa: E402
import orc  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--streams', type=int, default=4096)
    ap.add_argument('--frames', type=int, default=8)
    ap.add_argument('--steps', type=int, default=5)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--force-iters', type=int, default=50)
    ap.add_argument('--esn0', type=float, default=11.0)
    a = ap.parse_args()
    pkg = g.load_package()
    eng = pkg.Engine(0)
    mp = orc.modcod_params(14, 0, 0)
    step = 2 * a.frames * mp['plframe']
    nsteps = a.warmup + a.steps
    iq, _, _ = orc.transmit(14, 0, 0, nframes=2 * a.frames * nsteps + 2, seed=1, esn0_db=a.esn0, cfo=2e-4, timing=0.2, phase0=0.3)
    iq_d = torch.from_numpy(iq).cuda()
    eng.set_pipelined(1)
    dms = [eng.demod(eng.default_cfg(14, False, False, force_ldpc_iters=a.force_iters), max_samples=step) for _ in range(a.streams)]
    outs = [torch.zeros((a.frames + 4) * mp['kbch'] // 8, dtype=torch.uint8, device='cuda') for _ in range(a.streams)]
    res = {}
    for on in (0, 1, 0, 1):
        for d in dms:
            d.set_quality(on)
        times = []
        for s in range(nsteps):
            k = s * step
            ins = [iq_d[k:k + step]] * a.streams
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            eng.process_batch(dms, ins, outs)
            torch.cuda.synchronize()
            times.append(time.perf_counter() - t0)
        res.setdefault('quality_on' if on else 'quality_off', []).append(1e3 * float(np.median(times[a.warmup:])))
    off, on = min(res['quality_off']), min(res['quality_on'])
    print(json.dumps({'streams': a.streams, 'frames_per_step': a.frames, 'force_iters': a.force_iters, 'esn0_db': a.esn0, 'ms_per_step_off': round(off, 2), 'ms_per_step_on': round(on, 2),
                      'extra_pct': round(100.0 * (on - off) / off, 2), 'runs': res}))
    eng.set_pipelined(0)


if __name__ == '__main__':
    main()
