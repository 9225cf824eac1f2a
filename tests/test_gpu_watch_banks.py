"""GPU test of the three watched-PID banks side by side (csrc/watch_bank.h: the host half that pcr.hip, pes.hip and es.hip share): one
engine, the three device banks on the same buffers in HBM, each against its model and its host bank through two calls."""
import numpy as np
import pytest

import watch_cases as W

pytestmark = pytest.mark.gpu
NAMES = ('pcr', 'pes', 'es')
MAX_PACKETS = 64
MAX_ROWS = {'pcr': 64, 'pes': 64, 'es': 8}                  # the ES bank drops rows


def test_three_device_banks_on_the_same_buffers(pkg):
    import torch
    eng = pkg.Engine(0)
    mux = W.interleaved(np.random.default_rng(11), 2 * MAX_PACKETS + 2)
    # 3 streams: 64 packets a call, nothing, one packet a call
    calls = [[mux[:64], mux[:0], mux[128:129]], [mux[64:128], mux[:0], mux[129:130]]]
    cls = {'pcr': pkg.PcrBank, 'pes': pkg.PesBank, 'es': pkg.EsBank}
    dv = {n: cls[n](eng, 3, MAX_PACKETS, MAX_ROWS[n]) for n in NAMES}
    hb = {n: cls[n].host(3, MAX_PACKETS, MAX_ROWS[n]) for n in NAMES}
    models = {n: [W.model(n, MAX_ROWS[n]) for _ in range(3)] for n in NAMES}
    for n in NAMES:
        for i in range(3):
            W.watch(n, dv[n], i), W.watch(n, hb[n], i)
    for per_stream in calls:
        bufs = [torch.from_numpy(np.ascontiguousarray(ts).reshape(-1)).cuda() for ts in per_stream]
        nbytes = [ts.size for ts in per_stream]
        got = {n: dv[n].process(bufs, nbytes=nbytes) for n in NAMES}
        for n in NAMES:
            for i, ts in enumerate(per_stream):
                assert got[n][i] == models[n][i].process(ts) == hb[n].work(ts, stream=i), (n, i)
                W.SAME[n](dv[n], models[n][i], i), W.SAME[n](hb[n], models[n][i], i)
    assert dv['es'].stream_stats(0)['rows_dropped'] > 0 and dv['pcr'].stream_stats(0)['rows_dropped'] == 0
    # slot -1 on the stream with two active slots: the counters add up, the maxima stay maxima
    for n in NAMES:
        a, b = (dv[n].stats(0, s) for s in W.SLOTS[n])
        assert all(x['pcr_packets' if n == 'pcr' else 'packets'] > 0 for x in (a, b)), n
        for k in W.MAXIMA[n][:1]:
            assert a[k] > 0 and b[k] > 0 and a[k] != b[k], (n, k)
        assert dv[n].stats(0, -1) == {k: max(a[k], b[k]) if k in W.MAXIMA[n] else a[k] + b[k] for k in a}, n
