"""GPU test of the four watched-PID banks side by side (csrc/watch_bank.h: the host half that pcr.hip, pes.hip, es.hip and aud.hip
share): one engine, the four device banks on the same buffers in HBM, each against its model and its host bank through two calls.
And the ES and the audio device bank, whose kernels share their front (csrc/es_stream.h), on the same PIDs of the same buffers."""
import numpy as np
import pytest

import aud_ref as A
import es_ref as E
import watch_cases as W

pytestmark = pytest.mark.gpu
NAMES = ('pcr', 'pes', 'es', 'aud')
MAX_PACKETS = 64
MAX_ROWS = {'pcr': 64, 'pes': 64, 'es': 8, 'aud': 64}       # the ES bank drops rows


def test_four_device_banks_on_the_same_buffers(pkg):
    import torch
    eng = pkg.Engine(0)
    mux = W.interleaved(np.random.default_rng(11), 2 * MAX_PACKETS + 2)
    # 3 streams: 64 packets a call, nothing, one packet a call
    calls = [[mux[:64], mux[:0], mux[128:129]], [mux[64:128], mux[:0], mux[129:130]]]
    cls = {'pcr': pkg.PcrBank, 'pes': pkg.PesBank, 'es': pkg.EsBank, 'aud': pkg.AudBank}
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


def test_es_and_audio_device_banks_agree_on_what_the_shared_front_decides(pkg):
    """3 streams of at most 300 packets a call (more than one packet per thread, more than one wave) through nine calls: the audio
    multiplex in calls of 300 packets, in calls of 37 (most threads without a packet), and nothing (the front's path without a
    watched packet)"""
    import torch
    eng = pkg.Engine(0)
    ts, pids = W.stream_feeds()['aud']
    es, aud = pkg.EsBank(eng, 3, 300, 4096), pkg.AudBank(eng, 3, 300, 4096)
    models = [(E.Es(4096), A.Aud(4096)) for _ in range(3)]
    for i in range(3):
        W.watch_same_pids(es, aud, pids, i), W.watch_same_pids(*models[i], pids)
    pes_rows = [0, 0, 0]
    for c in range(9):
        per_stream = [ts[300 * c:300 * (c + 1)], ts[37 * c:37 * (c + 1)], ts[:0]]
        bufs = [torch.from_numpy(np.ascontiguousarray(x).reshape(-1)).cuda() for x in per_stream]
        nbytes = [x.size for x in per_stream]
        got = es.process(bufs, nbytes=nbytes), aud.process(bufs, nbytes=nbytes)
        for i, x in enumerate(per_stream):
            assert (got[0][i], got[1][i]) == (models[i][0].process(x), models[i][1].process(x)), (c, i)
            W.SAME['es'](es, models[i][0], i), W.SAME['aud'](aud, models[i][1], i)
            pes_rows[i] += W.same_stream_front(es, aud, i)
    assert all(es.stream_stats(i)['rows_dropped'] == 0 and aud.stream_stats(i)['rows_dropped'] == 0 for i in range(3))
    assert all(es.stats(0)[k] > 0 for k in W.COMMON_COUNTERS), es.stats(0)
    assert pes_rows[0] == 300 and pes_rows[1] > 0 and pes_rows[2] == 0 and es.stats(2)['packets'] == 0
