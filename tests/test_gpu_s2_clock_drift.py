"""The DVB-S2 front end under a sampling-clock error, bit for bit against the CPU oracle on every form of the bank.

The other chain tests sample at exactly 2 samples per symbol: the polyphase arm settles in the middle of the 128-arm bank, and what the
hand-written loops of csrc/s2_rx_kernels.hip do at its ends is hardly run.  The signals of s2_drift_cases.py walk the arm through the whole
bank and over both ends every few thousand symbols (one-sided derivative at arm 0 / 127, steps of 0 and 2 samples, the candidate window
pressed against 0 .. 127 and left when the arm moves), at several input levels, into the frequency clamp and the error clamp;
test_s2_drift_cpu.py shows on the oracle's event counters that they do.

Tolerance: none, as in test_gpu_s2chain.py -- taps 0..3, per-frame statistics (the floats as their bits), BBFRAME bytes and the NCO frequency
after every call are compared for equality; oracle and engine get the same calls."""
import numpy as np
import pytest
import s2_drift_cases as dc
from test_gpu_s2chain import same_bits

pytestmark = pytest.mark.gpu

# timing-recovery forms and slicings (context options): the candidate-table form, the resolver + producer form, the candidate form with its prediction skewed
# to the edge of the table (the fall-back is taken whenever the arm moves), one time slice, and the most (slices end in single steps, which have to
# reproduce a 0- or 2-sample step at a slice border)
ENGINES = [{'gardner_form': 4}, {'gardner_form': 2}, {'gardner_form': 4, 'gardner_cand_skew': 4}, {'gardner_form': 4, 'fe_slices': 1},
           {'gardner_form': 2, 'fe_slices': 32}]


def _opts_id(o):
    return ','.join('%s=%d' % kv for kv in o.items())


@pytest.fixture(scope='module', params=ENGINES, ids=_opts_id)
def drift_engine(request, pkg):
    import torch
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    eng = pkg.Engine(0, options=request.param)
    yield eng
    eng.close()


@pytest.fixture(scope='module', params=[2, 4], ids=['form2', 'form4'])
def form_engine(request, pkg):
    import torch
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    eng = pkg.Engine(0, options={'gardner_form': request.param})
    yield eng
    eng.close()


def _check_handle(rec, dm, got_bytes, where):
    """one call of one stream: the engine's handle against the oracle's record of the same call"""
    for t in range(4):
        assert same_bits(rec['taps'][t], dm.tap(t)), ('tap', t) + where
    assert [dc.stat_tuple(s, True) for s in dm.stats()] == rec['stats'], ('per-frame statistics',) + where
    assert np.array_equal(rec['bb'], got_bytes), ('BBFRAMEs',) + where
    assert dc._u32(dm.nco_freq()) == rec['nco'], ('NCO frequency',) + where


@pytest.mark.parametrize('case', dc.CASES, ids=[c['name'] for c in dc.CASES])
def test_single_stream_equals_oracle_call_by_call(drift_engine, case):
    iq = dc.signal(case)[0]
    run = dc.oracle_run(case)
    dm = drift_engine.demod(dc.engine_cfg(drift_engine, case), max_samples=max(case['call'], 4096))
    try:
        for k, rec in enumerate(run['calls']):
            g = dm.process(iq[rec['a']:rec['b']])
            _check_handle(rec, dm, dc.flat_bytes(g), (case['name'], 'call', k, 'samples', rec['b'] - rec['a']))
    finally:
        dm.close()
    assert run['symbols'] > 0 and sum(len(r['stats']) for r in run['calls']) >= 1         # (the comparison was not one of nothing; what the signal must show: test_s2_drift_cpu.py)


def _dev(x):
    """a device tensor of its own (the catalogue's arrays are shared and read-only)"""
    import torch
    return torch.from_numpy(np.array(x, np.complex64)).cuda()


def _batch_cuts(n, k, calls, odd):
    """`calls` calls of stream k, different from stream to stream; odd: the calls end at odd sample positions (between the two samples of a symbol), else at
    even ones (a call that is a slice of a device tensor then starts on the 16-byte grid, like the tensor)"""
    c = [0] + [(((n * (j + 1)) // calls - 2 * k) & ~1) + int(odd) for j in range(calls - 1)] + [n]
    assert all(b > a for a, b in zip(c[:-1], c[1:]))
    return c


def _batch(calls=4, frames=dc.BATCH_FRAMES, odd=True):
    cases = dc.batch_cases(frames)
    sigs = [dc.signal(c)[0] for c in cases]
    cuts = [_batch_cuts(x.size, k, calls, odd) for k, x in enumerate(sigs)]
    runs = [dc.oracle_run(c, cc) for c, cc in zip(cases, cuts)]
    return cases, sigs, cuts, runs


def test_nine_streams_of_different_drift_in_one_batch(form_engine):
    """process_batch over nine streams whose clocks differ (+-100 .. +-900 ppm and none) and whose inputs differ in length: the streams of one resolver wave
    yield different output counts per period and end at different times.  Every stream == the oracle's single-stream run of the same calls."""
    import torch
    eng = form_engine
    cases, sigs, cuts, runs = _batch()
    S, calls = len(cases), len(cuts[0]) - 1
    dms = [eng.demod(dc.engine_cfg(eng, c), max_samples=max(np.diff(cc))) for c, cc in zip(cases, cuts)]
    kb = dms[0].info['kbch'] // 8
    tout = [torch.zeros(14 * kb, dtype=torch.uint8, device='cuda') for _ in range(S)]
    try:
        assert len({x.size for x in sigs}) >= 5
        frames = 0
        for c in range(calls):
            tin = [_dev(sigs[s][cuts[s][c]:cuts[s][c + 1]]) for s in range(S)]
            nb = eng.process_batch(dms, tin, tout)
            for s in range(S):
                _check_handle(runs[s]['calls'][c], dms[s], tout[s][:nb[s]].cpu().numpy(), (cases[s]['name'], 'call', c))
                frames += len(runs[s]['calls'][c]['stats'])
        assert frames >= sum(dc.BATCH_FRAMES) - 4 * S
    finally:
        for d in dms:
            d.close()


def test_nine_drifting_streams_pipelined_deliver_the_same_one_call_later(form_engine):
    """throughput mode: outputs and statistics come one call later and are the synchronous ones -- which the test above holds to the oracle's, so the oracle's
    record of call c is what call c + 1 must deliver; a zero-sample call collects the tail"""
    import torch
    eng = form_engine
    cases, sigs, cuts, runs = _batch()
    S, calls = len(cases), len(cuts[0]) - 1
    dms = [eng.demod(dc.engine_cfg(eng, c), max_samples=max(np.diff(cc))) for c, cc in zip(cases, cuts)]
    kb = dms[0].info['kbch'] // 8
    tout = [torch.zeros(14 * kb, dtype=torch.uint8, device='cuda') for _ in range(S)]
    eng.set_pipelined(True)
    try:
        for c in range(calls + 1):
            if c < calls:
                tin = [_dev(sigs[s][cuts[s][c]:cuts[s][c + 1]]) for s in range(S)]
            else:
                tin = [torch.empty(0, dtype=torch.complex64, device='cuda') for _ in range(S)]
            nb = eng.process_batch(dms, tin, tout)
            for s in range(S):
                got, st = tout[s][:nb[s]].cpu().numpy(), [dc.stat_tuple(x, True) for x in dms[s].stats()]
                if c == 0:
                    assert got.size == 0 and st == [], (cases[s]['name'], 'nothing can be ready in the first call')
                else:
                    rec = runs[s]['calls'][c - 1]
                    assert st == rec['stats'], ('per-frame statistics', cases[s]['name'], 'call', c)
                    assert np.array_equal(got, rec['bb']), ('BBFRAMEs', cases[s]['name'], 'call', c)
    finally:
        eng.set_pipelined(False)
        for d in dms:
            d.close()


def test_bank_of_264_drifting_streams_equals_oracle(engine):
    """above 256 streams the engine takes the resolver + producer form by itself and runs the multi-stream frame loops behind the PL sync instead of the speculative
    small-bank loops; 264 is no multiple of 16 (the last workgroup is partly filled).  The streams carry the nine signals (6 frames each) cyclically, from nine
    device tensors, in two calls; every stream == the oracle's run of its signal: taps, statistics, BBFRAMEs, NCO frequency."""
    import torch
    S = 264
    cases, sigs, cuts, runs = _batch(calls=2, frames=(6,) * 9, odd=False)
    D = len(cases)
    dev = [_dev(x) for x in sigs]
    dms = [engine.demod(dc.engine_cfg(engine, cases[s % D]), max_samples=max(np.diff(cuts[s % D]))) for s in range(S)]
    kb = dms[0].info['kbch'] // 8
    tout = [torch.zeros(8 * kb, dtype=torch.uint8, device='cuda') for _ in range(S)]
    try:
        frames = 0
        for c in range(2):
            nb = engine.process_batch(dms, [dev[s % D][cuts[s % D][c]:cuts[s % D][c + 1]] for s in range(S)], tout)
            for s in range(S):
                _check_handle(runs[s % D]['calls'][c], dms[s], tout[s][:nb[s]].cpu().numpy(), (cases[s % D]['name'], 'stream', s, 'call', c))
                frames += len(runs[s % D]['calls'][c]['stats'])
        assert frames >= S * 3
    finally:
        for d in dms:
            d.close()
