"""The DVB-S2 and DVB-S receivers off their default configuration, bit for bit against the CPU oracle.

Every other GPU test creates its handles with the plugin's configuration: 65 taps, roll-off 0.35, exactly 2 samples per symbol, agc_rate 1e-4, the default
timing gains.  The catalogue of rx_cfg_cases.py walks what the C ABI accepts beyond it (csrc/rx_cfg_rules.h says what that is): roll-offs, tap counts 1 .. 129
(the decimator's even tail, no delay line at all, calls shorter than the delay line), rate ratios, AGC rates and input levels, timing gains up to the edge of the
rule in both signs, omega_rel_limit 0 and its maximum, wide and narrow carrier loops, and for DVB-S 1.5 .. 64 samples per symbol.  test_rx_cfg_cpu.py shows on
the oracle alone that each case is a comparison of something.  What the rule refuses is tested as a refusal, never run.

Tolerance: none, as in test_gpu_s2_clock_drift.py -- taps 0..3, per-frame statistics (the floats as their bits), BBFRAME bytes and the NCO frequency after every
call; for DVB-S the symbols, the 8 floats of loop state and the decoded bits.  Oracle and engine get the same calls."""
import numpy as np
import pytest
import s2_drift_cases as dc
import rx_cfg_cases as rc
from test_gpu_s2chain import same_bits

pytestmark = pytest.mark.gpu

S2_IDS = [c['name'] for c in rc.S2_CASES]
DVBS_IDS = [c['name'] for c in rc.DVBS_CASES]


def _need_gpu():
    import torch
    if not torch.cuda.is_available():
        pytest.skip('no GPU')


@pytest.fixture(scope='module', params=[2, 4], ids=['form2', 'form4'])
def form_engine(request, pkg):
    _need_gpu()
    eng = pkg.Engine(0, options={'gardner_form': request.param})
    yield eng
    eng.close()


@pytest.fixture(scope='module', params=[1, 3], ids=['bank_slices1', 'bank_slices3'])
def bank_engine(request, pkg):
    """the DVB-S bank kernels (several streams per wave) forced for small banks, as in test_dvbs_bank_kernels_equal_the_wave_per_stream_kernels"""
    _need_gpu()
    eng = pkg.Engine(0, options={'dvbs_bank_min': 1, 'dvbs_fe_slices': request.param})
    yield eng
    eng.close()


def _check_handle(rec, dm, got_bytes, where, taps=(0, 1, 2, 3)):
    """one call of one stream: the engine's handle against the oracle's record of the same call"""
    for t in taps:
        assert same_bits(rec['taps'][t], dm.tap(t)), ('tap', t) + where
    for t in set(range(4)) - set(taps):
        assert dm.tap(t).size == 0, ('tap', t, 'of a group whose scratch a later group of the batch has reused') + where
    assert [dc.stat_tuple(s, True) for s in dm.stats()] == rec['stats'], ('per-frame statistics',) + where
    assert np.array_equal(rec['bb'], got_bytes), ('BBFRAMEs',) + where
    assert dc._u32(dm.nco_freq()) == rec['nco'], ('NCO frequency',) + where


def _dev(x):
    import torch
    return torch.from_numpy(np.array(x, np.complex64)).cuda() if len(x) else torch.empty(0, dtype=torch.complex64, device='cuda')


# ---------------------------------------------------------------------------------------------------------------- DVB-S2, one stream
@pytest.mark.parametrize('plan', list(rc.S2_PLANS))
@pytest.mark.parametrize('case', rc.S2_CASES, ids=S2_IDS)
def test_s2_single_stream_equals_oracle_call_by_call(form_engine, case, plan):
    iq = rc.s2_signal(case)[0]
    run = rc.s2_oracle_run(case, rc.s2_cuts(iq.size, plan))
    dm = form_engine.demod(rc.s2_engine_cfg(form_engine, case), max_samples=rc.S2_CALL)
    try:
        for k, rec in enumerate(run['calls']):
            g = dm.process(iq[rec['a']:rec['b']])
            _check_handle(rec, dm, dc.flat_bytes(g), (case['name'], plan, 'call', k, 'samples', rec['b'] - rec['a']))
    finally:
        dm.close()
    assert run['symbols'] > 100000 and sum(len(r['stats']) for r in run['calls']) >= 1


# ---------------------------------------------------------------------------------------------------------------- DVB-S2, all cases in one batch
def _batch_cuts(n, k, calls=4):
    """`calls` calls of stream k ending at odd sample positions (between the two samples of a symbol), different from stream to stream"""
    c = [0] + [(((n * (j + 1)) // calls - 2 * k) & ~1) + 1 for j in range(calls - 1)] + [n]
    assert all(b > a for a, b in zip(c[:-1], c[1:]))
    return c


def _batch(cases):
    sigs = [rc.s2_signal(c)[0] for c in cases]
    cuts = [_batch_cuts(x.size, k) for k, x in enumerate(sigs)]
    runs = [rc.s2_oracle_run(c, cc) for c, cc in zip(cases, cuts)]
    return sigs, cuts, runs


def _run_batch(eng, cases, pipelined=False):
    """the cases as the streams of one process_batch, four calls; every stream == its own single-stream oracle run (pipelined: one call later)"""
    import torch
    sigs, cuts, runs = _batch(cases)
    S, calls = len(cases), len(cuts[0]) - 1
    dms = [eng.demod(rc.s2_engine_cfg(eng, c), max_samples=max(np.diff(cc))) for c, cc in zip(cases, cuts)]
    kb = dms[0].info['kbch'] // 8
    tout = [torch.zeros(16 * kb, dtype=torch.uint8, device='cuda') for _ in range(S)]
    frames = 0
    if pipelined:
        eng.set_pipelined(True)
    try:
        for c in range(calls + int(pipelined)):
            tin = [_dev(sigs[s][cuts[s][c]:cuts[s][c + 1]] if c < calls else ()) for s in range(S)]
            nb = eng.process_batch(dms, tin, tout)
            for s in range(S):
                got = tout[s][:nb[s]].cpu().numpy()
                if not pipelined:
                    # (the groups run one after another in the context's per-call scratch: the PLL output and the LLRs behind taps 2 and 3 are the last group's;
                    #  the other handles report none -- they used to hand out whatever the last group had left there)
                    _check_handle(runs[s]['calls'][c], dms[s], got, (cases[s]['name'], 'call', c), taps=(0, 1, 2, 3) if s == S - 1 else (0, 1))
                    frames += len(runs[s]['calls'][c]['stats'])
                elif c == 0:
                    assert got.size == 0 and dms[s].stats() == [], (cases[s]['name'], 'nothing can be ready in the first call')
                else:
                    rec = runs[s]['calls'][c - 1]
                    assert [dc.stat_tuple(x, True) for x in dms[s].stats()] == rec['stats'], ('per-frame statistics', cases[s]['name'], 'call', c)
                    assert np.array_equal(got, rec['bb']), ('BBFRAMEs', cases[s]['name'], 'call', c)
                    frames += len(rec['stats'])
    finally:
        if pipelined:
            eng.set_pipelined(False)
        for d in dms:
            d.close()
    return frames


def test_s2_all_cases_as_the_streams_of_one_batch(form_engine):
    """every stream is a configuration group of its own and the groups differ in their front-end settings: neither one stage pipeline for all (process_mixed)
    nor a common front-end pre-pass takes the batch"""
    assert len({repr(sorted(c['cfg'].items())) for c in rc.S2_CASES}) == len(rc.S2_CASES)
    assert _run_batch(form_engine, rc.S2_CASES) >= 8 * len(rc.S2_CASES)


@pytest.mark.parametrize('slices', [1, 32])
def test_s2_all_cases_in_one_batch_time_sliced(pkg, slices):
    _need_gpu()
    eng = pkg.Engine(0, options={'fe_slices': slices})
    try:
        assert _run_batch(eng, rc.S2_CASES) >= 8 * len(rc.S2_CASES)
    finally:
        eng.close()


def test_s2_cases_in_one_batch_pipelined_deliver_the_same_one_call_later(engine):
    """throughput mode (at most 16 configuration groups per batch: the catalogue in parts): the synchronous frames and statistics -- which the tests above hold to
    the oracle's -- one call later, as test_pipelined_mixed_modcod_batch_equals_synchronous states it; a zero-sample call collects the tail"""
    for a in range(0, len(rc.S2_CASES), 16):
        part = rc.S2_CASES[a:a + 16]
        assert _run_batch(engine, part, pipelined=True) >= 8 * len(part)


# ---------------------------------------------------------------------------------------------------------------- the RRC tap cache
def _s2_first_calls(eng, names, ncalls=2):
    """handles of the named cases, used for the first time in this order (a context fetches a handle's taps with its first call); then every call of every handle
    against the oracle"""
    cases = [rc.S2_BY_NAME[n] for n in names]
    dms = [eng.demod(rc.s2_engine_cfg(eng, c), max_samples=rc.S2_CALL) for c in cases]
    try:
        for k in range(ncalls):
            for c, dm in zip(cases, dms):
                iq = rc.s2_signal(c)[0]
                rec = rc.s2_oracle_run(c, rc.s2_cuts(iq.size, 'whole'))['calls'][k]
                g = dm.process(iq[rec['a']:rec['b']])
                _check_handle(rec, dm, dc.flat_bytes(g), (c['name'], 'order', names, 'call', k))
    finally:
        for d in dms:
            d.close()


def _dvbs_single(pkg, eng, case, nstreams=1):
    iq = rc.dvbs_signal(case)
    calls = rc.dvbs_oracle_run(case)
    bank = pkg.DvbsDemodBank(eng, nstreams, max_samples=max(c['b'] - c['a'] for c in calls), **case['cfg'])
    try:
        _dvbs_compare(bank, [iq] * nstreams, [calls] * nstreams, case['name'])
    finally:
        bank.close()
    return sum(c['syms'].size for c in calls)


def _dvbs_compare(bank, iqs, runs, name):
    import torch
    S = len(iqs)
    for k in range(len(runs[0])):
        recs = [r[k] for r in runs]
        if S == 1:
            bits = [bank.process(iqs[0][recs[0]['a']:recs[0]['b']])]
        else:
            tin = [_dev(iqs[s][recs[s]['a']:recs[s]['b']]) for s in range(S)]
            tout = [torch.zeros(4 * 8192 + tin[s].numel(), dtype=torch.uint8, device='cuda') for s in range(S)]
            nb = bank.process_batch(tin, tout)
            bits = [tout[s][:nb[s]].cpu().numpy() for s in range(S)]
        for s in range(S):
            assert same_bits(recs[s]['syms'], bank.symbols(s)), ('symbols', name, 'stream', s, 'call', k)
            assert np.array_equal(bank.loop_state(s).view(np.uint32), recs[s]['state'].view(np.uint32)), ('loop state', name, 'stream', s, 'call', k)
            assert np.array_equal(bits[s], recs[s]['bits']), ('decoded bits', name, 'stream', s, 'call', k)


@pytest.mark.parametrize('order', [('default', 'ratio_2.5', 'ratio_2.4'), ('ratio_2.4', 'ratio_2.5', 'default')], ids=['2.0_first', '2.4_first'])
def test_rrc_cache_s2_handles_of_three_rate_ratios_in_either_order(pkg, order):
    """regression test of the cache key: 2.4 samples per symbol rounds to 2, and a key that rounds hands the second handle the first one's taps"""
    _need_gpu()
    eng = pkg.Engine(0)
    try:
        _s2_first_calls(eng, order)
    finally:
        eng.close()


@pytest.mark.parametrize('s2_first', [True, False])
def test_rrc_cache_dvbs_bank_at_1_6_sps_beside_an_s2_handle(pkg, s2_first):
    """the DVB-S bank takes its taps from the same cache (65 taps, roll-off 0.35: the S2 default at 2 samples per symbol, the bank at 1.6)"""
    _need_gpu()
    eng = pkg.Engine(0)
    try:
        if s2_first:
            _s2_first_calls(eng, ('default',), ncalls=1)
        _dvbs_single(pkg, eng, rc.DVBS_BY_NAME['sps_1.6'])
        if not s2_first:
            _s2_first_calls(eng, ('default',), ncalls=1)
    finally:
        eng.close()


# ---------------------------------------------------------------------------------------------------------------- DVB-S
@pytest.mark.parametrize('case', rc.DVBS_CASES, ids=DVBS_IDS)
def test_dvbs_single_carrier_equals_oracle(engine, pkg, case):
    """one carrier: the wave-per-stream kernels, two calls with an odd cut"""
    n = _dvbs_single(pkg, engine, case)
    assert abs(n - case['nsym']) <= 0.01 * case['nsym']


@pytest.mark.parametrize('case', rc.DVBS_CASES, ids=DVBS_IDS)
def test_dvbs_bank_kernels_equal_oracle(bank_engine, pkg, case):
    """three carriers through the bank kernels, in one time slice and in three"""
    _dvbs_single(pkg, bank_engine, case, nstreams=3)


def test_dvbs_bank_of_carriers_of_different_length(bank_engine, pkg):
    case = rc.DVBS_BY_NAME['sps_2.5']
    iq = rc.dvbs_signal(case)
    lens = [iq.size, iq.size - 1001, iq.size // 3, iq.size - 7]
    runs = [rc.dvbs_oracle_run(case, rc.dvbs_cuts(n)) for n in lens]
    bank = pkg.DvbsDemodBank(bank_engine, len(lens), max_samples=max(c['b'] - c['a'] for r in runs for c in r), **case['cfg'])
    try:
        _dvbs_compare(bank, [iq[:n] for n in lens], runs, case['name'])
    finally:
        bank.close()


# ---------------------------------------------------------------------------------------------------------------- refusals
def test_s2_create_refuses_what_the_rule_refuses(engine, pkg):
    for name, o in rc.S2_REFUSED:
        with pytest.raises(pkg.Dvbs2GpuError) as e:
            engine.demod(engine.default_cfg(rc.S2_MODCOD, True, False, **o), max_samples=4096)
        assert e.value.code == pkg.ERR_ARG, name
    for name, o in rc.S2_EDGE_ACCEPTED:
        engine.demod(engine.default_cfg(rc.S2_MODCOD, True, False, **o), max_samples=4096).close()


def test_dvbs_create_refuses_what_the_rule_refuses(engine, pkg):
    for name, o in rc.DVBS_REFUSED:
        with pytest.raises(pkg.Dvbs2GpuError) as e:
            pkg.DvbsDemodBank(engine, 1, max_samples=4096, **o)
        assert e.value.code == pkg.ERR_ARG, name
    for name, o in rc.DVBS_EDGE_ACCEPTED:
        pkg.DvbsDemodBank(engine, 1, max_samples=4096, **o).close()


def test_refused_set_params_leaves_a_non_default_handle_as_it_was(engine, pkg):
    """set_params carries MODCOD, frame size, pilots, SOF threshold and trial count -- none of the front-end fields, so the rule cannot refuse it; what it does
    refuse (a MODCOD that does not exist) goes back through the rule with the handle's own configuration: the next calls equal the oracle's with it"""
    case = rc.S2_BY_NAME['rolloff_0.20']
    iq = rc.s2_signal(case)[0]
    run = rc.s2_oracle_run(case, rc.s2_cuts(iq.size, 'whole'))
    dm = engine.demod(rc.s2_engine_cfg(engine, case), max_samples=rc.S2_CALL)
    try:
        for k, rec in enumerate(run['calls'][:3]):
            if k == 1:
                for bad in ((0, True, False), (11, True, False)):      # no such MODCOD; short 9/10 does not exist
                    with pytest.raises(pkg.Dvbs2GpuError):
                        dm.set_params(*bad, sof_threshold=0.3, max_ldpc_trials=1)
            g = dm.process(iq[rec['a']:rec['b']])
            _check_handle(rec, dm, dc.flat_bytes(g), (case['name'], 'call', k))
    finally:
        dm.close()
