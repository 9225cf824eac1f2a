"""CPU test of the clock-drift signal catalogue (s2_drift_cases.py) on the oracle alone: the conditions that make the GPU comparison of
test_gpu_s2_clock_drift.py mean something.  A signal is in the catalogue because it drives the timing recovery to the ends of its interpolator
bank, through sample slips and into its clamps; the oracle's event counters (S2Rx::timing_events) say whether it does.  These are conditions,
not measurements: an entry that misses one is changed (more frames, another seed), not the threshold.

Thresholds, against what the oracle shows (12 frames of QPSK 3/4 short + pilots, 201 680 samples at 2 per symbol): without drift 43 / 105 on-symbol
outputs at arm 0 / arm 127 and 3 / 2 steps of 0 / 2 samples; at +-300 .. 600 ppm 740 .. 940 at either end and 60 .. 110 slips in the direction of the
clock error (one per 1 / ppm samples, less the acquisition).

What the oracle shows per entry (arm 0 / arm 127 / 0-sample steps / 2-sample steps / clamped errors / steps at the frequency limit, transmitted frames delivered):
    no_drift                  43 /  105 /   3 /   2 / 0 /     0   11        8psk_p300                733 /  803 /   1 /  53 / 0 / 0   11
    p300                     844 /  896 /   2 /  62 / 0 /     0    9        8psk_m300                721 /  759 /  52 /   0 / 0 / 0   11
    m300                     886 /  941 /  63 /   1 / 0 /     0   10        32apsk_pilots_p300       679 /  734 /   2 /  50 / 0 / 0   16
    p600                     738 /  806 /   1 / 111 / 0 /     0   10        16apsk_m300              865 / 1337 /  49 /   5 / 0 / 0   12
    m600                     766 /  826 / 109 /   1 / 0 /     0    8        p300_level_0.05         1064 / 1538 /   1 /  83 / 0 / 0   14
    p600_omega_limit_1e-4    624 /  497 /   5 /   7 / 0 / 39022    0        p300_level_0.25         1383 / 1555 /   2 /  98 / 0 / 0   17
    p300_level_1000         1257 / 1270 /  75 /  97 / 7 /     0    0        p300_level_4            1600 / 1482 /   7 /  95 / 0 / 0   16
    p300_level_1e-4       100871 /    0 / 285 / 285 / 0 /     0    0        m300_level_12           1293 / 1305 / 382 /   0 / 0 / 0    4
    vcm_p300                1601 / 1687 /   1 / 149 / 0 /     0   11        8psk_pilot_aided_m300    667 /  732 /  47 /   1 / 0 / 0   10
    tiny_calls_p300          851 /  888 /   1 /  61 / 0 /     0    9        tiny_calls_m300          885 /  958 /  63 /   1 / 0 / 0   10"""
import numpy as np
import pytest
import orc
import s2_drift_cases as dc

ALL = dc.CASES + dc.batch_cases() + dc.batch_cases(frames=(6,) * 9)


@pytest.mark.parametrize('case', ALL, ids=[c['name'] + ('' if k < len(dc.CASES) + 9 else '_6f') for k, c in enumerate(ALL)])
def test_every_tap_of_every_call_is_finite(case):
    """also the guard against handing a GPU a signal that drives a loop to non-finite state: such a signal does not go into the catalogue"""
    run = dc.oracle_run(case)
    assert np.isfinite(dc.signal(case)[0].view(np.float32)).all()
    for k, c in enumerate(run['calls']):
        for t in range(3):
            assert np.isfinite(c['taps'][t].view(np.float32)).all(), (case['name'], 'tap', t, 'call', k)
        assert np.isfinite(np.uint32(c['nco']).view(np.float32)), (case['name'], 'nco', k)
        for st in c['stats']:
            assert np.isfinite(np.array(st[:2], np.uint32).view(np.float32)).all(), (case['name'], 'stats', k)


@pytest.mark.parametrize('case', dc.CASES, ids=[c['name'] for c in dc.CASES])
def test_signal_drives_the_timing_recovery_where_it_says(case):
    run = dc.oracle_run(case)
    ev = run['events']
    good = dc.good_frames(case, run)
    print(case['name'], ev, 'good frames', len(good), 'symbols', run['symbols'], 'of', dc.signal(case)[2])
    name = case['name']
    if dc.is_drift(case):
        if name == 'p300_level_1e-4':
            assert ev['arm0'] >= 0.9 * (run['symbols']), ev          # (one on-symbol output per 1-sps symbol)
        else:
            assert ev['arm0'] >= 200 and ev['arm127'] >= 200, ev
        if name != 'p600_omega_limit_1e-4':
            assert (ev['step2'] if case['ppm'] > 0 else ev['step0']) >= 40, ev
    if name == 'p600_omega_limit_1e-4':
        assert ev['freq_limit'] >= 10000, ev
    if name == 'p300_level_1000':
        assert ev['clamped'] >= 1, ev
    if dc.has_decode_condition(case):
        assert len(good) >= 6 and good == sorted(set(good)), good              # transmitted frames, in transmitted order
        assert abs(run['symbols'] - dc.signal(case)[2]) <= 16, (run['symbols'], dc.signal(case)[2])


def test_catalogue_holds_what_the_gpu_tests_rely_on():
    names = set(dc.BY_NAME)
    assert len(dc.CASES) >= 17 and {'no_drift', 'p300', 'm300', 'p600', 'm600', 'p600_omega_limit_1e-4', 'p300_level_1000', 'p300_level_1e-4',
                                     'vcm_p300', '8psk_pilot_aided_m300', 'tiny_calls_p300', 'tiny_calls_m300'} <= names
    assert sum(dc.has_decode_condition(c) for c in dc.CASES) >= 9
    for c in dc.CASES:
        if c['head'] is not None:
            sizes = np.diff(dc.cuts(c, dc.signal(c)[0].size))
            assert (sizes == 0).any() and (sizes == 1).any() and sizes.max() == c['call']
    assert sorted(c['ppm'] for c in dc.batch_cases()) == [-900, -600, -300, -100, 0, 100, 300, 600, 900]
    assert len({dc.signal(c)[0].size for c in dc.batch_cases()}) >= 5            # the streams of the batch differ in length


def test_oracle_ends_a_call_whose_timing_loop_went_non_finite():
    """input x 100 with agc_rate 0.01: rate x amplitude > 2, FastAGC's recurrence diverges within 66 samples, the timing error becomes NaN (which passes both
    clamps), loop frequency and phase become NaN, and the sample offset (int) floorf(NaN) used to index the delay line at INT_MIN (SIGSEGV in the first call of
    100 samples).  What such calls deliver is unspecified; they return, and reset() followed by a clean signal decodes as a fresh receiver does."""
    case = dc.BY_NAME['no_drift']
    iq, sent, _ = dc.signal(case)
    rx = orc.OracleRx(orc.default_cfg(6, 1, 1, agc_rate=0.01, max_ldpc_trials=16))
    bad = (iq * np.float32(100.0)).astype(np.complex64)
    for a in range(0, 4000, 100):
        rx.process(bad[a:a + 100])
    rx.process(bad[4000:30000])
    rx.reset()
    fresh = orc.OracleRx(orc.default_cfg(6, 1, 1, agc_rate=0.01, max_ldpc_trials=16))
    clean, good = iq, 0
    for a in range(0, clean.size, 7001):
        o, f = rx.process(clean[a:a + 7001]), fresh.process(clean[a:a + 7001])
        assert np.array_equal(o, f)
        for t in range(4):
            x, y = rx.tap(t), fresh.tap(t)
            assert x.shape == y.shape and np.array_equal(x.view(np.uint8), y.view(np.uint8)), (t, a)
        assert [dc.stat_tuple(s, False) for s in rx.tap(4)] == [dc.stat_tuple(s, False) for s in fresh.tap(4)]
        good += sum(bytes(x) in set(sent) for x in o)
    assert good >= 6, good
