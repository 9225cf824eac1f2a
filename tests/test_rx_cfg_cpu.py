"""What the configurations of rx_cfg_cases.py do to the CPU oracle alone: that the GPU parity tests (test_gpu_rx_cfg.py) compare something.

  * DVB-S2: every case delivers BBFRAMEs; with the gains where decoding is to be expected, most of the 14 transmitted frames come out byte for byte;
    omega_rel_limit 0 pins the loop frequency to its limit; the clamp case holds the timing error in its clamp for thousands of symbols, and the outputs
    of every call of every case stay inside what the engine has room for (csrc/rx_cfg_rules.h).
    (The clamped error of a noise input has both signs: the output density stays near 1 per sample.  The one-sided worst case -- every error at the clamp that
    makes the loop emit most -- is run on a model of the kernels' loops by tests/cpp/rx_cfg_rules_host.cpp.)
  * RRC taps: the configurations the rounded cache key could not tell apart differ in their floats.
  * DVB-S: one symbol per `samples per symbol` input samples; where the loops lock, a QPSK constellation.
No GPU."""
import numpy as np
import pytest
import orc
import rx_cfg_cases as rc


@pytest.mark.parametrize('case', rc.S2_CASES, ids=[c['name'] for c in rc.S2_CASES])
def test_s2_case_on_the_oracle(case):
    iq, sent = rc.s2_signal(case)
    assert len(sent) == rc.S2_FRAMES and 220000 < iq.size < 260000
    run = rc.s2_oracle_run(case, rc.s2_cuts(iq.size, 'whole'))
    good, delivered = rc.s2_good_frames(case, run)
    print(case['name'], 'good', good, 'delivered', delivered, run['events'])
    assert delivered >= 1
    if case['min_good']:
        assert good >= case['min_good'], (good, delivered)
    # what the timing recovery emits fits the engine's buffer in every call: 2 outputs per symbol of tap 0, up to one held back between calls
    for c in run['calls']:
        assert 2 * c['taps'][0].size + 1 <= rc.s2_out_capacity(c['b'] - c['a'])


def test_omega_rel_limit_0_pins_the_loop_frequency():
    case = rc.S2_BY_NAME['omega_limit_0']
    run = rc.s2_oracle_run(case, rc.s2_cuts(rc.s2_signal(case)[0].size, 'whole'))
    assert run['events']['freq_limit'] > 0


def test_clamp_case_holds_the_error_in_its_clamp():
    case = rc.S2_BY_NAME['clamp_at_the_edge']
    assert case['cfg']['clock_mu_gain'] == rc.s2_mu_max(0.02)
    run = rc.s2_oracle_run(case, rc.s2_cuts(rc.s2_signal(case)[0].size, 'whole'))
    print(run['events'])
    assert run['events']['clamped'] > 1000
    # (steps of 0 and of 2 samples at the largest gain: the phase jumps by 0.078 per clamped symbol)
    assert run['events']['step0'] > 10 and run['events']['step2'] > 10


def test_short_call_plan_has_calls_below_the_delay_line():
    n = rc.s2_signal(rc.S2_BY_NAME['taps_129'])[0].size
    sizes = np.diff(rc.s2_cuts(n, 'short_calls')).tolist()
    assert 0 in sizes and 1 in sizes and 50 in sizes and max(sizes) == rc.S2_CALL and sum(sizes) == n


def _taps(n, alpha, ratio):
    out = np.zeros(n, np.float32)
    orc._bind_chain().orc_rrc_taps(n, float(np.float32(alpha)), 1.0, ratio, out)
    return out


def test_rrc_taps_the_rounded_key_confused_differ():
    """the old key: ntaps * 100000 + round(alpha * 1000) * 10 + round(samplerate / symbolrate)"""
    def old_key(n, alpha, ts):
        return n * 100000 + int(np.floor(float(np.float32(alpha)) * 1000 + 0.5)) * 10 + int(np.floor(ts + 0.5))       # (lround)
    pairs = [((65, 0.35, 2.0), (65, 0.35, 2.4)), ((65, 0.35, 2.0), (65, 0.35, 1.6)), ((65, 0.35, 2.4), (65, 0.35, 1.6)),
             ((65, 0.35, 2.0), (65, 0.3504, 2.0)), ((65, 0.20, 3.0), (65, 0.2004, 3.0)), ((129, 0.35, 11.6), (129, 0.35, 12.0))]
    for a, b in pairs:
        assert old_key(*a) == old_key(*b), (a, b)
        assert not np.array_equal(_taps(*a).view(np.uint32), _taps(*b).view(np.uint32)), (a, b)
    # (2.5 rounds to 3: the old key told it from 2.0, but not from 3.0 or 3.4)
    assert old_key(65, 0.35, 2.5) != old_key(65, 0.35, 2.0) and old_key(65, 0.35, 2.5) == old_key(65, 0.35, 3.0)
    assert not np.array_equal(_taps(65, 0.35, 2.5), _taps(65, 0.35, 3.0))


def test_refusal_lists_lie_beyond_the_restated_bounds():
    """the refusal lists are what they say: each entry breaks a bound as this file restates it, each edge entry keeps all of them"""
    def s2_ok(o):
        c = dict(omega_rel_limit=0.02, clock_mu_gain=rc.DEFAULT_MU, clock_omega_gain=rc.DEFAULT_OMEGA_GAIN, agc_rate=1e-4, loop_bw=0.00628, fll_bw=0.006,
                 rrc_taps=65, rrc_alpha=0.35, samplerate=55e6, symbolrate=27.5e6)
        c.update(o)
        f = {k: float(np.float32(c[k])) for k in ('omega_rel_limit', 'clock_mu_gain', 'clock_omega_gain', 'agc_rate', 'loop_bw', 'fll_bw', 'rrc_alpha')}
        if not all(np.isfinite(v) for v in f.values()):
            return False
        ts = c['samplerate'] / c['symbolrate'] if c['symbolrate'] > 0 and c['samplerate'] > 0 and np.isfinite(c['samplerate']) else 0.0
        return (0 <= f['omega_rel_limit'] <= float(rc.S2_LIM_MAX) and 1.0 - f['omega_rel_limit'] - abs(f['clock_mu_gain']) / 2 >= rc.S2_A_AVG_MIN and
                1 <= c['rrc_taps'] <= 129 and 0 <= f['rrc_alpha'] <= 1 and ts >= 2.0 ** -1000)

    def dvbs_ok(o):
        c = dict(omega_rel_limit=0.02, clock_mu_gain=rc.DEFAULT_MU, clock_omega_gain=rc.DEFAULT_OMEGA_GAIN, agc_rate=1e-4, loop_bw=0.00628, fll_bw=0.006,
                 rrc_taps=65, rrc_alpha=0.35, samplerate=4e6, symbolrate=2e6)
        c.update(o)
        f = {k: float(np.float32(c[k])) for k in ('omega_rel_limit', 'clock_mu_gain', 'clock_omega_gain', 'agc_rate', 'loop_bw', 'fll_bw', 'rrc_alpha')}
        if not all(np.isfinite(v) for v in f.values()) or not (1 <= c['samplerate'] < 2 ** 31 and 1 <= c['symbolrate'] < 2 ** 31):
            return False
        sps = c['samplerate'] / c['symbolrate']
        return (0 <= f['omega_rel_limit'] <= 0.25 and sps <= 64 and sps * (1 - f['omega_rel_limit']) >= 1.5 and
                sps * (1 - f['omega_rel_limit']) - abs(f['clock_mu_gain']) >= rc.DVBS_A_MIN and c['rrc_taps'] == 65 and 0 <= f['rrc_alpha'] <= 1)

    assert s2_ok({}) and dvbs_ok({})
    for name, o in rc.S2_REFUSED:
        assert not s2_ok(o), name
    for name, o in rc.S2_EDGE_ACCEPTED:
        assert s2_ok(o), name
    for name, o in rc.DVBS_REFUSED:
        assert not dvbs_ok(o), name
    for name, o in rc.DVBS_EDGE_ACCEPTED:
        assert dvbs_ok(o), name
    for c in rc.S2_CASES:
        assert s2_ok(c['cfg']), c['name']
    for c in rc.DVBS_CASES:
        assert dvbs_ok(c['cfg']), c['name']


@pytest.mark.parametrize('case', rc.DVBS_CASES, ids=[c['name'] for c in rc.DVBS_CASES])
def test_dvbs_case_on_the_oracle(case):
    iq = rc.dvbs_signal(case)
    calls = rc.dvbs_oracle_run(case)
    assert len(calls) == 2 and calls[0]['b'] % 2 == 1
    sy = np.concatenate([c['syms'] for c in calls])
    assert abs(sy.size - iq.size / case['sps']) <= 0.01 * iq.size / case['sps']           # one symbol per `sps` input samples
    h = sy[sy.size // 2:]
    v = np.concatenate([np.abs(h.real), np.abs(h.imag)])
    spread = float(v.std() / v.mean())
    print(case['name'], 'symbols', sy.size, 'spread %.3f' % spread, 'decoded bits', sum(c['bits'].size for c in calls))
    if case['max_spread'] is not None:
        assert spread <= case['max_spread']
