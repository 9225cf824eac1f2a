"""Receiver configurations off the plugin's defaults, for the CPU test of the oracle (test_rx_cfg_cpu.py) and the GPU parity tests (test_gpu_rx_cfg.py).
Test infrastructure only.

Everything else in the suite creates its handles with 65 taps, roll-off 0.35, exactly 2 samples per symbol, agc_rate 1e-4 and the default loop gains.  The
catalogue walks what the C ABI accepts beyond that -- csrc/rx_cfg_rules.h says what it accepts; the bounds are restated here on their own (S2_A_AVG_MIN,
DVBS_A_MIN, ...) so that the tests hold the library to the numbers, not to itself -- and lists what it must refuse.

S2_CASES / DVBS_CASES: one single-stream signal and configuration each.
    cfg     overrides of the default receiver configuration (engine field names; the oracles' names differ for DVB-S: dvbs_oracle_cfg)
    tx      what the modulator below gets: roll-off, Es/N0, level, noise_only
    min_good (DVB-S2)   delivered BBFRAMEs that must equal a transmitted one, where a bound is stated for the case (0: at least one delivered frame, whatever it holds)
    max_spread (DVB-S)  bound on std / mean of |re|, |im| over the second half of the symbols (None: no lock expected or no bound stated; equality only)
S2_REFUSED / DVBS_REFUSED: configurations on the far side of each bound (name, overrides)."""
import numpy as np
import orc
import orc_dvbs as od
import s2_drift_cases as dc

# ---- the rule, restated (csrc/rx_cfg_rules.h)
S2_A_AVG_MIN = 16.0 / 17.0 + 1e-6          # 1 - omega_rel_limit - |clock_mu_gain| / 2 at least: n samples -> fewer than n / a_avg + 2 outputs <= n + n/16 + 128
S2_LIM_MAX = np.float32(0.05)
DVBS_A_MIN = 1.3                           # samples per symbol * (1 - omega_rel_limit) - |clock_mu_gain| at least: <= 198 symbols per 256-sample tile
DVBS_LIM_MAX = np.float32(0.25)


def f32_below(x):
    """the largest float32 <= x"""
    f = np.float32(x)
    return float(f if float(f) <= x else np.nextafter(f, np.float32(-np.inf)))


def f32_above(x):
    """the smallest float32 > x"""
    f = np.float32(x)
    return float(f if float(f) > x else np.nextafter(f, np.float32(np.inf)))


def s2_mu_max(lim):
    """the largest clock_mu_gain (a float32) a DVB-S2 handle accepts at this omega_rel_limit"""
    return f32_below(2.0 * (1.0 - float(np.float32(lim)) - S2_A_AVG_MIN))


def dvbs_mu_max(sps, lim):
    return f32_below(sps * (1.0 - float(np.float32(lim))) - DVBS_A_MIN)


def s2_out_capacity(n):
    """outputs of the timing recovery the engine has room for in a call of n samples"""
    return n + n // 16 + 128


def timing_gains(bw, damp=0.707):
    """the critically damped (clock_mu_gain, clock_omega_gain) of a loop bandwidth, as the plugin computes them (main.cpp:134-140)"""
    bw, damp = np.float32(bw), np.float32(damp)
    den = np.float32(1.0 + 2.0 * float(damp) * float(bw) + float(bw * bw))
    return float(np.float32(4.0) * damp * bw / den), float(np.float32(4.0) * bw * bw / den)


DEFAULT_MU, DEFAULT_OMEGA_GAIN = timing_gains(0.00628)


# ---- modulator: numpy float64, any roll-off and any samples-per-symbol ratio (orc.transmit and orc_dvbs_modulate shape with 0.35 at 2 sps only)
def rrc_pulse(t, alpha):
    """the root-raised-cosine pulse of roll-off alpha (T = 1, unit energy) at times t"""
    t = np.asarray(t, np.float64)
    out = np.empty_like(t)
    zero = np.abs(t) < 1e-9
    sing = np.abs(np.abs(4.0 * alpha * t) - 1.0) < 1e-9 if alpha > 0 else np.zeros_like(zero)
    reg = ~(zero | sing)
    x = t[reg]
    out[reg] = (np.sin(np.pi * x * (1 - alpha)) + 4 * alpha * x * np.cos(np.pi * x * (1 + alpha))) / (np.pi * x * (1 - (4 * alpha * x) ** 2))
    out[zero] = 1 - alpha + 4 * alpha / np.pi
    if alpha > 0:
        out[sing] = alpha / np.sqrt(2.0) * ((1 + 2 / np.pi) * np.sin(np.pi / (4 * alpha)) + (1 - 2 / np.pi) * np.cos(np.pi / (4 * alpha)))
    return out


def modulate(syms, sps, alpha, esn0_db, cfo, timing, phase, seed, level=1.0, noise_only=False, span=16):
    """symbols (complex, unit power) -> complex64 [round(len * sps)]: sample n sits at symbol time (n + timing) / sps; seeded complex Gaussian noise of
    variance 10^(-esn0_db/10) * sps / 2 per component (Es/N0 after a unit-energy matched filter); then carrier offset (rad/sample) and phase, then the level"""
    syms = np.asarray(syms, np.complex128)
    n = int(round(syms.size * sps))
    t = (np.arange(n) + timing) / sps
    k0 = np.floor(t).astype(np.int64)
    x = np.zeros(n, np.complex128)
    if not noise_only:
        for d in range(-span, span + 1):
            k = k0 + d
            ok = (k >= 0) & (k < syms.size)
            x[ok] += syms[k[ok]] * rrc_pulse(t[ok] - k[ok], alpha)
    rng = np.random.default_rng(seed)
    sigma = np.sqrt(10.0 ** (-esn0_db / 10.0) * sps / 2.0)
    x += sigma * (rng.standard_normal(n) + 1j * rng.standard_normal(n))
    x *= np.exp(1j * (phase + cfo * np.arange(n)))
    out = (x * level).astype(np.complex64)
    out.setflags(write=False)
    return out


# ---- DVB-S2 cases: MODCOD 6 (QPSK 3/4), short frames, no pilots, 14 frames behind 211 lead symbols
S2_MODCOD, S2_SHORT, S2_PILOTS, S2_FRAMES, S2_LEAD = 6, 1, 0, 14, 211
S2_CALL = 30011
ESN0_NOISY = 9.0


def _s2(name, cfg=None, alpha=0.35, esn0=14.0, level=1.0, noise_only=False, min_good=8):
    c = dict(max_ldpc_trials=16)
    c.update(cfg or {})
    return dict(name=name, cfg=c, tx=dict(alpha=alpha, esn0=esn0, level=level, noise_only=noise_only), min_good=min_good)


def _gains(bw):
    mu, og = timing_gains(bw)
    return dict(clock_mu_gain=mu, clock_omega_gain=og)


S2_CASES = [
    _s2('default'),
    # roll-off: most carriers on air use 0.20 or 0.25 (transmitter and receiver); a receiver at 0.05 on the 0.35 signal
    _s2('rolloff_0.20', dict(rrc_alpha=0.20), alpha=0.20),
    _s2('rolloff_0.25', dict(rrc_alpha=0.25), alpha=0.25, min_good=4),      # (t = +-Ts / (4 alpha) falls on taps: the singular branch of the tap formula)
    _s2('rx_rolloff_0.05', dict(rrc_alpha=0.05), min_good=4),
    # tap counts: 1 (no delay line), 2, even counts (the decimator's even tail), the largest
    _s2('taps_1', dict(rrc_taps=1), min_good=0),
    _s2('taps_2', dict(rrc_taps=2), min_good=4),
    _s2('taps_33', dict(rrc_taps=33)),
    _s2('taps_64', dict(rrc_taps=64)),
    _s2('taps_128', dict(rrc_taps=128)),
    _s2('taps_129', dict(rrc_taps=129)),
    # samplerate / symbolrate enters the taps only (the loops run at 2 samples per symbol whatever it says)
    _s2('ratio_2.5', dict(samplerate=2.5 * 27.5e6)),
    _s2('ratio_2.4', dict(samplerate=2.4 * 27.5e6), min_good=0),       # (rounds to 2: the pair a rounded cache key takes for one filter)
    # AGC
    _s2('agc_1e-3_level_0.25', dict(agc_rate=1e-3), level=0.25),
    _s2('agc_1e-5_level_4', dict(agc_rate=1e-5), level=4.0),
    _s2('agc_0.01', dict(agc_rate=0.01)),
    # timing gains: the critically damped pair of 4 x and 1/4 of the plugin's bandwidth; the largest |clock_mu_gain| the rule accepts, both signs
    _s2('timing_bw_x4', _gains(0.00628 * 4), min_good=0),
    _s2('timing_bw_div4', _gains(0.00628 / 4), min_good=0),
    _s2('mu_max', dict(clock_mu_gain=s2_mu_max(0.02)), min_good=0),
    _s2('mu_min', dict(clock_mu_gain=-s2_mu_max(0.02)), min_good=0),
    # omega_rel_limit: 0 (the loop frequency cannot move) and the largest
    _s2('omega_limit_0', dict(omega_rel_limit=0.0), min_good=0),
    _s2('omega_limit_0.05', dict(omega_rel_limit=float(S2_LIM_MAX)), min_good=0),
    # carrier loops
    _s2('loop_bw_0.002', dict(loop_bw=0.002)),
    _s2('loop_bw_0.02', dict(loop_bw=0.02)),
    _s2('loop_bw_0.05', dict(loop_bw=0.05)),
    _s2('fll_bw_0', dict(fll_bw=0.0)),
    _s2('fll_bw_0.001', dict(fll_bw=0.001)),
    _s2('fll_bw_0.05', dict(fll_bw=0.05)),
    # PL sync threshold, decoder trials
    _s2('sof_0.3', dict(sof_threshold=0.3)),
    _s2('sof_0.99', dict(sof_threshold=0.99)),
    _s2('ldpc_trials_1', dict(max_ldpc_trials=1)),
    _s2('ldpc_trials_50_noisy', dict(max_ldpc_trials=50), esn0=ESN0_NOISY),
    # at the rule's edge with the error in its clamp: noise alone at an amplitude of 1400 (the error is a difference of neighbouring arms: 0.01 of the amplitude)
    # and an AGC that needs 1 / (1400 * 1e-7) = 7000 samples per factor e: the error leaves the clamp after some 20 000 samples
    _s2('clamp_at_the_edge', dict(clock_mu_gain=s2_mu_max(0.02), agc_rate=1e-7), level=5000.0, noise_only=True, min_good=None),
]
S2_BY_NAME = {c['name']: c for c in S2_CASES}
assert len(S2_BY_NAME) == len(S2_CASES)

# the call plans of the single-stream tests: whole calls; calls of 50, 1 and 0 samples in the middle (shorter than the delay line of 129 taps)
S2_PLANS = {'whole': None, 'short_calls': (S2_CALL, 50, 1, 0, 50, 127, S2_CALL, 1, 1, 50)}


def s2_cuts(n, plan):
    c = [0]
    for k in (S2_PLANS[plan] or ()):
        c.append(min(n, c[-1] + k))
    while c[-1] < n:
        c.append(min(n, c[-1] + S2_CALL))
    return c


_cache = {}


def _s2_symbols():
    if 's2' not in _cache:
        _, bb, syms = orc.transmit(S2_MODCOD, S2_SHORT, S2_PILOTS, nframes=S2_FRAMES, seed=9, lead_symbols=S2_LEAD)
        _cache['s2'] = (syms, [bytes(b) for b in bb])
    return _cache['s2']


def s2_signal(case):
    """-> (iq complex64, read-only; [transmitted BBFRAME bytes]); one array per distinct transmitter setting, shared"""
    syms, sent = _s2_symbols()
    k = ('s2sig',) + tuple(sorted(case['tx'].items()))
    if k not in _cache:
        tx = case['tx']
        _cache[k] = modulate(syms, 2.0, tx['alpha'], tx['esn0'], 2e-4, 0.3, 0.7, seed=77, level=tx['level'], noise_only=tx['noise_only'])
    return _cache[k], sent


def s2_oracle_cfg(case):
    return orc.default_cfg(S2_MODCOD, S2_SHORT, S2_PILOTS, **case['cfg'])


def s2_engine_cfg(engine, case):
    return engine.default_cfg(S2_MODCOD, bool(S2_SHORT), bool(S2_PILOTS), **case['cfg'])


def s2_oracle_run(case, cuts):
    """the case through the CPU oracle alone, call by call (the record layout of s2_drift_cases.oracle_run, plus the outputs of the timing recovery per call).
    Computed once per (case, calls); shared, not to be changed."""
    k = ('s2run', case['name'], tuple(cuts))
    if k not in _cache:
        iq, _ = s2_signal(case)
        rx = orc.OracleRx(s2_oracle_cfg(case))
        calls, nsymbols = [], 0
        for a, b in zip(cuts[:-1], cuts[1:]):
            o = rx.process(iq[a:b])
            taps = [rx.tap(t) for t in range(4)]
            nsymbols += taps[0].size
            calls.append(dict(a=a, b=b, taps=taps, stats=[dc.stat_tuple(s, False) for s in rx.tap(4)], bb=dc.flat_bytes(o), nco=dc._u32(rx.nco_freq())))
        _cache[k] = dict(calls=calls, events=rx.timing_events(), symbols=nsymbols)
    return _cache[k]


def s2_good_frames(case, run):
    """how many delivered BBFRAMEs are byte-equal to a transmitted one; how many were delivered"""
    sent = set(s2_signal(case)[1])
    got = dc.delivered_frames(case, run)
    return sum(f in sent for f in got), len(got)


# ---- DVB-S cases: QPSK of the inner code's bit stream, 30 000 symbols
def _dvbs(name, sps, cfg=None, alpha=0.35, nsym=30000, level=1.0, max_spread=None):
    c = dict(samplerate=sps * 2e6, symbolrate=2e6)
    c.update(cfg or {})
    return dict(name=name, sps=sps, nsym=nsym, cfg=c, tx=dict(alpha=alpha, level=level), max_spread=max_spread)


DVBS_CASES = [
    _dvbs('sps_1.6', 1.6, max_spread=0.25),
    _dvbs('sps_2', 2.0, max_spread=0.25),
    _dvbs('sps_2.5', 2.5, max_spread=0.25),
    _dvbs('sps_4', 4.0, max_spread=0.25),
    _dvbs('sps_3_rolloff_0.20', 3.0, dict(rrc_alpha=0.20), alpha=0.20, max_spread=0.45),
    _dvbs('sps_1.5_omega_limit_0', 1.5, dict(omega_rel_limit=0.0)),
    _dvbs('sps_8_omega_limit_0.25', 8.0, dict(omega_rel_limit=float(DVBS_LIM_MAX)), max_spread=0.45),
    _dvbs('sps_64', 64.0, nsym=3000),
    _dvbs('agc_1e-3_level_0.25', 2.0, dict(agc_rate=1e-3), level=0.25, max_spread=0.25),
    _dvbs('loop_bw_0.02', 2.0, dict(loop_bw=0.02)),
    _dvbs('fll_bw_0.05', 2.0, dict(fll_bw=0.05)),
]
DVBS_BY_NAME = {c['name']: c for c in DVBS_CASES}
assert len(DVBS_BY_NAME) == len(DVBS_CASES)


DVBS_ESN0 = 15.0       # (noise alone then spreads |re|, |im| of a locked constellation by 0.18 of their mean)


def dvbs_signal(case):
    k = ('dvbssig', case['name'])
    if k not in _cache:
        tx, _ = od.dvbs_tx_bits(2, 2 * case['nsym'], seed=13)
        b = tx.astype(np.float64).reshape(-1, 2)
        syms = ((1 - 2 * b[:, 0]) + 1j * (1 - 2 * b[:, 1])) / np.sqrt(2.0)
        _cache[k] = modulate(syms, case['sps'], case['tx']['alpha'], DVBS_ESN0, 3e-4, 0.37, 0.4, seed=78, level=case['tx']['level'])
    return _cache[k]


def dvbs_cuts(n):
    """two calls with an odd cut"""
    return [0, (n * 3 // 7) | 1, n]


_ORACLE_NAME = dict(loop_bw='costas_bw', clock_mu_gain='mu_gain', clock_omega_gain='omega_gain')


def dvbs_oracle_cfg(case):
    return od.qpsk_alt_default_cfg(**{_ORACLE_NAME.get(k, k): v for k, v in case['cfg'].items()})


def dvbs_oracle_run(case, cuts=None):
    """DVBSDemod's receive side on the CPU (QPSK_ALT front end, slicer, self-locking Viterbi: as test_gpu_dvbs_demod.py restates it), call by call
    -> [dict(a, b, bits, syms, state)].  Computed once; shared, not to be changed."""
    iq = dvbs_signal(case)
    cuts = tuple(cuts if cuts is not None else dvbs_cuts(iq.size))
    k = ('dvbsrun', case['name'], cuts)
    if k not in _cache:
        rx = od.OracleQpskAlt(dvbs_oracle_cfg(case))
        o = od.L()
        sl = od.VP(o.orc_dvbs_slicer_create())
        vit = od.OracleViterbi()
        calls = []
        for a, b in zip(cuts[:-1], cuts[1:]):
            sy = np.ascontiguousarray(rx.process(iq[a:b]))
            soft = np.zeros(2 * sy.size + 8192, np.int8)
            n = o.orc_dvbs_slicer_process(sl, sy.size, od.P(sy), od.P(soft))
            bits = []
            if n:
                eb, en, es = vit.work(soft[:n].reshape(-1, 8192))
                bits = [eb[i, :en[i]] for i in range(len(en))]
            calls.append(dict(a=a, b=b, bits=np.concatenate(bits) if bits else np.zeros(0, np.uint8), syms=sy, state=rx.state().copy()))
        _cache[k] = calls
    return _cache[k]


# ---- what create must refuse (DVBS2GPU_ERR_ARG): the far side of every bound
NAN, INF = float('nan'), float('inf')
S2_REFUSED = [
    ('omega_limit_above_0.05', dict(omega_rel_limit=f32_above(float(S2_LIM_MAX)))),
    ('omega_limit_negative', dict(omega_rel_limit=-1e-6)),
    ('omega_limit_nan', dict(omega_rel_limit=NAN)),
    ('mu_above_max', dict(clock_mu_gain=f32_above(2.0 * (1.0 - float(np.float32(0.02)) - S2_A_AVG_MIN)))),
    ('mu_below_min', dict(clock_mu_gain=-f32_above(2.0 * (1.0 - float(np.float32(0.02)) - S2_A_AVG_MIN)))),
    ('mu_above_max_at_limit_0.05', dict(omega_rel_limit=float(S2_LIM_MAX), clock_mu_gain=f32_above(2.0 * (1.0 - float(S2_LIM_MAX) - S2_A_AVG_MIN)))),
    ('mu_steps_backwards', dict(clock_mu_gain=-1.0)),
    ('mu_steps_three', dict(clock_mu_gain=1.5)),
    ('mu_nan', dict(clock_mu_gain=NAN)),
    ('omega_gain_inf', dict(clock_omega_gain=INF)),
    ('agc_rate_nan', dict(agc_rate=NAN)),
    ('loop_bw_inf', dict(loop_bw=-INF)),
    ('fll_bw_nan', dict(fll_bw=NAN)),
    ('taps_0', dict(rrc_taps=0)),
    ('taps_130', dict(rrc_taps=130)),
    ('rolloff_negative', dict(rrc_alpha=-0.01)),
    ('rolloff_above_1', dict(rrc_alpha=f32_above(1.0))),
    ('rolloff_nan', dict(rrc_alpha=NAN)),
    ('samplerate_0', dict(samplerate=0.0)),
    ('samplerate_inf', dict(samplerate=INF)),
    ('symbolrate_negative', dict(symbolrate=-27.5e6)),
    ('ratio_subnormal', dict(samplerate=1e-310, symbolrate=1.0)),
]
DVBS_REFUSED = [
    ('taps_33', dict(rrc_taps=33)),
    ('taps_129', dict(rrc_taps=129)),
    ('sps_1.2', dict(samplerate=2.4e6)),
    ('sps_1.6_omega_limit_0.07', dict(samplerate=3.2e6, omega_rel_limit=0.07)),
    ('sps_65', dict(samplerate=130e6)),
    ('omega_limit_above_0.25', dict(omega_rel_limit=f32_above(0.25))),
    ('omega_limit_negative', dict(omega_rel_limit=-0.01)),
    ('mu_above_max', dict(clock_mu_gain=f32_above(2.0 * (1.0 - float(np.float32(0.02))) - DVBS_A_MIN))),
    ('mu_below_min', dict(clock_mu_gain=-f32_above(2.0 * (1.0 - float(np.float32(0.02))) - DVBS_A_MIN))),
    ('mu_above_max_at_1.5_sps', dict(samplerate=3e6, omega_rel_limit=0.0, clock_mu_gain=f32_above(1.5 - DVBS_A_MIN))),
    ('mu_nan', dict(clock_mu_gain=NAN)),
    ('omega_gain_inf', dict(clock_omega_gain=INF)),
    ('agc_rate_nan', dict(agc_rate=NAN)),
    ('loop_bw_nan', dict(loop_bw=NAN)),
    ('fll_bw_inf', dict(fll_bw=INF)),
    ('rolloff_above_1', dict(rrc_alpha=1.5)),
    ('rolloff_nan', dict(rrc_alpha=NAN)),
    ('symbolrate_0', dict(symbolrate=0.0)),
    ('rates_below_1', dict(samplerate=1.0, symbolrate=0.5)),
    ('samplerate_2^31', dict(samplerate=2147483648.0, symbolrate=1073741824.0)),
]
# the last accepted value beside some of those bounds (create must succeed)
S2_EDGE_ACCEPTED = [
    ('omega_limit_0.05', dict(omega_rel_limit=float(S2_LIM_MAX))),
    ('mu_max', dict(clock_mu_gain=s2_mu_max(0.02))),
    ('mu_min', dict(clock_mu_gain=-s2_mu_max(0.02))),
    ('mu_max_at_limit_0.05', dict(omega_rel_limit=float(S2_LIM_MAX), clock_mu_gain=s2_mu_max(S2_LIM_MAX))),
    ('rolloff_0', dict(rrc_alpha=0.0)),
    ('rolloff_1', dict(rrc_alpha=1.0)),
]
DVBS_EDGE_ACCEPTED = [
    ('sps_1.5_omega_limit_0', dict(samplerate=3e6, omega_rel_limit=0.0)),
    ('sps_64', dict(samplerate=128e6)),
    ('omega_limit_0.25', dict(omega_rel_limit=0.25)),
    ('mu_max', dict(clock_mu_gain=dvbs_mu_max(2.0, 0.02))),
    ('mu_min', dict(clock_mu_gain=-dvbs_mu_max(2.0, 0.02))),
]
