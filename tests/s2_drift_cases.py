"""DVB-S2 signals with a sampling-clock error, for the CPU test of the oracle (test_s2_drift_cpu.py) and the GPU parity tests
(test_gpu_s2_clock_drift.py).  Test infrastructure only.

With exactly 2 samples per symbol the polyphase arm of the timing recovery settles in the middle of its 128-arm bank and stays there.  A
clock that is off by a few hundred ppm walks it through the whole bank and over both ends every few thousand symbols: the one-sided
derivative at arm 0 and arm 127, steps that consume 0 or 2 samples, a candidate window pressed against the ends of the bank.  Input levels
far from 1 and a narrow omega_rel_limit add the error clamp and the frequency clamp.

Every entry of CASES is one single-stream signal:
    tx      keyword arguments of orc.transmit (or orc.transmit_vcm when `vcm` names the PLS list)
    ppm     sampling-clock error: the block of 2 * symbols samples is resampled to round(2 * symbols * (1 + ppm * 1e-6)) samples
    level   factor on every sample (float32)
    cfg     overrides of the default receiver configuration (the same field names in the oracle's and the engine's configuration)
    head    None, or the call sizes to draw from for the first 2500 samples (odd and tiny calls, an empty one among them)
    call    samples per call after that
BATCH is the set of streams of the multi-stream tests: one MODCOD, nine clock errors, different lengths."""
import functools
import numpy as np
import orc

# (the PLS list of test_gpu_s2chain.py's ACM/VCM tests: seven MODCODs and a dummy PLFRAME)
from test_gpu_s2chain import VCM_PLS

TINY = (0, 1, 2, 3, 5, 8, 15, 16, 17, 31, 33, 40)


def _case(name, modcod, short, pilots, nframes, esn0, cfo, ppm, level=1.0, cfg=None, call=7001, head=None, vcm=None, seed=5):
    tx = dict(nframes=nframes, seed=seed, esn0_db=esn0, cfo=cfo, timing=0.3, phase0=0.1, lead_symbols=400)
    if vcm is None:
        tx.update(modcod=modcod, short=short, pilots=pilots)
    c = dict(max_ldpc_trials=16)
    c.update(cfg or {})
    return dict(name=name, modcod=modcod, short=short, pilots=pilots, tx=tx, ppm=ppm, level=level, cfg=c, call=call, head=head, vcm=vcm)


CASES = [
    # QPSK 3/4 short frames with pilots: what the suite used so far, then the same signal on a clock that is off
    _case('no_drift', 6, 1, 1, 12, 14.0, 1e-3, 0),
    _case('p300', 6, 1, 1, 12, 14.0, 1e-3, 300),
    _case('m300', 6, 1, 1, 12, 14.0, -1e-3, -300),
    _case('p600', 6, 1, 1, 12, 14.0, 1e-3, 600),
    _case('m600', 6, 1, 1, 12, 14.0, 1e-3, -600),
    _case('p600_omega_limit_1e-4', 6, 1, 1, 12, 14.0, 1e-3, 600, cfg=dict(omega_rel_limit=1e-4)),     # the loop cannot follow: freq sits at its limit
    # the AGC's first samples: errors beyond +-1, which leave the loop frequency high; it takes some 90 000 samples to come back (0-sample steps on a fast clock
    # until then), so 24 frames (12 frames of seed 5 end before it has: 199 steps of 0 samples and 1 of 2)
    _case('p300_level_1000', 6, 1, 1, 24, 14.0, 1e-3, 300, level=1000.0, seed=6),
    _case('p300_level_1e-4', 6, 1, 1, 12, 14.0, 1e-3, 300, level=1e-4),                                 # the AGC never gets there: every symbol at arm 0
    # other constellations
    _case('8psk_p300', 14, 1, 0, 16, 16.0, -1e-3, 300),
    _case('8psk_m300', 14, 1, 0, 16, 16.0, -1e-3, -300),
    _case('32apsk_pilots_p300', 27, 1, 1, 24, 30.0, 1e-3, 300, call=6007),
    _case('16apsk_m300', 19, 1, 0, 18, 30.0, 1e-3, -300, call=6007),      # (18 frames: 12 of these short frames are 100 160 samples, 31 slips at 300 ppm)
    # input levels the AGC has to pull in
    _case('p300_level_0.05', 6, 1, 1, 20, 14.0, -1e-3, 300, level=0.05),
    _case('p300_level_0.25', 6, 1, 1, 20, 14.0, -1e-3, 300, level=0.25),
    _case('p300_level_4', 6, 1, 1, 20, 14.0, -1e-3, 300, level=4.0),
    _case('m300_level_12', 6, 1, 1, 20, 14.0, -1e-3, -300, level=12.0),
    # ACM/VCM framing and the pilot-aided PLL behind a drifting front end
    _case('vcm_p300', 4, 1, 0, 26, 22.0, 1e-3, 300, cfg=dict(acm_vcm=1, max_ldpc_trials=25), vcm=VCM_PLS, seed=3),
    _case('8psk_pilot_aided_m300', 14, 1, 1, 14, 14.0, 1e-3, -300, cfg=dict(pilot_aided=1)),
    # odd and tiny calls while the arm is on its way
    _case('tiny_calls_p300', 6, 1, 1, 12, 14.0, 1e-3, 300, head=TINY),
    _case('tiny_calls_m300', 6, 1, 1, 12, 14.0, -1e-3, -300, head=TINY),
]
BY_NAME = {c['name']: c for c in CASES}
assert len(BY_NAME) == len(CASES)

# the streams of one batch: QPSK 3/4 short frames with pilots, nine clock errors, 6 .. 12 frames (so the inputs differ in length, the streams of one
# resolver wave yield different output counts per period and end at different times).  (+-900 ppm: parity only, no decode condition.)
BATCH_PPM = (600, -600, 300, -300, 0, 900, -900, 100, -100)
BATCH_FRAMES = (12, 7, 9, 6, 10, 8, 11, 6, 12)


def batch_cases(frames=BATCH_FRAMES):
    return [_case('batch_%+d' % ppm, 6, 1, 1, nf, 14.0, (1e-3, -1e-3, 5e-4)[k % 3], ppm, seed=40 + k) for k, (ppm, nf) in enumerate(zip(BATCH_PPM, frames))]


def is_drift(case):
    return case['ppm'] != 0


def has_decode_condition(case):
    """default configuration, level 1, |ppm| <= 600"""
    return case['cfg'] == dict(max_ldpc_trials=16) and case['level'] == 1.0 and abs(case['ppm']) <= 600


def _key(case):
    return repr(sorted((k, v) for k, v in case.items()))


_signals = {}


def signal(case):
    """-> (iq complex64, [transmitted BBFRAME bytes, in order], symbols transmitted); one array per case, shared and never written to"""
    k = _key(case)
    if k not in _signals:
        if case['vcm'] is not None:
            nsym = case['tx']['lead_symbols'] + sum(orc.pls_info(case['vcm'][f % len(case['vcm'])])[0] for f in range(case['tx']['nframes']))
        else:
            nsym = case['tx']['lead_symbols'] + case['tx']['nframes'] * orc.modcod_params(case['modcod'], case['short'], case['pilots'])['plframe']
        nsamples = int(round(2 * nsym * (1 + case['ppm'] * 1e-6))) if case['ppm'] else 0
        if case['vcm'] is not None:
            iq, bbs = orc.transmit_vcm(case['vcm'], nsamples=nsamples, **case['tx'])
            sent = [bytes(b) for b in bbs if b is not None]
        else:
            iq, bb, _ = orc.transmit(nsamples=nsamples, **case['tx'])
            sent = [bytes(b) for b in bb]
        if case['level'] != 1.0:
            iq = (iq * np.float32(case['level'])).astype(np.complex64)
        iq.setflags(write=False)
        _signals[k] = (iq, sent, nsym)
    return _signals[k]


def cuts(case, n):
    """sample positions of the calls: [0, ..., n]"""
    c = [0]
    if case['head'] is not None:
        rng = np.random.default_rng(5)
        while c[-1] < 2500:
            c.append(c[-1] + int(rng.choice(case['head'])))
    while c[-1] < n:
        c.append(min(n, c[-1] + case['call']))
    return c


def oracle_cfg(case):
    return orc.default_cfg(case['modcod'], case['short'], case['pilots'], **case['cfg'])


def engine_cfg(engine, case):
    return engine.default_cfg(case['modcod'], bool(case['short']), bool(case['pilots']), **case['cfg'])


def _u32(x):
    return int(np.float32(x).view(np.uint32))


def stat_tuple(st, gpu):
    """a per-frame statistics record of the oracle (gpu = False) or the engine as one comparable tuple; the floats as their bits"""
    if gpu:
        return (_u32(st.pl_sync_best_match), _u32(st.coarse_freq_err), st.detected_modcod, st.detected_shortframes, st.detected_pilots,
                st.ldpc_trials, st.bch_corrections, st.bbframe_bytes)
    return (_u32(st.best_match), _u32(st.fed_err), st.detect_modcod, st.detect_short, st.detect_pilots, st.ldpc_trials, st.bch_corr, st.bbframe_bytes)


def flat_bytes(frames):
    """what process() returned (an array of equal frames, or the list of an ACM/VCM stream) as one byte string"""
    if isinstance(frames, list):
        return np.concatenate(frames) if frames else np.zeros(0, np.uint8)
    return np.ascontiguousarray(frames).reshape(-1)


_runs = {}


def oracle_run(case, call_cuts=None):
    """the case through the CPU oracle alone, call by call -> dict(calls = [dict(a, b, taps = [4 arrays], stats = [tuples], bb = bytes array,
    nco = bits of nco_freq)], events = timing_events(), symbols = 1-sps symbols delivered).  Computed once per (case, calls); shared, not to be changed."""
    iq, sent, nsym = signal(case)
    cc = tuple(call_cuts if call_cuts is not None else cuts(case, iq.size))
    k = (_key(case), cc)
    if k not in _runs:
        rx = orc.OracleRx(oracle_cfg(case))
        calls, nsymbols = [], 0
        for a, b in zip(cc[:-1], cc[1:]):
            o = rx.process(iq[a:b])
            taps = [rx.tap(t) for t in range(4)]
            nsymbols += taps[0].size
            calls.append(dict(a=a, b=b, taps=taps, stats=[stat_tuple(s, False) for s in rx.tap(4)], bb=flat_bytes(o), nco=_u32(rx.nco_freq())))
        _runs[k] = dict(calls=calls, events=rx.timing_events(), symbols=nsymbols)
    return _runs[k]


def delivered_frames(case, run):
    """the BBFRAMEs of an oracle run, in order of delivery, as byte strings"""
    out = []
    for c in run['calls']:
        pos = 0
        for st in c['stats']:
            if st[7]:
                out.append(bytes(c['bb'][pos:pos + st[7]]))
                pos += st[7]
        assert pos == c['bb'].size
    return out


def good_frames(case, run):
    """indices (into the transmitted sequence) of the delivered BBFRAMEs that are byte-equal to a transmitted one, in order of delivery"""
    sent = signal(case)[1]
    index = {}
    for k, b in enumerate(sent):
        index.setdefault(b, k)
    return [index[f] for f in delivered_frames(case, run) if f in index]
