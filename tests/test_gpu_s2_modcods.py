"""Every MODCOD and every PLS code through the DVB-S2 symbol path between PL sync and the LDPC input, against the CPU oracle.

Tolerance: NONE, as in tests/test_gpu_s2chain.py (same separately rounded operations in the same order on both sides).

  test_demap_every_modcod_bit_exact      the 104 valid (MODCOD, frame size, pilots) through the demapper: every ring ratio, every LUT, both
                                         forms of the kernel, inputs on the table-cell seams and non-finite ones
  test_deinterleave_every_modcod         the reference's recorded de-interleaver output for all 52 (MODCOD, frame size)
  test_every_apsk_modcod_in_one_mixed_batch   the MIXED kernels with every 16APSK / 32APSK MODCOD, with and without pilots
  test_acm_vcm_stream_over_every_pls_code     the ACM/VCM kernels and the PLS codeword search over all 104 data codes and a dummy frame

Each test first shows, on the oracle alone, that its input exercises what it is about (LLRs that are not zeros, settled streams
delivering transmitted frames, every PLS code detected and decoded): an engine that equals an oracle which does nothing passes nothing."""
import json
import os
from concurrent.futures import ThreadPoolExecutor

import hashlib
import numpy as np
import pytest

import orc

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
G = json.load(open(os.path.join(HERE, 'golden', 's2_tables_golden.json')))

VALID = [(m, s) for m in range(1, 29) for s in (0, 1) if not (s == 1 and m in (11, 17, 23, 28))]      # short 9/10 does not exist
COMBOS = [(m, s, p) for m, s in VALID for p in (0, 1)]
assert len(VALID) == 52 and len(COMBOS) == 104


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.dtype.kind in 'fc':
        return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))
    return np.array_equal(a, b)


# ------------------------------------------------------------------------------------------------------------ B1: demapper
def seam_values():
    """k * 1.5 / 256 as float32 for k = -140..139 -- the edges of the demapper's 256 x 256 table cells (constellation.cpp:295-301), and
    twelve cells beyond the table on either side -- each with its two float32 neighbours: where the engine's binary32 fast path has to
    hand over to the double form, and a one-ULP slip lands in the neighbouring cell"""
    k = np.arange(-140, 140)
    v = (k * 1.5 / 256).astype(np.float32)
    return np.stack([np.nextafter(v, np.float32(-np.inf)), v, np.nextafter(v, np.float32(np.inf))], 1).reshape(-1)


SPECIAL = np.array([np.inf, -np.inf, np.nan, 1e30, -1e30, 3e7, -3e7, 1e-45], np.float32)
SEG_SEAM, SEG_ZERO, SEG_FAR = 90, 90 + 840, 90 + 840 + 110
SEG_SPECIAL = SEG_FAR + 60                    # 24 samples; everything ends before the first pilot block (symbol 1530)


def demap_frames(modcod, plframe):
    """two PLL-output frames: Gaussian x 0.6; frame 1 carries, from the first payload symbol on, the seams (real axis ascending, imaginary
    axis descending), exact zeros, samples x 50 outside the table, and the eight special values on the real axis, on the imaginary
    axis and on both"""
    rng = np.random.default_rng(modcod)
    fr = (rng.standard_normal((2, plframe)) + 1j * rng.standard_normal((2, plframe))).astype(np.complex64) * np.float32(0.6)
    sv = seam_values()
    assert sv.size == 840 and SEG_SPECIAL + 24 <= 1530
    fr[1, SEG_SEAM:SEG_ZERO] = sv + 1j * sv[::-1]
    fr[1, SEG_ZERO:SEG_FAR] = 0
    fr[1, SEG_FAR:SEG_SPECIAL] *= 50
    other = fr[1, SEG_SPECIAL:SEG_SPECIAL + 8].copy()
    sp = np.zeros(24, np.complex64)
    sp.real[0:8], sp.imag[0:8] = SPECIAL, other.imag
    sp.real[8:16], sp.imag[8:16] = other.real, SPECIAL
    sp.real[16:24], sp.imag[16:24] = SPECIAL, SPECIAL
    fr[1, SEG_SPECIAL:SEG_SPECIAL + 24] = sp
    return fr


def demap_oracle(modcod, short, pilots, fr):
    mp = orc.modcod_params(modcod, short, pilots)
    rx = orc.OracleRx(orc.default_cfg(modcod, short, pilots))
    want = np.zeros((fr.shape[0], mp['N']), np.int8)
    for f in range(fr.shape[0]):
        rx.L.orc_s2rx_to_soft(rx.h, np.ascontiguousarray(fr[f]).view(np.float32), want[f])
    return want


def llrs_of_symbols(mp, llr, j0, j1):
    """the LLRs of payload symbols j0..j1-1 of one de-interleaved frame, as [j1 - j0, bits] (s2_deinterleaver.cpp:72-136, either column order)"""
    bits, rows = mp['bits'], mp['N'] // mp['bits']
    if bits == 2:
        return llr[2 * j0:2 * j1].reshape(-1, 2)
    return np.stack([llr[c * rows + j0:c * rows + j1] for c in range(bits)], 1)


def check_demap_oracle(mp, want):
    """the comparison is not about zeros, on the oracle's output alone.  32APSK (computed per symbol): max |LLR| > 60, the bar of
    test_demap_32apsk_bit_exact.  The LUT constellations: their table ends at |re|, |im| = 0.75, where the 8PSK and 16APSK LLRs of a unit-power
    constellation stop growing well inside the int8 range, so the bar is a quarter of that range, 32 -- six of the eight bits in use.
    The seam run must take many different table entries (it crosses 280 cell edges on either axis; 16 distinct LLR tuples is the least a
    QPSK table can show along a line), and nine LLRs in ten of the frame with the special segments are non-zero."""
    bar = 60 if mp['constel'] == 3 else 32
    assert np.abs(want[0].astype(np.int32)).max() > bar
    seam = llrs_of_symbols(mp, want[1], SEG_SEAM - 90, SEG_ZERO - 90)
    assert len({bytes(x) for x in seam}) >= 16 and np.abs(seam.astype(np.int32)).max() > 32
    assert (want[1] != 0).mean() > 0.9


@pytest.mark.parametrize('modcod,short,pilots', COMBOS)
def test_demap_every_modcod_bit_exact(engine, modcod, short, pilots):
    """engine.demap == the oracle's to_soft for every valid (MODCOD, frame size, pilots): each MODCOD's own ring ratios and LUT, the
    four-symbols-per-lane form and the byte form (16APSK short frames: columns of 4050 bytes, nsym % 4 == 2; 32APSK; and, for the LUT
    constellations, the same symbols one sample off the 16-byte grid), the pilot skip, and inputs on the cell seams, at zero, far outside
    the table, infinite, NaN, huge and subnormal.  Non-finite samples: the reference's x86-64 outcome (constellation.cpp:295-309,
    clamp() :263-270, tests/test_det_math.py) is what both sides define."""
    import torch
    mp = orc.modcod_params(modcod, short, pilots)
    fr = demap_frames(modcod, mp['plframe'])
    want = demap_oracle(modcod, short, pilots, fr)
    check_demap_oracle(mp, want)
    got = engine.demap(torch.from_numpy(fr).cuda(), modcod, bool(short), bool(pilots)).cpu().numpy()
    assert np.array_equal(got, want), int((got != want).sum())
    if mp['constel'] != 3:
        buf = torch.zeros(2 * mp['plframe'] + 1, dtype=torch.complex64, device='cuda')
        buf[1:] = torch.from_numpy(fr).cuda().reshape(-1)
        got2 = engine.demap(buf[1:].reshape(2, mp['plframe']), modcod, bool(short), bool(pilots)).cpu().numpy()
        assert np.array_equal(got2, want), int((got2 != want).sum())


# ------------------------------------------------------------------------------------------------------------ B2: de-interleaver
@pytest.mark.parametrize('case', G['deinterleave'], ids=lambda c: 'm%d-s%d' % (c['modcod'], c['short']))
def test_deinterleave_every_modcod(engine, case):
    """the reference's S2Deinterleaver output for the index ramp (tests/golden/make_golden_s2tables.py), for every (MODCOD, frame size)"""
    import torch
    n = 16200 if case['short'] else 64800
    src = (np.arange(n) * 7 % 251).astype(np.int8)
    mp = orc.modcod_params(case['modcod'], case['short'], 0)
    assert (mp['constel'], orc.RATE_NAMES[mp['rate']]) == (case['constel'], case['rate'])
    out = engine.deinterleave(torch.from_numpy(np.stack([src, src[::-1].copy()])).cuda(), case['modcod'], bool(case['short'])).cpu().numpy()
    assert hashlib.sha256(out[0].tobytes()).hexdigest() == case['out_sha']
    assert sorted(out[1].tolist()) == sorted(src.tolist())


# ------------------------------------------------------------------------------------------------------------ B3: mixed batch, APSK
APSK_STREAMS = [(m, 0 if m in (23, 28) else 1, p) for m in range(18, 29) for p in (0, 1)]


def apsk_stream_input(m, short):
    nfr = 30 if short else 10
    return dict(nframes=nfr, seed=100 + 2 * m + short, esn0_db=30.0, lead_symbols=300)


def apsk_oracle_stream(spec):
    """-> (iq, set of transmitted BBFRAMEs, the oracle receiver's BBFRAMEs [n, kbch / 8])"""
    m, short, pilots = spec
    iq, bb, _ = orc.transmit(m, short, pilots, **apsk_stream_input(m, short))
    out = orc.OracleRx(orc.default_cfg(m, short, pilots)).process(iq)
    return iq, {bytes(b) for b in bb}, out


def test_every_apsk_modcod_in_one_mixed_batch(engine, pkg):
    """MODCODs 18..28 with and without pilots as 22 streams of ONE process_batch call (16APSK and 32APSK short frames, the two 9/10 MODCODs
    with normal frames): the MIXED instantiations of the demapper and the frame loops read each stream's ring ratios, LUT or point set, slot
    count and pilot flag from its table entry.  Every stream's bytes EQUAL the oracle receiver's; on the oracle alone, every stream has
    settled: its last three delivered frames are transmitted ones."""
    import torch
    assert len(APSK_STREAMS) == 22
    with ThreadPoolExecutor(max_workers=16) as ex:
        ref = list(ex.map(apsk_oracle_stream, APSK_STREAMS))
    for spec, (iq, sent, out) in zip(APSK_STREAMS, ref):
        good = [bytes(x) in sent for x in out]
        assert len(out) >= 3 and all(good[-3:]), ('oracle', spec, good)
    demods = [engine.demod(engine.default_cfg(m, bool(s), bool(p)), max_samples=ref[i][0].size) for i, (m, s, p) in enumerate(APSK_STREAMS)]
    kbs = [d.info['kbch'] // 8 for d in demods]
    cap = max((apsk_stream_input(m, s)['nframes'] + 1) * kb for (m, s, p), kb in zip(APSK_STREAMS, kbs))
    tout = [torch.zeros(cap, dtype=torch.uint8, device='cuda') for _ in demods]
    try:
        nb = engine.process_batch(demods, [torch.from_numpy(r[0]).cuda() for r in ref], tout)
    finally:
        for d in demods:
            d.close()
    for i, spec in enumerate(APSK_STREAMS):
        got = tout[i][:nb[i]].cpu().numpy().reshape(-1, kbs[i])
        assert got.shape == ref[i][2].shape and np.array_equal(got, ref[i][2]), spec


# ------------------------------------------------------------------------------------------------------------ B4: ACM/VCM, every PLS code
def vcm_pls_list(short):
    pls = [(m << 2) | (short << 1) | p for m, s in VALID if s == short for p in (0, 1)]
    if short:
        pls.insert(len(pls) // 2, 0)           # one dummy PLFRAME in the middle
    return pls


def check_vcm_oracle(pls, bbs, stats, delivered):
    """on the oracle's own results: every PLS code of the list detected, a frame of every data code decoded to what was sent, at most one
    delivered frame that was not sent"""
    seen = {(st.detect_modcod << 2) | (st.detect_short << 1) | st.detect_pilots if st.detect_modcod else 0 for st in stats}
    assert set(pls) <= seen, sorted(set(pls) - seen)
    code_of = {bytes(b): pls[f % len(pls)] for f, b in enumerate(bbs) if b is not None}
    assert len(code_of) == sum(b is not None for b in bbs)
    decoded = [code_of.get(bytes(x)) for x in delivered]
    assert {c for c in pls if c >> 2} <= set(decoded), sorted({c for c in pls if c >> 2} - set(decoded))
    assert sum(c is None for c in decoded) <= 1, decoded


@pytest.mark.parametrize('short,esn0,cfo,flags', [(1, 100.0, 0.0, {}), (1, 25.0, 1e-3, {}), (0, 100.0, 0.0, {}), (0, 25.0, 1e-3, {}),
                                                  (1, 25.0, 1e-3, dict(soft_plsc=1, pilot_aided=1))],
                         ids=['short-clean', 'short-25dB', 'normal-clean', 'normal-25dB', 'short-25dB-soft-plsc-pilot-aided'])
def test_acm_vcm_stream_over_every_pls_code(engine, short, esn0, cfo, flags):
    """ONE ACM/VCM stream whose frames run twice through every data PLS code of one frame size, with and without pilots (short frames: 48
    codes and a dummy PLFRAME; normal frames: 56 codes -- with pilots the first descrambling beyond Rn[32399]): the PLS codeword search, the
    per-code frame sizes and the VCM walk / loops / demap kernels meet every code.  Taps, per-frame statistics and BBFRAMEs EQUAL the
    oracle's, call by call."""
    pls = vcm_pls_list(short)
    assert len(pls) == (49 if short else 56)
    iq, bbs = orc.transmit_vcm(pls, 2 * len(pls), seed=5, esn0_db=esn0, cfo=cfo, timing=0.3, phase0=0.2, lead_symbols=500)
    chunk = 200001
    rx = orc.OracleRx(orc.default_cfg(4, 1, 0, acm_vcm=1, max_ldpc_trials=25, **flags))
    dm = engine.demod(engine.default_cfg(4, True, False, acm_vcm=1, max_ldpc_trials=25, **flags), max_samples=chunk)
    stats_all, want_all = [], []
    try:
        for ncall, a in enumerate(range(0, iq.size, chunk)):
            part = iq[a:a + chunk]
            o = rx.process(part)
            g = dm.process(part)
            for t in range(4):
                assert same_bits(rx.tap(t), dm.tap(t)), ('tap', t, ncall)
            st_o, st_g = rx.tap(4), dm.stats()
            assert len(st_o) == len(st_g), ncall
            for a_, b_ in zip(st_o, st_g):
                assert np.float32(a_.best_match).view(np.uint32) == np.float32(b_.pl_sync_best_match).view(np.uint32)
                assert np.float32(a_.fed_err).view(np.uint32) == np.float32(b_.coarse_freq_err).view(np.uint32)
                assert (a_.detect_modcod, a_.detect_short, a_.detect_pilots, a_.ldpc_trials, a_.bch_corr, a_.bbframe_bytes) == \
                       (b_.detected_modcod, b_.detected_shortframes, b_.detected_pilots, b_.ldpc_trials, b_.bch_corrections, b_.bbframe_bytes)
            assert len(o) == len(g) and all(np.array_equal(x, y) for x, y in zip(o, g)), ('BBFRAMEs', ncall)
            stats_all += st_o
            want_all += o
    finally:
        dm.close()
    check_vcm_oracle(pls, bbs, stats_all, want_all)
