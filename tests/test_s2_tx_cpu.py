"""The modulator's rules (csrc/s2_tx_rules.h) on the CPU, through the library's host-only entry points dvbs2gpu_s2_tx_host / dvbs2gpu_s2_tx_sizes, no GPU.
Symbols: equal to the oracle transmitter's (oracle/s2chain.cpp: s2_transmit) bit for bit, from the code words of the oracle's FEC encoder.  IQ: within a bound
derived from the number formats, not measured.  Noise: first and second moments."""
import numpy as np
import pytest

import orc
import s2_tx_cases as tc

SEED = 5

# (name, modcod, short, pilots): one MODCOD per constellation, 8PSK 3/5 (columns 2, 1, 0), a short 16APSK (column offset 4050 bits: no byte multiple; 4050 payload
# symbols: a last group of 2), 32APSK normal with pilots (144 slots: no pilot block behind the last one), QPSK short with pilots (8100 symbols: a last group of 4)
CCM = [('qpsk_1_2', 4, 0, 0), ('8psk_2_3', 13, 0, 0), ('16apsk_3_4', 19, 0, 0), ('32apsk_4_5', 25, 0, 0), ('8psk_3_5', 12, 0, 0), ('16apsk_2_3_short', 18, 1, 0),
       ('32apsk_3_4_pilots', 24, 0, 1), ('qpsk_1_2_short_pilots', 4, 1, 1)]


@pytest.mark.parametrize('name,modcod,short,pilots', CCM, ids=[c[0] for c in CCM])
def test_symbols_equal_the_oracle_transmitters(pkg, name, modcod, short, pilots):
    nframes = 2         # (the scrambler index restarts behind the second header)
    iq, bb, want = orc.transmit(modcod, short, pilots, nframes=nframes, seed=SEED)
    pls = [tc.pls_code(modcod, short, pilots)] * nframes
    code, bbs = tc.code_words(pls, SEED)
    assert np.array_equal(np.stack(bbs), bb)        # the same BBFRAMEs went in
    sz = pkg.s2_tx_sizes(pls)
    mp = orc.modcod_params(modcod, short, pilots)
    assert sz == {'symbols': nframes * mp['plframe'], 'bbframe_bytes': nframes * mp['kbch'] // 8, 'code_bytes': nframes * mp['N'] // 8}
    got, _ = pkg.s2_tx_host(pls, code, want_iq=False)
    assert tc.same_bits(got, want)


VCM = [tc.pls_code(4, 1, 1), tc.pls_code(0), tc.pls_code(13, 0, 0), tc.pls_code(18, 1, 0), tc.pls_code(0, 1, 1), tc.pls_code(24, 1, 1)]


def test_vcm_list_with_dummy_frames_equals_the_oracles(pkg):
    iq, want = tc.transmit_vcm_symbols(VCM, len(VCM), seed=SEED)
    code, bbs = tc.code_words(VCM, SEED)
    _, obb = orc.transmit_vcm(VCM, len(VCM), seed=SEED)
    assert all((a is None and b is None) or np.array_equal(a, b) for a, b in zip(bbs, obb))
    got, _ = pkg.s2_tx_host(VCM, code, want_iq=False)
    assert got.size == sum(orc.pls_info(p)[0] for p in VCM) and tc.same_bits(got, want)


def rrc(t, beta):
    t = np.asarray(t, np.float64)
    x = 4.0 * beta * t
    with np.errstate(divide='ignore', invalid='ignore'):
        v = (np.sin(np.pi * t * (1.0 - beta)) + x * np.cos(np.pi * t * (1.0 + beta))) / (np.pi * t * (1.0 - x * x))
    v = np.where(np.abs(t) < 1e-9, 1.0 + beta * (4.0 / np.pi - 1.0), v)
    edge = (beta / np.sqrt(2.0)) * ((1.0 + 2.0 / np.pi) * np.sin(np.pi / (4.0 * beta)) + (1.0 - 2.0 / np.pi) * np.cos(np.pi / (4.0 * beta)))
    return np.where(np.abs(np.abs(t) - 1.0 / (4.0 * beta)) < 1e-9, edge, v)


def iq_bound(symbols, timing, beta=0.35):
    """35 * 2^-24 * max_p sum_k |h_p[k]| * max |symbol|: one unit for the fp32 taps, 33 for the 33-term fp32 chain, one for the oracle's single rounding of its
    double sum; per component, and |symbol| bounds both components"""
    k = np.arange(-16, 17)
    taps = np.stack([rrc((p - timing) / 2.0 - k, beta).astype(np.float32) for p in (0, 1)])
    return 35.0 * 2.0 ** -24 * float(np.abs(taps.astype(np.float64)).sum(axis=1).max()) * float(np.abs(symbols).max())


@pytest.mark.parametrize('timing', [0.0, 0.3])
@pytest.mark.parametrize('circular', [0, 1])
def test_iq_within_the_derived_bound_of_the_oracles(pkg, timing, circular):
    modcod, short, pilots = 19, 1, 1        # 16APSK short with pilots: three amplitudes
    want, bb, osym = orc.transmit(modcod, short, pilots, nframes=2, seed=SEED, timing=timing, circular=circular)
    pls = [tc.pls_code(modcod, short, pilots)] * 2
    code, _ = tc.code_words(pls, SEED)
    sym, got = pkg.s2_tx_host(pls, code, rolloff=0.35, timing=timing, circular=circular)
    assert tc.same_bits(sym, osym)
    bound = iq_bound(sym, timing)
    err = max(float(np.abs(got.real.astype(np.float64) - want.real).max()), float(np.abs(got.imag.astype(np.float64) - want.imag).max()))
    print('timing %.1f circular %d: max error %.3g, bound %.3g' % (timing, circular, err, bound))
    assert 0 < bound < 2e-5 and err <= bound
    # the block's ends are where the two modes differ
    other = pkg.s2_tx_host(pls, code, rolloff=0.35, timing=timing, circular=not circular)[1]
    assert not np.array_equal(other[:32], got[:32]) and np.array_equal(other[64:-64], got[64:-64])


def test_esn0_200_without_offsets_changes_nothing(pkg):
    pls = [tc.pls_code(0)] * 2
    a = pkg.s2_tx_host(pls, np.zeros(0, np.uint8))[1]
    b = pkg.s2_tx_host(pls, np.zeros(0, np.uint8), esn0_db=200.0, cfo=0.0, phase0=0.0, seed=9)[1]
    assert tc.same_bits(a, b)


def test_noise_moments(pkg):
    n = 1 << 20
    pls = [tc.pls_code(0)] * (-(-n // (2 * 3330)))         # dummy frames: no code words needed
    clean = pkg.s2_tx_host(pls, np.zeros(0, np.uint8))[1]
    esn0_db = 3.0
    sigma = np.sqrt(10.0 ** (-esn0_db / 10.0))              # per dimension, the oracle transmitter's convention for 2 sps
    for stream, seed in ((0, 1), (3, 1), (0, 77)):
        noisy = pkg.s2_tx_host(pls, np.zeros(0, np.uint8), esn0_db=esn0_db, seed=seed, stream=stream)[1]
        w = (noisy.astype(np.complex128) - clean.astype(np.complex128))[:n]
        for part in (w.real, w.imag):
            assert abs(part.mean()) <= 6.0 * sigma / np.sqrt(n)
            assert abs(part.var() - sigma ** 2) <= 6.0 * sigma ** 2 * np.sqrt(2.0 / n)
        rho = float((w.real * w.imag).mean() / sigma ** 2)
        assert abs(rho) <= 6.0 / np.sqrt(n)
        if stream == 0 and seed == 1:
            first = w
        else:
            assert not np.array_equal(w[:64], first[:64])   # stream index and seed both enter the generator


def test_cfo_and_phase_rotate_the_block(pkg):
    pls = [tc.pls_code(0)]
    clean = pkg.s2_tx_host(pls, np.zeros(0, np.uint8))[1].astype(np.complex128)
    cfo, ph = 1e-3, 0.7
    got = pkg.s2_tx_host(pls, np.zeros(0, np.uint8), esn0_db=200.0, cfo=cfo, phase0=ph)[1]
    want = clean * np.exp(1j * (ph + cfo * np.arange(clean.size)))
    assert np.abs(got - want).max() < 1e-5      # (sincosf_det: 2.5 * 2^-24; amplitudes near 1)


def test_sizes_and_refusals(pkg):
    lib = pkg.load_library()
    assert pkg.s2_tx_sizes([]) == {'symbols': 0, 'bbframe_bytes': 0, 'code_bytes': 0}
    assert pkg.s2_tx_sizes([tc.pls_code(0), tc.pls_code(0, 1, 1)]) == {'symbols': 6660, 'bbframe_bytes': 0, 'code_bytes': 0}
    total = {'symbols': 0, 'bbframe_bytes': 0, 'code_bytes': 0}
    for p in tc.VALID_PLS:
        one = pkg.s2_tx_sizes([p])
        plf, kb = orc.pls_info(p)
        assert one['symbols'] == plf and one['bbframe_bytes'] == kb and one['code_bytes'] == (0 if p < 4 else (2025 if p & 2 else 8100))
        for k in total:
            total[k] += one[k]
    assert pkg.s2_tx_sizes(tc.VALID_PLS) == total and len(tc.VALID_PLS) == 4 + 4 * 28 - 2 * 4
    for p in tc.INVALID_PLS + [-1, 128]:
        with pytest.raises(pkg.Dvbs2GpuError, match='no valid PLS code'):
            pkg.s2_tx_sizes([tc.pls_code(4), p])
    with pytest.raises(pkg.Dvbs2GpuError, match='roll-off'):
        pkg.s2_tx_host([0], np.zeros(0, np.uint8), rolloff=0.3)
    with pytest.raises(pkg.Dvbs2GpuError, match='timing'):
        pkg.s2_tx_host([0], np.zeros(0, np.uint8), timing=float('nan'))
    for bad in (float('-inf'), -1e9, float('nan')):
        with pytest.raises(pkg.Dvbs2GpuError, match='channel parameter'):
            pkg.s2_tx_host([0], np.zeros(0, np.uint8), esn0_db=bad)
    assert lib.dvbs2gpu_s2_tx_sizes(None, 1, None, None, None) == -1 and b'null pointer' in lib.dvbs2gpu_last_error()
    assert lib.dvbs2gpu_s2_tx_sizes(None, -1, None, None, None) == -1 and b'negative' in lib.dvbs2gpu_last_error()
    for name in ('dvbs2gpu_pl_frame_batch', 'dvbs2gpu_pulse_shape_batch', 'dvbs2gpu_channel_batch', 'dvbs2gpu_s2_modulate_batch'):
        assert hasattr(lib, name) and name in pkg.PROTOTYPES
    # without a context the device calls answer with the argument error, they do not crash
    assert lib.dvbs2gpu_pl_frame_batch(None, None, 0, None, None, None, 1, None, None) == -1 and b'no context' in lib.dvbs2gpu_last_error()
    assert lib.dvbs2gpu_s2_modulate_batch(None, None, 0, None, 1, 0.35, 0.0, 0, None, None, None) == -1 and b'no context' in lib.dvbs2gpu_last_error()
