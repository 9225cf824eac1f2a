"""Signal-quality estimates (include/dvbs2gpu.h: dvbs2gpu_frame_quality, dvbs2gpu_dvbs_quality), CPU side: the numpy reference estimator
(tests/quality_ref.py) on the CPU oracle's receive chain against the transmitter's set Es/N0, and the new C ABI / ctypes / C++ host surface.

Bands, measured on the oracle (frames after the first two; transmitter cfo 2e-4, timing 0.2, phase 0.3; pilot frames with the pilot-aided loop):
  MODCOD 4 normal (QPSK 1/4):        mean Es/N0 -0.63 / -0.60 / -0.59 dB off the set 8 / 11 / 14 dB (per-frame std 0.23-0.28 dB)
  MODCOD 14 normal (8PSK 3/4):       -0.26 / -0.25 / -0.26 dB (std 0.26-0.50 dB)
  MODCOD 14 normal + pilots at 11 / 14 dB: -0.26 / -0.24 dB (std 0.22-0.24 dB; frames after the first three: the first frame counted at 11 dB
                                     still reads 0.4 dB, MER 4.1 dB -- the pilot-aided loop's acquisition -- and 10.4-11.0 dB from the next one on)
  DVB-S (M2M4 over 40 000 Costas symbols), rates 1/2 and 3/4: -0.06 ... -0.29 dB at 5 / 8 / 11 dB
So a mean lands within [-1.0, +0.3] dB of the set value (DVB-S: [-0.5, +0.3]) and a 3 dB step reads 3 +- 0.5 dB.
Left out, because the carrier loop never settles there (every frame's estimate lies several dB off, no BBFRAME decodes): MODCOD 14 normal
with pilots at 8 dB (Es/N0 -6.2 ... -0.5 dB, MER -9 ... 3 dB on every frame), MODCOD 18 normal with pilots (16APSK 2/3) at 8 / 11 / 14 dB (means
-2.6 / -3.9 / 3.1 dB, per-frame spread 2-7 dB) and MODCOD 27 short with pilots (32APSK 4/5) at 8 / 11 / 14 dB (means 2.6 / 5.5 / 6.2 dB,
spread 2.7-4.3 dB)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import orc
import orc_dvbs as od
import quality_ref as qr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG_DIR = os.path.join(ROOT, 'sdrpp-dvbs-demodulator_amd')
BAND_LO, BAND_HI = -1.0, 0.3
LEVELS = (8.0, 11.0, 14.0)
HELD = [(4, 0, 0, LEVELS, 2), (14, 0, 0, LEVELS, 2), (14, 0, 1, (11.0, 14.0), 3)]


def oracle_records(modcod, short, pilots, esn0, nframes=10, chunk=40000, skip=2):
    mp = orc.modcod_params(modcod, short, pilots)
    iq, _, _ = orc.transmit(modcod, short, pilots, nframes=nframes, seed=5 + modcod, esn0_db=esn0, cfo=2e-4, timing=0.2, phase0=0.3, lead_symbols=400)
    rx = orc.OracleRx(orc.default_cfg(modcod, short, pilots, pilot_aided=pilots))
    pls = modcod << 2 | short << 1 | pilots
    recs = []
    for a in range(0, iq.size, chunk):
        rx.process(iq[a:a + chunk])
        tap = rx.tap(2)
        recs += qr.frames(tap, [pls] * (tap.size // mp['plframe']))
    return recs[skip:]


@pytest.mark.parametrize('modcod,short,pilots,levels,skip', HELD)
def test_oracle_esn0_lands_in_band(modcod, short, pilots, levels, skip):
    means = []
    for es in levels:
        recs = oracle_records(modcod, short, pilots, es, skip=skip)
        assert len(recs) >= 6
        assert all(es - 1.5 <= r['esn0_db'] <= es + 0.7 for r in recs), [r['esn0_db'] for r in recs]
        m = np.mean([r['esn0_db'] for r in recs])
        assert es + BAND_LO <= m <= es + BAND_HI, (es, m)
        assert all(r['known_symbols'] == 90 + (36 * orc.modcod_params(modcod, short, pilots)['pilot_blocks'] if pilots else 0) for r in recs)
        means.append(m)
    for a, b in zip(means, means[1:]):
        assert abs((b - a) - 3.0) <= 0.5, means


def test_oracle_mer_follows_esn0():
    # decision-directed MER at these levels reads close to Es/N0 (few decision errors)
    for es in (11.0, 14.0):
        recs = oracle_records(4, 0, 0, es)
        mer, esn0 = np.mean([r['mer_db'] for r in recs]), np.mean([r['esn0_db'] for r in recs])
        assert abs(mer - esn0) < 1.0, (mer, esn0)


@pytest.mark.parametrize('rate', [0, 2])
def test_oracle_dvbs_m2m4_lands_in_band(rate):
    means = []
    for es in (5.0, 8.0, 11.0):
        iq, _ = od.dvbs_iq(rate, 60000, seed=3, esn0_db=es, cfo=1e-4, timing=0.2, phase0=0.3)
        y = od.OracleQpskAlt().process(iq)
        r = qr.dvbs(y[20000:])
        assert es - 0.5 <= r['esn0_db'] <= es + 0.3, (es, r)
        assert abs(r['mer_db'] - r['esn0_db']) < 1.0, r
        means.append(r['esn0_db'])
    for a, b in zip(means, means[1:]):
        assert abs((b - a) - 3.0) <= 0.5, means


def test_reference_estimator_on_known_noise():
    # a clean 8PSK frame plus complex Gaussian noise of known variance: the estimates recover it
    rng = np.random.default_rng(1)
    pls = 14 << 2 | 1
    plf, known, payload = qr.layout(pls)
    pts, _ = qr.constellation(14, 0, 1)
    fr = np.zeros(plf, np.complex128)
    hdr = np.concatenate([qr.sof(), qr.plsc(pls)])
    i = np.arange(90)
    fr[:90] = np.where(i & 1, -hdr.real + 1j * hdr.imag, hdr.imag + 1j * hdr.real)     # the tap's transform (its own inverse)
    fr[known[90:]] = qr.PILOT
    fr[payload] = pts[rng.integers(0, 8, payload.size)]
    g = 0.8 * np.exp(0.3j)
    sigma2 = 10 ** (-20 / 10) * abs(g) ** 2
    noise = np.sqrt(sigma2 / 2) * (rng.standard_normal(plf) + 1j * rng.standard_normal(plf))
    y = g * fr + noise
    y[:90] = np.where(i & 1, -(g * hdr + noise[:90]).real + 1j * (g * hdr + noise[:90]).imag,
                      (g * hdr + noise[:90]).imag + 1j * (g * hdr + noise[:90]).real)
    r = qr.frame(y.astype(np.complex64), pls)
    assert abs(r['esn0_db'] - 20.0) < 0.6 and abs(r['mer_db'] - 20.0) < 0.3, r
    assert abs(r['gain'] - 0.8) < 0.01 and abs(r['phase'] - 0.3) < 0.01, r
    assert r['known_symbols'] == 90 + 36 * 14 and r['payload_symbols'] == 21600


def test_quality_abi(pkg):
    lib = pkg.load_library()
    assert C.sizeof(pkg.FrameQuality) == 24 and C.sizeof(pkg.DvbsQuality) == 16
    for name in ('dvbs2gpu_demod_set_quality', 'dvbs2gpu_demod_get_quality', 'dvbs2gpu_dvbs_demod_set_quality', 'dvbs2gpu_dvbs_demod_get_quality'):
        assert hasattr(lib, name) and name in pkg.PROTOTYPES
    err = lib.dvbs2gpu_demod_set_quality(None, 1)
    assert err < 0
    assert lib.dvbs2gpu_demod_get_quality(None, None, 0) == err
    assert lib.dvbs2gpu_dvbs_demod_set_quality(None, 1) == err
    assert lib.dvbs2gpu_dvbs_demod_get_quality(None, None) == err
    rec = np.zeros(1, pkg._quality_dtype(pkg.FrameQuality))
    assert rec.itemsize == 24 and list(rec.dtype.names) == ['esn0_db', 'mer_db', 'gain', 'phase', 'known_symbols', 'payload_symbols']


def test_quality_host_program_builds(pkg, tmp_path):
    exe = tmp_path / 'quality_host'
    cmd = ['g++', '-std=c++17', '-O1', '-Wall', '-Wextra', '-Werror', '-I' + os.path.join(ROOT, 'include'), os.path.join(ROOT, 'tests', 'cpp', 'quality_host.cpp'),
           '-o', str(exe), '-L' + PKG_DIR, '-ldvbs2gpu', '-Wl,-rpath,' + PKG_DIR, '-pthread']
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert subprocess.run([str(exe)], capture_output=True).returncode == 2
