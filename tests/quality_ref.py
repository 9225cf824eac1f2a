"""Reference signal-quality estimators in numpy (float64), the definitions of include/dvbs2gpu.h (dvbs2gpu_frame_quality,
dvbs2gpu_dvbs_quality) written out independently of the kernels in csrc/quality.hip.

DVB-S2, per frame of tap 2 (PLL output): header positions 0..89 hold the derotated symbol transformed -- even i (im, re), odd i (-re, im) --
and payload / pilot positions the PL-descrambled symbol; pilots are (1+j)/sqrt2.  The header symbols come from the header demodulator's own
phase loop, so the header and the pilots each get their own complex gain (sigma^2 over both, K - 2 degrees of freedom with pilots), and the
payload's phase reference is the pilots' gain -- without pilots the header's magnitude at the PLL's own phase."""
import numpy as np

import orc

PILOT = (1 + 1j) / np.sqrt(2.0)


def sof():
    value = 0x18d2e82
    out = np.zeros(26, np.complex128)
    for s in range(26):
        angle = ((value >> (25 - s)) & 1) * 2 + (s & 1)
        out[s] = np.exp(1j * (np.pi / 4 + 2 * np.pi * angle / 4))
    return out


def plsc(pls):
    """the 64 scrambled PLS-code symbols of a PLS code (ETSI EN 302 307-1 5.5.2.4)"""
    g = [0x55555555, 0x33333333, 0x0f0f0f0f, 0x00ff00ff, 0x0000ffff, 0xffffffff]
    y = 0
    for row in range(6):
        if (pls >> (6 - row)) & 1:
            y ^= g[row]
    code = 0
    for bit in range(31, -1, -1):
        yi = (y >> bit) & 1
        code = (code << 2) | (yi << 1) | ((yi ^ 1) if pls & 1 else yi)
    code ^= 0x719d83c953422dfa
    out = np.zeros(64, np.complex128)
    for i in range(64):
        yi = (code >> (63 - i)) & 1
        nyi = yi ^ (i & 1)
        out[i] = complex(1 - 2 * nyi, 1 - 2 * yi) / np.sqrt(2.0)
    return out


def constellation(modcod, short=0, pilots=0):
    """unit-mean-energy points of a MODCOD's constellation (-> (points, is_psk))"""
    mp = orc.modcod_params(modcod, short, pilots)
    c = mp['constel']
    if c == 0:
        p = np.exp(1j * (np.pi / 4 + np.pi / 2 * np.arange(4)))
    elif c == 1:
        p = np.exp(1j * np.pi / 4 * np.arange(8))
    elif c == 2:
        g1 = mp['g1'] or 2.57
        p = np.concatenate([np.exp(1j * 2 * np.pi / 4 * (np.arange(4) + 0.5)), g1 * np.exp(1j * 2 * np.pi / 12 * (np.arange(12) + 0.5))])
    else:
        g1, g2 = mp['g1'] or 2.53, mp['g2'] or 4.30
        p = np.concatenate([np.exp(1j * 2 * np.pi / 4 * (np.arange(4) + 0.5)), g1 * np.exp(1j * 2 * np.pi / 12 * (np.arange(12) + 0.5)),
                            g2 * np.exp(1j * 2 * np.pi / 16 * np.arange(16))])
    return p / np.sqrt(np.mean(np.abs(p) ** 2)), c <= 1


def layout(pls):
    """(plframe, known positions, payload positions) of a data PLS code"""
    mp = orc.modcod_params(pls >> 2, (pls >> 1) & 1, pls & 1)
    pil = pls & 1
    blocks = mp['pilot_blocks'] if pil else 0
    known = list(range(90)) + [90 + (b + 1) * 1440 + b * 36 + i for b in range(blocks) for i in range(36)]
    j = np.arange(mp['slots'] * 90)
    payload = 90 + j + (36 * (j // 1440) if pil else 0)
    return mp['plframe'], np.array(known), payload


def frame(fr, pls):
    """one frame of tap 2 with PLS code `pls` -> dict of the dvbs2gpu_frame_quality fields"""
    fr = np.asarray(fr, np.complex64).astype(np.complex128)
    _, known, payload = layout(pls)
    hdr = fr[:90]
    i = np.arange(90)
    y_hdr = np.where(i & 1, -hdr.real + 1j * hdr.imag, hdr.imag + 1j * hdr.real)
    a_hdr = np.concatenate([sof(), plsc(pls)])
    y_pil = fr[known[90:]]
    P, K = y_pil.size, len(known)
    h_hdr = np.sum(y_hdr * np.conj(a_hdr)) / 90
    h_pil = np.sum(y_pil * np.conj(PILOT)) / P if P else 0j
    err = np.sum(np.abs(y_hdr - h_hdr * a_hdr) ** 2) + (np.sum(np.abs(y_pil - h_pil * PILOT) ** 2) if P else 0.0)
    sigma2 = err / (K - (2 if P else 1))
    g2 = (90 * np.abs(h_hdr) ** 2 + P * np.abs(h_pil) ** 2) / K
    h = h_pil if P else np.abs(h_hdr) + 0j        # the payload's phase reference
    pts, psk = constellation(pls >> 2, (pls >> 1) & 1, pls & 1)
    z = fr[payload] * np.conj(h) / np.abs(h) ** 2
    if psk:
        d = pts[np.argmax((z[:, None] * np.conj(pts)[None, :]).real, axis=1)]
    else:
        d = pts[np.argmin(np.abs(z[:, None] - pts[None, :]) ** 2, axis=1)]
    return dict(esn0_db=10 * np.log10(g2 / sigma2), mer_db=10 * np.log10(np.sum(np.abs(d) ** 2) / np.sum(np.abs(z - d) ** 2)),
                gain=np.sqrt(g2), phase=np.angle(h), known_symbols=K, payload_symbols=len(payload))


def frames(tap2, pls_list):
    """tap 2 of a call whose data frames had the PLS codes pls_list (in order) -> list of records"""
    out, pos = [], 0
    for pls in pls_list:
        n = layout(pls)[0]
        out.append(frame(tap2[pos:pos + n], pls))
        pos += n
    assert pos == len(tap2), (pos, len(tap2))
    return out


def dvbs(y):
    """DVB-S: symbols after the Costas loop of one call -> dict of the dvbs2gpu_dvbs_quality fields"""
    y = np.asarray(y, np.complex64).astype(np.complex128)
    if y.size == 0:
        return dict(esn0_db=np.nan, mer_db=np.nan, amplitude=np.nan, symbols=0)
    p = np.abs(y) ** 2
    m2, m4 = p.mean(), (p * p).mean()
    r = 2 * m2 * m2 - m4
    S = np.sqrt(r) if r >= 0 else -1.0
    N = m2 - S
    esn0 = 10 * np.log10(S / N) if (S > 0 and N > 0) else np.nan
    A = np.mean(np.abs(y.real) + np.abs(y.imag)) / 2
    d = A * (np.sign(y.real) + 1j * np.sign(y.imag))
    return dict(esn0_db=esn0, mer_db=10 * np.log10(np.sum(np.abs(d) ** 2) / np.sum(np.abs(y - d) ** 2)), amplitude=A, symbols=y.size)
