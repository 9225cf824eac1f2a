"""Constructed error patterns for the outer (BCH) code of every DVB-S2 FEC code: plain numpy and Python integers, no GPU.

patterns(rate, short) -> a deterministic list of Pattern(name, frame, flips, sent) for one (rate, short):
  frame   the K / 8 bytes handed to a decoder (K = nbch, the LDPC message; the first kbch bits are the BCH message, P = K - kbch parity bits follow)
  flips   the frame bits that differ from the transmitted codeword, or None where the pattern is not built from frame bits (`shortened`)
  sent    the transmitted codeword
Frame bit x is bit 7 - x % 8 of byte x // 8 and the coefficient of x^(K - 1 - x) of the received polynomial.

The positions follow the places where the kernels of csrc/bch_kernel.hip depend on (nbch, kbch): the syndrome kernel's 256 chunks of
chunk = ceil(nbytes / 256) bytes (chunk seams, the last chunk that holds data, the idle threads behind it), the two ends of the frame, the
message / parity seam, the closed forms for locators of degree 1 and 2, the Chien search for degree >= 3, and the rejection of roots that lie
in the shortened part of the code, in front of frame bit 0.

`shortened` patterns: the code is the unshortened BCH code of length N = 2^m - 1 with its first short_by = N - K message bits fixed to zero, so one
error at the virtual position -(s + 1) -- s + 1 bits in front of the frame -- is the polynomial x^(K + s).  No frame can carry it, but
r_s = x^(K + s) mod g has degree < P and the same syndromes (g's roots are the decoder's roots), and r_s fits into the parity bits.  g(x) comes from
the encoder alone: the message x^0 (only bit kbch - 1 set) has the parity x^P mod g, so g = x^P + parity.  A decoder sees a single error (or, with
further flips in the frame, 2 or 4 errors) of which one lies in the shortened part, and has to leave the frame as it is."""
import collections
import functools

import numpy as np

import orc

Pattern = collections.namedtuple('Pattern', 'name frame flips sent')

# families whose outcome follows from the code alone: `len(flips)` corrections and the transmitted codeword back
CORRECTABLE = ('clean', 'single', 'pair', 't-1', 't')


def family(name):
    return name.split('@')[0].split('/')[0]


def flip(frame, positions):
    for x in positions:
        frame[int(x) // 8] ^= 1 << (7 - int(x) % 8)


def codeword(rate, short, seed):
    p = orc.fec_params(rate, short)
    fr = np.zeros(p['K'] // 8, np.uint8)
    orc.lib().orc_make_bbframe(fr, p['kbch'], seed)
    orc.lib().orc_bch_encode(rate, short, fr)
    return fr


@functools.lru_cache(maxsize=None)
def gf_tables(m):
    """(EXP, LOG) of GF(2^m) over the DVB-S2 field polynomials (EN 302 307-1 5.3.1: the first minimal polynomial of the normal and the short code)"""
    poly = {16: 0x1002D, 14: 0x402B}[m]
    n = (1 << m) - 1
    exp, log = [0] * n, [0] * (n + 1)
    a = 1
    for i in range(n):
        exp[i], log[a] = a, i
        a <<= 1
        if a >> m:
            a ^= poly
    return exp, log


def generator(rate, short):
    """g(x) as a Python integer (bit k = coefficient of x^k), from the encoder alone"""
    p = orc.fec_params(rate, short)
    P = p['K'] - p['kbch']
    fr = np.zeros(p['K'] // 8, np.uint8)
    flip(fr, [p['kbch'] - 1])
    orc.lib().orc_bch_encode(rate, short, fr)
    assert p['kbch'] % 8 == 0 and P % 8 == 0
    return (1 << P) | int.from_bytes(fr[p['kbch'] // 8:].tobytes(), 'big')


def x_pow_mod(e, g, P):
    """x^e mod g, shift and reduce"""
    r = 1
    for _ in range(e):
        r <<= 1
        if r >> P:
            r ^= g
    return r


def syndromes(rate, short, frame):
    p = orc.fec_params(rate, short)
    syn = np.zeros(64, np.uint16)
    orc.lib().orc_bch_syndromes(rate, short, np.ascontiguousarray(frame), syn)
    return [int(v) for v in syn[:2 * p['t']]]


def chunking(p):
    """(nbytes, chunk, index of the last chunk that holds data) of the syndrome kernel's cut of a frame into 256 chunks"""
    nbytes = p['K'] // 8
    chunk = (nbytes + 255) // 256
    return nbytes, chunk, (nbytes - 1) // chunk


def chunk_seams(p, n):
    """n chunk indices spread over 1..last chunk that holds data, that one included"""
    _, _, last = chunking(p)
    return sorted({int(round(c)) for c in np.linspace(1, last, n)})


def shortened_shifts(p):
    short_by = ((1 << p['m']) - 1) - p['K']
    return sorted({s for s in (0, 1, short_by // 2, short_by - 1) if 0 <= s < short_by})


@functools.lru_cache(maxsize=None)
def patterns(rate, short):
    p = orc.fec_params(rate, short)
    K, kbch, t, m = p['K'], p['kbch'], p['t'], p['m']
    P, N = K - kbch, (1 << m) - 1
    assert P == m * t
    nbytes, chunk, last = chunking(p)
    rng = np.random.default_rng(7000 + 2 * rate + short)
    out = []
    seed = [100 * (2 * rate + short)]

    def keep(name, fr, flips, sent):
        fr.setflags(write=False)
        sent.setflags(write=False)
        out.append(Pattern(name, fr, flips, sent))

    def add(name, positions):
        seed[0] += 1
        sent = codeword(rate, short, seed[0])
        positions = sorted(int(x) for x in positions)
        assert len(set(positions)) == len(positions) and (not positions or (0 <= positions[0] and positions[-1] < K)), (name, positions)
        fr = sent.copy()
        flip(fr, positions)
        keep(name, fr, tuple(positions), sent)

    add('clean/first', [])

    # ---- one error: the degree-1 closed form
    seams = chunk_seams(p, 8)
    single = [0, 7, 8, K - 1, K - 8, kbch - 1, kbch]
    for c in seams:
        single += [8 * c * chunk - 1, 8 * c * chunk]
    single.append(min(8 * (last + 1) * chunk, K) - 1)            # the last bit of the last chunk that holds data
    for x in dict.fromkeys(single):
        add('single@%d' % x, [x])

    # ---- two errors: the degree-2 closed form (locations from the Artin-Schreier map, not from the Chien search)
    cs = 8 * seams[len(seams) // 2] * chunk
    pairs = [(0, 1), (0, K - 1), (K - 2, K - 1), (cs - 1, cs), (kbch - 1, kbch), (kbch + 3, K - 5)]
    pairs += [tuple(rng.choice(K, 2, replace=False)) for _ in range(3)]
    for a, b in pairs:
        add('pair@%d,%d' % (min(a, b), max(a, b)), [a, b])

    # ---- t - 1 and t errors: the Chien search
    seam_bits = [8 * c * chunk - (k & 1) for k, c in enumerate(chunk_seams(p, 12))]
    assert len(set(seam_bits)) == 12
    for ne, tag in ((t - 1, 't-1'), (t, 't')):
        add('%s/run16-start' % tag, rng.choice(16, ne, replace=False))
        add('%s/run16-end' % tag, K - 16 + rng.choice(16, ne, replace=False))
        add('%s/chunk-seams' % tag, seam_bits[:ne])
        add('%s/parity' % tag, kbch + rng.choice(P, ne, replace=False))
        for k in range(2):
            add('%s/random%d' % (tag, k), rng.choice(K, ne, replace=False))

    # ---- a root in the shortened part: x^(K + s) mod g in the parity bits
    g = generator(rate, short)
    exp, log = gf_tables(m)
    for s in shortened_shifts(p):
        r = np.frombuffer(x_pow_mod(K + s, g, P).to_bytes(P // 8, 'big'), np.uint8)
        extra = [int(x) for x in rng.choice(K, 3, replace=False)]
        for tag, flips in (('deg1', []), ('deg2', extra[:1]), ('chien', extra)):
            seed[0] += 1
            sent = codeword(rate, short, seed[0])
            fr = sent.copy()
            fr[kbch // 8:] ^= r
            if not flips:
                # the construction, before anything is decoded: the syndromes of ONE bit at x^(K + s) of the unshortened code, S_k = alpha^(k (K + s))
                S = syndromes(rate, short, fr)
                assert S[0] != 0 and K + s < N
                assert all(S[k - 1] == exp[k * (K + s) % N] for k in range(1, 2 * t + 1)), (rate, short, s)
                assert all(S[2 * k - 1] == exp[2 * log[S[k - 1]] % N] for k in range(1, t + 1))          # S_2k == S_k^2
            flip(fr, flips)
            keep('shortened/%s@-%d' % (tag, s + 1), fr, None, sent)

    # ---- more errors than the code corrects: whatever the reference does (too few roots -> -1, or a miscorrection)
    for ne in (t + 1, t + 2, 2 * t, 40):
        for k in range(3):
            add('beyond/%d-%d' % (ne, k), rng.choice(K, ne, replace=False))

    add('clean/last', [])
    return tuple(out)


@functools.lru_cache(maxsize=None)
def oracle_outcomes(rate, short):
    """(return values int32 [n], frames after orc_bch_decode uint8 [n, K / 8]) of patterns(rate, short), each decoded once"""
    pats = patterns(rate, short)
    frames = np.stack([q.frame for q in pats])
    ret = np.zeros(len(pats), np.int32)
    for n in range(len(pats)):
        ret[n] = orc.lib().orc_bch_decode(rate, short, frames[n])
    frames.setflags(write=False)
    ret.setflags(write=False)
    return ret, frames


def check_independent(rate, short, ret, frames):
    """what follows from the code alone, for a decoder's return values and output frames over patterns(rate, short)"""
    for n, q in enumerate(patterns(rate, short)):
        fam = family(q.name)
        if fam in CORRECTABLE:
            assert ret[n] == len(q.flips), (rate, short, q.name, int(ret[n]))
            assert np.array_equal(frames[n], q.sent), (rate, short, q.name)
        elif fam == 'shortened':
            assert ret[n] == -1, (rate, short, q.name, int(ret[n]))
            assert np.array_equal(frames[n], q.frame), (rate, short, q.name)
        else:
            assert fam == 'beyond', q.name
