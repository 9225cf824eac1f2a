"""Constructed error patterns for the DVB-S outer code RS(204,188): plain numpy and Python integers, no GPU.

patterns() -> a deterministic tuple of Pattern(name, packet, flips, sent, expect):
  packet  the 204 bytes handed to a decoder (188 message bytes, 16 parity bytes)
  flips   the coefficient indices (below 204) at which the packet differs from `sent`, ascending
  sent    the transmitted codeword c
  expect  Expect(status, corrected, rs_err, padding) -- what follows from the code alone -- or None (family `beyond`)
            status     1: the decoder produces a message
            corrected  the 204 bytes after the in-place correction
            rs_err     the message bytes that the correction changed (what the reference's wrapper returns)
            padding    how many of the decoder's error locations lie in the zero padding (coefficient indices 204 .. 254)

The code is RS(255,239) over GF(256) (polynomial 0x11d, generator roots alpha^0 .. alpha^15) shortened by 51 leading zero bytes.  Coefficient
index i of the received polynomial is packet[203 - i] for i < 204 (so the 16 parity bytes are the indices 0 .. 15 and packet[0] is index 203);
the indices 204 .. 254 are the padding.  The syndromes are S_r = sum_i e_i alpha^(r i), r = 0 .. 15, over the errors e_i.

Families (the part of a name in front of '/' or '@'):
  clean       codewords
  single      one error at every one of the 204 positions: the log/exp conventions at both ends (index 0 <-> root 1 <-> packet[203]) and at
              every lane seam of the kernel's 64-lane coefficient layout
  zero-syn    k + 1 errors whose values are solved so that S_0 .. S_(k-1) = 0 and S_k != 0: Berlekamp-Massey starts with k zero discrepancies
  t-1, t      7 and 8 errors: the full Chien search and all Forney lanes
  miscorrect  a codeword d of weight 17 on a chosen support A u B (|A| + |B| = 17, |B| <= 8, A inside the packet); the packet is c + d|A.  It lies
              at distance |B| from the codeword c + d, so every bounded-distance decoder returns c + d, by "correcting" the B positions.  Those
              of them that lie in the padding are not part of the packet: the 204 bytes that come out are c + d restricted to the packet, and
              the wrapper counts the B positions with index 16 .. 203.  d is the null vector of the 16 x 17 Vandermonde system
              sum_j d_j alpha^(r i_j) = 0 (r = 0 .. 15); by the MDS property all 17 values are non-zero (asserted).
  beyond      9 .. 204 random errors: whatever the reference does (it gives up, or -- about once in 8! packets -- finds another codeword).  The only
              family without an independent expectation."""
import collections
import functools

import numpy as np

import orc_dvbs_tail as ot
from orc_dvbs import P, VP

Pattern = collections.namedtuple('Pattern', 'name packet flips sent expect')
Expect = collections.namedtuple('Expect', 'status corrected rs_err padding')
Outcome = collections.namedtuple('Outcome', 'status message rs_err')

# (|A|, |B|) of the weight-17 codewords
SPLITS = ((9, 8), (10, 7), (12, 5), (16, 1))
BEYOND = (9, 10, 16, 17, 40, 204)
# coefficient indices on both sides of the seams of the kernel's layout (lane + 64 q), and the two ends
LANE_SEAMS = (63, 64, 127, 128, 191, 192, 0, 203)


def family(name):
    return name.split('@')[0].split('/')[0]


# ---- GF(256): orc_dvbs_tail's tables (log 1 = 0 there)
def gexp(k):
    return int(ot._EXP[k % 255])


def ginv(a):
    assert a != 0
    return int(ot._EXP[255 - ot._LOG[a]])


def vandermonde(indices, nrows):
    """row r, column j: alpha^(r * indices[j])"""
    return [[gexp(r * i) for i in indices] for r in range(nrows)]


def null_vector(M):
    """the v with M v = 0 and v[-1] = 1 for a k x (k + 1) matrix whose first k columns are independent (Gauss-Jordan over GF(256))"""
    M = [list(r) for r in M]
    k = len(M)
    assert all(len(r) == k + 1 for r in M)
    for c in range(k):
        piv = next(r for r in range(c, k) if M[r][c])
        M[c], M[piv] = M[piv], M[c]
        inv = ginv(M[c][c])
        M[c] = [ot.gmul(x, inv) for x in M[c]]
        for r in range(k):
            if r != c and M[r][c]:
                f = M[r][c]
                M[r] = [x ^ ot.gmul(f, y) for x, y in zip(M[r], M[c])]
    return [M[r][k] for r in range(k)] + [1]           # (characteristic 2: minus is plus)


def syndromes(packet, padding=None):
    """S_0 .. S_15 of a 204-byte packet (and, where given, of error values {index: value} in the padding), straight from the definition"""
    coeff = {203 - k: int(b) for k, b in enumerate(packet) if b}
    coeff.update(padding or {})
    S = []
    for r in range(16):
        s = 0
        for i, c in coeff.items():
            s ^= ot.gmul(c, gexp(r * i))
        S.append(s)
    return S


def apply_errors(packet, errors):
    """packet with {coefficient index: value} added; indices in the padding are not part of the packet"""
    out = packet.copy()
    for i, v in errors.items():
        assert 0 <= i < 255 and 0 < v < 256
        if i < 204:
            out[203 - i] ^= v
    return out


def codeword(rng, first=0x47):
    msg = rng.integers(0, 256, 188, dtype=np.uint8)
    msg[0] = first
    return ot.rs_encode_204(msg)


def weight17(A, B):
    """{index: value} of the codeword of RS(255,239) with support A u B"""
    idx = list(A) + list(B)
    assert len(idx) == 17 and len(set(idx)) == 17 and all(0 <= i < 204 for i in A) and all(0 <= i < 255 for i in B)
    v = null_vector(vandermonde(idx, 16))
    assert all(v), 'a codeword of weight 17 has 17 non-zero values'
    return dict(zip(idx, v))


def b_placements(rng, nb):
    """(name, the B positions that go into the padding) for a B part of nb positions; the rest of B lies inside the packet"""
    pad = [int(x) for x in 204 + rng.choice(51, 8, replace=False)]
    out = [('inside', [])]
    out.append(('pad204', [204]))
    out.append(('pad254', [254]))
    if nb > 4:
        out.append(('pad4', pad[:4]))
    if nb > 1:
        out.append(('padall', pad[:nb]))
    return out


@functools.lru_cache(maxsize=None)
def patterns():
    rng = np.random.default_rng(20488)
    out = []

    def keep(name, packet, sent, expect):
        flips = tuple(int(203 - k) for k in np.flatnonzero(packet != sent)[::-1])
        for a in (packet, sent) + ((expect.corrected,) if expect else ()):
            a.setflags(write=False)
        out.append(Pattern(name, packet, flips, sent, expect))

    def correctable(name, sent, errors):
        """errors {index: value} inside the packet, at most 8: the decoder restores `sent`"""
        assert 0 <= len(errors) <= 8 and all(i < 204 for i in errors)
        packet = apply_errors(sent, errors)
        keep(name, packet, sent, Expect(1, sent.copy(), sum(i >= 16 for i in errors), 0))

    def values(n):
        return [int(v) for v in rng.integers(1, 256, n)]

    def at(indices):
        indices = [int(i) for i in indices]
        return dict(zip(indices, values(len(indices))))

    # ---- clean (the 0xB8 codeword comes first: it starts the energy-dispersal generator for everything behind it)
    correctable('clean/b8', codeword(rng, 0xB8), {})
    for k in range(3):
        correctable('clean/random%d' % k, codeword(rng), {})
    correctable('clean/zero', np.zeros(204, np.uint8), {})

    # ---- one error at every position
    for i in range(204):
        v = (0x01, 0x80, 0xFF, int(rng.integers(1, 256)))[i % 4]
        correctable('single@%d' % i, codeword(rng), {i: v})

    # ---- leading zero syndromes
    for k in (1, 2, 3):
        ends = [0, 203, 1, 202][:k + 1]
        for tag, idx in (('random0', rng.choice(204, k + 1, replace=False)), ('random1', rng.choice(204, k + 1, replace=False)), ('ends', ends)):
            idx = [int(i) for i in idx]
            v = null_vector(vandermonde(idx, k))
            scale = int(rng.integers(1, 256))
            errors = {i: ot.gmul(x, scale) for i, x in zip(idx, v)}
            sent = codeword(rng)
            S = syndromes(apply_errors(sent, errors))
            assert not any(S[:k]) and S[k] != 0, (k, tag, S)
            correctable('zero-syn/%d-%s' % (k, tag), sent, errors)

    # ---- t - 1 and t errors
    for ne, tag in ((7, 't-1'), (8, 't')):
        correctable('%s/msg-run' % tag, codeword(rng), at(203 - rng.choice(8, ne, replace=False)))              # message bytes 0 .. 7
        correctable('%s/parity' % tag, codeword(rng), at(rng.choice(16, ne, replace=False)))                    # rs_err 0, packet restored
        correctable('%s/msg-parity-seam' % tag, codeword(rng), at(203 - (184 + rng.choice(8, ne, replace=False))))   # bytes 184 .. 191
        correctable('%s/lane-seams' % tag, codeword(rng), at(LANE_SEAMS[:ne]))
        for k in range(2):
            correctable('%s/random%d' % (tag, k), codeword(rng), at(rng.choice(204, ne, replace=False)))

    # ---- miscorrections: c + d|A comes back as c + d
    for na, nb in SPLITS:
        for tag, pad in b_placements(rng, nb):
            inside = [int(i) for i in rng.choice(204, na + nb - len(pad), replace=False)]
            A, B = inside[:na], inside[na:] + pad
            d = weight17(A, B)
            sent = codeword(rng)
            packet = apply_errors(sent, {i: d[i] for i in A})
            # the construction, before anything is decoded: the packet and the B values (those in the padding included) add up to a codeword
            assert any(syndromes(packet))
            assert not any(syndromes(apply_errors(packet, {i: d[i] for i in B}), {i: d[i] for i in B if i >= 204}))
            corrected = apply_errors(sent, d)
            keep('miscorrect/%d+%d-%s' % (na, nb, tag), packet, sent,
                 Expect(1, corrected, sum(16 <= i < 204 for i in B), sum(i >= 204 for i in B)))

    # ---- more errors than the code corrects
    for ne in BEYOND:
        for k in range(3):
            sent = codeword(rng)
            keep('beyond/%d-%d' % (ne, k), apply_errors(sent, at(rng.choice(204, ne, replace=False))), sent, None)

    assert len({q.name for q in out}) == len(out)
    assert 10 * sum(family(q.name) == 'beyond' for q in out) < len(out)
    return tuple(out)


def family_counts():
    return dict(collections.Counter(family(q.name) for q in patterns()))


def padded(packets):
    """packets [n, 204] -> [n, 255]: the 51 leading zeros of the wrapper (dvbs_reedsolomon.h:27-29)"""
    return np.concatenate([np.zeros((len(packets), 51), np.uint8), packets], axis=1)


@functools.lru_cache(maxsize=None)
def oracle_outcomes():
    """Outcome(status uint8 [n], message uint8 [n, 188], rs_err int32 [n]) of patterns(), each decoded in a wrapper of its own: status from
    rs255_decode; message = the wrapper's output where it decoded, the received message where it gave up (the bytes a decoder that works in
    place leaves behind); rs_err = the wrapper's return value (after a failure in a fresh wrapper: the non-zero message bytes)"""
    o = ot.L()
    pats = patterns()
    status, rs_err = np.zeros(len(pats), np.uint8), np.zeros(len(pats), np.int32)
    message = np.zeros((len(pats), 188), np.uint8)
    enc = padded(np.stack([q.packet for q in pats]))
    for n, q in enumerate(pats):
        msg = np.zeros(239, np.uint8)
        status[n] = o.orc_rs255_decode(P(np.ascontiguousarray(enc[n])), P(msg)) == 239
        h = VP(o.orc_dvbsrs_create())
        data = q.packet.copy()
        rs_err[n] = o.orc_dvbsrs_decode(h, P(data))
        o.orc_dvbsrs_destroy(h)
        message[n] = data[:188] if status[n] else q.packet[:188]
        assert not status[n] or np.array_equal(data[:188], msg[51:])
    for a in (status, message, rs_err):
        a.setflags(write=False)
    return Outcome(status, message, rs_err)


HighDegree = collections.namedtuple('HighDegree', 'order packet sent ret message')


@functools.lru_cache(maxsize=None)
def high_degree():
    """packets that the reference decodes with an error locator of degree 9 (tests/golden/make_rs_high_degree.py): the packet, the codeword it was
    made from, and what the reference's wrapper -- a fresh one per packet -- returned and handed out"""
    import json
    import os
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'rs_high_degree.json')) as f:
        G = json.load(f)
    arr = lambda h: np.frombuffer(bytes.fromhex(h), np.uint8)
    return tuple(HighDegree(c['order'], arr(c['packet']), arr(c['sent']), c['ret'], arr(c['message'])) for c in G['cases'])


def check_independent(status, corrected, rs_err):
    """what follows from the code alone, for a decoder's outcomes over patterns(): status [n], corrected [n, 204] (or [n, 188]: the message
    alone, for a decoder that hands out no parity bytes), rs_err [n] (looked at only where the decoder has to succeed)"""
    pats = patterns()
    corrected = np.asarray(corrected)
    width = corrected.shape[1]
    assert len(status) == len(pats) == len(corrected) == len(rs_err) and width in (188, 204)
    for n, q in enumerate(pats):
        if q.expect is None:
            assert family(q.name) == 'beyond', q.name
            continue
        assert int(status[n]) == q.expect.status, (q.name, int(status[n]))
        wrong = np.flatnonzero(corrected[n] != q.expect.corrected[:width])
        assert wrong.size == 0, (q.name, 'bytes', wrong.tolist())
        assert int(rs_err[n]) == q.expect.rs_err, (q.name, int(rs_err[n]), q.expect.rs_err)
