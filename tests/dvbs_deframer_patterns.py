"""Constructed bit streams for the DVB-S TS deframer (DVBS_TS_Deframer::work, dvbs_ts_deframer.cpp:37-92), numpy only, shared by
tests/test_oracle_dvbs_deframer_patterns.py (CPU) and tests/test_gpu_dvbs_deframer_patterns.py (GPU).  Test infrastructure only.

The deframer tests a 13 056-bit window at every bit: the eight bytes at 1632-bit spacing against B8 47 47 47 47 47 47 47 (t_nor) and
against the complement (t_inv = 64 - t_nor); at most 8 differing bits on either side is a hit, and a hit delivers the window (complemented for
an inverted hit) and sets (errors_nor, errors_inv) to (t_nor, 0) or (0, t_inv).  A natural stream has one hit per 13 056 bits.  Every
Pattern here states, next to its bits, what the deframer must make of it: the frames in order, the number of bits after which each
hit fires (the stream length that contains the window's last bit) and the error pair each hit leaves."""
from dataclasses import dataclass
import numpy as np
from orc_dvbs_tail import dvbs_outer_tx

FRAME_BITS = 13056
FRAME_BYTES = 1632
THRESHOLD_KS = (0, 8, 9, 55, 56, 64)


@dataclass
class Pattern:
    name: str
    what: str                # what the pattern exercises
    bits: np.ndarray         # uint8, one bit per byte
    frames: list             # expected frames in order, uint8 [1632] each
    ends: list               # per hit: it fires when this many bits of the stream have been pushed
    errs: list               # per hit: (errors_nor, errors_inv) after it


def _flip_sync_bits(data, col, nflip, rng):
    """flip nflip of the 64 sync bits of the group whose sync bytes are data[204 * i + col], i = 0 .. 7"""
    for q in rng.choice(64, nflip, replace=False):
        data[204 * (q // 8) + col] ^= 0x80 >> (q % 8)


def dense(J, lead, alternate, errors=True, seed=1):
    """J byte-aligned hits 8 bits apart: `lead` zero bits, then eight 204-byte rows of which row 0 has B8 and rows 1 .. 7 have 47 at
    byte j for every j < J (complemented for odd j when `alternate`), then J + 15 more bytes so that the last window is complete; every other
    byte random.  With `errors`, (j + j // 9) % 9 of the 64 sync bits of hit j are flipped (0 .. 8: still a hit), so that no two neighbouring
    hits leave the same error pair and the 'last hit' of a tile, a wave or a call is told apart from its neighbours.
    J <= 204: hit j's sync bytes are column j of the rows, and a row has 204 columns."""
    assert 1 <= J <= 204
    rng = np.random.default_rng(seed)
    data = rng.integers(0, 256, FRAME_BYTES + J + 15, dtype=np.uint8)
    frames, ends, errs = [], [], []
    for j in range(J):
        inv = 0xFF if (alternate and j % 2) else 0
        for i in range(8):
            data[204 * i + j] = (0xB8 if i == 0 else 0x47) ^ inv
    for j in range(J):
        e = (j + j // 9) % 9 if errors else 0
        _flip_sync_bits(data, j, e, rng)
        errs.append((0, e) if (alternate and j % 2) else (e, 0))
    for j in range(J):
        frames.append(data[j:j + FRAME_BYTES] ^ np.uint8(0xFF if (alternate and j % 2) else 0))
        ends.append(lead + 8 * j + FRAME_BITS)
    bits = np.concatenate([np.zeros(lead, np.uint8), np.unpackbits(data)])
    what = (f'{J} hits 8 bits apart from bit {lead} on' + (', normal and inverted in turn' if alternate else '') +
            ': several hits per wave and per 256-position tile, on both sides of the seams; first hit at tile position ' + str((ends[0] - 1) % 256))
    return Pattern(f'dense{J}_lead{lead}_{"alt" if alternate else "nor"}{"_err" if errors else ""}', what, bits, frames, ends, errs)


def _threshold_frames(ks, seed):
    bits, _ = dvbs_outer_tx(8 * len(ks), seed)
    data = np.packbits(bits)
    rng = np.random.default_rng(seed + 1000)
    frames, ends, errs = [], [], []
    for f, k in enumerate(ks):
        fr = data[FRAME_BYTES * f:FRAME_BYTES * (f + 1)]                   # (a view: the flips land in data)
        _flip_sync_bits(fr, 0, k, rng)
        if k <= 8 or k >= 56:
            frames.append(fr.copy() if k <= 8 else ~fr)
            ends.append(FRAME_BITS * (f + 1))
            errs.append((k, 0) if k <= 8 else (0, 64 - k))
    return np.unpackbits(data), frames, ends, errs


def threshold(k, lead=0, seed=40):
    """one clean frame of the outer transmitter with k of its 64 sync bits flipped, behind `lead` zero bits and in front of 100 more:
    k <= 8 is a normal hit with k errors, k >= 56 an inverted one with 64 - k, anything between is no hit"""
    bits, frames, ends, errs = _threshold_frames([k], seed + k)
    bits = np.concatenate([np.zeros(lead, np.uint8), bits, np.zeros(100, np.uint8)])
    return Pattern(f'threshold{k}', f'the <= 8 bound of the sync comparison: {k} of 64 sync bits differ', bits, frames, [e + lead for e in ends], errs)


def threshold_run(ks=THRESHOLD_KS, lead=3, seed=60):
    """consecutive frames of one stream with ks[f] sync bits flipped in frame f: the error pair of the last hit changes from frame to frame"""
    bits, frames, ends, errs = _threshold_frames(list(ks), seed)
    bits = np.concatenate([np.zeros(lead, np.uint8), bits, np.zeros(100, np.uint8)])
    return Pattern('threshold_run', f'frames with {list(ks)} flipped sync bits in a row: errors_nor / errors_inv follow the last hit', bits, frames,
                   [e + lead for e in ends], errs)


def empty():
    return Pattern('empty', 'a stream that brings 0 bits in every call', np.zeros(0, np.uint8), [], [], [])


def bank_patterns():
    """the streams that run side by side in one bank: dense runs of 40 hits behind eight consecutive leads (every residue mod 8, so the hits
    of some stream fall on lane 0, on lane 63 and on tile positions 255 and 0; 320 positions cross a tile seam and every wave seam), with
    and without inverted hits, the six threshold frames, their run, and a stream without bits"""
    pats = [dense(40, 250 + r, alternate=bool(a), errors=True, seed=10 + 2 * r + a) for r in range(8) for a in (0, 1)]
    pats.append(dense(40, 5, alternate=True, errors=False, seed=30))
    pats += [threshold(k, lead=17 * i) for i, k in enumerate(THRESHOLD_KS)]
    pats += [threshold_run(), empty()]
    return pats


def dense204(alternate=True):
    """the longest run that cannot collide with itself: all 204 columns of the eight rows are sync bytes"""
    return dense(204, 131, alternate, errors=True, seed=77)


CUTTINGS = ('whole', 'before1', 'before7', 'before8', 'before9', 'before13055', 'mid_run', 'tiny_calls')


def cut_bounds(p, rule):
    """call boundaries of stream p under a cutting rule: ascending stream positions, the last one the stream's length; call c brings
    bits [bounds[c - 1], bounds[c]) (a repeated boundary is a 0-bit call).
      whole          one call
      beforeD        a call boundary D bits before the first hit fires: D = 1 .. 9 leave all of the window but its last D bits in the history,
                     D = 13055 all but its first bit in the new call
      mid_run        a boundary between two hits in the middle of the stream's hits (for a dense run: 3 bits behind one of them)
      tiny_calls     everything up to the bit in front of the first hit, a 0-bit call, the 1-bit call that fires it, a 0-bit call, a 1-bit
                     call, the rest
    A stream without hits is cut at the same distances from its end."""
    n = int(p.bits.size)
    first = p.ends[0] if p.ends else n
    if rule == 'whole':
        b = [n]
    elif rule.startswith('before'):
        b = [max(first - int(rule[6:]), 0), n]
    elif rule == 'mid_run':
        b = [min(p.ends[len(p.ends) // 2] + 3, n) if p.ends else n // 2, n]
    elif rule == 'tiny_calls':
        b = [first - 1, first - 1, first, first, first + 1, n]
    else:
        raise ValueError(rule)
    b = [min(max(x, 0), n) for x in b]
    assert b == sorted(b) and b[-1] == n
    return b


def expected_calls(p, bounds):
    """what the pattern states for each call of a cutting: [(frames uint8 [k, 1632], (errors_nor, errors_inv) after the call)]"""
    out, a, last = [], 0, (0, 0)
    for b in bounds:
        idx = [i for i, e in enumerate(p.ends) if a < e <= b]
        if idx:
            last = p.errs[idx[-1]]
        out.append((np.stack([p.frames[i] for i in idx]) if idx else np.zeros((0, FRAME_BYTES), np.uint8), last))
        a = b
    return out
