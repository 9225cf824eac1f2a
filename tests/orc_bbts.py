"""Helpers for the BBFRAME -> TS / GSE parser: ctypes access to oracle/bbframe_ts.cpp and a small transmitter side in numpy
(TS packets -> user packets with CRC-8 -> BBFRAMEs with BBHEADER, EN 302 307-1 5.1.4-5.1.6; GSE packets / fragments with CRC-32,
TS 102 606), the reference's own parser from oracle/_ref where that is built, and the parser test cases that the CPU pins, the
golden generator and the GPU tests share.  Test infrastructure only."""
import ctypes as C
import numpy as np
from orc import lib, ref

VP = C.c_void_p
_b = False
UB_INPUT, UB_OUTPUT, UB_LENGTH, UB_SLOT = 1, 2, 4, 8
STAT_KEYS = ('ts_gs', 'sis_mis', 'ccm_acm', 'issyi', 'npd', 'ro', 'isi', 'upl', 'dfl', 'sync', 'syncd',
             'last_gse_crc_err', 'last_bb_cnt', 'last_bb_proc', 'last_ts_errs', 'synched', 'count')


def L():
    global _b
    l = lib()
    if not _b:
        l.orc_bbts_create.restype = VP
        l.orc_bbts_create.argtypes = [C.c_int]
        l.orc_bbts_destroy.restype = None
        l.orc_bbts_destroy.argtypes = [VP]
        l.orc_bbts_set_frame_size.restype = None
        l.orc_bbts_set_frame_size.argtypes = [VP, C.c_int]
        l.orc_bbts_work.argtypes = [VP, VP, C.c_int, VP, C.c_int]
        l.orc_bbts_get_stats.restype = None
        l.orc_bbts_get_stats.argtypes = [VP, VP]
        l.orc_bbts_last_undefined.argtypes = [VP]
        l.orc_bbts_crc8_bits.restype = C.c_uint
        l.orc_bbts_crc8_bits.argtypes = [VP, C.c_int]
        _b = True
    return l


class OracleBbTs:
    def __init__(self, kbch_bits):
        self.kbch = kbch_bits
        self.h = L().orc_bbts_create(kbch_bits)

    def __del__(self):
        if getattr(self, 'h', None):
            L().orc_bbts_destroy(self.h)
            self.h = None

    def set_frame_size(self, kbch_bits):
        L().orc_bbts_set_frame_size(self.h, kbch_bits)
        self.kbch = kbch_bits

    def work(self, bbframes, cap=None):
        bb = np.ascontiguousarray(bbframes, np.uint8).reshape(-1)
        cnt = bb.size // (self.kbch // 8)
        cap = cap if cap is not None else bb.size + 376
        out = np.zeros(max(cap, 1), np.uint8)
        n = L().orc_bbts_work(self.h, bb.ctypes.data, cnt, out.ctypes.data, cap)
        if n < 0:
            return None
        return out[:n].copy()

    def work_raw(self, bbframes, cap, fill=0):
        """-> (return value, the whole `cap`-byte output buffer, pre-filled with `fill`)"""
        bb = np.ascontiguousarray(bbframes, np.uint8).reshape(-1)
        out = np.full(max(cap, 1), fill, np.uint8)
        n = L().orc_bbts_work(self.h, bb.ctypes.data, bb.size // (self.kbch // 8), out.ctypes.data, cap)
        return n, out[:cap]

    def undefined(self):
        """UB_* bits: where the last call left what the reference defines (oracle/bbframe_ts.h)"""
        return L().orc_bbts_last_undefined(self.h)

    def stats(self):
        a = np.zeros(17, np.int32)
        L().orc_bbts_get_stats(self.h, a.ctypes.data)
        return dict(zip(STAT_KEYS, [int(x) for x in a]))


def crc8(data):
    """CRC-8 x^8+x^7+x^6+x^4+x^2+1, MSB first, zero initial state (EN 302 307-1 5.1.4 / 5.1.6)"""
    crc = 0
    for byte in bytes(data):
        for k in range(7, -1, -1):
            fb = ((byte >> k) & 1) ^ (crc >> 7)
            crc = (crc << 1) & 0xff
            if fb:
                crc ^= 0xD5
    return crc


def bbheader(ts_gs, dfl_bits, syncd_bits=0, upl_bits=0, sync=0, sis=1, ccm=1, issyi=0, npd=0, ro=0, isi=0, good_crc=True):
    h = np.zeros(10, np.uint8)
    h[0] = (ts_gs << 6) | (sis << 5) | (ccm << 4) | (issyi << 3) | (npd << 2) | ro
    h[1] = isi
    h[2], h[3] = upl_bits >> 8, upl_bits & 0xff
    h[4], h[5] = dfl_bits >> 8, dfl_bits & 0xff
    h[6] = sync
    h[7], h[8] = syncd_bits >> 8, syncd_bits & 0xff
    h[9] = crc8(h[:9]) ^ (0 if good_crc else 0x5a)
    return h


def ts_packets(n, rng):
    p = rng.integers(0, 256, (n, 188), dtype=np.uint8)
    p[:, 0] = 0x47
    return p


def bbframes_from_ts(packets, kbch_bits, nframes, dfl_bytes=None):
    """Slice the user-packet stream (sync byte of packet k replaced by the CRC-8 of packet k-1's 187 bytes) into data fields."""
    fb = kbch_bits // 8
    D = dfl_bytes if dfl_bytes is not None else fb - 10
    ups = packets.copy()
    for k in range(len(ups)):
        ups[k, 0] = crc8(packets[k - 1, 1:]) if k else 0
    stream = ups.reshape(-1)
    assert stream.size >= nframes * D
    frames = np.zeros((nframes, fb), np.uint8)
    for f in range(nframes):
        off = f * D
        syncd = (-off) % 188
        frames[f, :10] = bbheader(3, D * 8, syncd * 8, upl_bits=1504, sync=0x47)
        frames[f, 10:10 + D] = stream[off:off + D]
    return frames


def crc32_mpeg(data, crc=0xffffffff):
    for byte in bytes(data):
        crc ^= byte << 24
        for _ in range(8):
            crc = ((crc << 1) ^ 0x04c11db7) & 0xffffffff if crc & 0x80000000 else (crc << 1) & 0xffffffff
    return crc


def gse_complete(proto, pdu, label=None):
    """one unfragmented GSE packet; label: 6 bytes (label type 00) or None (label type 10, broadcast)"""
    lt = 0 if label is not None else 2
    body = bytes([proto >> 8, proto & 0xff]) + (bytes(label) if label is not None else b'') + bytes(pdu)
    n = len(body)
    return bytes([0xC0 | (lt << 4) | (n >> 8), n & 0xff]) + body


def gse_fragments(proto, pdu, cuts, frag_id, label=None, corrupt_crc=False):
    """PDU cut at the byte positions `cuts` into START / middle / END packets"""
    lt = 0 if label is not None else 2
    lab = bytes(label) if label is not None else b''
    total = 2 + len(lab) + len(pdu)
    tl = bytes([total >> 8, total & 0xff])
    pr = bytes([proto >> 8, proto & 0xff])
    crc = crc32_mpeg(tl + pr + lab + bytes(pdu))
    if corrupt_crc:
        crc ^= 0x1000
    tail = bytes(pdu) + bytes([(crc >> 24) & 0xff, (crc >> 16) & 0xff, (crc >> 8) & 0xff, crc & 0xff])
    pieces = [tail[a:b] for a, b in zip([0] + list(cuts), list(cuts) + [len(tail)])]
    out = []
    for i, pc in enumerate(pieces):
        if i == 0:
            body = bytes([frag_id]) + tl + pr + lab + pc
            h = 0x80 | (lt << 4)
        elif i == len(pieces) - 1:
            body = bytes([frag_id]) + pc
            h = 0x40 | 0x30
        else:
            body = bytes([frag_id]) + pc
            h = 0x30
        n = len(body)
        out.append(bytes([h | (n >> 8), n & 0xff]) + body)
    return out


def gse_bbframe(gse_packets, kbch_bits):
    """GSE packets back to back in one data field, zero padding after them"""
    fb = kbch_bits // 8
    data = b''.join(gse_packets)
    dfl = fb - 10
    assert len(data) <= dfl
    fr = np.zeros(fb, np.uint8)
    fr[:10] = bbheader(1, dfl * 8, 0, upl_bits=0, sync=0)
    fr[10:10 + len(data)] = np.frombuffer(data, np.uint8)
    return fr


def fuzz_frames(rng, kbch_bits, nframes, ts_gs_choices=(3,), p_bad=0.15):
    """random data fields behind mostly-valid random BBHEADERs (some with bad CRC / DFL / SYNCD)"""
    fb = kbch_bits // 8
    fr = rng.integers(0, 256, (nframes, fb), dtype=np.uint8)
    for f in range(nframes):
        r = rng.random()
        dfl = int(rng.integers(0, (fb - 10) + 1)) * 8
        if rng.random() < 0.5:
            dfl = (fb - 10) * 8
        if rng.random() < 0.1:
            dfl = int(rng.integers(0, 400)) * 8
        syncd = int(rng.integers(0, 188)) * 8
        good = True
        if r < p_bad / 3:
            good = False
        elif r < 2 * p_bad / 3:
            dfl += int(rng.integers(1, 8))
        elif r < p_bad:
            syncd = dfl + int(rng.integers(0, 100))
        tg = int(rng.choice(ts_gs_choices))
        fr[f, :10] = bbheader(tg, dfl & 0xffff, syncd & 0xffff, upl_bits=0 if tg == 1 else 1504, sync=0x47, good_crc=good,
                              issyi=int(rng.random() < 0.03), npd=int(rng.random() < 0.03), sis=int(rng.random() < 0.8), isi=int(rng.integers(0, 256)))
    return fr


def gse_fuzz_frames(rng, kbch_bits, nframes, p_bad=0.1):
    """fuzz_frames that mostly announce GSE, with short plausible packets (complete PDUs, START / END fragments over five fragment
    IDs, some with a bad CRC-32) at the start of most data fields so that GSE-looking content is frequent"""
    fr = fuzz_frames(rng, kbch_bits, nframes, ts_gs_choices=(1, 1, 1, 3, 0), p_bad=p_bad)
    for f in range(len(fr)):
        if rng.random() < 0.7:
            pk = []
            for _k in range(int(rng.integers(1, 6))):
                pdu = rng.integers(0, 256, int(rng.integers(4, 120)), dtype=np.uint8)
                if rng.random() < 0.5:
                    pk.append(gse_complete(int(rng.choice([0x0800, 0x86DD, 0x1234])), pdu, label=bytes(6) if rng.random() < 0.5 else None))
                else:
                    pk += gse_fragments(0x0800, pdu, [int(rng.integers(1, len(pdu)))], frag_id=int(rng.integers(0, 5)),
                                        corrupt_crc=bool(rng.random() < 0.2))[int(rng.integers(0, 2)):]
            data = np.frombuffer(b''.join(pk), np.uint8)[:kbch_bits // 8 - 11]
            fr[f, 10:10 + data.size] = data
    return fr


# ------------------------------------------------------------------ the reference's parser (oracle/_ref)
FIELD_KEYS = STAT_KEYS[:15]          # BBFrameTSParser's public fields; synched and count are private


def R():
    r = ref()
    if r is None or not hasattr(r, 'ref_bbts_create'):
        return None
    if not getattr(r, '_bbts_bound', False):
        r.ref_bbts_create.restype = VP
        r.ref_bbts_create.argtypes = [C.c_int, C.c_int]
        r.ref_bbts_destroy.restype = None
        r.ref_bbts_destroy.argtypes = [VP]
        r.ref_bbts_set_frame_size.restype = None
        r.ref_bbts_set_frame_size.argtypes = [VP, C.c_int]
        r.ref_bbts_work.argtypes = [VP, VP, C.c_int, VP, C.c_int]
        r.ref_bbts_left_output.argtypes = [VP]
        r.ref_bbts_get_fields.restype = None
        r.ref_bbts_get_fields.argtypes = [VP, VP]
        r._bbts_bound = True
    return r


class RefBbTs:
    """dsp::dvbs2::BBFrameTSParser.  It runs on copies of the buffers with guard zones behind them (oracle/ref_shim.cpp): `guard_fill`
    is what reads beyond the last frame of a call see, left_output() tells whether the last call wrote beyond `cap`."""

    def __init__(self, kbch_bits, guard_fill=0):
        self.kbch = kbch_bits
        self.h = R().ref_bbts_create(kbch_bits, guard_fill)

    def __del__(self):
        if getattr(self, 'h', None):
            R().ref_bbts_destroy(self.h)
            self.h = None

    def set_frame_size(self, kbch_bits):
        R().ref_bbts_set_frame_size(self.h, kbch_bits)
        self.kbch = kbch_bits

    def work_raw(self, bbframes, cap, fill=0):
        """-> (return value, the whole `cap`-byte output buffer, pre-filled with `fill`)"""
        bb = np.ascontiguousarray(bbframes, np.uint8).reshape(-1)
        out = np.full(max(cap, 1), fill, np.uint8)
        n = R().ref_bbts_work(self.h, bb.ctypes.data, bb.size // (self.kbch // 8), out.ctypes.data, cap)
        return n, out[:cap]

    def left_output(self):
        return bool(R().ref_bbts_left_output(self.h))

    def fields(self):
        a = np.zeros(15, np.int32)
        R().ref_bbts_get_fields(self.h, a.ctypes.data)
        return dict(zip(FIELD_KEYS, [int(x) for x in a]))


# ------------------------------------------------------------------ shared parser cases: (name, kbch, [frames of call 0, frames of call 1, ...])
def ragged(rng, frames):
    """cut [n, fb] frames into calls of 0 to 5 frames"""
    calls, pos = [], 0
    while pos < len(frames):
        k = int(rng.integers(0, 6))
        calls.append(frames[pos:pos + k])
        pos += k
    return calls


def call_cap(frames):
    return int(frames.size) + 376


TS_ROUND_TRIPS = ((14232, None), (48408, None), (3072, None), (14232, 1000))
TS_FUZZ = ((1, 3072, (3, 3, 0, 2)), (2, 14232, (3, 1, 1, 0)), (3, 3072, (1, 1, 3)))
GSE_FUZZ_KBCH = (3072, 14232)
FUZZ_SEEDS = 8


def ts_round_trip_frames(kbch, dfl, nfr=9):
    """-> (frames, the packets that must come out)"""
    rng = np.random.default_rng(kbch + (dfl or 0))
    D = dfl if dfl is not None else kbch // 8 - 10
    pk = ts_packets(nfr * D // 188 + 2, rng)
    return bbframes_from_ts(pk, kbch, nfr, dfl), pk[:(nfr * D - 1) // 188]


def _padding_frame(kbch):
    fr = np.zeros(kbch // 8, np.uint8)
    fr[:10] = bbheader(1, (kbch // 8 - 10) * 8, 0)
    return fr


def gse_structured_cases():
    """GSE cases built packet by packet; every one starts with an all-padding frame that absorbs the SYNCD/8 + 1 bytes the parser
    skips when it synchronises (bbframe_ts_parser.cpp:158-169)"""
    cases = []
    for kbch in (3072, 14232):
        rng = np.random.default_rng(1000 + kbch)
        small = kbch == 3072
        pre = _padding_frame(kbch)
        lab = bytes(range(1, 7))
        pdu = lambda n: rng.integers(0, 256, n, dtype=np.uint8)
        B = lambda *pk: gse_bbframe(list(pk), kbch)
        p1, p2, p3 = pdu(90 if small else 300), pdu(400 if small else 1200), pdu(77)
        # complete PDUs: 6-byte label / broadcast, IPv4 / IPv6 / another protocol (no protocol bytes in the GRE header), padding after them
        cases.append((f'complete_{kbch}', kbch, ragged(rng, np.stack([pre, B(gse_complete(0x0800, p1, label=lab), gse_complete(0x86DD, p3)),
                                                                       B(gse_complete(0x1234, p3, label=lab)), B(), B(gse_complete(0x0800, p1))]))))
        # START / middle / END over three fragment IDs at once, interleaved with complete PDUs, ENDs in another order than the STARTs
        fa = gse_fragments(0x86DD, p2, [130, 300] if small else [400, 900], frag_id=9, label=lab)
        fb_ = gse_fragments(0x0800, p1, [40] if small else [120], frag_id=3)
        fc = gse_fragments(0x1234, p3, [10, 30, 50], frag_id=200)
        fr = [pre, B(fa[0], fb_[0]), B(fc[0], fa[1], fc[1]), B(gse_complete(0x0800, p3), fc[2], fb_[1]), B(fa[2], fc[3])]
        cases.append((f'three_ids_{kbch}', kbch, ragged(rng, np.stack(fr))))
        # a fourth open ID finds no slot: its fragments are dropped, the other three complete; then the freed slots serve it
        fd = gse_fragments(0x0800, p3, [20, 40], frag_id=77)
        fr = [pre, B(fa[0], fb_[0], fc[0]), B(fd[0], fd[1], fc[1], fc[2]), B(fd[2], fa[1], fb_[1], fc[3]), B(fa[2], *fd)]
        cases.append((f'fourth_id_{kbch}', kbch, ragged(rng, np.stack(fr))))
        # a START that re-opens an ID in flight restarts its slot; an END and a middle fragment for an ID that is not open are ignored
        fe = gse_fragments(0x0800, p3, [33], frag_id=9)
        cases.append((f'restart_{kbch}', kbch, ragged(rng, np.stack([pre, B(fa[0], fb_[1], fc[1]), B(fa[1], fe[0]), B(fe[1])]))))
        # a bad CRC-32 raises last_gse_crc_err and emits nothing; the next good PDU of the same ID clears it
        bad = gse_fragments(0x0800, p1, [35] if small else [100], frag_id=5, corrupt_crc=True)
        good = gse_fragments(0x0800, p3, [35], frag_id=5)
        cases.append((f'bad_crc_{kbch}', kbch, [np.stack([pre, B(*bad)]), np.stack([B(gse_complete(0x86DD, p3))]), np.stack([B(*good)])]))
        # malformed lengths that stay in defined memory: an END too short to hold a CRC-32, and a complete PDU whose length runs over
        # the data field into the next BBFRAME of the same call (read as is)
        short_end = bytes([0x40 | 0x30, 3, 5, 1, 2])
        over = bytearray(gse_complete(0x0800, pdu(kbch // 8 - 120)))
        n_over = (kbch // 8 - 120 + 2) + 150
        over[0], over[1] = 0xC0 | 0x20 | (n_over >> 8), n_over & 0xff
        cases.append((f'bad_length_{kbch}', kbch, [np.stack([pre, B(good[0], short_end)]), np.stack([B(gse_complete(0x0800, p3), bytes(over)), B(*good), pre])]))
        # ts_gs changes between frames: TS, GSE, generic continuous (ignored), TS again (the carried partial survives the GSE frames)
        ts, _ = ts_round_trip_frames(kbch, None, 4)
        g0 = pre.copy()
        g0[:10] = bbheader(0, (kbch // 8 - 10) * 8, 0)
        fr = [ts[0], B(gse_complete(0x0800, p3)), ts[1], g0, B(fb_[0]), ts[2], B(fb_[1]), ts[3]]
        cases.append((f'ts_gs_changes_{kbch}', kbch, ragged(rng, np.stack(fr))))
    # fragments that carry a slot past 64 KiB (bbframe_ts_parser.cpp:371 writes on, into the next slot's buffer; the oracle and the engine
    # free the slot instead): nothing else is disturbed, and a new START of that ID then reassembles as usual
    kbch = 58192
    rng = np.random.default_rng(1000 + kbch)
    pre = _padding_frame(kbch)
    big = gse_fragments(0x0800, rng.integers(0, 256, 4000, dtype=np.uint8), [3500], frag_id=7)
    mid = lambda: bytes([0x30 | (3601 >> 8), 3601 & 0xff, 7]) + bytes(rng.integers(0, 256, 3600, dtype=np.uint8))
    p3 = rng.integers(0, 256, 77, dtype=np.uint8)
    again = gse_fragments(0x86DD, p3, [30], frag_id=7)
    fr = [pre, gse_bbframe([big[0], mid()], kbch)] + [gse_bbframe([mid(), mid()], kbch) for _ in range(9)] + [gse_bbframe([gse_complete(0x0800, p3), again[0]], kbch), gse_bbframe([again[1]], kbch)]
    cases.append((f'past_64k_{kbch}', kbch, ragged(rng, np.stack(fr))))
    return cases


def gse_fuzz_cases():
    return [(f'gse_fuzz_{kbch}_{seed}', kbch, [gse_fuzz_frames(rng, kbch, int(rng.integers(0, 6))) for _ in range(6)])
            for kbch in GSE_FUZZ_KBCH for seed in range(FUZZ_SEEDS) for rng in [np.random.default_rng(7000 + kbch + seed)]]


def ts_fuzz_cases():
    """the three fuzz configurations of the golden file, FUZZ_SEEDS seeds each (the first is the configuration's historical seed)"""
    return [(f'ts_fuzz_{cfg}_{k}', kbch, [fuzz_frames(rng, kbch, int(rng.integers(0, 6)), ts_gs_choices=choices, p_bad=0.2) for _ in range(6)])
            for cfg, kbch, choices in TS_FUZZ for k in range(FUZZ_SEEDS) for rng in [np.random.default_rng(cfg + 100 * k)]]


def ts_round_trip_cases():
    out = []
    for kbch, dfl in TS_ROUND_TRIPS:
        fr, _ = ts_round_trip_frames(kbch, dfl)
        out.append((f'ts_{kbch}_{dfl}', kbch, ragged(np.random.default_rng(kbch), fr)))
    return out


def all_parser_cases():
    return ts_round_trip_cases() + ts_fuzz_cases() + gse_structured_cases() + gse_fuzz_cases()


def walk_case(name, kbch, calls, fill=0xA5):
    """One case through the oracle and the reference side by side, call by call with `cap` as in the golden generator.  Per call:
    dict(ub=the oracle's UB_* bits, orc=(n, out, fields), ref=(n, out, fields), left_output=the reference wrote beyond cap).
    A call with UB bits set is one where the reference's behaviour is undefined (it reads beyond the frames it was given, or writes
    beyond `cap`: bbframe_ts_parser.cpp:217-218,233-269,275-321,328-357,366-373 bound none of it), so the two need not agree from
    there on: both parsers are replaced by fresh ones after such a call.  The one exception is UB_SLOT alone in the past_64k case,
    which is built so that the reference's overflow lands in an idle neighbour slot and the agreement must hold on."""
    o, r = OracleBbTs(kbch), RefBbTs(kbch)
    recs = []
    for fr in calls:
        cap = call_cap(fr)
        n, out = o.work_raw(fr, cap, fill)
        st = o.stats()
        rn, rout = r.work_raw(fr, cap, fill)
        ub = o.undefined()
        if ub == UB_SLOT and name.startswith('past_64k'):
            ub = 0
        recs.append(dict(ub=ub, orc=(n, out, {k: st[k] for k in FIELD_KEYS}), ref=(rn, rout, r.fields()), left_output=r.left_output()))
        if ub:
            o, r = OracleBbTs(kbch), RefBbTs(kbch)
    return recs
