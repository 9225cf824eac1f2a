"""The constructed edges of the T2-MI bank's tests, shared by the CPU and the GPU tests: every case is a run of TS packets on PID
0x1000 (slot 0 of the tests' banks, every PLP) whose continuity counter and packet_count go on from the case before it, so the cases
can be fed one by one, cut anywhere, or back to back as one stream.  ROWS holds what each case must give when it is fed alone, in that
order, to a slot that has seen the cases before it: (packet_type, packet_count, flags, plp_id, payload_bits, length, offset,
bbframe_bytes, first_packet, last_packet) per row, written out."""
import numpy as np

import psi_ref as S
import t2mi_ref as T

PID = 0x1000
ROW_FIELDS = ('packet_type', 'packet_count', 'flags', 'plp_id', 'payload_bits', 'length', 'offset', 'bbframe_bytes', 'first_packet', 'last_packet')
# flags in ROWS: 1 CRC_ERROR, 2 COUNT_ERROR, 4 BBFRAME, 8 INTL_FRAME_START, 16 BAD_PAYLOAD


def _bytes(n, seed):
    return bytes(np.random.default_rng(seed).integers(0, 256, n, dtype=np.uint8))


def edge_cases():
    """-> [(name, packets [k, 188])]"""
    z, out, cnt = T.Packetiser(PID, cc=9), [], [250]

    def c():
        cnt[0] = (cnt[0] + 1) & 255
        return cnt[0]

    def add(name, *parts):
        out.append((name, np.concatenate([np.asarray(p, np.uint8).reshape(-1, S.TS) for p in parts])))

    def raw(payload, **kw):
        return S.packet(PID, z._next(), payload, **kw)

    def sized(n, ptype=0x20):
        """a T2-MI packet of n bytes"""
        return T.t2mi_packet(ptype, c(), _bytes(n - 10, n))

    add('eighteen packets of 10 bytes in one TS packet', z.lay([T.t2mi_packet(0x20, c(), b'') for _ in range(18)]))
    add('payload_bits 13: pad bits', z.lay([T.t2mi_packet(0x10, c(), b'\xab\xc8', payload_bits=13)]))
    add('payload_bits 65535: 8202 bytes over 45 TS packets', z.lay([T.t2mi_packet(0x21, c(), _bytes(8192, 1), payload_bits=65535, superframe=9, stream_id=5)]))
    add('BBFRAME of 7274 bytes', z.lay([T.bb_packet(c(), 3, _bytes(7274, 2), frame_idx=200, start=1)]))
    add('BBFRAME of 7275 bytes', z.lay([T.bb_packet(c(), 3, _bytes(7275, 3))]))
    add('payload_bits 96 and 104', z.lay([T.bb_packet(c(), 4, _bytes(9, 4)), T.bb_packet(c(), 4, _bytes(10, 5), frame_idx=7)]))
    add('type 0 with payload_bits 16 and 107', z.lay([T.t2mi_packet(0, c(), b'\x01\x02'), T.t2mi_packet(0, c(), bytes([1, 2, 0]) + _bytes(11, 6), payload_bits=107)]))
    for h in (1, 2, 3, 4, 5):
        add('header split after %d bytes' % h, z.lay([sized(183 - h), T.bb_packet(c(), h, _bytes(40 + h, 10 + h))]))
    add('ends exactly at the TS packet end', z.lay([sized(183)]), z.lay([sized(30)]))
    add('ends exactly at the end of a continuation packet', z.lay([sized(183 + 184)]), z.lay([sized(12)]))
    x = sized(366)
    add('pointer = the whole rest', raw(b'\x00' + x[:183], pusi=1), raw(bytes([183]) + x[183:], pusi=1), z.lay([sized(20)]))
    add('pointer one beyond', raw(bytes([184]) + bytes(183), pusi=1))
    add('a payload of the pointer byte alone', raw(b'\x00', pusi=1, af_len=182), z.lay([sized(15)]))
    add('no payload left by the adaptation field', raw(b'', pusi=1, af_len=183), z.lay([sized(16)]))
    x = sized(400)
    add('pointer bytes leave the open packet incomplete', raw(b'\x00' + x[:183], pusi=1), raw(bytes([50]) + x[183:233] + sized(133), pusi=1))
    x = sized(200)
    add('pointer bytes overshoot the open packet', raw(b'\x00' + x[:183], pusi=1), raw(bytes([60]) + x[183:] + bytes(43) + sized(123), pusi=1))
    add('continuation with nothing open', raw(bytes(184)), raw(bytes(184)))
    x = sized(300)
    add('adaptation only in the middle', raw(b'\x00' + x[:183], pusi=1), S.packet(PID, z.cc, None, af_len=183), raw(x[183:], af_len=184 - 117 - 1))
    for k, inject in enumerate(S.INJECTORS):
        clean = np.concatenate([z.lay([T.bb_packet(c(), 1, _bytes(5 * 184 - 40, 30 + k))]), z.lay([sized(33)])])
        add(inject.__name__, inject(clean, 2)[0])
    one = lambda: z.lay([T.bb_packet(c(), 2, _bytes(60, cnt[0]))])
    hit = lambda ts, at: (ts.__setitem__((0, 188 - 73 + at), ts[0, 188 - 73 + at] ^ 0x10), ts)[1]    # byte `at` of the 73-byte T2-MI packet
    add('a flipped bit in the header, the payload and the CRC field', hit(one(), 0), one(), hit(one(), 30), one(), hit(one(), 71), one())
    a = one()
    c()
    add('a skipped packet_count', a, one())
    a = one()
    cnt[0] -= 1
    add('a repeated packet_count', a, one())
    a, b = one(), hit(one(), 20)
    cnt[0] -= 1
    add('a repeated packet_count behind a CRC error', a, b, one(), one())
    return out


# the cases of edge_cases() that the shared reassembly walk (csrc/ts_reasm.h) takes down a branch of its own
WALK_EDGES = tuple('header split after %d bytes' % h for h in (1, 2, 3, 4, 5)) + (
    'pointer = the whole rest', 'pointer bytes leave the open packet incomplete', 'pointer bytes overshoot the open packet')


def walk_cases():
    """further branches of the walk, each for a slot that has seen nothing -> [(name, packets [k, 188], rows as in ROWS for the packets in
    one call, dropped_packets)]"""
    x, y = T.t2mi_packet(0x20, 1, _bytes(390, 70)), T.t2mi_packet(0x20, 2, _bytes(50, 71))
    lost = np.concatenate([S.packet(PID, 1, b'\x00' + x[:183], pusi=1), S.packet(PID, 2, x[183:367]),                   # (continuity counter 3 is lost)
                           S.packet(PID, 4, bytes([33]) + x[367:] + y, pusi=1, af_len=184 - 94 - 1)]).reshape(-1, S.TS)
    three = T.Packetiser(PID).lay([T.t2mi_packet(0x20, 1, _bytes(40, 72)), T.t2mi_packet(0x10, 2, _bytes(50, 73)), T.t2mi_packet(0x20, 3, _bytes(140, 74))])
    return [('PUSI packet behind a lost TS packet with a packet open', lost, [(32, 2, 0, 0, 400, 60, -1, 0, 2, 2)], 1),
            ('two whole packets and a third cut by the TS packet end', three,
             [(32, 1, 0, 0, 320, 50, -1, 0, 0, 0), (16, 2, 0, 0, 400, 60, -1, 0, 0, 0), (32, 3, 0, 0, 1120, 150, -1, 0, 0, 1)], 0)]


def whole_stream(rng=None, cases=None):
    """the edge cases back to back with packets of another PID, a TEI packet and a null packet between them"""
    rng = rng or np.random.default_rng(1)
    parts, cc = [], 0
    for _, ts in cases or edge_cases():
        n = int(rng.integers(0, 3))
        parts += [ts, S.filler(0x99, n, rng, cc)]
        cc += n
    tei = S.packet(PID, 0, b'\x00' * 10, pusi=1).copy()
    tei[1] |= 0x80
    parts += [tei.reshape(1, -1), S.packet(0x1FFF, 0).reshape(1, -1)]
    return np.concatenate(parts)


ROWS = {
    'eighteen packets of 10 bytes in one TS packet': [(32, (251 + i) & 255, 0, 0, 0, 10, -1, 0, 0, 0) for i in range(18)],
    'payload_bits 13: pad bits': [(16, 13, 0, 0, 13, 12, -1, 0, 0, 0)],
    'payload_bits 65535: 8202 bytes over 45 TS packets': [(33, 14, 0, 0, 65535, 8202, -1, 0, 0, 44)],
    'BBFRAME of 7274 bytes': [(0, 15, 12, 3, 58216, 7287, 0, 7274, 0, 39)],
    'BBFRAME of 7275 bytes': [(0, 16, 16, 3, 58224, 7288, -1, 0, 0, 39)],
    'payload_bits 96 and 104': [(0, 17, 16, 4, 96, 22, -1, 0, 0, 0), (0, 18, 4, 4, 104, 23, 0, 10, 0, 0)],
    'type 0 with payload_bits 16 and 107': [(0, 19, 16, 0, 16, 12, -1, 0, 0, 0), (0, 20, 16, 2, 107, 24, -1, 0, 0, 0)],
    'header split after 1 bytes': [(32, 21, 0, 0, 1376, 182, -1, 0, 0, 0), (0, 22, 4, 1, 352, 54, 0, 41, 0, 1)],
    'header split after 2 bytes': [(32, 23, 0, 0, 1368, 181, -1, 0, 0, 0), (0, 24, 4, 2, 360, 55, 0, 42, 0, 1)],
    'header split after 3 bytes': [(32, 25, 0, 0, 1360, 180, -1, 0, 0, 0), (0, 26, 4, 3, 368, 56, 0, 43, 0, 1)],
    'header split after 4 bytes': [(32, 27, 0, 0, 1352, 179, -1, 0, 0, 0), (0, 28, 4, 4, 376, 57, 0, 44, 0, 1)],
    'header split after 5 bytes': [(32, 29, 0, 0, 1344, 178, -1, 0, 0, 0), (0, 30, 4, 5, 384, 58, 0, 45, 0, 1)],
    'ends exactly at the TS packet end': [(32, 31, 0, 0, 1384, 183, -1, 0, 0, 0), (32, 32, 0, 0, 160, 30, -1, 0, 1, 1)],
    'ends exactly at the end of a continuation packet': [(32, 33, 0, 0, 2856, 367, -1, 0, 0, 1), (32, 34, 0, 0, 16, 12, -1, 0, 2, 2)],
    'pointer = the whole rest': [(32, 35, 0, 0, 2848, 366, -1, 0, 0, 1), (32, 36, 0, 0, 80, 20, -1, 0, 2, 2)],
    'pointer one beyond': [],
    'a payload of the pointer byte alone': [(32, 37, 0, 0, 40, 15, -1, 0, 1, 1)],
    'no payload left by the adaptation field': [(32, 38, 0, 0, 48, 16, -1, 0, 1, 1)],
    'pointer bytes leave the open packet incomplete': [(32, 40, 2, 0, 984, 133, -1, 0, 1, 1)],
    'pointer bytes overshoot the open packet': [(32, 41, 0, 0, 1520, 200, -1, 0, 0, 1), (32, 42, 0, 0, 904, 123, -1, 0, 1, 1)],
    'continuation with nothing open': [],
    'adaptation only in the middle': [(32, 43, 0, 0, 2320, 300, -1, 0, 0, 2)],
    'drop_middle': [(32, 45, 2, 0, 184, 33, -1, 0, 4, 4)],
    'announce_discontinuity': [(32, 47, 2, 0, 184, 33, -1, 0, 5, 5)],
    'scramble': [(32, 49, 2, 0, 184, 33, -1, 0, 5, 5)],
    'flip_bit': [(0, 50, 1, 0, 7064, 893, -1, 0, 0, 4), (32, 51, 2, 0, 184, 33, -1, 0, 5, 5)],
    'duplicate': [(0, 52, 4, 1, 7064, 893, 0, 880, 0, 5), (32, 53, 0, 0, 184, 33, -1, 0, 6, 6)],
    'a flipped bit in the header, the payload and the CRC field': [(16, 54, 1, 0, 504, 73, -1, 0, 0, 0), (0, 55, 6, 2, 504, 73, 0, 60, 1, 1), (0, 56, 1, 0, 504, 73, -1, 0, 2, 2), (0, 57, 6, 2, 504, 73, 60, 60, 3, 3), (0, 58, 1, 0, 504, 73, -1, 0, 4, 4), (0, 59, 6, 2, 504, 73, 120, 60, 5, 5)],
    'a skipped packet_count': [(0, 60, 4, 2, 504, 73, 0, 60, 0, 0), (0, 62, 6, 2, 504, 73, 60, 60, 1, 1)],
    'a repeated packet_count': [(0, 63, 4, 2, 504, 73, 0, 60, 0, 0), (0, 63, 6, 2, 504, 73, 60, 60, 1, 1)],
    'a repeated packet_count behind a CRC error': [(0, 64, 4, 2, 504, 73, 0, 60, 0, 0), (0, 65, 1, 0, 504, 73, -1, 0, 1, 1), (0, 65, 4, 2, 504, 73, 60, 60, 2, 2), (0, 66, 4, 2, 504, 73, 120, 60, 3, 3)],
}
