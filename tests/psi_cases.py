"""The constructed edges of the PSI section bank's tests, shared by the CPU and the GPU tests: every case is a run of packets on PID
0x30 (slot 1 of the tests' banks) whose continuity counter goes on from the case before it, so the cases can be fed one by one, cut
anywhere, or back to back as one stream."""
import numpy as np

import psi_ref as P

PID = 0x30


def _sec(n, seed, table_id=0x42):
    """a long section of n bytes"""
    body = np.random.default_rng(seed).integers(0, 255, n - 12, dtype=np.uint8)      # (never 0xFF: a body byte may follow a section's end)
    return P.long_section(table_id, seed, bytes(body), version=seed & 31)


def edge_cases():
    """-> [(name, packets [k, 188], multi: the case holds a section that spans packets)]"""
    z, out = P.Packetiser(PID, cc=5), []

    def add(name, ts, multi=False):
        out.append((name, np.asarray(ts, np.uint8).reshape(-1, P.TS), multi))
    def first(sections, k=1):
        """the first k packets of the sections' run; the continuity counter goes on behind them"""
        ts = z.lay(sections)
        z.cc = (z.cc - (len(ts) - k)) & 15
        return ts[:k]
    add('pointer 0', z.lay([_sec(100, 1)]))
    add('pointer mid-packet, nothing open', z.lay([_sec(50, 2)], pointer=20, before=bytes(range(20))))
    add('largest pointer that leaves one byte', z.lay([_sec(60, 3)], pointer=182), True)
    add('pointer past the payload', [P.packet(PID, z._next(), bytes([184]) + bytes(183), pusi=1)])
    add('three sections in one packet', z.lay([_sec(20, 4), P.short_section(0x70, bytes(range(10))), _sec(30, 5)]))
    add('section ends exactly at the packet end', z.lay([_sec(183, 6)], stuffing=False))
    add('ends exactly at the end of a continuation packet', z.lay([_sec(183 + 184, 7)], stuffing=False), True)
    add('header cut after 1 byte', z.lay([_sec(182, 8), _sec(40, 9)]), True)
    add('header cut after 2 bytes', z.lay([_sec(181, 10), _sec(40, 11)]), True)
    add('largest section', z.lay([_sec(4096, 12)]), True)
    add('section_length 4094', z.lay([bytes([0x42, 0x3F, 0xFE]) + bytes(100)]))
    add('section_length 4094 in a cut header', z.lay([_sec(182, 13), bytes([0x42, 0x3F, 0xFE]) + bytes(100)]), True)
    add('ssi section of 11 bytes', z.lay([bytes([0x42, 0xB0, 8]) + bytes(8), _sec(20, 14)]))
    add('short section of 3 bytes', z.lay([P.short_section(0x71, b''), P.short_section(0x72, b'\x01')]))
    add('one byte of payload per packet', z.lay([_sec(200, 15)], cont_af=182), True)
    add('adaptation field leaves one byte: the pointer', z.lay([], af_len=182))
    add('adaptation field leaves no payload with AFC 3', [P.packet(PID, z._next(), b'', af_len=183)])
    add('pointer completes the open section', np.concatenate([first([_sec(300, 16)]), z.lay([_sec(40, 17)], pointer=300 - 183, before=_sec(300, 16)[183:])]), True)
    add('pointer too short for the open section', np.concatenate([first([_sec(300, 18)]), z.lay([_sec(40, 19)], pointer=50, before=_sec(300, 18)[183:])]), True)
    add('pointer longer than the open section needs', np.concatenate([first([_sec(200, 20)]), z.lay([_sec(40, 21)], pointer=60, before=_sec(200, 20)[183:])]), True)
    add('continuation with nothing open', z.other(2, bytes([0x42, 0xB0, 20]) + bytes(30)))
    add('adaptation only in the middle', np.concatenate([first([_sec(400, 22)], 2), [P.packet(PID, z.cc, None, af_len=183)], z.other(1, _sec(400, 22)[183 + 184:])]), True)
    for k, inject in enumerate(P.INJECTORS):
        clean = np.concatenate([z.lay([_sec(5 * 184 - 20, 30 + k)]), z.lay([_sec(33, 40 + k)])])
        add(inject.__name__, inject(clean, 2)[0], True)
    return out


# the cases of edge_cases() that the shared reassembly walk (csrc/ts_reasm.h) takes down a branch of its own
WALK_EDGES = ('header cut after 1 byte', 'header cut after 2 bytes', 'section_length 4094 in a cut header', 'pointer completes the open section',
              'pointer too short for the open section', 'pointer longer than the open section needs')


def walk_cases():
    """further branches of the walk, each for a slot that has seen nothing -> [(name, packets [k, 188], rows, (dropped_sections,
    malformed_sections))]; rows: (table_id, length, first_packet) of the sections the packets give in one call, written out"""
    out = []

    def add(name, ts, rows, counts):
        out.append((name, np.asarray(ts, np.uint8).reshape(-1, P.TS), rows, counts))
    z = P.Packetiser(PID)
    a = _sec(584, 50)                                       # 183 + 184 + 184 + 33 bytes: the third packet is lost
    head = z.lay([a])[:2]
    z.cc = 3
    add('PUSI packet behind a lost packet with a section open', np.concatenate([head, z.lay([_sec(40, 51, 0x43)], pointer=33, before=a[551:])]),
        [(0x43, 40, 2)], (1, 0))
    z = P.Packetiser(PID)
    add('two whole sections and a third cut in its body', z.lay([_sec(60, 52), _sec(70, 53, 0x43), _sec(100, 54, 0x44)]),
        [(0x42, 60, 0), (0x43, 70, 0), (0x44, 100, 0)], (0, 0))
    z = P.Packetiser(PID)
    add('two whole sections and a third cut after 2 header bytes', z.lay([_sec(60, 55), _sec(121, 56, 0x43), _sec(100, 57, 0x44)]),
        [(0x42, 60, 0), (0x43, 121, 0), (0x44, 100, 0)], (0, 0))
    z = P.Packetiser(PID)
    add('ssi section of 11 bytes that ends in the next packet', z.lay([_sec(178, 58), bytes([0x42, 0xB0, 8]) + bytes(8)]), [(0x42, 178, 0)], (0, 1))
    z = P.Packetiser(PID)
    add('ssi section of 11 bytes in a header cut after 1 byte', z.lay([_sec(182, 59), bytes([0x42, 0xB0, 8]) + bytes(8)]), [(0x42, 182, 0)], (0, 1))
    z = P.Packetiser(PID)
    add('stuffing directly behind a section, a section header behind the stuffing', z.lay([_sec(30, 60), b'\xff', _sec(20, 61, 0x43)]), [(0x42, 30, 0)], (0, 0))
    return out


def whole_stream(rng, cases=None):
    """the edge cases back to back with a PAT on PID 0 and packets of an unwatched PID, a TEI packet and a null packet between them"""
    cases = cases or edge_cases()
    zp = P.Packetiser(0)
    parts = []
    for i, (_, ts, _) in enumerate(cases):
        parts += [ts, zp.lay([P.pat(7, [(0, 0x10), (1, PID)], version=i // 9)]), P.filler(0x99, int(rng.integers(0, 3)), rng)]
    tei = P.packet(PID, 0, b'\x00' * 10, pusi=1).copy()
    tei[1] |= 0x80
    parts += [tei.reshape(1, -1), P.packet(0x1FFF, 0).reshape(1, -1)]
    return np.concatenate(parts)
