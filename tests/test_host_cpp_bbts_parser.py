"""csrc/bbts_host.h (BbtsHostParser: the reference-mode fallback of every GSE call the kernels hand back) on its own, driven by
tests/cpp/bbts_host_parser.cpp: no GPU, no HIP header.  Every case is cut into calls of 1 to 5 frames and compared call by call with
oracle/bbframe_ts.cpp for all the oracle exposes (output bytes, the header / stat words, synched, count); rows and counters, which the
oracle does not have, are checked against what the case transmitted."""
import os
import subprocess

import numpy as np
import pytest

import orc_bbts as B
import test_gpu_gse as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, 'tests', 'cpp', 'build', 'bbts_host_parser')
COUNTERS = ('frames', 'packets', 'complete_pdus', 'reassembled_pdus', 'crc_failures', 'dropped_no_slot', 'dropped_overflow', 'dropped_no_fit',
            'bytes_delivered')


@pytest.fixture(scope='module')
def exe():
    os.makedirs(os.path.dirname(EXE), exist_ok=True)
    cmd = ['g++', '-std=c++17', '-O1', '-Wall', '-Wextra', '-Werror', '-I' + os.path.join(ROOT, 'sdrpp-dvbs-demodulator_amd', 'csrc'),
           os.path.join(ROOT, 'tests', 'cpp', 'bbts_host_parser.cpp'), '-o', EXE]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return EXE


def cut_calls(n, pattern=(2, 5, 1, 4, 3, 1)):
    cuts = []
    while n:
        cuts.append(min(pattern[len(cuts) % len(pattern)], n))
        n -= cuts[-1]
    return cuts


def run_case(exe, tmp_path, kbch, frames, cuts, cap=None):
    """frames cut into calls of cuts[k] frames through the driver and the oracle; returns (outputs per call, rows per call, counters)"""
    fb = kbch // 8
    frames = np.ascontiguousarray(frames, np.uint8).reshape(-1, fb)
    assert len(frames) <= 16 and sum(cuts) == len(frames) and all(1 <= c <= 5 for c in cuts)
    cap = cap if cap is not None else 5 * fb + 376 + 3 * 65536
    with open(tmp_path / 'in.bin', 'wb') as f:
        f.write(np.array([kbch, cap, len(cuts)] + list(cuts), np.int32).tobytes())
        f.write(frames.tobytes())
    r = subprocess.run([exe, str(tmp_path / 'in.bin'), str(tmp_path / 'out.bin')], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr
    out = np.fromfile(tmp_path / 'out.bin', np.uint8)
    lines = [l.split() for l in r.stdout.splitlines()]
    assert lines[-1][0] == 'gse' and sum(l[0] == 'call' for l in lines) == len(cuts)
    counters = dict(zip(COUNTERS, map(int, lines[-1][1:])))
    orc = B.OracleBbTs(kbch)
    outs, tables, at, f0 = [], [], 0, 0
    for l in lines[:-1]:
        if l[0] == 'row':
            tables[-1].append(tuple(int(x) for x in l[1:]))
            continue
        n, st = int(l[1]), dict(zip(B.STAT_KEYS, map(int, l[2:])))
        want = orc.work(frames[f0:f0 + cuts[len(outs)]], cap=cap)
        f0 += cuts[len(outs)]
        got = out[at:at + max(n, 0)]
        at += max(n, 0)
        if want is None:
            assert n == -5
        else:
            assert n == want.size and np.array_equal(got, want), (len(outs), n, want.size)
        ws = orc.stats()
        keys = [k for k in B.STAT_KEYS if k != 'count' or ws['synched']]
        assert {k: st[k] for k in keys} == {k: ws[k] for k in keys}, len(outs)
        outs.append(got)
        tables.append([])
    assert at == out.size
    for o, rows in zip(outs, tables):             # every row is a GRE packet inside its call's output, in order, none overlapping
        end = 0
        for off, n, proto, flags in rows:
            assert off >= end and off + n <= o.size and bytes(o[off:off + 2]) == b'\0\0' and flags < 4
            if proto in (0x0800, 0x86DD):
                assert bytes(o[off + 2:off + 4]) == bytes([proto >> 8, proto & 0xff])
            end = off + n
    assert counters['bytes_delivered'] == sum(n for rows in tables for _, n, _, _ in rows)
    assert counters['complete_pdus'] + counters['reassembled_pdus'] == sum(map(len, tables))
    return outs, tables, counters


def test_well_formed_mixed_ts_and_gse(exe, tmp_path):
    kbch = 14232
    rng = np.random.default_rng(50)
    D = kbch // 8 - 10
    tsp = B.ts_packets(6 * D // 188 + 2, rng)
    ts = B.bbframes_from_ts(tsp, kbch, 6)
    pk, want = T.transmitter(rng, 4.3 * D)
    g = T.pack_frames(pk, kbch)
    assert 5 <= len(g) <= 10
    order = [ts[0], g[0], ts[1], ts[2], g[1], g[2], g[3], ts[3], ts[4], g[4], ts[5]] + list(g[5:])
    outs, tables, c = run_case(exe, tmp_path, kbch, np.stack(order), [3, 1, 5, 2] + [1] * (len(order) - 11))
    got = [(bytes(o[off:off + n]), proto, flags) for o, rows in zip(outs, tables) for off, n, proto, flags in rows]
    assert got == [(T.gre(p, d), p, (1 if reasm else 0) | (2 if lab else 0)) for p, d, reasm, lab in want]
    mask = [np.ones(o.size, bool) for o in outs]
    for m, rows in zip(mask, tables):
        for off, n, _, _ in rows:
            m[off:off + n] = False
    assert np.array_equal(np.concatenate([o[m] for o, m in zip(outs, mask)]).reshape(-1, 188), tsp[:(6 * D - 1) // 188])
    assert c['frames'] == len(g) and c['packets'] >= len(pk) - 20 and c['dropped_no_fit'] == 0


@pytest.mark.parametrize('kbch', [3072, 14232])
def test_well_formed_gse(exe, tmp_path, kbch):
    pk, want = T.transmitter(np.random.default_rng(kbch), 13 * (kbch // 8 - 10), max_pdu=(kbch // 8 - 30))
    g = T.pack_frames(pk, kbch)[:16]
    outs, tables, c = run_case(exe, tmp_path, kbch, g, cut_calls(len(g)))
    got = [bytes(o[off:off + n]) for o, rows in zip(outs, tables) for off, n, _, _ in rows]
    assert len(got) > 10 and got == [T.gre(p, d) for p, d, _, _ in want][:len(got)]     # a prefix: the 16 frames may end inside a PDU
    assert c['frames'] == len(g)


def test_rejected_header_then_resync(exe, tmp_path):
    kbch = 14232
    fb, rng = kbch // 8, np.random.default_rng(60)
    pk, _ = T.transmitter(rng, 8 * (fb - 10), max_pdu=600)
    g = T.pack_frames(pk, kbch)
    assert len(g) >= 8
    bad = g[2].copy(); bad[9] ^= 0x5a                               # BBHEADER CRC-8: the frame is lost, the next one resynchronises
    nxt = g[3].copy(); nxt[:10] = B.bbheader(1, (fb - 10) * 8, syncd_bits=24 * 8)     # ... SYNCD/8 + 1 bytes in, for DFL/8 bytes
    issy = g[4].copy(); issy[:10] = B.bbheader(1, (fb - 10) * 8, 0, issyi=1)          # ISSY, NPD: GSE frames that are not walked
    npd = g[5].copy(); npd[:10] = B.bbheader(1, (fb - 10) * 8, 0, npd=1)
    long_ = g[6].copy()                                             # a complete packet announcing more bytes than the call has left
    long_[10:14] = [0xC0 | 0x20 | 0x0f, 0xff, 0x08, 0x00]
    frames = [g[0], g[1], bad, nxt, g[4], issy, npd, g[5], g[6], long_, long_, g[7], g[0], g[1]]
    outs, tables, c = run_case(exe, tmp_path, kbch, np.stack(frames), [5, 3, 2, 4])
    assert c['frames'] == 11 and tables[-1][0] == (0, 4097, 0x0800, 0)           # the same packet with enough frames behind it is a packet


def test_more_packets_in_a_frame_than_the_device_has_records(exe, tmp_path):
    kbch = 14232
    rng = np.random.default_rng(70)
    small = [B.gse_complete(0x0800, rng.integers(0, 256, 1, dtype=np.uint8)) for _ in range(T.PKT_CAP + 1)]     # 5 bytes each
    frames = np.stack([B.gse_bbframe([], kbch), B.gse_bbframe(small, kbch), B.gse_bbframe(small[:7], kbch)])
    outs, tables, c = run_case(exe, tmp_path, kbch, frames, [2, 1])
    assert len(tables[0]) == T.PKT_CAP + 1 and c['packets'] == T.PKT_CAP + 8 and c['complete_pdus'] == c['packets']


def test_corrupted_end_crc_and_a_fourth_open_pdu(exe, tmp_path):
    kbch = 3072
    rng = np.random.default_rng(80)
    pdus = [rng.integers(0, 256, 400, dtype=np.uint8).tobytes() for _ in range(5)]
    fr = [T.fragments(0x0800 if k % 2 else 0x88B5, pdus[k], [150, 300], 10 + k, label=bytes(6) if k == 1 else None, corrupt_crc=(k == 2)) for k in range(5)]
    # four PDUs are started: the fourth finds no slot and all its fragments are ignored; the third fails its CRC-32 at its END; the
    # fifth takes the slot the first has left
    pk = [fr[0][0], fr[1][0], fr[2][0], fr[3][0], fr[0][1], fr[3][1], fr[1][1], fr[2][1], fr[0][2], fr[4][0], fr[3][2], fr[2][2], fr[1][2], fr[4][1], fr[4][2]]
    g = T.pack_frames(pk, kbch)
    assert 5 < len(g) <= 16
    outs, tables, c = run_case(exe, tmp_path, kbch, g, cut_calls(len(g), (1, 2, 1, 3, 5, 4)))
    got = [bytes(o[off:off + n]) for o, rows in zip(outs, tables) for off, n, _, _ in rows]
    assert got == [T.gre(0x88B5, pdus[0]), T.gre(0x0800, pdus[1]), T.gre(0x88B5, pdus[4])]
    assert [fl for rows in tables for _, _, _, fl in rows] == [1, 3, 1]
    assert (c['crc_failures'], c['dropped_no_slot'], c['reassembled_pdus'], c['packets']) == (1, 1, 3, len(pk))


def test_fragment_that_would_pass_64_kib(exe, tmp_path):
    """normal frames for this one case: sixteen frames of 1779 bytes cannot fill a 64 KiB reassembly buffer"""
    kbch = 58192
    rng = np.random.default_rng(90)
    pdu = rng.integers(0, 256, 60 * 1024, dtype=np.uint8).tobytes()
    fr = T.fragments(0x0800, pdu, list(range(3600, len(pdu), 3600)), 7)
    # 1 + 18 fragments of 3600 bytes under one START: the last would pass 64 KiB and frees the slot; the END that follows finds no
    # PDU; a new START with the same id is taken
    over = [fr[0]] + [fr[1]] * 18 + [fr[-1]] + T.fragments(0x86DD, pdu[:3000], [1000], 7)
    g = T.pack_frames(over, kbch)
    assert len(g) <= 16
    outs, tables, c = run_case(exe, tmp_path, kbch, g, [5, 5] + [1] * (len(g) - 10))
    assert (c['dropped_overflow'], c['reassembled_pdus'], c['crc_failures']) == (1, 1, 0)
    assert bytes(np.concatenate(outs)) == T.gre(0x86DD, pdu[:3000])


def _packet(head, frag_id, body):
    n = 1 + len(body)
    return bytes([head | n >> 8, n & 0xff, frag_id]) + bytes(body)


def test_end_shorter_than_its_crc(exe, tmp_path):
    """The reference takes the four bytes before the END packet's end as the received CRC-32 and the reassembled length as
    fill + payload - 4, whatever the payload's length: a 3-byte END whose frag id and payload are the register's bytes passes and
    delivers the START's payload less one byte; a 2-byte END after an empty START passes too and has the length -2: dropped."""
    kbch = 3072
    rng = np.random.default_rng(100)
    data = rng.integers(0, 256, 10, dtype=np.uint8).tobytes()
    head = bytes([0, 12, 0x08, 0x00])                               # total length, protocol type
    crc = B.crc32_mpeg(head + data).to_bytes(4, 'big')
    a = [_packet(0xA0, crc[0], head + data), _packet(0x70, crc[0], crc[1:])]
    # empty START: the register is the CRC-32 of total length and protocol type; the END's length byte (3), its frag id and two payload bytes must equal it
    tl = next(t for t in range(65536) if B.crc32_mpeg(bytes([t >> 8, t & 0xff, 0x08, 0x00])) >> 24 == 3)
    crc2 = B.crc32_mpeg(bytes([tl >> 8, tl & 0xff, 0x08, 0x00])).to_bytes(4, 'big')
    b = [_packet(0xA0, crc2[1], bytes([tl >> 8, tl & 0xff, 0x08, 0x00])), _packet(0x70, crc2[1], crc2[2:])]
    bad = [_packet(0xA0, 9, head + data), _packet(0x70, 9, b'\1\2')]                 # and one whose four bytes are not the register
    frames = np.stack([B.gse_bbframe([], kbch), B.gse_bbframe(a, kbch), B.gse_bbframe(b[:1], kbch), B.gse_bbframe(b[1:] + bad, kbch)])
    outs, tables, c = run_case(exe, tmp_path, kbch, frames, [2, 1, 1])
    assert bytes(outs[0]) == T.gre(0x0800, data[:9]) and tables[0] == [(0, 13, 0x0800, 1)]
    assert (c['reassembled_pdus'], c['dropped_no_fit'], c['crc_failures'], c['packets']) == (1, 1, 1, 6)


def test_small_cap_stops_after_a_frame_and_drops_what_does_not_fit(exe, tmp_path):
    kbch = 3072
    rng = np.random.default_rng(110)
    D = kbch // 8 - 10
    ts = B.bbframes_from_ts(B.ts_packets(3 * D // 188 + 2, rng), kbch, 3)
    big, small = rng.integers(0, 256, 300, dtype=np.uint8).tobytes(), rng.integers(0, 256, 60, dtype=np.uint8).tobytes()
    gf = B.gse_bbframe([B.gse_complete(0x0800, big), B.gse_complete(0x86DD, small)], kbch)
    # cap 250: after the first TS frame's packet no more than 188 bytes are left, so the call stops there (.cpp:206-209) and the frames
    # behind it are not parsed; the 300-byte PDU never fits and is dropped, the 60-byte one is delivered
    outs, tables, c = run_case(exe, tmp_path, kbch, np.stack([ts[0], ts[1], ts[2], gf]), [3, 1], cap=250)
    assert outs[0].size == 188 and bytes(outs[1]) == T.gre(0x86DD, small)
    assert (c['dropped_no_fit'], c['complete_pdus']) == (1, 1)
    # less than one packet of room with a whole packet waiting: undefined in the reference, an error here and in the oracle
    outs, _, _ = run_case(exe, tmp_path, kbch, ts[:2], [1, 1], cap=100)
    assert all(o.size == 0 for o in outs)
