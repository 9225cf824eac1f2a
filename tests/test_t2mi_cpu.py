"""T2-MI bank without a GPU: the library's host bank (T2miBank.host, csrc/t2mi_rules.h) against the model of tests/t2mi_ref.py in
bytes, rows, counters and frame sizes -- on the constructed cases with their rows written out, for every cutting of a stream into
calls, on random feeds over four slots, and at the capacity limits."""
import numpy as np
import pytest

import psi_ref as S
import t2mi_cases as K
import t2mi_ref as T

PID = K.PID


class Pair:
    """a host bank of one stream and the model, fed the same calls: watches [(slot, pid, plp)]"""

    def __init__(self, pkg, watches=((0, PID, -1),), max_packets=4096, max_rows=1024):
        self.hb, self.m = pkg.T2miBank.host(1, max_packets, max_rows), T.T2mi()
        for slot, pid, plp in watches:
            self.hb.set_watch(0, slot, pid, plp), self.m.set_watch(slot, pid, plp)

    def call(self, ts, deliver=True):
        want = self.m.process(ts, deliver)
        for slot in range(T.SLOTS):
            got = self.hb.work(ts, slot=slot, deliver=deliver)
            assert (got is None) == (want[slot] is None) and (got is None or np.array_equal(got, want[slot])), slot
            assert self.hb.row_table(0, slot) == self.m.table(slot), slot
            assert self.hb.frame_bytes(0, slot) == self.m.frame_bytes(slot), slot
            assert self.hb.stats(0, slot) == self.m.stats(slot), slot
        assert self.hb.stats(0) == self.m.stats()
        return want


def test_layout_and_the_crc_anchor(pkg):
    """a 10-byte packet written by hand: type 0x20, count 1, no payload; its CRC-32/MPEG is 0x1B355226 (checked against zlib on the bit-reversed bytes)"""
    assert pkg.T2miBank.layout() == T.LAYOUT
    anchor = bytes([0x20, 0x01, 0x00, 0x00, 0x00, 0x00, ANCHOR >> 24, ANCHOR >> 16 & 255, ANCHOR >> 8 & 255, ANCHOR & 255])
    assert T.t2mi_packet(0x20, 1, b'') == anchor and S.crc32_mpeg(anchor) == 0
    pair = Pair(pkg)
    pair.call(S.packet(PID, 0, b'\x00' + anchor, pusi=1, af_len=184 - 11 - 1))
    assert pair.m.table(0) == [dict(packet_type=0x20, packet_count=1, superframe_idx=0, stream_id=0, flags=0, plp_id=0, frame_idx=0, payload_bits=0, length=10,
                                    offset=-1, bbframe_bytes=0, first_packet=0, last_packet=0)]
    bad = bytearray(anchor)
    bad[9] ^= 1
    pair.call(S.packet(PID, 1, b'\x00' + bytes(bad), pusi=1, af_len=184 - 11 - 1))
    assert pair.m.table(0)[0]['flags'] == T.CRC_ERROR


ANCHOR = 0x1B355226
CASES = K.edge_cases()


def test_constructed_cases_one_by_one(pkg):
    assert [c[0] for c in CASES] == list(K.ROWS)
    pair = Pair(pkg)
    for name, ts in CASES:
        before = pair.m.stats(0)['packets']
        out = pair.call(ts)[0]
        rows = [tuple(r[k] for k in K.ROW_FIELDS) for r in pair.m.table(0)]
        assert rows == K.ROWS[name], name
        assert pair.m.stats(0)['packets'] - before == len(ts), name
        assert out.size == sum(r[7] for r in rows if r[6] >= 0) and not pair.m.slot[0].buf, name
    st = pair.m.stats(0)
    assert (st['dropped_packets'], st['malformed_packets'], st['scrambled_packets'], st['pointer_slack'], st['bad_payload'], st['crc_errors']) == (4, 2, 1, 1, 4, 5)


def test_walk_cases_whole_and_cut_at_every_packet(pkg):
    """the written-out rows of K.walk_cases(), and the same rows but for the packet indices from two calls cut at every TS packet boundary"""
    for name, ts, rows, dropped in K.walk_cases():
        for at in range(len(ts)):                                    # 0: one call
            pair, got = Pair(pkg), []
            for part in ([ts[:at], ts[at:]] if at else [ts]):
                pair.call(part)
                got += [tuple(r[k] for k in K.ROW_FIELDS) for r in pair.m.table(0)]
            assert [r[:8] for r in got] == [r[:8] for r in rows] and pair.m.stats(0)['dropped_packets'] == dropped, (name, at)
            assert at or got == rows, name


def test_row_fields_of_the_largest_packets(pkg):
    pair = Pair(pkg)
    cases = dict(CASES)
    pair.call(cases['payload_bits 65535: 8202 bytes over 45 TS packets'])
    assert pair.m.table(0) == [dict(packet_type=0x21, packet_count=14, superframe_idx=9, stream_id=5, flags=0, plp_id=0, frame_idx=0, payload_bits=65535, length=8202,
                                    offset=-1, bbframe_bytes=0, first_packet=0, last_packet=44)]
    out = pair.call(cases['BBFRAME of 7274 bytes'])[0]
    assert bytes(out) == K._bytes(7274, 2)
    assert pair.m.table(0) == [dict(packet_type=0, packet_count=15, superframe_idx=0, stream_id=0, flags=T.BBFRAME | T.INTL_FRAME_START, plp_id=3, frame_idx=200,
                                    payload_bits=58216, length=7287, offset=0, bbframe_bytes=7274, first_packet=0, last_packet=39)]


@pytest.mark.parametrize('per_call', [1, 7])
def test_every_cutting_into_calls(pkg, per_call):
    ts = K.whole_stream()
    whole, cut = Pair(pkg), Pair(pkg)
    want = whole.call(ts)[0]
    got, rows = [], 0
    for a in range(0, len(ts), per_call):
        got.append(cut.call(ts[a:a + per_call])[0])
        rows += len(cut.m.table(0))
    assert np.array_equal(np.concatenate(got), want) and rows == len(whole.m.table(0)) == sum(len(r) for r in K.ROWS.values())
    assert cut.m.stats() == whole.m.stats()
    carried = Pair(pkg)                                              # rows only: the same rows but for offsets, no bytes
    assert carried.call(ts, deliver=False)[0] is None
    assert [dict(r, offset=-1) for r in whole.m.table(0)] == carried.m.table(0) and carried.m.stats()['bytes_delivered'] == 0


def random_feed(rng, pids, n_packets, plps=(0, 3, 7)):
    """T2-MI feeds on `pids` with BBFRAMEs of several PLPs, other packet types and faults, interleaved with a filler PID"""
    streams = []
    for pid in pids:
        z, parts, count = T.Packetiser(pid, cc=int(rng.integers(16))), [], int(rng.integers(256))
        while sum(len(p) for p in parts) < n_packets:
            pk = []
            for _ in range(int(rng.integers(1, 6))):
                count = (count + 1 + (rng.random() < 0.05)) & 255
                kind = rng.random()
                if kind < 0.6:
                    pk.append(T.bb_packet(count, int(rng.choice(plps)), bytes(rng.integers(0, 256, int(rng.choice([10, 60, 183, 900, 3000])), dtype=np.uint8)),
                                          frame_idx=count, start=int(rng.integers(2))))
                elif kind < 0.8:
                    pk.append(T.t2mi_packet(int(rng.choice([0x10, 0x20, 0x21])), count, bytes(rng.integers(0, 256, int(rng.integers(0, 40)), dtype=np.uint8))))
                else:
                    pk.append(T.t2mi_packet(0, count, bytes(rng.integers(0, 256, 20, dtype=np.uint8)), payload_bits=int(rng.integers(0, 160))))
            ts = z.lay(pk, flush=rng.random() < 0.5, af_len=None if rng.random() < 0.8 else int(rng.integers(0, 100)))
            if len(ts) > 2 and rng.random() < 0.5:
                ts = S.INJECTORS[int(rng.integers(len(S.INJECTORS)))](ts, int(rng.integers(1, len(ts) - 1)))[0]
            parts.append(ts)
        streams.append(np.concatenate(parts)[:n_packets])
    streams.append(S.filler(0x99, n_packets // 4, rng))
    return S.interleave(rng, streams)


@pytest.mark.parametrize('seed', [1, 2, 3])
def test_random_feeds_over_four_slots(pkg, seed):
    rng = np.random.default_rng(seed)
    ts = random_feed(rng, [0x1000, 0x1001, 0x1002], 300)
    pair = Pair(pkg, watches=[(0, 0x1000, 3), (1, 0x1001, -1), (2, 0x1000, -1), (3, 0x1002, 7)])     # PID 0x1000 in two slots with different PLPs
    a = 0
    while a < len(ts):
        n = int(rng.integers(1, 120))
        pair.call(ts[a:a + n], deliver=rng.random() < 0.8)
        a += n
    st = [pair.m.stats(k) for k in range(4)]
    assert all(s['t2mi_packets'] > 50 and s['bbframes'] > 20 for s in st)
    assert st[0]['t2mi_packets'] == st[2]['t2mi_packets'] and 0 < st[0]['bbframes_delivered'] < st[2]['bbframes_delivered']
    tot = pair.m.stats()
    assert min(tot[k] for k in ('crc_errors', 'count_errors', 'bad_payload', 'dropped_packets', 'scrambled_packets')) > 0, tot


def test_capacity_failure_then_the_repeated_call(pkg):
    ts = K.whole_stream()
    head, rest = ts[:60], ts[60:]
    probe = Pair(pkg)
    probe.call(head)
    need = probe.call(rest)[0].size
    rows = len(probe.m.table(0))
    pair = Pair(pkg)
    pair.call(head)
    before = pair.hb.stats(0)
    with pytest.raises(pkg.Dvbs2GpuError) as e:
        pair.hb.work(rest, cap=need - 1)
    assert e.value.code == -5 and (e.value.needed, e.value.rows) == (need, rows)
    assert pair.hb.stats(0) == before and pair.hb.row_table(0, 0) == [] and pair.hb.frame_bytes(0, 0) == []
    pair.call(rest)                                                  # the repeat, with room, equals the model
    small = Pair(pkg, max_rows=rows - 1)
    small.call(head)
    before = small.hb.stats(0)
    with pytest.raises(pkg.Dvbs2GpuError) as e:
        small.hb.work(rest)
    assert e.value.code == -5 and (e.value.needed, e.value.rows) == (-1, rows) and small.hb.stats(0) == before
    again = pkg.T2miBank.host(1, 4096, rows)                          # exactly enough rows
    again.set_watch(0, 0, PID)
    again.work(head), again.work(rest)
    assert again.row_table(0, 0) == probe.m.table(0)


def test_watch_rules(pkg):
    hb = pkg.T2miBank.host(2, 64, 16)
    hb.set_watch(1, 0, 0x40, 3), hb.set_watch(1, 3, 0x40, -1)        # the same PID in two slots is allowed
    for bad in ((1, 4, 0x40, 0), (2, 0, 0x40, 0), (0, 0, 0x1FFF, 0), (0, 0, 0x40, 256), (0, 0, -2, 0)):
        with pytest.raises(pkg.Dvbs2GpuError):
            hb.set_watch(*bad)
    ts = T.Packetiser(0x40).lay([T.bb_packet(0, 3, bytes(range(20)))])
    assert bytes(hb.work(ts, stream=1, slot=0)) == bytes(range(20)) and hb.stats(1, 0)['bbframes_delivered'] == 1
    assert hb.stats(1, 3)['packets'] == 0                            # work() serves one slot
    hb.set_watch(1, 0, 0x40, 4)                                      # a changed watch starts the slot afresh
    assert hb.stats(1, 0)['packets'] == 0 and hb.row_table(1, 0) == []
    hb.reset()
    assert hb.stats(1)['packets'] == 0
    with pytest.raises(pkg.Dvbs2GpuError):
        pkg.T2miBank.host(1, 4097, 16)
