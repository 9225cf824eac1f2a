"""ULE bank without a GPU: the library's host bank (UleBank.host, csrc/ule_rules.h) against the model of tests/ule_ref.py in bytes,
rows, counters, needed sizes and state through the next call -- on the constructed cases with their rows written out, whole and cut
into calls of 1, 7 and 64 packets and in two at every packet boundary, on seeded random feeds (whose floors are checked on the model
alone first), at the capacity limits, with several filters on one PID and across a watch change."""
import numpy as np
import pytest

import ule_cases as K
import ule_ref as R

PID = K.PID
CASES = K.edge_cases()
MAIN, NO_ACCEPT = (0, PID, K.NPA, K.MASK, True), (1, PID, K.NPA, K.MASK, False)
# what a random feed must have met before anything is compared: every counter that a rule steps
FLOOR_KEYS = ('crc_errors', 'filtered', 'no_address', 'test', 'bridged', 'extension', 'other_protocol', 'bad_ip', 'datagrams', 'datagrams_delivered',
              'bytes_delivered', 'dropped_sndus', 'malformed_sndus', 'slack', 'malformed_packets', 'scrambled_packets')


class Pair:
    """a host bank of one stream and the model, fed the same calls: watches [(slot, pid, npa, mask, accept_unaddressed)]"""

    def __init__(self, pkg, watches=(MAIN,), max_packets=4096, max_rows=1024):
        self.hb, self.m = pkg.UleBank.host(1, max_packets, max_rows), R.Ule()
        for w in watches:
            self.hb.set_watch(0, *w), self.m.set_watch(*w)

    def call(self, ts, deliver=True):
        want = self.m.process(ts, deliver)
        for slot in range(R.SLOTS):
            got = self.hb.work(ts, slot=slot, deliver=deliver)
            assert (got is None) == (want[slot] is None) and (got is None or np.array_equal(got, want[slot])), slot
            assert self.hb.row_table(0, slot) == self.m.table(slot), slot
            assert self.hb.stats(0, slot) == self.m.stats(slot), slot
            assert self.hb.needed(0, slot) == (want[slot].size if deliver else 0, len(self.m.table(slot))), slot
        assert self.hb.stats(0) == self.m.stats()
        return want


def rows_of(table, fields=K.ROW_FIELDS):
    return [tuple(r[k] for k in fields) for r in table]


def test_layout_and_the_published_checksums(pkg):
    assert pkg.UleBank.layout() == R.LAYOUT
    lay = R.LAYOUT
    assert lay['head_bytes'] == lay['header_bytes'] + lay['npa_bytes'] + lay['max_extension_bytes'] + lay['mac_header_bytes'] + 60 + 4 == 128
    assert R.crc32_mpeg(b'123456789') == 0x0376E6E7
    hdr = bytes.fromhex('450000730000400040110000c0a80001c0a800c7')
    assert R.inet_checksum(hdr) == 0xB861
    # the same header, by the library: a datagram of 0x73 bytes with the published checksum is a DATAGRAM, with another one BAD_IP
    pair = Pair(pkg, watches=[(0, PID, None, None, False)])
    good = hdr[:10] + b'\xb8\x61' + hdr[12:] + bytes(0x73 - 20)
    z = R.Packetiser(PID)
    pair.call(z.lay([R.sndu(0x0800, good, npa=K.GROUP)]))
    assert rows_of(pair.m.table(0), ('flags', 'bytes', 'src4', 'dst4', 'src_port')) == [(R.DATAGRAM, 0x73, 0xC0A80001, 0xC0A800C7, 0)]
    pair.call(z.lay([R.sndu(0x0800, good[:11] + b'\x60' + good[12:], npa=K.GROUP)]))
    assert pair.m.table(0)[0]['flags'] == R.BAD_IP
    # the CRC of an SNDU written out byte by byte: D = 1, Length 8, Type 0x0000, four bytes, and the register over all of it is 0
    test = bytes([0x80, 0x08, 0x00, 0x00, 1, 2, 3, 4])
    assert R.sndu(0, bytes([1, 2, 3, 4])) == test + R.crc32_mpeg(test).to_bytes(4, 'big') and R.crc32_mpeg(R.sndu(0, bytes([1, 2, 3, 4]))) == 0


def test_constructed_cases_one_by_one(pkg):
    assert [c[0] for c in CASES] == list(K.ROWS) and set(K.ROWS_NO_ACCEPT) < set(K.ROWS)
    pair = Pair(pkg, watches=[MAIN, NO_ACCEPT])
    flags = 0
    for name, ts in CASES:
        before = pair.m.stats(0)['packets']
        out = pair.call(ts)[0]
        rows = rows_of(pair.m.table(0))
        assert rows == K.ROWS[name], name
        if name in K.ROWS_NO_ACCEPT:
            assert rows_of(pair.m.table(1)) == K.ROWS_NO_ACCEPT[name], name
        else:
            assert pair.m.table(1) == pair.m.table(0), name
        assert pair.m.stats(0)['packets'] - before == len(ts), name
        assert out.size == sum(r[12] for r in rows if r[11] >= 0) and not pair.m.slot[0].buf, name
        for r in rows:
            flags |= r[0]
    assert flags == 1023                                             # every row flag in a case
    assert pair.m.stats(0) == K.STATS and pair.m.stats(1) == K.STATS_NO_ACCEPT
    assert all(K.STATS[k] > 0 for k in FLOOR_KEYS if k != 'malformed_packets')


@pytest.mark.parametrize('half', [0, 1])
def test_every_case_whole_and_cut_in_two_at_every_packet(pkg, half):
    """each case by itself on a fresh bank, in one call and cut in two at every TS packet boundary (for the long ones: at the first
    and last 12): the same rows but for the packet indices, which count from a call's start, and the offsets, which count in a call's
    buffer"""
    skip = ('offset', 'first_packet', 'last_packet')
    key = lambda r, off: tuple(r[f] for f in K.ROW_FIELDS if f not in skip) + (r['offset'] + off if r['offset'] >= 0 else -1,)
    for name, ts in CASES[half::2]:
        whole = None
        cuts = [a for a in range(len(ts)) if a < 12 or a > len(ts) - 12]
        for at in cuts:                                                # 0: one call
            pair, got, off, data = Pair(pkg), [], 0, []
            for part in ([ts[:at], ts[at:]] if at else [ts]):
                data.append(pair.call(part)[0])
                got += [key(r, off) for r in pair.m.table(0)]
                off += data[-1].size
            res = (got, pair.m.stats(0), bytes(np.concatenate(data)))
            if at == 0:
                whole = res
                assert rows_of(pair.m.table(0)) == K.ROWS[name], name
            assert res == whole and not pair.m.slot[0].buf, (name, at)


@pytest.mark.parametrize('per_call', [1, 7, 64])
def test_every_cutting_into_calls(pkg, per_call):
    ts = K.whole_stream(CASES)
    whole, cut = Pair(pkg), Pair(pkg)
    want = whole.call(ts)[0]
    got, rows = [], 0
    for a in range(0, len(ts), per_call):
        got.append(cut.call(ts[a:a + per_call])[0])
        rows += len(cut.m.table(0))
    assert np.array_equal(np.concatenate(got), want) and rows == len(whole.m.table(0)) == sum(len(r) for r in K.ROWS.values())
    assert cut.m.stats() == whole.m.stats() == K.STATS
    carried = Pair(pkg)                                              # rows only: the same rows but for offsets, no bytes
    assert carried.call(ts, deliver=False)[0] is None
    assert [dict(r, offset=-1) for r in whole.m.table(0)] == carried.m.table(0) and carried.m.stats()['bytes_delivered'] == 0


@pytest.mark.parametrize('seed,per_call', [(1, 0), (3, 1), (4, 7), (5, 64)])
def test_wild_packets_whole_and_cut_into_calls(pkg, seed, per_call):
    """the floors first, on the model alone: more than 1000 packets, 200 SNDUs and 30 datagrams, and every counter that a rule steps
    above zero; then host bank == model, call by call"""
    ts = K.wild_packets(seed, 1500)
    probe = R.Slot(0x40, K.NPA, K.MASK, True)
    probe.process(ts)
    st = probe.st
    assert st['packets'] > 1000 and st['sndus'] > 200 and st['datagrams'] > 30, st
    assert min(st[k] for k in FLOOR_KEYS) > 0, st
    pair = Pair(pkg, watches=[(0, 0x40, K.NPA, K.MASK, True), (1, 0x41, None, None, False), (3, 0x40, K.GROUP, b'\xff' * 6, False)])
    step = per_call or len(ts)
    for a in range(0, len(ts), step):
        pair.call(ts[a:a + step], deliver=(a // step) % 5 != 4)
    assert pair.m.stats(0)['sndus'] == st['sndus'] == pair.m.stats(3)['sndus'] and pair.m.stats(3)['filtered'] > pair.m.stats(0)['filtered']


def test_capacity_failure_then_the_repeated_call(pkg):
    ts = K.whole_stream(CASES)
    head, rest = ts[:30], ts[30:]                                    # the cut lies inside the largest SNDU: it is open at the failure
    probe = Pair(pkg)
    probe.call(head)
    assert probe.m.slot[0].buf
    need = probe.call(rest)[0].size
    rows = len(probe.m.table(0))
    pair = Pair(pkg)
    pair.call(head)
    before = pair.hb.stats(0)
    with pytest.raises(pkg.Dvbs2GpuError) as e:
        pair.hb.work(rest, cap=need - 1)
    assert e.value.code == -5 and (e.value.needed, e.value.rows) == (need, rows) == pair.hb.needed(0, 0)
    assert pair.hb.stats(0) == before and pair.hb.row_table(0, 0) == []
    pair.call(rest)                                                  # the repeat, with room, equals the model
    small = Pair(pkg, max_rows=rows - 1)
    small.call(head)
    before = small.hb.stats(0)
    with pytest.raises(pkg.Dvbs2GpuError) as e:
        small.hb.work(rest)
    assert e.value.code == -5 and (e.value.needed, e.value.rows) == (-1, rows) and small.hb.stats(0) == before
    again = pkg.UleBank.host(1, 4096, rows)                          # exactly enough rows
    again.set_watch(0, *MAIN)
    again.work(head), again.work(rest)
    assert again.row_table(0, 0) == probe.m.table(0)


def test_four_slots_on_one_pid_with_different_filters(pkg):
    a, b = bytes.fromhex('02aabbccdd01'), bytes.fromhex('02aabbccdd02')
    ts = R.Packetiser(PID).lay([K.ip4(100 + i, i, npa=(a, b, a, None)[i % 4]) for i in range(12)])
    pair = Pair(pkg, watches=[(0, PID, a, b'\xff' * 6, False), (3, PID, b, b'\xff' * 6, True), (1, PID, None, None, False), (2, PID, None, None, True)])
    out = pair.call(ts[:4]), pair.call(ts[4:])
    st = [pair.m.stats(k) for k in range(4)]
    assert [(s['sndus'], s['datagrams'], s['filtered'], s['no_address']) for s in st] == [(12, 6, 6, 3), (12, 9, 3, 3), (12, 12, 0, 3), (12, 6, 6, 3)]
    assert sum(o[0].size for o in out) == sum(100 + i for i in range(0, 12, 2)) and sum(o[3].size for o in out) == sum(100 + i for i in (1, 5, 9, 3, 7, 11))


def test_a_watch_change_restarts_a_slot(pkg):
    ts = dict(CASES)['a 1400-byte datagram over 8 packets']
    pair = Pair(pkg)
    pair.call(ts[:4])
    assert pair.m.slot[0].buf and pair.hb.stats(0, 0)['packets'] == 4
    pair.hb.set_watch(0, *MAIN), pair.m.set_watch(*MAIN)             # the same watch again: the open SNDU is gone
    assert pair.hb.stats(0, 0)['packets'] == 0 and pair.hb.row_table(0, 0) == []
    pair.call(ts[4:])
    assert pair.m.table(0) == [] and pair.m.stats(0)['dropped_sndus'] == 0 and pair.m.stats(0)['packets'] == 4
    pair.call(ts)
    assert pair.m.table(0)[0]['bytes'] == 1400
    pair.hb.reset()
    assert pair.hb.stats(0)['packets'] == 0


def test_watch_rules(pkg):
    hb = pkg.UleBank.host(2, 64, 16)
    hb.set_watch(1, 0, 0x40, K.GROUP, b'\xff' * 6), hb.set_watch(1, 3, 0x40)      # the same PID in two slots is allowed
    for bad in ((1, 4, 0x40), (2, 0, 0x40), (0, 0, 0x1FFF), (0, 0, -2)):
        with pytest.raises(pkg.Dvbs2GpuError):
            hb.set_watch(*bad)
    with pytest.raises(ValueError):
        hb.set_watch(0, 0, 0x40, b'\x01\x02')
    ts = R.Packetiser(0x40).lay([K.ip4(40, 1)])
    assert hb.work(ts, stream=1, slot=0).size == 40 and hb.stats(1, 0)['datagrams_delivered'] == 1
    assert hb.stats(1, 3)['packets'] == 0                            # work() serves one slot
    with pytest.raises(pkg.Dvbs2GpuError):
        pkg.UleBank.host(1, 4097, 16)
    assert not hasattr(pkg.UleBank, 'follow_pmts')                   # the caller names the PID
