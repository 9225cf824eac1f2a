"""MPE bank without a GPU: the library's host bank (MpeBank.host, csrc/mpe_rules.h) against the model of tests/mpe_ref.py in bytes,
rows, counters, needed sizes and state through the next call -- on the constructed cases with their rows written out, whole and cut in
two at every packet boundary, on random feeds over four slots, at the capacity limits, with two MAC filters on one PID, across a watch
change, and behind a PSI bank's PMTs."""
import numpy as np
import pytest

import mpe_cases as K
import mpe_ref as R
import psi_ref as S

PID = K.PID
CASES = K.edge_cases()


class Pair:
    """a host bank of one stream and the model, fed the same calls: watches [(slot, pid, mac, mask)]"""

    def __init__(self, pkg, watches=((0, PID, K.MAC, K.MASK),), max_packets=4096, max_rows=1024):
        self.hb, self.m = pkg.MpeBank.host(1, max_packets, max_rows), R.Mpe()
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
    assert pkg.MpeBank.layout() == R.LAYOUT
    assert R.crc32_mpeg(b'123456789') == 0x0376E6E7 == S.crc32_mpeg(b'123456789')
    hdr = bytes.fromhex('450000730000400040110000c0a80001c0a800c7')
    assert R.inet_checksum(hdr) == 0xB861
    # the same header, by the library: a datagram of 0x73 bytes with the published checksum is a DATAGRAM, with another one BAD_IP
    pair = Pair(pkg, watches=[(0, PID, None, None)])
    good = hdr[:10] + b'\xb8\x61' + hdr[12:] + bytes(0x73 - 20)
    z = R.Packetiser(PID)
    pair.call(z.lay([R.section(good)]))
    assert rows_of(pair.m.table(0), ('flags', 'bytes', 'src4', 'dst4', 'src_port')) == [(R.DATAGRAM, 0x73, 0xC0A80001, 0xC0A800C7, 0)]
    pair.call(z.lay([R.section(good[:11] + b'\x60' + good[12:])]))
    assert pair.m.table(0)[0]['flags'] == R.BAD_IP


def test_constructed_cases_one_by_one(pkg):
    assert [c[0] for c in CASES] == list(K.ROWS)
    pair = Pair(pkg)
    for name, ts in CASES:
        before = pair.m.stats(0)['packets']
        out = pair.call(ts)[0]
        rows = rows_of(pair.m.table(0))
        assert rows == K.ROWS[name], name
        assert pair.m.stats(0)['packets'] - before == len(ts), name
        assert out.size == sum(r[12] for r in rows if r[11] >= 0) and not pair.m.slot[0].buf, name
    assert pair.m.stats(0) == K.STATS


@pytest.mark.parametrize('half', [0, 1])
def test_every_case_whole_and_cut_in_two_at_every_packet(pkg, half):
    """each case by itself on a fresh bank, in one call and cut in two at every TS packet boundary: the same rows but for the packet
    indices, which count from a call's start, and the offsets, which count in a call's buffer"""
    key = lambda r, off: tuple(r[f] for f in K.ROW_FIELDS[:11]) + (r['offset'] + off if r['offset'] >= 0 else -1, r['bytes'], r['ethertype'], r['stuffing'])
    for name, ts in CASES[half::2]:
        whole = None
        for at in range(len(ts)):                                      # 0: one call
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


@pytest.mark.parametrize('per_call', [1, 7])
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


@pytest.mark.parametrize('seed', [1, 2, 3])
def test_random_feeds_over_four_slots(pkg, seed):
    rng = np.random.default_rng(seed)
    ts = K.random_feed(rng, [0x1000, 0x1001, 0x1002], 300)
    # PID 0x1000 in two slots with different MAC filters
    pair = Pair(pkg, watches=[(0, 0x1000, K.MAC, K.MASK), (1, 0x1001, None, None), (2, 0x1000, bytes.fromhex('0200c0ffee01'), b'\xff' * 6), (3, 0x1002, K.GROUP, b'\xff' * 6)])
    a = 0
    while a < len(ts):
        n = int(rng.integers(1, 120))
        pair.call(ts[a:a + n], deliver=rng.random() < 0.8)
        a += n
    st = [pair.m.stats(k) for k in range(4)]
    assert all(s['sections'] > 50 and s['datagrams'] > 5 for s in st)
    assert st[0]['sections'] == st[2]['sections'] and st[0]['datagrams'] != st[2]['datagrams'] and st[0]['filtered'] > 0 and st[2]['filtered'] > 0
    tot = pair.m.stats()
    assert min(tot[k] for k in ('crc_errors', 'bad_ip', 'other_protocol', 'other_table', 'fragments', 'dropped_sections', 'scrambled_packets', 'unchecked')) > 0, tot


def test_capacity_failure_then_the_repeated_call(pkg):
    ts = K.whole_stream(CASES)
    head, rest = ts[:30], ts[30:]
    probe = Pair(pkg)
    probe.call(head)
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
    again = pkg.MpeBank.host(1, 4096, rows)                          # exactly enough rows
    again.set_watch(0, 0, PID, K.MAC, K.MASK)
    again.work(head), again.work(rest)
    assert again.row_table(0, 0) == probe.m.table(0)


def test_two_slots_on_one_pid_with_different_macs(pkg):
    a, b = bytes.fromhex('02aabbccdd01'), bytes.fromhex('02aabbccdd02')
    ts = R.Packetiser(PID).lay([R.section(K.dgram(100 + i, i), mac=(a, b, a, K.GROUP)[i % 4]) for i in range(12)])
    pair = Pair(pkg, watches=[(0, PID, a, b'\xff' * 6), (3, PID, b, b'\xff' * 6), (1, PID, None, None)])
    out = pair.call(ts[:4]), pair.call(ts[4:])
    st = [pair.m.stats(k) for k in range(4)]
    assert [(s['sections'], s['datagrams'], s['filtered']) for s in st] == [(12, 6, 6), (12, 12, 0), (0, 0, 0), (12, 3, 9)]
    assert sum(o[0].size for o in out) == sum(100 + i for i in range(0, 12, 2)) and sum(o[3].size for o in out) == 101 + 105 + 109


def test_a_watch_change_restarts_a_slot(pkg):
    ts = dict(CASES)['a 1400-byte datagram over 8 packets']
    pair = Pair(pkg)
    pair.call(ts[:4])
    assert pair.m.slot[0].buf and pair.hb.stats(0, 0)['packets'] == 4
    pair.hb.set_watch(0, 0, PID, K.MAC, K.MASK), pair.m.set_watch(0, PID, K.MAC, K.MASK)       # the same watch again: the open section is gone
    assert pair.hb.stats(0, 0)['packets'] == 0 and pair.hb.row_table(0, 0) == []
    pair.call(ts[4:])
    assert pair.m.table(0) == [] and pair.m.stats(0)['dropped_sections'] == 0 and pair.m.stats(0)['packets'] == 4
    pair.call(ts)
    assert pair.m.table(0)[0]['bytes'] == 1400
    pair.hb.reset()
    assert pair.hb.stats(0)['packets'] == 0


def test_watch_rules(pkg):
    hb = pkg.MpeBank.host(2, 64, 16)
    hb.set_watch(1, 0, 0x40, K.GROUP, b'\xff' * 6), hb.set_watch(1, 3, 0x40)      # the same PID in two slots is allowed
    for bad in ((1, 4, 0x40), (2, 0, 0x40), (0, 0, 0x1FFF), (0, 0, -2)):
        with pytest.raises(pkg.Dvbs2GpuError):
            hb.set_watch(*bad)
    with pytest.raises(ValueError):
        hb.set_watch(0, 0, 0x40, b'\x01\x02')
    ts = R.Packetiser(0x40).lay([R.section(K.dgram(40, 1))])
    assert hb.work(ts, stream=1, slot=0).size == 40 and hb.stats(1, 0)['datagrams_delivered'] == 1
    assert hb.stats(1, 3)['packets'] == 0                            # work() serves one slot
    with pytest.raises(pkg.Dvbs2GpuError):
        pkg.MpeBank.host(1, 4097, 16)


def test_follow_pmts(pkg):
    psi, mpe = pkg.PsiBank.host(1, 64, 16), pkg.MpeBank.host(1, 64, 16)
    psi.work(S.Packetiser(0).lay([S.pat(9, [(1, 0x100)])]))
    assert psi.follow_pat(0) == []
    psi.work(S.Packetiser(0x100).lay([S.pmt(1, 0x200, [(0x0D, 0x300), (0x1B, 0x200), (0x0A, 0x301)])]))
    assert mpe.follow_pmts(psi, 0) == [] and mpe._watched[0] == {0: 0x300, 1: 0x301}              # the video PID is not taken
    assert mpe.follow_pmts(psi, 0) == [] and mpe._watched[0] == {0: 0x300, 1: 0x301}              # and nothing twice
    ts = np.concatenate([R.Packetiser(0x301).lay([R.section(K.dgram(90, 3))]), R.Packetiser(0x300).lay([R.raw_section(0x3B, bytes(40), ssi=1)])])
    assert mpe.work(ts, slot=1).size == 90 and mpe.work(ts, slot=0).size == 0 and mpe.row_table(0, 0)[0]['flags'] == R.OTHER_TABLE
    full = pkg.MpeBank.host(1, 64, 16)
    for s in range(3):
        full.set_watch(0, s, 0x400 + s)
    assert full.follow_pmts(psi, 0) == [0x301] and full._watched[0][3] == 0x300
    only_a = pkg.MpeBank.host(1, 64, 16)
    assert only_a.follow_pmts(psi, 0, stream_types=(0x0A,)) == [] and only_a._watched[0] == {0: 0x301}
