"""IP-TS bank without a GPU: the library's host bank (IpTsBank.host, csrc/ipts_rules.h) through the C ABI against the model of
tests/ipts_ref.py in bytes, rows, counters, needed sizes and state through the next call -- on the constructed cases with their rows
written out, on seeded random tables, each whole and cut into calls of 1 and 7 rows, at the capacity limit, across set_flow and reset,
and with wrong arguments."""
import ctypes as C

import numpy as np
import pytest

import ipts_cases as K
import ipts_ref as R

CASES, GRE_CASES = K.cases(), K.gre_cases()


class Pair:
    """a host bank of one stream and the model, with the same flows, fed the same calls"""

    def __init__(self, pkg, max_rows=1024, flows=True):
        self.hb, self.m = pkg.IpTsBank.host(1, max_rows), R.Stream()
        if flows:
            K.set_flows(self.hb, 0), K.set_flows(self.m)

    def call(self, data, table, kind=R.RAW_IP, deliver=True):
        want = self.m.process(data, table, kind, deliver)
        got = self.hb.work(data, table, kind, deliver=deliver)
        assert (got is None) == (want is None)
        for slot in range(R.SLOTS):
            assert got is None or np.array_equal(got[slot], want[slot]), slot
            assert self.hb.stats(0, slot) == self.m.stats(slot), slot
            assert self.hb.needed(0, slot) == (want[slot].size if deliver else 0), slot
        assert self.hb.row_table(0) == self.m.table
        assert self.hb.stats(0) == self.m.stats()
        return want


def brief(table):
    return [(r['flags'], r['slot'], r['packets'], r['lost']) for r in table]


def test_layout_and_the_checksum_of_the_model(pkg):
    assert pkg.IpTsBank.layout() == R.LAYOUT
    assert C.sizeof(pkg.IptsRow) == R.LAYOUT['row_bytes'] and C.sizeof(pkg.IptsView) == R.LAYOUT['view_bytes']
    # the IPv4 header of the MPE tests with its published checksum; the two forms of the sum on random bytes of odd and even length
    hdr = bytes.fromhex('450000730000400040110000c0a80001c0a800c7')
    assert R.ones_sum(hdr) ^ 0xFFFF == 0xB861
    rng = np.random.default_rng(1)
    for n in (0, 1, 2, 3, 1315, 1316):
        b = bytes(rng.integers(0, 256, n, dtype=np.uint8))
        s = R.word_sum(b)
        while s >> 16:
            s = (s & 0xFFFF) + (s >> 16)
        assert s == R.ones_sum(b), n
    assert R.ones_sum(b'\xff\xff\xff\xff') == 0xFFFF and R.ones_sum(bytes(4)) == 0


@pytest.mark.parametrize('cases,kind', [(CASES, R.RAW_IP), (GRE_CASES, R.GRE)], ids=['raw_ip', 'gre'])
def test_constructed_cases_give_their_written_rows(pkg, cases, kind):
    pair = Pair(pkg)
    data, table = K.table_of(cases)
    out = pair.call(data, table, kind)
    for (name, *_), got, want in zip(cases, brief(pair.m.table), K.expected_rows(cases)):
        assert got == want, name
    assert pair.m.stats() == K.expected_stats(cases)
    assert [o.size for o in out] == [188 * sum(p for _, _, _, s, p, _ in cases if s == k) for k in range(4)]
    assert pair.m.stats(2)['matched'] == 0                            # slot 2 names slot 0's flow: the lowest wins
    if kind == R.RAW_IP:
        seen = 0
        for _, _, f, *_ in cases:
            seen |= K.flags(f)
        assert seen == (1 << 17) - 1                                   # every flag has a case


@pytest.mark.parametrize('per_call', [1, 7])
@pytest.mark.parametrize('cases,kind', [(CASES, R.RAW_IP), (GRE_CASES, R.GRE)], ids=['raw_ip', 'gre'])
def test_constructed_cases_cut_into_calls(pkg, cases, kind, per_call):
    data, table = K.table_of(cases, shift=3, gap=4)
    whole, cut = Pair(pkg), Pair(pkg)
    want = whole.call(data, table, kind)
    got, rows = [[] for _ in range(4)], []
    for part in K.calls_of(table, per_call):
        out = cut.call(data, part, kind)
        base = [sum(o.size for o in g) for g in got]
        rows += [dict(r, offset=r['offset'] + base[r['slot']] if r['offset'] >= 0 else -1) for r in cut.m.table]
        for k in range(4):
            got[k].append(out[k])
    assert all(np.array_equal(np.concatenate(got[k]), want[k]) for k in range(4))
    assert rows == whole.m.table and cut.m.stats() == whole.m.stats() == K.expected_stats(cases)
    carried = Pair(pkg)                                              # rows only: the same rows but for offsets, no bytes
    assert carried.call(data, table, kind, deliver=False) is None
    assert [dict(r, offset=-1) for r in whole.m.table] == carried.m.table and carried.m.stats() == K.expected_stats(cases, delivered=False)


@pytest.mark.parametrize('per_call', [0, 1, 7])
@pytest.mark.parametrize('seed,kind', [(1, R.RAW_IP), (2, R.RAW_IP), (3, R.GRE)])
def test_random_tables(pkg, seed, kind, per_call):
    data, table = K.random_table(seed, 700, kind)
    pair = Pair(pkg)
    rng = np.random.default_rng(seed)
    for part in K.calls_of(table, per_call):
        pair.call(data, part, kind, deliver=per_call == 0 or rng.random() < 0.8)
    st = pair.m.stats()
    assert min(st.values()) > 0, st                                  # on the model alone: the table has met every rule
    assert all(pair.m.stats(k)['ts'] > 20 for k in (0, 1, 3)) and pair.m.stats(2)['matched'] == 0


def test_capacity_failure_then_the_repeated_call(pkg):
    data, table = K.table_of(CASES)
    head, rest = table[:30], table[30:]
    probe = Pair(pkg)
    probe.call(data, head)
    need = probe.m.sizes(data, rest)
    pair = Pair(pkg)
    pair.call(data, head)
    before = [pair.hb.stats(0, k) for k in (-1, 0, 1, 2, 3)]
    with pytest.raises(pkg.Dvbs2GpuError) as e:
        pair.hb.work(data, rest, cap=max(need) - 1)
    assert e.value.code == -5 and e.value.needed == need == [pair.hb.needed(0, k) for k in range(4)]
    assert [pair.hb.stats(0, k) for k in (-1, 0, 1, 2, 3)] == before and pair.hb.row_table(0) == []
    pair.call(data, rest)                                            # the repeat, with room, equals the model: LATE and LOSS rows as if nothing had been
    assert pair.m.stats(3)['late'] > 0 and pair.m.stats(3)['loss_events'] > 0
    exact = pkg.IpTsBank.host(1, len(rest))                          # exactly enough room and rows
    K.set_flows(exact, 0)
    exact.work(data, head[:len(rest)]), exact.work(data, rest, cap=max(need))
    with pytest.raises(pkg.Dvbs2GpuError) as e:                      # one row too many is an argument error
        exact.work(data, table[:len(rest) + 1])
    assert e.value.code == -1


def test_set_flow_and_reset(pkg):
    s3 = [c for c in CASES if c[3] == 3]
    data, table = K.table_of(s3)
    pair = Pair(pkg)
    pair.call(data, table[:4])
    assert pair.m.stats(3)['loss_events'] == 1 and pair.m.stats()['rows'] == 4
    fam, addr, port = K.FLOWS[3]
    pair.hb.set_flow(0, 3, fam, addr, port), pair.m.set_flow(3, fam, addr, port)     # the same flow again: the slot's counters and RTP state are gone,
    assert pair.hb.stats(0, 3) == dict.fromkeys(R.STAT_KEYS, 0) and pair.hb.stats(0)['rows'] == 4     # the stream's own counters stay
    pair.call(data, table[4:5])                                      # sequence 1 behind 2: late no more, nothing is stored
    assert brief(pair.m.table) == [(R.RTP | R.TS_ROW, 3, 2, 0)]
    pair.call(data, table[4:5])                                      # and now it is
    assert brief(pair.m.table) == [(R.RTP | R.LATE, 3, 0, 0)]
    pair.hb.reset(), pair.m.reset()
    assert pair.hb.stats(0) == dict.fromkeys(R.STAT_KEYS, 0) and pair.hb.row_table(0) == []
    pair.call(data, table[4:5])                                      # the flows have stayed, the state has not
    assert brief(pair.m.table) == [(R.RTP | R.TS_ROW, 3, 2, 0)]
    pair.hb.set_flow(0, 3, 0), pair.m.set_flow(3, 0)                 # the slot emptied
    pair.call(data, table[5:7])
    assert [r['flags'] for r in pair.m.table] == [R.UNWATCHED] * 2
    none = Pair(pkg, flows=False)                                    # a bank with no flow watches nothing
    none.call(*K.table_of(CASES))
    assert none.m.stats()['unwatched'] > 20 and none.m.stats()['matched'] == 0


def test_two_streams_are_apart(pkg):
    hb, m = pkg.IpTsBank.host(2, 64), [R.Stream(), R.Stream()]
    K.set_flows(hb, 1), K.set_flows(m[1])
    s3 = [c for c in CASES if c[3] == 3]
    data, table = K.table_of(s3)
    for a in (0, 3):
        want = m[1].process(data, table[a:a + 3])
        got = hb.work(data, table[a:a + 3], stream=1)
        assert all(np.array_equal(g, w) for g, w in zip(got, want)) and hb.row_table(1) == m[1].table and hb.row_table(0) == []
    m[0].process(data, table[:3])
    hb.work(data, table[:3], stream=0)                               # stream 0 has no flow; stream 1 received an empty call
    assert hb.row_table(0) == m[0].table and hb.row_table(1) == [] and hb.stats(0) == m[0].stats() and hb.stats(1) == m[1].stats()


def test_argument_errors(pkg):
    hb = pkg.IpTsBank.host(2, 16)
    for bad in ((2, 0, 4, R.V4_DST, 1), (0, 4, 4, R.V4_DST, 1), (0, -1, 4, R.V4_DST, 1), (0, 0, 5, R.V6_DST, 1), (0, 0, 4, R.V4_DST, 65536), (0, 0, 4, R.V4_DST, -1)):
        with pytest.raises(pkg.Dvbs2GpuError):
            hb.set_flow(*bad)
    with pytest.raises(ValueError):
        hb.set_flow(0, 0, 6, R.V4_DST, 1)
    for create in ((0, 16), (1, 0), (1, 16385)):
        with pytest.raises(pkg.Dvbs2GpuError):
            pkg.IpTsBank.host(*create)
    data, table = K.table_of(CASES[:4])
    with pytest.raises(pkg.Dvbs2GpuError):
        hb.work(data, table, stream=2)
    with pytest.raises(pkg.Dvbs2GpuError):
        hb.work(data, table, kind=2)
    lib, V = hb.lib, pkg.IptsView
    tab = np.ascontiguousarray(table)
    p, q = C.c_void_p(data.ctypes.data), tab.ctypes.data
    ok = dict(bytes=p, rows=C.c_void_p(q), stride=8, offset_at=0, bytes_at=4, kind=0, n=len(tab), reserved=0)
    assert lib.dvbs2gpu_ipts_work(hb.h, 0, C.byref(V(**ok)), None, 0, None) == 0
    for change in (dict(stride=6), dict(stride=4), dict(offset_at=2), dict(bytes_at=8), dict(offset_at=-4), dict(rows=C.c_void_p(q + 2)), dict(rows=None),
                   dict(bytes=None), dict(n=-1), dict(n=17)):
        assert lib.dvbs2gpu_ipts_work(hb.h, 0, C.byref(V(**dict(ok, **change))), None, 0, None) == -1, change
    assert lib.dvbs2gpu_ipts_work(hb.h, 0, None, None, 0, None) == -1 and lib.dvbs2gpu_ipts_work(hb.h, 0, C.byref(V(**ok)), None, -1, None) == -1
    assert lib.dvbs2gpu_ipts_process_batch(hb.h, C.byref(V(**ok)), None, 0, None, None, None) == -1        # a host bank takes host buffers
    K.set_flows(hb, 0)
    outs = (C.c_void_p * 4)()                                        # a slot with a flow needs its buffer
    assert lib.dvbs2gpu_ipts_work(hb.h, 0, C.byref(V(**ok)), outs, 100, None) == -1
    n = C.c_int()
    assert lib.dvbs2gpu_ipts_get_needed(hb.h, 0, 4, C.byref(n)) == -1 and lib.dvbs2gpu_ipts_get_stats(hb.h, 0, 4, C.byref(pkg.IptsStats())) == -1
    assert lib.dvbs2gpu_ipts_get_row_table_device(hb.h, 0, C.byref(C.c_void_p()), C.byref(n)) == -1        # device banks only
    assert lib.dvbs2gpu_ipts_get_layout(None) == -1
