"""PCR bank without a GPU: the library's host bank (PcrBank.host, csrc/pcr_rules.h) against the model of tests/pcr_ref.py in rows,
counters, stream counters and rate -- on the literal anchors, the constructed edges, for every cut of a stream into calls, and at the
row limit."""
import numpy as np
import pytest

import pcr_cases as K
import pcr_ref as P
import psi_ref as S

PID = K.PID


class Pair:
    """a host bank of one stream and the model, fed the same calls"""

    def __init__(self, pkg, max_packets=4096, max_rows=1024, watches=((0, PID),), tpp=K.TPP_Q24):
        self.hb, self.m = pkg.PcrBank.host(1, max_packets, max_rows), P.Clock(max_rows)
        for slot, pid in watches:
            self.set_watch(slot, pid)
        if tpp:
            self.hb.set_rate(0, tpp), self.m.set_rate(tpp)

    def set_watch(self, slot, pid):
        self.hb.set_watch(0, slot, pid), self.m.set_watch(slot, pid)

    def call(self, ts):
        assert self.hb.work(ts) == self.m.process(ts)
        K.same(self.hb, self.m)
        return self.m.table


def _tuples(rows):
    return [(r['kind'], r['flags'], r['delta_ticks'], r['delta_packets'], r['accuracy']) for r in rows]


@pytest.mark.parametrize('name,values,want', K.ANCHORS, ids=[a[0] for a in K.ANCHORS])
def test_literal_anchors(pkg, name, values, want):
    rows = Pair(pkg).call(K.spaced(values))
    assert _tuples(rows) == [(P.FIRST, 0, 0, 0, 0)] + want
    assert [r['packet'] for r in rows] == [K.GAP * j for j in range(len(values))] and [r['pcr'] for r in rows] == values


def test_model_values(pkg):
    assert P.MOD == 2576980377600 and (pkg.PcrBank.OK, pkg.PcrBank.LATE, pkg.PcrBank.JUMP) == (P.OK, P.LATE, P.JUMP)
    p = P.pcr_packet(0x1ABC, 123456789012)
    assert int(p[6]) << 25 | int(p[7]) << 17 | int(p[8]) << 9 | int(p[9]) << 1 | int(p[10]) >> 7 == 123456789012 // 300
    assert (int(p[10]) & 1) << 8 | int(p[11]) == 123456789012 % 300 and p[4] == 7 and p[5] == 0x10


def test_constructed_edges_one_by_one(pkg):
    pair = Pair(pkg)
    for name, ts in K.edge_cases():
        before, unw = pair.m.stats(0), pair.m.unwatched
        rows = pair.call(ts)
        d = {k: pair.m.stats(0)[k] - before[k] for k in ('pcr_packets', 'malformed')}
        if name in K.MIDDLE:
            counter, records = K.MIDDLE[name]
            assert d == dict(pcr_packets=records, malformed=int(counter == 'malformed')), name
            assert [r['packet'] for r in rows] == ([0, 30, 60] if records == 3 else [0, 60]), name
        if name == 'DI with an equal value':
            assert rows[1]['kind'] == P.ANNOUNCED and rows[1]['pcr'] == rows[0]['pcr']
        if name.startswith('scrambled'):
            assert pair.m.unwatched - unw == 1 and pair.hb.stream_stats()['first_unwatched_pid'] == K.OTHER
    st = pair.m.stats()
    assert st['malformed'] == 4 and st['repeated'] == 2 and st['announced'] == 1 and st['first'] == 1 and st['accuracy_errors'] > 3


def test_cut_independence(pkg):
    rng = np.random.default_rng(17)
    pids = [PID, 0x130, 0x131]
    ts = P.stamped_mux(rng, 300, pids, tpp=K.TPP, jitter=20)
    recs = [k for k in range(300) if ts[k, 3] & 0x20]
    ts[recs[5], 6:12] = ts[recs[2], 6:12]                          # (values of another PID's packet: a jump, or by chance nothing)
    for a in recs[8:28:4]:                                         # equal runs: a duplicate of a PCR packet right behind it
        if not ts[a + 1, 3] & 0x20:
            ts[a + 1] = ts[a]
    ts[recs[12], 5] |= 0x80                                        # (its duplicate announces nothing: REPEATED behind ANNOUNCED)
    watches = tuple(enumerate(pids))
    whole = Pair(pkg, watches=watches)
    want = [dict(r) for r in whole.call(ts)]
    assert whole.m.stats()['repeated'] >= 3 and whole.m.stats()['announced'] >= 1 and whole.m.stats()['ok'] > 15
    cuts = [[c] for c in recs[8:14]] + [sorted(set(rng.integers(0, 301, int(rng.integers(1, 8))).tolist())) for _ in range(20)]
    for cut in cuts:
        pair, rows = Pair(pkg, watches=watches), []
        edges = [0] + cut + [300]
        for a, b in zip(edges[:-1], edges[1:]):
            rows += [dict(r, packet=r['packet'] + a) for r in pair.call(ts[a:b])]
        assert rows == want, cut
        assert pair.m.stats() == whole.m.stats() and pair.hb.stats() == whole.hb.stats(), cut
        assert pair.hb.stream_stats()['packets_since_pcr'] == whole.hb.stream_stats()['packets_since_pcr'], cut


def test_dn_32767_and_32768_through_calls_of_null_packets(pkg):
    calls, want = K.saturation_calls()
    pair = Pair(pkg, tpp=80 << 24)
    rows = [r for c in calls for r in pair.call(c)]
    assert rows[1:] == want
    st = pair.hb.stats()
    assert (st['sum_packets'], st['sum_ticks'], st['accuracy_measured'], st['accuracy_errors'], st['max_abs_accuracy']) == (32767, 32767 * 80, 2, 1, 80 << 6)
    assert pair.hb.stream_stats()['packets'] == 65536 and pair.hb.stream_stats()['packets_since_pcr'][0] == 1


def test_rows_limit_rate_unset_unwatched_and_rewatching(pkg):
    ts = K.spaced([30000 * j for j in range(10)])
    small = Pair(pkg, max_rows=3)
    assert len(small.call(ts)) == 3 and small.hb.work(ts[:0]) == 0
    assert small.hb.stream_stats()['rows_dropped'] == 7 and small.hb.stats()['ok'] == 9 and small.hb.row_table() == []
    unset = Pair(pkg, tpp=0)
    rows = unset.call(K.spaced([0, 30014, 60000]))
    assert _tuples(rows)[1:] == [(P.OK, 0, 30014, 30, 0), (P.OK, 0, 29986, 30, 0)] and unset.hb.stats()['accuracy_measured'] == 0
    assert unset.hb.rate() == 1504 * 27e6 * 60 / 60000 == 40.608e6
    blind = Pair(pkg, watches=())
    assert blind.call(ts) == [] and blind.hb.stream_stats()['unwatched_pcr_packets'] == 10 and blind.hb.stream_stats()['first_unwatched_pid'] == PID
    blind.set_watch(5, PID)
    assert _tuples(blind.call(K.spaced([300000, 330000])))[0] == (P.FIRST, 0, 0, 0, 0) and blind.hb.stream_stats()['first_unwatched_pid'] == -1
    blind.set_watch(5, PID)                                        # re-watching: state and counters start afresh, the position goes on
    assert _tuples(blind.call(K.spaced([360000])))[0] == (P.FIRST, 0, 0, 0, 0) and blind.hb.stats(0, 5)['first'] == 1
    assert blind.hb.stream_stats()['packets'] == 390
    blind.hb.reset(), blind.m.reset()
    assert blind.hb.stream_stats()['packets'] == 0 and _tuples(blind.call(K.spaced([0, 30014])))[1] == (P.OK, K.A, 30014, 30, 896)   # watch and rate stayed


def test_follow_pmts(pkg):
    psi, pcr = pkg.PsiBank.host(1, 64, 16), pkg.PcrBank.host(1, 64, 16)
    pmts = [(1, 0x100, 0x200), (2, 0x101, 0x210), (3, 0x102, 0x1FFF), (4, 0x103, 0x200)]      # programme 3 has no PCR, 4 shares programme 1's
    psi.work(S.Packetiser(0).lay([S.pat(9, [(n, p) for n, p, _ in pmts])]))
    assert psi.follow_pat(0) == []
    psi.work(np.concatenate([S.Packetiser(p).lay([S.pmt(n, c, [(0x1b, c)])]) for n, p, c in pmts]))
    pcr.set_watch(0, 0, 0x210)
    assert pcr.follow_pmts(psi, 0) == [] and pcr._watched[0] == {0: 0x210, 1: 0x200}
    full = pkg.PcrBank.host(1, 64, 16)
    for s in range(15):
        full.set_watch(0, s, 0x400 + s)
    assert full.follow_pmts(psi, 0) == [0x210] and full._watched[0][15] == 0x200
    assert full.work(K.spaced([0, 30000], pid=0x200)) == 2 and full.stats(0, 15)['ok'] == 1


def test_argument_checks(pkg):
    import ctypes as C
    lib, h, ARG = pkg.load_library(), C.c_void_p(), -1
    assert lib.dvbs2gpu_pcr_create(None, 1, 16, 16, C.byref(h)) == ARG
    assert lib.dvbs2gpu_pcr_create_host(0, 16, 16, C.byref(h)) == ARG and lib.dvbs2gpu_pcr_create_host(1, 4097, 16, C.byref(h)) == ARG
    assert lib.dvbs2gpu_pcr_create_host(1, 16, 0, C.byref(h)) == ARG and lib.dvbs2gpu_pcr_create_host(1, 16, 16, None) == ARG
    assert lib.dvbs2gpu_pcr_reset(None) == ARG
    lib.dvbs2gpu_pcr_destroy(None)
    assert lib.dvbs2gpu_pcr_create_host(2, 16, 16, C.byref(h)) == 0
    assert lib.dvbs2gpu_pcr_set_watch(h, 2, 0, 5) == ARG and lib.dvbs2gpu_pcr_set_watch(h, 0, 16, 5) == ARG
    assert lib.dvbs2gpu_pcr_set_watch(h, 0, 1, 0x1FFF) == ARG and lib.dvbs2gpu_pcr_set_watch(h, 0, 1, -2) == ARG
    assert lib.dvbs2gpu_pcr_set_watch(h, 0, 1, 5) == 0 and lib.dvbs2gpu_pcr_set_watch(h, 0, 2, 5) == ARG and lib.dvbs2gpu_pcr_set_watch(h, 1, 2, 5) == 0
    assert lib.dvbs2gpu_pcr_set_watch(h, 0, 1, 5) == 0                                  # the same slot again is no clash
    assert lib.dvbs2gpu_pcr_set_rate(h, 0, 1 << 48, 864) == ARG and lib.dvbs2gpu_pcr_set_rate(h, 0, 1000 << 24, -1) == ARG
    assert lib.dvbs2gpu_pcr_set_rate(h, 2, 0, 864) == ARG and lib.dvbs2gpu_pcr_set_rate(h, 0, (1 << 48) - 1, 0) == 0
    buf = np.zeros(17 * 188, np.uint8)
    pb = C.c_void_p(buf.ctypes.data)
    assert lib.dvbs2gpu_pcr_work(h, 0, pb, 187) == ARG and lib.dvbs2gpu_pcr_work(h, 0, pb, 17 * 188) == ARG and lib.dvbs2gpu_pcr_work(h, 0, None, 188) == ARG
    assert b'PCR bank: ' in lib.dvbs2gpu_last_error()
    pp = (C.c_void_p * 2)(buf.ctypes.data, buf.ctypes.data)
    assert lib.dvbs2gpu_pcr_process_batch(h, pp, (C.c_int * 2)(0, 0), None, None) == ARG   # a host bank has no device buffers
    st, ss, n, p, v = pkg.PcrStats(), pkg.PcrStreamStats(), C.c_int(), C.c_void_p(), C.c_double()
    assert lib.dvbs2gpu_pcr_get_stats(h, 0, 16, C.byref(st)) == ARG and lib.dvbs2gpu_pcr_get_stats(h, 0, -1, None) == ARG
    assert lib.dvbs2gpu_pcr_get_stream_stats(h, 2, C.byref(ss)) == ARG and lib.dvbs2gpu_pcr_get_rate(h, 0, 0, None) == ARG
    assert lib.dvbs2gpu_pcr_get_row_table(h, 0, None, 1, C.byref(n)) == ARG
    assert lib.dvbs2gpu_pcr_get_row_table_device(h, 0, C.byref(p), C.byref(n)) == ARG
    assert lib.dvbs2gpu_pcr_get_rate(h, 0, -1, C.byref(v)) == 0 and v.value == 0.0
    assert C.sizeof(pkg.PcrRow) == 32 and pkg.PcrRow.pcr.offset == 12
    lib.dvbs2gpu_pcr_destroy(h)
