"""PES bank without a GPU: the library's host bank (PesBank.host, csrc/pes_rules.h) against the model of tests/pes_ref.py in rows,
counters, stream counters and state (through the calls that follow) -- on the constructed cases with their literal rows, for cuts of
the stream into calls, on seeded random multiplexes over 16 slots, and at the row limit."""
import ctypes as C

import numpy as np
import pytest

import pes_cases as K
import pes_ref as P
import psi_ref as S

PID = K.PID


class Pair:
    """a host bank of one stream and the model, fed the same calls"""

    def __init__(self, pkg, max_packets=4096, max_rows=1024, watches=((0, PID),), tpp=K.TPP_Q24):
        self.hb, self.m = pkg.PesBank.host(1, max_packets, max_rows), P.Pes(max_rows)
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

    def cut(self, ts, per_call):
        """the stream in calls of per_call packets -> the concatenated rows, `packet` counted from the stream's start"""
        rows = []
        for a in range(0, len(ts), per_call):
            rows += [dict(r, packet=r['packet'] + a) for r in self.call(ts[a:a + per_call])]
        return rows


def test_timestamp_encoder_and_model_values(pkg):
    """0x123456789 = 100 | 10001101 0001010 | 11001111 0001001 in bits 32-30 | 29-15 | 14-0; behind prefix 0010 and with the marker bits
    that is 0010 100 1, 10001101, 0001010 1, 11001111, 0001001 1, written out by hand"""
    assert P.ts_bytes(2, 0x123456789) == bytes([0x29, 0x8D, 0x15, 0xCF, 0x13])
    assert P.ts_bytes(3, (1 << 33) - 1, (0, 0, 0)) == bytes([0x3E, 0xFF, 0xFE, 0xFF, 0xFE]) and P.ts_bytes(1, 0) == bytes([0x11, 0, 1, 0, 1])
    assert P.parse_start(P.pes_head(0xE0, 0x123456789, 0x1FFFFFFFF, 77) + b'x', 0) == (P.HEADER, 0xE0, 77, 0x123456789, 0x1FFFFFFFF)
    B = pkg.PesBank
    assert (B.SCRAMBLED, B.SHORT, B.BAD_START, B.PLAIN, B.MALFORMED, B.HEADER) == (P.SCRAMBLED, P.SHORT, P.BAD_START, P.PLAIN, P.MALFORMED, P.HEADER)
    assert (B.CLOSED, B.CLOSED_GAP, B.CLOSED_MISMATCH, B.CLOSED_UNCHECKED, B.UNBOUNDED_NONVIDEO) == (1, 2, 4, 8, 16) == (P.CLOSED, P.CLOSED_GAP, P.CLOSED_MISMATCH,
                                                                                                                        P.CLOSED_UNCHECKED, P.UNBOUNDED_NONVIDEO)
    assert (B.TS_FIRST, B.TS_BACKWARD, B.TS_GAP, B.PTS_LATE, B.DTS_AFTER_PTS) == (32, 64, 128, 256, 512) == (P.TS_FIRST, P.TS_BACKWARD, P.TS_GAP, P.PTS_LATE, P.DTS_AFTER_PTS)
    assert B.NO_TS == P.NO_TS and P.late_packets(K.TPP_Q24) == K.LATE and P.late_packets(1000 << 24) == 18900
    assert C.sizeof(pkg.PesRow) == 48 and [getattr(pkg.PesRow, k).offset for k in ('flags', 'stream_id', 'packet', 'declared', 'pts', 'dts', 'closed_bytes',
                                                                                   'delta_packets', 'delta_ts')] == [4, 6, 8, 12, 16, 24, 32, 40, 44]


def test_constructed_cases_one_by_one(pkg):
    pair = Pair(pkg)
    for j, (name, ts, want) in enumerate(K.edge_cases()):
        rows = pair.call(ts)
        assert [(r['kind'], r['flags'], r['closed_bytes']) for r in rows][1:] == want, name
        if j == 0:
            assert (rows[0]['kind'], rows[0]['flags'], rows[0]['closed_bytes'], rows[0]['delta_ts']) == (P.HEADER, P.TS_FIRST, 0, 0)
            assert [(r['stream_id'], r['declared']) for r in rows[1:4]] == [(0, 0), (0xE0, 0), (0xE0, 0)] and rows[9]['dts'] == rows[9]['pts'] - 1800
        if name.startswith('dT 2^32'):
            assert [(r['delta_ts'], r['delta_packets']) for r in rows[1:]] == [((1 << 31) - 1, 1), (-(1 << 31), 1)]
        if name.startswith('dT 63000'):
            assert [r['delta_ts'] for r in rows] == [K.STEP, 63000, 63001]
        if name.startswith('PTS wrap'):
            assert (rows[0]['pts'], rows[1]['pts'], rows[1]['delta_ts']) == ((1 << 33) - 1000, 2600, K.STEP)
        if name.startswith('dN'):
            assert [r['delta_packets'] for r in rows[1:]] == [210, 211] and [r['packet'] for r in rows] == [0, 210, 421]
        if name.startswith('a duplicate'):
            assert [r['closed_packets'] for r in rows] == [1, 1, 3]
    st = pair.m.stats()
    assert min(st.values()) > 0, st                               # every counter has been reached
    assert (st['duplicates'], st['cc_errors'], st['malformed_packets'], st['scrambled_packets'], st['starts_plain'], st['starts_scrambled']) == (3, 2, 1, 2, 8, 1)
    assert (st['closed_mismatch'], st['closed_gap'], st['ts_backward'], st['ts_gap'], st['pts_late'], st['dts_after_pts'], st['max_delta_packets']) == (2, 4, 1, 3, 1, 1, 211)
    assert pair.hb.stream_stats()['packets_since_start'][0] == 1


@pytest.mark.parametrize('per_call', [1, 7, 100])
def test_cut_independence_of_the_constructed_stream(pkg, per_call):
    ts = K.whole_stream()
    whole, cut = Pair(pkg), Pair(pkg)
    want = whole.cut(ts, len(ts))
    assert cut.cut(ts, per_call) == want and len(want) == whole.m.stats()['starts'] == 85
    assert cut.m.stats() == whole.m.stats() and cut.hb.stats() == whole.hb.stats() and cut.hb.stream_stats() == whole.hb.stream_stats()


@pytest.mark.parametrize('seed', [1, 2, 3])
def test_random_multiplexes_over_16_slots(pkg, seed):
    rng = np.random.default_rng(seed)
    pids = [0x100 + 7 * s for s in range(16)]
    ts = P.random_mux(rng, 1500, pids, tpp=K.TPP)
    watches = tuple((int(s), pids[s]) for s in rng.permutation(16))
    whole, cut = Pair(pkg, watches=watches), Pair(pkg, watches=watches)
    want = whole.cut(ts, len(ts))
    edges = [0] + sorted(set(rng.integers(0, 1501, 12).tolist())) + [1500]
    rows = []
    for a, b in zip(edges[:-1], edges[1:]):
        rows += [dict(r, packet=r['packet'] + a) for r in cut.call(ts[a:b])]
    assert rows == want
    st = whole.m.stats()
    assert cut.m.stats() == st and cut.hb.stats() == whole.hb.stats()
    assert min(st[k] for k in ('duplicates', 'cc_errors', 'scrambled_packets', 'malformed_packets', 'starts_short', 'starts_malformed', 'starts_plain', 'with_dts',
                               'closed_ok', 'closed_gap', 'closed_unchecked', 'dts_after_pts')) > 0, st
    assert all(whole.m.stats(s)['starts'] > 0 for s in range(16))


def test_rows_limit_rewatching_and_reset(pkg):
    ln = K.Line()
    for _ in range(10):
        ln.start(declared=178)
    ts = ln.take()
    small = Pair(pkg, max_rows=3)
    assert len(small.call(ts)) == 3 and small.hb.work(ts[:0]) == 0
    assert small.hb.stream_stats()['rows_dropped'] == 7 and small.hb.stats()['closed_ok'] == 9 and small.hb.row_table() == []
    blind = Pair(pkg, watches=())
    assert blind.call(ts) == [] and blind.hb.stats()['packets'] == 0 and blind.hb.stream_stats()['packets'] == 10
    blind.set_watch(5, PID)
    rows = blind.call(ts)
    assert (rows[0]['flags'], rows[1]['flags'], rows[1]['delta_packets']) == (P.TS_FIRST, P.CLOSED, 1) and rows[0]['slot'] == 5
    blind.set_watch(5, PID)                                        # re-watching: state and counters start afresh, the position goes on
    rows = blind.call(ts[:2])
    assert rows[0]['flags'] == P.TS_FIRST and blind.hb.stats(0, 5)['starts'] == 2 and blind.hb.stream_stats()['packets'] == 22
    unset = Pair(pkg, tpp=0)
    late = K.edge_cases()[-2][1]
    assert [r['flags'] & P.PTS_LATE for r in unset.call(late)] == [0, 0, 0] and unset.hb.stats()['max_delta_packets'] == 211
    blind.hb.reset(), blind.m.reset()
    assert blind.hb.stream_stats()['packets'] == 0 and blind.hb.stats()['starts'] == 0
    assert [r['flags'] & P.PTS_LATE for r in blind.call(late)] == [0, 0, P.PTS_LATE] and blind.m.table[0]['slot'] == 5          # watch and rate stayed


def test_follow_pmts(pkg):
    psi, pes = pkg.PsiBank.host(1, 64, 16), pkg.PesBank.host(1, 64, 16)
    pmts = [(1, 0x100, [(0x1b, 0x200), (0x0f, 0x201), (0x05, 0x202)]), (2, 0x101, [(0x02, 0x210), (0x86, 0x211), (0x06, 0x201)])]
    psi.work(S.Packetiser(0).lay([S.pat(9, [(n, p) for n, p, _ in pmts])]))
    assert psi.follow_pat(0) == []
    psi.work(np.concatenate([S.Packetiser(p).lay([S.pmt(n, es[0][1], es)]) for n, p, es in pmts]))
    pes.set_watch(0, 0, 0x210)
    assert pes.follow_pmts(psi, 0) == [] and pes._watched[0] == {0: 0x210, 1: 0x200, 2: 0x201}       # sections and SCTE 35 skipped, 0x201 once
    every = pkg.PesBank.host(1, 64, 16)
    assert every.follow_pmts(psi, 0, skip_types=()) == [] and list(every._watched[0].values()) == [0x200, 0x201, 0x202, 0x210, 0x211]
    full = pkg.PesBank.host(1, 64, 16)
    for s in range(14):
        full.set_watch(0, s, 0x400 + s)
    assert full.follow_pmts(psi, 0) == [0x210] and full._watched[0][14] == 0x200 and full._watched[0][15] == 0x201
    ln = K.Line(0x201)
    assert full.work(ln.start().start().take()) == 2 and full.stats(0, 15)['starts_header'] == 2


def test_argument_checks(pkg):
    lib, h, ARG = pkg.load_library(), C.c_void_p(), -1
    assert lib.dvbs2gpu_pes_create(None, 1, 16, 16, C.byref(h)) == ARG
    assert lib.dvbs2gpu_pes_create_host(0, 16, 16, C.byref(h)) == ARG and lib.dvbs2gpu_pes_create_host(1, 4097, 16, C.byref(h)) == ARG
    assert b'PES bank: max_packets' in lib.dvbs2gpu_last_error()
    assert lib.dvbs2gpu_pes_create_host(1, 16, 0, C.byref(h)) == ARG and lib.dvbs2gpu_pes_create_host(1, 16, 16, None) == ARG
    assert lib.dvbs2gpu_pes_reset(None) == ARG
    lib.dvbs2gpu_pes_destroy(None)
    assert lib.dvbs2gpu_pes_create_host(2, 16, 16, C.byref(h)) == 0
    assert lib.dvbs2gpu_pes_set_watch(h, 2, 0, 5) == ARG and lib.dvbs2gpu_pes_set_watch(h, 0, 16, 5) == ARG
    assert lib.dvbs2gpu_pes_set_watch(h, 0, 1, 0x1FFF) == ARG and lib.dvbs2gpu_pes_set_watch(h, 0, 1, -2) == ARG
    assert lib.dvbs2gpu_pes_set_watch(h, 0, 1, 5) == 0 and lib.dvbs2gpu_pes_set_watch(h, 0, 2, 5) == ARG and lib.dvbs2gpu_pes_set_watch(h, 1, 2, 5) == 0
    assert b'another slot' in lib.dvbs2gpu_last_error()
    assert lib.dvbs2gpu_pes_set_watch(h, 0, 1, 5) == 0                                  # the same slot again is no clash
    assert lib.dvbs2gpu_pes_set_rate(h, 0, 1 << 48) == ARG and lib.dvbs2gpu_pes_set_rate(h, 2, 0) == ARG and lib.dvbs2gpu_pes_set_rate(h, 0, (1 << 48) - 1) == 0
    buf = np.zeros(17 * 188, np.uint8)
    pb = C.c_void_p(buf.ctypes.data)
    assert lib.dvbs2gpu_pes_work(h, 0, pb, 187) == ARG
    assert lib.dvbs2gpu_last_error() == b'PES bank: a byte count is a whole number of 188-byte packets'
    assert lib.dvbs2gpu_pes_work(h, 0, pb, 17 * 188) == ARG
    assert lib.dvbs2gpu_last_error() == b'PES bank: packet count exceeds max_packets'
    assert lib.dvbs2gpu_pes_work(h, 0, None, 188) == ARG and lib.dvbs2gpu_pes_work(h, 0, pb, 16 * 188) == 0
    pp = (C.c_void_p * 2)(buf.ctypes.data, buf.ctypes.data)
    assert lib.dvbs2gpu_pes_process_batch(h, pp, (C.c_int * 2)(0, 0), None, None) == ARG   # a host bank has no device buffers
    st, ss, n, p = pkg.PesStats(), pkg.PesStreamStats(), C.c_int(), C.c_void_p()
    assert lib.dvbs2gpu_pes_get_stats(h, 0, 16, C.byref(st)) == ARG and lib.dvbs2gpu_pes_get_stats(h, 0, -1, None) == ARG
    assert lib.dvbs2gpu_pes_get_stream_stats(h, 2, C.byref(ss)) == ARG
    assert lib.dvbs2gpu_pes_get_row_table(h, 0, None, 1, C.byref(n)) == ARG
    assert lib.dvbs2gpu_pes_get_row_table_device(h, 0, C.byref(p), C.byref(n)) == ARG
    lib.dvbs2gpu_pes_destroy(h)
