"""PSI section bank without a GPU: the library's host bank (PsiBank.host, csrc/psi_rules.h) against the model of tests/psi_ref.py in
bytes, rows, counters and decoded views -- on the constructed edges, for every cutting of a stream into calls, and at the capacity
limits."""
import numpy as np
import pytest

import psi_cases as K
import psi_ref as P

PID = K.PID


class Pair:
    """a host bank of one stream and the model, fed the same calls"""

    def __init__(self, pkg, max_packets=4096, max_sections=512, expect=-1, deliver=0):
        self.hb, self.m = pkg.PsiBank.host(1, max_packets, max_sections), P.Assembler()
        self.hb.set_watch(0, 1, PID, expect), self.m.set_watch(1, PID, expect)
        self.hb.set_deliver(0, deliver)
        self.m.deliver = deliver

    def call(self, ts, deliver=True):
        want, got = self.m.process(ts, deliver), self.hb.work(ts, deliver=deliver)
        assert (got is None) == (want is None) and (got is None or np.array_equal(got, want))
        assert self.hb.section_table() == self.m.table
        self.same_state()
        return want

    def same_state(self):
        for slot in (-1, 0, 1):
            assert self.hb.stats(0, slot) == self.m.stats(slot), slot
        hdr, rows = self.hb.programs()
        assert (hdr, rows) == self.m.programs()
        assert self.hb.program_map(0, 1) == self.m.program_map(1)


def test_model_crc_and_layout(pkg):
    assert P.crc32_mpeg(b'123456789') == 0x0376E6E7
    assert pkg.PsiBank.layout() == P.LAYOUT
    assert P.crc32_mpeg(P.pat(1, [(1, 0x100)])) == 0


CASES = K.edge_cases()
# what every case must show: (sections, valid, dropped_sections, malformed_sections, malformed_packets, crc_errors) of slot 1
EXPECT = {'pointer 0': (1, 1, 0, 0, 0, 0), 'pointer mid-packet, nothing open': (1, 1, 0, 0, 0, 0), 'largest pointer that leaves one byte': (1, 1, 0, 0, 0, 0),
          'pointer past the payload': (0, 0, 0, 0, 1, 0), 'three sections in one packet': (3, 3, 0, 0, 0, 0),
          'section ends exactly at the packet end': (1, 1, 0, 0, 0, 0), 'ends exactly at the end of a continuation packet': (1, 1, 0, 0, 0, 0),
          'header cut after 1 byte': (2, 2, 0, 0, 0, 0), 'header cut after 2 bytes': (2, 2, 0, 0, 0, 0), 'largest section': (1, 1, 0, 0, 0, 0),
          'section_length 4094': (0, 0, 0, 1, 0, 0), 'section_length 4094 in a cut header': (1, 1, 0, 1, 0, 0), 'ssi section of 11 bytes': (1, 1, 0, 1, 0, 0),
          'short section of 3 bytes': (2, 2, 0, 0, 0, 0), 'one byte of payload per packet': (1, 1, 0, 0, 0, 0),
          'adaptation field leaves one byte: the pointer': (0, 0, 0, 0, 0, 0), 'adaptation field leaves no payload with AFC 3': (0, 0, 0, 0, 1, 0),
          'pointer completes the open section': (2, 2, 0, 0, 0, 0), 'pointer too short for the open section': (1, 1, 1, 0, 0, 0),
          'pointer longer than the open section needs': (2, 2, 0, 0, 0, 0), 'continuation with nothing open': (0, 0, 0, 0, 0, 0),
          'adaptation only in the middle': (1, 1, 0, 0, 0, 0), 'drop_middle': (1, 1, 1, 0, 0, 0), 'announce_discontinuity': (1, 1, 1, 0, 0, 0),
          'scramble': (1, 1, 1, 0, 0, 0), 'flip_bit': (2, 1, 0, 0, 0, 1), 'duplicate': (2, 2, 0, 0, 0, 0)}


def test_constructed_edges_one_by_one(pkg):
    assert {c[0] for c in CASES} == set(EXPECT)
    pair = Pair(pkg)
    for name, ts, _ in CASES:
        before = pair.m.stats(1)
        pair.call(ts)
        d = {k: pair.m.stats(1)[k] - before[k] for k in P.STAT_KEYS}
        got = (d['sections'], d['valid'], d['dropped_sections'], d['malformed_sections'], d['malformed_packets'], d['crc_errors'])
        assert got == EXPECT[name], (name, got)
        assert d['packets'] == len(ts), name
    assert max(r['length'] for r in pair.m.table) < 4096 and pair.m.stats(1)['bytes_delivered'] > 4096


def test_walk_cases_whole_and_cut_at_every_packet(pkg):
    """the written-out rows of K.walk_cases(), and the same sections and counters from two calls cut at every packet boundary"""
    for name, ts, rows, counts in K.walk_cases():
        for at in range(len(ts)):                                   # 0: one call
            pair, got = Pair(pkg), []
            for part in ([ts[:at], ts[at:]] if at else [ts]):
                pair.call(part)
                got += [(r['table_id'], r['length']) for r in pair.m.table]
            st = pair.m.stats(1)
            assert got == [r[:2] for r in rows] and (st['dropped_sections'], st['malformed_sections']) == counts, (name, at)
            assert at or [r['first_packet'] for r in pair.m.table] == [r[2] for r in rows], name


def test_largest_section_and_row_fields(pkg):
    pair = Pair(pkg)
    sec = K._sec(4096, 12)
    out = pair.call(dict((c[0], c[1]) for c in CASES)['largest section'])
    assert bytes(out) == sec
    assert pair.m.table == [dict(pid=PID, flags=P.CHANGED, table_id=0x42, ssi=1, version=12, current_next=1, section_number=0, last_section_number=0,
                                 table_id_ext=12, length=4096, offset=0, first_packet=0)]


@pytest.mark.parametrize('inject', P.INJECTORS, ids=lambda f: f.__name__)
def test_each_fault_costs_what_its_injector_says(pkg, inject):
    z = P.Packetiser(PID)
    clean = np.concatenate([z.lay([K._sec(5 * 184 - 20, 1)]), z.lay([K._sec(33, 2)])])
    bad, cost = inject(clean, 2)
    a, b = Pair(pkg), Pair(pkg)
    a.call(clean), b.call(bad)
    for k in P.STAT_KEYS:
        if k != 'bytes_delivered':
            assert b.m.stats(1)[k] - a.m.stats(1)[k] == cost.get(k, 0), (k, cost)


def test_same_pat_is_changed_once_per_version(pkg):
    pair = Pair(pkg)
    z = P.Packetiser(0)
    progs = [(0, 0x10), (1, PID), (2, 0x31)]
    flags = []
    for version in (3, 3, 3, 4, 4):
        pair.call(z.lay([P.pat(9, progs, version=version)]))
        flags.append(pair.m.table[0]['flags'])
        assert pair.hb.programs() == (dict(transport_stream_id=9, version=version, malformed=0), progs)
    assert flags == [P.CHANGED, 0, 0, P.CHANGED, 0]
    pair.call(z.lay([P.pat(9, progs + [(3, 0x32)], version=5, current_next=0)]))          # a next PAT is flagged but is no view
    assert pair.m.table[0]['flags'] == P.CHANGED and pair.hb.programs()[0]['version'] == 4


def test_deliver_mode_1_against_mode_0_and_expect_table_id(pkg):
    ts = K.whole_stream(np.random.default_rng(3))
    all_, chg = Pair(pkg, expect=0x42, deliver=0), Pair(pkg, expect=0x42, deliver=1)
    a, b = all_.call(ts), chg.call(ts)
    strip = lambda t: [dict(r, offset=0) for r in t]
    assert strip(all_.m.table) == strip(chg.m.table)
    assert {k: v for k, v in all_.m.stats().items() if k != 'bytes_delivered'} == {k: v for k, v in chg.m.stats().items() if k != 'bytes_delivered'}
    keep = [r for r in all_.m.table if r['flags'] & P.CHANGED]
    assert 0 < len(keep) < len(all_.m.table) and b.size == sum(r['length'] for r in keep) < a.size
    assert bytes(b) == b''.join(bytes(a[r['offset']:r['offset'] + r['length']]) for r in keep)
    assert [r['offset'] for r in chg.m.table if not r['flags'] & P.CHANGED] == [-1] * (len(all_.m.table) - len(keep))
    assert all_.m.stats(1)['unexpected_table_id'] == sum(r['table_id'] != 0x42 for r in all_.m.table if r['pid'] == PID) > 0
    assert all_.m.stats(0)['unexpected_table_id'] == 0 and all_.m.stats(0)['changed'] == 3            # the PAT's versions 0, 1, 2
    rows_only = Pair(pkg, expect=0x42)
    assert rows_only.call(ts, deliver=False) is None and rows_only.m.stats()['bytes_delivered'] == 0


def _rebased(pair, pieces):
    """the calls' bytes and rows as one call would have given them.  A row's first_packet is rebased to the whole stream; where it is
    -1 the section must have begun in an earlier call: it becomes the index at which the PID's open section began, kept here from
    call to call"""
    out, rows = [], []
    opened = {}                                                   # PID -> whole-stream index where its open section began
    for a, ts in pieces:
        got = pair.call(ts)
        for r in pair.m.table:
            r = dict(r, offset=r['offset'] + sum(len(o) for o in out))
            if r['first_packet'] >= 0:
                r['first_packet'] += a
            else:
                assert r['pid'] in opened and opened[r['pid']] < a, (a, r)     # -1 exactly when it began before this call
                r['first_packet'] = opened[r['pid']]
            rows.append(r)
        out.append(got)
        for i, w in enumerate(pair.m.watch):                          # what is open behind this call, and since when
            s = pair.m.slot[i]
            if w[0] >= 0 and s['buf']:
                if s['first'] >= 0:
                    opened[w[0]] = a + s['first']
            else:
                opened.pop(w[0], None)
    return np.concatenate(out), rows


def test_cut_independence(pkg):
    rng = np.random.default_rng(17)
    z, zp = P.Packetiser(PID), P.Packetiser(0)
    five = z.lay([K._sec(4 * 184 + 100, 50)])
    assert len(five) == 5
    parts = [zp.lay([P.pat(7, [(1, PID)])]), P.filler(0x99, 40, rng), z.lay([K._sec(90, 51), K._sec(120, 52)]), P.filler(0x98, 30, rng)]
    start = sum(len(p) for p in parts)
    parts += [five, zp.lay([P.pat(7, [(1, PID)])]), P.filler(0x99, 100, rng), z.lay([K._sec(700, 53)]), P.filler(0x98, 110, rng), z.lay([K._sec(30, 54)])]
    ts = np.concatenate(parts)
    assert 290 <= len(ts) <= 310
    whole = Pair(pkg)
    want = whole.call(ts)
    want_rows = [dict(r) for r in whole.m.table]
    cuts = [[c] for c in range(start, start + 6)] + [sorted(set(rng.integers(0, len(ts) + 1, int(rng.integers(1, 8))).tolist())) for _ in range(20)]
    for cut in cuts:
        pair = Pair(pkg)
        edges = [0] + cut + [len(ts)]
        got, rows = _rebased(pair, [(a, ts[a:b]) for a, b in zip(edges[:-1], edges[1:])])
        assert np.array_equal(got, want), cut
        assert rows == want_rows, cut
        assert pair.m.stats() == whole.m.stats() and pair.hb.stats() == whole.hb.stats(), cut


def test_programs_program_map_and_follow_pat(pkg):
    hb, m = pkg.PsiBank.host(2, 256, 64), P.Assembler()
    progs = [(0, 0x10)] + [(n, 0x100 + n) for n in range(1, 21)]
    zp = P.Packetiser(0)
    pat_ts = zp.lay([P.pat(0x1234, progs, version=6)])
    hb.work(pat_ts, stream=1), m.process(pat_ts)
    assert hb.programs(1) == (dict(transport_stream_id=0x1234, version=6, malformed=0), progs) == m.programs()
    assert hb.programs(0) == (dict(transport_stream_id=-1, version=-1, malformed=0), [])
    assert hb.follow_pat(1) == progs[16:] and len(progs[16:]) == 5
    for slot, (n, p) in enumerate(progs[1:16], 1):
        m.set_watch(slot, p, 2)
    streams = [(0x1b, 0x200), (0x0f, 0x201), (0x06, 0x202)]
    good = P.pmt(1, 0x200, streams, version=2, program_info=b'\x09\x04abcd', es_info=b'\x0a\x04eng\x00')
    bad = P.pmt(2, 0x210, streams, es_info_length=40)                                  # runs past the section's end
    ts = np.concatenate([P.Packetiser(0x101).lay([good]), P.Packetiser(0x102).lay([bad]), P.Packetiser(0x103).lay([P.pat(1, [(5, 6)])])])
    hb.work(ts, stream=1), m.process(ts)
    assert hb.program_map(1, 1) == (dict(program_number=1, version=2, pcr_pid=0x200, malformed=0), streams) == m.program_map(1)
    assert hb.program_map(1, 2) == (dict(program_number=2, version=0, pcr_pid=0x210, malformed=1), []) == m.program_map(2)
    assert hb.program_map(1, 3) == (dict(program_number=-1, version=-1, pcr_pid=-1, malformed=0), []) == m.program_map(3)   # a PAT on a PMT PID
    assert hb.stats(1, 3)['unexpected_table_id'] == 1 == m.stats(3)['unexpected_table_id']
    assert hb.programs(1)[1] == progs                                                  # slot 0 holds the stream's PAT, not slot 3
    with pytest.raises(pkg.Dvbs2GpuError) as e:
        hb.set_watch(1, 5, 0x101)                                                      # watched in slot 1 already
    assert e.value.code == -1
    hb.set_watch(1, 1, -1)
    assert hb.program_map(1, 1)[0]['program_number'] == -1 and hb.stats(1, 1)['packets'] == 0
    hb.reset()
    assert hb.programs(1)[1] == [] and hb.stats(1)['packets'] == 0


def test_follow_pat_when_slot_0_watches_another_pid(pkg):
    hb = pkg.PsiBank.host(1, 64, 16)
    hb.set_watch(0, 0, 0x50, 0)                                    # the PAT of this feed travels on PID 0x50, and names it as a PMT PID too
    hb.work(P.Packetiser(0x50).lay([P.pat(1, [(1, 0x50), (2, 0x60)])]))
    assert hb.follow_pat(0) == [] and hb.programs(0)[1] == [(1, 0x50), (2, 0x60)]
    hb.work(P.Packetiser(0x60).lay([P.pmt(2, 0x61, [(2, 0x61)])]))
    assert hb.program_map(0, 1)[0]['program_number'] == 2 and hb.stats(0, 2)['packets'] == 0


def test_capacity_bytes_and_rows(pkg):
    ts = K.whole_stream(np.random.default_rng(5))
    probe = P.Assembler()
    probe.set_watch(1, PID)
    need, rows = probe.process(ts).size, len(probe.table)
    for kw, cap in ((dict(max_sections=rows), need - 1), (dict(max_sections=rows - 1), need)):
        pair = Pair(pkg, **kw)
        pair.call(ts[:40])
        before = pair.hb.stats()
        with pytest.raises(pkg.Dvbs2GpuError) as e:
            pair.hb.work(ts, cap=cap)
        probe2 = P.Assembler()
        probe2.set_watch(1, PID)
        probe2.process(ts[:40])
        want = probe2.process(ts)
        assert e.value.code == -5 and e.value.rows == len(probe2.table) and e.value.needed == (want.size if cap < need else -1)
        assert pair.hb.stats() == before and pair.hb.section_table() == []
    pair = Pair(pkg, max_sections=rows)
    pair.call(ts[:40])
    with pytest.raises(pkg.Dvbs2GpuError):
        pair.hb.work(ts[40:], cap=10)
    pair.call(ts[40:])                                                                  # the repeated call with room equals the model


def test_argument_checks(pkg):
    import ctypes as C
    lib, h, ARG = pkg.load_library(), C.c_void_p(), -1
    assert lib.dvbs2gpu_psi_create(None, 1, 16, 16, C.byref(h)) == ARG
    assert lib.dvbs2gpu_psi_create_host(0, 16, 16, C.byref(h)) == ARG
    assert lib.dvbs2gpu_psi_create_host(1, 4097, 16, C.byref(h)) == ARG
    assert lib.dvbs2gpu_psi_create_host(1, 16, 0, C.byref(h)) == ARG
    assert lib.dvbs2gpu_psi_create_host(1, 16, 16, None) == ARG
    assert lib.dvbs2gpu_psi_reset(None) == ARG and lib.dvbs2gpu_psi_get_layout(None) == ARG
    lib.dvbs2gpu_psi_destroy(None)
    assert lib.dvbs2gpu_psi_create_host(2, 16, 16, C.byref(h)) == 0
    assert lib.dvbs2gpu_psi_set_watch(h, 2, 0, 5, -1) == ARG and lib.dvbs2gpu_psi_set_watch(h, 0, 16, 5, -1) == ARG
    assert lib.dvbs2gpu_psi_set_watch(h, 0, 1, 0x1FFF, -1) == ARG and lib.dvbs2gpu_psi_set_watch(h, 0, 1, 5, 256) == ARG
    assert lib.dvbs2gpu_psi_set_watch(h, 0, 1, 0, 0) == ARG                            # PID 0 is in slot 0
    assert lib.dvbs2gpu_psi_set_deliver(h, 0, 2) == ARG
    buf = np.zeros(17 * 188, np.uint8)
    pb = C.c_void_p(buf.ctypes.data)
    assert lib.dvbs2gpu_psi_work(h, 0, pb, 187, None, 0) == ARG and lib.dvbs2gpu_psi_work(h, 0, pb, 17 * 188, None, 0) == ARG
    assert lib.dvbs2gpu_psi_work(h, 0, pb, 188, pb, 188) == ARG and lib.dvbs2gpu_psi_work(h, 0, None, 188, None, 0) == ARG
    pp = (C.c_void_p * 2)(buf.ctypes.data, buf.ctypes.data)
    assert lib.dvbs2gpu_psi_process_batch(h, pp, (C.c_int * 2)(0, 0), None, 0, None, None, None) == ARG    # a host bank has no device buffers
    st, n, p = pkg.PsiStats(), C.c_int(), C.c_void_p()
    assert lib.dvbs2gpu_psi_get_stats(h, 0, 16, C.byref(st)) == ARG and lib.dvbs2gpu_psi_get_stats(h, 0, -1, None) == ARG
    assert lib.dvbs2gpu_psi_get_section_table(h, 0, None, 1, C.byref(n)) == ARG
    assert lib.dvbs2gpu_psi_get_section_table_device(h, 0, C.byref(p), C.byref(n)) == ARG
    assert lib.dvbs2gpu_psi_get_stats(h, 0, -1, C.byref(st)) == 0 and st.packets == 0
    lib.dvbs2gpu_psi_destroy(h)
