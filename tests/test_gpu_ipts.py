"""GPU tests of the IP-TS bank (csrc/ipts.hip): the kernels against the library's host bank and the model of tests/ipts_ref.py in
bytes, rows, needed sizes, counters and state through the next call, at the row counts, stream shapes, alignments, datagram sizes and
UDP lengths where the wave per row, the head gather, the checksum's lead-in and tail, the ballot loop, the sequence walk, the prefix
sums and the copy can go wrong; and chained on the device behind the MPE bank and behind a GSE PDU table, in front of the TS monitor."""
import numpy as np
import pytest

import ipts_cases as K
import ipts_ref as R
import mpe_ref as MP
import tsmon_ref as TM

pytestmark = pytest.mark.gpu
EMPTY = (np.zeros(0, np.uint8), np.zeros((0, 2), np.int32))


@pytest.fixture(scope='module')
def eng(pkg):
    return pkg.Engine(0)


def _dev(a, shift=0):
    """a on the device, `shift` bytes behind a 16-byte boundary"""
    import torch
    a = np.ascontiguousarray(a).view(np.uint8).reshape(-1)
    buf = torch.zeros(a.size + 32, dtype=torch.uint8, device='cuda')
    assert buf.data_ptr() % 16 == 0
    buf[shift:shift + a.size] = torch.from_numpy(a.copy()).cuda()
    return buf[shift:]


class Rig:
    """a device bank, a host bank and one model per stream, fed the same calls.  flows[i]: [(slot, family, addr, port)]"""

    def __init__(self, pkg, eng, nstreams=1, max_rows=512, flows=None, cap=1 << 16):
        import torch
        self.pkg, self.eng, self.n = pkg, eng, nstreams
        self.dv, self.hb = pkg.IpTsBank(eng, nstreams, max_rows), pkg.IpTsBank.host(nstreams, max_rows)
        self.models = [R.Stream() for _ in range(nstreams)]
        self.used = [[False] * 4 for _ in range(nstreams)]
        self.outs = [[torch.zeros(cap + 32, dtype=torch.uint8, device='cuda') for _ in range(4)] for _ in range(nstreams)]
        self.cap = cap
        for i in range(nstreams):
            for f in (flows[i] if flows else [(k,) + fl for k, fl in enumerate(K.FLOWS)]):
                self.set_flow(i, *f)

    def set_flow(self, i, slot, family, addr=None, port=0):
        self.dv.set_flow(i, slot, family, addr, port), self.hb.set_flow(i, slot, family, addr, port), self.models[i].set_flow(slot, family, addr, port)
        self.used[i][slot] = family != 0

    def views(self, per_stream, kind, shift):
        """-> (views, the tensors that must outlive the call)"""
        views, keep = [], []
        for data, table in per_stream:
            if len(table) == 0:
                views.append(None)
                continue
            d, t = _dev(data, shift), _dev(np.ascontiguousarray(table, np.int32))
            keep += [d, t]
            views.append(self.pkg.IptsView(d.data_ptr(), t.data_ptr(), 8, 0, 4, kind, len(table), 0))
        return views, keep

    def call(self, per_stream, kind=R.RAW_IP, deliver=True, shift=0, out_shift=0):
        views, keep = self.views(per_stream, kind, shift)
        # an empty slot has no buffer
        outs = [[o[out_shift:out_shift + self.cap] if self.used[i][k] else None for k, o in enumerate(per)] for i, per in enumerate(self.outs)]
        k0 = self.eng.get_state('kernel_launches')
        nb = self.dv.process(views, outs if deliver else None)
        assert self.eng.get_state('kernel_launches') - k0 == 2       # whatever the bank size
        res = []
        for i, (data, table) in enumerate(per_stream):
            want = self.models[i].process(data, table, kind, deliver)
            host = self.hb.work(data, table, kind, stream=i, deliver=deliver)
            got = self.dv.row_table(i)
            for j, (a, b) in enumerate(zip(got, self.models[i].table)):
                assert a == b, (i, j, a, b)
            assert got == self.models[i].table == self.hb.row_table(i), i
            for k in range(4):
                if deliver:
                    assert nb[i][k] == want[k].size, (i, k, nb[i][k], want[k].size)
                    if self.used[i][k]:
                        assert np.array_equal(outs[i][k][:nb[i][k]].cpu().numpy(), want[k]), (i, k)
                    assert np.array_equal(host[k], want[k]), (i, k)
                assert self.dv.needed(i, k) == (want[k].size if deliver else 0) == self.hb.needed(i, k), (i, k)
                assert self.dv.stats(i, k) == self.models[i].stats(k) == self.hb.stats(i, k), (i, k)
            assert self.dv.stats(i) == self.models[i].stats() == self.hb.stats(i), i
            res.append(want)
        del keep
        return res


def test_row_counts_at_wave_and_workgroup_edges(pkg, eng):
    """0, 1, 4, 5 and 257 rows: fewer rows than waves, one more than the waves of a workgroup, more rows than threads; one bank through
    all of them, so every call starts from the state the one before left"""
    sizes = [0, 1, 4, 5, 257, 5, 0, 4]
    data, table = K.random_table(11, sum(sizes))
    rig, rows_only = Rig(pkg, eng, cap=1 << 18), Rig(pkg, eng)
    a = 0
    for c, n in enumerate(sizes):
        part = table[a:a + n]
        rig.call([(data, part)], shift=c % 4, out_shift=(c + 1) % 4)
        rows_only.call([(data, part)], deliver=False, shift=(c + 2) % 4)
        a += n
    st = rig.models[0].stats()
    assert min(st[k] for k in R.STAT_KEYS) > 0, st                   # the calls have met every rule
    assert rows_only.models[0].stats()['bytes_delivered'] == 0 and rows_only.models[0].stats()['ts'] == st['ts']


def test_three_streams_with_different_flows(pkg, eng):
    """stream 0 with the four flows, stream 1 with none, stream 2 with the IPv6 flow in slot 3 alone; now and then an empty view"""
    flows = [[(k,) + f for k, f in enumerate(K.FLOWS)], [], [(3,) + K.FLOWS[1]]]
    rig = Rig(pkg, eng, 3, 64, flows)
    tabs = [K.random_table(20 + i, 150) for i in range(3)]
    for c, a in enumerate(range(0, 150, 50)):
        per = [(d, t[a:a + 50 - 7 * i]) for i, (d, t) in enumerate(tabs)]
        per[c % 3] = EMPTY
        rig.call(per, shift=c, out_shift=3 - c)
    assert rig.models[1].stats()['matched'] == 0 and rig.models[1].stats()['unwatched'] > 30
    assert rig.models[2].stats(3)['ts'] > 5 and rig.models[2].stats(0)['matched'] == 0 and rig.models[0].stats(0)['ts'] > 5
    one = Rig(pkg, eng, 1, 64)                                       # the same table through a bank of one stream: the streams are apart
    for c, a in enumerate(range(0, 150, 50)):
        if c % 3 != 0:
            one.call([(tabs[0][0], tabs[0][1][a:a + 50])])
    assert one.dv.stats(0) == rig.dv.stats(0)


@pytest.mark.parametrize('per_call', [0, 1, 7])
@pytest.mark.parametrize('kind', [R.RAW_IP, R.GRE])
def test_constructed_cases_cut_into_calls(pkg, eng, kind, per_call):
    """the written rows, in one call and in calls of 1 and 7 rows: LOSS, LATE and NEW_SOURCE across call boundaries"""
    cases = K.cases() if kind == R.RAW_IP else K.gre_cases()
    data, table = K.table_of(cases, shift=per_call, gap=3)
    rig = Rig(pkg, eng, 1, 128)
    got = []
    for c, part in enumerate(K.calls_of(table, per_call)):
        rig.call([(data, part)], kind, shift=c % 4, out_shift=(c // 4) % 4)
        got += [(r['flags'], r['slot'], r['packets'], r['lost']) for r in rig.models[0].table]
    for (name, *_), g, w in zip(cases, got, K.expected_rows(cases)):
        assert g == w, name
    assert rig.models[0].stats() == K.expected_stats(cases) == rig.dv.stats(0)


@pytest.mark.parametrize('shift', [0, 1, 2, 3])
def test_datagrams_of_1_to_66_packets(pkg, eng, shift):
    """1, 7, 64, 65 and 66 TS packets, raw and in RTP: one round of the ballot, one round exactly, a second round of one and of two lanes,
    and the long copy; a wrong sync byte in the last packet of each must be found"""
    ds, seq = [], 0
    for n in (1, 7, 64, 65, 66):
        ts = R.ts_packets(n, seed=n)
        bad = bytearray(ts)
        bad[188 * (n - 1)] = 0x48
        seq += 2
        ds += [R.datagram(ts), R.datagram(R.rtp(ts, seq=seq)), R.datagram(ts, 6), R.datagram(R.rtp(ts, seq=seq // 2, cc=shift), 6),
               R.datagram(R.rtp(bytes(bad), seq=seq + 1)), R.datagram(bytes(bad)), R.datagram(R.rtp(ts, seq=seq + 1, pad=1 + shift))]
    data, table = R.lay(ds, gap=7, seed=shift)
    rig = Rig(pkg, eng, 1, 64, cap=1 << 17)
    rig.call([(data, table)], shift=shift, out_shift=3 - shift)
    st = rig.models[0].stats()
    assert (st['raw'], st['rtp'], st['bad_payload'], st['ts'], st['loss_events']) == (10, 15, 10, 25, 0)
    rig.call([(data, table[::-1].copy())], shift=shift + 4, out_shift=shift)    # and backwards: late ones, other offsets
    assert rig.models[0].stats()['late'] == 15


def test_udp_lengths_at_every_alignment(pkg, eng):
    """UDP lengths 8, 9, 11, 12 and up to 41, each datagram at each of the 16 places against a 16-byte boundary, so that a UDP datagram
    ends one byte before, on and one byte behind a boundary with every lead-in: the checksum must hold (the payload is then found bad),
    and with one bit turned over it must not"""
    rng = np.random.default_rng(5)
    lengths = [8, 9, 11, 12, 23, 24, 25, 39, 40, 41]
    rig = Rig(pkg, eng, 1, 64)
    for shift in range(16):
        ds = []
        for L in lengths:
            p = bytes(rng.integers(0, 256, L - 8, dtype=np.uint8))
            good = R.datagram(b'\x40' + p[1:] if p else p, 4 if L % 2 else 6)
            ds += [good, K.flip(good)]                               # (the last payload byte, or the checksum's of an empty datagram)
        data, table = R.lay(ds, shift=shift)
        rig.call([(data, table)], shift=0, out_shift=shift % 4)
        assert [r['flags'] for r in rig.models[0].table] == [R.BAD_PAYLOAD, R.BAD_CHECKSUM] * len(lengths), shift
    ends = set()
    for shift in range(16):
        at = shift
        for L in lengths:
            ends.add((at + (20 if L % 2 else 40) + L) % 16)
            at += 2 * ((20 if L % 2 else 40) + L)
    assert ends == set(range(16))                                    # every place of a UDP datagram's end against the boundary was met


def test_capacity_failure_then_the_repeated_call(pkg, eng):
    import torch
    cases = K.cases()
    tabs = [K.table_of(cases), K.random_table(31, 90)]
    rig = Rig(pkg, eng, 2, 128)
    heads = [(d, t[:40]) for d, t in tabs]
    rests = [(d, t[40:]) for d, t in tabs]
    rig.call(heads)
    need = [m.sizes(d, t) for m, (d, t) in zip(rig.models, rests)]
    before = [[rig.dv.stats(i, k) for k in (-1, 0, 1, 2, 3)] for i in range(2)]
    views, keep = rig.views(rests, R.RAW_IP, 1)
    top = max(max(n) for n in need)
    small = lambda cap: [[torch.zeros(cap, dtype=torch.uint8, device='cuda') for _ in range(4)] for _ in range(2)]
    k0 = eng.get_state('kernel_launches')
    with pytest.raises(pkg.Dvbs2GpuError) as e:
        rig.dv.process(views, small(top - 1))                        # one byte short for the slot that needs most
    assert eng.get_state('kernel_launches') - k0 == 1                # the sizes come first: nothing was committed
    assert e.value.code == -5 and e.value.needed == need and need == [[rig.dv.needed(i, k) for k in range(4)] for i in range(2)]
    assert [[rig.dv.stats(i, k) for k in (-1, 0, 1, 2, 3)] for i in range(2)] == before
    assert rig.dv.row_table(0) == [] and rig.dv.row_table(1) == []
    exact = small(top)
    assert rig.dv.process(views, exact) == need                      # exactly enough room; the state was what the failed call found
    want = rig.models[0].process(*rests[0])
    assert all(np.array_equal(exact[0][k][:need[0][k]].cpu().numpy(), want[k]) for k in range(4)) and rig.dv.row_table(0) == rig.models[0].table
    rig.models[1].process(*rests[1])
    for i in range(2):
        rig.hb.work(*rests[i], stream=i)
    assert rig.models[0].stats(3)['late'] > 0 and rig.models[0].stats(3)['loss_events'] > 0
    rig.call([(d, t[-20:]) for d, t in tabs])                        # and the state behind it
    with pytest.raises(pkg.Dvbs2GpuError) as e:                      # more rows than max_rows: an argument error, before any launch
        rig.dv.process(rig.views([K.random_table(3, 129), EMPTY], R.RAW_IP, 0)[0])
    assert e.value.code == -1
    del keep


def test_work_with_host_buffers_on_a_device_bank(pkg, eng):
    """dvbs2gpu_ipts_work on a device bank: the view's bytes and table staged, the other stream an empty call; with delivery, rows
    only, and at the capacity limit"""
    rig = Rig(pkg, eng, 2, 128)
    data, table = K.table_of(K.cases(), shift=5, gap=2)
    m = rig.models[1]
    for part, deliver in ((table[:30], True), (table[30:50], False), (table[50:], True)):
        want = m.process(data, part, deliver=deliver)
        k0 = eng.get_state('kernel_launches')
        got = rig.dv.work(data, part, stream=1, deliver=deliver)
        assert eng.get_state('kernel_launches') - k0 == 2
        assert (got is None) == (want is None) and (got is None or all(np.array_equal(g, w) for g, w in zip(got, want)))
        assert rig.dv.row_table(1) == m.table and rig.dv.row_table(0) == [] and rig.dv.stats(1) == m.stats()
        assert [rig.dv.needed(1, k) for k in range(4)] == ([w.size for w in want] if deliver else [0] * 4)
    need, before = m.sizes(data, table[:30]), rig.dv.stats(1)
    with pytest.raises(pkg.Dvbs2GpuError) as e:
        rig.dv.work(data, table[:30], stream=1, cap=max(need) - 1)
    assert e.value.code == -5 and e.value.needed == need and rig.dv.stats(1) == before and rig.dv.row_table(1) == []
    want = m.process(data, table[:30])
    got = rig.dv.work(data, table[:30], stream=1, cap=max(need))
    assert all(np.array_equal(g, w) for g, w in zip(got, want)) and rig.dv.row_table(1) == m.table and rig.dv.stats(1) == m.stats()
    assert rig.dv.stats(0) == rig.models[0].stats()                  # stream 0 saw nothing


def test_chained_on_the_device_behind_the_mpe_bank(pkg, eng):
    """an inner TS in RTP datagrams in MPE sections in an outer TS -> MpeBank -> the view of its row table -> IpTsBank -> TsMonitorBank,
    all in HBM, against the three models in sequence; no packet visits the host"""
    import torch
    rng = np.random.default_rng(17)
    inner, _ = TM.make_mux(rng, 7 * 12, [0x100, 0x101, 0x102])
    inner = np.ascontiguousarray(inner, np.uint8).reshape(-1, 188)
    ds = [R.datagram(R.rtp(inner[a:a + 7].tobytes(), seq=65530 + a // 7 & 0xFFFF, timestamp=3000 * a)) for a in range(0, len(inner), 7)]
    secs = [MP.section(d) for d in ds]
    secs.insert(5, MP.raw_section(0x3B, bytes(50)))                  # another table between them: a row without a datagram
    secs.insert(9, MP.section(R.datagram(R.rtp(inner[:7].tobytes(), seq=5), dport=99)))      # and a datagram of another port
    outer = MP.Packetiser(0x0300).lay(secs)
    mpe = pkg.MpeBank(eng, 1, 4096, 64)
    mpe.set_watch(0, 0, 0x0300)
    ip_dev = torch.zeros(outer.size, dtype=torch.uint8, device='cuda')
    nip = mpe.process([_dev(outer)], [[ip_dev]], nbytes=[outer.size])[0][0]
    view, src = pkg.IpTsBank.view_from_mpe(mpe, ip_dev, 0, 0)
    assert src is ip_dev and view.n == len(secs) and view.kind == pkg.IpTsBank.KIND_RAW_IP
    bank = pkg.IpTsBank(eng, 1, 64)
    bank.set_flow(0, 0, 4, R.V4_DST, K.PORT)
    ts_dev = torch.zeros(inner.size + 8, dtype=torch.uint8, device='cuda')[3:]
    nts = bank.process([view], [[ts_dev]])[0][0]
    mon = pkg.TsMonitorBank(eng, 1, 4096)
    mon.process([ts_dev], None, nbytes=[nts])
    # the three models in sequence
    m1 = MP.Slot(0x0300)
    ip_want = m1.process(outer)
    assert nip == ip_want.size and np.array_equal(ip_dev[:nip].cpu().numpy(), ip_want) and mpe.row_table(0, 0) == m1.table
    m2 = R.Stream()
    m2.set_flow(0, 4, R.V4_DST, K.PORT)
    ts_want = m2.process(ip_want, [(r['offset'], r['bytes']) for r in m1.table])[0]
    assert bank.row_table(0) == m2.table and [r['flags'] for r in m2.table].count(R.RTP | R.TS_ROW) == len(ds)
    assert {r['flags'] for r in m2.table} == {R.RTP | R.TS_ROW, R.NOT_DELIVERED, R.UNWATCHED}
    assert nts == ts_want.size == inner.size and np.array_equal(ts_dev[:nts].cpu().numpy(), inner.reshape(-1))
    m3 = TM.Monitor()
    m3.process(ts_want)
    assert mon.stats(0) == m3.stats() and mon.pid_table(0) == m3.table and m3.stats()['cc_errors'] == 0
    assert bank.stats(0) == m2.stats() and m2.stats()['lost'] == 0 and m2.stats()['ts_packets'] == len(inner)


def test_chained_on_the_device_behind_a_gse_pdu_table(pkg, eng):
    """the same inner TS in RTP datagrams in GSE packets in BBFRAMEs -> BbTsParserBank -> the view of its PDU table (kind GRE) ->
    IpTsBank -> TsMonitorBank"""
    import torch
    import orc_bbts as B
    from test_gpu_gse import pack_frames
    rng = np.random.default_rng(19)
    kbch = 14232
    inner, _ = TM.make_mux(rng, 7 * 9, [0x200, 0x201])
    inner = np.ascontiguousarray(inner, np.uint8).reshape(-1, 188)
    ds = [R.datagram(R.rtp(inner[a:a + 7].tobytes(), seq=a // 7), 6) for a in range(0, len(inner), 7)]
    pdus = [(0x86DD, d) for d in ds]
    pdus.insert(4, (0x88B5, bytes(60)))                              # a PDU that is not IP: a two-byte GRE header
    frames = pack_frames([B.gse_complete(p, d) for p, d in pdus], kbch)
    parser = pkg.BbTsParserBank(eng, 1, kbch, len(frames))
    gre_dev = torch.zeros(frames.size + 376 + 3 * 65536, dtype=torch.uint8, device='cuda')
    ngre = parser.process_batch([torch.from_numpy(np.ascontiguousarray(frames).reshape(-1)).cuda()], [gre_dev])[0]
    rows = parser.pdu_table(0)
    assert len(rows) == len(pdus) and sum(r[1] for r in rows) == ngre
    view, _ = pkg.IpTsBank.view_from_pdu_table(parser, gre_dev, 0)
    assert view.n == len(pdus) and view.kind == pkg.IpTsBank.KIND_GRE
    bank = pkg.IpTsBank(eng, 1, 64)
    bank.set_flow(0, 1, 6, R.V6_DST, K.PORT)
    ts_dev = torch.zeros(inner.size, dtype=torch.uint8, device='cuda')
    nts = bank.process([view], [[None, ts_dev]])[0][1]
    mon = pkg.TsMonitorBank(eng, 1, 4096)
    mon.process([ts_dev], None, nbytes=[nts])
    m2 = R.Stream()
    m2.set_flow(1, 6, R.V6_DST, K.PORT)
    ts_want = m2.process(gre_dev[:ngre].cpu().numpy(), [(r[0], r[1]) for r in rows], R.GRE)[1]
    assert bank.row_table(0) == m2.table and [r['flags'] for r in m2.table] == [R.RTP | R.TS_ROW] * 4 + [R.NOT_IP] + [R.RTP | R.TS_ROW] * 5
    assert nts == ts_want.size == inner.size and np.array_equal(ts_dev[:nts].cpu().numpy(), inner.reshape(-1))
    m3 = TM.Monitor()
    m3.process(ts_want)
    assert mon.stats(0) == m3.stats() and mon.pid_table(0) == m3.table and bank.stats(0) == m2.stats()
