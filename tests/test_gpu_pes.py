"""GPU tests of the PES bank (csrc/pes.hip): the kernel against the library's host bank and the model of tests/pes_ref.py in rows,
counters and state (through the next call), at the packet counts, slot shapes, call boundaries, alignments and payload offsets
where the compaction, the sort by slot, the parity of equal counters, the prefix sums and the unaligned header read can go wrong."""
import numpy as np
import pytest

import orc_bbts as B
import pes_cases as K
import pes_ref as P
import psi_ref as S

pytestmark = pytest.mark.gpu
PID = K.PID
NONE = np.zeros((0, 188), np.uint8)


@pytest.fixture(scope='module')
def eng(pkg):
    return pkg.Engine(0)


def _dev(ts, shift=0):
    import torch
    ts = np.ascontiguousarray(ts, np.uint8).reshape(-1)
    buf = torch.zeros(ts.size + 8, dtype=torch.uint8, device='cuda')
    buf[shift:shift + ts.size] = torch.from_numpy(ts).cuda()
    return buf[shift:]


class Rig:
    """a device bank, a host bank and one model per stream, fed the same calls"""

    def __init__(self, pkg, eng, nstreams=1, max_packets=600, max_rows=1024, watches=None, tpp=K.TPP_Q24):
        self.eng, self.n = eng, nstreams
        self.dv, self.hb = pkg.PesBank(eng, nstreams, max_packets, max_rows), pkg.PesBank.host(nstreams, max_packets, max_rows)
        self.models = [P.Pes(max_rows) for _ in range(nstreams)]
        for i in range(nstreams):
            for slot, pid in (watches[i] if watches else [(0, PID)]):
                self.dv.set_watch(i, slot, pid), self.hb.set_watch(i, slot, pid), self.models[i].set_watch(slot, pid)
            if tpp:
                self.dv.set_rate(i, tpp), self.hb.set_rate(i, tpp), self.models[i].set_rate(tpp)

    def call(self, per_stream, shift=0):
        k0 = self.eng.get_state('kernel_launches')
        got = self.dv.process([_dev(ts, shift) for ts in per_stream], nbytes=[ts.size for ts in per_stream])
        assert self.eng.get_state('kernel_launches') - k0 == 1       # one launch per call, whatever the bank size
        for i, ts in enumerate(per_stream):
            assert got[i] == self.models[i].process(ts) == self.hb.work(ts, stream=i), i
            K.same(self.dv, self.models[i], i), K.same(self.hb, self.models[i], i)
        return [m.table for m in self.models]

    def cut(self, ts, edges, shift=0):
        """one stream in calls that end at `edges` -> the concatenated rows, `packet` counted from the stream's start"""
        rows, a = [], 0
        for b in list(edges) + [len(ts)]:
            rows += [dict(r, packet=r['packet'] + a) for r in self.call([ts[a:b]], shift)[0]]
            a = b
        return rows


@pytest.fixture(scope='module')
def mux3():
    """a faulty multiplex on three PIDs, long enough for every packet count below"""
    return P.random_mux(np.random.default_rng(21), 9300, [0x150, 0x151, 0x152], tpp=K.TPP)


def test_packet_counts_at_wave_workgroup_and_thread_run_edges(pkg, eng, mux3):
    sizes = [0, 1, 63, 64, 65, 255, 256, 257, 4095, 4096]
    rig = Rig(pkg, eng, 1, 4096, 4096, watches=[[(4, 0x150), (0, 0x151), (9, 0x152)]])
    a = 0
    for k, s in enumerate(sizes):
        rig.call([mux3[a:a + s]], shift=k % 4)
        a += s
    st = rig.models[0].stats()
    assert st['starts'] > 1500 and min(st[k] for k in ('duplicates', 'cc_errors', 'closed_ok', 'closed_gap', 'ts_backward', 'dts_after_pts', 'starts_short', 'starts_malformed', 'with_dts')) > 10


def test_slot_shapes_and_a_call_of_starts_only(pkg, eng, mux3):
    rng = np.random.default_rng(5)
    pids = [0x100 + 3 * s for s in range(16)]
    sixteen = P.random_mux(rng, 1200, pids, tpp=K.TPP)
    ln = K.Line(0x44)
    for _ in range(4096):
        ln.start(declared=178, step=300)
    every = ln.take()                                                # every packet a start of one PID, at max_packets
    every[100:104] = every[100]                                      # and a run of equal counters among them: two duplicates, and a continuity error at 102 and at 104
    rig = Rig(pkg, eng, 3, 4096, 1000, watches=[[(7, 0x44)], [(s, pids[s]) for s in reversed(range(16))], [(3, 0x55), (9, 0x150), (2, 0x152), (1, 0x151)]])
    rows = rig.call([every, sixteen[:700], mux3[:500]])
    assert len(rows[0]) == 1000 and rig.dv.stream_stats(0)['rows_dropped'] == 4094 - 1000 and rig.models[0].stats(7)['closed_ok'] == 4091
    rig.call([NONE, sixteen[700:], mux3[500:1500]], shift=1)          # stream 0 brings nothing
    rig.call([every[:300], sixteen[:300], NONE], shift=3)             # stream 0: the timestamps step back over the quiet call
    m = rig.models
    assert m[0].stats(7)['ts_backward'] == 1 and m[0].stats(7)['duplicates'] == 4 and m[0].stats(7)['cc_errors'] == 4
    assert all(m[1].stats(s)['starts'] > 10 for s in range(16)) and m[2].stats(3)['packets'] == 0 and m[2].stream_stats()['packets_since_start'][3] == -1


def test_three_streams_with_an_empty_one_in_the_middle_and_a_stream_of_one_packet(pkg, eng):
    """an odd stream count: the arrays of the argument table lie where the declared layout puts them"""
    rig = Rig(pkg, eng, 3, 64)
    ln = K.Line()
    two, one = ln.start().start().take(), ln.start(declared=178).take()
    rows = rig.call([two, NONE, one])
    assert [len(r) for r in rows] == [2, 0, 1] and rows[2][0]['flags'] == P.TS_FIRST and rig.dv.stream_stats(1)['packets'] == 0
    rows = rig.call([one, one, NONE])
    assert [[r['flags'] for r in t] for t in rows] == [[K.CU], [P.TS_FIRST], []]


def test_constructed_cases_whole_and_cut_in_two(pkg, eng):
    rig, cut = Rig(pkg, eng, 1, 512), Rig(pkg, eng, 1, 512)
    for k, (name, ts, want) in enumerate(K.edge_cases()):
        rows = rig.call([ts], shift=k % 4)[0]
        assert cut.cut(ts, [len(ts) // 2], shift=(k + 1) % 4) == rows, name
        assert [(r['kind'], r['flags'], r['closed_bytes']) for r in rows][1:] == want, name
    assert rig.models[0].stats() == cut.models[0].stats() and min(rig.models[0].stats().values()) > 0
    one = Rig(pkg, eng, 1, 1024)
    one.call([K.whole_stream()])                                    # and back to back in one call
    assert one.models[0].stats() == rig.models[0].stats()


def test_a_pes_packet_over_two_and_three_calls(pkg, eng):
    ln = K.Line()
    ts = ln.start().start(declared=5 * 184 - 6).body(4).start().take()
    whole = Rig(pkg, eng, 1, 16)
    want = whole.cut(ts, [])
    assert [(r['flags'], r['closed_bytes'], r['closed_packets']) for r in want] == [(P.TS_FIRST, 0, 0), (K.CU, 184, 1), (P.CLOSED, 920, 5)]
    for c in range(1, len(ts)):
        assert Rig(pkg, eng, 1, 16).cut(ts, [c], shift=c % 4) == want, c
    for c in ((2, 4), (3, 5), (1, 6), (2, 3)):
        assert Rig(pkg, eng, 1, 16).cut(ts, c) == want, c


def test_a_run_of_equal_counters_across_a_cut(pkg, eng):
    ln = K.Line()
    ts = ln.start().start(declared=6 * 184 - 6).body().again().again().again().again().again().start().take()
    whole = Rig(pkg, eng, 1, 16)
    want = whole.cut(ts, [])                                        # behind the body: duplicate, error, duplicate, error, duplicate
    assert (want[2]['flags'], want[2]['closed_bytes'], want[2]['closed_packets']) == (K.CG, 4 * 184, 4)
    assert (whole.models[0].stats()['duplicates'], whole.models[0].stats()['cc_errors']) == (3, 2)
    for c in range(1, len(ts)):
        rig = Rig(pkg, eng, 1, 16)
        assert rig.cut(ts, [c]) == want and rig.models[0].stats() == whole.models[0].stats(), c
    rig = Rig(pkg, eng, 1, 16)
    assert rig.cut(ts, [3, 4, 5, 6, 7]) == want                      # the run one packet per call


def test_every_adaptation_field_length_on_a_start_at_every_alignment(pkg, eng):
    """the header read crosses every dword phase: payload offsets 4 and 5..187, input pointers at byte offsets 0..3"""
    ln = K.Line()
    ln.start()
    for a in range(183):
        ln.start(af_len=a, dts=ln.pts + K.STEP - 7, declared=a)
    ts = ln.take()
    for shift in range(4):
        rig = Rig(pkg, eng, 1, 256)
        rows = rig.call([ts], shift=shift)[0]
        assert [r['kind'] for r in rows[1:]] == [P.HEADER] * 165 + [P.SHORT] * 18 and [r['declared'] for r in rows[1:178]] == list(range(177))
        assert all((r['pts'] - r['dts']) % P.MOD == 7 for r in rows[1:166]) and rows[166]['pts'] == P.NO_TS


def _psi_pes_mux(rng):
    """a multiplex with a PAT, two PMTs that name elementary PIDs 0x200, 0x201 and 0x210, and PES packets on the three; PID 0x300 fills"""
    zp, zm = S.Packetiser(0), [S.Packetiser(0x100), S.Packetiser(0x101)]
    ts = P.random_mux(rng, 400, [0x200, 0x201, 0x210], other=0x300, tpp=K.TPP, faults=False)
    spare = [k for k in range(400) if (int(ts[k, 1]) & 0x1f) << 8 | int(ts[k, 2]) in (0x300, 0x1FFF)]
    sections = [(zp, S.pat(5, [(0, 0x10), (1, 0x100), (2, 0x101)])), (zm[0], S.pmt(1, 0x200, [(0x1b, 0x200), (0x0f, 0x201), (0x05, 0x300)])),
                (zm[1], S.pmt(2, 0x210, [(0x02, 0x210)]))]
    for j, k in enumerate(spare[:18]):                               # the tables, six times each, in place of filler
        z, sec = sections[j % 3]
        ts[k] = z.lay([sec])[0]
    return ts


def _watch_from_pmts(pkg, eng, src, nbytes, max_packets):
    """a PsiBank reads the buffer twice (PAT, then PMTs); a PesBank and the model take their watches from it"""
    psi = pkg.PsiBank(eng, 1, max_packets, 64)
    psi.process([src], nbytes=[nbytes])
    assert psi.follow_pat(0) == []
    psi.process([src], nbytes=[nbytes])
    pes, m = pkg.PesBank(eng, 1, max_packets, 256), P.Pes(256)
    pes.set_rate(0, K.TPP_Q24), m.set_rate(K.TPP_Q24)
    assert pes.follow_pmts(psi, 0) == [] and pes._watched[0] == {0: 0x200, 1: 0x201, 2: 0x210}      # (the section stream 0x300 is skipped)
    for s, pid in pes._watched[0].items():
        m.set_watch(s, pid)
    return pes, m


def test_chained_behind_the_monitor_with_watches_from_the_pmts(pkg, eng):
    """the monitor's filter output is the PES bank's input, and its watches come from a PsiBank that read the same buffer"""
    import torch
    mux = _psi_pes_mux(np.random.default_rng(11))
    src = _dev(mux)
    pes, m = _watch_from_pmts(pkg, eng, src[:mux.size], mux.size, 512)
    mon = pkg.TsMonitorBank(eng, 1, 512)
    mon.set_filter(0, mode=2, pids=[0x300], drop_null=True)         # the filter drops the filler: the positions change
    passed = torch.zeros(mux.size, dtype=torch.uint8, device='cuda')
    nb = mon.process([src[:mux.size]], [passed])[0]
    pid = (mux[:, 1].astype(int) & 0x1f) << 8 | mux[:, 2]
    kept = mux[(pid != 0x300) & (pid != 0x1FFF)]
    assert nb == kept.size and 0 < nb < mux.size
    assert pes.process([passed], nbytes=[nb]) == [m.process(kept)]
    K.same(pes, m)
    assert all(m.stats(s)['closed_ok'] > 3 for s in range(3)) and m.stats()['cc_errors'] == 0 and m.stats()['with_pts'] > 20


def test_chained_behind_the_packetiser_in_hbm(pkg, eng):
    """the output buffer of a BbTsParserBank call is the PES bank's input, on the engine's stream: no host copy in between"""
    import torch
    mux = _psi_pes_mux(np.random.default_rng(13))
    kbch, nfr = 14232, 16
    frames = B.bbframes_from_ts(mux, kbch, nfr)
    bank = pkg.BbTsParserBank(eng, 1, kbch, nfr)
    ts_dev = torch.zeros(nfr * kbch // 8 + 376, dtype=torch.uint8, device='cuda')
    nb = bank.process_batch([torch.from_numpy(frames.reshape(-1)).cuda()], [ts_dev])[0]
    assert nb % 188 == 0 and nb // 188 >= nfr * (kbch // 8 - 10) // 188 - 1
    pes, m = _watch_from_pmts(pkg, eng, ts_dev, nb, 256)
    assert pes.process([ts_dev], nbytes=[nb]) == [m.process(mux[:nb // 188])]
    K.same(pes, m)
    assert m.stats()['starts_header'] >= 8 and m.stats()['closed_ok'] >= 5 and m.stats()['cc_errors'] == 0
