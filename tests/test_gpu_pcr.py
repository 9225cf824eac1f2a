"""GPU tests of the PCR bank (csrc/pcr.hip): the kernel against the library's host bank and the model of tests/pcr_ref.py in rows,
counters, state (through the next call) and rate, at the packet counts, slot shapes and call boundaries where the compaction, the
sort by slot, the neighbour step and the reference position behind equal values can go wrong."""
import numpy as np
import pytest

import orc_bbts as B
import pcr_cases as K
import pcr_ref as P
import psi_ref as S

pytestmark = pytest.mark.gpu
PID = K.PID


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
        self.dv, self.hb = pkg.PcrBank(eng, nstreams, max_packets, max_rows), pkg.PcrBank.host(nstreams, max_packets, max_rows)
        self.models = [P.Clock(max_rows) for _ in range(nstreams)]
        for i in range(nstreams):
            for slot, pid in (watches[i] if watches else [(0, PID)]):
                self.set_watch(i, slot, pid)
            if tpp:
                self.dv.set_rate(i, tpp), self.hb.set_rate(i, tpp), self.models[i].set_rate(tpp)

    def set_watch(self, i, slot, pid):
        self.dv.set_watch(i, slot, pid), self.hb.set_watch(i, slot, pid), self.models[i].set_watch(slot, pid)

    def call(self, per_stream, shift=0):
        k0 = self.eng.get_state('kernel_launches')
        got = self.dv.process([_dev(ts, shift) for ts in per_stream], nbytes=[ts.size for ts in per_stream])
        assert self.eng.get_state('kernel_launches') - k0 == 1       # one launch per call, whatever the bank size
        for i, ts in enumerate(per_stream):
            assert got[i] == self.models[i].process(ts) == self.hb.work(ts, stream=i), i
            K.same(self.dv, self.models[i], i), K.same(self.hb, self.models[i], i)
        return [m.table for m in self.models]


def test_packet_counts_at_wave_and_workgroup_edges(pkg, eng):
    sizes = [0, 1, 2, 63, 64, 65, 255, 256, 257, 600]
    rng = np.random.default_rng(1)
    pids = [PID, 0x130]
    ts = P.stamped_mux(rng, sum(sizes), pids, tpp=K.TPP, jitter=16)    # a PCR every 7-40 packets per PID: pairs straddle most cuts
    rig = Rig(pkg, eng, watches=[list(enumerate(pids))])
    a, straddled = 0, 0
    for k, s in enumerate(sizes):
        rows = rig.call([ts[a:a + s]], shift=k % 2)[0]
        straddled += sum(r['kind'] == P.OK and r['delta_packets'] > r['packet'] for r in rows)
        a += s
    st = rig.models[0].stats()
    assert straddled >= 8 and st['ok'] > 60 and st['first'] == 2 and st['accuracy_errors'] > 5 and st['accuracy_measured'] - st['accuracy_errors'] > 5


def test_slot_shapes(pkg, eng):
    rng = np.random.default_rng(5)
    mp = 4096
    every = np.array([P.pcr_packet(0x44, 1000 * k + int(rng.integers(-14, 15)), cc=k) for k in range(mp)])      # every packet a PCR packet, at max_packets
    every[100:140] = every[100]                                                                                # and a long run of equal values
    pids = [0x100 + 3 * s for s in range(16)]
    sixteen = np.array([P.pcr_packet(pids[k % 16], 1000 * k, cc=k // 16) for k in range(16 * 25)])             # packet by packet: slot 0, 1, ... 15, 0, ...
    quiet = P.payload_packets(0x300, 50, rng)
    rig = Rig(pkg, eng, 3, mp, 8192, watches=[[(7, 0x44)], [(s, pids[s]) for s in reversed(range(16))], [(3, 0x55), (9, 0x44)]])
    rig.call([every, sixteen[:201], np.zeros((0, 188), np.uint8)])           # stream 2 brings nothing
    rig.call([quiet, sixteen[201:], every[:100]], shift=1)                   # stream 0: no PCR at all; stream 2: PID 0x55 never appears, 0x44 in slot 9
    rig.call([every[:300], quiet, np.zeros((0, 188), np.uint8)])             # stream 0: the pair reaches over the quiet call (a step back: JUMP)
    m = rig.models
    assert m[0].stats(7)['repeated'] == 2 * 39 and m[0].stats(7)['ok'] == 4056 + 260 and m[0].stats(7)['jumps'] == 1
    assert all(m[1].stats(s)['ok'] == 24 and m[1].stats(s)['first'] == 1 for s in range(16)) and m[1].stats()['accuracy_errors'] == 0
    assert m[2].stats(3)['pcr_packets'] == 0 and m[2].stats(9)['ok'] == 99 and m[2].stream_stats()['packets_since_pcr'][3] == -1


def test_three_streams_with_an_empty_one_in_the_middle(pkg, eng):
    """an odd stream count: the arrays of the argument table lie where the declared layout puts them"""
    rig = Rig(pkg, eng, 3, 64)
    rows = rig.call([K.spaced([0, 30000]), np.zeros((0, 188), np.uint8), K.spaced([0, 30014])])
    assert [len(r) for r in rows] == [2, 0, 2] and rows[2][1]['flags'] == K.A and rig.dv.stream_stats(1)['packets'] == 0


def _tuples(rows):
    return [(r['kind'], r['flags'], r['delta_ticks'], r['delta_packets'], r['accuracy']) for r in rows]


def test_constructed_edges_whole_and_cut_in_two(pkg, eng):
    rig, cut = Rig(pkg, eng, 1, 128), Rig(pkg, eng, 1, 128)
    anchors = {name: want for name, _, want in K.ANCHORS}
    for k, (name, ts) in enumerate(K.edge_cases()):
        rows = rig.call([ts], shift=k % 2)[0]
        halves = cut.call([ts[:len(ts) // 2]])[0] + [dict(r, packet=r['packet'] + len(ts) // 2) for r in cut.call([ts[len(ts) // 2:]], shift=1)[0]]
        assert halves == rows, name
        if name in anchors:
            assert _tuples(rows)[1:] == anchors[name], name
        if name in K.MIDDLE:
            assert len(rows) == K.MIDDLE[name][1], name
    assert rig.models[0].stats() == cut.models[0].stats() and rig.models[0].stats()['malformed'] == 4 and rig.models[0].stats()['repeated'] == 2
    assert rig.dv.stream_stats(0)['unwatched_pcr_packets'] == 1
    one = Rig(pkg, eng, 1, 2048)
    one.call([K.whole_stream()])                                    # and back to back in one call
    assert one.models[0].stats() == rig.models[0].stats()


def test_dn_32767_and_32768_through_calls_of_null_packets(pkg, eng):
    calls, want = K.saturation_calls()
    rig = Rig(pkg, eng, 1, 4096, tpp=80 << 24)
    rows = [r for c in calls for r in rig.call([c])[0]]
    assert rows[1:] == want and rig.dv.stats(0)['sum_packets'] == 32767


def test_rows_limit_rate_unset_unwatched_and_rewatching(pkg, eng):
    ts = K.spaced([30000 * j for j in range(10)])
    small = Rig(pkg, eng, 1, 512, 3)
    assert len(small.call([ts])[0]) == 3 and small.dv.stream_stats(0)['rows_dropped'] == 7 and small.dv.stats(0)['ok'] == 9
    p, n = small.dv.row_table_device(0)
    assert p and n == 3
    unset = Rig(pkg, eng, 1, 512, tpp=0)
    assert _tuples(unset.call([K.spaced([0, 30014, 60000])])[0])[1:] == [(P.OK, 0, 30014, 30, 0), (P.OK, 0, 29986, 30, 0)] and unset.dv.rate(0) == 40.608e6
    blind = Rig(pkg, eng, 1, 512, watches=[[]])
    assert blind.call([ts])[0] == [] and blind.dv.stream_stats(0)['first_unwatched_pid'] == PID
    blind.set_watch(0, 5, PID)
    assert _tuples(blind.call([K.spaced([300000, 330000])])[0]) == [(P.FIRST, 0, 0, 0, 0), (P.OK, 0, 30000, 30, 0)]
    blind.set_watch(0, 5, PID)                                      # re-watching: the slot starts afresh, the position goes on
    assert _tuples(blind.call([K.spaced([360000, 390000])])[0])[0] == (P.FIRST, 0, 0, 0, 0) and blind.dv.stats(0, 5)['first'] == 1
    for b in (blind.dv, blind.hb, blind.models[0]):
        b.reset()
    assert _tuples(blind.call([K.spaced([0, 30014])])[0])[1] == (P.OK, K.A, 30014, 30, 896)          # watch and rate stayed


def _psi_pcr_mux(rng, gap=(15, 40)):
    """a multiplex with a PAT, two PMTs that name PCR PIDs 0x200 and 0x210, and PCRs on both, stamped at 1000 ticks per packet"""
    zp, zm = S.Packetiser(0), [S.Packetiser(0x100), S.Packetiser(0x101)]
    ts = P.stamped_mux(rng, 400, [0x200, 0x210], tpp=K.TPP, gap=gap, jitter=5, other=0x201)
    at = 0
    for r in range(6):
        for sec in (zp.lay([S.pat(5, [(0, 0x10), (1, 0x100), (2, 0x101)])]), zm[0].lay([S.pmt(1, 0x200, [(0x1b, 0x200), (0x0f, 0x201)])]),
                    zm[1].lay([S.pmt(2, 0x210, [(0x02, 0x210)])])):
            while ts[at, 3] & 0x20:
                at += 1
            ts[at] = sec[0]
            at += 11
    return ts


def test_chained_behind_the_monitor_with_watches_from_the_pmts(pkg, eng):
    """the monitor's filter output is the PCR bank's input, and its watches come from a PsiBank that read the same buffer"""
    import torch
    mux = _psi_pcr_mux(np.random.default_rng(11))
    src = _dev(mux)
    psi = pkg.PsiBank(eng, 1, 512, 64)
    psi.process([src[:mux.size]])
    assert psi.follow_pat(0) == []
    psi.process([src[:mux.size]])
    pcr, m = pkg.PcrBank(eng, 1, 512, 64), P.Clock(64)
    assert pcr.follow_pmts(psi, 0) == [] and pcr._watched[0] == {0: 0x200, 1: 0x210}
    m.set_watch(0, 0x200), m.set_watch(1, 0x210)
    mon = pkg.TsMonitorBank(eng, 1, 512)
    mon.set_filter(0, mode=2, pids=[0x201])                         # the filter drops the filler PID: the positions change, the rate with them
    passed = torch.zeros(mux.size, dtype=torch.uint8, device='cuda')
    nb = mon.process([src[:mux.size]], [passed])[0]
    kept = mux[((mux[:, 1].astype(int) & 0x1f) << 8 | mux[:, 2]) != 0x201]
    assert nb == kept.size and 0 < nb < mux.size
    assert pcr.process([passed], nbytes=[nb]) == [m.process(kept)]
    K.same(pcr, m)
    assert m.stats(0)['ok'] > 5 and m.stats(1)['ok'] > 5 and m.stats()['jumps'] == 0


def test_chained_behind_the_packetiser_in_hbm(pkg, eng):
    """the output buffer of a BbTsParserBank call is the PCR bank's input, on the engine's stream: no host copy in between"""
    import torch
    mux = _psi_pcr_mux(np.random.default_rng(13), gap=(8, 20))
    kbch, nfr = 14232, 16
    frames = B.bbframes_from_ts(mux, kbch, nfr)
    bank = pkg.BbTsParserBank(eng, 1, kbch, nfr)
    ts_dev = torch.zeros(nfr * kbch // 8 + 376, dtype=torch.uint8, device='cuda')
    nb = bank.process_batch([torch.from_numpy(frames.reshape(-1)).cuda()], [ts_dev])[0]
    assert nb % 188 == 0 and nb // 188 >= nfr * (kbch // 8 - 10) // 188 - 1
    psi = pkg.PsiBank(eng, 1, 256, 64)
    psi.process([ts_dev], nbytes=[nb])
    assert psi.follow_pat(0) == []
    psi.process([ts_dev], nbytes=[nb])
    pcr, m = pkg.PcrBank(eng, 1, 256, 64), P.Clock(64)
    pcr.set_rate(0, K.TPP_Q24), m.set_rate(K.TPP_Q24)
    assert pcr.follow_pmts(psi, 0) == []
    m.set_watch(0, 0x200), m.set_watch(1, 0x210)
    assert pcr.process([ts_dev], nbytes=[nb]) == [m.process(mux[:nb // 188])]
    K.same(pcr, m)
    assert m.stats()['ok'] >= 8 and m.stats()['accuracy_measured'] == m.stats()['ok'] and m.stats()['accuracy_errors'] == 0
