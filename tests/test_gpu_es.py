"""GPU tests of the ES bank (csrc/es.hip): the kernel against the library's host bank and the model of tests/es_ref.py in rows, counters
and state (through the next call), with one launch per call, at the packet counts, slot shapes, call boundaries, alignments, payload
lengths and window splits where the compaction, the sort by slot, the prefix sums, the gathering of the 7 bytes in front of a segment
and the unaligned reads can go wrong."""
import numpy as np
import pytest

import es_cases as K
import es_ref as E
import orc_bbts as B
import pes_ref as P
import psi_ref as S

pytestmark = pytest.mark.gpu
NONE = np.zeros((0, 188), np.uint8)
THREE = [(4, K.PIDS[E.MPEG2], E.MPEG2), (0, K.PIDS[E.H264], E.H264), (9, K.PIDS[E.H265], E.H265)]
M2 = [(0, 0x150, E.MPEG2)]
CODE = K.SC + b'\xB8' + b'\x21\x22\x23\x24'                   # a GOP header of MPEG-2: 8 bytes, one window
GOP = (E.GOP, 0xB8, 0, 0x21222324)


@pytest.fixture(scope='module')
def eng(pkg):
    return pkg.Engine(0)


def _dev(ts, shift=0):
    import torch
    ts = np.array(ts, np.uint8).reshape(-1)                           # (a copy: the shared multiplex is read-only)
    buf = torch.zeros(ts.size + 8, dtype=torch.uint8, device='cuda')
    buf[shift:shift + ts.size] = torch.from_numpy(ts).cuda()
    return buf[shift:]


class Rig:
    """a device bank, a host bank and one model per stream, fed the same calls"""

    def __init__(self, pkg, eng, nstreams=1, max_packets=64, max_rows=4096, watches=None):
        self.eng, self.n = eng, nstreams
        self.dv, self.hb = pkg.EsBank(eng, nstreams, max_packets, max_rows), pkg.EsBank.host(nstreams, max_packets, max_rows)
        self.models = [E.Es(max_rows) for _ in range(nstreams)]
        for i in range(nstreams):
            for slot, pid, codec in (watches[i] if watches else M2):
                self.dv.set_watch(i, slot, pid, codec), self.hb.set_watch(i, slot, pid, codec), self.models[i].set_watch(slot, pid, codec)

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


def codes(rows):
    """the code rows as (unit, code, flags, head, es_offset, packet)"""
    return [(r['unit'], r['code'], r['flags'], r['head'], r['es_offset'], r['packet']) for r in rows if r['unit'] != E.PES]


def test_packet_counts_at_wave_workgroup_and_thread_run_edges(pkg, eng):
    mux = K.gpu_mux()                                                 # (tests/test_es_cpu.py: at least 10 of everything per codec)
    rig = Rig(pkg, eng, 1, 4096, 8192, watches=[THREE])
    a = 0
    for k, s in enumerate([0, 1, 63, 64, 65, 255, 256, 257, 4095, 4096]):
        rig.call([mux[a:a + s]], shift=k % 4)
        a += s
    st = rig.models[0].stats()
    assert st['pictures'] > 500 and st['resets'] > 100 and rig.dv.stream_stats(0) == dict(packets=a, rows_dropped=0)


@pytest.mark.parametrize('c', range(1, 8))
def test_one_window_split_at_each_inner_position(pkg, eng, c):
    """the 8 bytes of a code, c of them in front of the split: between two packets, between two calls, and across a valid PES start
    whose header lies between its bytes"""
    tail = b'\x31' * 3 + CODE                                        # a second code of the last packet alone
    want = [GOP[:2] + (0,) + GOP[3:] + (5, 1), GOP[:2] + (0,) + GOP[3:] + (16, 1)]
    ln = K.Line(0x150).pes(b'\x30' * 5 + CODE[:c], sizes=[19 + c]).put(CODE[c:] + tail)
    ts = ln.take()
    assert codes(Rig(pkg, eng).cut(ts, [], shift=c % 4)) == want
    assert codes(Rig(pkg, eng).cut(ts, [1], shift=(c + 1) % 4)) == want
    ts = K.Line(0x150).pes(b'\x30' * 5 + CODE[:c], sizes=[19 + c]).pes(CODE[c:] + tail, stuffing=c % 3).take()
    rig = Rig(pkg, eng)
    rows = rig.cut(ts, [], shift=c % 4)
    assert codes(rows) == want and [r['es_offset'] for r in rows if r['unit'] == E.PES] == [0, 5 + c] and rig.models[0].stats()['resets'] == 0
    assert Rig(pkg, eng).cut(ts, [1]) == rows


def test_one_window_over_eight_packets_of_one_byte(pkg, eng):
    """adaptation_field_length 182 leaves one payload byte: the 7 bytes in front of the last lie in 7 packets, with a duplicate, a
    packet without payload and packets of other PIDs between them; whole, and cut into calls at every packet"""
    ln = K.Line(0x150).pes(b'\x30' * 5, sizes=[19])
    for i, b in enumerate(CODE):
        ln.put(bytes([b]))
        if i == 2:
            ln.again()
        if i == 4:
            ln.no_payload()
        if i == 5:
            ln.out.append(P.null_packets(1)[0])
            ln.out.append(P.ts_packet(0x151, 3, CODE))
    ln.put(CODE)                                                     # and one more code, its first 7 bytes' window reaching back over the single bytes
    ts = ln.take()
    want = [GOP[:2] + (0,) + GOP[3:] + (5, 12), GOP[:2] + (0,) + GOP[3:] + (13, 13)]
    for shift in range(4):
        assert codes(Rig(pkg, eng).cut(ts, [], shift)) == want
    assert codes(Rig(pkg, eng).cut(ts, range(1, len(ts)))) == want
    assert codes(Rig(pkg, eng).cut(ts, range(2, len(ts), 3), shift=3)) == want


def test_a_header_that_ends_with_its_packet_and_one_that_is_split(pkg, eng):
    ln = K.Line(0x150)
    ln.put(K.head(93600) + CODE[:3], pusi=1).put(K.head(97200), pusi=1).put(CODE[3:] + CODE)       # an empty segment between the bytes of a window
    ln.put(K.head(100800, stuffing=6)[:16], pusi=1).put(b'\xFF' * 4 + CODE)                          # 9 + 11 > 16: split; the code is not scanned
    ln.put(K.head(104400) + CODE[:5], pusi=1).put(CODE[5:] + CODE)
    ts = ln.take()
    rig = Rig(pkg, eng)
    rows = rig.cut(ts, [], shift=1)
    U, SP, RS, H = E.UNSYNCED, E.SPLIT_HEADER, E.RESYNC, P.HEADER
    assert [(r['unit'], r['detail'] if r['unit'] == E.PES else r['code'], r['flags'], r['packet'], r['es_offset']) for r in rows] == [
        (E.PES, H, 0, 0, 0), (E.PES, H, 0, 1, 3), (E.GOP, 0xB8, 0, 2, 0), (E.GOP, 0xB8, 0, 2, 8),
        (E.PES, H, U | SP, 3, 16), (E.PES, H, RS, 5, 16), (E.GOP, 0xB8, 0, 6, 16), (E.GOP, 0xB8, 0, 6, 24)]
    st = rig.models[0].stats()
    assert (st['split_headers'], st['pes_invalid'], st['bytes_unsynced'], st['resets']) == (1, 1, 12, 1)
    for c in range(1, len(ts)):
        assert Rig(pkg, eng).cut(ts, [c], shift=c % 4) == rows, c


@pytest.mark.parametrize('shift', range(4))
def test_every_adaptation_field_length_on_a_start_and_on_a_packet_that_completes_a_code(pkg, eng, shift):
    """payload offsets 4 and 5..187: the start's header read and the segment's dwords cross every phase, at input pointers 0..3"""
    ln = K.Line(0x150)
    for L in range(184, 0, -1):
        ln.put((K.head(ln.pts + 3600 * L, stuffing=L % 3) + CODE + b'\x35' * 170)[:L], pusi=1)      # a start of L payload bytes
        ln.pes(b'\x36' * 163 + CODE[:7])                                                           # a full packet that ends 7 bytes into a code
        ln.put((CODE[7:] + CODE * 23)[:L])                                                         # L bytes, the first of which completes it
    ts = ln.take()
    rig = Rig(pkg, eng, 1, 600)
    rows = rig.call([ts], shift)[0]
    st = rig.models[0].stats()
    assert st['codes'] > 184 * 13 and st['pes_invalid'] >= 13 and st['pes_starts'] == 368
    assert sum(r['unit'] == E.GOP and r['packet'] % 3 == 2 and ts[r['packet'], 4] == 182 for r in rows) == 1


@pytest.mark.parametrize('fault', ['duplicate', 'lost', 'di', 'scrambled', 'malformed'])
def test_a_fault_between_the_bytes_of_a_window(pkg, eng, fault):
    """a duplicate changes nothing; any other fault loses the code and the next row carries RESYNC; the same when cut at every packet"""
    ln = K.Line(0x150).pes(b'\x33' * 10 + CODE[:4], sizes=[28])
    if fault == 'duplicate':
        ln.again()
    if fault == 'lost':
        ln.lose()
    if fault == 'di':
        ln.no_payload(di=1)
    if fault == 'scrambled':
        ln.put(b'\x5A' * 184, tsc=1)
    if fault == 'malformed':
        ln.out.append(P.ts_packet(0x150, ln.cc, b'', af_len=183, afc=3))
        ln.cc += 1
    ts = ln.put(CODE[4:] + b'\x33' * 3 + CODE).pes(CODE).take()
    rig = Rig(pkg, eng)
    rows = rig.cut(ts, [], shift=2)
    k = len(ts) - 2
    if fault == 'duplicate':
        assert codes(rows) == [GOP[:2] + (0,) + GOP[3:] + (10, k), GOP[:2] + (0,) + GOP[3:] + (21, k), GOP[:2] + (0,) + GOP[3:] + (29, k + 1)]
    else:
        assert codes(rows) == [GOP[:2] + (E.RESYNC,) + GOP[3:] + (21, k), GOP[:2] + (0,) + GOP[3:] + (29, k + 1)] and rig.models[0].stats()['resets'] == 1
    assert Rig(pkg, eng).cut(ts, range(1, len(ts)), shift=1) == rows


def test_back_to_back_codes_at_max_packets_with_a_short_table(pkg, eng):
    """46 codes per packet, 4096 packets, a table of 1000 rows: truncation, rows_dropped, and the counters cover all"""
    ln = K.Line(0x150).pes((K.SC + b'\xB8') * 4)
    for _ in range(4095):
        ln.put((K.SC + b'\xB8') * 46)
    ts = ln.take()
    rig = Rig(pkg, eng, 1, 4096, 1000)
    rows = rig.call([ts])[0]
    total = 1 + 3 + 4095 * 46                                        # (the last code of the call waits for its head)
    assert len(rows) == 1000 and rig.dv.stream_stats(0)['rows_dropped'] == total - 1000 and rig.models[0].stats()['gops'] == total - 1
    assert [r['es_offset'] for r in rows[1:5]] == [0, 4, 8, 12] and rows[4]['packet'] == 1 and rows[999]['head'] == 0x000001B8
    rows = rig.call([ts[1:300]], shift=3)[0]
    assert rows[0]['es_offset'] == 16 + 4095 * 184 and rows[0]['flags'] == E.RESYNC and rig.models[0].stats()['gops'] == total - 1 + 299 * 46 - 1


def test_sixteen_slots_reversed_three_streams_and_a_quiet_call_inside_a_window(pkg, eng):
    rng = np.random.default_rng(5)
    w16 = [(s, 0x100 + 3 * (15 - s), 1 + s % 3) for s in reversed(range(16))]
    sixteen = K.random_mux(rng, 1300, [(p, c) for _, p, c in w16])
    mux = K.gpu_mux()
    split = K.Line(0x150).pes(b'\x30' * 5 + CODE[:3]).put(CODE[3:] + b'\x37' * 5).take()
    rig = Rig(pkg, eng, 3, 1024, 4096, watches=[M2, w16, THREE])
    rig.call([split[:1], sixteen[:700], mux[:500]])
    rig.call([NONE, sixteen[700:], NONE], shift=1)                    # stream 0 brings nothing between two calls that share a window
    rows = rig.call([split[1:], NONE, mux[500:1500]], shift=2)
    assert codes(rows[0]) == [GOP[:2] + (0,) + GOP[3:] + (5, 0)] and rows[1] == []
    assert all(rig.models[1].stats(s)['codes'] > 10 for s in range(16)) and rig.dv.stream_stats(1)['packets'] == 1300


def _psi_es_mux(rng):
    """a multiplex with a PAT, two PMTs that name video PIDs 0x200 (H.264), 0x210 (MPEG-2) and 0x211 (H.265) and an audio PID 0x201, and
    PES packets on the four; PID 0x300 fills"""
    zp, zm = S.Packetiser(0), [S.Packetiser(0x100), S.Packetiser(0x101)]
    ts = K.random_mux(rng, 500, [(0x200, E.H264), (0x201, E.MPEG2), (0x210, E.MPEG2), (0x211, E.H265)], faults=False)
    spare = [k for k in range(500) if (int(ts[k, 1]) & 0x1f) << 8 | int(ts[k, 2]) in (0x300, 0x1FFF)]
    sections = [(zp, S.pat(5, [(0, 0x10), (1, 0x100), (2, 0x101)])), (zm[0], S.pmt(1, 0x200, [(0x1b, 0x200), (0x0f, 0x201), (0x05, 0x300)])),
                (zm[1], S.pmt(2, 0x210, [(0x02, 0x210), (0x24, 0x211)]))]
    for j, k in enumerate(spare[:18]):                               # the tables, six times each, in place of filler
        z, sec = sections[j % 3]
        ts[k] = z.lay([sec])[0]
    return ts


def _watch_from_pmts(pkg, eng, src, nbytes, max_packets):
    """a PsiBank reads the buffer twice (PAT, then PMTs); an EsBank and the model take their watches from it"""
    psi = pkg.PsiBank(eng, 1, max_packets, 64)
    psi.process([src], nbytes=[nbytes])
    assert psi.follow_pat(0) == []
    psi.process([src], nbytes=[nbytes])
    es, m = pkg.EsBank(eng, 1, max_packets, 2048), E.Es(2048)
    assert es.follow_pmts(psi, 0) == [] and es._watched[0] == {0: (0x200, E.H264), 1: (0x210, E.MPEG2), 2: (0x211, E.H265)}     # (audio and sections are skipped)
    for s, (pid, codec) in es._watched[0].items():
        m.set_watch(s, pid, codec)
    return es, m


def test_chained_behind_the_monitor_with_watches_from_the_pmts_and_beside_a_pes_bank(pkg, eng):
    """the monitor's filter output is the ES bank's input, its watches come from a PsiBank that read the same buffer, and a PesBank on
    the same buffer sees the same starts"""
    import torch
    mux = _psi_es_mux(np.random.default_rng(11))
    src = _dev(mux)
    es, m = _watch_from_pmts(pkg, eng, src[:mux.size], mux.size, 512)
    mon = pkg.TsMonitorBank(eng, 1, 512)
    mon.set_filter(0, mode=2, pids=[0x300], drop_null=True)         # the filter drops the filler: the positions change
    passed = torch.zeros(mux.size, dtype=torch.uint8, device='cuda')
    nb = mon.process([src[:mux.size]], [passed])[0]
    pid = (mux[:, 1].astype(int) & 0x1f) << 8 | mux[:, 2]
    kept = mux[(pid != 0x300) & (pid != 0x1FFF)]
    assert nb == kept.size and 0 < nb < mux.size
    assert es.process([passed], nbytes=[nb]) == [m.process(kept)]
    K.same(es, m)
    assert all(m.stats(s)['pictures'] > 3 for s in range(3)) and m.stats()['cc_errors'] == 0 and m.stats()['resets'] == 0
    pes = pkg.PesBank(eng, 1, 512, 2048)
    for s, (p, _) in es._watched[0].items():
        pes.set_watch(0, s, p)
    pes.process([passed], nbytes=[nb])
    mine = [(r['packet'], r['pts']) for r in es.rows(0) if r['unit'] == E.PES and r['detail'] == P.HEADER]
    assert mine == [(r['packet'], r['pts']) for r in pes.row_table(0) if r['kind'] == P.HEADER] and len(mine) > 20
    assert all(not r['flags'] & E.UNSYNCED for r in es.rows(0) if r['unit'] == E.PES)


def test_chained_behind_the_packetiser_in_hbm(pkg, eng):
    """the output buffer of a BbTsParserBank call is the ES bank's input, on the engine's stream: no host copy in between"""
    import torch
    mux = _psi_es_mux(np.random.default_rng(13))
    kbch, nfr = 14232, 16
    frames = B.bbframes_from_ts(mux, kbch, nfr)
    bank = pkg.BbTsParserBank(eng, 1, kbch, nfr)
    ts_dev = torch.zeros(nfr * kbch // 8 + 376, dtype=torch.uint8, device='cuda')
    nb = bank.process_batch([torch.from_numpy(frames.reshape(-1)).cuda()], [ts_dev])[0]
    assert nb % 188 == 0 and nb // 188 >= nfr * (kbch // 8 - 10) // 188 - 1
    es, m = _watch_from_pmts(pkg, eng, ts_dev, nb, 256)
    assert es.process([ts_dev], nbytes=[nb]) == [m.process(mux[:nb // 188])]
    K.same(es, m)
    assert m.stats()['pes_starts'] >= 8 and m.stats()['pictures'] >= 8 and m.stats()['cc_errors'] == 0
