"""GPU tests of the audio bank (csrc/aud.hip): the kernel against the library's host bank and the model of tests/aud_ref.py in rows,
counters and state (through the next call), with one launch per call, at the packet counts, slot shapes, call boundaries, alignments,
payload lengths, window splits and chain shapes where the compaction, the sort by slot, the prefix sums, the speculative walks, the
join of the slots' chains and the unaligned reads can go wrong."""
import numpy as np
import pytest

import aud_cases as K
import aud_ref as A
import pes_ref as P
import psi_ref as S

pytestmark = pytest.mark.gpu
NONE = np.zeros((0, 188), np.uint8)
ADTS = [(0, 0x161, A.ADTS)]
RNG = np.random.default_rng(77)
F60, F40, F50, F33 = (K.adts_frame(RNG, n) for n in (60, 40, 50, 33))          # ADTS frames full of false sync words


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
        self.dv, self.hb = pkg.AudBank(eng, nstreams, max_packets, max_rows), pkg.AudBank.host(nstreams, max_packets, max_rows)
        self.models = [A.Aud(max_rows) for _ in range(nstreams)]
        for i in range(nstreams):
            for slot, pid, codec in (watches[i] if watches else ADTS):
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


def frames(rows):
    """the FRAME and LOSS rows as (unit, flags, es_offset, frame_bytes, packet)"""
    return [(r['unit'], r['flags'], r['es_offset'], r['frame_bytes'], r['packet']) for r in rows if r['unit'] != A.PES]


def test_packet_counts_at_wave_workgroup_and_thread_run_edges(pkg, eng):
    mux = K.mux()                                                     # (tests/test_aud_cpu.py: what it yields)
    rig = Rig(pkg, eng, 1, 600, 8192, watches=[K.WATCHES])
    a = 0
    for k, s in enumerate([0, 1, 63, 64, 65, 255, 256, 257, 512, 513]):      # 512 / 513: two and three packets per thread
        rig.call([mux[a:a + s]], shift=k % 4)
        a += s
    st = rig.models[0].stats()
    assert st['frames'] > 200 and st['resets'] > 50 and st['sync_losses'] >= 3 and rig.dv.stream_stats(0) == dict(packets=a, rows_dropped=0)


def test_the_faulty_multiplex_whole_and_cut_on_three_streams_and_an_empty_one(pkg, eng):
    mux = K.mux()
    rig = Rig(pkg, eng, 4, 2600, 8192, watches=[K.WATCHES] * 4)
    cuts = [[0, 2600], [0, 1, 38, 900, 2600], [0, 2600], list(range(0, 2600, 650)) + [2600]]
    for c in range(4):
        part = lambda i: mux[cuts[i][c]:cuts[i][c + 1]] if c + 1 < len(cuts[i]) and i != 2 else NONE        # stream 2 never brings a byte
        rig.call([part(i) for i in range(4)], shift=c)
    whole = rig.models[0].stats()
    assert whole['frames'] > 200 and rig.models[1].stats() == whole == rig.models[3].stats() and rig.dv.stats(2)['packets'] == 0


@pytest.mark.parametrize('c', range(1, 8))
def test_one_header_split_at_each_inner_position(pkg, eng, c):
    """the 8 bytes that decide the second frame, c of them in front of the split: between two packets, between two calls, and across a
    valid PES start whose header lies between its bytes (an unaligned start)"""
    es = F60 + F40 + F50 + F33[:8]
    want = [(A.FRAME, A.ACQUIRED, 0, 60, 0), (A.FRAME, 0, 60, 40, 1), (A.FRAME, 0, 100, 50, 1), (A.FRAME, 0, 150, 33, 1)]
    ts = K.Line(0x161).pes(es, sizes=[14 + 60 + c]).take()
    assert frames(Rig(pkg, eng).cut(ts, [], shift=c % 4)) == want
    assert frames(Rig(pkg, eng).cut(ts, [1], shift=(c + 1) % 4)) == want
    ts = K.Line(0x161).pes(es[:60 + c]).pes(es[60 + c:], stuffing=c % 3).take()
    rig = Rig(pkg, eng)
    rows = rig.cut(ts, [], shift=c % 4)
    assert frames(rows) == want and [r['es_offset'] for r in rows if r['unit'] == A.PES] == [0, 60 + c] and rig.models[0].stats()['unaligned_starts'] == 1
    assert Rig(pkg, eng).cut(ts, [1]) == rows


def test_one_header_over_eight_packets_of_one_byte(pkg, eng):
    """adaptation_field_length 182 leaves one payload byte: a header's 8 bytes lie in 8 packets, with a duplicate, a packet without
    payload and packets of other PIDs between them; whole, and cut into calls at every packet"""
    ln = K.Line(0x161).pes(F60)
    for i, b in enumerate(F40[:8]):
        ln.put(bytes([b]))
        if i == 2:
            ln.again()
        if i == 4:
            ln.no_payload()
        if i == 5:
            ln.out.append(P.null_packets(1)[0])
            ln.out.append(P.ts_packet(0x162, 3, F40))
    ts = ln.put(F40[8:] + F50[:8]).take()
    want = [(A.FRAME, A.ACQUIRED, 0, 60, 0), (A.FRAME, 0, 60, 40, 12), (A.FRAME, 0, 100, 50, 13)]
    for shift in range(4):
        assert frames(Rig(pkg, eng).cut(ts, [], shift)) == want
    assert frames(Rig(pkg, eng).cut(ts, range(1, len(ts)))) == want
    assert frames(Rig(pkg, eng).cut(ts, range(2, len(ts), 3), shift=3)) == want


def test_next_on_a_segments_first_byte_its_last_byte_and_behind_the_calls_end(pkg, eng):
    big = K.adts_frame(RNG, 367)                                      # from the first byte of packet 1 to the last but one of packet 2
    ln = K.Line(0x161).pes(K.adts_frame(RNG, 170) + big + F40 + F60 + F50 + F33[:8], sizes=[184, 184, 184])   # PES header of 14 bytes: 170 ES bytes in packet 0
    ts = ln.take()
    assert len(ts) == 4
    want = [(A.FRAME, A.ACQUIRED, 0, 170, 0), (A.FRAME, 0, 170, 367, 1), (A.FRAME, 0, 537, 40, 3), (A.FRAME, 0, 577, 60, 3), (A.FRAME, 0, 637, 50, 3), (A.FRAME, 0, 687, 33, 3)]
    assert frames(Rig(pkg, eng).cut(ts, [])) == want                  # 170: the first byte of packet 1; 537: the last byte of packet 2
    for edges in ([1], [2], [3], [1, 2, 3]):                          # cut at 1: next (170) is the byte behind the call's end; at 3: next (537) its last byte
        assert frames(Rig(pkg, eng).cut(ts, edges, shift=len(edges))) == want, edges
    ts = K.Line(0x161).pes(K.adts_frame(RNG, 170)).pes(F40 + F60[:8]).take()        # aligned: next is the byte behind the call's end at a PES boundary
    assert frames(Rig(pkg, eng).cut(ts, [1])) == [(A.FRAME, A.ACQUIRED, 0, 170, 0), (A.FRAME, 0, 170, 40, 1), (A.FRAME, 0, 210, 60, 1)]


def test_next_carried_over_fifty_calls_of_one_packet(pkg, eng):
    es = K.adts_frame(RNG, 8191) + F40 + F60 + K.adts_frame(RNG, 1200)[:900]
    ts = K.Line(0x161).pes(es).take()
    assert len(ts) == 51
    rig = Rig(pkg, eng)
    rows = rig.cut(ts, range(1, 51))
    assert frames(rows) == [(A.FRAME, A.ACQUIRED, 0, 8191, 0), (A.FRAME, 0, 8191, 40, 44), (A.FRAME, 0, 8231, 60, 44), (A.FRAME, 0, 8291, 1200, 45)]
    assert frames(Rig(pkg, eng, 1, 64).cut(ts, [], shift=1)) == frames(rows)


def test_seven_byte_frames_give_twenty_seven_rows_in_a_packet(pkg, eng):
    tiny = K.adts_header(7)
    ts = K.Line(0x161).pes(tiny * 400, sizes=[14 + 3]).take()
    rig = Rig(pkg, eng)
    rows = rig.cut(ts, [], shift=3)
    per_packet = np.bincount([r['packet'] for r in rows if r['unit'] == A.FRAME])
    assert per_packet.max() == 27 and rig.models[0].stats()['frames'] == 399 and [r['es_offset'] for r in rows[1:4]] == [0, 7, 14]
    assert Rig(pkg, eng).cut(ts, [3, 4, 9]) == rows


def _aligned_then_unaligned(fault):
    """aligned PES packets; a fault; PES packets cut inside frames, the first of which begins with a frame"""
    rng = np.random.default_rng(12)
    fr = [K.adts_frame(rng, int(n)) for n in rng.integers(30, 500, 40)]
    ln = K.Line(0x161)
    for i in range(0, 12, 3):
        ln.pes(b''.join(fr[i:i + 3]))
    fault(ln)
    es, at = b''.join(fr[12:]), 0
    for size in [333, 512, 77, 1000, 5, 640, 2000]:
        ln.pes(es[at:at + size])
        at += size
    return ln.take()


def test_an_aligned_stream_an_unaligned_one_and_a_change_between_them_at_a_cc_error(pkg, eng):
    ts = _aligned_then_unaligned(lambda ln: ln.lose())
    rig = Rig(pkg, eng, 1, 128)
    rows = rig.cut(ts, [], shift=1)
    st = rig.models[0].stats()
    assert (st['acquisitions'], st['unaligned_starts'], st['sync_losses'], st['cc_errors']) == (2, 6, 0, 1) and st['frames'] > 20
    assert sum(r['flags'] == A.ACQUIRED for r in rows) == 2 and [r['packet'] for r in rows if r['flags'] & A.RESYNC] == [[r['packet'] for r in rows if r['unit'] == A.PES][4]]
    assert Rig(pkg, eng, 1, 128).cut(ts, range(5, len(ts), 5), shift=2) == rows
    ts = _aligned_then_unaligned(lambda ln: None)                     # without the fault the chain goes on: one acquisition
    rig = Rig(pkg, eng, 1, 128)
    rig.cut(ts, [], shift=3)
    assert (rig.models[0].stats()['acquisitions'], rig.models[0].stats()['unaligned_starts'], rig.models[0].stats()['resets']) == (1, 6, 0)


def test_a_loss_inside_a_pes_packet_a_reacquisition_and_a_loss_at_an_acquisition(pkg, eng):
    bad = bytes([F50[0], F50[1] ^ 0x06]) + F50[2:]                    # layer bits set
    ts = K.Line(0x161).pes(F60 + bad + F40 + F33).pes(F40 + F33).pes(bad + F60).pes(F60 + F40[:8]).take()
    rig = Rig(pkg, eng)
    rows = rig.cut(ts, [], shift=2)
    assert frames(rows) == [(A.FRAME, A.ACQUIRED, 0, 60, 0), (A.LOSS, 0, 60, 0, 0), (A.FRAME, A.ACQUIRED, 183, 40, 2), (A.FRAME, 0, 223, 33, 2),
                            (A.LOSS, 0, 256, 0, 3), (A.FRAME, A.ACQUIRED, 366, 60, 4), (A.FRAME, 0, 426, 40, 4)]
    st = rig.models[0].stats()
    assert (st['acquisitions'], st['sync_losses'], st['bytes_unlocked']) == (3, 2, 183 - 68 + 366 - 264)
    for edges in ([1], [2], [3], [1, 2, 3, 4]):
        assert Rig(pkg, eng).cut(ts, edges) == rows


def test_pes_packets_without_an_es_byte_before_and_between_the_frames(pkg, eng):
    """a start whose segment is empty keeps a pending acquisition, or continues the chain without a frame of its own: the parameters in
    front of the next frame lie three starts back"""
    mono = K.adts_frame(RNG, 50, chan=1)
    ts = K.Line(0x161).pes(b'').pes(b'').pes(F60 + F40).pes(b'').pes(b'').pes(mono + F33[:8]).take()
    assert len(ts) == 6
    rig = Rig(pkg, eng)
    rows = rig.cut(ts, [], shift=1)
    assert frames(rows) == [(A.FRAME, A.ACQUIRED, 0, 60, 2), (A.FRAME, 0, 60, 40, 2), (A.FRAME, A.CHANGE, 100, 50, 5), (A.FRAME, A.CHANGE, 150, 33, 5)]
    st = rig.models[0].stats()
    assert (st['acquisitions'], st['unaligned_starts'], st['pes_starts'], st['param_changes']) == (1, 0, 6, 2)
    for edges in ([3], [4], [5], range(1, 6)):
        assert Rig(pkg, eng).cut(ts, edges) == rows


@pytest.mark.parametrize('fault', ['duplicate', 'lost', 'di', 'scrambled', 'malformed'])
def test_a_fault_in_the_middle_of_a_frame(pkg, eng, fault):
    """a duplicate changes nothing; any other fault unlocks without a row, and the next start acquires with RESYNC"""
    big, g50 = K.adts_frame(RNG, 700, body=b'\x55'), K.adts_frame(RNG, 50, body=b'\x55')     # (a body that is no header: the LOSS rows below are certain)
    ln = K.Line(0x161).pes(F60 + big[:300], sizes=[100])
    if fault == 'duplicate':
        ln.again()
    if fault == 'lost':
        ln.lose()
    if fault == 'di':
        ln.no_payload(di=1)
    if fault == 'scrambled':
        ln.put(b'\x5A' * 184, tsc=1)
    if fault == 'malformed':
        ln.out.append(P.ts_packet(0x161, ln.cc, b'', af_len=183, afc=3))
        ln.cc += 1
    ts = ln.pes(big[300:] + F40 + F33[:8]).pes(g50 + F33[:8]).take()
    rig = Rig(pkg, eng)
    rows = rig.cut(ts, [], shift=2)
    st = rig.models[0].stats()
    if fault == 'duplicate':
        assert [f[:4] for f in frames(rows)] == [(A.FRAME, A.ACQUIRED, 0, 60), (A.FRAME, 0, 60, 700), (A.FRAME, 0, 760, 40), (A.FRAME, 0, 800, 33), (A.LOSS, 0, 833, 0)]
        assert (st['duplicates'], st['acquisitions'], st['unaligned_starts']) == (1, 1, 2)
    else:
        assert st['resets'] == 1 and st['acquisitions'] == 3 and st['sync_losses'] == 1 and frames(rows)[2][:3] == (A.LOSS, A.ACQUIRED, 360)
        assert frames(rows)[3:] == [(A.FRAME, A.ACQUIRED, 808, 50, len(ts) - 1), (A.FRAME, 0, 858, 33, len(ts) - 1)]
        assert [r['flags'] & A.RESYNC for r in rows if r['unit'] == A.PES] == [0, A.RESYNC, 0]
    assert Rig(pkg, eng).cut(ts, range(1, len(ts)), shift=1) == rows


def test_an_invalid_start_a_split_header_filler_and_a_bitrate_switch(pkg, eng):
    rng = np.random.default_rng(9)
    m1 = [K.mpa_frame(rng, bri=10, sri=1, pad=i & 1) for i in range(4)]
    m2 = [K.mpa_frame(rng, bri=12, sri=1) for i in range(3)]
    ln = K.Line(0x160).pes(b''.join(m1)).pes(b''.join(m2))
    ln.put(K.head(ln.pts, stream_id=0xC0, start=b'\x00\x01\x01') + m1[0][:100], pusi=1).put(m1[1][:184])         # BAD_START: unsynced, not scanned
    ln.put(K.head(ln.pts, stream_id=0xC0, stuffing=6)[:16], pusi=1).put(b'\xFF' * 4 + m1[0][:180])         # 9 + 11 > 16: split
    ts = ln.pes(m1[0] + m2[0] + m1[1][:8]).take()
    rig = Rig(pkg, eng, 1, 64, watches=[[(2, 0x160, A.MPA)]])
    rows = rig.cut(ts, [], shift=1)
    fl = [r['flags'] for r in rows if r['unit'] == A.FRAME]
    assert fl == [A.ACQUIRED, 0, 0, 0, A.CHANGE, 0, 0, A.ACQUIRED, A.CHANGE, A.CHANGE]       # (the filler's FF FB 90 00 words give no row)
    assert [r['flags'] for r in rows if r['unit'] == A.PES] == [0, 0, A.UNSYNCED, A.UNSYNCED | A.SPLIT_HEADER | A.RESYNC, A.RESYNC]
    st = rig.models[0].stats()
    assert (st['frames'], st['param_changes'], st['pes_invalid'], st['split_headers'], st['sync_losses'], st['bytes_unsynced']) == (10, 3, 2, 1, 0, 368)
    assert Rig(pkg, eng, 1, 64, watches=[[(2, 0x160, A.MPA)]]).cut(ts, range(1, len(ts), 2)) == rows


def test_sixteen_slots_of_the_three_codecs_and_a_short_table(pkg, eng):
    rng = np.random.default_rng(5)
    w16 = [(s, 0x100 + 3 * (15 - s), 1 + s % 3) for s in reversed(range(16))]
    ts = K.random_mux(rng, 1300, [(p, c) for _, p, c in w16], unaligned=(0x100, 0x103))
    rig = Rig(pkg, eng, 2, 1024, 4096, watches=[w16, w16])
    rig.call([ts[:700], ts[:300]])
    rig.call([ts[700:], ts[300:]], shift=1)
    assert all(rig.models[0].stats(s)['frames'] > 0 for s in range(16)) and rig.models[0].stats()['frames'] > 200 and rig.models[0].stats() == rig.models[1].stats()
    small = Rig(pkg, eng, 1, 1300, 100, watches=[w16])
    total = small.call([ts], shift=3)
    assert len(total[0]) == 100 and small.dv.stream_stats(0)['rows_dropped'] == small.models[0].nrows - 100 > 200 and small.models[0].stats() == rig.models[0].stats()


@pytest.mark.parametrize('shift', range(4))
def test_every_adaptation_field_length_on_a_start_and_inside_a_chain(pkg, eng, shift):
    """payload offsets 4 and 5..187: the start's header read and the frame header reads cross every phase, at input pointers 0..3"""
    rng = np.random.default_rng(6)
    es = b''.join(K.adts_frame(rng, int(n)) for n in rng.integers(7, 90, 1600))
    ln, at = K.Line(0x161), 0
    for L in range(184, 0, -1):
        data = K.head(ln.pts + 3600 * L, stream_id=0xC0, stuffing=L % 3) + es[at:at + 184]
        ln.put(data[:L], pusi=1)                                     # a start of L payload bytes: short of its header, or with the first ES bytes
        at += max(0, L - 14 - L % 3)
        ln.put(es[at:at + 184]).put(es[at + 184:at + 184 + L])       # a full packet, and one of L bytes
        at += 184 + L
    ts = ln.take()
    rig = Rig(pkg, eng, 1, 600)
    rig.call([ts], shift)
    st = rig.models[0].stats()
    assert st['frames'] > 700 and st['pes_invalid'] >= 13 and st['pes_starts'] == 184 and st['unaligned_starts'] > 100 and st['acquisitions'] >= 1


def _psi_aud_mux(rng):
    """a multiplex with a PAT, a PMT that names an MPEG audio PID 0x201 (type 0x03), an ADTS PID 0x202 (0x0F), an AC-3 PID 0x203 (0x81),
    a video PID 0x200 (0x1B) and a private PES PID 0x204 (0x06), and PES packets of audio frames on the five; PID 0x300 fills"""
    ts = K.random_mux(rng, 500, [(0x201, A.MPA), (0x202, A.ADTS), (0x203, A.AC3), (0x200, A.ADTS), (0x204, A.AC3)], faults=False)
    spare = [k for k in range(500) if (int(ts[k, 1]) & 0x1f) << 8 | int(ts[k, 2]) in (0x300, 0x1FFF)]
    zp, zm = S.Packetiser(0), S.Packetiser(0x100)
    sections = [(zp, S.pat(5, [(0, 0x10), (1, 0x100)])), (zm, S.pmt(1, 0x200, [(0x1b, 0x200), (0x03, 0x201), (0x0f, 0x202), (0x81, 0x203), (0x06, 0x204)]))]
    for j, k in enumerate(spare[:12]):                               # the tables, six times each, in place of filler
        z, sec = sections[j % 2]
        ts[k] = z.lay([sec])[0]
    return ts


def test_chained_behind_the_monitor_with_watches_from_the_pmt(pkg, eng):
    """the monitor's filter output is the audio bank's input, its watches come from a PsiBank that read the same buffer: stream types
    0x03, 0x0F and 0x81 are followed, video (0x1B) and private PES (0x06) are not"""
    import torch
    mux = _psi_aud_mux(np.random.default_rng(11))
    src = _dev(mux)
    psi = pkg.PsiBank(eng, 1, 512, 64)
    psi.process([src[:mux.size]], nbytes=[mux.size])
    assert psi.follow_pat(0) == []
    psi.process([src[:mux.size]], nbytes=[mux.size])
    aud, m = pkg.AudBank(eng, 1, 512, 2048), A.Aud(2048)
    assert aud.follow_pmts(psi, 0) == [] and aud._watched[0] == {0: (0x201, A.MPA), 1: (0x202, A.ADTS), 2: (0x203, A.AC3)}
    for s, (pid, codec) in aud._watched[0].items():
        m.set_watch(s, pid, codec)
    mon = pkg.TsMonitorBank(eng, 1, 512)
    mon.set_filter(0, mode=2, pids=[0x300], drop_null=True)         # the filter drops the filler: the positions change
    passed = torch.zeros(mux.size, dtype=torch.uint8, device='cuda')
    nb = mon.process([src[:mux.size]], [passed])[0]
    pid = (mux[:, 1].astype(int) & 0x1f) << 8 | mux[:, 2]
    kept = mux[(pid != 0x300) & (pid != 0x1FFF)]
    assert nb == kept.size and 0 < nb < mux.size
    assert aud.process([passed], nbytes=[nb]) == [m.process(kept)]
    K.same(aud, m)
    assert all(m.stats(s)['frames'] > 10 for s in range(3)) and m.stats()['sync_losses'] == 0 and m.stats()['resets'] == 0 and m.stats()['acquisitions'] == 3
    assert {r['pid'] for r in aud.rows(0)} == {0x201, 0x202, 0x203}
