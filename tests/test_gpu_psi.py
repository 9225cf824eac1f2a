"""GPU tests of the PSI section bank (csrc/psi.hip): the kernels against the library's host bank and the model of tests/psi_ref.py in
bytes, rows, counters and decoded views, at the packet counts, slot shapes and call boundaries where the compaction, the section
chains, the row numbering and the parallel CRC can go wrong."""
import numpy as np
import pytest

import orc_bbts as B
import psi_cases as K
import psi_ref as P

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

    def __init__(self, pkg, eng, nstreams, max_packets, max_sections=512, watches=None, deliver=None):
        import torch
        self.n = nstreams
        self.dv, self.hb = pkg.PsiBank(eng, nstreams, max_packets, max_sections), pkg.PsiBank.host(nstreams, max_packets, max_sections)
        self.models = [P.Assembler() for _ in range(nstreams)]
        self.outs = [torch.zeros(max_packets * 188 + 16 * 4096 + 8, dtype=torch.uint8, device='cuda') for _ in range(nstreams)]
        for i in range(nstreams):
            for slot, pid, expect in (watches[i] if watches else [(1, PID, -1)]):
                self.set_watch(i, slot, pid, expect)
            if deliver:
                self.dv.set_deliver(i, deliver[i]), self.hb.set_deliver(i, deliver[i])
                self.models[i].deliver = deliver[i]

    def set_watch(self, i, slot, pid, expect=-1):
        self.dv.set_watch(i, slot, pid, expect), self.hb.set_watch(i, slot, pid, expect), self.models[i].set_watch(slot, pid, expect)

    def call(self, per_stream, deliver=True, shift=0):
        ins = [_dev(ts, shift) for ts in per_stream]
        outs = [o[1 - shift:] for o in self.outs]     # an unaligned input with an aligned output, and the other way round
        nb = self.dv.process(ins, outs if deliver else None, nbytes=[ts.size for ts in per_stream])
        for i, ts in enumerate(per_stream):
            want = self.models[i].process(ts, deliver)
            host = self.hb.work(ts, stream=i, deliver=deliver)
            if deliver:
                assert nb[i] == want.size, (i, nb[i], want.size)
                assert np.array_equal(outs[i][:nb[i]].cpu().numpy(), want), i
                assert np.array_equal(host, want), i
            assert self.dv.section_table(i) == self.models[i].table == self.hb.section_table(i), i
            self.same_state(i)

    def same_state(self, i):
        m = self.models[i]
        for slot in range(-1, 16):
            assert self.dv.stats(i, slot) == m.stats(slot) == self.hb.stats(i, slot), (i, slot)
        assert self.dv.programs(i) == m.programs() == self.hb.programs(i), i
        for slot in range(16):
            assert self.dv.program_map(i, slot) == m.program_map(slot) == self.hb.program_map(i, slot), (i, slot)


def test_packet_counts_at_wave_and_workgroup_edges(pkg, eng):
    sizes = [0, 1, 2, 63, 64, 65, 255, 256, 257, 600]
    rng = np.random.default_rng(1)
    z, zp, parts = P.Packetiser(PID), P.Packetiser(0), []
    while sum(len(p) for p in parts) < sum(sizes):                 # sections of 1 to 8 packets: one crosses every boundary
        parts += [z.lay([K._sec(int(rng.integers(150, 1400)), int(rng.integers(0, 1 << 15)))], pointer=int(rng.integers(0, 3))),
                  P.filler(0x99, int(rng.integers(0, 3)), rng)]
        if rng.random() < 0.2:
            parts.append(zp.lay([P.pat(3, [(1, PID)], version=len(parts) // 40)]))
    ts = np.concatenate(parts)[:sum(sizes)]
    rig, rows_only = Rig(pkg, eng, 1, 600), Rig(pkg, eng, 1, 600)
    a, open_at_cut = 0, 0
    for k, s in enumerate(sizes):
        rig.call([ts[a:a + s]], shift=k % 2)
        rows_only.call([ts[a:a + s]], deliver=False)
        a += s
        open_at_cut += len(rig.models[0].slot[1]['buf']) > 0
    st = rig.models[0].stats()
    assert open_at_cut >= 6 and st['sections'] > 100 and st['crc_errors'] == 0 and st['dropped_sections'] == 0
    assert rows_only.models[0].stats()['bytes_delivered'] == 0


def test_constructed_edges_whole_and_cut_in_two(pkg, eng):
    cases = K.edge_cases()
    rig, cut = Rig(pkg, eng, 1, 64), Rig(pkg, eng, 1, 64)
    for k, (name, ts, multi) in enumerate(cases):
        rig.call([ts], shift=k % 2)
        if multi:
            cut.call([ts[:len(ts) // 2]]), cut.call([ts[len(ts) // 2:]], shift=1)
        else:
            cut.call([ts])
    assert rig.models[0].stats() == cut.models[0].stats() and rig.models[0].stats()['malformed_sections'] == 3
    one = Rig(pkg, eng, 1, 512)
    one.call([K.whole_stream(np.random.default_rng(2), cases)])    # and back to back with a PAT between them, in one call
    assert one.models[0].stats(0)['changed'] == 3


def test_walk_cases_whole_and_cut_at_every_packet(pkg, eng):
    """the branches of the shared walk (csrc/ts_reasm.h) that this format takes with its own header length, or alone: each case by
    itself on a fresh bank, in one call and cut in two at every packet boundary"""
    edges = {name: ts for name, ts, _ in K.edge_cases()}
    for name, ts, rows, counts in [(name, edges[name], None, None) for name in K.WALK_EDGES] + K.walk_cases():
        whole = None
        for at in range(len(ts)):                                  # 0: one call
            rig, got = Rig(pkg, eng, 1, 8, 16), []
            for k, part in enumerate([ts[:at], ts[at:]] if at else [ts]):
                rig.call([part], shift=(at + k) % 2)
                got += [(r['table_id'], r['length'], r['flags']) for r in rig.models[0].table]
            st = rig.models[0].stats(1)
            if at == 0:
                whole = (got, st)
                if rows is not None:
                    assert [(r['table_id'], r['length'], r['first_packet']) for r in rig.models[0].table] == rows, name
                    assert (st['dropped_sections'], st['malformed_sections']) == counts, name
            assert (got, st) == whole and not rig.models[0].slot[1]['buf'], (name, at)


def test_slot_shapes(pkg, eng):
    rng = np.random.default_rng(5)
    z = P.Packetiser(0x44)
    one = np.concatenate([z.lay([K._sec(int(n), 100 + i) for n in rng.integers(12, 400, 3)], pointer=0) for i in range(200)])[:500]
    pids = [0x100 + 3 * s for s in range(16)]
    zs = [P.Packetiser(p) for p in pids]
    lanes = [np.concatenate([zs[s].lay([K._sec(int(n), 200 + s)]) for n in rng.integers(100, 900, 12)])[:30] for s in range(16)]
    sixteen = np.stack(lanes, axis=1).reshape(-1, 188)             # packet by packet: slot 0, 1, ... 15, 0, ...
    rig = Rig(pkg, eng, 3, 512, 2048, watches=[[(0, 0x44, 0x42)], [(s, pids[s], -1) for s in range(16)], [(3, 0x55, -1), (9, 0x44, -1)]], deliver=[0, 1, 0])
    rig.call([one[:250], sixteen[:201], np.zeros((0, 188), np.uint8)])
    rig.call([one[250:], sixteen[201:], one[:100]], shift=1)       # stream 2: PID 0x55 never appears, 0x44 in slot 9
    assert rig.models[0].stats()['packets'] == 500 and rig.models[0].stats()['sections'] > 150
    assert all(rig.models[1].stats(s)['sections'] >= 3 for s in range(16))
    assert rig.models[2].stats(3)['packets'] == 0 and rig.models[2].stats(9)['sections'] > 20


def test_three_streams_with_an_empty_one_in_the_middle(pkg, eng):
    """an odd stream count: the three arrays of the argument table (input pointers, output pointers, byte counts) lie where the
    declared layout puts them, which for 3 streams is not where 3 x 8 and 3 x 16 bytes would; the empty stream has its output buffer"""
    zp = P.Packetiser(0)
    pats = [zp.lay([P.pat(7 + i, [(0, 0x10), (1, 0x100 + i)])]) for i in range(2)]
    rig = Rig(pkg, eng, 3, 8, 16, watches=[[(0, 0, 0)]] * 3)
    rig.call([pats[0], np.zeros((0, 188), np.uint8), pats[1]])
    assert [rig.models[i].stats()['changed'] for i in range(3)] == [1, 0, 1] and rig.models[1].stats()['packets'] == 0
    assert rig.dv.programs(0)[1] == [(0, 0x10), (1, 0x100)] and rig.dv.programs(1)[1] == [] and rig.dv.programs(2)[1] == [(0, 0x10), (1, 0x101)]


def test_a_call_with_only_the_tail_of_a_carried_section(pkg, eng):
    z = P.Packetiser(PID)
    ts = z.lay([K._sec(900, 77)])
    rig = Rig(pkg, eng, 1, 16)
    rig.call([ts[:2]])
    rig.call([ts[2:3]])                                            # still open: nothing but state moves
    assert rig.models[0].table == [] and len(rig.models[0].slot[1]['buf']) == 183 + 2 * 184
    rig.call([ts[3:]])                                             # no PUSI in the call
    assert [r['first_packet'] for r in rig.models[0].table] == [-1] and rig.models[0].stats(1)['valid'] == 1


def test_capacity_failure_leaves_every_stream_where_it_was(pkg, eng):
    import torch
    rng = np.random.default_rng(8)
    ts = K.whole_stream(rng)
    rig = Rig(pkg, eng, 3, 512, 256)
    rig.call([ts[:50], ts[:70], ts[:90]])
    rest = [ts[50:], ts[70:], ts[90:]]
    probes = []
    for i in range(3):
        m = P.Assembler()
        m.set_watch(1, PID)
        m.process(ts[:50 + 20 * i])
        probes.append((m.process(rest[i]).size, len(m.table)))
    before = [rig.dv.stats(i) for i in range(3)]
    ins = [_dev(t) for t in rest]
    cap = max(p[0] for p in probes) - 1                             # one byte short for the stream that needs most, room for the others
    assert sum(p[0] > cap for p in probes) == 1
    outs = [torch.zeros(cap, dtype=torch.uint8, device='cuda') for i in range(3)]
    with pytest.raises(pkg.Dvbs2GpuError) as e:
        rig.dv.process(ins, outs, nbytes=[t.size for t in rest])
    assert e.value.code == -5 and e.value.needed == [p[0] for p in probes] and e.value.rows == [p[1] for p in probes]
    assert [rig.dv.stats(i) for i in range(3)] == before and all(rig.dv.section_table(i) == [] for i in range(3))
    small = pkg.PsiBank(eng, 1, 512, probes[0][1] - 1)             # and one row short
    small.set_watch(0, 1, PID)
    small.process([_dev(ts[:50])], nbytes=[50 * 188])
    was = small.stats(0)
    with pytest.raises(pkg.Dvbs2GpuError) as e:
        small.process(ins[:1], outs[:1], nbytes=[rest[0].size])
    assert e.value.code == -5 and e.value.rows == [probes[0][1]] and e.value.needed == [-1] and small.stats(0) == was
    rig.call(rest)                                                 # the repeat, with room, equals the model


def test_two_launches_and_chained_behind_the_monitor(pkg, eng):
    """the monitor's pass list comes from follow_pat: the filter is configured from PSI with no packet on the host"""
    import torch
    rng = np.random.default_rng(11)
    pmt_pids = [0x100, 0x101]
    streams = [[(0x1b, 0x200), (0x0f, 0x201)], [(0x02, 0x210)]]
    zp, zm = P.Packetiser(0), [P.Packetiser(p) for p in pmt_pids]
    parts = []
    for r in range(6):
        parts += [zp.lay([P.pat(5, [(0, 0x10), (1, pmt_pids[0]), (2, pmt_pids[1])])]), P.filler(0x200, 20, rng, 20 * r), zm[0].lay([P.pmt(1, 0x200, streams[0])]),
                  P.filler(0x210, 15, rng, 15 * r), zm[1].lay([P.pmt(2, 0x210, streams[1])]), P.filler(0x201, 9, rng, 9 * r)]
    ts = np.concatenate(parts)
    src = _dev(ts)
    psi = pkg.PsiBank(eng, 1, 512, 64)
    k0 = eng.get_state('kernel_launches')
    psi.process([src[:100 * 188]])
    assert eng.get_state('kernel_launches') - k0 == 2
    assert psi.follow_pat(0) == [] and psi.programs(0)[1] == [(0, 0x10), (1, 0x100), (2, 0x101)]
    mon = pkg.TsMonitorBank(eng, 1, 512)
    mon.set_filter(0, mode=1, pids=[0] + pmt_pids)
    passed = torch.zeros(ts.size, dtype=torch.uint8, device='cuda')
    nb = mon.process([src[:ts.size]], [passed])[0]
    assert nb == 18 * 188
    psi.process([passed], nbytes=[nb])                             # the monitor's output tensor, straight in
    assert psi.program_map(0, 1) == (dict(program_number=1, version=0, pcr_pid=0x200, malformed=0), streams[0])
    assert psi.program_map(0, 2) == (dict(program_number=2, version=0, pcr_pid=0x210, malformed=0), streams[1])
    m = P.Assembler()
    m.process(ts[:100], deliver=False)                             # (the bank's calls had no output buffers: rows and counters only)
    m.set_watch(1, 0x100, 2), m.set_watch(2, 0x101, 2)
    m.process(ts[np.isin((ts[:, 1].astype(int) & 0x1f) << 8 | ts[:, 2], [0] + pmt_pids)], deliver=False)
    assert psi.section_table(0) == m.table and psi.stats(0) == m.stats() and m.stats()['changed'] == 3 and m.stats()['unexpected_table_id'] == 0     # the PAT once, in the first call; each PMT once
    p, rows = psi.section_table_device(0)
    assert p and rows == len(m.table)


def test_chained_behind_the_packetiser_in_hbm(pkg, eng):
    """the output buffer of a BbTsParserBank call is the section bank's input, on the engine's stream: no host copy in between"""
    import torch
    rng = np.random.default_rng(13)
    zp, z1, z2 = P.Packetiser(0), P.Packetiser(0x100), P.Packetiser(K.PID)
    streams = [(0x1b, 0x200), (0x0f, 0x201)]
    parts = []
    for r in range(8):
        parts += [zp.lay([P.pat(5, [(0, 0x10), (1, 0x100)], version=r // 4)]), P.filler(0x200, 9, rng, 9 * r), z1.lay([P.pmt(1, 0x200, streams, program_info=bytes(200))]),
                  z2.lay([K._sec(int(rng.integers(100, 900)), 300 + r)], pointer=r % 3), P.filler(0x201, 4, rng, 4 * r)]
    mux = np.concatenate(parts)
    kbch, nfr = 14232, 16
    frames = B.bbframes_from_ts(mux, kbch, nfr)
    bank = pkg.BbTsParserBank(eng, 1, kbch, nfr)
    ts_dev = torch.zeros(nfr * kbch // 8 + 376, dtype=torch.uint8, device='cuda')
    nb = bank.process_batch([torch.from_numpy(frames.reshape(-1)).cuda()], [ts_dev])[0]
    assert nb % 188 == 0 and nb // 188 >= nfr * (kbch // 8 - 10) // 188 - 1
    psi, m = pkg.PsiBank(eng, 1, 256, 64), P.Assembler()
    for slot, pid, expect in ((1, 0x100, 2), (2, K.PID, -1)):
        psi.set_watch(0, slot, pid, expect), m.set_watch(slot, pid, expect)
    out = torch.zeros(1 << 16, dtype=torch.uint8, device='cuda')
    got = psi.process([ts_dev], [out], nbytes=[nb])[0]
    want = m.process(mux[:nb // 188])
    assert got == want.size and np.array_equal(out[:got].cpu().numpy(), want)
    assert psi.section_table(0) == m.table and psi.stats(0) == m.stats()
    assert m.stats(0)['changed'] == 2 and m.stats(1)['changed'] == 1 and m.stats(2)['sections'] >= 6 and m.stats()['crc_errors'] == 0
    assert psi.programs(0) == m.programs() and psi.program_map(0, 1) == m.program_map(1) == (dict(program_number=1, version=0, pcr_pid=0x200, malformed=0), streams)
