"""GPU tests of the T2-MI bank (csrc/t2mi.hip): the kernels against the library's host bank and the model of tests/t2mi_ref.py in bytes,
rows, counters, frame sizes and state through the next call, at the packet counts, packet sizes, header placements, pointer cases and
slot shapes where the compaction, the header chains, the row numbering, the chunked CRC and the piecewise copy can go wrong; and
chained on the device in front of the mode-adaptation packetiser."""
import numpy as np
import pytest

import ma_ref as M
import psi_ref as S
import t2mi_cases as K
import t2mi_ref as T

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
    """a device bank, a host bank and one model per stream, fed the same calls.  watches[i]: [(slot, pid, plp)]"""

    def __init__(self, pkg, eng, nstreams, max_packets, max_rows=512, watches=None):
        import torch
        self.eng, self.n = eng, nstreams
        self.dv, self.hb = pkg.T2miBank(eng, nstreams, max_packets, max_rows), pkg.T2miBank.host(nstreams, max_packets, max_rows)
        self.models = [T.T2mi() for _ in range(nstreams)]
        self.used = [[False] * 4 for _ in range(nstreams)]
        self.outs = [[torch.zeros(max_packets * 188 + 8, dtype=torch.uint8, device='cuda') for _ in range(4)] for _ in range(nstreams)]
        for i in range(nstreams):
            for slot, pid, plp in (watches[i] if watches else [(0, PID, -1)]):
                self.dv.set_watch(i, slot, pid, plp), self.hb.set_watch(i, slot, pid, plp), self.models[i].set_watch(slot, pid, plp)
                self.used[i][slot] = pid >= 0

    def call(self, per_stream, deliver=True, shift=0):
        ins = [_dev(ts, shift) for ts in per_stream]
        # an unaligned input with an aligned output, and the other way round; an empty slot has no buffer
        outs = [[o[(1 - shift) & 3:] if self.used[i][k] else None for k, o in enumerate(per)] for i, per in enumerate(self.outs)]
        k0 = self.eng.get_state('kernel_launches')
        nb = self.dv.process(ins, outs if deliver else None, nbytes=[ts.size for ts in per_stream])
        assert self.eng.get_state('kernel_launches') - k0 == 2       # whatever the bank size
        for i, ts in enumerate(per_stream):
            want = self.models[i].process(ts, deliver)
            for k in range(4):
                host = self.hb.work(ts, stream=i, slot=k, deliver=deliver)
                if deliver:
                    assert nb[i][k] == want[k].size, (i, k, nb[i][k], want[k].size)
                    if self.used[i][k]:
                        assert np.array_equal(outs[i][k][:nb[i][k]].cpu().numpy(), want[k]), (i, k)
                    assert np.array_equal(host, want[k]), (i, k)
                assert self.dv.row_table(i, k) == self.models[i].table(k) == self.hb.row_table(i, k), (i, k)
                assert self.dv.frame_bytes(i, k) == self.models[i].frame_bytes(k) == self.hb.frame_bytes(i, k), (i, k)
                assert self.dv.stats(i, k) == self.models[i].stats(k) == self.hb.stats(i, k), (i, k)
            assert self.dv.stats(i) == self.models[i].stats(), i


def feed(rng, pid, n_packets, sizes, plps=(3, 5), cc=0):
    """n_packets TS packets of a T2-MI feed: BBFRAMEs of the given sizes on the PLPs in turn, an L1-type or timestamp-type packet now and then"""
    z, parts, count, got = T.Packetiser(pid, cc), [], int(rng.integers(256)), 0
    while got < n_packets:
        pk = []
        for _ in range(4):
            count = (count + 1) & 255
            if rng.random() < 0.25:
                pk.append(T.t2mi_packet(int(rng.choice([0x10, 0x20])), count, bytes(rng.integers(0, 256, int(rng.integers(0, 30)), dtype=np.uint8))))
            else:
                pk.append(T.bb_packet(count, plps[count % len(plps)], bytes(rng.integers(0, 256, int(rng.choice(sizes)), dtype=np.uint8)), frame_idx=count))
        parts.append(z.lay(pk, flush=rng.random() < 0.3))
        got += len(parts[-1])
    return np.concatenate(parts)[:n_packets]


def test_packet_counts_at_wave_and_workgroup_edges(pkg, eng):
    sizes = [0, 1, 63, 64, 65, 255, 256, 257, 4095, 4096]
    rng = np.random.default_rng(1)
    ts = feed(rng, PID, sum(sizes), [10, 40, 150, 700, 2500, 6500])
    ts[5000, 100] ^= 4                                               # and one bit error in the long calls
    rig = Rig(pkg, eng, 1, 4096, 2048, watches=[[(0, PID, -1), (2, PID, 3)]])
    rows_only = Rig(pkg, eng, 1, 4096, 2048)
    a, open_at_cut = 0, 0
    for k, s in enumerate(sizes):
        rig.call([ts[a:a + s]], shift=k % 4)
        if s < 4095:
            rows_only.call([ts[a:a + s]], deliver=False)
        a += s
        open_at_cut += len(rig.models[0].slot[0].buf) > 0
    st = rig.models[0].stats(0)
    assert open_at_cut >= 6 and st['t2mi_packets'] > 1000 and st['crc_errors'] == 1 and st['dropped_packets'] == 0 and st['count_errors'] == 1
    assert 0 < rig.models[0].stats(2)['bytes_delivered'] < st['bytes_delivered']
    assert rows_only.models[0].stats()['bytes_delivered'] == 0 and rows_only.models[0].stats()['bbframes'] > 0


def test_constructed_cases_whole_and_cut_in_two(pkg, eng):
    """the header splits after 1 to 5 bytes fall on a TS packet's end in `rig` and on a call's end in `cut`"""
    cases = K.edge_cases()
    rig, cut = Rig(pkg, eng, 1, 64), Rig(pkg, eng, 1, 64)
    for k, (name, ts) in enumerate(cases):
        rig.call([ts], shift=k % 4)
        assert [tuple(r[f] for f in K.ROW_FIELDS) for r in rig.models[0].table(0)] == K.ROWS[name], name
        if len(ts) > 1:
            cut.call([ts[:len(ts) // 2]], shift=(k + 1) % 4), cut.call([ts[len(ts) // 2:]], shift=(k + 2) % 4)
        else:
            cut.call([ts])
    assert rig.models[0].stats() == cut.models[0].stats() and rig.models[0].stats()['pointer_slack'] == 1
    one = Rig(pkg, eng, 1, 512, watches=[[(0, PID, -1), (1, PID, 2)]])
    one.call([K.whole_stream(cases=cases)])                          # and back to back in one call, beside a slot that takes PLP 2 alone
    assert one.models[0].stats(0) == rig.models[0].stats(0) and one.models[0].stats(1)['bbframes_delivered'] == 11


def test_walk_cases_whole_and_cut_at_every_packet(pkg, eng):
    """the branches of the shared walk (csrc/ts_reasm.h) that this format takes with its own header length, or alone: each case by
    itself on a fresh bank, in one call and cut in two at every TS packet boundary"""
    edges = dict(K.edge_cases())
    key = lambda r: tuple(r[f] for f in K.ROW_FIELDS[:8])          # (all but first_packet and last_packet, which count from the call's start)
    for name, ts, rows, dropped in [(name, edges[name], None, None) for name in K.WALK_EDGES] + K.walk_cases():
        whole = None
        for at in range(len(ts)):                                  # 0: one call
            rig, got, off = Rig(pkg, eng, 1, 8, 32), [], 0
            for k, part in enumerate([ts[:at], ts[at:]] if at else [ts]):
                rig.call([part], shift=(at + k) % 4)
                got += [key(dict(r, offset=r['offset'] + off if r['offset'] >= 0 else -1)) for r in rig.models[0].table(0)]
                off += sum(rig.models[0].frame_bytes(0))
            st = rig.models[0].stats(0)
            if at == 0:
                whole = (got, st)
                if rows is not None:
                    assert [tuple(r[f] for f in K.ROW_FIELDS) for r in rig.models[0].table(0)] == rows and st['dropped_packets'] == dropped, name
            assert (got, st) == whole and not rig.models[0].slot[0].buf, (name, at)


def test_packets_carried_over_two_and_three_calls(pkg, eng):
    cases = dict(K.edge_cases())
    big, bb = cases['payload_bits 65535: 8202 bytes over 45 TS packets'], cases['BBFRAME of 7274 bytes']
    rig = Rig(pkg, eng, 1, 64)
    for a in (0, 15, 30):
        rig.call([big[a:a + 15]], shift=a % 4)                       # three calls; the first two move nothing but state
        assert len(rig.models[0].table(0)) == (a == 30)
    assert rig.models[0].table(0)[0]['first_packet'] == -1 and rig.models[0].table(0)[0]['last_packet'] == 14
    rig.call([bb[:39]]), rig.call([bb[39:]], shift=3)                # two calls; the last brings one TS packet
    assert rig.models[0].stats()['bytes_delivered'] == 7274 and rig.models[0].stats()['crc_errors'] == 0
    for h in (1, 2, 3, 4, 5):                                        # an open header of h bytes through an EMPTY call and on
        ts = cases['header split after %d bytes' % h]
        rig.call([ts[:1]]), rig.call([NONE]), rig.call([ts[1:]], shift=h % 4)
        assert rig.models[0].table(0)[0]['first_packet'] == -1 and rig.models[0].table(0)[0]['bbframe_bytes'] == 40 + h


def test_slot_shapes(pkg, eng):
    rng = np.random.default_rng(5)
    pids = [0x1000, 0x1001, 0x0020, 0x1FFE]
    four = S.interleave(rng, [feed(rng, p, 60, [10, 100, 900], cc=i) for i, p in enumerate(pids)] + [S.filler(0x99, 30, rng)])
    two = S.interleave(rng, [feed(rng, 0x1000, 150, [30, 400, 3000], plps=(3, 5, 3)), S.filler(0x1FFF, 20, rng)])
    rig = Rig(pkg, eng, 3, 512, 512, watches=[[(k, p, -1) for k, p in enumerate(pids)], [], [(1, 0x1000, 3), (3, 0x1000, -1)]])
    rig.call([four[:130], NONE, two[:1]])                            # a stream of one TS packet beside an empty one
    rig.call([four[130:], NONE, two[1:]], shift=1)
    assert all(rig.models[0].stats(k)['t2mi_packets'] > 20 for k in range(4))
    assert rig.models[1].stats()['packets'] == 0
    a, b = rig.models[2].stats(1), rig.models[2].stats(3)
    assert a['t2mi_packets'] == b['t2mi_packets'] > 30 and 0 < a['bbframes_delivered'] < b['bbframes_delivered'] == b['bbframes']
    rig.dv.set_watch(2, 1, 0x1000, 5), rig.hb.set_watch(2, 1, 0x1000, 5), rig.models[2].set_watch(1, 0x1000, 5)     # a changed watch starts afresh
    rig.call([NONE, NONE, two[:40]])
    assert rig.models[2].stats(1)['packets'] == rig.dv.stats(2, 1)['packets'] < rig.dv.stats(2, 3)['packets']


def test_capacity_failure_leaves_every_slot_where_it_was(pkg, eng):
    import torch
    rng = np.random.default_rng(8)
    ts = [feed(rng, PID, 120, [50, 600, 2000], cc=i) for i in range(2)]
    watches = [[(0, PID, -1), (1, PID, 3)], [(2, PID, -1)]]
    rig = Rig(pkg, eng, 2, 128, 256, watches=watches)
    rig.call([ts[0][:50], ts[1][:70]])
    rest = [ts[0][50:], ts[1][70:]]
    need, rows = [[0] * 4, [0] * 4], [[0] * 4, [0] * 4]
    for i in range(2):
        m = T.T2mi()
        for slot, pid, plp in watches[i]:
            m.set_watch(slot, pid, plp)
        m.process(ts[i][:50 + 20 * i])
        need[i] = [o.size for o in m.process(rest[i])]
        rows[i] = [len(m.table(k)) for k in range(4)]
    before = [[rig.dv.stats(i, k) for k in range(4)] for i in range(2)]
    ins = [_dev(t) for t in rest]
    top = max(max(n) for n in need)
    assert sum(v == top for n in need for v in n) == 1               # one byte short for the slot that needs most, room for the others
    small = lambda cap: [[torch.zeros(cap, dtype=torch.uint8, device='cuda') if rig.used[i][k] else None for k in range(4)] for i in range(2)]
    with pytest.raises(pkg.Dvbs2GpuError) as e:
        rig.dv.process(ins, small(top - 1), nbytes=[t.size for t in rest])
    assert e.value.code == -5 and e.value.needed == need and e.value.rows == rows
    assert [[rig.dv.stats(i, k) for k in range(4)] for i in range(2)] == before
    assert all(rig.dv.row_table(i, k) == [] and rig.dv.frame_bytes(i, k) == [] for i in range(2) for k in range(4))
    tight = pkg.T2miBank(eng, 1, 128, rows[0][0] - 1)                # and one row short
    tight.set_watch(0, 0, PID)
    tight.process([_dev(ts[0][:50])], nbytes=[50 * 188])
    was = tight.stats(0)
    with pytest.raises(pkg.Dvbs2GpuError) as e:
        tight.process(ins[:1], [small(top)[0][:1]], nbytes=[rest[0].size])
    assert e.value.code == -5 and e.value.rows[0][0] == rows[0][0] and e.value.needed[0][0] == -1 and tight.stats(0) == was
    rig.call(rest)                                                   # the repeat, with room, equals the model and the host bank
    fresh = Rig(pkg, eng, 2, 128, 256, watches=watches)              # ... and a first call on a fresh rig
    fresh.call([ts[0][:50], ts[1][:70]]), fresh.call(rest)
    assert all(fresh.dv.row_table(i, k) == rig.dv.row_table(i, k) and fresh.dv.stats(i, k) == rig.dv.stats(i, k) for i in range(2) for k in range(4))


def test_end_to_end_chained_on_the_device(pkg, eng):
    """outer TS -> T2-MI -> BBFRAMEs -> inner TS -> monitor, all in HBM: only the frame-size list visits the host"""
    import torch
    rng = np.random.default_rng(13)
    kbch = {3: 7032, 5: 13152}                                       # two PLPs with short-frame T2 sizes
    inner = {plp: M.make_ts(150, rng, null_runs=False) for plp in kbch}
    for ts in inner.values():                                        # orderly headers for the monitor: three PIDs, payload only, counters in step
        for i, p in enumerate(ts):
            p[1], p[2], p[3] = (p[1] & 0x40) | 0x01, i % 3, 0x10 | (i // 3 & 15)
    frames = {plp: [f for f, _ in M.frames_of_stream(M.slot_stream(inner[plp])[0], 188, [kbch[plp]], sis=True)] for plp in kbch}
    order = [plp for i in range(max(len(f) for f in frames.values())) for plp in kbch if i < len(frames[plp])]
    at, pk, count = dict.fromkeys(kbch, 0), [], 77
    for i, plp in enumerate(order):
        count = (count + 1) & 255
        pk.append(T.bb_packet(count, plp, bytes(frames[plp][at[plp]]), frame_idx=i, start=int(i % 7 == 0)))
        at[plp] += 1
        if i % 3 == 0:                                               # an L1-type and a timestamp-type packet between
            pk += [T.t2mi_packet(0x10, count + 1, bytes(rng.integers(0, 256, 60, dtype=np.uint8))), T.t2mi_packet(0x20, count + 2, bytes(11), payload_bits=88)]
            count += 2
    t2 = T.Packetiser(0x1000).lay(pk)
    outer = S.interleave(rng, [t2, S.filler(0x31, len(t2) // 10, rng), S.filler(0x32, len(t2) // 7, rng)])
    assert len(outer) <= 4096
    bank = pkg.T2miBank(eng, 1, 4096, 512)
    bank.set_watch(0, 0, 0x1000, 3), bank.set_watch(0, 1, 0x1000, 5)
    bb = [torch.zeros(len(outer) * 188, dtype=torch.uint8, device='cuda') for _ in range(2)]
    nb = bank.process([_dev(outer)], [bb], nbytes=[outer.size])[0]
    st = bank.stats(0)
    assert st['crc_errors'] == st['count_errors'] == st['dropped_packets'] == 0 and st['t2mi_packets'] == 2 * len(pk)
    mon = pkg.TsMonitorBank(eng, 1, 4096)
    for k, plp in enumerate(kbch):
        sizes = bank.frame_bytes(0, k)                               # the one thing that visits the host
        assert sizes == [kbch[plp] // 8] * len(frames[plp]) and nb[k] == sum(sizes)
        ma = pkg.BbTsParserBank(eng, 1, kbch[plp], len(sizes))
        ma.set_mode_adaptation(True)
        ts_dev = torch.zeros(nb[k] + 376, dtype=torch.uint8, device='cuda')
        n = ma.process_ma([bb[k]], [[ts_dev]], frame_bytes=[sizes])[0][0]
        want = M.Receiver((0,)).process(frames[plp])[0]
        assert n == want.size > 140 * 188 and np.array_equal(ts_dev[:n].cpu().numpy(), want)
        mon.reset()
        mon.process([ts_dev], nbytes=[n])
        assert mon.stats(0)['cc_errors'] == 0 and mon.stats(0)['sync_byte_errors'] == 0 and mon.stats(0)['packets'] == n // 188
