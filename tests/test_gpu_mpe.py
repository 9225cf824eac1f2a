"""GPU tests of the MPE bank (csrc/mpe.hip): the kernels against the library's host bank and the model of tests/mpe_ref.py in bytes,
rows, counters, needed sizes and state through the next call, at the packet counts, datagram sizes, header placements, piece counts
and slot shapes where the compaction, the header chains, the row numbering, the head gather, the chunked CRC and the piecewise copy
can go wrong; and chained on the device behind the mode-adaptation packetiser."""
import numpy as np
import pytest

import ma_ref as M
import mpe_cases as K
import mpe_ref as R
import psi_ref as S

pytestmark = pytest.mark.gpu
PID = K.PID
NONE = np.zeros((0, 188), np.uint8)
ALL = b'\xff' * 6


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
    """a device bank, a host bank and one model per stream, fed the same calls.  watches[i]: [(slot, pid, mac, mask)]"""

    def __init__(self, pkg, eng, nstreams, max_packets, max_rows=512, watches=None):
        import torch
        self.eng, self.n = eng, nstreams
        self.dv, self.hb = pkg.MpeBank(eng, nstreams, max_packets, max_rows), pkg.MpeBank.host(nstreams, max_packets, max_rows)
        self.models = [R.Mpe() for _ in range(nstreams)]
        self.used = [[False] * 4 for _ in range(nstreams)]
        self.outs = [[torch.zeros(max_packets * 188 + 8, dtype=torch.uint8, device='cuda') for _ in range(4)] for _ in range(nstreams)]
        for i in range(nstreams):
            for w in (watches[i] if watches else [(0, PID, K.MAC, K.MASK)]):
                self.set_watch(i, *w)

    def set_watch(self, i, slot, pid, mac=None, mask=None):
        self.dv.set_watch(i, slot, pid, mac, mask), self.hb.set_watch(i, slot, pid, mac, mask), self.models[i].set_watch(slot, pid, mac, mask)
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
                assert self.dv.needed(i, k) == (want[k].size if deliver else 0, len(self.models[i].table(k))), (i, k)
                assert self.dv.stats(i, k) == self.models[i].stats(k) == self.hb.stats(i, k), (i, k)
            assert self.dv.stats(i) == self.models[i].stats(), i


SIZES = [20, 28, 100, 183, 700, 1400, 4080]


def feed(rng, pid, n_packets, sizes=SIZES, macs=(K.GROUP,), cc=0):
    """n_packets TS packets of an MPE feed: IPv4/UDP datagrams of the given sizes (20: a bare header) to the MAC addresses in turn, now and
    then behind LLC/SNAP, with stuffing, as IPv6 or as another table"""
    z, parts, got, i = R.Packetiser(pid, cc), [], 0, 0
    while got < n_packets:
        secs = []
        for _ in range(4):
            n, mac, kind = int(rng.choice(sizes)), macs[i % len(macs)], rng.random()
            i += 1
            d = R.ipv4(R.udp(int(rng.integers(65536)), 1234, bytes(rng.integers(0, 256, n - 28, dtype=np.uint8)))) if n >= 28 else R.ipv4(b'')
            if kind < 0.1 and n <= 4072:
                secs.append(R.section(R.llc_snap(0x0800) + d, mac=mac, llc=1))
            elif kind < 0.2 and n <= 4000:
                secs.append(R.section(R.ipv6(d[20:]), mac=mac, stuffing=int(rng.integers(0, 4))))
            elif kind < 0.25:
                secs.append(R.raw_section(0x3B, d[:60]))
            else:
                secs.append(R.section(d, mac=mac))
        parts.append(z.lay(secs, flush=rng.random() < 0.3))
        got += len(parts[-1])
    return np.concatenate(parts)[:n_packets]


def test_packet_counts_at_wave_and_workgroup_edges(pkg, eng):
    sizes = [0, 1, 63, 64, 65, 255, 256, 257, 4095, 4096]
    rng = np.random.default_rng(1)
    ts = feed(rng, PID, sum(sizes))
    ts[5000, 100] ^= 4                                               # and one bit error in the long calls
    rig = Rig(pkg, eng, 1, 4096, 2048)
    rows_only = Rig(pkg, eng, 1, 4096, 2048)
    a, open_at_cut = 0, 0
    for k, s in enumerate(sizes):
        rig.call([ts[a:a + s]], shift=k % 4)
        if s < 4095:
            rows_only.call([ts[a:a + s]], deliver=False)
        a += s
        open_at_cut += len(rig.models[0].slot[0].buf) > 0
    st = rig.models[0].stats(0)
    assert open_at_cut >= 5 and st['sections'] > 1000 and st['crc_errors'] == 1 and st['dropped_sections'] == 0
    assert {r['bytes'] for r in rig.models[0].table(0)} >= {20, 4080} and st['datagrams_delivered'] > 900
    assert rows_only.models[0].stats()['bytes_delivered'] == 0 and rows_only.models[0].stats()['datagrams'] > 50


def test_constructed_cases_whole_and_cut_in_two(pkg, eng):
    """the header splits after 1 and 2 bytes fall on a TS packet's end in `rig` and on a call's end in `cut`"""
    cases = K.edge_cases()
    rig, cut = Rig(pkg, eng, 1, 64), Rig(pkg, eng, 1, 64)
    for k, (name, ts) in enumerate(cases):
        rig.call([ts], shift=k % 4)
        assert [tuple(r[f] for f in K.ROW_FIELDS) for r in rig.models[0].table(0)] == K.ROWS[name], name
        if len(ts) > 1:
            cut.call([ts[:len(ts) // 2]], shift=(k + 1) % 4), cut.call([ts[len(ts) // 2:]], shift=(k + 2) % 4)
        else:
            cut.call([ts])
    assert rig.models[0].stats() == cut.models[0].stats() == K.STATS
    one = Rig(pkg, eng, 1, 512, watches=[[(0, PID, K.MAC, K.MASK), (1, PID, bytes.fromhex('01005e7fffff'), ALL)]])
    one.call([K.whole_stream(cases)])                                # and back to back in one call, beside a slot that takes one address alone
    assert one.models[0].stats(0) == K.STATS and one.models[0].stats(1)['datagrams_delivered'] == 1 and one.models[0].stats(1)['filtered'] == 30


@pytest.mark.parametrize('npieces,size', [(63, 900), (64, 900), (65, 900), (140, 900), (4, 300), (5, 300), (16, 1416), (17, 1416), (32, 4096), (33, 4096)])
def test_sections_of_many_pieces(pkg, eng, npieces, size):
    """one section through adaptation fields over that many TS packets: the CRC's further rounds (a round takes 4, 8, 16 or 32 pieces
    for a section of 300, 900, 1416 or 4096 bytes: one piece fewer than two rounds and one more, and up to 18 rounds), and a head
    gathered from pieces of one to three bytes; whole, and cut inside the thin packets"""
    ts, cc, sec = K.many_pieces(npieces, size=size)
    again, _, _ = K.many_pieces(npieces, cc=cc, seed=60, size=size)
    bad = again.copy()
    bad[5 if npieces > 8 else -1, 187] ^= 0x40                       # the last payload byte of a thin packet (section byte 11), or the section's last: the CRC must see it
    rig = Rig(pkg, eng, 1, 512, 8, watches=[[(0, PID, None, None)]])
    rig.call([np.concatenate([ts, bad])], shift=1)
    rows = rig.models[0].table(0)
    assert [(r['flags'], r['bytes'], r['first_packet'], r['last_packet']) for r in rows] == [(R.DATAGRAM, size - 16, 0, npieces - 1), (R.CRC_ERROR, 0, npieces, 2 * npieces - 1)]
    cut = Rig(pkg, eng, 1, 512, 8, watches=[[(0, PID, None, None)]])
    cut.call([ts[:npieces // 2]], shift=2), cut.call([ts[npieces // 2:]], shift=3)       # the head itself, or a part of it, carried in the slot's buffer
    assert cut.models[0].table(0)[0]['first_packet'] == -1 and cut.models[0].stats()['bytes_delivered'] == size - 16


def test_sections_carried_over_two_and_three_calls(pkg, eng):
    cases = dict(K.edge_cases())
    big, mid = cases['the largest section: 4096 bytes, datagram 4080'], cases['a 1400-byte datagram over 8 packets']
    rig = Rig(pkg, eng, 1, 64)
    for a in (0, 8, 16):
        rig.call([big[a:a + 8]], shift=a % 3)                        # three calls; the first two move nothing but state
        assert len(rig.models[0].table(0)) == (a == 16)
    assert rig.models[0].table(0)[0]['first_packet'] == -1 and rig.models[0].table(0)[0]['last_packet'] == 6
    rig.call([mid[:7]]), rig.call([mid[7:]], shift=3)                # two calls; the last brings one TS packet
    assert rig.models[0].stats()['bytes_delivered'] == 4080 + 1400 and rig.models[0].stats()['crc_errors'] == 0
    for h in (1, 2):                                                 # an open header of h bytes through an EMPTY call and on
        ts = cases['header split after %d byte%s' % (h, 's' * (h > 1))]
        rig.call([ts[:1]]), rig.call([NONE]), rig.call([ts[1:]], shift=h)
        assert rig.models[0].table(0)[0]['first_packet'] == -1 and rig.models[0].table(0)[0]['bytes'] == 39 + h


def test_slot_shapes(pkg, eng):
    rng = np.random.default_rng(5)
    pids = [0x1000, 0x1001, 0x0020, 0x1FFE]
    small = [20, 100, 900]
    four = S.interleave(rng, [feed(rng, p, 60, small, cc=i) for i, p in enumerate(pids)] + [S.filler(0x99, 30, rng)])
    a, b = bytes.fromhex('02aabbccdd01'), bytes.fromhex('02aabbccdd02')
    two = S.interleave(rng, [feed(rng, 0x1000, 150, [30, 400, 3000], macs=(a, b, a)), S.filler(0x1FFF, 20, rng)])
    three = feed(rng, 0x0300, 40, small)
    rig = Rig(pkg, eng, 5, 512, 512, watches=[[(k, p, None, None) for k, p in enumerate(pids)], [], [(1, 0x1000, b, ALL), (3, 0x1000, None, None)],
                                               [(2, 0x0300, None, None)], [(0, 0x0300, None, None), (1, 0x0300, K.GROUP, ALL), (2, 0x0301, None, None)]])
    rig.call([four[:130], NONE, two[:1], three[:20], NONE])          # a stream of one TS packet beside empty ones
    rig.call([four[130:], three, two[1:], three[20:], three], shift=1)           # (stream 1 watches nothing and is fed all the same)
    assert all(rig.models[0].stats(k)['sections'] > 20 for k in range(4))
    assert rig.models[1].stats()['packets'] == 0
    sa, sb = rig.models[2].stats(1), rig.models[2].stats(3)
    assert sa['sections'] == sb['sections'] > 15 and 0 < sa['datagrams_delivered'] < sb['datagrams_delivered'] and sa['filtered'] > 0
    assert rig.models[4].stats(2)['packets'] == 0 and rig.models[4].stats(0) == rig.models[4].stats(1) == rig.models[3].stats(2)     # one call or two
    rig.set_watch(2, 1, 0x1000, a, ALL)                              # a changed watch starts afresh
    rig.call([NONE, NONE, two[:40], NONE, NONE])
    assert rig.models[2].stats(1)['packets'] == rig.dv.stats(2, 1)['packets'] < rig.dv.stats(2, 3)['packets']


def test_host_buffers_on_a_device_bank(pkg, eng):
    """work(): one slot of a device bank with host buffers; the other slot on the same PID receives an empty call"""
    ts = dict(K.edge_cases())['a 1400-byte datagram over 8 packets']
    dv, m = pkg.MpeBank(eng, 2, 16, 8), R.Mpe()
    dv.set_watch(1, 2, PID), dv.set_watch(1, 3, PID), m.set_watch(2, PID)
    for part in (ts[:3], ts[3:]):
        want = m.process(part)[2]
        assert np.array_equal(dv.work(part, stream=1, slot=2), want) and dv.row_table(1, 2) == m.table(2)
    assert dv.stats(1, 2) == m.stats(2) and dv.stats(1, 2)['bytes_delivered'] == 1400 and dv.stats(1, 3)['packets'] == 0
    with pytest.raises(pkg.Dvbs2GpuError) as e:
        dv.work(ts, stream=1, slot=2, cap=1399)
    assert e.value.code == -5 and (e.value.needed, e.value.rows) == (1400, 1) and dv.stats(1, 2) == m.stats(2)


def test_wide_bank_with_mostly_empty_slots(pkg, eng):
    """300 streams of 16 packets: 1200 workgroups, more than the device has compute units, most of them for empty slots"""
    rng = np.random.default_rng(6)
    base = [feed(rng, PID, 16, [20, 60, 300], cc=i) for i in range(3)]
    watches = [[(i % 4, PID, None, None)] if i % 7 == 0 else [(0, PID, K.GROUP, ALL), (3, PID, None, None)] if i % 50 == 1 else [] for i in range(300)]
    rig = Rig(pkg, eng, 300, 16, 64, watches=watches)
    rig.call([base[i % 3] for i in range(300)], shift=1)
    rig.call([base[(i + 1) % 3][:i % 17] for i in range(300)])
    assert sum(rig.models[i].stats()['datagrams_delivered'] > 0 for i in range(300)) == sum(bool(w) for w in watches) == 49


def test_capacity_failure_leaves_every_slot_where_it_was(pkg, eng):
    import torch
    rng = np.random.default_rng(8)
    ts = [feed(rng, PID, 120, [50, 600, 2000], cc=i) for i in range(2)]
    watches = [[(0, PID, None, None), (1, PID, K.GROUP, ALL)], [(2, PID, None, None)]]
    rig = Rig(pkg, eng, 2, 128, 256, watches=watches)
    rig.call([ts[0][:50], ts[1][:70]])
    rest = [ts[0][50:], ts[1][70:]]
    need, rows = [[0] * 4, [0] * 4], [[0] * 4, [0] * 4]
    for i in range(2):
        m = R.Mpe()
        for w in watches[i]:
            m.set_watch(*w)
        m.process(ts[i][:50 + 20 * i])
        need[i] = [o.size for o in m.process(rest[i])]
        rows[i] = [len(m.table(k)) for k in range(4)]
    before = [[rig.dv.stats(i, k) for k in range(4)] for i in range(2)]
    ins = [_dev(t) for t in rest]
    top = max(max(n) for n in need)
    small = lambda cap: [[torch.zeros(cap, dtype=torch.uint8, device='cuda') if rig.used[i][k] else None for k in range(4)] for i in range(2)]
    with pytest.raises(pkg.Dvbs2GpuError) as e:
        rig.dv.process(ins, small(top - 1), nbytes=[t.size for t in rest])      # one byte short for the slot that needs most
    assert e.value.code == -5 and e.value.needed == need and e.value.rows == rows
    assert [[rig.dv.stats(i, k) for k in range(4)] for i in range(2)] == before
    assert all(rig.dv.row_table(i, k) == [] for i in range(2) for k in range(4))
    tight = pkg.MpeBank(eng, 1, 128, rows[0][0] - 1)                 # and one row short
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
    """BBFRAMEs -> mode-adaptation packetiser -> TS -> MPE bank on one stream, all in HBM: the datagrams that come out are the ones
    that went in, and no packet visits the host"""
    import torch
    rng = np.random.default_rng(13)
    kbch = 7032
    sent = [R.ipv4(R.udp(4000 + i, 5000, bytes(rng.integers(0, 256, int(rng.choice([12, 200, 1372])), dtype=np.uint8)))) for i in range(40)]
    mpe = R.Packetiser(0x0300).lay([R.section(d) for d in sent])
    inner = S.interleave(rng, [mpe, S.filler(0x31, len(mpe) // 5, rng)])
    frames = [f for f, _ in M.frames_of_stream(M.slot_stream(inner)[0], 188, [kbch], sis=True)]
    sizes = [int(f.size) for f in frames]
    ma = pkg.BbTsParserBank(eng, 1, kbch, len(frames))
    ma.set_mode_adaptation(True)
    bb = torch.from_numpy(np.concatenate(frames)).cuda()
    ts_dev = torch.zeros(sum(sizes) + 376, dtype=torch.uint8, device='cuda')
    n = ma.process_ma([bb], [[ts_dev]], frame_bytes=[sizes])[0][0]
    want_ts = M.Receiver((0,)).process(frames)[0]
    assert n == want_ts.size and n % 188 == 0 and n // 188 >= len(inner) - 40
    bank = pkg.MpeBank(eng, 1, 4096, 128)
    bank.set_watch(0, 0, 0x0300)
    out = torch.zeros(n, dtype=torch.uint8, device='cuda')
    nb = bank.process([ts_dev], [[out]], nbytes=[n])[0][0]
    model = R.Slot(0x0300)
    want = model.process(want_ts)
    got = out[:nb].cpu().numpy()
    assert np.array_equal(got, want) and bank.row_table(0, 0) == model.table
    k = len(model.table)
    assert k >= 36 and bytes(got) == b''.join(sent[:k]) and bank.stats(0)['crc_errors'] == 0 and bank.stats(0)['datagrams_delivered'] == k
