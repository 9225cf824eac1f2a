"""GPU tests of the ULE bank (csrc/ule.hip): the kernels against the library's host bank and the model of tests/ule_ref.py in bytes,
rows, counters, needed sizes and state through the next call, at the packet counts, SNDU sizes, header placements, piece counts and
slot shapes where the compaction, the header chains, the row numbering, the head gather, the extension-header walk, the chunked CRC
and the piecewise copy can go wrong; and chained on the device behind the mode-adaptation packetiser."""
import numpy as np
import pytest

import ma_ref as M
import psi_ref as S
import ule_cases as K
import ule_ref as R

pytestmark = pytest.mark.gpu
PID = K.PID
NONE = np.zeros((0, 188), np.uint8)
ALL = b'\xff' * 6
MAIN = (0, PID, K.NPA, K.MASK, True)


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
    """a device bank, a host bank and one model per stream, fed the same calls.  watches[i]: [(slot, pid, npa, mask, accept_unaddressed)]"""

    def __init__(self, pkg, eng, nstreams, max_packets, max_rows=512, watches=None):
        import torch
        self.eng, self.n = eng, nstreams
        self.dv, self.hb = pkg.UleBank(eng, nstreams, max_packets, max_rows), pkg.UleBank.host(nstreams, max_packets, max_rows)
        self.models = [R.Ule() for _ in range(nstreams)]
        self.used = [[False] * 4 for _ in range(nstreams)]
        self.outs = [[torch.zeros(max_packets * 188 + 8, dtype=torch.uint8, device='cuda') for _ in range(4)] for _ in range(nstreams)]
        for i in range(nstreams):
            for w in (watches[i] if watches else [MAIN]):
                self.set_watch(i, *w)

    def set_watch(self, i, slot, pid, npa=None, mask=None, accept=False):
        self.dv.set_watch(i, slot, pid, npa, mask, accept), self.hb.set_watch(i, slot, pid, npa, mask, accept), self.models[i].set_watch(slot, pid, npa, mask, accept)
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


SIZES = [20, 28, 100, 183, 700, 1400, 4082]


def feed(rng, pid, n_packets, sizes=SIZES, npas=(K.GROUP,), cc=0):
    """n_packets TS packets of a ULE feed: IPv4/UDP datagrams of the given sizes (20: a bare header) to the addresses in turn (None:
    D = 1), now and then behind optional headers, in a bridged frame, with stuffing, as IPv6, as a Test SNDU or with an unknown Type;
    now and then the TS packet is padded with 0xFF behind them"""
    z, parts, got, i = R.Packetiser(pid, cc), [], 0, 0
    while got < n_packets:
        sndus = []
        for _ in range(4):
            n, npa, kind = int(rng.choice(sizes)), npas[i % len(npas)], rng.random()
            i += 1
            d = R.ipv4(R.udp(int(rng.integers(65536)), 1234, bytes(rng.integers(0, 256, n - 28, dtype=np.uint8)))) if n >= 28 else R.ipv4(b'')
            if kind < 0.1 and n <= 4000:
                hdrs = [(int(h), 9, bytes(2 * int(h) - 2)) for h in rng.integers(1, 6, int(rng.integers(1, 5)))]
                sndus.append(R.sndu(*R.extended(hdrs, 0x0800, d), npa=npa))
            elif kind < 0.2 and n <= 4000:
                sndus.append(R.sndu(*R.bridged(0x0800, d), npa=npa))
            elif kind < 0.3 and n <= 4000:
                sndus.append(R.sndu(0x86DD, R.ipv6(d[20:]) + bytes(int(rng.integers(0, 4))), npa=npa))
            elif kind < 0.35:
                sndus.append(R.sndu(int(rng.choice([0x0000, 0x0002, 0x0806])), d[:60], npa=npa))
            else:
                sndus.append(R.sndu(0x0800, d, npa=npa))
        flush = rng.random() < 0.3
        parts.append(z.lay(sndus, flush=flush, pad=flush and rng.random() < 0.5))
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
    assert open_at_cut >= 5 and st['sndus'] > 1000 and st['crc_errors'] == 1 and st['dropped_sndus'] == 0
    assert {r['bytes'] for r in rig.models[0].table(0)} >= {20, 4082} and st['datagrams_delivered'] > 900 and st['bridged'] > 50 and st['extension'] > 5
    assert rows_only.models[0].stats()['bytes_delivered'] == 0 and rows_only.models[0].stats()['datagrams'] > 50


def test_constructed_cases_whole_and_cut_in_two(pkg, eng):
    """the base header splits after 1, 2 and 3 bytes fall on a TS packet's end in `rig` and on a call's end in `cut`; slot 1 does not
    accept SNDUs without an address"""
    cases = K.edge_cases()
    both = [[MAIN, (1, PID, K.NPA, K.MASK, False)]]
    rig, cut = Rig(pkg, eng, 1, 256, watches=both), Rig(pkg, eng, 1, 256, watches=both)
    for k, (name, ts) in enumerate(cases):
        rig.call([ts], shift=k % 4)
        assert [tuple(r[f] for f in K.ROW_FIELDS) for r in rig.models[0].table(0)] == K.ROWS[name], name
        if name in K.ROWS_NO_ACCEPT:
            assert [tuple(r[f] for f in K.ROW_FIELDS) for r in rig.models[0].table(1)] == K.ROWS_NO_ACCEPT[name], name
        if len(ts) > 1:
            cut.call([ts[:len(ts) // 2]], shift=(k + 1) % 4), cut.call([ts[len(ts) // 2:]], shift=(k + 2) % 4)
        else:
            cut.call([ts])
    assert rig.models[0].stats(0) == cut.models[0].stats(0) == K.STATS and rig.models[0].stats(1) == cut.models[0].stats(1) == K.STATS_NO_ACCEPT
    one = Rig(pkg, eng, 1, 512, watches=[[MAIN, (1, PID, bytes.fromhex('01005e7fffff'), ALL, False)]])
    one.call([K.whole_stream(cases)])                                # and back to back in one call, beside a slot that takes one address alone
    st = one.models[0].stats(1)
    assert one.models[0].stats(0) == K.STATS and st['datagrams_delivered'] == 1 and st['filtered'] == K.STATS['sndus'] - 1 - K.STATS['crc_errors'] - 2


@pytest.mark.parametrize('npieces,size', [(63, 900), (64, 900), (65, 900), (140, 900), (4, 300), (5, 300), (16, 1416), (17, 1416), (32, 4096), (33, 4096)])
def test_sndus_of_many_pieces(pkg, eng, npieces, size):
    """one SNDU through adaptation fields over that many TS packets: the CRC's further rounds (a round takes 4, 8, 16 or 32 pieces
    for an SNDU of 300, 900, 1416 or 4096 bytes: one piece fewer than two rounds and one more, and up to 18 rounds), and a head
    gathered from pieces of one to three bytes; whole, and cut inside the thin packets"""
    ts, cc, sec = K.many_pieces(npieces, size=size)
    again, _, _ = K.many_pieces(npieces, cc=cc, seed=60, size=size)
    bad = again.copy()
    bad[5 if npieces > 8 else -1, 187] ^= 0x40                       # the last payload byte of a thin packet, or the SNDU's last: the CRC must see it
    rig = Rig(pkg, eng, 1, 512, 8, watches=[[(0, PID, None, None, False)]])
    rig.call([np.concatenate([ts, bad])], shift=1)
    rows = rig.models[0].table(0)
    assert [(r['flags'], r['bytes'], r['first_packet'], r['last_packet']) for r in rows] == [(R.DATAGRAM, size - 14, 0, npieces - 1), (R.CRC_ERROR, 0, npieces, 2 * npieces - 1)]
    cut = Rig(pkg, eng, 1, 512, 8, watches=[[(0, PID, None, None, False)]])
    cut.call([ts[:npieces // 2]], shift=2), cut.call([ts[npieces // 2:]], shift=3)       # the head itself, or a part of it, carried in the slot's buffer
    assert cut.models[0].table(0)[0]['first_packet'] == -1 and cut.models[0].stats()['bytes_delivered'] == size - 14


def test_the_head_a_byte_per_ts_packet(pkg, eng):
    """the SNDU whose row needs all 128 leading bytes (NPA, 40 bytes of optional headers, a bridged frame, IHL 15, UDP), each of them
    in a TS packet of its own: whole; cut so that 1, 64 and 127 of them come from the slot's buffer; and with a bit error in byte 127,
    the second destination-port byte, which the CRC catches"""
    sec = K.full_head()
    assert len(sec) == 368

    def lay(cc):
        thin, cc = R.thin_packets(PID, cc, sec[:130])
        tail = sec[130:]
        cc1, cc2 = (cc + 1) & 15, (cc + 2) & 15
        rest = [S.packet(PID, cc1, tail[:184]), S.packet(PID, cc2, tail[184:], af_len=184 - len(tail[184:]) - 1)]
        return np.concatenate([thin, np.array(rest, np.uint8).reshape(-1, 188)]), cc2

    rig = Rig(pkg, eng, 1, 512, 8)
    cc = 0
    for cut in (0, 1, 64, 127):
        ts, cc = lay(cc)
        for part in ([ts[:cut], ts[cut:]] if cut else [ts]):
            rig.call([part], shift=cut % 4)
        row = rig.models[0].table(0)[0]
        assert (row['flags'], row['ip_at'], row['extension_bytes'], row['bytes'], row['dst_port']) == (R.DATAGRAM | R.BRIDGED, 64, 40, 300, 1234)
        assert row['first_packet'] == (-1 if cut else 0)
    ts, cc = lay(cc)
    ts[127, 187] ^= 1
    rig.call([ts])
    assert rig.models[0].table(0)[0]['flags'] == R.CRC_ERROR and rig.models[0].stats()['datagrams_delivered'] == 4


def test_sndus_carried_over_two_and_three_calls(pkg, eng):
    cases = dict(K.edge_cases())
    big, mid = cases['Length 4092: the largest SNDU, datagram 4082'], cases['a 1400-byte datagram over 8 packets']
    rig = Rig(pkg, eng, 1, 64)
    for a in (0, 8, 16):
        rig.call([big[a:a + 8]], shift=a % 3)                        # three calls; the first two move nothing but state
        assert len(rig.models[0].table(0)) == (a == 16)
    assert rig.models[0].table(0)[0]['first_packet'] == -1 and rig.models[0].table(0)[0]['last_packet'] == 6
    rig.call([mid[:7]]), rig.call([mid[7:]], shift=3)                # two calls; the last brings one TS packet
    assert rig.models[0].stats()['bytes_delivered'] == 4082 + 1400 and rig.models[0].stats()['crc_errors'] == 0
    for h in (1, 2, 3):                                              # an open header of h bytes through an EMPTY call and on
        ts = cases['base header split after %d byte%s' % (h, 's' * (h > 1))]
        rig.call([ts[:1]]), rig.call([NONE]), rig.call([ts[1:]], shift=h)
        assert rig.models[0].table(0)[0]['first_packet'] == -1 and rig.models[0].table(0)[0]['bytes'] == 39 + h


def test_slot_shapes(pkg, eng):
    """all four slots on one PID with different masks, one slot of four, no slot, four PIDs in four slots"""
    rng = np.random.default_rng(5)
    pids = [0x1000, 0x1001, 0x0020, 0x1FFE]
    small = [20, 100, 900]
    four = S.interleave(rng, [feed(rng, p, 60, small, cc=i) for i, p in enumerate(pids)] + [S.filler(0x99, 30, rng)])
    a, b = bytes.fromhex('02aabbccdd01'), bytes.fromhex('02aabbccdd02')
    two = S.interleave(rng, [feed(rng, 0x1000, 150, [30, 400, 3000], npas=(a, b, a, None)), S.filler(0x1FFF, 20, rng)])
    three = feed(rng, 0x0300, 40, small)
    rig = Rig(pkg, eng, 5, 512, 512, watches=[[(k, p, None, None, False) for k, p in enumerate(pids)], [],
                                               [(0, 0x1000, a, ALL, False), (1, 0x1000, b, ALL, True), (2, 0x1000, a, bytes.fromhex('ffffffffff00'), False), (3, 0x1000, None, None, True)],
                                               [(2, 0x0300, None, None, False)], [(0, 0x0300, None, None, False), (1, 0x0300, K.GROUP, ALL, False), (2, 0x0301, None, None, False)]])
    rig.call([four[:130], NONE, two[:1], three[:20], NONE])          # a stream of one TS packet beside empty ones
    rig.call([four[130:], three, two[1:], three[20:], three], shift=1)           # (stream 1 watches nothing and is fed all the same)
    assert all(rig.models[0].stats(k)['sndus'] > 20 for k in range(4))
    assert rig.models[1].stats()['packets'] == 0
    s = [rig.models[2].stats(k) for k in range(4)]
    assert s[0]['sndus'] == s[1]['sndus'] == s[2]['sndus'] == s[3]['sndus'] > 15 and s[3]['filtered'] == 0 and s[3]['no_address'] > 0
    assert 0 < s[0]['datagrams_delivered'] < s[2]['datagrams_delivered'] < s[3]['datagrams_delivered'] and s[1]['datagrams_delivered'] > 0
    assert rig.models[4].stats(2)['packets'] == 0 and rig.models[4].stats(0) == rig.models[4].stats(1) == rig.models[3].stats(2)     # one call or two
    rig.set_watch(2, 1, 0x1000, a, ALL)                              # a changed watch starts afresh
    rig.call([NONE, NONE, two[:40], NONE, NONE])
    assert rig.models[2].stats(1)['packets'] == rig.dv.stats(2, 1)['packets'] < rig.dv.stats(2, 3)['packets']


def test_host_buffers_on_a_device_bank(pkg, eng):
    """work(): one slot of a device bank with host buffers; the other slot on the same PID receives an empty call"""
    ts = dict(K.edge_cases())['a 1400-byte datagram over 8 packets']
    dv, m = pkg.UleBank(eng, 2, 16, 8), R.Ule()
    dv.set_watch(1, 2, PID), dv.set_watch(1, 3, PID), m.set_watch(2, PID)
    for part in (ts[:3], ts[3:]):
        want = m.process(part)[2]
        assert np.array_equal(dv.work(part, stream=1, slot=2), want) and dv.row_table(1, 2) == m.table(2)
    assert dv.stats(1, 2) == m.stats(2) and dv.stats(1, 2)['bytes_delivered'] == 1400 and dv.stats(1, 3)['packets'] == 0
    with pytest.raises(pkg.Dvbs2GpuError) as e:
        dv.work(ts, stream=1, slot=2, cap=1399)
    assert e.value.code == -5 and (e.value.needed, e.value.rows) == (1400, 1) and dv.stats(1, 2) == m.stats(2)


def test_sixty_four_streams_three_in_four_empty(pkg, eng):
    """256 workgroups of which 16 have a slot to serve: the early return beside working neighbours, in every slot position"""
    rng = np.random.default_rng(6)
    base = [feed(rng, PID, 16, [20, 60, 300], cc=i) for i in range(3)]
    watches = [[(i // 4 % 4, PID, None, None, True)] if i % 4 == 0 else [] for i in range(64)]
    rig = Rig(pkg, eng, 64, 16, 64, watches=watches)
    rig.call([base[i % 3] for i in range(64)], shift=1)
    rig.call([base[(i + 1) % 3][:i % 17] for i in range(64)])
    assert sum(rig.models[i].stats()['datagrams_delivered'] > 0 for i in range(64)) == sum(bool(w) for w in watches) == 16


def test_capacity_failure_leaves_every_slot_where_it_was(pkg, eng):
    """an SNDU is open in every watching slot at the failing call: nothing advances, and the retry with room gives the model's result"""
    import torch
    rng = np.random.default_rng(8)
    ts = [feed(rng, PID, 120, [50, 600, 2000], cc=i) for i in range(2)]
    watches = [[(0, PID, None, None, True), (1, PID, K.GROUP, ALL, False)], [(2, PID, None, None, False)]]
    rig = Rig(pkg, eng, 2, 128, 256, watches=watches)
    cuts = [next(c for c in range(40 + 20 * i, 120) if _open_after(ts[i][:c])) for i in range(2)]
    rig.call([ts[0][:cuts[0]], ts[1][:cuts[1]]])
    assert all(rig.models[i].slot[w[0]].buf for i in range(2) for w in watches[i])
    rest = [ts[0][cuts[0]:], ts[1][cuts[1]:]]
    need, rows = [[0] * 4, [0] * 4], [[0] * 4, [0] * 4]
    for i in range(2):
        m = R.Ule()
        for w in watches[i]:
            m.set_watch(*w)
        m.process(ts[i][:cuts[i]])
        need[i] = [o.size for o in m.process(rest[i])]
        rows[i] = [len(m.table(k)) for k in range(4)]
    before = [[rig.dv.stats(i, k) for k in range(4)] for i in range(2)]
    ins = [_dev(t) for t in rest]
    top = max(max(n) for n in need)
    small = lambda cap: [[torch.zeros(cap, dtype=torch.uint8, device='cuda') if rig.used[i][k] else None for k in range(4)] for i in range(2)]
    with pytest.raises(pkg.Dvbs2GpuError) as e:
        rig.dv.process(ins, small(top - 1), nbytes=[t.size for t in rest])      # one byte short for the slot that needs most
    assert e.value.code == -5 and e.value.needed == need and e.value.rows == rows
    assert [rig.dv.needed(i, k) for i in range(2) for k in range(4)] == [(need[i][k], rows[i][k]) for i in range(2) for k in range(4)]
    assert [[rig.dv.stats(i, k) for k in range(4)] for i in range(2)] == before
    assert all(rig.dv.row_table(i, k) == [] for i in range(2) for k in range(4))
    tight = pkg.UleBank(eng, 1, 128, rows[0][0] - 1)                 # and one row short
    tight.set_watch(0, 0, PID, None, None, True)
    tight.process([_dev(ts[0][:cuts[0]])], nbytes=[cuts[0] * 188])
    was = tight.stats(0)
    with pytest.raises(pkg.Dvbs2GpuError) as e:
        tight.process(ins[:1], [small(top)[0][:1]], nbytes=[rest[0].size])
    assert e.value.code == -5 and e.value.rows[0][0] == rows[0][0] and e.value.needed[0][0] == -1 and tight.stats(0) == was
    rig.call(rest)                                                   # the repeat, with room, equals the model and the host bank
    fresh = Rig(pkg, eng, 2, 128, 256, watches=watches)              # ... and a first call on a fresh rig
    fresh.call([ts[0][:cuts[0]], ts[1][:cuts[1]]]), fresh.call(rest)
    assert all(fresh.dv.row_table(i, k) == rig.dv.row_table(i, k) and fresh.dv.stats(i, k) == rig.dv.stats(i, k) for i in range(2) for k in range(4))


def _open_after(ts):
    m = R.Slot(PID)
    m.process(ts)
    return len(m.buf) > 0


def test_end_to_end_chained_on_the_device(pkg, eng):
    """BBFRAMEs -> mode-adaptation packetiser -> TS -> ULE bank on one stream, all in HBM: the datagrams that come out are the ones
    that went in, and no packet visits the host"""
    import torch
    rng = np.random.default_rng(13)
    kbch = 7032
    sent = [R.ipv4(R.udp(4000 + i, 5000, bytes(rng.integers(0, 256, int(rng.choice([12, 200, 1372])), dtype=np.uint8)))) for i in range(40)]
    ule = R.Packetiser(0x0300).lay([R.sndu(0x0800, d, npa=K.GROUP) for d in sent], pad=True)
    inner = S.interleave(rng, [ule, S.filler(0x31, len(ule) // 5, rng)])
    frames = [f for f, _ in M.frames_of_stream(M.slot_stream(inner)[0], 188, [kbch], sis=True)]
    sizes = [int(f.size) for f in frames]
    ma = pkg.BbTsParserBank(eng, 1, kbch, len(frames))
    ma.set_mode_adaptation(True)
    bb = torch.from_numpy(np.concatenate(frames)).cuda()
    ts_dev = torch.zeros(sum(sizes) + 376, dtype=torch.uint8, device='cuda')
    n = ma.process_ma([bb], [[ts_dev]], frame_bytes=[sizes])[0][0]
    want_ts = M.Receiver((0,)).process(frames)[0]
    assert n == want_ts.size and n % 188 == 0 and n // 188 >= len(inner) - 40
    bank = pkg.UleBank(eng, 1, 4096, 128)
    bank.set_watch(0, 0, 0x0300, K.GROUP, ALL)
    out = torch.zeros(n, dtype=torch.uint8, device='cuda')
    nb = bank.process([ts_dev], [[out]], nbytes=[n])[0][0]
    model = R.Slot(0x0300, K.GROUP, ALL)
    want = model.process(want_ts)
    got = out[:nb].cpu().numpy()
    assert np.array_equal(got, want) and bank.row_table(0, 0) == model.table
    k = len(model.table)
    assert k >= 36 and bytes(got) == b''.join(sent[:k]) and bank.stats(0)['crc_errors'] == 0 and bank.stats(0)['datagrams_delivered'] == k


def test_an_mpe_and_a_ule_bank_side_by_side(pkg, eng):
    """the two banks are two instantiations of one core (csrc/dgram_bank.h) in one process and share no state: on one engine an MpeBank
    and a UleBank take the same two streams, each carrying an MPE PID and a ULE PID interleaved, in calls of 1, 64 and 65 packets,
    turn and turn about.  Every call of either bank equals its model and its host bank in bytes, rows, needed sizes and counters and
    costs two launches (Rig.call, here and in test_gpu_mpe.py).  The call of 64 packets first goes to a pair of banks with max_rows = 2
    that took the first call too: it fails for capacity in both, advances nothing, and is repeated on the banks with room.  The last
    call has deliver=False in the ULE bank.  Each bank watches the other's PID in a further slot and finds no unit of its own there."""
    import test_gpu_mpe as TM
    MP, UP, sizes = 0x0300, 0x0301, [28, 100, 700]
    rng = np.random.default_rng(21)
    ts = [S.interleave(rng, [TM.feed(rng, MP, 65, sizes, cc=i), feed(rng, UP, 65, sizes, cc=3 + i)]) for i in range(2)]
    wm = [[(0, MP, None, None)], [(1, MP, None, None), (2, UP, None, None)]]
    wu = [[(0, UP, None, None, True)], [(3, UP, None, None, True), (1, MP, None, None, True)]]
    mpe, ule = TM.Rig(pkg, eng, 2, 65, 64, watches=wm), Rig(pkg, eng, 2, 65, 64, watches=wu)
    tight = [pkg.MpeBank(eng, 2, 65, 2), pkg.UleBank(eng, 2, 65, 2)]
    for bank, watches in zip(tight, (wm, wu)):
        for i in range(2):
            for w in watches[i]:
                bank.set_watch(i, *w)
    calls = [[t[a:b] for t in ts] for a, b in ((0, 1), (1, 65), (65, 130))]
    mpe.call(calls[0]), ule.call(calls[0], shift=1)
    undelivered = lambda st: {n: v for n, v in st.items() if n not in ('datagrams_delivered', 'bytes_delivered')}   # (they take rows only)
    failed, was = [], []
    for bank, rig in zip(tight, (mpe, ule)):
        bank.process([_dev(t) for t in calls[0]], None, nbytes=[t.size for t in calls[0]])
        was.append([[bank.stats(i, k) for k in range(4)] for i in range(2)])
        assert all(was[-1][i][k] == undelivered(rig.dv.stats(i, k)) | {'datagrams_delivered': 0, 'bytes_delivered': 0} for i in range(2) for k in range(4))
    for bank, before in zip(tight, was):
        with pytest.raises(pkg.Dvbs2GpuError) as e:
            bank.process([_dev(t) for t in calls[1]], None, nbytes=[t.size for t in calls[1]])
        assert e.value.code == -5 and all(bank.stats(i, k) == before[i][k] and bank.row_table(i, k) == [] for i in range(2) for k in range(4))
        failed.append(e.value)
    mpe.call(calls[1], shift=2), ule.call(calls[1], shift=3)         # the repeat, with room
    for e, bank, rig in zip(failed, tight, (mpe, ule)):
        rows = [[rig.dv.needed(i, k)[1] for k in range(4)] for i in range(2)]
        assert e.rows == rows and max(max(r) for r in rows) > 2 and e.needed == [[-1 if n > 2 else 0 for n in r] for r in rows]
        assert [[bank.needed(i, k) for k in range(4)] for i in range(2)] == [[(b, n) for b, n in zip(e.needed[i], rows[i])] for i in range(2)]
    mpe.call(calls[2], shift=1), ule.call(calls[2], deliver=False)
    assert all(bank.stats(i, k) == before[i][k] for bank, before in zip(tight, was) for i in range(2) for k in range(4))     # untouched by the others' calls
    assert mpe.models[1].stats(1)['datagrams_delivered'] > 10 and mpe.models[1].stats(2)['dropped_sections'] > 0 and mpe.models[1].stats(2)['sections'] == 0
    assert ule.models[1].stats(3)['datagrams'] > 10 and ule.models[1].stats(3)['datagrams_delivered'] < ule.models[1].stats(3)['datagrams']
    assert ule.models[1].stats(1)['sndus'] + ule.models[1].stats(1)['malformed_sndus'] > 0 and ule.models[1].stats(1)['datagrams'] == 0
