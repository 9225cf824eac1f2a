"""GPU tests of GSE decapsulation in the mode-adaptation bank (csrc/bbts_ma.hip): the kernels against the library's host bank and the
receiver model of tests/ma_gse_ref.py, byte for byte: outputs, byte counts, PDU table rows and every counter."""
import numpy as np
import pytest

import ma_gse_ref as G
import ma_ref as M
import orc_bbts as B

pytestmark = pytest.mark.gpu

CFG = {'issy_bytes': 0, 'crc_span': 0, 'reinsert_nulls': 1, 'check_crc': 1}


@pytest.fixture(scope='module')
def eng(pkg):
    return pkg.Engine(0)


def _dev(frames):
    import torch
    if not len(frames):
        return torch.zeros(4, dtype=torch.uint8, device='cuda')
    return torch.from_numpy(np.concatenate(frames)).cuda()


class Bank:
    """a device bank whose streams each have their own frames and selection"""

    def __init__(self, pkg, eng, sels, max_frames=48, cap=1 << 18, gse=True):
        import torch
        self.n, self.sels, self.cap = len(sels), sels, cap
        self.bank = pkg.BbTsParserBank(eng, self.n, 58192, max_frames)
        self.bank.set_mode_adaptation(True, **CFG)
        for i, s in enumerate(sels):
            self.bank.select_isi(i, s)
        if gse:
            self.bank.ma_set_gse(True)
        self.buf = torch.zeros((sum(len(s) for s in sels), cap), dtype=torch.uint8, device='cuda')
        rows = iter(self.buf)
        self.outs = [[next(rows) for _ in s] for s in sels]

    def run(self, per_stream_frames):
        nb = self.bank.process_ma([_dev(f) for f in per_stream_frames], self.outs, frame_bytes=[[x.size for x in f] for f in per_stream_frames])
        host = self.buf.cpu().numpy()
        k, res = 0, []
        for i in range(self.n):
            res.append([host[k + j, :nb[i][j]].copy() for j in range(len(self.sels[i]))])
            k += len(self.sels[i])
        return res


def host_bank(pkg, sel, gse=True, max_frames=48):
    hb = pkg.BbTsParserBank.host(58192, max_frames)
    hb.set_mode_adaptation(True, **CFG)
    hb.select_isi(0, sel)
    if gse:
        hb.ma_set_gse(True)
    return hb


def same_lane(bank, stream, rx, j, fallback=0):
    a, b = rx.stats(j), bank.ma_stats(stream, j)
    assert {k: a[k] for k in M.STAT_KEYS} == {k: b[k] for k in M.STAT_KEYS}, (stream, j)
    a, b = rx.gse_stats(j), bank.ma_gse_stats(stream, j)
    assert a == {k: b[k] for k in G.GSE_KEYS}, (stream, j)
    assert b['host_fallback_calls'] == fallback, (stream, j)


def three_ways(pkg, eng, frames, sel, cuts, fallback=0):
    """the frames through a device bank, a host bank and the model, cut into calls at `cuts`; all three equal in bytes, rows and
    counters -> (model, the lanes' concatenated outputs)"""
    rx, hb, dv = G.Receiver(sel, **CFG), host_bank(pkg, sel), Bank(pkg, eng, [sel])
    outs = [[] for _ in sel]
    for a, b in zip([0] + list(cuts), list(cuts) + [len(frames)]):
        want, host, got = rx.process(frames[a:b]), hb.ma_work(frames[a:b]), dv.run([frames[a:b]])[0]
        for j in range(len(sel)):
            assert got[j].size == want[j].size and np.array_equal(got[j], want[j]), (a, j)
            assert np.array_equal(host[j], want[j]), (a, j)
            assert dv.bank.ma_pdu_table(0, j) == rx.rows(j) == hb.ma_pdu_table(0, j), (a, j)
            outs[j].append(want[j])
    for j in range(len(sel)):
        same_lane(dv.bank, 0, rx, j, fallback)
        same_lane(hb, 0, rx, j)
    assert dv.bank.isi_seen(0) == sorted(rx.seen)
    hb.close()
    return rx, [np.concatenate(o) for o in outs]


@pytest.mark.parametrize('seed,mis,mixed,nisi,with_ts', G.GRID)
def test_device_equals_host_bank_equals_model(pkg, eng, seed, mis, mixed, nisi, with_ts):
    frames, carries, sel = G.scenario(seed, mis, mixed, nisi, with_ts)
    assert len(frames) <= 48
    if mixed:
        assert {384, 7274} <= {f.size for f in frames}
    frames = list(frames)
    frames[3] = frames[3].copy()
    frames[3][4] ^= 0x40                                           # one header fails its CRC-8
    step = 1 + 2 * (seed % 3)
    rx, _ = three_ways(pkg, eng, frames, sel, range(step, len(frames), step))
    assert sum(rx.gse_stats(j)['reassembled_pdus'] for j in range(len(sel))) > 0


@pytest.mark.parametrize('cuts', ['one', 'ragged', 'all'])
def test_calls_cut_anywhere_give_the_same_output(pkg, eng, cuts):
    frames, carries, sel = G.scenario(6, True, True, 2, True)
    rng = np.random.default_rng(2)
    dv = Bank(pkg, eng, [sel])
    outs, pdus, a = [[] for _ in sel], [[] for _ in sel], 0
    while a < len(frames):
        n = {'one': 1, 'ragged': int(rng.integers(0, 9)), 'all': len(frames)}[cuts]
        got = dv.run([frames[a:a + n]])[0]
        for j in range(len(sel)):
            outs[j].append(got[j])
            pdus[j] += G.split_output(got[j], dv.bank.ma_pdu_table(0, j))[0]
        a += n
    want = G.Receiver(sel, **CFG).process(frames)                   # the whole sequence as one call of the model
    for j, isi in enumerate(sel):
        assert np.array_equal(np.concatenate(outs[j]), want[j])
        assert [(p, b) for p, b, _ in pdus[j]] == [(p, G.gre(p, d)) for p, d, _ in carries[isi]['gse']]


def test_sixty_four_streams_equal_single_stream_banks(pkg, eng):
    S = 64
    sc = [G.scenario(100 + i, *G.GRID[i % len(G.GRID)][1:], npdus=6 + i % 4) for i in range(S)]
    sels = [s[2] if i % 3 else s[2][::-1] for i, s in enumerate(sc)]
    dv = Bank(pkg, eng, sels, max_frames=8, cap=1 << 16)
    hbs = [host_bank(pkg, sels[i], max_frames=8) for i in range(S)]
    pos, rng = [0] * S, np.random.default_rng(5)
    while any(pos[i] < len(sc[i][0]) for i in range(S)):
        take = [int(rng.integers(0, 9)) for _ in range(S)]
        call = [sc[i][0][pos[i]:pos[i] + take[i]] for i in range(S)]
        pos = [pos[i] + take[i] for i in range(S)]
        got = dv.run(call)
        for i in range(S):
            want = hbs[i].ma_work(call[i])
            for j in range(len(sels[i])):
                assert np.array_equal(got[i][j], want[j]), (i, j)
                assert dv.bank.ma_pdu_table(i, j) == hbs[i].ma_pdu_table(0, j), (i, j)
    for i in range(S):
        for j in range(len(sels[i])):
            assert dv.bank.ma_stats(i, j) == hbs[i].ma_stats(0, j) and dv.bank.ma_gse_stats(i, j) == hbs[i].ma_gse_stats(0, j), (i, j)
        hbs[i].close()


def _pdu(rng, n):
    return bytes(rng.integers(0, 256, n, dtype=np.uint8))


def test_corrupted_end_is_counted_delivers_nothing_and_frees_its_slot(pkg, eng):
    rng = np.random.default_rng(1)
    s1, rest = G.start_packet(9, 0x0800, _pdu(rng, 900), 300)
    bad = rest[:-1] + bytes([rest[-1] ^ 1])
    m1, bad = G.next_packet(9, bad, 200)
    e1, _ = G.next_packet(9, bad, len(bad))
    s2, rest2 = G.start_packet(9, 0x86DD, _pdu(rng, 500), 100, lt=0, label=b'abcdef')
    e2, _ = G.next_packet(9, rest2, len(rest2))
    frames = [G.gse_frame(s1 + m1, 1779, sis=True), G.gse_frame(e1 + s2, 7274, sis=True), G.gse_frame(e2, 1779, sis=True)]
    for cuts in ([], [1, 2]):
        rx, out = three_ways(pkg, eng, frames, (0,), cuts)
        g = rx.gse_stats(0)
        assert (g['crc_failures'], g['reassembled_pdus'], g['open_slots'], g['last_crc_err']) == (1, 1, 0, 0)
        assert out[0].size == 4 + 500


def test_fourth_open_pdu_is_dropped_and_counted(pkg, eng):
    rng = np.random.default_rng(2)
    st = [G.start_packet(i, 0x0806, _pdu(rng, 300 + i), 100) for i in (1, 2, 3, 4)]
    ends = [G.next_packet(i, r, len(r))[0] for i, (_, r) in zip((1, 2, 3, 4), st)]
    frames = [G.gse_frame(b''.join(p for p, _ in st), 1779, sis=True), G.gse_frame(b''.join(reversed(ends)), 1779, sis=True)]
    for cuts in ([], [1]):
        rx, out = three_ways(pkg, eng, frames, (0,), cuts)
        g = rx.gse_stats(0)
        assert (g['dropped_no_slot'], g['reassembled_pdus'], g['packets'], g['open_slots']) == (1, 3, 8, 0)


def test_fragment_past_64k_frees_the_slot(pkg, eng):
    rng = np.random.default_rng(3)
    data = _pdu(rng, 70000)
    pkts, rest = [G.start_packet(5, 0x0800, data[:60000], 4000)[0]], data[4000:]
    while len(rest) > 4000:
        p, rest = G.next_packet(5, rest, 4094)
        pkts.append(p)
    pkts.append(G.next_packet(5, rest, len(rest))[0])               # an END for a slot that is gone: ignored
    s2, r2 = G.start_packet(5, 0x0800, _pdu(rng, 50), 10)
    pkts.append(s2 + G.next_packet(5, r2, len(r2))[0])
    frames = [G.gse_frame(p, 7274 if k % 2 else 4200, sis=True) for k, p in enumerate(pkts)]
    assert len(frames) <= 48
    rx, out = three_ways(pkg, eng, frames, (0,), [7, 8, 16])
    g = rx.gse_stats(0)
    assert (g['dropped_overflow'], g['reassembled_pdus'], g['crc_failures'], g['open_slots']) == (1, 1, 0, 0)


def test_malformed_length_ends_its_frame_only(pkg, eng):
    rng = np.random.default_rng(4)
    good = [G.complete_packet(0x0800, _pdu(rng, 40 + k)) for k in range(4)]
    short_start = G.header(1, 0, 0, 8) + bytes(8)                   # START with a 6-byte label needs 11 bytes
    short_end = G.header(0, 1, 3, 4) + bytes(4)                     # an END shorter than frag id + CRC-32
    beyond = G.header(1, 1, 2, 600) + bytes(100)                    # passes the end of the data field
    frames = [G.gse_frame(good[0] + short_start + good[1], 384, sis=True), G.gse_frame(good[2] + short_end, 384, sis=True),
              G.gse_frame(good[3] + beyond, 384, sis=True, dfl_bytes=len(good[3]) + 102), G.gse_frame(good[1] + b'\x81', 384, sis=True, dfl_bytes=len(good[1]) + 1)]
    rx, out = three_ways(pkg, eng, frames, (0,), [2])
    g = rx.gse_stats(0)
    assert (g['malformed_frames'], g['complete_pdus'], g['frames']) == (4, 4, 4)


def test_more_than_256_packets_take_the_host_fallback(pkg, eng):
    rng = np.random.default_rng(5)
    s1, rest = G.start_packet(3, 0x0800, _pdu(rng, 2000), 500)
    m1, rest = G.next_packet(3, rest, 700)
    e1, _ = G.next_packet(3, rest, len(rest))
    tiny = b''.join(G.complete_packet(0x1234 + k, b'') for k in range(300))
    assert len(tiny) == 300 * 4
    ts = M.make_ts(12, rng, null_runs=False)
    tsf = [f for f, _ in M.frames_of_stream(M.slot_stream(ts)[0], 188, [3072], sis=True)]
    frames = [G.gse_frame(s1, 1779, sis=True), tsf[0], G.gse_frame(tiny[:400] + m1 + tiny[400:], 7274, sis=True), tsf[1], G.gse_frame(e1, 1779, sis=True)] + tsf[2:]
    rx, out = three_ways(pkg, eng, frames, (0,), [1, 4], fallback=1)
    g = rx.gse_stats(0)
    assert (g['complete_pdus'], g['reassembled_pdus'], g['open_slots']) == (300, 1, 0)


def _capacity_case(pkg, eng, frames, sel, cut, fallback=0):
    """frames[:cut] as one call, then frames[cut:] with buffers that are too small: the error leaves TS and GSE state, slot buffers
    and table as they were, needed[] has the host bank's sizes (GRE bytes included), and the repeated call equals the host bank"""
    import torch
    dv, hb = Bank(pkg, eng, [sel]), host_bank(pkg, sel)
    first, hfirst = dv.run([frames[:cut]])[0], hb.ma_work(frames[:cut])
    assert all(np.array_equal(x, y) for x, y in zip(first, hfirst))
    assert any(dv.bank.ma_gse_stats(0, j)['open_slots'] for j in range(len(sel)))       # the slot buffers hold bytes the rest needs
    before = [(dv.bank.ma_stats(0, j), dv.bank.ma_gse_stats(0, j)) for j in range(len(sel))]
    rest = frames[cut:]
    small = [[torch.zeros(64, dtype=torch.uint8, device='cuda') for _ in sel]]
    with pytest.raises(pkg.Dvbs2GpuError) as e:
        dv.bank.process_ma([_dev(rest)], small, frame_bytes=[[x.size for x in rest]])
    assert e.value.code == -5
    assert [(dv.bank.ma_stats(0, j), dv.bank.ma_gse_stats(0, j)) for j in range(len(sel))] == before
    assert all(dv.bank.ma_pdu_table(0, j) == [] for j in range(len(sel)))
    want = hb.ma_work(rest)
    assert e.value.needed[0][:len(sel)] == [w.size for w in want[:len(sel)]] and max(e.value.needed[0]) > 64
    assert sum(len(hb.ma_pdu_table(0, j)) for j in range(len(sel))) > 0                 # GRE bytes are part of those sizes
    got = dv.run([rest])[0]
    for j in range(len(sel)):
        assert np.array_equal(got[j], want[j]), j
        assert dv.bank.ma_pdu_table(0, j) == hb.ma_pdu_table(0, j)
        a, b = dv.bank.ma_gse_stats(0, j), hb.ma_gse_stats(0, j)
        assert {k: a[k] for k in G.GSE_KEYS} == {k: b[k] for k in G.GSE_KEYS} and a['host_fallback_calls'] == fallback
        assert dv.bank.ma_stats(0, j) == hb.ma_stats(0, j)
    hb.close()


def test_capacity_error_leaves_ts_and_gse_state_on_the_device(pkg, eng):
    frames, carries, sel = G.scenario(6, True, True, 2, True)
    _capacity_case(pkg, eng, frames, sel, 7)


def test_capacity_error_with_a_stream_in_the_host_fallback(pkg, eng):
    rng = np.random.default_rng(9)
    s1, rest = G.start_packet(3, 0x0800, _pdu(rng, 2000), 500)
    m1, rest = G.next_packet(3, rest, 700)
    e1, _ = G.next_packet(3, rest, len(rest))
    tiny = b''.join(G.complete_packet(0x1234 + k, b'') for k in range(300))
    frames = [G.gse_frame(s1, 1779, sis=True), G.gse_frame(tiny[:400] + m1 + tiny[400:], 7274, sis=True), G.gse_frame(e1, 1779, sis=True)]
    _capacity_case(pkg, eng, frames, (0,), 1, fallback=1)


def test_reselection_keeps_the_other_streams_open_pdus(pkg, eng):
    """stream 0 has a PDU open in the slot pool when stream 1 is given more ISIs than the pool has places for: the pool grows, stream 0's
    bytes move with it and its PDU completes; stream 1 starts afresh on its new lanes"""
    rng = np.random.default_rng(10)
    pdu0, pdu1 = _pdu(rng, 3000), _pdu(rng, 700)
    s0, rest = G.start_packet(1, 0x0800, pdu0, 1000)
    m0, rest = G.next_packet(1, rest, 1200)
    e0, _ = G.next_packet(1, rest, len(rest))
    s1, rest1 = G.start_packet(1, 0x86DD, pdu1, 300)
    e1, _ = G.next_packet(1, rest1, len(rest1))
    f = lambda p, isi: G.gse_frame(p, 1779, isi)
    dv = Bank(pkg, eng, [(5,), (5,)], max_frames=4)
    got = dv.run([[f(s0, 5)], [f(s1, 5)]])                           # the first GSE frames: the pool gets its two places
    assert [g[0].size for g in got] == [0, 0]
    assert dv.bank.ma_gse_stats(0, 0)['open_slots'] == 1 and dv.bank.ma_gse_stats(1, 0)['open_slots'] == 1
    dv.bank.select_isi(1, (200, 17, 5, 9))                           # four lanes where there was one
    assert dv.bank.ma_gse_stats(1, 2)['open_slots'] == 0 and dv.bank.ma_gse_stats(0, 0)['open_slots'] == 1
    import torch
    outs = [[torch.zeros(1 << 14, dtype=torch.uint8, device='cuda')], [torch.zeros(1 << 14, dtype=torch.uint8, device='cuda') for _ in range(4)]]
    call = [[f(m0, 5), f(e0, 5)], [f(e1, 5), f(s1, 17), f(s1, 9), f(e1, 9)]]       # stream 1: the END of a PDU that is gone, then new ones
    nb = dv.bank.process_ma([_dev(c) for c in call], outs, frame_bytes=[[x.size for x in c] for c in call])
    assert nb[0][0] == 4 + 3000 and bytes(outs[0][0][:nb[0][0]].cpu().numpy()) == G.gre(0x0800, pdu0)
    assert nb[1][:4] == [0, 0, 0, 4 + 700] and bytes(outs[1][3][:nb[1][3]].cpu().numpy()) == G.gre(0x86DD, pdu1)
    assert dv.bank.ma_gse_stats(1, 1)['open_slots'] == 1 and dv.bank.ma_gse_stats(1, 2)['reassembled_pdus'] == 0
    dv.bank.select_isi(0, (5, 200))                                  # back and forth: places return to the free list and are reused
    dv.bank.select_isi(1, (17,))
    nb = dv.bank.process_ma([_dev([f(s0, 200), f(m0, 200), f(e0, 200)]), _dev([f(s1, 17), f(e1, 17)])], [[outs[0][0], outs[1][1]], [outs[1][0]]],
                            frame_bytes=[[1779] * 3, [1779] * 2])
    assert nb[0][:2] == [0, 4 + 3000] and nb[1][0] == 4 + 700
    assert bytes(outs[1][1][:nb[0][1]].cpu().numpy()) == G.gre(0x0800, pdu0) and bytes(outs[1][0][:nb[1][0]].cpu().numpy()) == G.gre(0x86DD, pdu1)


def test_isis_keep_their_own_slots(pkg, eng):
    rng = np.random.default_rng(6)
    fr = {}
    for isi in (5, 200):
        s, rest = G.start_packet(7, 0x0800, _pdu(rng, 1500 + isi), 400)         # the same frag id on both
        m, rest = G.next_packet(7, rest, 500)
        e, _ = G.next_packet(7, rest, len(rest))
        fr[isi] = [G.gse_frame(p, 1779, isi) for p in (s, m, e)]
    other = G.gse_frame(G.start_packet(7, 0x0800, _pdu(rng, 99), 9)[0], 384, 9)   # not selected
    frames = [fr[5][0], fr[200][0], other, fr[200][1], fr[5][1], fr[5][2], other, fr[200][2]]
    rx, out = three_ways(pkg, eng, frames, (200, 5), [3, 4])
    for j, isi in enumerate((200, 5)):
        g = rx.gse_stats(j)
        assert (g['reassembled_pdus'], g['crc_failures'], g['open_slots']) == (1, 0, 0) and out[j].size == 4 + 1500 + isi
    assert rx.skipped == 2


def test_switch_off_skips_gse_frames(pkg, eng):
    frames, carries, sel = G.scenario(6, True, True, 2, True)
    dv, rx = Bank(pkg, eng, [sel], gse=False), G.Receiver(sel, gse=False, **CFG)
    want, got = rx.process(frames), dv.run([frames])[0]
    for j in range(len(sel)):
        assert np.array_equal(got[j], want[j])
        a, b = rx.stats(j), dv.bank.ma_stats(0, j)
        assert {k: a[k] for k in M.STAT_KEYS} == {k: b[k] for k in M.STAT_KEYS}
        assert dv.bank.ma_gse_stats(0, j)['frames'] == 0 and dv.bank.ma_pdu_table(0, j) == []
    assert rx.skipped >= sum(len(c['gse']) > 0 for c in carries.values())
    # on, and off again: the open reassemblies are gone and the frames are skipped again
    on = Bank(pkg, eng, [sel])
    on.run([frames[:9]])
    assert any(on.bank.ma_gse_stats(0, j)['open_slots'] for j in range(len(sel)))
    on.bank.ma_set_gse(False)
    assert all(on.bank.ma_gse_stats(0, j) == dv.bank.ma_gse_stats(0, j) for j in range(len(sel)))
    before = on.bank.ma_stats(0, 0)['skipped_frames']
    on.run([frames[9:]])
    assert on.bank.ma_stats(0, 0)['skipped_frames'] > before and on.bank.ma_gse_stats(0, 0)['frames'] == 0


def test_reference_mode_bank_gives_the_same_bytes_and_rows(pkg, eng):
    """SIS, CCM, label types 00 and 10 only, SYNCD 0 and a first frame of pure padding: no quirk of the reference mode fires, so
    process_batch of a reference-mode bank and lane 0 of the mode-adaptation bank agree in bytes and rows, call by call"""
    import torch
    rng = np.random.default_rng(7)
    kbch = 14232
    gf, sent = G.gse_frames(rng, 0, [kbch // 8], 30, sis=True, lts=(0, 2))
    frames = [G.gse_frame(b'', kbch // 8, sis=True)] + gf
    for f in frames:
        f[0] |= 0x10                                                # CCM
        f[9] = B.crc8(f[:9])
    ref = pkg.BbTsParserBank(eng, 1, kbch, 16)
    ma = pkg.BbTsParserBank(eng, 1, kbch, 16)
    ma.set_mode_adaptation(True, **CFG)
    ma.ma_set_gse(True)
    out_r = torch.zeros(1 << 17, dtype=torch.uint8, device='cuda')
    out_m = torch.zeros(1 << 17, dtype=torch.uint8, device='cuda')
    total = 0
    for a in range(0, len(frames), 5):
        bb = _dev(frames[a:a + 5])
        nr = ref.process_batch([bb], [out_r])[0]
        nm = ma.process_ma([bb], [[out_m]])[0][0]
        assert nr == nm and torch.equal(out_r[:nr], out_m[:nm])
        assert ref.pdu_table(0) == ma.ma_pdu_table(0, 0)
        p, n = ma.ma_pdu_table_device(0, 0)
        assert n == len(ma.ma_pdu_table(0, 0)) and (p is not None) == (n > 0)
        total += len(ref.pdu_table(0))
    assert total == len(sent) and ref.gse_stats(0)['host_fallback_calls'] == 0
    a, b = ref.gse_stats(0), ma.ma_gse_stats(0, 0)
    assert all(a[k] == b[k] for k in G.GSE_KEYS[:9])


def test_4096_streams_in_one_call(pkg, eng):
    """the largest bank: 4096 streams x 2 frames; every stream equals the host bank of its pattern"""
    import torch
    S, rng = 4096, np.random.default_rng(8)
    pats = []
    for k in range(4):
        s, rest = G.start_packet(k, 0x0800, _pdu(rng, 300 + k), 120)
        e, _ = G.next_packet(k, rest, len(rest))
        c = G.complete_packet(0x86DD, _pdu(rng, 60 + k), 1, b'xyz')
        pats.append([G.gse_frame(c + s, 384, 5), G.gse_frame(e + c, 384, 5) if k % 2 else G.gse_frame(c + s, 384, 200)])
    want = []
    for p in pats:
        hb = host_bank(pkg, (5, 200))
        want.append((hb.ma_work(p), [hb.ma_pdu_table(0, j) for j in range(2)], [hb.ma_gse_stats(0, j) for j in range(2)]))
        hb.close()
    bank = pkg.BbTsParserBank(eng, S, 3072, 2)
    bank.set_mode_adaptation(True, **CFG)
    for i in range(S):
        bank.select_isi(i, (5, 200))
    bank.ma_set_gse(True)
    inp = torch.from_numpy(np.stack([np.concatenate(pats[i % 4]) for i in range(S)])).cuda()
    out = torch.zeros((S, 2, 1024), dtype=torch.uint8, device='cuda')
    nb = bank.process_ma([inp[i] for i in range(S)], [[out[i, 0], out[i, 1]] for i in range(S)])
    host = out.cpu().numpy()
    for i in range(S):
        w = want[i % 4]
        for j in range(2):
            assert nb[i][j] == w[0][j].size and np.array_equal(host[i, j, :nb[i][j]], w[0][j]), (i, j)
    for i in (0, 1, 2, 3, 2047, 4094, 4095):
        for j in range(2):
            assert bank.ma_pdu_table(i, j) == want[i % 4][1][j] and bank.ma_gse_stats(i, j) == want[i % 4][2][j]
