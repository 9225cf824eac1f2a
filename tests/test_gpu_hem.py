"""GPU tests of DVB-T2 high-efficiency-mode BBFRAMEs in the mode-adaptation mode (csrc/bbts_ma.hip with dvbs2gpu_bbts_ma_set_t2_hem on):
the kernels against the library's host parser and the receiver model of tests/hem_ref.py in bytes, every statistic and the state
through the next call, on small frames cut where the framing can go wrong; and the chain outer TS -> T2-MI bank -> this bank ->
monitor on the device, which delivers nothing with the switch off."""
import numpy as np
import pytest

import hem_ref as H
import ma_ref as M
import psi_ref as S
import t2mi_ref as T

pytestmark = pytest.mark.gpu

CARRIERS = H.carriers()


@pytest.fixture(scope='module')
def eng(pkg):
    return pkg.Engine(0)


def _dev(frames):
    import torch
    if not len(frames):
        return torch.zeros(4, dtype=torch.uint8, device='cuda')
    return torch.from_numpy(np.concatenate(frames)).cuda()


class Bank:
    """a device bank with the switch on; every stream has its own selection"""

    def __init__(self, pkg, eng, sels, max_frames=16, cap=1 << 18, kbch=58192, hem=True, gse=False, cfg=H.CFG):
        import torch
        self.eng, self.n, self.sels = eng, len(sels), sels
        self.bank = pkg.BbTsParserBank(eng, self.n, kbch, max_frames)
        self.bank.set_mode_adaptation(True, **cfg)
        for i, s in enumerate(sels):
            self.bank.select_isi(i, s)
        if gse:
            self.bank.ma_set_gse(True)
        if hem:
            self.bank.ma_set_t2_hem(True)
        self.launches = 3 if not gse else None                     # frame, lane and emit passes, whatever the bank size
        self.outs = [[torch.zeros(cap, dtype=torch.uint8, device='cuda') for _ in s] for s in sels]

    def run(self, per_stream_frames, ccm=False):
        k0 = self.eng.get_state('kernel_launches')
        nb = self.bank.process_ma([_dev(f) for f in per_stream_frames], self.outs,
                                  frame_bytes=None if ccm else [[x.size for x in f] for f in per_stream_frames])
        if self.launches:
            assert self.eng.get_state('kernel_launches') - k0 == self.launches
        return [[self.outs[i][k][:nb[i][k]].cpu().numpy() for k in range(len(self.sels[i]))] for i in range(self.n)]


def _host(pkg, sel, gse=False, kbch=58192, cfg=H.CFG):
    hb = pkg.BbTsParserBank.host(kbch, 16)
    hb.set_mode_adaptation(True, **cfg)
    hb.select_isi(0, sel)
    if gse:
        hb.ma_set_gse(True)
    hb.ma_set_t2_hem(True)
    return hb


def _same_stats(dv, stream, hb, rx, nsel):
    for j in range(nsel):
        a, b = rx.stats(j), dv.ma_stats(stream, j)
        assert {k: a[k] for k in H.STAT_KEYS} == {k: b[k] for k in H.STAT_KEYS}, (stream, j)
        assert hb is None or hb.ma_stats(0, j) == b, (stream, j)
    assert dv.isi_seen(stream) == sorted(rx.seen)


def _three_ways(pkg, eng, frames, sel, step, gse=False, kbch=58192, ccm=False, cfg=H.CFG):
    """device, host bank and model on the same calls: bytes and statistics after every call and after the flush"""
    rx, hb, dv = H.HemReceiver(sel, **cfg), _host(pkg, sel, gse, kbch, cfg), Bank(pkg, eng, [sel], gse=gse, kbch=kbch, cfg=cfg)
    total = 0
    for a in range(0, len(frames), step):
        want, host, got = rx.process(frames[a:a + step]), hb.ma_work(frames[a:a + step]), dv.run([frames[a:a + step]], ccm)[0]
        for j in range(len(sel)):
            assert got[j].size == want[j].size and np.array_equal(got[j], want[j]), (a, j)
            assert np.array_equal(host[j], want[j]), (a, j)
            total += want[j].size
        _same_stats(dv.bank, 0, hb, rx, len(sel))
    want, host, got = rx.flush(), hb.ma_flush()[0], dv.bank.ma_flush()[0]
    for j in range(len(sel)):
        assert np.array_equal(got[j], want[j]) and np.array_equal(host[j], want[j])
    _same_stats(dv.bank, 0, hb, rx, len(sel))
    hb.close()
    return rx, total


@pytest.mark.parametrize('name', sorted(CARRIERS))
def test_device_equals_host_parser_equals_model(pkg, eng, name):
    """what each carrier is for, and that it does occur, is in tests/hem_ref.py and tests/test_hem_cpu.py"""
    frames, sel = CARRIERS[name]
    assert len(frames) <= 16 and all(f.size <= 800 for f in frames)
    rx, total = _three_ways(pkg, eng, frames, sel, 3, gse='GSE' in name)
    assert total > 0 and rx.stats(0)['hem_frames'] > 0


def test_whole_slot_behind_a_no_start_frame_leaves_with_the_flush(pkg, eng):
    """the DNP as the last carried byte with no frame behind it: edge cuts up to the SYNCD = 65535 frame that completes the slot"""
    frames = CARRIERS['edge cuts'][0][:8]
    rx, _ = _three_ways(pkg, eng, frames, (0,), 8)
    assert rx.stats(0)['carried'] == 0


def test_dnp_is_ignored_without_reinsertion(pkg, eng):
    rx, total = _three_ways(pkg, eng, CARRIERS['edge cuts'][0], (0,), 4, cfg=dict(H.CFG, reinsert_nulls=0))
    assert rx.stats(0)['nulls'] == 0 and total == 188 * rx.stats(0)['packets'] > 0


@pytest.mark.parametrize('kbch,npd', [(7032, False), (58192, True)])
def test_ccm_sizes(pkg, eng, kbch, npd):
    """no size table: every frame kbch/8 bytes (the last one padded behind its DFL); 7274 bytes hold 38 slots, most of a wave"""
    rng = np.random.default_rng(kbch)
    fb = kbch // 8
    ts = M.make_ts(3 * (fb - 10) // 187, rng, null_runs=npd)
    frames = H.frames_of_stream(H.slot_stream(ts, npd), H.slot_len(npd), [fb - 10], sis=True, issyi=True, npd=npd, frame_bytes=fb)
    assert 3 <= len(frames) <= 4
    rx, total = _three_ways(pkg, eng, frames, (0,), 2, kbch=kbch, ccm=True)
    assert total == ts.size and rx.stats(0)['broken_joins'] == 0


@pytest.mark.parametrize('cuts', ['one', 'ragged', 'all'])
def test_calls_cut_anywhere_give_the_same_output(pkg, eng, cuts):
    frames, ts, sel = H.random_carrier(9, True, True, mis=True)
    rng = np.random.default_rng(2)
    dv = Bank(pkg, eng, [sel])
    outs, a = [[] for _ in sel], 0
    while a < len(frames):
        n = {'one': 1, 'ragged': int(rng.integers(0, 5)), 'all': len(frames)}[cuts]
        got = dv.run([frames[a:a + n]])[0]
        for j in range(len(sel)):
            outs[j].append(got[j])
        a += n
    _, want = H.run_model(frames, sel, H.CFG, step=len(frames))
    fl = dv.bank.ma_flush()[0]
    for j, isi in enumerate(sel):
        got = np.concatenate(outs[j] + [fl[j]])
        assert np.array_equal(got, want[j]) and np.array_equal(got, ts[isi].reshape(-1)[:got.size]) and got.size > 0


def test_capacity_error_leaves_state_and_output_untouched(pkg, eng):
    import torch
    frames, sel = CARRIERS['random seed 3 npd 1 issyi 0 mis 1']
    a, b = Bank(pkg, eng, [sel]), Bank(pkg, eng, [sel])
    assert all(np.array_equal(x, y) for x, y in zip(a.run([frames[:3]])[0], b.run([frames[:3]])[0]))
    small = [[torch.full((188,), 0x5a, dtype=torch.uint8, device='cuda') for _ in sel]]
    before = [a.bank.ma_stats(0, j) for j in range(len(sel))]
    rest = frames[3:]
    with pytest.raises(pkg.Dvbs2GpuError) as e:
        a.bank.process_ma([_dev(rest)], small, frame_bytes=[[x.size for x in rest]])
    assert e.value.code == -5
    assert [a.bank.ma_stats(0, j) for j in range(len(sel))] == before
    assert all(bool((t == 0x5a).all()) for t in small[0])
    want = b.run([rest])[0]
    assert e.value.needed[0][:len(sel)] == [w.size for w in want] and max(e.value.needed[0]) > 188
    got = a.run([rest])[0]
    assert all(np.array_equal(x, y) for x, y in zip(got, want))
    assert [a.bank.ma_stats(0, j) for j in range(len(sel))] == [b.bank.ma_stats(0, j) for j in range(len(sel))]


def test_sixty_four_streams_equal_single_stream_banks(pkg, eng):
    S64 = 64
    names = sorted(CARRIERS)
    sc = []
    for i in range(S64):
        if i % 3 == 2:
            sc.append(CARRIERS[names[(i // 3) % len(names)]])
        else:
            frames, _, sel = H.random_carrier(100 + i, bool(i & 1), bool(i & 2), mis=bool(i & 4), nframes=8 + i % 5)
            sc.append((frames, sel if i % 5 else sel[::-1]))
    many = Bank(pkg, eng, [s[1] for s in sc], max_frames=4)
    ones = [Bank(pkg, eng, [s[1]], max_frames=4) for s in sc]
    pos = [0] * S64
    rng = np.random.default_rng(5)
    while any(pos[i] < len(sc[i][0]) for i in range(S64)):
        take = [int(rng.integers(0, 5)) for _ in range(S64)]
        call = [sc[i][0][pos[i]:pos[i] + take[i]] for i in range(S64)]
        pos = [pos[i] + take[i] for i in range(S64)]
        got = many.run(call)
        for i in range(S64):
            if take[i] and call[i]:
                alone = ones[i].run([call[i]])[0]
                assert all(np.array_equal(x, y) for x, y in zip(got[i], alone)), i
    for i in range(S64):
        assert [many.bank.ma_stats(i, j) for j in range(len(sc[i][1]))] == [ones[i].bank.ma_stats(0, j) for j in range(len(sc[i][1]))], i
    assert sum(many.bank.ma_stats(i, 0)['hem_frames'] for i in range(S64)) > 100


def test_normal_mode_results_do_not_depend_on_the_switch(pkg, eng):
    frames, ts, sel, cfg = M.scenario(2, True, 'auto', True, True, npk=30, damage=(3,))
    a, b = Bank(pkg, eng, [sel], max_frames=64, cap=1 << 18, hem=False), Bank(pkg, eng, [sel], max_frames=64, cap=1 << 18, hem=True)
    x, y = a.run([frames])[0], b.run([frames])[0]
    assert all(np.array_equal(p, q) and p.size > 0 for p, q in zip(x, y))
    assert [a.bank.ma_stats(0, j) for j in range(2)] == [b.bank.ma_stats(0, j) for j in range(2)]


@pytest.mark.parametrize('hem', [True, False])
def test_end_to_end_chained_on_the_device(pkg, eng, hem):
    """outer TS -> T2-MI -> HEM BBFRAMEs -> inner TS -> monitor, all in HBM.  With the switch off every frame is rejected and nothing
    comes out: what the chain did before the switch existed."""
    import torch
    rng = np.random.default_rng(21)
    kbch = {3: 7032, 5: 13152}                                       # two PLPs with short-frame T2 sizes
    inner = {plp: M.make_ts(60, rng, null_runs=False) for plp in kbch}
    for ts in inner.values():                                        # orderly headers for the monitor: three PIDs, payload only, counters in step
        for i, p in enumerate(ts):
            p[1], p[2], p[3] = (p[1] & 0x40) | 0x01, i % 3, 0x10 | (i // 3 & 15)
    frames = {plp: H.frames_of_stream(H.slot_stream(inner[plp]), 187, [kbch[plp] // 8 - 10], isi=plp, issyi=True, frame_bytes=kbch[plp] // 8) for plp in kbch}
    order = [plp for i in range(max(len(f) for f in frames.values())) for plp in kbch if i < len(frames[plp])]
    at, pk, count = dict.fromkeys(kbch, 0), [], 40
    for i, plp in enumerate(order):
        count = (count + 1) & 255
        pk.append(T.bb_packet(count, plp, bytes(frames[plp][at[plp]]), frame_idx=i))
        at[plp] += 1
        if i % 3 == 0:                                               # an L1-type packet between
            count = (count + 1) & 255
            pk.append(T.t2mi_packet(0x10, count, bytes(rng.integers(0, 256, 60, dtype=np.uint8))))
    t2 = T.Packetiser(0x1000).lay(pk)
    outer = S.interleave(rng, [t2, S.filler(0x31, len(t2) // 10, rng)])
    bank = pkg.T2miBank(eng, 1, 1024, 128)
    bank.set_watch(0, 0, 0x1000, 3), bank.set_watch(0, 1, 0x1000, 5)
    bb = [torch.zeros(len(outer) * 188, dtype=torch.uint8, device='cuda') for _ in range(2)]
    buf = torch.zeros(outer.size + 8, dtype=torch.uint8, device='cuda')
    buf[:outer.size] = torch.from_numpy(np.ascontiguousarray(outer).reshape(-1)).cuda()
    nb = bank.process([buf], [bb], nbytes=[outer.size])[0]
    st = bank.stats(0)
    assert st['crc_errors'] == st['count_errors'] == st['dropped_packets'] == 0
    mon = pkg.TsMonitorBank(eng, 1, 1024)
    for k, plp in enumerate(kbch):
        sizes = bank.frame_bytes(0, k)
        assert sizes == [kbch[plp] // 8] * len(frames[plp]) and nb[k] == sum(sizes)
        ma = pkg.BbTsParserBank(eng, 1, kbch[plp], len(sizes))
        ma.set_mode_adaptation(True)
        ma.select_isi(0, (plp,))
        if hem:
            ma.ma_set_t2_hem(True)
        ts_dev = torch.zeros(nb[k] + 376, dtype=torch.uint8, device='cuda')
        n = ma.process_ma([bb[k]], [[ts_dev]], frame_bytes=[sizes])[0][0]
        ms = ma.ma_stats(0, 0)
        if not hem:
            assert n == 0 and ms['rejected_frames'] == len(sizes) and ms['frames'] == 0
            continue
        assert n == inner[plp].size and np.array_equal(ts_dev[:n].cpu().numpy(), inner[plp].reshape(-1))
        assert (ms['hem_frames'], ms['rejected_frames'], ms['broken_joins'], ms['iscr_valid']) == (len(sizes), 0, 0, 1)
        mon.reset()
        mon.process([ts_dev], nbytes=[n])
        assert mon.stats(0)['cc_errors'] == 0 and mon.stats(0)['sync_byte_errors'] == 0 and mon.stats(0)['packets'] == n // 188
