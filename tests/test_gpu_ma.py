"""GPU tests of the mode-adaptation mode of the BBFRAME -> TS bank (csrc/bbts_ma.hip): the kernels against the library's host parser
and the receiver model of tests/ma_ref.py, byte for byte: outputs, byte counts and every statistic."""
import json
import os

import numpy as np
import pytest

import ma_ref as M
import orc_bbts as B

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope='module')
def eng(pkg):
    return pkg.Engine(0)


def _dev(frames):
    import torch
    if not len(frames):
        return torch.zeros(4, dtype=torch.uint8, device='cuda')
    return torch.from_numpy(np.concatenate(frames)).cuda()


class Bank:
    """a device bank whose streams each have their own frames, selection and model"""

    def __init__(self, pkg, eng, sels, cfg, max_frames=64, cap=1 << 18):
        import torch
        self.n, self.sels, self.cap = len(sels), sels, cap
        self.bank = pkg.BbTsParserBank(eng, self.n, 58192, max_frames)
        self.bank.set_mode_adaptation(True, **cfg)
        for i, s in enumerate(sels):
            self.bank.select_isi(i, s)
        self.outs = [[torch.zeros(cap, dtype=torch.uint8, device='cuda') for _ in s] for s in sels]

    def run(self, per_stream_frames):
        nb = self.bank.process_ma([_dev(f) for f in per_stream_frames], self.outs, frame_bytes=[[x.size for x in f] for f in per_stream_frames])
        return [[self.outs[i][k][:nb[i][k]].cpu().numpy() for k in range(len(self.sels[i]))] for i in range(self.n)]


def _same_stats(bank, stream, rx, nsel):
    for j in range(nsel):
        a, b = rx.stats(j), bank.ma_stats(stream, j)
        assert {k: a[k] for k in M.STAT_KEYS} == {k: b[k] for k in M.STAT_KEYS}, (stream, j)
    assert bank.isi_seen(stream) == sorted(rx.seen)


def _damaged(frames):
    frames = list(frames)
    frames[3] = frames[3].copy()
    frames[3][4] ^= 0x40                                           # one header fails its CRC-8
    return frames


@pytest.mark.parametrize('seed,mis,issy_mode,npd,mixed', M.GRID)
def test_device_equals_host_parser_equals_model(pkg, eng, seed, mis, issy_mode, npd, mixed):
    frames, ts, sel, cfg = M.scenario(seed, mis, issy_mode, npd, mixed, span=seed % 2, damage=(7, 30))
    frames = _damaged(frames)
    rx = M.Receiver(sel, **cfg)
    hb = pkg.BbTsParserBank.host(58192, 64)
    hb.set_mode_adaptation(True, **cfg)
    hb.select_isi(0, sel)
    dv = Bank(pkg, eng, [sel], cfg)
    step = 3 + seed
    for a in range(0, len(frames), step):
        want, host, got = rx.process(frames[a:a + step]), hb.ma_work(frames[a:a + step]), dv.run([frames[a:a + step]])[0]
        for j in range(len(sel)):
            assert got[j].size == want[j].size and np.array_equal(got[j], want[j]), (a, j)
            assert np.array_equal(host[j], want[j]), (a, j)
    _same_stats(dv.bank, 0, rx, len(sel))
    want, host, got = rx.flush(), hb.ma_flush()[0], dv.bank.ma_flush()[0]
    for j in range(len(sel)):
        assert np.array_equal(got[j], want[j]) and np.array_equal(host[j], want[j])
    _same_stats(dv.bank, 0, rx, len(sel))
    _same_stats(hb, 0, rx, len(sel))


@pytest.mark.parametrize('cuts', ['one', 'ragged', 'all'])
def test_calls_cut_anywhere_give_the_same_output(pkg, eng, cuts):
    frames, ts, sel, cfg = M.scenario(11, True, 'auto', True, True, npk=150)
    assert len(frames) <= 64
    rng = np.random.default_rng(2)
    dv = Bank(pkg, eng, [sel], cfg, cap=1 << 20)
    outs, a = [[] for _ in sel], 0
    while a < len(frames):
        n = {'one': 1, 'ragged': int(rng.integers(0, 9)), 'all': len(frames)}[cuts]
        got = dv.run([frames[a:a + n]])[0]
        for j in range(len(sel)):
            outs[j].append(got[j])
        a += n
    fl = dv.bank.ma_flush()[0]
    for j, isi in enumerate(sel):
        assert np.array_equal(np.concatenate(outs[j] + [fl[j]]), ts[isi].reshape(-1))


def test_sixty_four_streams_equal_single_stream_banks(pkg, eng):
    S = 64
    grid = [M.GRID[(7 * i) % len(M.GRID)] for i in range(S)]
    sc = [M.scenario(100 + i, *g[1:], npk=40 + i % 5, span=0, damage=(3,)) for i, g in enumerate(grid)]
    cfg = {'issy_bytes': 0, 'crc_span': 0, 'reinsert_nulls': 1, 'check_crc': 1}     # one configuration per bank: ISSY length from the streams
    sels = [s[2] if i % 3 else s[2][::-1] for i, s in enumerate(sc)]
    dv = Bank(pkg, eng, sels, cfg, max_frames=8)
    rxs = [M.Receiver(sels[i], **cfg) for i in range(S)]
    pos = [0] * S
    rng = np.random.default_rng(5)
    while any(pos[i] < len(sc[i][0]) for i in range(S)):
        take = [int(rng.integers(0, 9)) for _ in range(S)]
        call = [sc[i][0][pos[i]:pos[i] + take[i]] for i in range(S)]
        pos = [pos[i] + take[i] for i in range(S)]
        got = dv.run(call)
        for i in range(S):
            want = rxs[i].process(call[i])
            for j in range(len(sels[i])):
                assert np.array_equal(got[i][j], want[j]), (i, j)
    for i in range(S):
        _same_stats(dv.bank, i, rxs[i], len(sels[i]))
    # and one of them through a bank of its own
    one = Bank(pkg, eng, [sels[9]], cfg, max_frames=64)
    alone = one.run([sc[9][0]])[0]
    again = M.Receiver(sels[9], **cfg).process(sc[9][0])
    assert all(np.array_equal(x, y) for x, y in zip(alone, again))
    assert one.bank.ma_stats(0, 0) == dv.bank.ma_stats(9, 0)


def test_capacity_error_leaves_the_state_untouched(pkg, eng):
    frames, ts, sel, cfg = M.scenario(4, True, '2', True, True)
    a, b = Bank(pkg, eng, [sel], cfg, cap=1 << 20), Bank(pkg, eng, [sel], cfg, cap=1 << 20)
    first = a.run([frames[:6]])[0]
    assert all(np.array_equal(x, y) for x, y in zip(first, b.run([frames[:6]])[0]))
    import torch
    small = [[torch.zeros(376, dtype=torch.uint8, device='cuda') for _ in sel]]
    before = [a.bank.ma_stats(0, j) for j in range(len(sel))]
    with pytest.raises(pkg.Dvbs2GpuError) as e:
        a.bank.process_ma([_dev(frames[6:20])], small, frame_bytes=[[x.size for x in frames[6:20]]])
    assert e.value.code == -5
    assert [a.bank.ma_stats(0, j) for j in range(len(sel))] == before
    want = b.run([frames[6:20]])[0]
    assert e.value.needed[0][:len(sel)] == [w.size for w in want]
    a.cap = max(e.value.needed[0])
    a.outs = [[torch.zeros(a.cap, dtype=torch.uint8, device='cuda') for _ in sel]]
    got = a.run([frames[6:20]])[0]
    assert all(np.array_equal(x, y) for x, y in zip(got, want))
    assert [a.bank.ma_stats(0, j) for j in range(len(sel))] == [b.bank.ma_stats(0, j) for j in range(len(sel))]


def test_ccm_sizes_and_tiny_data_fields(pkg, eng):
    """no size table (every frame kbch/8 bytes), and data fields shorter than a slot (SYNCD 65535 in between)"""
    import torch
    rng = np.random.default_rng(8)
    ts = M.make_ts(40, rng)
    st, _ = M.slot_stream(ts, 3, True)
    frames = [f for f, _ in M.frames_of_stream(st, 192, [3072], isi=0, sis=True, issyi=True, npd=True, dfl_list=[100, 60, 374, 31, 250])]
    rx = M.Receiver((0,), issy_bytes=3)
    bank = pkg.BbTsParserBank(eng, 1, 3072, 16)
    bank.set_mode_adaptation(True, issy_bytes=3)
    outs = [[torch.zeros(1 << 18, dtype=torch.uint8, device='cuda')]]
    got = []
    for a in range(0, len(frames), 7):
        want = rx.process(frames[a:a + 7])
        nb = bank.process_ma([_dev(frames[a:a + 7])], outs)
        got.append(outs[0][0][:nb[0][0]].cpu().numpy())
        assert np.array_equal(got[-1], want[0]), a
    got.append(bank.ma_flush()[0][0])
    assert np.array_equal(got[-1], rx.flush()[0])
    assert np.array_equal(np.concatenate(got), ts.reshape(-1))
    _same_stats(bank, 0, rx, 1)


def test_mode_off_is_the_reference_parser(pkg, eng):
    """a bank that had the mode on and off again continues like a fresh reference-mode bank, which equals the oracle"""
    kbch = 14232
    rng = np.random.default_rng(10)
    nfr = 12
    pk = B.ts_packets(nfr * (kbch // 8 - 10) // 188 + 2, rng)
    fr = B.bbframes_from_ts(pk, kbch, nfr)
    fresh, used = pkg.BbTsParserBank(eng, 1, kbch, 16), pkg.BbTsParserBank(eng, 1, kbch, 16)
    used.work(fr[:5])                                                # reference-mode state, then the mode on and off
    used.set_mode_adaptation(True)
    assert used.ma_work([f for f in fr[:3]])[0].size > 0
    used.set_mode_adaptation(False)
    orc = B.OracleBbTs(kbch)
    for a in range(0, nfr, 4):
        want = orc.work(fr[a:a + 4])
        assert np.array_equal(fresh.work(fr[a:a + 4]), want) and np.array_equal(used.work(fr[a:a + 4]), want)
        assert fresh.stats() == used.stats()


def test_mode_off_reproduces_the_golden_file(pkg, eng):
    """tests/golden/bbts_golden.json (the comparison of tests/test_oracle_bbts.py::test_golden_vectors) through a device bank that has
    the new code linked in and the mode off, and through one that had it on before"""
    import hashlib
    G = json.load(open(os.path.join(ROOT, 'tests', 'golden', 'bbts_golden.json')))
    sha = lambda a: hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()
    for was_on in (False, True):
        for c in G['ts_round_trip']:
            rng = np.random.default_rng(c['seed'])
            D = c['dfl_bytes'] if c['dfl_bytes'] is not None else c['kbch'] // 8 - 10
            pk = B.ts_packets(c['nframes'] * D // 188 + 2, rng)
            fr = B.bbframes_from_ts(pk, c['kbch'], c['nframes'], c['dfl_bytes'])
            assert sha(fr) == c['sha256_in']
            p = pkg.BbTsParserBank(eng, 1, c['kbch'], 16)
            if was_on:
                p.set_mode_adaptation(True)
                p.set_mode_adaptation(False)
            out = np.concatenate([p.work(fr[:4]), p.work(fr[4:])])
            assert sha(out) == c['sha256_out'] and out.size == 188 * c['packets_out']
        for c in G['fuzz']:
            rng = np.random.default_rng(c['seed'])
            p = pkg.BbTsParserBank(eng, 1, c['kbch'], 16)
            if was_on:
                p.set_mode_adaptation(True)
                p.set_mode_adaptation(False)
            for call in range(c['calls']):
                fr = B.fuzz_frames(rng, c['kbch'], int(rng.integers(0, 6)), ts_gs_choices=tuple(c['ts_gs_choices']), p_bad=0.2)
                o = p.work(fr, cap=fr.size + 376)
                st = p.stats()
                assert sha(o) == c['sha256_out_per_call'][call]
                assert [st['synched'], st['last_bb_proc'], st['last_gse_crc_err'], st['ts_gs'], int(o.size)] == c['state_per_call'][call]


VCM_PLS = [(4 << 2) | 2, (14 << 2) | 2, (6 << 2) | 2 | 1, 0, (19 << 2) | 2, (27 << 2) | 2 | 1, 13 << 2, (12 << 2) | 2]


def test_vcm_decode_feeds_the_bank_with_per_frame_sizes(pkg, eng):
    """IQ of a VCM carrier -> engine (ACM/VCM handle, device output) -> bank, sizes from bbframe_bytes, nothing copied through the
    host.  The oracle's transmitter takes no payload: it writes a valid BBHEADER (TS, SIS, UPL 1504, DFL = kbch - 80, SYNCD 0) in front
    of random bits, for every seed, so the case "no header passes its CRC-8, everything is rejected" cannot be had from it.  What the
    frames do allow is asked instead, and it is more: every frame is accepted at ITS size (a wrong size would fail the header check or
    shift the slots), the random data fields are cut into packets whose CRC-8 fails, and output, byte counts and statistics equal the
    model's on the same frames.  This checks the plumbing of the sizes, not TS content."""
    import torch
    import orc
    iq, bbs = orc.transmit_vcm(VCM_PLS, 26, seed=3, esn0_db=100.0, timing=0.3, phase0=0.2, lead_symbols=500)
    dm = eng.demod(eng.default_cfg(4, True, False, acm_vcm=1, max_ldpc_trials=25), max_samples=iq.size)
    bb_dev = torch.zeros(iq.size // 2 + 65536 + 40000, dtype=torch.uint8, device='cuda')
    nbytes = eng.process_batch([dm], [torch.from_numpy(iq).cuda()], [bb_dev])[0]
    sizes = [st.bbframe_bytes for st in dm.stats() if st.bbframe_bytes]
    assert len(sizes) >= 12 and len(set(sizes)) >= 4 and sum(sizes) == nbytes
    host = bb_dev[:nbytes].cpu().numpy()
    frames = [host[a:a + n] for a, n in zip(np.cumsum([0] + sizes[:-1]), sizes)]
    sent = {bytes(b) for b in bbs if b is not None}
    assert sum(bytes(f) in sent for f in frames) >= len(frames) - 2
    rx = M.Receiver((0,))
    want = rx.process(frames)[0]
    assert rx.rejected == 0 and rx.stats(0)['frames'] == len(frames) and want.size > 188 * len(frames)
    bank = pkg.BbTsParserBank(eng, 1, 58192, 64)
    bank.set_mode_adaptation(True)
    out = [[torch.zeros(1 << 18, dtype=torch.uint8, device='cuda')]]
    nb = bank.process_ma_from_demods([dm], [bb_dev], out)
    assert nb[0] == [want.size] + [0] * 7
    assert np.array_equal(out[0][0][:want.size].cpu().numpy(), want)
    _same_stats(bank, 0, rx, 1)
    st = bank.ma_stats(0, 0)
    assert st['ts_errs'] > st['packets'] // 2 and st['broken_joins'] > 0          # random bits: neither CRC-8s nor joins hold
    dm.close()
