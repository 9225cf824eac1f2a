"""Mode adaptation without a GPU: the transmitter and receiver halves of tests/ma_ref.py against each other (the receiver model is
the yardstick of the GPU tests), the library's host parser (a host-only bank) against the model, and the argument checks of the new
C ABI calls that need no device."""
import ctypes as C

import numpy as np
import pytest

import ma_ref as M


def _run_model(frames, sel, cfg, step=5):
    rx = M.Receiver(sel, **cfg)
    outs = [[] for _ in sel]
    for a in range(0, len(frames), step):
        for j, o in enumerate(rx.process(frames[a:a + step])):
            outs[j].append(o)
    for j, o in enumerate(rx.flush()):
        outs[j].append(o)
    return rx, [np.concatenate(o) for o in outs]


@pytest.mark.parametrize('seed,mis,issy_mode,npd,mixed', M.GRID)
def test_model_round_trip(seed, mis, issy_mode, npd, mixed):
    frames, ts, sel, cfg = M.scenario(seed, mis, issy_mode, npd, mixed)
    rx, got = _run_model(frames, sel, cfg)
    for j, isi in enumerate(sel):
        assert np.array_equal(got[j], ts[isi].reshape(-1)), (isi, got[j].size, ts[isi].size)
        st = rx.stats(j)
        assert (st['ts_errs'], st['broken_joins'], st['undecided'], st['carried']) == (0, 0, 0, 0)
        assert st['packets'] + st['nulls'] == len(ts[isi])
        assert st['issy_bytes'] == {'none': 0, '2': 2, '3': 3, 'auto': 2 + seed % 2}[issy_mode]
    assert sorted(rx.seen) == sorted(ts)


@pytest.mark.parametrize('span', [0, 1])
def test_damaged_packets_come_back_with_tei_only(span):
    damage = (3, 20, 41)
    frames, ts, sel, cfg = M.scenario(5, True, '3', True, True, span=span, damage=damage)
    rx, got = _run_model(frames, sel, cfg)
    clean_frames, _, _, _ = M.scenario(5, True, '3', True, True, span=span)
    _, clean = _run_model(clean_frames, sel, cfg)
    for j, isi in enumerate(sel):
        a, b = got[j].reshape(-1, 188), clean[j].reshape(-1, 188)
        assert a.shape == b.shape
        bad = np.flatnonzero((a != b).any(axis=1))
        assert len(bad) == len(damage) and rx.stats(j)['ts_errs'] == len(damage)
        for r in bad:
            d = np.flatnonzero(a[r] != b[r])
            assert a[r, 1] == b[r, 1] | 0x80                       # transport_error_indicator
            assert len(d) <= 2 and np.all((a[r, d[d != 1]] ^ b[r, d[d != 1]]) == 0x10)      # and the bit error itself


def test_removed_frame_costs_its_packets_and_one_broken_join():
    rng = np.random.default_rng(9)
    ts = M.make_ts(150, rng, null_runs=False)
    L = M.slot_len(2, False)
    st, _ = M.slot_stream(ts, 2, False)
    cut = M.frames_of_stream(st, L, [14232], isi=0, sis=True, issyi=True)
    lost = 4
    a, b = cut[lost][1]
    assert (b - a) % L                                             # else the neighbours would join by accident
    touched = set(range(a // L, -(-b // L)))                       # slots with a byte in the lost frame
    if b % L == 0:
        touched.add(b // L - 1)
    rx, got = _run_model([f for k, (f, _) in enumerate(cut) if k != lost], (0,), {'issy_bytes': 2})
    want = np.array([ts[k] for k in range(len(ts)) if k not in touched]).reshape(-1)
    # the last packet before the gap is checked against a byte that is not its CRC-8 only if it ends exactly at the frame's end;
    # it does not here (the tail is cut), so nothing else changes
    assert np.array_equal(got[0], want)
    assert rx.stats(0)['broken_joins'] == 1 and rx.stats(0)['ts_errs'] == 0


def test_unknown_issy_length_waits_for_an_iscr():
    rng = np.random.default_rng(3)
    ts = M.make_ts(60, rng, null_runs=False)
    st, _ = M.slot_stream(ts, 3, False, issy_kinds=lambda k: 'bufs' if k < 12 else 'long')
    frames = [f for f, _ in M.frames_of_stream(st, 191, [3072], isi=0, sis=True, issyi=True)]   # one slot starts per frame
    rx, got = _run_model(frames, (0,), {'issy_bytes': 0})
    s = rx.stats(0)
    assert s['undecided'] > 0 and s['issy_bytes'] == 3
    first = got[0].reshape(-1, 188)[0]
    k = next(i for i in range(len(ts)) if np.array_equal(ts[i], first))
    assert k >= 12 and np.array_equal(got[0], ts[k:].reshape(-1))


# ------------------------------------------------------------------------------------------ the library's host parser
@pytest.fixture(scope='module')
def lib(pkg):
    return pkg.load_library()


def test_layout_is_the_models(lib):
    a = (C.c_int32 * 4)()
    assert lib.dvbs2gpu_bbts_ma_get_layout(a) == 0
    assert list(a) == [M.LAYOUT['crc_off'], M.LAYOUT['up_off'], M.LAYOUT['up_len'], M.LAYOUT['issy_off']]


@pytest.mark.parametrize('seed,mis,issy_mode,npd,mixed', M.GRID)
@pytest.mark.parametrize('step', [1, 4])
def test_host_parser_equals_model(pkg, seed, mis, issy_mode, npd, mixed, step):
    frames, ts, sel, cfg = M.scenario(seed, mis, issy_mode, npd, mixed, span=seed % 2, damage=(7, 30))
    frames = list(frames)
    frames[3] = frames[3].copy()
    frames[3][4] ^= 0x40                                           # one header fails its CRC-8
    rx = M.Receiver(sel, **cfg)
    hb = pkg.BbTsParserBank.host(58192, 8)
    hb.set_mode_adaptation(True, **cfg)
    hb.select_isi(0, sel)
    for a in range(0, len(frames), step):
        want, got = rx.process(frames[a:a + step]), hb.ma_work(frames[a:a + step])
        for j in range(len(sel)):
            assert np.array_equal(want[j], got[j]), (a, j)
    want, got = rx.flush(), hb.ma_flush()[0]
    for j in range(len(sel)):
        assert np.array_equal(want[j], got[j])
        a, b = rx.stats(j), hb.ma_stats(0, j)
        assert {k: a[k] for k in M.STAT_KEYS} == {k: b[k] for k in M.STAT_KEYS}
    assert hb.isi_seen(0) == sorted(rx.seen)
    hb.close()


def test_host_bank_capacity_error_leaves_state(pkg):
    frames, ts, sel, cfg = M.scenario(4, True, '2', True, True)
    a, b = pkg.BbTsParserBank.host(58192, 64), pkg.BbTsParserBank.host(58192, 64)
    for h in (a, b):
        h.set_mode_adaptation(True, **cfg)
        h.select_isi(0, sel)
    with pytest.raises(pkg.Dvbs2GpuError) as e:
        a.ma_work(frames[:20], cap=188)
    assert e.value.code == -5
    want = b.ma_work(frames[:20])
    assert e.value.needed == [w.size for w in want]
    got = a.ma_work(frames[:20], cap=max(e.value.needed))
    assert all(np.array_equal(x, y) for x, y in zip(got, want))
    assert a.ma_stats(0, 0) == b.ma_stats(0, 0)


def test_argument_checks_need_no_device(pkg, lib):
    cfg = pkg.BbtsMaCfg()
    lib.dvbs2gpu_bbts_ma_default_cfg(C.byref(cfg))
    assert (cfg.issy_bytes, cfg.crc_span, cfg.reinsert_nulls, cfg.check_crc) == (0, 0, 1, 1)
    st, m, nb, isi = pkg.BbtsMaStats(), (C.c_uint32 * 8)(), (C.c_int * 8)(), (C.c_uint8 * 8)()
    p8 = (C.c_void_p * 8)()
    assert lib.dvbs2gpu_bbts_set_mode_adaptation(None, C.byref(cfg)) == -1
    assert lib.dvbs2gpu_bbts_select_isi(None, 0, isi, 1) == -1
    assert lib.dvbs2gpu_bbts_process_ma_batch(None, p8, None, nb, p8, 0, nb, nb, None) == -1
    assert lib.dvbs2gpu_bbts_ma_work(None, None, None, 0, p8, 0, nb, nb) == -1
    assert lib.dvbs2gpu_bbts_ma_flush(None, p8, 0, nb) == -1 and lib.dvbs2gpu_bbts_ma_flush_host(None, p8, 0, nb) == -1
    assert lib.dvbs2gpu_bbts_ma_get_stats(None, 0, 0, C.byref(st)) == -1
    assert lib.dvbs2gpu_bbts_get_isi_seen(None, 0, m) == -1
    assert lib.dvbs2gpu_bbts_ma_get_layout(None) == -1
    h = C.c_void_p()
    assert lib.dvbs2gpu_bbts_create_host(58192, 0, C.byref(h)) == -1 and lib.dvbs2gpu_bbts_create_host(58193, 4, C.byref(h)) == -1
    assert lib.dvbs2gpu_bbts_create_host(58192, 4, C.byref(h)) == 0
    try:
        assert lib.dvbs2gpu_bbts_select_isi(h, 0, isi, 1) == -1                      # the mode is off
        assert lib.dvbs2gpu_bbts_ma_get_stats(h, 0, 0, C.byref(st)) == -1
        assert lib.dvbs2gpu_bbts_work(h, None, 0, None, 0) == -1                     # a host bank has no reference-mode path
        bad = pkg.BbtsMaCfg(1, 0, 1, 1)
        assert lib.dvbs2gpu_bbts_set_mode_adaptation(h, C.byref(bad)) == -1
        assert lib.dvbs2gpu_bbts_set_mode_adaptation(h, C.byref(cfg)) == 0
        assert lib.dvbs2gpu_bbts_select_isi(h, 0, isi, 9) == -1 and lib.dvbs2gpu_bbts_select_isi(h, 1, isi, 1) == -1
        assert lib.dvbs2gpu_bbts_ma_get_stats(h, 0, 8, C.byref(st)) == -1
        assert lib.dvbs2gpu_bbts_ma_get_stats(h, 0, 0, C.byref(st)) == 0 and st.selected == 1 and st.isi == 0
        sizes = (C.c_int * 1)(9)
        buf = (C.c_uint8 * 16)()
        assert lib.dvbs2gpu_bbts_ma_work(h, buf, sizes, 1, p8, 0, nb, nb) == -1      # no frame is shorter than its header
        assert lib.dvbs2gpu_bbts_ma_work(h, buf, None, 5, p8, 0, nb, nb) == -1       # more than max_frames
        assert lib.dvbs2gpu_bbts_set_mode_adaptation(h, None) == 0
        assert lib.dvbs2gpu_bbts_ma_get_stats(h, 0, 0, C.byref(st)) == -1
    finally:
        lib.dvbs2gpu_bbts_destroy(h)
