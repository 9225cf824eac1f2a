"""GSE in the mode-adaptation mode without a GPU: the transmitter and receiver halves of tests/ma_gse_ref.py against each other, the
library's host bank against the receiver model (bytes, rows, counters), the capacity rule, argument checks and struct sizes."""
import ctypes as C

import numpy as np
import pytest

import ma_gse_ref as G
import ma_ref as M

CFG = {'issy_bytes': 0, 'crc_span': 0, 'reinsert_nulls': 1, 'check_crc': 1}


def host_bank(pkg, sel, gse=True, max_frames=64):
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
    assert b['host_fallback_calls'] == fallback


@pytest.mark.parametrize('seed,mis,mixed,nisi,with_ts', G.GRID)
def test_model_round_trip(seed, mis, mixed, nisi, with_ts):
    """well-formed carriers: the model delivers EVERY PDU that was sent, unchanged and in order, and the TS of a mixed lane too"""
    frames, carries, sel = G.scenario(seed, mis, mixed, nisi, with_ts)
    assert len(frames) <= 48 and all(10 <= f.size <= 7274 for f in frames)
    if mixed:
        assert {384, 7274} <= {f.size for f in frames}
    rx = G.Receiver(sel, **CFG)
    pdus, ts = [[] for _ in sel], [[] for _ in sel]
    for a in range(0, len(frames), 5):
        outs = rx.process(frames[a:a + 5])
        for j in range(len(sel)):
            p, t = G.split_output(outs[j], rx.rows(j))
            pdus[j] += p
            ts[j].append(t)
    for j, o in enumerate(rx.flush()):
        ts[j].append(o)
    kinds = set()
    for j, isi in enumerate(sel):
        sent = carries[isi]['gse']
        assert len(pdus[j]) == len(sent)
        for (proto, b, flags), (sproto, spdu, lt) in zip(pdus[j], sent):
            assert proto == sproto and b == G.gre(sproto, spdu) and bool(flags & G.PDU_LABEL) == (lt < 2)
            kinds.add((lt, flags & G.PDU_REASSEMBLED))
        want_ts = carries[isi]['ts'].reshape(-1) if carries[isi]['ts'] is not None else np.zeros(0, np.uint8)
        assert np.array_equal(np.concatenate(ts[j]), want_ts)
        g = rx.gse_stats(j)
        assert (g['crc_failures'], g['dropped_no_slot'], g['dropped_overflow'], g['malformed_frames'], g['open_slots']) == (0, 0, 0, 0, 0)
        assert g['complete_pdus'] + g['reassembled_pdus'] == len(sent)
    assert len({lt for lt, _ in kinds}) == 4 and len({r for _, r in kinds}) == 2       # all label types, whole and fragmented


@pytest.mark.parametrize('seed,mis,mixed,nisi,with_ts', G.GRID)
@pytest.mark.parametrize('step', [1, 5, 48])
def test_host_bank_equals_model(pkg, seed, mis, mixed, nisi, with_ts, step):
    frames, carries, sel = G.scenario(seed, mis, mixed, nisi, with_ts)
    rx = G.Receiver(sel, **CFG)
    hb = host_bank(pkg, sel)
    for a in range(0, len(frames), step):
        want, got = rx.process(frames[a:a + step]), hb.ma_work(frames[a:a + step])
        for j in range(len(sel)):
            assert np.array_equal(want[j], got[j]), (a, j)
            assert hb.ma_pdu_table(0, j) == rx.rows(j), (a, j)
    want, got = rx.flush(), hb.ma_flush()[0]
    for j in range(len(sel)):
        assert np.array_equal(want[j], got[j])
        same_lane(hb, 0, rx, j)
    assert hb.isi_seen(0) == sorted(rx.seen)
    hb.close()


def test_switch_off_skips_gse_frames_and_drops_the_state(pkg):
    frames, carries, sel = G.scenario(6, True, True, 2, True)
    off, rx = host_bank(pkg, sel, gse=False), G.Receiver(sel, gse=False, **CFG)
    want, got = rx.process(frames), off.ma_work(frames)
    assert all(np.array_equal(want[j], got[j]) for j in range(len(sel)))
    assert off.ma_stats(0, 0)['skipped_frames'] == rx.skipped > 0 and off.ma_gse_stats(0, 0)['frames'] == 0
    on = host_bank(pkg, sel)
    on.ma_work(frames[:7])
    assert any(on.ma_gse_stats(0, j)['open_slots'] for j in range(len(sel)))
    on.ma_set_gse(False)
    assert all(on.ma_gse_stats(0, j) == off.ma_gse_stats(0, j) for j in range(len(sel)))


def test_capacity_error_leaves_ts_and_gse_state(pkg):
    frames, carries, sel = G.scenario(6, True, True, 2, True)
    a, b = host_bank(pkg, sel), host_bank(pkg, sel)
    a.ma_work(frames[:6]), b.ma_work(frames[:6])
    before = [(a.ma_stats(0, j), a.ma_gse_stats(0, j)) for j in range(len(sel))]
    with pytest.raises(pkg.Dvbs2GpuError) as e:
        a.ma_work(frames[6:30], cap=100)
    assert e.value.code == -5
    assert [(a.ma_stats(0, j), a.ma_gse_stats(0, j)) for j in range(len(sel))] == before
    assert any(b.ma_pdu_table(0, j) for j in range(len(sel)))      # the call before had rows; the failed call has none
    assert all(a.ma_pdu_table(0, j) == [] for j in range(len(sel)))
    want = b.ma_work(frames[6:30])
    assert e.value.needed == [w.size for w in want] and max(e.value.needed) > 100
    got = a.ma_work(frames[6:30], cap=max(e.value.needed))
    assert all(np.array_equal(x, y) for x, y in zip(got, want))
    for j in range(len(sel)):
        assert (a.ma_stats(0, j), a.ma_gse_stats(0, j), a.ma_pdu_table(0, j)) == (b.ma_stats(0, j), b.ma_gse_stats(0, j), b.ma_pdu_table(0, j))


def test_argument_checks_need_no_device(pkg):
    lib = pkg.load_library()
    st, n, rows, p = pkg.BbtsMaGseStats(), C.c_int(), (pkg.GsePdu * 4)(), C.c_void_p()
    assert lib.dvbs2gpu_bbts_ma_set_gse(None, 1) == -1
    assert lib.dvbs2gpu_bbts_ma_get_gse_stats(None, 0, 0, C.byref(st)) == -1
    assert lib.dvbs2gpu_bbts_ma_get_pdu_table(None, 0, 0, rows, 4, C.byref(n)) == -1
    assert lib.dvbs2gpu_bbts_ma_get_pdu_table_device(None, 0, 0, C.byref(p), C.byref(n)) == -1
    h = C.c_void_p()
    assert lib.dvbs2gpu_bbts_create_host(58192, 4, C.byref(h)) == 0
    try:
        assert lib.dvbs2gpu_bbts_ma_set_gse(h, 1) == -1                              # the mode is off
        assert lib.dvbs2gpu_bbts_ma_get_gse_stats(h, 0, 0, C.byref(st)) == -1
        cfg = pkg.BbtsMaCfg()
        lib.dvbs2gpu_bbts_ma_default_cfg(C.byref(cfg))
        assert lib.dvbs2gpu_bbts_set_mode_adaptation(h, C.byref(cfg)) == 0
        assert lib.dvbs2gpu_bbts_ma_set_gse(h, 1) == 0
        assert lib.dvbs2gpu_bbts_ma_get_gse_stats(h, 0, 8, C.byref(st)) == -1 and lib.dvbs2gpu_bbts_ma_get_gse_stats(h, 1, 0, C.byref(st)) == -1
        assert lib.dvbs2gpu_bbts_ma_get_gse_stats(h, 0, 0, None) == -1
        assert lib.dvbs2gpu_bbts_ma_get_gse_stats(h, 0, 7, C.byref(st)) == 0 and st.frames == 0 and st.open_slots == 0
        assert lib.dvbs2gpu_bbts_ma_get_pdu_table(h, 0, 0, None, 4, C.byref(n)) == -1
        assert lib.dvbs2gpu_bbts_ma_get_pdu_table(h, 0, -1, rows, 4, C.byref(n)) == -1
        assert lib.dvbs2gpu_bbts_ma_get_pdu_table(h, 0, 0, rows, 4, C.byref(n)) == 0 and n.value == 0
        assert lib.dvbs2gpu_bbts_ma_get_pdu_table_device(h, 0, 0, C.byref(p), C.byref(n)) == -1      # a host bank has no device table
    finally:
        lib.dvbs2gpu_bbts_destroy(h)


def test_struct_sizes_are_pinned(pkg):
    assert C.sizeof(pkg.BbtsMaGseStats) == 96 and pkg.BbtsMaGseStats.open_slots.offset == 88
    assert C.sizeof(pkg.GsePdu) == 16 and C.sizeof(pkg.BbtsMaStats) == 72 and C.sizeof(pkg.BbtsMaCfg) == 16 and C.sizeof(pkg.GseStats) == 96
