"""DVB-T2 high-efficiency-mode BBFRAMEs without a GPU: the transmitter and receiver halves of tests/hem_ref.py against each other,
the library's host parser (a host-only bank with dvbs2gpu_bbts_ma_set_t2_hem on) against the model in bytes, statistics and carried
state, the compiled-in layout against the model's, and the switch's own conditions."""
import ctypes as C

import numpy as np
import pytest

import hem_ref as H
import ma_ref as M


def _in_step(got, sent):
    """got is a run of the sent packets that reaches the last whole one the frames brought"""
    a, b = got.reshape(-1, 188), sent.reshape(-1, 188)
    k = next(i for i in range(len(b)) if np.array_equal(b[i], a[0]))
    return np.array_equal(a, b[k:k + len(a)]), k, len(a)


@pytest.mark.parametrize('seed', [1, 2, 3])
@pytest.mark.parametrize('npd', [False, True])
@pytest.mark.parametrize('issyi', [False, True])
@pytest.mark.parametrize('mis', [False, True])
def test_model_round_trip(seed, npd, issyi, mis):
    frames, ts, sel = H.random_carrier(seed, npd, issyi, mis)
    rx, got = H.run_model(frames, sel, H.CFG)
    for j, isi in enumerate(sel):
        same, first, n = _in_step(got[j], ts[isi])
        st = rx.stats(j)
        assert same and first == 0 and n >= 1                      # the first frame starts a packet: in step from the start
        assert (st['ts_errs'], st['broken_joins'], st['undecided'], st['issy_bytes']) == (0, 0, 0, 0)
        assert st['packets'] + st['nulls'] == n and st['hem_frames'] == st['frames'] > 0 and st['iscr_valid'] == int(issyi)
    assert rx.rejected == 0 and rx.skipped == (len([1 for f in frames if f[1] == 17]) if mis else 0)


def test_model_edge_cuts_return_every_packet():
    frames, ts = H.edge_carrier()
    rx, got = H.run_model(frames, (0,), H.CFG)
    assert np.array_equal(got[0], ts.reshape(-1))                  # the last frame takes what is left: nothing stays open
    st = rx.stats(0)
    assert (st['broken_joins'], st['carried'], st['hem_frames']) == (0, 0, len(frames))
    # and the whole slot that a SYNCD = 65535 frame completes leaves with a flush when no frame follows
    rx, got = H.run_model(frames[:8], (0,), H.CFG)
    assert got[0].size % 188 == 0 and np.array_equal(got[0], ts.reshape(-1)[:got[0].size])
    rx2 = H.HemReceiver((0,), **H.CFG)
    before = rx2.process(frames[:8])[0]
    assert rx2.stats(0)['carried'] == 188 and got[0].size > before.size


def _host(pkg, sel, cfg, hem=True, gse=False, max_frames=16):
    hb = pkg.BbTsParserBank.host(58192, max_frames)
    hb.set_mode_adaptation(True, **cfg)
    hb.select_isi(0, sel)
    if gse:
        hb.ma_set_gse(True)
    if hem:
        hb.ma_set_t2_hem(True)
    return hb


def _equal_through(hb, rx, frames, sel, step):
    for a in range(0, len(frames), step):
        want, got = rx.process(frames[a:a + step]), hb.ma_work(frames[a:a + step])
        for j in range(len(sel)):
            assert np.array_equal(want[j], got[j]), (a, j)
            x, y = rx.stats(j), hb.ma_stats(0, j)
            assert {k: x[k] for k in H.STAT_KEYS} == {k: y[k] for k in H.STAT_KEYS}, (a, j)
    want, got = rx.flush(), hb.ma_flush()[0]
    for j in range(len(sel)):
        assert np.array_equal(want[j], got[j])
        x, y = rx.stats(j), hb.ma_stats(0, j)
        assert {k: x[k] for k in H.STAT_KEYS} == {k: y[k] for k in H.STAT_KEYS}
    assert hb.isi_seen(0) == sorted(rx.seen)


CARRIERS = H.carriers()


@pytest.mark.parametrize('name', sorted(CARRIERS))
@pytest.mark.parametrize('step', [1, 4])
def test_host_parser_equals_model(pkg, name, step):
    frames, sel = CARRIERS[name]
    gse = 'GSE' in name
    hb = _host(pkg, sel, H.CFG, gse=gse)
    rx = H.HemReceiver(sel, **H.CFG)
    _equal_through(hb, rx, frames, sel, step)
    hb.close()


def test_dnp_is_ignored_without_reinsertion(pkg):
    cfg = dict(H.CFG, reinsert_nulls=0)
    frames = CARRIERS['edge cuts'][0]
    hb, rx = _host(pkg, (0,), cfg), H.HemReceiver((0,), **cfg)
    _equal_through(hb, rx, frames, (0,), 4)
    full, _ = H.run_model(frames, (0,), H.CFG)
    assert rx.stats(0)['nulls'] == 0 < full.stats(0)['nulls'] and rx.stats(0)['packets'] == full.stats(0)['packets']
    hb.close()


def test_carriers_meet_what_they_are_for():
    """the counters that show that each constructed case does occur (on the model; the banks are compared with it elsewhere)"""
    rx, got = H.run_model(CARRIERS['edge cuts, frame 2 removed'][0], (0,), H.CFG)
    full = H.edge_carrier()[1]
    assert rx.stats(0)['broken_joins'] == 1
    a = got[0].reshape(-1, 188)
    sent = [bytes(p) for p in full if not M.is_null(p)]            # (the data packets: null packets are all alike)
    idx = [sent.index(bytes(p)) for p in a if not M.is_null(p)]                      # every packet that left is one that was sent, in order, one gap
    assert idx == sorted(idx) and len(set(np.diff(idx))) == 2
    frames, parts = H.mixed_modes()
    rx, got = H.run_model(frames, (0,), H.CFG)
    st = rx.stats(0)
    assert st['broken_joins'] == 2 and st['ts_errs'] == 0 and 0 < st['hem_frames'] < st['frames']
    a = got[0].reshape(-1, 188)
    nm = [bytes(p) for p in parts[1]]
    assert sum(bytes(p) in nm for p in a) >= 4                     # normal-mode packets in between, CRC-checked and clean
    rx, _ = H.run_model(CARRIERS['HEM GSE frames between'][0], (0,), H.CFG)
    assert rx.skipped == 2
    rx, _ = H.run_model(CARRIERS['random seed 2 npd 1 issyi 1 mis 0'][0], (0,), H.CFG)
    assert rx.rejected == 1 and rx.stats(0)['broken_joins'] == 1 and rx.stats(0)['nulls'] > 0


def test_layout_is_the_models(pkg):
    lib = pkg.load_library()
    a = (C.c_int32 * 4)()
    assert lib.dvbs2gpu_bbts_ma_get_hem_layout(a) == 0
    assert list(a) == [H.LAYOUT[k] for k in ('up_off', 'up_len', 'dnp_off', 'mode')]
    assert pkg.BbTsParserBank.ma_hem_layout() == H.LAYOUT
    assert lib.dvbs2gpu_bbts_ma_get_hem_layout(None) == -1


def test_switch_off_rejects_hem_frames_as_before(pkg):
    frames, _, sel = H.random_carrier(1, True, True)
    hb = _host(pkg, sel, H.CFG, hem=False)
    rx = H.HemReceiver(sel, hem=False, **H.CFG)
    out = hb.ma_work(frames)
    assert all(o.size == 0 for o in out) and all(o.size == 0 for o in rx.process(frames))
    st = hb.ma_stats(0, 0)
    assert st['rejected_frames'] == rx.rejected == len(frames) and (st['frames'], st['hem_frames'], st['packets'], st['carried']) == (0, 0, 0, 0)
    hb.ma_set_t2_hem(True)                                         # on: the same frames deliver
    assert hb.ma_work(frames)[0].size > 0 and hb.ma_stats(0, 0)['hem_frames'] == len(frames)
    hb.ma_set_t2_hem(False)                                        # off again: every lane afresh, and rejected as before
    assert hb.ma_stats(0, 0)['carried'] == 0 and hb.ma_stats(0, 0)['packets'] == 0
    assert hb.ma_work(frames)[0].size == 0 and hb.ma_stats(0, 0)['rejected_frames'] == 2 * len(frames)
    hb.close()


def test_normal_mode_results_do_not_depend_on_the_switch(pkg):
    frames, ts, sel, cfg = M.scenario(2, True, 'auto', True, True, npk=30, damage=(3,))
    a, b = _host(pkg, sel, cfg, hem=False), _host(pkg, sel, cfg, hem=True)
    for k in range(0, len(frames), 3):
        x, y = a.ma_work(frames[k:k + 3]), b.ma_work(frames[k:k + 3])
        assert all(np.array_equal(p, q) for p, q in zip(x, y))
    assert [a.ma_stats(0, j) for j in range(2)] == [b.ma_stats(0, j) for j in range(2)]


def test_setter_needs_the_mode(pkg):
    lib = pkg.load_library()
    assert lib.dvbs2gpu_bbts_ma_set_t2_hem(None, 1) == -1
    hb = pkg.BbTsParserBank.host(58192, 4)
    with pytest.raises(pkg.Dvbs2GpuError) as e:
        hb.ma_set_t2_hem(True)
    assert e.value.code == -1
    hb.set_mode_adaptation(True)
    hb.ma_set_t2_hem(True)
    hb.set_mode_adaptation(False)
    with pytest.raises(pkg.Dvbs2GpuError):
        hb.ma_set_t2_hem(False)
    hb.close()


def test_host_bank_capacity_error_leaves_state(pkg):
    frames, sel = CARRIERS['random seed 3 npd 1 issyi 0 mis 1']
    a, b = _host(pkg, sel, H.CFG), _host(pkg, sel, H.CFG)
    first = a.ma_work(frames[:3])
    assert all(np.array_equal(x, y) for x, y in zip(first, b.ma_work(frames[:3])))
    with pytest.raises(pkg.Dvbs2GpuError) as e:
        a.ma_work(frames[3:], cap=188)
    assert e.value.code == -5
    want = b.ma_work(frames[3:])
    assert e.value.needed == [w.size for w in want]
    got = a.ma_work(frames[3:], cap=max(e.value.needed))
    assert all(np.array_equal(x, y) for x, y in zip(got, want))
    assert [a.ma_stats(0, j) for j in range(2)] == [b.ma_stats(0, j) for j in range(2)]
