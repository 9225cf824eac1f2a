"""CPU tests of the constructed deframer streams (tests/dvbs_deframer_patterns.py): the oracle deframer (oracle/dvbs_tail.cpp) makes of every
pattern what its builder states -- the number of frames, the planted bytes, the error pair after every call -- whole and under every cutting,
and the reference's own DVBS_TS_Deframer (oracle/_ref, where it is built) delivers the same frames."""
import ctypes as C
import numpy as np
import pytest
import orc
import dvbs_deframer_patterns as dp
from orc_dvbs import P, VP
from orc_dvbs_tail import OracleDeframer, OracleTail


def _patterns():
    return dp.bank_patterns() + [dp.dense204(True), dp.dense204(False)]


def test_builders_state_the_issue_counts():
    by = {p.name: p for p in _patterns()}
    assert len(by) == len(_patterns())
    assert sum(len(p.frames) == 40 for p in by.values()) == 17
    assert len(by['dense204_lead131_alt_err'].frames) == len(by['dense204_lead131_nor_err'].frames) == 204
    assert [len(by[f'threshold{k}'].frames) for k in dp.THRESHOLD_KS] == [1, 1, 0, 0, 1, 1]
    assert [by[f'threshold{k}'].errs for k in (8, 56)] == [[(8, 0)], [(0, 8)]]
    assert by['threshold_run'].errs == [(0, 0), (8, 0), (0, 8), (0, 0)]
    # eight consecutive leads: the first hits of the dense streams fire on every residue mod 8, and each run of 320 positions covers a
    # whole 256-position tile, so some hit of every residue class sits on tile positions 0 / 255 (lane 0 of wave 0, lane 63 of wave 3)
    firsts = [(p.ends[0] - 1) for p in by.values() if p.name.startswith('dense40_lead25')]
    assert sorted({f % 8 for f in firsts}) == list(range(8))
    tile_pos = {(e - 1) % 256 for p in by.values() if p.name.startswith('dense40') for e in p.ends}
    assert {0, 63, 64, 127, 128, 191, 192, 255} <= tile_pos
    for p in by.values():
        assert p.what and len(p.frames) == len(p.ends) == len(p.errs)


@pytest.mark.parametrize('rule', dp.CUTTINGS)
def test_oracle_deframer_delivers_what_the_builders_state(rule):
    for p in _patterns():
        d = OracleDeframer()
        bounds = dp.cut_bounds(p, rule)
        a, total = 0, 0
        for b, (want, werr) in zip(bounds, dp.expected_calls(p, bounds)):
            got, err = d.work(p.bits[a:b], capacity=len(p.frames) + 4)
            assert got.shape == want.shape, (p.name, rule, a, b, got.shape, want.shape)
            assert np.array_equal(got, want), (p.name, rule, a, b)
            assert err == werr, (p.name, rule, a, b, err, werr)
            total += len(got)
            a = b
        assert total == len(p.frames), (p.name, rule)


def test_cuttings_put_the_boundary_where_they_say():
    p = dp.bank_patterns()[0]
    e = p.ends[0]
    assert dp.cut_bounds(p, 'whole') == [p.bits.size]
    assert [dp.cut_bounds(p, f'before{d}')[0] for d in (1, 7, 8, 9, 13055)] == [e - 1, e - 7, e - 8, e - 9, e - 13055]
    assert e - 13055 == p.ends[0] - dp.FRAME_BITS + 1 > 0                      # all of the window but its first bit lies in the second call
    m = dp.cut_bounds(p, 'mid_run')[0]
    assert p.ends[20] < m < p.ends[21]
    assert np.diff([0] + dp.cut_bounds(p, 'tiny_calls')).tolist()[1:5] == [0, 1, 0, 1]
    calls = dp.expected_calls(p, dp.cut_bounds(p, 'tiny_calls'))
    assert [len(c[0]) for c in calls] == [0, 0, 1, 0, 0, 39]


def test_reference_deframer_delivers_the_same_frames():
    r = orc.ref()
    if r is None or not hasattr(r, 'ref_tsdef_create'):
        pytest.skip('oracle/_ref not built')
    r.ref_tsdef_create.restype = VP
    r.ref_tsdef_work.argtypes = [VP, VP, C.c_int, VP]
    for p in _patterns():
        for rule in ('whole', 'before8', 'mid_run', 'tiny_calls'):
            h = VP(r.ref_tsdef_create())
            bounds = dp.cut_bounds(p, rule)
            a = 0
            for b, (want, _) in zip(bounds, dp.expected_calls(p, bounds)):
                seg = np.ascontiguousarray(p.bits[a:b])
                out = np.zeros(1632 * (len(p.frames) + 4), np.uint8)
                n = r.ref_tsdef_work(h, P(seg), seg.size, P(out)) if seg.size else 0
                assert n == len(want) and np.array_equal(out[:1632 * n].reshape(n, 1632), want), (p.name, rule, a, b, n)
                a = b


def test_oracle_tail_capacity_and_keep():
    """OracleTail.process with a stated capacity takes a dense run whole; with keep it hands on the first frames only, while the deframer sees everything"""
    p = dp.bank_patterns()[1]
    full, part = OracleTail(), OracleTail()
    ts, nf = full.process(p.bits, capacity=44)
    assert nf == 40 and ts.size == 40 * 8 * 188 and np.array_equal(full.call_frames, np.stack(p.frames))
    ts4, nf4 = part.process(p.bits, capacity=44, keep=4)
    assert nf4 == 4 and part.call_hits == 40 and np.array_equal(ts4, ts[:4 * 8 * 188]) and np.array_equal(part.call_frames, np.stack(p.frames[:4]))
    assert tuple(part.errs) == tuple(full.errs) == p.errs[-1]
