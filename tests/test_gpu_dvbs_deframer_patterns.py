"""GPU tests of the TS deframer (dvbs_tsdef_find_kernel / dvbs_tsdef_emit_kernel) on constructed sync patterns (tests/dvbs_deframer_patterns.py):
many hits per wave and tile and across their seams, normal and inverted hits side by side, the <= 8 error bound from both sides, call
boundaries 1 .. 13 055 bits before a hit, 0-bit and 1-bit calls -- as streams of ONE bank, call by call against the CPU oracle
(oracle/dvbs_tail.cpp, which tests/test_oracle_dvbs_deframer_patterns.py holds to the builders' statements and to the reference's deframer):
frames (tap 0), frame count, errors_nor / errors_inv, RS error counts and the TS bytes, all with equality.  Then the two capacity rules of
include/dvbs2gpu.h: hits beyond a handle's max_bits / 13056 + 3 frames are counted in dvbs2gpu_dvbs_tail_get_dropped, and TS packets
that do not fit into cap are dropped."""
import numpy as np
import pytest
import dvbs_deframer_patterns as dp
import orc_dvbs_tail as ot
from orc_dvbs_tail import OracleDeframer, OracleTail

pytestmark = pytest.mark.gpu

_whole = {}


def _whole_run(p):
    """the oracle tail over the whole stream in one call, computed once per pattern: what comes behind the deframer is a function of the frame
    sequence alone, so the TS bytes and RS counts of any cutting are slices of it; the deframer itself runs call by call for every cutting"""
    if p.name not in _whole:
        o = OracleTail()
        ts, nf = o.process(p.bits, capacity=len(p.frames) + 4)
        assert nf == len(p.frames), (p.name, nf)
        _whole[p.name] = (ts.reshape(nf, 8 * 188), np.asarray(o.call_rs, np.int32).reshape(nf, 8))
    return _whole[p.name]


def _capacity(max_bits):
    """frames a handle holds per stream and call (include/dvbs2gpu.h)"""
    return max_bits // dp.FRAME_BITS + 3


def _run_cutting(engine, pkg, pats, rule, max_bits):
    import torch
    S = len(pats)
    bounds = [dp.cut_bounds(p, rule) for p in pats]
    ncalls = max(len(b) for b in bounds)
    bounds = [b + [b[-1]] * (ncalls - len(b)) for b in bounds]                    # (a stream that has no more bits brings 0-bit calls)
    bank = pkg.DvbsTailBank(engine, S, max_bits=max_bits)
    cap = _capacity(max_bits)
    assert cap >= max(len(p.frames) for p in pats)
    dev = [torch.from_numpy(p.bits).cuda() for p in pats]
    tout = [torch.zeros(188 * 8 * cap, dtype=torch.uint8, device='cuda') for _ in pats]
    defr = [OracleDeframer() for _ in pats]
    done = [0] * S
    for c in range(ncalls):
        a = [0 if c == 0 else bounds[s][c - 1] for s in range(S)]
        nb = bank.process_batch([dev[s][a[s]:bounds[s][c]] for s in range(S)], tout)
        for s, p in enumerate(pats):
            where = (p.name, rule, c, a[s], bounds[s][c])
            frames, errs = defr[s].work(p.bits[a[s]:bounds[s][c]], capacity=len(p.frames) + 4)
            nf = len(frames)
            ts, rs = _whole_run(p)
            st = bank.stats(s)
            assert st['frames'] == nf, (where, st, nf)
            assert (st['errors_nor'], st['errors_inv']) == errs, (where, st, errs)
            assert np.array_equal(bank.tap(0, s).reshape(-1, 1632), frames), where
            assert nb[s] == 1504 * nf, (where, nb[s])
            assert np.array_equal(tout[s][:nb[s]].cpu().numpy().reshape(nf, 1504), ts[done[s]:done[s] + nf]), where
            if nf:
                assert st['rs_errors'] == rs[done[s] + nf - 1].tolist(), (where, st)
            done[s] += nf
    assert done == [len(p.frames) for p in pats]
    bank.close()


@pytest.mark.parametrize('rule', dp.CUTTINGS)
def test_constructed_streams_in_one_bank(engine, pkg, rule):
    pats = dp.bank_patterns()
    assert {len(p.frames) for p in pats} == {0, 1, 4, 40} and any(p.bits.size == 0 for p in pats)
    _run_cutting(engine, pkg, pats, rule, max_bits=40 * dp.FRAME_BITS)


@pytest.mark.parametrize('rule', dp.CUTTINGS)
def test_run_of_204_hits(engine, pkg, rule):
    _run_cutting(engine, pkg, [dp.dense204(True)], rule, max_bits=204 * dp.FRAME_BITS)


def test_dropped_count_is_kept_per_stream(engine, pkg):
    """the bank's streams on a handle of 4 frames, one call: every stream delivers its first min(hits, 4) frames and reports hits - 4 or 0
    dropped in its own row; on a handle that holds everything nothing is reported; reset() clears the count"""
    import torch
    pats = [p for p in dp.bank_patterns() if p.bits.size <= 14000]
    assert sorted({len(p.frames) for p in pats}) == [0, 1, 40]
    for max_bits, cap in ((14000, 4), (40 * dp.FRAME_BITS, 43)):
        bank = pkg.DvbsTailBank(engine, len(pats), max_bits=max_bits)
        assert bank.max_frames == cap == _capacity(max_bits)
        tout = [torch.zeros(188 * 8 * cap, dtype=torch.uint8, device='cuda') for _ in pats]
        nb = bank.process_batch([torch.from_numpy(p.bits).cuda() for p in pats], tout)
        for s, p in enumerate(pats):
            kept = min(len(p.frames), cap)
            assert bank.stats(s)['frames'] == kept and nb[s] == 1504 * kept, (p.name, cap)
            assert bank.dropped(s) == len(p.frames) - kept, (p.name, cap, bank.dropped(s))
            assert np.array_equal(bank.tap(0, s).reshape(-1, 1632), np.stack(p.frames[:kept]) if kept else np.zeros((0, 1632), np.uint8)), (p.name, cap)
            st = bank.stats(s)
            assert (st['errors_nor'], st['errors_inv']) == (p.errs[-1] if p.errs else (0, 0)), (p.name, cap, st)
        bank.reset()
        assert [bank.dropped(s) for s in range(len(pats))] == [0] * len(pats)
        bank.close()


def test_hits_beyond_the_handle_capacity_are_counted(engine, pkg):
    """a handle of 4 frames fed 40 hits in one call: the oracle's first 4 frames come out, 36 are reported dropped, errors_nor / errors_inv
    are those of the 40th hit, and the calls that follow -- a clean stream, cut in two -- equal an oracle whose deframer saw all 40 and
    whose later stages got the 4 delivered frames"""
    import torch
    p = dp.dense(40, 3, alternate=True, errors=True, seed=5)
    assert p.errs[-1] not in p.errs[:4]                                          # the 40th hit's error pair is none of the delivered frames'
    clean, _ = ot.dvbs_outer_tx(16, seed=70)
    bank = pkg.DvbsTailBank(engine, 1, max_bits=14000)
    cap = bank.max_frames
    assert cap == 4 and p.bits.size <= 14000
    o = OracleTail()
    out = torch.zeros(188 * 8 * cap, dtype=torch.uint8, device='cuda')
    for k, seg in enumerate((p.bits, clean[:13500], clean[13500:])):
        want, nf = o.process(seg, capacity=44, keep=cap)
        nb = bank.process_batch([torch.from_numpy(np.ascontiguousarray(seg)).cuda()], [out])
        st = bank.stats(0)
        assert st['frames'] == nf and bank.dropped(0) == o.call_hits - nf, (k, st, bank.dropped(0), o.call_hits)
        assert (st['errors_nor'], st['errors_inv']) == tuple(int(x) for x in o.errs), (k, st, o.errs)
        assert np.array_equal(bank.tap(0).reshape(-1, 1632), o.call_frames), k
        assert nb[0] == want.size and np.array_equal(out[:nb[0]].cpu().numpy(), want), k
        assert st['rs_errors'] == o.last_rs, (k, st, o.last_rs)
        if k == 0:
            assert nf == cap and o.call_hits == 40 and bank.dropped(0) == 40 - cap
            assert np.array_equal(o.call_frames, np.stack(p.frames[:cap])) and tuple(int(x) for x in o.errs) == p.errs[-1]
        else:
            assert nf == 1 and bank.dropped(0) == 0
    bank.close()


def test_ts_packets_beyond_cap_are_dropped(engine, pkg):
    """'packets that do not fit into cap are dropped' (include/dvbs2gpu.h): with cap = 188 k + 100 the first k packets of the call come out,
    out_bytes = 188 k, nothing is written behind them, and the next call equals the oracle that saw every packet"""
    import torch
    bits, _ = ot.dvbs_outer_tx(64, seed=71)
    half = bits.size // 2
    bank = pkg.DvbsTailBank(engine, 1, max_bits=half)
    for k in (5, 0, 31):
        bank.reset()
        o = OracleTail()
        want, nf = o.process(bits[:half])
        assert nf == 4 and want.size == 32 * 188
        out = torch.full((188 * k + 100,), 0xEE, dtype=torch.uint8, device='cuda')
        nb = bank.process_batch([torch.from_numpy(bits[:half]).cuda()], [out])
        got = out.cpu().numpy()
        assert nb[0] == 188 * k and np.array_equal(got[:188 * k], want[:188 * k]) and (got[188 * k:] == 0xEE).all(), (k, nb)
        assert bank.stats(0)['frames'] == 4
        want2, nf2 = o.process(bits[half:])
        out2 = torch.zeros(188 * 8 * _capacity(half), dtype=torch.uint8, device='cuda')
        nb2 = bank.process_batch([torch.from_numpy(bits[half:]).cuda()], [out2])
        assert nf2 == 4 and nb2[0] == want2.size and np.array_equal(out2[:nb2[0]].cpu().numpy(), want2), k
        assert bank.stats(0)['rs_errors'] == o.last_rs
    bank.close()
