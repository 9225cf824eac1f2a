"""The outer-code kernels (BCH syndromes, BCH correction, BB de-scrambling) on all 21 codes: the constructed patterns of tests/bch_patterns.py
against the CPU oracle (bit-exact) and against what the code itself promises, a work list longer than both launches' grids, and the
de-scrambler on data."""
import numpy as np
import pytest

import bch_patterns as bp
import orc

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize('rate,short', orc.ALL_CODES)
def test_bch_every_code_constructed_patterns(engine, rate, short):
    """one launch with every pattern of the code, a clean frame first and last: corrections and every byte equal the oracle's, and the GPU output itself
    meets the independent expectations (flipped bits corrected and counted; a root in the shortened part: -1, frame untouched)"""
    import torch
    pats = bp.patterns(rate, short)
    assert bp.family(pats[0].name) == 'clean' and bp.family(pats[-1].name) == 'clean'
    want_ret, want = bp.oracle_outcomes(rate, short)
    d = torch.from_numpy(np.stack([q.frame for q in pats])).cuda()
    corr = engine.bch_decode(d, rate, bool(short))
    torch.cuda.synchronize()
    got_ret, got = corr.cpu().numpy(), d.cpu().numpy()
    bad = [q.name for n, q in enumerate(pats) if got_ret[n] != want_ret[n] or not np.array_equal(got[n], want[n])]
    assert not bad, bad
    bp.check_independent(rate, short, got_ret, got)


@pytest.mark.parametrize('rate,short', [(5, 0), (0, 1)])
def test_bch_work_list_larger_than_the_grid(engine, rate, short):
    """4500 frames: more than the syndrome launch's 4096 workgroups (its frame loop takes a second turn) and, with two of three frames dirty, 3000
    entries on a work list served by 2048 correction workgroups; every third frame is clean, so the list is sparse in the batch.  Each frame against the
    oracle's outcome for its pattern.  And the empty batch."""
    import torch
    nf = 4500
    pats = bp.patterns(rate, short)
    want_ret, want = bp.oracle_outcomes(rate, short)
    clean = [n for n, q in enumerate(pats) if bp.family(q.name) == 'clean']
    dirty = [n for n, q in enumerate(pats) if bp.family(q.name) != 'clean']
    idx = np.array([clean[(f // 3) % 2] if f % 3 == 0 else dirty[(f - f // 3 - 1) % len(dirty)] for f in range(nf)])
    assert nf > 4096 and (want_ret[idx] != 0).sum() > 2048 and set(idx) == set(range(len(pats)))
    d = torch.from_numpy(np.stack([q.frame for q in pats])[idx]).cuda()
    corr = engine.bch_decode(d, rate, bool(short))
    torch.cuda.synchronize()
    got_ret, got = corr.cpu().numpy(), d.cpu().numpy()
    wrong = np.flatnonzero((got_ret != want_ret[idx]) | (got != want[idx]).any(axis=1))
    assert wrong.size == 0, [(int(f), pats[idx[f]].name) for f in wrong[:8]]
    e = torch.empty((0, d.shape[1]), dtype=torch.uint8, device='cuda')
    assert engine.bch_decode(e, rate, bool(short)).shape == (0,)
    torch.cuda.synchronize()
    assert np.array_equal(d.cpu().numpy(), got)


@pytest.mark.parametrize('rate,short', orc.ALL_CODES)
def test_bb_descramble_every_code_on_data(engine, rate, short):
    """random bytes, not zeros: the first kbch / 8 bytes of each frame XOR the PRBS, nothing else in and nothing else out"""
    import torch
    p = orc.fec_params(rate, short)
    nb, kb = p['K'] // 8, p['kbch'] // 8
    rng = np.random.default_rng(300 + 2 * rate + short)
    frames = rng.integers(0, 256, (3, nb), dtype=np.uint8)
    want = np.ascontiguousarray(frames[:, :kb])
    for f in range(3):
        orc.lib().orc_bb_descramble(want[f], kb)
    assert not np.array_equal(want, frames[:, :kb])
    out = engine.bb_descramble(torch.from_numpy(frames).cuda(), rate, bool(short))
    torch.cuda.synchronize()
    assert tuple(out.shape) == (3, kb)
    assert np.array_equal(out.cpu().numpy(), want)
    other = frames.copy()
    other[:, kb:] ^= rng.integers(1, 256, (3, nb - kb), dtype=np.uint8)       # every byte behind the BBFRAME changes
    out2 = engine.bb_descramble(torch.from_numpy(other).cuda(), rate, bool(short))
    torch.cuda.synchronize()
    assert np.array_equal(out2.cpu().numpy(), want)
