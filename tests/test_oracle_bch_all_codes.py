"""The CPU oracle's BCH decoder on the constructed patterns of tests/bch_patterns.py, for all 21 codes: against what the code itself
promises and, when oracle/_ref is built, against the reference's decoder on every pattern (the oracle's BCH pin over all codes)."""
import numpy as np
import pytest

import bch_patterns as bp
import orc

needs_ref = pytest.mark.skipif(orc.ref() is None, reason='oracle/_ref not built (reference sources absent)')


@pytest.mark.parametrize('rate,short', orc.ALL_CODES)
def test_bch_pattern_list_is_what_it_says(rate, short):
    """every family is there, the clean frames sit at both ends, the list stays small, and it is the same list on every call"""
    pats = bp.patterns(rate, short)
    p = orc.fec_params(rate, short)
    fams = [bp.family(q.name) for q in pats]
    assert fams[0] == 'clean' and fams[-1] == 'clean' and fams.count('clean') == 2
    assert set(fams) == {'clean', 'single', 'pair', 't-1', 't', 'shortened', 'beyond'}
    assert fams.count('shortened') == 3 * len(bp.shortened_shifts(p)) == 12
    assert len(pats) <= 72
    assert len({q.name for q in pats}) == len(pats)
    for q in pats:
        assert q.frame.shape == (p['K'] // 8,) and q.frame.dtype == np.uint8
        if q.flips is not None:
            diff = np.flatnonzero(np.unpackbits(q.frame ^ q.sent))
            assert tuple(diff) == q.flips, q.name
            assert bp.syndromes(rate, short, q.sent) == [0] * (2 * p['t']), q.name
    bp.patterns.cache_clear()
    again = bp.patterns(rate, short)
    assert [q.name for q in again] == [q.name for q in pats] and all(np.array_equal(a.frame, b.frame) for a, b in zip(again, pats))


@pytest.mark.parametrize('rate,short', orc.ALL_CODES)
def test_bch_oracle_constructed_patterns(rate, short):
    """clean, single, pair, t-1, t: as many corrections as bits were flipped and the transmitted codeword back; shortened: -1 and the frame as it came
    (the reference agrees with this expectation on all 21 codes, test below); beyond: no claim of its own"""
    ret, frames = bp.oracle_outcomes(rate, short)
    bp.check_independent(rate, short, ret, frames)


@needs_ref
@pytest.mark.parametrize('rate,short', orc.ALL_CODES)
def test_bch_oracle_equals_reference_on_constructed_patterns(rate, short):
    """the reference's decoder is the authority: same return value and same bytes as the oracle on every pattern of every code, the patterns beyond the
    code's correction capacity included; and the oracle's encoder is the reference's"""
    pats = bp.patterns(rate, short)
    ret, frames = bp.oracle_outcomes(rate, short)
    p = orc.fec_params(rate, short)
    enc = np.zeros(p['K'] // 8, np.uint8)
    enc[:p['kbch'] // 8] = pats[0].sent[:p['kbch'] // 8]
    orc.ref().ref_bch_encode(rate, short, enc)
    assert np.array_equal(enc, pats[0].sent)
    for n, q in enumerate(pats):
        fr = q.frame.copy()
        r = orc.ref().ref_bch_decode(rate, short, fr)
        assert r == ret[n], (q.name, r, int(ret[n]))
        assert np.array_equal(fr, frames[n]), q.name
