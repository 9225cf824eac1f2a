"""CPU tests of the RS(204,188) oracle (oracle/dvbs_tail.cpp) on the constructed error patterns of tests/rs_patterns.py: what follows from the
code alone, and the reference's own libcorrect decoder + DVBSReedSolomon wrapper compiled in place (oracle/_ref) on every pattern."""
import numpy as np
import pytest

import orc
import orc_dvbs_tail as ot
import rs_patterns as rp
from orc_dvbs import P, VP


def _ref():
    r = orc.ref()
    if r is None or not hasattr(r, 'ref_dvbsrs_create'):
        pytest.skip('oracle/_ref not built')
    r.ref_dvbsrs_create.restype = VP
    r.ref_dvbsrs_decode.argtypes = [VP, VP]
    return r


def test_pattern_set_is_what_the_families_promise():
    pats = rp.patterns()
    cnt = rp.family_counts()
    assert cnt == {'clean': 5, 'single': 204, 'zero-syn': 9, 't-1': 6, 't': 6, 'miscorrect': 18, 'beyond': 18}
    assert 10 * cnt['beyond'] < len(pats)
    assert sorted(q.flips[0] for q in pats if rp.family(q.name) == 'single') == list(range(204))
    for q in pats:
        fam = rp.family(q.name)
        assert (q.expect is None) == (fam == 'beyond')
        clean = not any(rp.syndromes(q.packet))
        assert clean == (fam == 'clean'), q.name
        assert not any(rp.syndromes(q.sent)), q.name
        if fam in ('single', 'zero-syn', 't-1', 't'):
            assert 1 <= len(q.flips) <= 8 and np.array_equal(q.expect.corrected, q.sent)
        if fam == 'miscorrect':
            na, nb = (int(x) for x in q.name.split('/')[1].split('-')[0].split('+'))
            moved = np.count_nonzero(q.expect.corrected != q.packet)
            assert len(q.flips) == na and na > 8 and moved == nb - q.expect.padding and q.expect.rs_err <= moved
            assert np.count_nonzero(q.expect.corrected[:188] != q.sent[:188]) >= q.expect.rs_err           # a wrong message comes out
        if fam == 'beyond':
            assert len(q.flips) == int(q.name.split('/')[1].split('-')[0])
    assert sum(q.expect is not None and q.expect.padding > 0 for q in pats) == 14
    assert pats is rp.patterns()


def test_oracle_meets_the_independent_expectations():
    out = rp.oracle_outcomes()
    rp.check_independent(out.status, out.message, out.rs_err)
    assert 0 in out.status and 1 in out.status


def test_reference_wrapper_on_every_pattern_fresh_wrapper_each():
    r = _ref()
    out = rp.oracle_outcomes()
    for n, q in enumerate(rp.patterns()):
        data = q.packet.copy()
        ret = r.ref_dvbsrs_decode(VP(r.ref_dvbsrs_create()), P(data))
        assert ret == out.rs_err[n], (q.name, ret, int(out.rs_err[n]))
        # a fresh wrapper that gives up hands out its zeroed buffer
        assert np.array_equal(data[:188], out.message[n] if out.status[n] else np.zeros(188, np.uint8)), q.name
        assert np.array_equal(data[188:], q.packet[188:]), q.name


def _one_wrapper(decode, handle, order):
    pats = rp.patterns()
    rets, msgs = [], []
    for n in order:
        data = pats[n].packet.copy()
        rets.append(int(decode(handle, P(data))))
        msgs.append(data[:188].copy())
    return rets, np.stack(msgs)


@pytest.mark.parametrize('shuffle', [False, True])
def test_reference_wrapper_all_patterns_through_one_wrapper(shuffle):
    """return values and the 188 bytes handed out, the stale-output rule included: a packet the decoder gives up on comes out as the last
    message that decoded"""
    o, r = ot.L(), _ref()
    out = rp.oracle_outcomes()
    order = list(range(len(rp.patterns())))
    if shuffle:
        order = [int(n) for n in np.random.default_rng(31).permutation(len(order))]
    ra, ma = _one_wrapper(o.orc_dvbsrs_decode, VP(o.orc_dvbsrs_create()), order)
    rb, mb = _one_wrapper(r.ref_dvbsrs_decode, VP(r.ref_dvbsrs_create()), order)
    assert ra == rb
    assert np.array_equal(ma, mb)
    # the stale-output rule, from the per-pattern outcomes: it was exercised, and it is what the two wrappers did
    prev, stale = np.zeros(188, np.uint8), 0
    for k, n in enumerate(order):
        if out.status[n]:
            prev = out.message[n]
        else:
            stale += 1
        assert np.array_equal(ma[k], prev), (k, rp.patterns()[n].name)
    assert stale >= 10


def test_high_degree_locators_oracle_reproduces_the_recorded_reference_outcomes():
    """the eight packets of tests/golden/rs_high_degree.json: Berlekamp-Massey ends with a locator of degree 9, which has 9 roots, and the decoder
    hands out a message (up to nine changed message bytes)"""
    o = ot.L()
    cases = rp.high_degree()
    assert len(cases) == 8
    for k, c in enumerate(cases):
        loc2, msg = np.zeros(2, np.int32), np.zeros(239, np.uint8)
        assert o.orc_rs255_locator(P(rp.padded(c.packet[None])[0].copy()), P(msg), P(loc2)) == 239
        assert loc2[0] == loc2[1] == c.order >= 9, (k, loc2)
        data = c.packet.copy()
        assert o.orc_dvbsrs_decode(VP(o.orc_dvbsrs_create()), P(data)) == c.ret
        assert np.array_equal(data[:188], c.message) and np.array_equal(data[:188], msg[51:]), k
        assert c.ret == np.count_nonzero(c.message != c.packet[:188]) and np.count_nonzero(c.packet != c.sent) > 16
    assert max(c.ret for c in cases) > 8


def test_high_degree_locators_reference_reproduces_its_recorded_outcomes():
    r = _ref()
    for k, c in enumerate(rp.high_degree()):
        data = c.packet.copy()
        assert r.ref_dvbsrs_decode(VP(r.ref_dvbsrs_create()), P(data)) == c.ret, k
        assert np.array_equal(data[:188], c.message), k
