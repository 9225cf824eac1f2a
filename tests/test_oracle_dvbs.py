"""CPU tests of the DVB-S oracle (oracle/dvbs.cpp): pinned against the compiled reference (de-puncturers, Forney de-interleaver, soft
rotation as they are; Viterbi_DVBS, CCDecoder and CCEncoder over the stand-in headers of oracle/shim), plus
encode -> noise -> decode round trips and lock behaviour."""
import ctypes as C
import numpy as np
import pytest
import orc
import orc_dvbs as od
from orc_dvbs import P, VP


def _ref():
    r = orc.ref()
    if r is None or not hasattr(r, 'ref_forney_create'):
        pytest.skip('oracle/_ref not built')
    for n in ('ref_depunc23_create', 'ref_depunc56_create', 'ref_forney_create'):
        getattr(r, n).restype = VP
    r.ref_depunc23_static.argtypes = r.ref_depunc56_static.argtypes = [VP, VP, VP, C.c_int, C.c_int]
    r.ref_depunc23_cont.argtypes = r.ref_depunc56_cont.argtypes = [VP, VP, VP, C.c_int]
    r.ref_depunc23_set_shift.argtypes = r.ref_depunc56_set_shift.argtypes = [VP, C.c_int]
    r.ref_forney_deinterleave.argtypes = [VP, VP, VP]
    r.ref_rotate_soft.argtypes = [VP, C.c_int, C.c_int, C.c_int]
    return r


@pytest.mark.parametrize('period,nm', [(3, '23'), (6, '56')])
def test_depunc_matches_reference(period, nm):
    o, r = od.L(), _ref()
    rng = np.random.default_rng(period)
    for shift in range(2 * period):
        ho = VP(o.orc_depunc_create(period)); hr = VP(getattr(r, f'ref_depunc{nm}_create')())
        for size in (2048, 8192, 100, 7):
            x = rng.integers(0, 256, size, dtype=np.uint8)
            a = np.full(4 * size + 64, 7, np.uint8); b = a.copy()
            na = o.orc_depunc_static(ho, P(x), P(a), size, shift)
            nb = getattr(r, f'ref_depunc{nm}_static')(hr, P(x), P(b), size, shift)
            assert na == nb and (a == b).all()
        o.orc_depunc_set_shift(ho, shift); getattr(r, f'ref_depunc{nm}_set_shift')(hr, shift)
        for size in (8192, 8192, 8191, 8192, 33, 8192, 8192):
            x = rng.integers(0, 256, size, dtype=np.uint8)
            a = np.full(4 * size + 64, 9, np.uint8); b = a.copy()
            na = o.orc_depunc_cont(ho, P(x), P(a), size)
            nb = getattr(r, f'ref_depunc{nm}_cont')(hr, P(x), P(b), size)
            assert na == nb and (a == b).all()
        o.orc_depunc_destroy(ho)


def test_forney_matches_reference_and_closed_form():
    o, r = od.L(), _ref()
    rng = np.random.default_rng(5)
    ho = VP(o.orc_forney_create()); hr = VP(r.ref_forney_create())
    xs, ys = [], []
    for _ in range(6):
        x = rng.integers(0, 256, 1632, dtype=np.uint8); a = np.zeros_like(x); b = np.zeros_like(x)
        o.orc_forney_deinterleave(ho, P(x), P(a)); r.ref_forney_deinterleave(hr, P(x), P(b))
        assert (a == b).all()
        xs.append(x); ys.append(b)
    xi, xo = np.concatenate(xs), np.concatenate(ys)
    n = np.arange(len(xi)); p = n - 204 * (11 - n % 12)
    assert (np.where(p >= 0, xi[np.maximum(p, 0)], 0) == xo).all()   # the gather form the GPU kernel uses


def test_rotate_soft_matches_reference():
    o, r = od.L(), _ref()
    rng = np.random.default_rng(6)
    for phase in range(4):
        for sw in (0, 1):
            x = rng.integers(-128, 128, 4096, dtype=np.int8); a = x.copy(); b = x.copy()
            o.orc_rotate_soft(P(a), 4096, phase, sw); r.ref_rotate_soft(P(b), 4096, phase, sw)
            assert (a == b).all()


def test_slicer_blocks_and_clamp():
    o = od.L()
    h = VP(o.orc_dvbs_slicer_create())
    rng = np.random.default_rng(7)
    iq = (rng.normal(0, 0.8, 2 * 5000)).astype(np.float32)
    iq[:6] = [1.27, -1.27, 1.2701, -1.28, 5.0, -5.0]
    out = np.zeros(3 * 8192, np.int8)
    n1 = o.orc_dvbs_slicer_process(h, 5000, P(iq), P(out))
    assert n1 == 8192
    exp = np.clip(np.trunc(iq * np.float32(100)), -127, 127).astype(np.int8)
    assert (out[:8192] == exp[:8192]).all()
    n2 = o.orc_dvbs_slicer_process(h, 5000, P(iq), P(out))     # 1808 left over + 10000 new -> one more block
    assert n2 == 8192 and (out[:1808] == exp[8192:]).all() and (out[1808:8192] == exp[:8192 - 1808]).all()
    o.orc_dvbs_slicer_destroy(h)


def test_cc_roundtrip_chained_blocks():
    o = od.L()
    rng = np.random.default_rng(8)
    frame, nblk = 512, 6
    bits = rng.integers(0, 2, frame * nblk + 16, dtype=np.uint8)
    enc = od.cc_encode(bits)
    soft = np.where(enc > 0, 127 + 40, 127 - 40) + rng.normal(0, 14, len(enc))
    soft = np.clip(np.rint(soft), 0, 255).astype(np.uint8)
    soft[soft == 128] = 127
    h = VP(o.orc_ccdec_create(frame))
    for b in range(nblk):
        out = np.zeros(frame, np.uint8)
        o.orc_ccdec_work(h, P(soft[2 * frame * b:]), P(out))
        assert (out == bits[frame * b:frame * (b + 1)]).all()
    o.orc_ccdec_destroy(h)


@pytest.mark.parametrize('rate', range(5))
@pytest.mark.parametrize('variant', [(0, False), (1, True)])
def test_viterbi_dvbs_locks_and_decodes(rate, variant):
    drop, rot = variant
    if drop and rate in (2, 4):
        drop = 2      # 3/4 and 7/8 hypotheses shift by whole I/Q pairs (viterbi_all.h:92-150)
    nb = 4
    soft, bits = od.dvbs_tx(rate, nb * 8192, seed=100 + rate, drop=drop, rot90=rot)
    v = od.OracleViterbi()
    out, nbits, stats = v.work(soft.reshape(nb, 8192))
    assert (stats[:, 1] == 1).all() and (stats[:, 2] == rate).all(), stats
    assert (stats[:, 3] == (1 if rot else 0)).all()
    got = np.concatenate([out[b, :(nbits[b] if rate != 3 else min(nbits[b], 6799))] for b in range(nb)])
    if rate == 3:
        # rate 5/6: the reference's main decoder handles 6799 of the ~6826 bits of a block (SURVEY Q-list): only block 0 lines up
        got = out[0, :6799]
    # decoded stream equals the transmitted bits from some small offset on
    ok = False
    for off in range(0, 12):
        n = min(len(got), len(bits) - off) - 64
        if n > 1000 and (got[:n] == bits[off:off + n]).mean() > 0.999:
            ok = True
            break
    assert ok
    assert np.frombuffer(stats[:, 0].astype(np.int32).tobytes(), np.float32).max() < 0.15


def test_viterbi_dvbs_noise_never_locks_and_watchdog_unlocks():
    rng = np.random.default_rng(11)
    noise = rng.integers(-60, 61, (3, 8192)).astype(np.int8)
    v = od.OracleViterbi(max_outsync=2)
    out, nbits, stats = v.work(noise)
    assert (nbits == 0).all() and (stats[:, 1] == 0).all()
    soft, _ = od.dvbs_tx(2, 2 * 8192, seed=12)
    _, nbits, stats = v.work(soft.reshape(2, 8192))
    assert (stats[:, 1] == 1).all() and (nbits == 6144).all()
    _, nbits, stats = v.work(rng.integers(-60, 61, (5, 8192)).astype(np.int8))
    # invalid counts 1, 2, 3 (> max_outsync = 2 -> IDLE after the third bad block), then stays idle
    assert list(stats[:, 1]) == [1, 1, 0, 0, 0] and list(nbits) == [6144, 6144, 6144, 0, 0]


# ---------------------------------------------------------------- committed golden vectors (generated from the reference)
def _golden():
    import json, os
    with open(os.path.join(os.path.dirname(__file__), 'golden', 'dvbs_golden.json')) as f:
        return json.load(f)


def _sha(a):
    import hashlib
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def test_depunc_golden_vectors():
    o = od.L()
    for case in _golden()['depunc']:
        rng = np.random.default_rng(case['seed'])
        h = VP(o.orc_depunc_create(case['period']))
        x = rng.integers(0, 256, 2048, dtype=np.uint8)
        out = np.full(8192 + 64, 7, np.uint8)
        n = o.orc_depunc_static(h, P(x), P(out), 2048, case['shift'])
        assert n == case['static_n'] and _sha(out[:n]) == case['static_sha']
        o.orc_depunc_set_shift(h, case['shift'])
        for c in case['cont']:
            x = rng.integers(0, 256, c['size'], dtype=np.uint8)
            out = np.full(4 * c['size'] + 64, 9, np.uint8)
            n = o.orc_depunc_cont(h, P(x), P(out), c['size'])
            assert n == c['n'] and _sha(out[:n + 1]) == c['sha']
        o.orc_depunc_destroy(h)


def test_forney_and_rotation_golden_vectors():
    o = od.L()
    g = _golden()
    rng = np.random.default_rng(g['forney']['seed'])
    h = VP(o.orc_forney_create())
    outs = []
    for _ in range(g['forney']['calls']):
        x = rng.integers(0, 256, 1632, dtype=np.uint8)
        e = np.zeros(1632, np.uint8)
        o.orc_forney_deinterleave(h, P(x), P(e))
        outs.append(e)
    assert _sha(np.concatenate(outs)) == g['forney']['sha'] and outs[0][-16:].tolist() == g['forney']['first_call_tail_16']
    o.orc_forney_destroy(h)
    for c in g['rotate']:
        rng = np.random.default_rng(c['seed'])
        x = rng.integers(-128, 128, 512, dtype=np.int8)
        o.orc_rotate_soft(P(x), 512, c['phase'], c['iqswap'])
        assert _sha(x) == c['sha']


# ---------------------------------------------------------------- Viterbi_DVBS / CCDecoder / CCEncoder pinned to the compiled reference
def _ref_inner():
    r = od.R()
    if r is None:
        pytest.skip('oracle/_ref not built')
    return r


_streams = {}


def _viterbi_streams():
    if not _streams:
        _streams.update(od.viterbi_case_streams(8))
    return _streams


@pytest.mark.parametrize('thr,max_outsync', [(0.15, 3), (0.15, 20)])
def test_viterbi_dvbs_matches_reference(thr, max_outsync):
    """Viterbi_DVBS::work over 8 blocks of 8192 softs per stream: per block the output count, state / rate / phase / shift, the BER as
    float bits and the whole output buffer (pre-filled alike on both sides: rate 5/6 leaves bits [6799, count) unwritten)"""
    _ref_inner()
    for name, soft in _viterbi_streams().items():
        eb, en, es = od.RefViterbi(thr, max_outsync).work(soft, fill=0xA5)
        ob, on, os_ = od.OracleViterbi(thr, max_outsync).work(soft, fill=0xA5)
        assert (on == en).all(), (name, on, en)
        assert (os_ == es).all(), (name, os_, es)
        assert (ob == eb).all(), (name, np.argwhere(ob != eb)[:4])
    # the scenario did what it is for: every rate locked, both phases, non-zero shifts, the relock stream fell back to IDLE
    seen = np.concatenate([od.OracleViterbi(thr, max_outsync).work(s)[2] for s in _viterbi_streams().values()])
    locked = seen[seen[:, 1] == 1]
    assert set(locked[:, 2]) == set(range(5)) and set(locked[:, 3]) == {0, 1} and (locked[:, 4] > 1).any() and (seen[:, 1] == 0).any()


def _oracle_lock_results(streams):
    from concurrent.futures import ThreadPoolExecutor
    od.L()                                                        # (bind the library before the pool starts)
    with ThreadPoolExecutor(max_workers=16) as ex:
        return list(ex.map(lambda x: od.OracleViterbi(0.15, od.VITERBI_LOCK_WATCHDOG).work(x, fill=0xA5), [s[1] for s in streams]))


def test_viterbi_lock_streams_reach_what_they_are_for():
    """on the oracle alone: the final locks of the 'lock' streams are the 34 reachable ones, the odd-drop 3/4 and 7/8 streams stay IDLE with count 0,
    the late streams lock in block 2 at a shift with a leading erasure, and a same-rate re-lock yields other counts than a fresh decoder"""
    streams = od.viterbi_lock_streams()
    kinds = [s[2] for s in streams]
    assert kinds.count('lock') == 34 and kinds.count('idle') >= 4 and kinds.count('late') == 4 and kinds.count('relock') == 2
    assert {s[3][0] for s in streams if s[2] == 'relock'} == {1, 3} and {s[0][:7] for s in streams if s[2] == 'idle'} == {'idle_r2', 'idle_r4'}
    od.check_viterbi_lock_streams(streams, _oracle_lock_results(streams))


def test_viterbi_lock_streams_match_reference():
    """the same list through the reference's Viterbi_DVBS: counts, stats rows and the written bits (viterbi_written_bits); rate, phase and shift read 0
    before the first lock on both sides"""
    _ref_inner()
    streams = od.viterbi_lock_streams()
    wd = od.VITERBI_LOCK_WATCHDOG
    for (name, soft, kind, lock), (ob, on, os_) in zip(streams, _oracle_lock_results(streams)):
        eb, en, es = od.RefViterbi(0.15, wd).work(soft, fill=0xA5)
        assert (on == en).all(), (name, on, en)
        assert (os_ == es).all(), (name, os_, es)
        assert np.array_equal(od.viterbi_written_bits(ob, on, os_), od.viterbi_written_bits(eb, en, es)), name
        first = int(np.argmax(es[:, 1] == 1)) if (es[:, 1] == 1).any() else len(es)
        assert (es[:first, 2:5] == 0).all() and (os_[:first, 2:5] == 0).all(), name


@pytest.mark.parametrize('frame', od.CCDEC_FRAMES)
def test_ccdec_chained_blocks_match_reference(frame):
    """CCDecoder::work, 4 chained blocks twice over, six input kinds (noise levels, erasures, garbage)"""
    o, r = od.L(), _ref_inner()
    soft = od.ccdec_case_softs(frame)
    for s in range(soft.shape[0]):
        ho, hr = VP(o.orc_ccdec_create(frame)), VP(r.ref_ccdec_create(frame))
        for rep in range(2):
            for b in range(4):
                x = np.ascontiguousarray(soft[s, 2 * frame * b:])
                a = np.full(frame + 8, 0xA5, np.uint8); e = a.copy()
                o.orc_ccdec_work(ho, P(x), P(a)); r.ref_ccdec_work(hr, P(x.copy()), P(e))
                assert (a == e).all(), (s, rep, b, int((a != e).sum()))
        o.orc_ccdec_destroy(ho); r.ref_ccdec_destroy(hr)


def test_ccenc_matches_reference():
    """CCEncoder::work on random bits (values 0..255: only bit 0 counts), the register carried across calls"""
    o, r = od.L(), _ref_inner()
    rng = np.random.default_rng(9)
    for frame in (1, 7, 1024, 1792):
        ho, hr = VP(o.orc_ccenc_create(frame)), VP(r.ref_ccenc_create(frame))
        for rep in range(3):
            x = rng.integers(0, 256 if rep == 2 else 2, frame, dtype=np.uint8)
            a = np.full(2 * frame + 8, 0xA5, np.uint8); e = a.copy()
            o.orc_ccenc_work(ho, P(x), P(a)); r.ref_ccenc_work(hr, P(x.copy()), P(e))
            assert (a == e).all(), (frame, rep)
            if rep == 0:
                assert (od.cc_encode(x) == e[:2 * frame]).all()
        o.orc_ccenc_destroy(ho); r.ref_ccenc_destroy(hr)
