"""GPU parity tests for the DVB-S inner-code path (rows a18-a20), through the C ABI, against the CPU oracle (bit-exact)."""
import numpy as np
import pytest
import orc_dvbs as od
from orc_dvbs import P, VP

pytestmark = pytest.mark.gpu


def test_slice_matches_oracle(engine, pkg):
    import torch
    rng = np.random.default_rng(1)
    n = 8192 * 3 // 2
    iq = rng.normal(0, 0.9, 2 * n).astype(np.float32)
    iq[:10] = [1.27, -1.27, 1.2700001, -1.2700001, 1.28, -1.28, 0.0099999, -0.0099999, 50.0, -50.0]
    soft = pkg.dvbs_slice(engine, torch.from_numpy(iq).view(torch.complex64).cuda()).cpu().numpy()
    o = od.L()
    h = VP(o.orc_dvbs_slicer_create())
    exp = np.zeros(3 * 8192, np.int8)
    got_n = o.orc_dvbs_slicer_process(h, n, P(iq), P(exp))
    o.orc_dvbs_slicer_destroy(h)
    assert got_n == 3 * 8192 and (soft == exp).all()
    assert pkg.dvbs_slice(engine, torch.zeros(0, dtype=torch.complex64, device='cuda')).numel() == 0


@pytest.mark.parametrize('frame', od.CCDEC_FRAMES)
def test_ccdec_chained_blocks_bit_exact(engine, pkg, frame):
    import torch
    S, nblk = 6, 4
    stride = 2 * frame
    soft = od.ccdec_case_softs(frame, S, nblk)
    dec = pkg.CcDecoderBatch(engine, S, frame)
    got = dec.work(torch.from_numpy(soft).cuda(), nblk, stride).cpu().numpy()
    got2 = dec.work(torch.from_numpy(soft).cuda(), nblk, stride).cpu().numpy()   # second call continues the chain
    o = od.L()
    for s in range(S):
        h = VP(o.orc_ccdec_create(frame))
        for rep, g in ((0, got), (1, got2)):
            for b in range(nblk):
                out = np.zeros(frame, np.uint8)
                o.orc_ccdec_work(h, P(soft[s, stride * b:]), P(out))
                assert (g[s, b] == out).all(), (s, rep, b, int((g[s, b] != out).sum()))
        o.orc_ccdec_destroy(h)
    dec.close()


def _check_viterbi(names, soft, gb, gn, gs, thr, max_outsync, want=None):
    """want: the oracle's (bits, counts, stats) per stream where the caller has them already"""
    for s, name in enumerate(names):
        eb, en, es = want[s] if want is not None else od.OracleViterbi(thr, max_outsync).work(soft[s])
        assert (gn[s] == en).all(), (name, gn[s], en)
        assert (gs[s] == es).all(), (name, gs[s], es)
        for b in range(soft.shape[1]):
            n = int(en[b])
            if es[b, 2] == 3:
                n = min(n, 6799)   # rate 5/6: the reference's decoder leaves [6799, nbits) unwritten
            assert (gb[s, b, :n] == eb[b, :n]).all(), (name, b, int((gb[s, b, :n] != eb[b, :n]).sum()))


def test_viterbi_dvbs_bit_exact(engine, pkg):
    import torch
    nb = 8
    cases = od.viterbi_case_streams(nb)
    soft = np.stack([c[1] for c in cases])
    vit = pkg.ViterbiBatch(engine, len(cases), 0.15, 3)     # short watchdog so the relock case goes through IDLE again
    d = torch.from_numpy(soft).cuda()
    # two calls of 3 + 5 blocks: state must carry across calls exactly like one call of 8
    gb1, gn1, gs1 = vit.work(d[:, :3].contiguous())
    gb2, gn2, gs2 = vit.work(d[:, 3:].contiguous())
    gb = torch.cat([gb1, gb2], 1).cpu().numpy(); gn = torch.cat([gn1, gn2], 1).cpu().numpy(); gs = torch.cat([gs1, gs2], 1).cpu().numpy()
    _check_viterbi([c[0] for c in cases], soft, gb, gn, gs, 0.15, 3)
    # sanity on the scenario itself: every coded stream locked to its rate, noise never did
    for s, (name, _) in enumerate(cases):
        if name.startswith('rate'):
            assert (gs[s, :, 1] == 1).all() and (gs[s, :, 2] == int(name[4])).all(), name
        if 'noise' in name:
            assert (gn[s] == 0).all()
    relock = gs[[c[0] for c in cases].index('relock')]
    assert relock[0, 2] == 1 and relock[-1, 2] == 3 and 0 in relock[:, 1]
    # reset brings the handle back to a fresh decoder
    vit.reset()
    gb3, gn3, gs3 = vit.work(d[:, :3].contiguous())
    assert (gn3.cpu().numpy() == gn[:, :3]).all() and (gs3.cpu().numpy() == gs[:, :3]).all()
    vit.close()


def test_viterbi_lock_search_every_reachable_lock(engine, pkg):
    """the ST_IDLE search on od.viterbi_lock_streams(): one stream per final lock a coded stream can produce (34 of the 52 hypotheses), coded streams
    that stay IDLE, locks in the middle of a call at shifts with a leading erasure, and re-locks at the same punctured rate (the de-puncturer's
    stale got_extra / buf) -- all in one batch, as calls of 3 + 5 blocks; the streams' own preconditions are asserted on the oracle alone"""
    import torch
    from concurrent.futures import ThreadPoolExecutor
    streams = od.viterbi_lock_streams()
    names = [s[0] for s in streams]
    soft = np.stack([s[1] for s in streams])
    wd = od.VITERBI_LOCK_WATCHDOG
    od.L()
    with ThreadPoolExecutor(max_workers=16) as ex:
        want = list(ex.map(lambda x: od.OracleViterbi(0.15, wd).work(x), [s[1] for s in streams]))
    od.check_viterbi_lock_streams(streams, want)
    vit = pkg.ViterbiBatch(engine, len(streams), 0.15, wd)
    d = torch.from_numpy(soft).cuda()
    parts = [vit.work(d[:, :3].contiguous()), vit.work(d[:, 3:].contiguous())]
    gb, gn, gs = [torch.cat([p[k] for p in parts], 1).cpu().numpy() for k in range(3)]
    vit.close()
    _check_viterbi(names, soft, gb, gn, gs, 0.15, wd, want)


def test_viterbi_dvbs_default_watchdog(engine, pkg):
    import torch
    nb = 4
    soft = np.stack([od.dvbs_tx(r, nb * 8192, seed=600 + r, sigma=20.0)[0].reshape(nb, 8192) for r in range(5)])
    vit = pkg.ViterbiBatch(engine, 5)
    gb, gn, gs = [x.cpu().numpy() for x in vit.work(torch.from_numpy(soft).cuda())]
    _check_viterbi([f'r{r}' for r in range(5)], soft, gb, gn, gs, 0.15, 20)
    vit.close()


def test_viterbi_many_streams_identical(engine, pkg):
    """size-independent property at scale: 1024 streams fed the same blocks produce identical output"""
    import torch
    soft, bits = od.dvbs_tx(2, 2 * 8192, seed=9)
    S = 1024
    d = torch.from_numpy(soft.reshape(1, 2, 8192)).cuda().repeat(S, 1, 1).contiguous()
    vit = pkg.ViterbiBatch(engine, S)
    gb, gn, gs = vit.work(d)
    assert bool((gb == gb[0:1]).all()) and bool((gn == gn[0:1]).all()) and bool((gs == gs[0:1]).all())
    g0 = gb[0, 0, :6144].cpu().numpy()
    assert (g0[:6000] == bits[:6000]).mean() > 0.999
    vit.close()


def test_forney_bit_exact_across_calls(engine, pkg):
    import torch
    rng = np.random.default_rng(3)
    S = 5
    f = pkg.ForneyBatch(engine, S)
    o = od.L()
    hs = [VP(o.orc_forney_create()) for _ in range(S)]
    for groups in (1, 3, 1, 7):
        x = rng.integers(0, 256, (S, groups * 1632), dtype=np.uint8)
        got = f.deinterleave(torch.from_numpy(x).cuda()).cpu().numpy()
        for s in range(S):
            for g in range(groups):
                e = np.zeros(1632, np.uint8)
                o.orc_forney_deinterleave(hs[s], P(np.ascontiguousarray(x[s, g * 1632:(g + 1) * 1632])), P(e))
                assert (got[s, g * 1632:(g + 1) * 1632] == e).all(), (groups, s, g)
    for h in hs:
        o.orc_forney_destroy(h)
    f.close()


def test_dvbs_error_codes(engine, pkg):
    import ctypes as C
    lib = engine.lib
    h = C.c_void_p()
    assert lib.dvbs2gpu_viterbi_create(engine.h, 0, 0.15, 20, C.byref(h)) == pkg.ERR_ARG
    assert lib.dvbs2gpu_ccdec_create(engine.h, 4, 2, C.byref(h)) == pkg.ERR_ARG
    assert lib.dvbs2gpu_forney_create(None, 4, C.byref(h)) == pkg.ERR_ARG
    f = pkg.ForneyBatch(engine, 1)
    assert lib.dvbs2gpu_forney_deinterleave_batch(f.h, None, 1632, None, None) == pkg.ERR_ARG
    assert lib.dvbs2gpu_forney_deinterleave_batch(f.h, None, 7, None, None) == pkg.ERR_ARG
    assert lib.dvbs2gpu_forney_deinterleave_batch(f.h, None, 0, None, None) == 0
    f.close()
