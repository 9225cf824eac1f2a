"""GPU test of the handles' lifecycle (csrc/dev_buf.h: every handle and the context hold their device memory in owners): per handle
kind, at small sizes, create -> one call that reaches the members allocated on first use -> reset -> destroy, and the same again on
the same Engine; the second round's outputs equal the first round's and every call returns without an error.  A second Engine is
created and closed at the end.  Nothing here looks at the free device memory (the cards are shared), and nothing asks a card for
memory it does not have: the failure paths are tests/test_host_cpp_dev_buf.py's."""
import ctypes as C

import numpy as np
import pytest

import ma_gse_ref as G
import orc
import orc_bbts as B
import orc_dvbs as od
import pcr_cases as KP
import psi_cases as KS
import tsmon_ref as T

pytestmark = pytest.mark.gpu

CFG = {'issy_bytes': 0, 'crc_span': 0, 'reinsert_nulls': 1, 'check_crc': 1}
KBCH = 58192


@pytest.fixture(scope='module')
def eng(pkg):
    e = pkg.Engine(0)
    yield e
    e.close()


@pytest.fixture(scope='module')
def data():
    """the inputs of every kind, made once"""
    rng = np.random.default_rng(5)
    s2_iq, _, _ = orc.transmit(6, 1, 1, nframes=6, seed=21, esn0_db=14.0, cfo=1e-3, timing=0.3, phase0=0.2, lead_symbols=300)
    dvbs_iq, _ = od.dvbs_iq(2, 32768, seed=3, esn0_db=12.0, cfo=1e-4, timing=0.3, phase0=0.6)
    soft, _ = od.dvbs_tx(2, 2 * 8192, seed=3)
    gse_frames, _, gse_sel = G.scenario(1, False, False, 1, False)
    frag = B.gse_fragments(0x0800, rng.integers(0, 256, 300, dtype=np.uint8).tobytes(), [120], 3)       # one PDU across two frames of a reference-mode bank
    gse_ref = np.stack([B.gse_bbframe([B.gse_complete(0x0800, bytes(range(40))), frag[0]], 14232), B.gse_bbframe([frag[1], B.gse_complete(0x86DD, bytes(60))], 14232)])
    return dict(s2_iq=s2_iq, dvbs_iq=dvbs_iq, soft=soft, mux=T.make_mux(rng, 300, [0, 0x11, 0x100])[0], psi=KS.whole_stream(rng), pcr=KP.whole_stream(),
                bb=B.bbframes_from_ts(B.ts_packets(5 * (KBCH // 8 - 10) // 188 + 2, rng), KBCH, 5), gse=list(gse_frames), gse_sel=gse_sel, gse_ref=gse_ref,
                forney=rng.integers(0, 256, (1, 204 * 12), dtype=np.uint8), rs=rng.integers(0, 256, (8, 204), dtype=np.uint8))


def _demod(pkg, eng, d):
    dm = eng.demod(eng.default_cfg(6, True, True), max_samples=20000)
    dm.set_quality(True)
    out = [dm.process(d['s2_iq'][:20000])] + [dm.tap(t) for t in range(4)] + [dm.quality()]
    dm.reset()
    dm.close()
    return out


def _dvbs_demod(pkg, eng, d):
    bank, tail = pkg.DvbsDemodBank(eng, 1, max_samples=16384), pkg.DvbsTailBank(eng, 1)
    bank.set_quality(True)
    out = [bank.process(d['dvbs_iq'][:16384]), bank.quality(), bank.symbols()]
    iq, ts = np.ascontiguousarray(d['dvbs_iq'][16384:32768]), np.zeros(1 << 16, np.uint8)       # the TS entry point: its staging buffer
    n = eng._check(eng.lib.dvbs2gpu_dvbs_process_ts(bank.h, tail.h, int(iq.size), C.c_void_p(iq.ctypes.data), C.c_void_p(ts.ctypes.data), ts.size))
    out.append(ts[:n].copy())
    bank.reset(), tail.reset()
    bank.close(), tail.close()
    return out


def _dvbs_batch_handles(pkg, eng, d):
    import torch
    vit, dec, fy, tail = pkg.ViterbiBatch(eng, 1), pkg.CcDecoderBatch(eng, 1, 64), pkg.ForneyBatch(eng, 1), pkg.DvbsTailBank(eng, 1, max_bits=1632 * 8 * 8)
    out = [x.cpu().numpy() for x in vit.work(torch.from_numpy(d['soft'].reshape(1, 2, 8192)).cuda())]
    u8 = torch.from_numpy(d['soft'].view(np.uint8).reshape(1, -1)).cuda()
    out.append(dec.work(u8, 4, 2 * 64).cpu().numpy())
    out.append(fy.deinterleave(torch.from_numpy(d['forney']).cuda()).cpu().numpy())
    out.append(tail.rs_stage(d['rs'], skip_rs=True))                # host buffers: a temporary on the device
    state = np.array([0, 0, 0, 0], np.int32)
    out.append(np.asarray(eng.dvbs_depuncture(3, 0, d['soft'][:600].view(np.uint8), state)[0]))
    vit.reset(), tail.reset()
    for h in (vit, dec, fy, tail):
        h.close()
    return out


def _bbts(pkg, eng, d):
    bank = pkg.BbTsParserBank(eng, 1, KBCH, 8)
    out = [bank.work(d['bb'])]                                      # reference mode, host buffers
    bank.set_mode_adaptation(True, **CFG)
    bank.select_isi(0, d['gse_sel'])
    bank.ma_set_gse(True)
    lanes = bank.ma_work(d['gse'][:8])                              # GSE BBFRAMEs: contexts, records, rows and the slot pool
    assert bank.ma_gse_stats(0, 0)['frames'] > 0
    out += lanes + [bank.ma_pdu_table(0, 0)]
    bank.set_mode_adaptation(False)                                 # drops the mode's storage; the reference-mode parser starts afresh
    bank.close()
    return out


def _bbts_gse(pkg, eng, d):
    """a reference-mode bank that meets a GSE frame: the device storage of bbts_gse.hip"""
    bank = pkg.BbTsParserBank(eng, 1, 14232, 8)
    out = [bank.work(d['gse_ref']), bank.pdu_table(0)]
    assert bank.gse_stats(0)['frames'] > 0
    bank.close()
    return out


def _ts_banks(pkg, eng, d):
    mon, psi, pcr = pkg.TsMonitorBank(eng, 1, 512), pkg.PsiBank(eng, 1, 512), pkg.PcrBank(eng, 1, 512)
    psi.set_watch(0, 1, KS.PID)
    pcr.set_watch(0, 0, KP.PID), pcr.set_rate(0, KP.TPP_Q24)
    out = [mon.work(d['mux']), mon.pid_table(0), psi.work(d['psi'][:512]), psi.section_table(0), pcr.work(d['pcr'][:512]), pcr.row_table(0)]
    for b in (mon, psi, pcr):
        b.reset()
        b.close()
    return out


def _segrx(pkg, eng, d):
    import torch
    kb = pkg.modcod_info(6, True, True)['kbch'] // 8
    rx = pkg.SegmentReceiver(eng, eng.default_cfg(6, True, True), 2, 2, 2)
    iq = torch.from_numpy(d['s2_iq']).cuda()
    buf = torch.zeros(16 * kb, dtype=torch.uint8, device='cuda')
    out = []
    for a in range(0, 2 * rx.chunk_samples, rx.chunk_samples):     # two calls: the history buffers change places
        n = rx.process(iq[a:a + rx.chunk_samples], buf)
        out.append(buf[:n].cpu().numpy().copy())
    rx.reset()
    rx.close()
    return out


def _dvbs_segrx(pkg, eng, d):
    import torch
    rx = pkg.DvbsSegmentReceiver(eng, 2, 8192, 8192)
    iq = torch.from_numpy(d['dvbs_iq']).cuda()
    buf = torch.zeros(4 * rx.chunk_samples + 4 * 65536, dtype=torch.uint8, device='cuda')
    out = []
    for a in (0, rx.chunk_samples):
        n = rx.process(iq[a:a + rx.chunk_samples], buf)
        out += [buf[:n].cpu().numpy().copy(), rx.stats()]
    rx.reset()
    rx.close()
    return out


def _fleet(pkg, eng, d):
    fl = pkg.Fleet([0])
    fl.assign([eng.default_cfg(6, True, True), eng.default_cfg(4, True, False)], max_samples=20000, out_cap=1 << 16, tolerance=1.0)
    out = fl.process([d['s2_iq'][:20000], np.zeros(0, np.complex64)])
    fl.close()
    return out


def _context_tables(pkg, eng, d):
    """the context's own caches: FEC tables of two codes, a decoder-plan change that drops the LDPC cache, the ACM/VCM tables"""
    import torch
    llr = torch.zeros((2, 16200), dtype=torch.int8, device='cuda')
    llr[:] = 20
    out = [x.cpu().numpy() for x in eng.fec_decode(llr, 6, True, max_trials=4)]
    eng.set_option('ldpc_wave', 1 - int(eng.ldpc_decoder_form(6, True) == 1))
    out += [x.cpu().numpy() for x in eng.fec_decode(llr, 6, True, max_trials=4)]
    eng.set_option('ldpc_wave', -1)
    dm = eng.demod(eng.default_cfg(6, True, True, acm_vcm=1), max_samples=20000)
    out += dm.process(d['s2_iq'][:20000])
    dm.close()
    return out


KINDS = [_demod, _dvbs_demod, _dvbs_batch_handles, _bbts, _bbts_gse, _ts_banks, _segrx, _dvbs_segrx, _fleet, _context_tables]


@pytest.mark.parametrize('kind', KINDS, ids=[k.__name__.strip('_') for k in KINDS])
def test_create_use_reset_destroy_twice(pkg, eng, data, kind):
    first, again = kind(pkg, eng, data), kind(pkg, eng, data)
    assert len(first) == len(again) and len(first) > 0
    for k, (a, b) in enumerate(zip(first, again)):
        if isinstance(a, np.ndarray):
            assert a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes(), k
        else:
            assert a == b, k
    assert any(isinstance(a, np.ndarray) and a.size > 0 for a in first)


def test_a_second_engine_is_created_and_closed(pkg, eng):
    import torch
    second = pkg.Engine(0)
    llr = torch.full((1, 16200), 20, dtype=torch.int8, device='cuda')
    out = [x.cpu().numpy() for x in second.fec_decode(llr, 6, True, max_trials=4)]
    second.close()
    want = [x.cpu().numpy() for x in eng.fec_decode(llr, 6, True, max_trials=4)]
    assert all(np.array_equal(a, b) for a, b in zip(out, want))
