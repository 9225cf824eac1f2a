"""The FEC encoder (csrc/fec_encode.hip) and the channel-error count on the GPU against the CPU oracle's encoders, byte for byte: all 21 codes as one call and stage
by stage on constructed messages, odd frame counts with sentinel rows, the round trip through the pinned decoder, the error count on constructed LLRs and behind
the receiver, and the argument errors.  Every comparison is exact."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import orc

pytestmark = pytest.mark.gpu

CODE_IDS = ['%s-%s' % (orc.RATE_NAMES[r].replace('/', '_'), 'short' if s else 'normal') for r, s in orc.ALL_CODES]
AMPLITUDE = 20


def dev(a):
    return torch.from_numpy(np.array(a, order='C')).cuda()          # (a copy: the shared references are read-only)


def oracle_scramble(bb, p):
    """BBFRAME -> K / 8 bytes: scrambled message, parity area zero"""
    fr = np.zeros(p['K'] // 8, np.uint8)
    fr[:p['kbch'] // 8] = bb
    orc.lib().orc_bb_descramble(fr, p['kbch'] // 8)          # (XOR with the PRBS: its own inverse)
    return fr


def oracle_bch(msg, rate, short, p):
    fr = np.zeros(p['K'] // 8, np.uint8)
    fr[:p['kbch'] // 8] = msg
    orc.lib().orc_bch_encode(rate, short, fr)
    return fr


def oracle_ldpc(info, rate, short, p):
    bits = np.zeros(p['N'], np.uint8)
    bits[:p['K']] = np.unpackbits(info)
    assert orc.lib().orc_ldpc_encode(rate, short, bits) == 0
    return np.packbits(bits)


def oracle_encode(bb, rate, short):
    p = orc.fec_params(rate, short)
    return oracle_ldpc(oracle_bch(oracle_scramble(bb, p)[:p['kbch'] // 8], rate, short, p), rate, short, p)


@functools.lru_cache(maxsize=None)
def oracle_frames(rate, short):
    """three frames of orc.encode_frame -> (BBFRAMEs uint8 [3, kbch / 8], code bits uint8 [3, N]), computed once and read-only"""
    bbs, bits = zip(*[orc.encode_frame(rate, short, 500 + 10 * (2 * rate + short) + k) for k in range(3)])
    bbs, bits = np.stack(bbs), np.stack(bits)
    bbs.setflags(write=False)
    bits.setflags(write=False)
    return bbs, bits


def single_bits(nbytes, positions):
    m = np.zeros((len(positions), nbytes), np.uint8)
    for k, x in enumerate(positions):
        m[k, x // 8] = 1 << (7 - x % 8)
    return m


# ---- 1. against the oracle's whole transmitter
@pytest.mark.parametrize('rate,short', orc.ALL_CODES, ids=CODE_IDS)
def test_fec_encode_equals_oracle(engine, rate, short):
    bbs, bits = oracle_frames(rate, short)
    code, llr = engine.fec_encode(dev(bbs), rate, bool(short), amplitude=AMPLITUDE)
    assert np.array_equal(code.cpu().numpy(), np.packbits(bits, axis=1))
    assert np.array_equal(llr.cpu().numpy(), np.where(bits != 0, -AMPLITUDE, AMPLITUDE).astype(np.int8))
    code2, none = engine.fec_encode(dev(bbs), rate, bool(short))
    assert none is None and torch.equal(code, code2)


# ---- 2. stage by stage on constructed messages
@pytest.mark.parametrize('rate,short', orc.ALL_CODES, ids=CODE_IDS)
def test_stages_on_constructed_messages(engine, pkg, rate, short):
    p = orc.fec_params(rate, short)
    K, kbch, N = p['K'], p['kbch'], p['N']
    kb = kbch // 8
    plan = pkg.fec_encode_plan(rate, bool(short))
    seams = plan['seams']               # where the BCH kernel's chunks begin: taken from the plan, not from a constant here
    assert seams and all(0 < s < kbch for s in seams)
    rng = np.random.default_rng(900 + 2 * rate + short)
    msgs = np.concatenate([np.zeros((1, kb), np.uint8), np.full((1, kb), 0xff, np.uint8),
                           single_bits(kb, [0, kbch - 1] + [s - 1 for s in seams] + list(seams)),
                           rng.integers(0, 256, (2, kb), dtype=np.uint8)])
    # BB scrambler
    got = engine.bb_scramble(dev(msgs[:4]), rate, bool(short)).cpu().numpy()
    assert np.array_equal(got, np.stack([oracle_scramble(m, p) for m in msgs[:4]]))
    # BCH: the parity of bit kbch - 1 alone is g - x^P
    want = np.stack([oracle_bch(m, rate, short, p) for m in msgs])
    frames = np.full((len(msgs), K // 8), 0x5a, np.uint8)       # (whatever lies in the parity area is overwritten)
    frames[:, :kb] = msgs
    got = engine.bch_encode(dev(frames), rate, bool(short)).cpu().numpy()
    bad = np.nonzero((got != want).any(axis=1))[0]
    assert bad.size == 0, ('BCH messages that differ', bad.tolist())
    g = sum(int(c) << k for k, c in enumerate(plan['generator']))
    assert int.from_bytes(want[3, kb:].tobytes(), 'big') == g ^ (1 << (K - kbch))
    # LDPC: single information bits in the first and the last block column at the word and rotation seams, and the BCH code words above
    last = K - 360
    info = np.concatenate([np.zeros((1, K // 8), np.uint8), np.full((1, K // 8), 0xff, np.uint8),
                           single_bits(K // 8, [o for o in (0, 31, 32, 359)] + [last + o for o in (0, 31, 32, 359)]), want[-2:]])
    want_code = np.stack([oracle_ldpc(m, rate, short, p) for m in info])
    got = engine.ldpc_encode(dev(info), rate, bool(short)).cpu().numpy()
    assert got.shape == (len(info), N // 8)
    bad = np.nonzero((got != want_code).any(axis=1))[0]
    assert bad.size == 0, ('LDPC messages that differ', bad.tolist())


# ---- 3. frame counts around the kernels' frames-per-workgroup unit, rows beyond the count untouched
def test_frame_counts_and_sentinel_rows(engine, pkg):
    rate, short = 3, 1
    p = orc.fec_params(rate, short)
    plan = pkg.fec_encode_plan(rate, True)
    unit = plan['bch_frames_per_workgroup']
    counts = sorted({1, unit - 1, unit + 1, plan['ldpc_frames_per_workgroup'] + 1, 0} - {-1})
    rng = np.random.default_rng(31)
    bbs = rng.integers(0, 256, (max(counts), p['kbch'] // 8), dtype=np.uint8)
    assert len({bytes(b) for b in bbs}) == len(bbs)
    want = np.stack([oracle_encode(b, rate, short) for b in bbs])
    for n in counts:
        out = torch.full((n + 2, p['N'] // 8), 0xa5, dtype=torch.uint8, device='cuda')
        llr = torch.full((n + 2, p['N']), 77, dtype=torch.int8, device='cuda')
        d_bb = dev(bbs[:n]) if n else torch.empty((0, p['kbch'] // 8), dtype=torch.uint8, device='cuda')
        before = engine.get_state('kernel_launches')
        engine.fec_encode(d_bb, rate, True, amplitude=5, out=out, llr=llr)
        if n == 0:
            assert engine.get_state('kernel_launches') == before
        o, l = out.cpu().numpy(), llr.cpu().numpy()
        assert np.array_equal(o[:n], want[:n]), n
        assert np.array_equal(l[:n], np.where(np.unpackbits(want[:n], axis=1) != 0, -5, 5).astype(np.int8)), n
        assert (o[n:] == 0xa5).all() and (l[n:] == 77).all(), n
        # the stages on their own
        if n:
            sc = engine.bb_scramble(d_bb, rate, True)
            assert np.array_equal(sc.cpu().numpy(), np.stack([oracle_scramble(b, p) for b in bbs[:n]]))
            big = torch.full((n + 2, p['K'] // 8), 0xa5, dtype=torch.uint8, device='cuda')
            big[:n] = sc
            engine.bch_encode(big[:n], rate, True)
            assert (big[n:] == 0xa5).all() and torch.equal(big[:n], dev(want[:n, :p['K'] // 8]))
            out2 = torch.full((n + 2, p['N'] // 8), 0xa5, dtype=torch.uint8, device='cuda')
            engine.ldpc_encode(big[:n].contiguous(), rate, True, out=out2)
            assert (out2[n:] == 0xa5).all() and torch.equal(out2[:n], dev(want[:n]))


def test_more_frames_than_one_launch_has_workgroups(engine, pkg):
    """every kernel's workgroups take further frames in turn: more frames than max_workgroups x frames per workgroup, of the smallest code"""
    rate, short = 0, 1
    p = orc.fec_params(rate, short)
    plan = pkg.fec_encode_plan(rate, True)
    n = plan['max_workgroups'] * plan['bch_frames_per_workgroup'] + 3
    rng = np.random.default_rng(32)
    bbs = rng.integers(0, 256, (5, p['kbch'] // 8), dtype=np.uint8)
    want = dev(np.stack([oracle_encode(b, rate, short) for b in bbs]))
    idx = torch.arange(n, device='cuda') % 5
    code, llr = engine.fec_encode(dev(bbs)[idx].contiguous(), rate, True, amplitude=1)
    assert torch.equal(code, want[idx])
    # (bit x of a row: bit 7 - x % 8 of byte x // 8)
    sh = (7 - torch.arange(8, device='cuda')).to(torch.int32)
    bits = ((code[n - 1].to(torch.int32).unsqueeze(1) >> sh) & 1).reshape(-1)
    assert torch.equal(llr[n - 1], torch.where(bits != 0, -1, 1).to(torch.int8)) and int((llr.abs() != 1).sum()) == 0


# ---- 4. round trip through the pinned decoder: zero sweeps = a zero syndrome in the reference's own check
@pytest.mark.parametrize('rate,short', orc.ALL_CODES, ids=CODE_IDS)
def test_round_trip_through_the_decoder(engine, rate, short):
    bbs, _ = oracle_frames(rate, short)
    d_bb = dev(bbs)
    _, llr = engine.fec_encode(d_bb, rate, bool(short), amplitude=AMPLITUDE)
    out, trials, corr = engine.fec_decode(llr, rate, bool(short), max_trials=25)
    assert torch.equal(out, d_bb)
    assert trials.cpu().tolist() == [0, 0, 0] and corr.cpu().tolist() == [0, 0, 0]


# ---- 5. the error count on constructed input
@pytest.mark.parametrize('rate,short', [(6, 0), (9, 1)], ids=['3_4-normal', '8_9-short'])
def test_channel_ber_on_constructed_llrs(engine, rate, short):
    p = orc.fec_params(rate, short)
    N, K = p['N'], p['K']
    bbs, _ = oracle_frames(rate, short)
    d_bb = dev(bbs)
    _, llr = engine.fec_encode(d_bb, rate, bool(short), amplitude=AMPLITUDE)
    flips = sorted({0, 7, 8, K - 1, K, N - 1} | {int(x) for x in np.linspace(100, N - 100, 11)})
    zeros = sorted({1, K + 1, N - 2} | set(range(0, N, 97)))
    assert len(flips) == 17 and 0 in set(flips) & set(zeros) and 5000 not in set(flips) | set(zeros)        # (a flipped position that is also erased does not count)
    l = llr.cpu().numpy().copy()
    l[:, flips] = -l[:, flips]
    l[2, 5000] = -l[2, 5000]            # (and one more in the last frame: the frames' counts differ)
    l[:, zeros] = 0
    want_err, want_cnt = len(set(flips) - set(zeros)), N - len(zeros)
    err, cnt = engine.channel_ber(dev(l), d_bb, rate, bool(short))
    assert err.cpu().tolist() == [want_err, want_err, want_err + 1] and cnt.cpu().tolist() == [want_cnt] * 3
    err, cnt = engine.channel_ber(dev(l), d_bb, rate, bool(short), corrections=dev(np.array([0, -1, 3], np.int32)))
    assert err.cpu().tolist() == [want_err, -1, want_err + 1] and cnt.cpu().tolist() == [want_cnt, 0, want_cnt]
    # the encoder's own LLRs: nothing wrong, everything counted; and LLRs at an odd address
    err, cnt = engine.channel_ber(llr, d_bb, rate, bool(short))
    assert err.cpu().tolist() == [0, 0, 0] and cnt.cpu().tolist() == [N] * 3
    odd = torch.zeros(3 * N + 1, dtype=torch.int8, device='cuda')
    odd[1:] = dev(l).reshape(-1)
    err, cnt = engine.channel_ber(odd[1:].view(3, N), d_bb, rate, bool(short))
    assert err.cpu().tolist() == [want_err, want_err, want_err + 1] and cnt.cpu().tolist() == [want_cnt] * 3


def test_channel_ber_over_more_frames_than_one_pass(engine, pkg):
    rate, short = 0, 1
    p = orc.fec_params(rate, short)
    N = p['N']
    n = pkg.fec_encode_plan(rate, True)['ber_chunk_frames'] + 3
    rng = np.random.default_rng(33)
    bbs = dev(rng.integers(0, 256, (5, p['kbch'] // 8), dtype=np.uint8))
    f = torch.arange(n, device='cuda')
    d_bb = bbs[f % 5].contiguous()
    _, llr = engine.fec_encode(d_bb, rate, True, amplitude=3)
    # frame f: the first f % 7 positions from f % 11 on flipped, position 16000 erased
    pos = torch.arange(N, device='cuda').unsqueeze(0)
    a = (f % 11).unsqueeze(1)
    flip = (pos >= a) & (pos < a + (f % 7).unsqueeze(1))
    llr = torch.where(flip, -llr, llr)
    llr[:, 16000] = 0
    corr = torch.where(f % 13 == 12, -1, 0).to(torch.int32)
    err, cnt = engine.channel_ber(llr.contiguous(), d_bb, rate, True, corrections=corr)
    assert torch.equal(err, torch.where(corr < 0, -1, f % 7).to(torch.int32))
    assert torch.equal(cnt, torch.where(corr < 0, 0, N - 1).to(torch.int32))


# ---- 6. behind the receiver: tap 3, the delivered BBFRAMEs and bch_corrections of a synchronous call
def test_channel_ber_behind_the_receiver(engine):
    """the smallest CCM case of test_gpu_s2chain.py (QPSK 1/2 short frames, Es/N0 12 dB, seed 4).  The oracle receiver on the CPU delivers 7 frames of it, all of
    which pass BCH (corrections 0), with (errors, counted) = (136, 16194), (1, 16200), (0, 16199), (2, 16200), (1, 16200), (1, 16200), (0, 16200)."""
    modcod, short, rate, N = 4, 1, 3, 16200
    iq, bb, _ = orc.transmit(modcod, short, 0, nframes=8, seed=4, esn0_db=12.0, cfo=1e-3, timing=0.3, phase0=0.1, lead_symbols=700)
    dm = engine.demod(engine.default_cfg(modcod, True, False, max_ldpc_trials=16), max_samples=iq.size)
    got_err, got_cnt, want_err, want_cnt, corrs = [], [], [], [], []
    for a in range(0, iq.size, iq.size):        # (one call, as the oracle run quoted above)
        frames = dm.process(iq[a:a + iq.size])
        if not len(frames):
            continue
        llr = dm.tap(3).reshape(-1, N)
        corr = np.array([s.bch_corrections for s in dm.stats()], np.int32)
        assert llr.shape[0] == len(frames) == len(corr)
        e, c = engine.channel_ber(dev(llr), dev(frames), rate, True, corrections=dev(corr))
        got_err += e.cpu().tolist()
        got_cnt += c.cpu().tolist()
        corrs += corr.tolist()
        for f in range(len(frames)):
            if corr[f] < 0:
                want_err.append(-1)
                want_cnt.append(0)
                continue
            bits = np.unpackbits(oracle_encode(frames[f], rate, short))
            want_err.append(int(((llr[f] != 0) & ((llr[f] < 0) != (bits != 0))).sum()))
            want_cnt.append(int((llr[f] != 0).sum()))
    dm.close()
    assert len(got_err) >= 5 and all(c >= 0 for c in corrs), corrs
    assert got_err == want_err and got_cnt == want_cnt
    assert max(got_err) > 0 and got_err == [136, 1, 0, 2, 1, 1, 0] and got_cnt == [16194, 16200, 16199, 16200, 16200, 16200, 16200]


# ---- 7. argument errors: DVBS2GPU_ERR_ARG and a text, nothing launched
def test_argument_errors(engine, pkg):
    lib, h = engine.lib, engine.h
    p = orc.fec_params(6, 1)
    bb = torch.zeros((2, p['kbch'] // 8), dtype=torch.uint8, device='cuda')
    fr = torch.zeros((2, p['K'] // 8), dtype=torch.uint8, device='cuda')
    code = torch.zeros((2, p['N'] // 8), dtype=torch.uint8, device='cuda')
    llr = torch.zeros((2, p['N']), dtype=torch.int8, device='cuda')
    cnt = torch.zeros(4, dtype=torch.int32, device='cuda')
    P = lambda t: C.c_void_p(t.data_ptr())
    e, c = P(cnt), C.c_void_p(cnt.data_ptr() + 8)
    cases = []
    for rate, short in ((-1, 0), (11, 0), (10, 1)):
        cases += [lambda r=rate, s=short: lib.dvbs2gpu_bb_scramble_batch(h, r, s, P(bb), 2, P(fr), None),
                  lambda r=rate, s=short: lib.dvbs2gpu_bch_encode_batch(h, r, s, P(fr), 2, None),
                  lambda r=rate, s=short: lib.dvbs2gpu_ldpc_encode_batch(h, r, s, P(fr), 2, P(code), None),
                  lambda r=rate, s=short: lib.dvbs2gpu_fec_encode_batch(h, r, s, P(bb), 2, P(code), None, 0, None),
                  lambda r=rate, s=short: lib.dvbs2gpu_fec_channel_ber_batch(h, r, s, P(llr), P(bb), None, 2, e, c, None)]
    cases += [
        # NULL pointers
        lambda: lib.dvbs2gpu_bb_scramble_batch(h, 6, 1, None, 2, P(fr), None), lambda: lib.dvbs2gpu_bb_scramble_batch(h, 6, 1, P(bb), 2, None, None),
        lambda: lib.dvbs2gpu_bch_encode_batch(h, 6, 1, None, 2, None),
        lambda: lib.dvbs2gpu_ldpc_encode_batch(h, 6, 1, None, 2, P(code), None), lambda: lib.dvbs2gpu_ldpc_encode_batch(h, 6, 1, P(fr), 2, None, None),
        lambda: lib.dvbs2gpu_fec_encode_batch(h, 6, 1, None, 2, P(code), None, 0, None), lambda: lib.dvbs2gpu_fec_encode_batch(h, 6, 1, P(bb), 2, None, None, 0, None),
        lambda: lib.dvbs2gpu_fec_channel_ber_batch(h, 6, 1, None, P(bb), None, 2, e, c, None), lambda: lib.dvbs2gpu_fec_channel_ber_batch(h, 6, 1, P(llr), None, None, 2, e, c, None),
        lambda: lib.dvbs2gpu_fec_channel_ber_batch(h, 6, 1, P(llr), P(bb), None, 2, None, c, None), lambda: lib.dvbs2gpu_fec_channel_ber_batch(h, 6, 1, P(llr), P(bb), None, 2, e, None, None),
        lambda: lib.dvbs2gpu_fec_encode_batch(None, 6, 1, P(bb), 2, P(code), None, 0, None),
        # negative counts
        lambda: lib.dvbs2gpu_bb_scramble_batch(h, 6, 1, P(bb), -1, P(fr), None), lambda: lib.dvbs2gpu_bch_encode_batch(h, 6, 1, P(fr), -1, None),
        lambda: lib.dvbs2gpu_ldpc_encode_batch(h, 6, 1, P(fr), -1, P(code), None), lambda: lib.dvbs2gpu_fec_encode_batch(h, 6, 1, P(bb), -1, P(code), None, 0, None),
        lambda: lib.dvbs2gpu_fec_channel_ber_batch(h, 6, 1, P(llr), P(bb), None, -1, e, c, None),
        # amplitudes
        lambda: lib.dvbs2gpu_fec_encode_batch(h, 6, 1, P(bb), 2, P(code), P(llr), 0, None), lambda: lib.dvbs2gpu_fec_encode_batch(h, 6, 1, P(bb), 2, P(code), P(llr), 128, None),
        lambda: lib.dvbs2gpu_fec_encode_batch(h, 6, 1, P(bb), 2, P(code), P(llr), -20, None),
    ]
    torch.cuda.synchronize()
    before = engine.get_state('kernel_launches')
    for k, call in enumerate(cases):
        lib.dvbs2gpu_bb_scramble_batch(h, 6, 1, P(bb), 0, P(fr), None)           # (a good call in between: the text below is this case's own)
        assert call() == -1, k
        text = lib.dvbs2gpu_last_error().decode()
        assert text and '_batch: ' in text, (k, text)
    # nframes == 0 succeeds, without a launch
    assert lib.dvbs2gpu_bb_scramble_batch(h, 6, 1, P(bb), 0, P(fr), None) == 0 and lib.dvbs2gpu_bch_encode_batch(h, 6, 1, P(fr), 0, None) == 0
    assert lib.dvbs2gpu_ldpc_encode_batch(h, 6, 1, P(fr), 0, P(code), None) == 0 and lib.dvbs2gpu_fec_encode_batch(h, 6, 1, P(bb), 0, P(code), P(llr), 20, None) == 0
    assert lib.dvbs2gpu_fec_channel_ber_batch(h, 6, 1, P(llr), P(bb), None, 0, e, c, None) == 0
    assert engine.get_state('kernel_launches') == before
    torch.cuda.synchronize()
    assert int(code.sum()) == 0 and int(fr.sum()) == 0 and int(cnt.sum()) == 0
