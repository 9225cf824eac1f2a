"""The DVB-S2 modulator on the GPU (csrc/s2_tx.hip): PL framing, pulse shaping, channel, and the whole of it as Engine.modulate, against the same rules on the CPU
(dvbs2gpu_s2_tx_host / dvbs2gpu_pulse_shape_host; tests/test_s2_tx_cpu.py ties those to the oracle transmitter).  Exact equality, bit for bit, unless a case says
otherwise."""
import ctypes as C

import numpy as np
import pytest
import torch

import orc
import s2_tx_cases as tc

pytestmark = pytest.mark.gpu


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(t):
    return t.cpu().numpy()


def random_code(pkg, pls, nstreams, seed):
    return np.random.default_rng(seed).integers(0, 256, (nstreams, pkg.s2_tx_sizes(pls)['code_bytes']), dtype=np.uint8)


# ---- 1. PL framing: every PLS code
def test_pl_frame_all_128_pls_codes(engine, pkg):
    """the 108 codes that name a frame, in four calls (random code words: the framing does not care whether a word is one of the code); the other 20 are refused"""
    assert len(tc.VALID_PLS) == 108 and len(tc.INVALID_PLS) == 20
    for part in range(4):
        pls = tc.VALID_PLS[part::4]
        code = random_code(pkg, pls, 1, 10 + part)
        got = engine.pl_frame(dev(code), pls)
        want, _ = pkg.s2_tx_host(pls, code[0], want_iq=False)
        assert tc.same_bits(host(got)[0], want), pls
    ok = [tc.pls_code(13, 1, 1)]
    code = dev(random_code(pkg, ok, 1, 3))
    out = torch.full((1, pkg.s2_tx_sizes(ok)['symbols'] + 40000), 7.0 + 9.0j, dtype=torch.complex64, device='cuda')
    torch.cuda.synchronize()
    before = engine.get_state('kernel_launches')
    for bad in tc.INVALID_PLS + [-1, 128]:
        pls = np.array(ok + [bad], np.int32)
        rc = engine.lib.dvbs2gpu_pl_frame_batch(engine.h, pls.ctypes.data, 2, C.c_void_p(code.data_ptr()), None, None, 1, C.c_void_p(out.data_ptr()), None)
        assert rc == -1 and b'pl_frame_batch: frame 1 has no valid PLS code' in engine.lib.dvbs2gpu_last_error(), bad
    assert engine.get_state('kernel_launches') == before
    torch.cuda.synchronize()
    assert bool((out == 7.0 + 9.0j).all())


# ---- 2. seams: frame and stream offsets, mixed frame kinds, both code-word layouts
SEAM_LISTS = {'ccm_3_frames': [tc.pls_code(18, 1, 1)] * 3,
              'vcm_normal_short_dummy': [tc.pls_code(25, 0, 1), tc.pls_code(4, 1, 0), tc.pls_code(0), tc.pls_code(12, 0, 0), tc.pls_code(22, 1, 1), tc.pls_code(0, 0, 1)]}


@pytest.mark.parametrize('name', list(SEAM_LISTS))
def test_pl_frame_streams_frames_and_layouts(engine, pkg, name):
    pls, S = SEAM_LISTS[name], 2
    code = random_code(pkg, pls, S, 21)
    sizes = [pkg.s2_tx_sizes([p])['code_bytes'] for p in pls]
    want = np.stack([pkg.s2_tx_host(pls, code[s], want_iq=False)[0] for s in range(S)])
    # stream-major: [stream][a stream's code words]
    got = engine.pl_frame(dev(code), pls)
    assert tc.same_bits(host(got), want)
    # frame-major: [frame][stream][N / 8], behind 3 bytes of something else (short code words are 2025 bytes: every alignment occurs anyway)
    parts, off, stride, pos, at = [np.full(3, 0xA5, np.uint8)], [], [], 3, 0
    for n in sizes:
        off.append(pos)
        stride.append(n)
        for s in range(S):
            parts.append(code[s, at:at + n])
        pos += S * n
        at += n
    fm = np.concatenate(parts)
    got = engine.pl_frame(dev(fm), pls, nstreams=S, code_off=off, code_stride=stride)
    assert tc.same_bits(host(got), want)
    # stride 0: every stream reads the same code word
    got = engine.pl_frame(dev(code[1]), pls, nstreams=3, code_off=np.concatenate([[0], np.cumsum(sizes)[:-1]]), code_stride=[0] * len(pls))
    assert all(tc.same_bits(host(got)[s], want[1]) for s in range(3))


# ---- 3. shaping
@pytest.fixture(scope='module')
def blocks():
    rng = np.random.default_rng(5)
    one = (rng.standard_normal((2, 3331)) + 1j * rng.standard_normal((2, 3331))).astype(np.complex64)
    return {3330: np.ascontiguousarray(one[:, 1:]), 3331: one, 20: np.ascontiguousarray(one[:, :20])}      # 3331: 3330 with one symbol in front


@pytest.mark.parametrize('rolloff', [0.35, 0.25, 0.20])
@pytest.mark.parametrize('n', [3330, 3331, 20])
def test_pulse_shape_block_lengths_ends_timing_rolloffs(engine, pkg, blocks, n, rolloff):
    """3330 and 3331 symbols: no multiple of the 256-symbol tile, 14 tiles, the last one of 2 or 3 symbols; 20: shorter than the pulse's span, circular wraps more
    than once; two streams; nothing written behind 2 * symbols samples"""
    sym = blocks[n]
    d_sym = dev(sym)
    for circular in (False, True):
        for timing in (0.0, 0.3):
            buf = torch.full((2 * 2 * n + 512,), 3.0 - 4.0j, dtype=torch.complex64, device='cuda')
            out = buf[:2 * 2 * n].view(2, 2 * n)
            engine.pulse_shape(d_sym, rolloff, timing, circular, out=out)
            want = np.stack([pkg.pulse_shape_host(sym[s], rolloff, timing, circular) for s in range(2)])
            assert tc.same_bits(host(out), want), (circular, timing)
            assert bool((buf[2 * 2 * n:] == 3.0 - 4.0j).all())
    if n == 3330:       # the same block through the framing rules' own host path: a dummy PLFRAME
        d = engine.pl_frame(torch.zeros((1, 0), dtype=torch.uint8, device='cuda'), [0])
        assert tc.same_bits(host(engine.pulse_shape(d, rolloff, 0.3))[0], pkg.s2_tx_host([0], np.zeros(0, np.uint8), rolloff=rolloff, timing=0.3)[1])


# ---- 4. channel
def test_channel_is_a_function_of_seed_stream_and_index(engine, pkg, blocks):
    iq0 = np.concatenate([blocks[3331][0], blocks[3331][1]])        # 6662 samples: more than one pass of a small grid would not matter either
    three = dev(np.stack([iq0, iq0, iq0]))
    one = dev(iq0[None, :])
    kw = dict(esn0_db=6.0, cfo=2e-3, phase0=0.4, seed=11)
    engine.channel(three, **kw)
    engine.channel(one, **kw)
    a, b = host(three), host(one)
    assert tc.same_bits(a[0], b[0])                                  # two launches of different stream counts: the same samples for (seed, stream 0)
    assert not np.array_equal(a[1], a[0]) and not np.array_equal(a[2], a[1])        # the stream index enters the generator
    for s in range(3):
        assert tc.same_bits(a[s], pkg.channel_host(iq0, stream=s, **kw))
    # per-stream parameters
    mixed = dev(np.stack([iq0, iq0]))
    engine.channel(mixed, esn0_db=[200.0, 6.0], cfo=[0.0, 2e-3], phase0=[0.0, 0.4], seed=[1, 11])
    m = host(mixed)
    assert tc.same_bits(m[0], iq0) and tc.same_bits(m[1], a[1])     # esn0 200, cfo 0, phase0 0: the identity, bit for bit
    # a long block: indices beyond one pass of the grid (1024 workgroups of 256)
    n = 1024 * 256 + 999
    big = np.zeros((1, n), np.complex64)
    big[0, ::7] = 1.0
    d = dev(big)
    engine.channel(d, esn0_db=10.0, cfo=1e-3, phase0=0.0, seed=2)
    assert tc.same_bits(host(d)[0], pkg.channel_host(big[0], esn0_db=10.0, cfo=1e-3, phase0=0.0, seed=2))


# ---- 5. modulate against the separate stages
MOD_LISTS = {'ccm': [tc.pls_code(14, 1, 0)] * 3,
             'vcm': [tc.pls_code(14, 1, 0), tc.pls_code(14, 1, 1), tc.pls_code(0), tc.pls_code(14, 1, 0), tc.pls_code(19, 0, 1), tc.pls_code(4, 1, 0)]}


@pytest.mark.parametrize('name', list(MOD_LISTS))
def test_modulate_equals_the_stages_one_by_one(engine, pkg, name):
    pls, S, seed = MOD_LISTS[name], 2, 6
    code0, bbs = tc.code_words(pls, seed)                           # stream 0: the oracle's frames; stream 1: random BBFRAMEs
    rng = np.random.default_rng(8)
    per_frame = [np.stack([bb, rng.integers(0, 256, bb.size, dtype=np.uint8)]) for bb in bbs if bb is not None]      # [stream][kbch / 8] per coded frame
    flat = dev(np.concatenate([p.reshape(-1) for p in per_frame]))
    kw = dict(esn0_db=9.0, cfo=1e-3, phase0=0.2, seed=4)
    torch.cuda.synchronize()
    before = engine.get_state('kernel_launches')
    got = engine.modulate(flat, pls, S, rolloff=0.25, timing=0.3, circular=True, **kw)
    launches = engine.get_state('kernel_launches') - before
    # the runs of one code: ccm 1; vcm: 8PSK 3/4 short (frames 0, 1, 3: the dummy frame between them takes no bytes), 16APSK 3/4 normal, QPSK 1/2 short
    runs = 1 if name == 'ccm' else 3
    assert launches == 3 * runs + 1 + 1 + 1, launches               # scramble + BCH + LDPC per run, framing (<= 16 frames), shaping, channel
    # one by one
    codes, k = [], 0
    for p in pls:
        if p >> 2 == 0:
            continue
        cw, _ = engine.fec_encode(dev(per_frame[k]), tc.RATE_OF_MODCOD[p >> 2], bool(p & 2))
        codes.append(cw)                                            # [stream][N / 8]
        k += 1
    stream_major = torch.cat(codes, dim=1).contiguous()
    assert np.array_equal(host(stream_major)[0], code0)             # the encoder's code words are the oracle's
    sym = engine.pl_frame(stream_major, pls)
    iq = engine.pulse_shape(sym, 0.25, 0.3, True)
    clean = iq.clone()
    engine.channel(iq, **kw)
    assert tc.same_bits(host(got), host(iq))
    assert tc.same_bits(host(engine.modulate(flat, pls, S, rolloff=0.25, timing=0.3, circular=True)), host(clean))      # no channel pointer: no channel
    # stream 0 against the CPU
    want = pkg.s2_tx_host(pls, code0, rolloff=0.25, timing=0.3, circular=True, stream=0, **kw)[1]
    assert tc.same_bits(host(got)[0], want)


# ---- 6. loopback: modulator -> channel -> receiver -> channel BER, no sample on the host
def test_loopback_through_the_receiver(engine, pkg):
    """8PSK 3/4 short frames, 12 frames, cfo 1e-3 rad/sample, timing 0.3; seed 1 (orc.transmit's default).
    Es/N0: at the issue's 14 dB the oracle transmitter into the oracle receiver does not deliver 8 of its 12 frames -- the receiver outputs 11 blocks, but with
    seed 1 none of them equals a transmitted frame (over seeds 1..6: 0, 9, 4, 3, 0, 7; the test looks at its own seed below) -- so it is raised, to 17 dB.
    What goes wrong at either level is the receiver's acquisition, not the decoding: it starts cold, there are no pilots and no lead-in, the first block it
    outputs is never a frame and the carrier loop needs 1 to 5 frames more (17 dB, seeds 1..6: 7, 10, 10, 7, 10, 9 of 12 right from orc.transmit, 7, 5, 7, 10, 7,
    6 from this modulator's signal); every block it fails on carries a negative BCH result, for which channel_ber answers -1.  So that the count and the
    'no -1' of the issue measure the signal and not the acquisition, the 12-frame block goes through the receiver twice: it is shaped circularly (seamless when
    repeated), the second pass starts at the carrier phase the first one ended with and has noise of its own (stream 1 of the same modulate call), the first pass
    warms the receiver up and the second is the one that is counted.  On the CPU (oracle transmitter, oracle receiver) the second pass delivers 12 frames, all 12
    right, for seeds 1..6 at 17 dB (at 14 dB: 12, 8, 7, 12, 12, 12)."""
    modcod, short, pilots, nf, seed, esn0, cfo, timing = 14, 1, 0, 12, 1, 17.0, 1e-3, 0.3
    rate, N = tc.RATE_OF_MODCOD[modcod], 16200
    nsamples = 2 * nf * orc.modcod_params(modcod, short, pilots)['plframe']
    phase1 = float(np.fmod(cfo * nsamples, 2.0 * np.pi))            # where the first pass leaves the carrier
    cfg = orc.default_cfg(modcod, short, pilots, max_ldpc_trials=16)
    # the oracle's own loop, computed here: cold at 14 dB (why the Es/N0 is raised), then the two passes at 17 dB
    cold_iq, obb, _ = orc.transmit(modcod, short, pilots, nframes=nf, seed=seed, esn0_db=14.0, cfo=cfo, timing=timing)
    sent = {bytes(b) for b in obb}
    assert sum(bytes(f) in sent for f in orc.OracleRx(cfg).process(cold_iq)) < 8
    rx = orc.OracleRx(cfg)
    rx.process(orc.transmit(modcod, short, pilots, nframes=nf, seed=seed, esn0_db=esn0, cfo=cfo, timing=timing, circular=1)[0])
    oracle_out = rx.process(orc.transmit(modcod, short, pilots, nframes=nf, seed=seed, esn0_db=esn0, cfo=cfo, timing=timing, circular=1, phase0=phase1)[0])
    oracle_good = sum(bytes(f) in sent for f in oracle_out)
    assert oracle_good >= 8
    # the device's loop: the same BBFRAMEs on two streams, frame-major
    pls = [tc.pls_code(modcod, short, pilots)] * nf
    bb2 = np.repeat(obb[:, None, :], 2, axis=1)
    iq = engine.modulate(dev(bb2), pls, 2, timing=timing, circular=True, esn0_db=esn0, cfo=cfo, phase0=[0.0, phase1], seed=seed)
    assert iq.shape == (2, nsamples)
    dm = engine.demod(engine.default_cfg(modcod, True, False, max_ldpc_trials=16), max_samples=nsamples)
    out = torch.zeros((nf + 4) * obb.shape[1], dtype=torch.uint8, device='cuda')
    want_rx = orc.OracleRx(cfg)
    for p in range(2):
        nbytes = engine.process_batch([dm], [iq[p]], [out])[0]
        frames = host(out)[:nbytes].reshape(-1, obb.shape[1]).copy()
        assert np.array_equal(frames, want_rx.process(host(iq)[p]))          # what the oracle receiver delivers from the same IQ
    good = [bytes(f) in sent for f in frames]
    print('second pass: delivered %d, equal to a transmitted frame %d (oracle loop: %d of %d)' % (len(frames), sum(good), oracle_good, len(oracle_out)))
    assert sum(good) >= oracle_good
    corr = np.array([s.bch_corrections for s in dm.stats()], np.int32)
    llr = dm.tap(3).reshape(-1, N)
    assert len(corr) == len(frames) == llr.shape[0]
    err, cnt = engine.channel_ber(dev(llr), dev(frames), rate, True, corrections=dev(corr))
    err, cnt = host(err), host(cnt)
    dm.close()
    print('channel errors', err.tolist(), 'of', cnt.tolist())
    assert (err >= 0).all() and (cnt > 16000).all() and (err < cnt // 20).all()         # no -1 on any delivered frame
    # without noise the modulator's IQ is the oracle transmitter's within the bound of tests/test_s2_tx_cpu.py (rotation: 2.5 * 2^-24 per factor more)
    clean = host(engine.modulate(dev(obb), pls, 1, timing=timing))[0]
    ref = orc.transmit(modcod, short, pilots, nframes=nf, seed=seed, timing=timing)[0]
    assert np.abs(clean - ref).max() < 2e-5


# ---- 7. argument errors: DVBS2GPU_ERR_ARG and a text, nothing launched, nothing written
def test_argument_errors(engine, pkg):
    lib, h = engine.lib, engine.h
    pls = np.array([tc.pls_code(14, 1, 0)] * 2, np.int32)
    sz = pkg.s2_tx_sizes(pls)
    code = torch.zeros((1, sz['code_bytes']), dtype=torch.uint8, device='cuda')
    bb = torch.zeros(sz['bbframe_bytes'], dtype=torch.uint8, device='cuda')
    sym = torch.full((1, sz['symbols']), 5.0 + 0j, dtype=torch.complex64, device='cuda')
    iq = torch.full((1, 2 * sz['symbols']), 5.0 + 0j, dtype=torch.complex64, device='cuda')
    P = lambda t, off=0: C.c_void_p(t.data_ptr() + off)
    ch, keep = pkg._tx_channel(10.0, 0.0, 0.0, 1, 1)
    nullch = pkg.TxChannel(None, ch.cfo, ch.phase0, ch.seed)
    A = C.addressof
    n, ns = sz['symbols'], 2 * sz['symbols']
    cases = [
        # NULL pointers
        lambda: lib.dvbs2gpu_pl_frame_batch(h, None, 2, P(code), None, None, 1, P(sym), None), lambda: lib.dvbs2gpu_pl_frame_batch(h, pls.ctypes.data, 2, None, None, None, 1, P(sym), None),
        lambda: lib.dvbs2gpu_pl_frame_batch(h, pls.ctypes.data, 2, P(code), None, None, 1, None, None), lambda: lib.dvbs2gpu_pl_frame_batch(None, pls.ctypes.data, 2, P(code), None, None, 1, P(sym), None),
        lambda: lib.dvbs2gpu_pl_frame_batch(h, pls.ctypes.data, 2, P(code), pls.ctypes.data, None, 1, P(sym), None),
        lambda: lib.dvbs2gpu_pulse_shape_batch(h, None, 1, n, 0.35, 0.0, 0, P(iq), None), lambda: lib.dvbs2gpu_pulse_shape_batch(h, P(sym), 1, n, 0.35, 0.0, 0, None, None),
        lambda: lib.dvbs2gpu_channel_batch(h, None, 1, ns, ch.esn0_db, ch.cfo, ch.phase0, ch.seed, None), lambda: lib.dvbs2gpu_channel_batch(h, P(iq), 1, ns, None, ch.cfo, ch.phase0, ch.seed, None),
        lambda: lib.dvbs2gpu_channel_batch(h, P(iq), 1, ns, ch.esn0_db, ch.cfo, ch.phase0, None, None),
        lambda: lib.dvbs2gpu_s2_modulate_batch(h, None, 2, P(bb), 1, 0.35, 0.0, 0, None, P(iq), None), lambda: lib.dvbs2gpu_s2_modulate_batch(h, pls.ctypes.data, 2, None, 1, 0.35, 0.0, 0, None, P(iq), None),
        lambda: lib.dvbs2gpu_s2_modulate_batch(h, pls.ctypes.data, 2, P(bb), 1, 0.35, 0.0, 0, None, None, None), lambda: lib.dvbs2gpu_s2_modulate_batch(h, pls.ctypes.data, 2, P(bb), 1, 0.35, 0.0, 0, A(nullch), P(iq), None),
        # negative counts
        lambda: lib.dvbs2gpu_pl_frame_batch(h, pls.ctypes.data, -1, P(code), None, None, 1, P(sym), None), lambda: lib.dvbs2gpu_pl_frame_batch(h, pls.ctypes.data, 2, P(code), None, None, -1, P(sym), None),
        lambda: lib.dvbs2gpu_pulse_shape_batch(h, P(sym), -1, n, 0.35, 0.0, 0, P(iq), None), lambda: lib.dvbs2gpu_pulse_shape_batch(h, P(sym), 1, -1, 0.35, 0.0, 0, P(iq), None),
        lambda: lib.dvbs2gpu_channel_batch(h, P(iq), -1, ns, ch.esn0_db, ch.cfo, ch.phase0, ch.seed, None), lambda: lib.dvbs2gpu_channel_batch(h, P(iq), 1, -1, ch.esn0_db, ch.cfo, ch.phase0, ch.seed, None),
        lambda: lib.dvbs2gpu_s2_modulate_batch(h, pls.ctypes.data, -1, P(bb), 1, 0.35, 0.0, 0, None, P(iq), None), lambda: lib.dvbs2gpu_s2_modulate_batch(h, pls.ctypes.data, 2, P(bb), -1, 0.35, 0.0, 0, None, P(iq), None),
        # roll-offs outside the three, timing
        lambda: lib.dvbs2gpu_pulse_shape_batch(h, P(sym), 1, n, 0.3, 0.0, 0, P(iq), None), lambda: lib.dvbs2gpu_pulse_shape_batch(h, P(sym), 1, n, 0.0, 0.0, 0, P(iq), None),
        lambda: lib.dvbs2gpu_pulse_shape_batch(h, P(sym), 1, n, float(np.float32(0.35)), 0.0, 0, P(iq), None), lambda: lib.dvbs2gpu_pulse_shape_batch(h, P(sym), 1, n, 0.35, 2.5, 0, P(iq), None),
        lambda: lib.dvbs2gpu_s2_modulate_batch(h, pls.ctypes.data, 2, P(bb), 1, 0.5, 0.0, 0, None, P(iq), None), lambda: lib.dvbs2gpu_s2_modulate_batch(h, pls.ctypes.data, 2, P(bb), 1, 0.35, float('nan'), 0, None, P(iq), None),
        # outputs that are not 16-byte aligned; in place
        lambda: lib.dvbs2gpu_pl_frame_batch(h, pls.ctypes.data, 1, P(code), None, None, 1, P(sym, 8), None), lambda: lib.dvbs2gpu_pulse_shape_batch(h, P(sym), 1, n - 1, 0.35, 0.0, 0, P(iq, 8), None),
        lambda: lib.dvbs2gpu_pulse_shape_batch(h, P(iq), 1, n, 0.35, 0.0, 0, P(iq), None),
    ]
    torch.cuda.synchronize()
    before = engine.get_state('kernel_launches')
    for k, call in enumerate(cases):
        lib.dvbs2gpu_channel_batch(h, P(iq), 0, ns, None, None, None, None, None)       # (a good call in between: the text below is this case's own)
        assert call() == -1, k
        text = lib.dvbs2gpu_last_error().decode()
        assert text and '_batch: ' in text, (k, text)
    # a count of 0 succeeds, without a launch
    assert lib.dvbs2gpu_pl_frame_batch(h, None, 0, None, None, None, 1, None, None) == 0 and lib.dvbs2gpu_pl_frame_batch(h, pls.ctypes.data, 2, P(code), None, None, 0, P(sym), None) == 0
    assert lib.dvbs2gpu_pulse_shape_batch(h, P(sym), 0, n, 0.35, 0.0, 0, P(iq), None) == 0 and lib.dvbs2gpu_pulse_shape_batch(h, P(sym), 1, 0, 0.35, 0.0, 0, P(iq), None) == 0
    assert lib.dvbs2gpu_channel_batch(h, P(iq), 1, 0, ch.esn0_db, ch.cfo, ch.phase0, ch.seed, None) == 0
    assert lib.dvbs2gpu_s2_modulate_batch(h, None, 0, None, 1, 0.35, 0.0, 0, None, None, None) == 0 and lib.dvbs2gpu_s2_modulate_batch(h, pls.ctypes.data, 2, P(bb), 0, 0.35, 0.0, 0, None, P(iq), None) == 0
    assert engine.get_state('kernel_launches') == before
    torch.cuda.synchronize()
    assert bool((sym == 5.0).all()) and bool((iq == 5.0).all())
