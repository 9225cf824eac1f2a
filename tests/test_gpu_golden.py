"""The HIP kernels against the committed golden vectors (tests/golden/) DIRECTLY: the stored outputs / SHA-256 digests were produced
by the REFERENCE's own code (oracle/_ref, built from /root/reference by oracle/Makefile; generators tests/golden/make_golden*.py), so
these tests tie the GPU path to the reference without the CPU oracle in between as the checker.  The oracle's transmitter side
(encoder, bit -> LLR mapping, RS encoder) is used only to regenerate the recorded INPUTS from their seeds; every input digest is
checked against the fixture before it is fed to the GPU.

Covers: all 84 LDPC cases over the 21 codes + the stored full vector (bbframe_ldpc.cpp:123-139), the 28 BCH cases + stored vectors
(bbframe_bch.cpp:380-405), the BB PRBS (bbframe_descramble.cpp:122-143), the bit de-interleaver maps (s2_deinterleaver.cpp:72-136),
the DVB-S de-puncturers (depunc.h), soft rotation (rotation.cpp), Forney de-interleaver (dvbs_interleaving.h), TS deframer
(dvbs_ts_deframer.cpp), RS(204,188) wrapper (dvbs_reedsolomon.h over libcorrect), energy-dispersal removal (dvbs_scrambling.h), the
self-locking Viterbi decoder (viterbi_all.cpp) with its K=7 block decoder (viterbi/cc_decoder.cpp), and the BBFRAME -> TS / GSE parser
(dvbs2/bbframe_ts_parser.cpp)."""
import hashlib
import json
import os

import numpy as np
import pytest

import orc

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
G = json.load(open(os.path.join(HERE, 'golden', 'fec_golden.json')))
GD = json.load(open(os.path.join(HERE, 'golden', 'dvbs_golden.json')))
GB = json.load(open(os.path.join(HERE, 'golden', 'bbts_golden.json')))


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def ldpc_input(rate, short, seed, snr_db):
    rng = np.random.default_rng(seed)
    _, bits = orc.encode_frame(rate, short, seed)
    return orc.bits_to_llr(bits, snr_db, rng)


def _codes():
    seen = []
    for c in G['ldpc']:
        if (c['rate'], c['short']) not in seen:
            seen.append((c['rate'], c['short']))
    return seen


@pytest.mark.parametrize('rate,short', _codes(), ids=lambda v: str(v))
def test_ldpc_kernel_reproduces_reference_outputs(engine, rate, short):
    """every LDPC golden case of one code: posteriors (SHA of the int8 soft outputs) and return value of BBFrameLDPC::decode"""
    import torch
    cases = [c for c in G['ldpc'] if (c['rate'], c['short']) == (rate, short)]
    assert len(cases) == 4
    for trials in sorted({c['trials'] for c in cases}):
        sub = [c for c in cases if c['trials'] == trials]
        llr = np.stack([ldpc_input(rate, short, c['seed'], c['snr_db']) for c in sub])
        for k, c in enumerate(sub):
            assert sha(llr[k]) == c['in_sha'], 'input generator drifted; regenerate the goldens'
        hard, tr, post = engine.ldpc_decode(torch.from_numpy(llr).cuda(), rate, bool(short), max_trials=trials, want_post=True)
        torch.cuda.synchronize()
        post, tr, hard = post.cpu().numpy(), tr.cpu().numpy(), hard.cpu().numpy()
        K = orc.fec_params(rate, short)['K']
        for k, c in enumerate(sub):
            assert int(tr[k]) == c['ret'], (c['kind'], trials)
            assert sha(post[k]) == c['out_sha'], (c['kind'], trials)
            assert np.array_equal(hard[k], np.packbits((post[k, :K] < 0).astype(np.uint8)))      # module_dvbs2_demod.cpp:357-360


def test_ldpc_kernel_full_vector(engine):
    import torch
    c = G['ldpc_full']
    llr = np.load(os.path.join(HERE, 'golden', c['infile']))
    want = np.load(os.path.join(HERE, 'golden', c['outfile']))
    _, tr, post = engine.ldpc_decode(torch.from_numpy(llr[None]).cuda(), c['rate'], bool(c['short']), max_trials=c['trials'], want_post=True)
    assert int(tr.cpu()[0]) == c['ret'] and np.array_equal(post.cpu().numpy()[0], want)


def test_bch_kernels_reproduce_reference_outputs(engine):
    """all 28 BCH golden cases (0 .. 2t flipped bits incl. uncorrectable ones, four code families), batched per family"""
    import torch
    fams = []
    for c in G['bch']:
        if (c['rate'], c['short']) not in fams:
            fams.append((c['rate'], c['short']))
    assert len(G['bch']) == 28 and len(fams) == 4
    for rate, short in fams:
        cases = [c for c in G['bch'] if (c['rate'], c['short']) == (rate, short)]
        p = orc.fec_params(rate, short)
        frames = np.zeros((len(cases), p['K'] // 8), np.uint8)
        for k, c in enumerate(cases):
            fr = frames[k]
            orc.lib().orc_make_bbframe(fr, p['kbch'], c['frame_seed'])
            orc.lib().orc_bch_encode(rate, short, fr)
            for x in c['errors']:
                fr[x // 8] ^= 1 << (7 - x % 8)
            assert sha(fr) == c['in_sha']
        d = torch.from_numpy(frames).cuda()
        corr = engine.bch_decode(d, rate, bool(short)).cpu().numpy()
        out = d.cpu().numpy()
        for k, c in enumerate(cases):
            assert int(corr[k]) == c['ret'], (rate, short, len(c['errors']))
            assert sha(out[k]) == c['out_sha'], (rate, short, len(c['errors']))


def test_bch_kernels_full_vectors(engine):
    import torch
    c = G['bch_full']
    fin = np.load(os.path.join(HERE, 'golden', c['infile']))
    fout = np.load(os.path.join(HERE, 'golden', c['outfile']))
    d = torch.from_numpy(fin.copy()).cuda()
    corr = engine.bch_decode(d, c['rate'], bool(c['short'])).cpu().numpy()
    assert [int(x) for x in corr] == c['ret'] and np.array_equal(d.cpu().numpy(), fout)


def test_bb_descrambler_prbs(engine):
    """descrambling zeros yields the PRBS of BBFrameDescrambler (rate 9/10 normal: the longest kbch)"""
    import torch
    p = orc.fec_params(10, 0)
    z = torch.zeros((2, p['K'] // 8), dtype=torch.uint8, device='cuda')
    out = engine.bb_descramble(z, 10, False).cpu().numpy()
    assert out.shape[1] == 58192 // 8
    assert [int(x) for x in out[0, :256]] == G['bb_prbs_first_256'] and sha(out[1]) == G['bb_prbs_sha_7274']


MODCOD_OF = {(0, 3): 4, (1, 6): 14, (1, 4): 12, (2, 6): 19, (2, 7): 20, (3, 6): 24, (3, 9): 27}


@pytest.mark.parametrize('case', G['deinterleave'], ids=lambda c: 'c%d-r%d-s%d' % (c['constel'], c['rate'], c['short']))
def test_bit_deinterleaver_maps(engine, case):
    """the reference's S2Deinterleaver output for an index ramp, through the index function of the fused demapper"""
    import torch
    n = 16200 if case['short'] else 64800
    src = (np.arange(n) * 7 % 251).astype(np.int8)
    modcod = MODCOD_OF[(case['constel'], case['rate'])]
    assert orc.modcod_params(modcod, case['short'], 0)['constel'] == case['constel'] and orc.modcod_params(modcod, case['short'], 0)['rate'] == case['rate']
    out = engine.deinterleave(torch.from_numpy(np.stack([src, src[::-1].copy()])).cuda(), modcod, bool(case['short'])).cpu().numpy()
    assert sha(out[0]) == case['out_sha']


@pytest.mark.parametrize('case', GD['depunc'], ids=lambda c: 'p%d-s%d' % (c['period'], c['shift']))
def test_depuncturers(engine, case):
    """Depunc23 / Depunc56 (rates 2/3 and 5/6) as they run inside the Viterbi kernel: depunc_static and the stateful depunc_cont"""
    period, shift = case['period'], case['shift']
    rng = np.random.default_rng(case['seed'])
    x = rng.integers(0, 256, 2048, dtype=np.uint8)
    out, n, _ = engine.dvbs_depuncture(period, 0, x, [0, shift, 0, 128], fill=7)
    assert n == case['static_n'] and sha(out[:n]) == case['static_sha']
    state = [int(shift > period - 1), shift, 0, 128]           # set_shift(shift)
    for step in case['cont']:
        x = rng.integers(0, 256, step['size'], dtype=np.uint8)
        out, n, state = engine.dvbs_depuncture(period, 1, x, state, fill=9)
        assert n == step['n'] and sha(out[:n + 1]) == step['sha'], step


def test_soft_rotation(engine):
    """rotate_soft for the two phases DVBSDemod uses (module_dvbs_demod.cpp:23), no IQ swap"""
    done = 0
    for c in GD['rotate']:
        if c['iqswap'] or c['phase'] > 1:
            continue
        rng = np.random.default_rng(c['seed'])
        x = rng.integers(-128, 128, 512, dtype=np.int8)
        out, n, _ = engine.dvbs_depuncture(0, 2, x, [c['phase'], 0, 0, 0])
        assert n == 512 and sha(out[:512].view(np.int8)) == c['sha']
        done += 1
    assert done == 2


def test_forney_deinterleaver(engine, pkg):
    import torch
    c = GD['forney']
    rng = np.random.default_rng(c['seed'])
    f = pkg.ForneyBatch(engine, 1)
    outs = []
    for _ in range(c['calls']):
        x = rng.integers(0, 256, 1632, dtype=np.uint8)
        outs.append(f.deinterleave(torch.from_numpy(x[None]).cuda()).cpu().numpy()[0])
    f.close()
    assert outs[0][-16:].tolist() == c['first_call_tail_16'] and sha(np.concatenate(outs)) == c['sha']


def test_ts_deframer(engine, pkg):
    """DVBS_TS_Deframer::work on a bit stream with junk in front, bit errors and an inverted stretch: frames found and their bytes"""
    import torch
    import orc_dvbs_tail as ot
    c = GD['deframer']
    bits, _ = ot.dvbs_outer_tx(48, seed=c['seeds'][0])
    rng = np.random.default_rng(c['seeds'][1])
    stream = np.concatenate([rng.integers(0, 2, 777, dtype=np.uint8), bits, 1 - bits[:1632 * 8 * 2]])
    stream = (stream ^ (rng.random(stream.size) < 0.002)).astype(np.uint8)
    tail = pkg.DvbsTailBank(engine, 1, max_bits=int(stream.size))
    out = torch.zeros(64 * 1504, dtype=torch.uint8, device='cuda')
    tail.process_batch([torch.from_numpy(stream).cuda()], [out])
    frames = tail.tap(0)
    assert tail.stats()['frames'] == c['frames'] and frames.size == 1632 * c['frames'] and sha(frames) == c['sha']
    tail.close()


def test_reed_solomon_wrapper(engine, pkg):
    """DVBSReedSolomon::decode over libcorrect for 40 packets with 0 .. 40 byte errors (beyond 8: the decoder gives up or
    miscorrects, and the wrapper hands out the PREVIOUS message): return values and bytes as the reference produced them"""
    import orc_dvbs_tail as ot
    c = GD['rs']
    rng = np.random.default_rng(c['seed'])
    nes = [0, 1, 3, 8, 9, 12, 0, 8, 20, 40, 2, 9, 9, 0, 7, 8, 8, 10, 11, 0] * 2
    pk = np.zeros((len(nes), 204), np.uint8)
    for k, ne in enumerate(nes):
        msg = rng.integers(0, 256, 188, dtype=np.uint8)
        cw = ot.rs_encode_204(msg)
        pos = rng.choice(204, ne, replace=False)
        cw[pos] ^= rng.integers(1, 256, ne, dtype=np.uint8)
        pk[k] = cw
    tail = pkg.DvbsTailBank(engine, 1, max_bits=1632 * 8 * 8)
    ts = tail.rs_stage(pk)                                    # dispersal never reset (no stage before it): bytes 1..187 pass unchanged
    corrected, status, nerr = tail.tap(1).reshape(-1, 204), tail.tap(2), tail.tap(3)
    tail.close()
    assert ts.shape == (len(nes), 188) and corrected.shape == pk.shape
    outs, errs, prev, dispersal_idle = [], [], np.zeros(188, np.uint8), True
    for k in range(len(nes)):
        msg = corrected[k, :188] if status[k] else prev       # dvbs_reedsolomon.h:26-47: obuffer is only written by a successful decode
        prev = msg
        # the TS output of the same stage run shows the stale-output rule as the kernel applies it: until a message starts with 0xB8
        # (which starts the dispersal generator) bytes 1..187 pass unchanged
        dispersal_idle = dispersal_idle and msg[0] != 0xB8
        if dispersal_idle:
            assert np.array_equal(ts[k, 1:], msg[1:]), k
        outs.append(np.concatenate([msg, pk[k, 188:]]))
        errs.append(int(np.count_nonzero(pk[k, :188] != msg)))
        assert errs[-1] == int(nerr[k]), k
    assert errs == c['errors'] and sha(np.concatenate(outs)) == c['sha']
    assert 0 in status and 1 in status                       # both paths occurred


def test_energy_dispersal_removal(engine, pkg):
    """DVBSScrambling::descramble on 12 frames with inverted sync bytes at varying packets (generator resets)"""
    c = GD['descramble']
    rng = np.random.default_rng(c['seed'])
    tail = pkg.DvbsTailBank(engine, 1, max_bits=1632 * 8 * 4)
    outs = []
    for rep in range(12):
        frm = rng.integers(0, 256, 1632, dtype=np.uint8)
        for k in range(8):
            frm[204 * k] = 0xB8 if (rep % 3 != 0 and k == (rep % 8)) else 0x47
        ts = tail.rs_stage(frm.reshape(8, 204), skip_rs=True)
        o = frm.reshape(8, 204).copy()
        o[:, :188] = ts
        outs.append(o.reshape(-1))
    tail.close()
    assert sha(np.concatenate(outs)) == c['sha']


def test_viterbi_reproduces_reference_outputs(engine, pkg):
    """Viterbi_DVBS::work as the reference ran it over every golden stream: one ViterbiBatch, two calls of 3 + 5 blocks; per block the
    output count and the state row (BER bits, state, rate, phase, shift), per stream the digest of the bits written"""
    import torch
    import orc_dvbs as od
    g = GD['viterbi']
    cases = od.viterbi_case_streams(g['blocks'])
    assert [c[0] for c in cases] == [c['name'] for c in g['streams']]
    for (name, soft), c in zip(cases, g['streams']):
        assert sha(soft) == c['in_sha'], 'input generator drifted; regenerate the goldens'
    d = torch.from_numpy(np.stack([c[1] for c in cases])).cuda()
    vit = pkg.ViterbiBatch(engine, len(cases), g['ber_threshold'], g['max_outsync'])
    parts = [vit.work(d[:, :3].contiguous()), vit.work(d[:, 3:].contiguous())]
    gb, gn, gs = [torch.cat([parts[0][k], parts[1][k]], 1).cpu().numpy() for k in range(3)]
    vit.close()
    for s, c in enumerate(g['streams']):
        assert gn[s].tolist() == c['counts'], c['name']
        assert gs[s].tolist() == c['state_rows'], c['name']
        assert sha(od.viterbi_written_bits(gb[s], gn[s], gs[s])) == c['bits_sha'], c['name']


def test_ccdec_reproduces_reference_outputs(engine, pkg):
    """CCDecoder::work, chained blocks twice over, for every golden frame size: the digest of each decoded block"""
    import torch
    import orc_dvbs as od
    assert [c['frame'] for c in GD['ccdec']] == od.CCDEC_FRAMES
    for c in GD['ccdec']:
        frame, S, nblk = c['frame'], c['streams'], c['blocks']
        soft = od.ccdec_case_softs(frame, S, nblk)
        assert sha(soft) == c['in_sha'], 'input generator drifted; regenerate the goldens'
        dec = pkg.CcDecoderBatch(engine, S, frame)
        got = [dec.work(torch.from_numpy(soft).cuda(), nblk, 2 * frame).cpu().numpy() for _ in range(c['reps'])]
        dec.close()
        assert [sha(got[rep][s, b]) for s in range(S) for rep in range(c['reps']) for b in range(nblk)] == c['block_sha'], frame


def _bbts_golden_cases():
    """(golden case, its calls' frames) for kbch 3072 and 14232, cut after 9 frames"""
    import orc_bbts as B
    frames = {c[0]: c for c in B.all_parser_cases()}
    out = []
    for c in GB['ts_fuzz'] + GB['gse']:
        if c['kbch'] not in (3072, 14232):
            continue
        calls, used = [], 0
        for fr, want in zip(frames[c['name']][2], c['calls']):
            used += len(fr)
            if used > 9:
                break
            assert sha(fr) == want['sha256_in'], 'input generator drifted; regenerate the goldens'
            calls.append((fr, want))
        out.append((c, calls))
    return out


@pytest.mark.parametrize('variant', ['gse_on_device', 'gse_on_host', 'mode_adaptation_switched_off'])
def test_bbts_parser_reproduces_reference_outputs(engine, pkg, variant):
    """BBFrameTSParser::work as the reference ran it, call by call: return value, bytes and the public fields.  A call recorded as
    undefined in the reference is not fed; a fresh bank follows it, as in the generator."""
    import orc_bbts as B
    compared = gse_bytes = 0

    def bank(kbch):
        p = pkg.BbTsParserBank(engine, 1, kbch, 8)
        if variant == 'gse_on_host':
            p.set_gse_path(p.GSE_HOST)
        if variant == 'mode_adaptation_switched_off':
            p.set_mode_adaptation(True)
            p.set_mode_adaptation(False)
        return p

    for c in GB['ts_round_trip']:
        if c['kbch'] not in (3072, 14232):
            continue
        fr, _ = B.ts_round_trip_frames(c['kbch'], c['dfl_bytes'], c['nframes'])
        assert sha(fr) == c['sha256_in']
        p = bank(c['kbch'])
        out = np.concatenate([p.work(fr[:4]), p.work(fr[4:])])
        assert sha(out) == c['sha256_out'] and out.size == 188 * c['packets_out']
    for c, calls in _bbts_golden_cases():
        p = bank(c['kbch'])
        for ci, (fr, want) in enumerate(calls):
            if want['undefined']:
                p = bank(c['kbch'])
                continue
            out = p.work(fr, cap=B.call_cap(fr))
            st = p.stats()
            assert out.size == want['n'] and sha(out) == want['sha256_out'], (c['name'], ci)
            assert [st[k] for k in B.FIELD_KEYS] == want['fields'], (c['name'], ci)
            compared += 1
            gse_bytes += out.size if c['name'] in [g['name'] for g in GB['gse']] else 0
    assert compared > 100 and gse_bytes > 10000       # the cut to 9 frames and the undefined calls left the comparison its substance
