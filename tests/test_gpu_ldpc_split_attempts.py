"""The half-row LDPC decoder's ATTEMPTS (csrc/ldpc_split_kernel.hip: chain_layer, spec_layer): a layer with shared bits whose predecessor changed no shared posterior first runs
the plain row update of every row with NO store to a shared slot and asks whether any row's update changed a posterior of its shared slots; where none did the layer is done,
where one did it goes the long way (chain walk / passes) from the inputs in the registers -- and the rows of level 1 still owe their shared slots' stores.

Three engines -- the decoder as it is, the decoder with every attempt made to fail (context option ldpc_split_fail_attempts: the long way after an attempt, in every layer that
tries), and the lane-per-row decoder (ldpc_split = 0: no attempts at all) -- must leave the same posteriors, trial counts and hard bits, and those must be the oracle's
(orc_fec_decode_frame: the reference's decoder, then hard decisions, BCH and descrambling), on 48 frames per launch (every workgroup slot of the persistent grid sees a frame
change where the grid is smaller, and neighbouring workgroups work on different frames): frames that decode at once (attempts hold), frames at the code's threshold (attempts
start, fail and start again inside one frame) and uniform int8 noise (the verdicts rarely invite an attempt, and the attempts made fail) -- with 50 forced iterations and with 16
trials and early exit.  A batch that alternates decodable and noise frames puts neighbouring workgroups of a compute unit into different regimes; a launch repeated into the same
workspace, with another one between, must repeat its outputs (the verdict words are cleared per frame, the records per frame slot)."""
import functools
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest
import orc
from test_gpu_fec import MARGINAL_SNR

pytestmark = pytest.mark.gpu
CODES = [0, 2, 3, 4, 5, 6]            # normal frames, rates 1/4, 2/5, 1/2, 3/5, 2/3, 3/4: what the half-row decoder takes (2/5 and 2/3: layer 0, with the row that has no previous parity bit, has shared bits)
INPUTS = ['decodable', 'threshold', 'noise']
MODES = [(1, 50), (0, 16)]            # (force, max_trials)
NF = 48
ENGINES = [('half_row', {'ldpc_split': 1}), ('half_row_attempts_fail', {'ldpc_split': 1, 'ldpc_split_fail_attempts': 1}), ('lane_per_row', {'ldpc_split': 0})]


@functools.lru_cache(maxsize=None)
def frames(rate, kind):
    """48 frames of one kind, int8 [48, N] (read-only): 12 codewords of the CPU encoder, every frame with noise of its own"""
    p = orc.fec_params(rate, 0)
    rng = np.random.default_rng(4000 + 10 * rate + INPUTS.index(kind))
    if kind == 'noise':
        llr = rng.integers(-128, 128, size=(NF, p['N'])).astype(np.int8)
    else:
        snr = MARGINAL_SNR[rate] + (3.0 if kind == 'decodable' else 0.0)
        words = [orc.encode_frame(rate, 0, 7000 + 100 * rate + k)[1] for k in range(12)]
        llr = np.stack([orc.bits_to_llr(words[f % 12], snr, rng) for f in range(NF)])
    llr.setflags(write=False)
    return llr


def oracle(rate, llr, force, max_trials):
    """-> (posteriors int8 [F, N], trials int32 [F], hard uint8 [F, K/8], bbframes uint8 [F, kbch/8], bch corrections int32 [F]), frame by frame (the oracle takes no lock while it decodes)"""
    p = orc.fec_params(rate, 0)
    F = llr.shape[0]
    post = llr.copy()
    trials = np.zeros(F, np.int32)
    bb = np.zeros((F, p['kbch'] // 8), np.uint8)
    corr = np.zeros(F, np.int32)
    orc.lib()

    def one(f):
        c = np.zeros(1, np.int32)
        trials[f] = orc.lib().orc_fec_decode_frame(rate, 0, post[f], max_trials, force, bb[f], c)
        corr[f] = c[0]
    with ThreadPoolExecutor(max_workers=min(8, os.cpu_count() or 1)) as ex:
        list(ex.map(one, range(F)))
    hard = np.packbits((post[:, :p['K']] < 0).astype(np.uint8), axis=1)
    return post, trials, hard, bb, corr


@pytest.fixture(scope='module')
def engines(pkg):
    import torch
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    made = []
    try:
        for name, opts in ENGINES:
            eng = pkg.Engine(0, options=opts)
            made.append((name, eng))
            for r in CODES:
                assert eng.ldpc_decoder_form(r, False) == (2 if opts['ldpc_split'] else 0)
        yield made
    finally:
        for _, eng in made:
            eng.close()


def check_engines(engines, rate, llr, force, max_trials, with_fec):
    import torch
    want_post, want_trials, want_hard, want_bb, want_corr = oracle(rate, llr, force, max_trials)
    x = torch.from_numpy(np.array(llr)).cuda()             # (a writable copy: the shared inputs are read-only)
    for name, eng in engines:
        hard, trials, post = eng.ldpc_decode(x, rate, False, max_trials=max_trials, force=bool(force), want_post=True)
        torch.cuda.synchronize()
        assert np.array_equal(trials.cpu().numpy(), want_trials), name
        assert np.array_equal(post.cpu().numpy(), want_post), name
        assert np.array_equal(hard.cpu().numpy(), want_hard), name
        if with_fec:
            out, ftrials, corr = eng.fec_decode(x, rate, False, max_trials=max_trials)
            torch.cuda.synchronize()
            assert np.array_equal(ftrials.cpu().numpy(), want_trials), name
            assert np.array_equal(out.cpu().numpy(), want_bb), name
            assert np.array_equal(corr.cpu().numpy(), want_corr), name
    return want_trials


@pytest.mark.parametrize('force,max_trials', MODES, ids=['forced50', 'trials16'])
@pytest.mark.parametrize('kind', INPUTS)
@pytest.mark.parametrize('rate', CODES)
def test_attempts_three_engines_and_the_oracle(engines, rate, kind, force, max_trials):
    trials = check_engines(engines, rate, frames(rate, kind), force, max_trials, with_fec=not force)
    if not force:
        # the inputs are what their names say: every decodable frame decodes well inside the limit, no noise frame does
        if kind == 'decodable':
            assert (trials >= 0).all() and (trials < max_trials).all()
        if kind == 'noise':
            assert (trials < 0).all()


@pytest.mark.parametrize('rate', CODES)
def test_attempts_alternating_decodable_and_noise(engines, rate):
    """neighbouring workgroups of a compute unit in different regimes: frame 2k decodes, frame 2k + 1 is noise"""
    llr = np.empty_like(frames(rate, 'decodable'))
    llr[0::2] = frames(rate, 'decodable')[:NF // 2]
    llr[1::2] = frames(rate, 'noise')[:NF // 2]
    check_engines(engines, rate, llr, 1, 50, with_fec=False)
    trials = check_engines(engines, rate, llr, 0, 16, with_fec=True)
    assert (trials[0::2] >= 0).all() and (trials[1::2] < 0).all()


@pytest.mark.parametrize('rate', [6, 2])
def test_attempts_same_launch_twice_into_the_same_workspace(engines, rate):
    """what a frame left behind -- verdict words, records, posteriors in LDS -- must not reach the next launch's frames: A, B, A again gives A's outputs again (both modes)"""
    import torch
    a = torch.from_numpy(np.array(frames(rate, 'threshold'))).cuda()
    b = torch.from_numpy(np.array(frames(rate, 'noise'))).cuda()
    for name, eng in engines[:2]:
        for force, mt in MODES:
            first = [t.clone() for t in eng.ldpc_decode(a, rate, False, max_trials=mt, force=bool(force), want_post=True)]
            eng.ldpc_decode(b, rate, False, max_trials=mt, force=bool(force), want_post=True)
            again = eng.ldpc_decode(a, rate, False, max_trials=mt, force=bool(force), want_post=True)
            twice = eng.ldpc_decode(a, rate, False, max_trials=mt, force=bool(force), want_post=True)
            torch.cuda.synchronize()
            for u, v, w in zip(first, again, twice):
                assert torch.equal(u, v) and torch.equal(u, w), (name, force, mt)
