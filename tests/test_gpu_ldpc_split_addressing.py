"""The half-row LDPC decoder (csrc/ldpc_split_kernel.hip) fetches a thread's table entry and message record, and stores the record, through STRIDED buffer resources: the
hardware adds lane x stride, the wave's base and the pseudo-layer's offset ride in the scalar offset.  A wrong stride, record count or per-wave offset shows at thread 767, at
wave 11, at the last pseudo-layer and at the end of the LAST workgroup's message workspace -- places a large batch of decodable frames can leave looking plausible.  So: every
code the decoder serves, batches of 1, 2, 3 and grid + 1 frames (the last workgroup's workspace is used, one workgroup decodes a second frame on used records), forced and
normal mode, decodable frames and a uniform-noise frame (never converges: chain walks and speculative passes run, every table and record path is taken).  BBFRAME bytes and
trial counts must equal the oracle's FEC chain, with the speculative layers' attempts left alone and with every attempt made to fail."""
import numpy as np
import pytest
import orc
from test_gpu_fec import MARGINAL_SNR, make_llrs
from test_gpu_ldpc_split import CODES

pytestmark = pytest.mark.gpu
MODES = [(1, 6), (0, 16)]          # (force, max_trials)


@pytest.fixture(scope='module', params=[{'ldpc_split': 1}, {'ldpc_split': 1, 'ldpc_split_fail_attempts': 1}], ids=['half_row', 'half_row_attempts_fail'])
def split_engine(pkg, request):
    import torch
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    eng = pkg.Engine(0, options=request.param)
    yield eng
    eng.close()


_cases = {}


def case(rate, short):
    """three frames of the code -- decodable, uniform noise, decodable -- and the oracle's FEC chain on them in both modes (computed once per code, never changed)"""
    if (rate, short) not in _cases:
        rng = np.random.default_rng(4100 + rate)
        m = MARGINAL_SNR[rate]
        p, llr, _ = make_llrs(rate, short, 3, rng, [m + 0.5, m + 1.0, m + 1.0])
        llr[1] = rng.integers(-128, 128, size=p['N']).astype(np.int8)
        want = {}
        for force, mt in MODES:
            out = np.zeros((3, p['kbch'] // 8), np.uint8)
            trials = np.zeros(3, np.int32)
            for f in range(3):
                c = np.zeros(1, np.int32)
                trials[f] = orc.lib().orc_fec_decode_frame(rate, short, llr[f].copy(), mt, force, out[f], c)
            want[(force, mt)] = (out, trials)
        llr.setflags(write=False)
        _cases[(rate, short)] = (llr, want)
    return _cases[(rate, short)]


@pytest.mark.parametrize('rate,short', CODES)
def test_strided_addressing_every_batch_shape(split_engine, rate, short):
    import torch
    assert split_engine.ldpc_decoder_form(rate, bool(short)) == 2
    info = split_engine.ldpc_plan_info(rate, bool(short))
    grid = info['cus'] * info['blocks_per_cu']          # what a launch of at least that many frames uses
    llr3, want = case(rate, short)
    for nf in (1, 2, 3, grid + 1):
        idx = (np.arange(nf) + nf) % 3                  # (one frame: the noise frame)
        x = torch.from_numpy(llr3[idx]).cuda()
        for force, mt in MODES:
            want_out, want_trials = want[(force, mt)]
            out, trials, _ = split_engine.fec_decode(x, rate, bool(short), max_trials=mt, force=bool(force))
            torch.cuda.synchronize()
            trials = trials.cpu().numpy()
            out = out.cpu().numpy()
            assert np.array_equal(trials, want_trials[idx]), (nf, force, mt, np.flatnonzero(trials != want_trials[idx])[:8])
            bad = np.flatnonzero((out != want_out[idx]).any(axis=1))
            assert bad.size == 0, (nf, force, mt, bad[:8])
