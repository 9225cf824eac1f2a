"""The throughput mode's stream plan: a big single-configuration bank drives at most three HIP streams of the engine's own -- AGC + timing
recovery, post stages, decoder -- so that with the host's stream each has a hardware queue to itself on the runtime's default of four, whatever the priority balancer
does; and what the plan delivers is what the synchronous mode delivers on the same input."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

CALLS = 12
CHUNK = 2 * 21690 + 20        # a PLFRAME of 8PSK 3/4 (normal frames, no pilots) at 2 samples per symbol, and a little more: the frame boundaries drift through the calls
DISTINCT = 4


def _signals():
    import orc
    return [orc.transmit(14, 0, 0, nframes=CALLS + 1, seed=300 + i, esn0_db=14.0, cfo=1e-4, timing=0.1 * i, phase0=0.2, lead_symbols=200 + 70 * i)[0] for i in range(DISTINCT)]


def _run(pkg, sigs, S, pipelined, duty=None, max_streams=None):
    """-> per stream (delivered bytes, byte count of every call, per-frame statistics); asserts the engine's stream count after every call when max_streams is given"""
    import torch
    eng = pkg.Engine(0)
    cfg = eng.default_cfg(14, False, False, force_ldpc_iters=20, max_ldpc_trials=20)
    dms = [eng.demod(cfg, max_samples=CHUNK) for _ in range(S)]
    outs = [torch.zeros(4 * 6000, dtype=torch.uint8, device='cuda') for _ in range(S)]
    d_sigs = [torch.from_numpy(x).cuda() for x in sigs]
    if duty is not None:
        eng.set_option('g_prio_duty', duty)
    eng.set_pipelined(pipelined)
    data, counts, stats = [bytearray() for _ in range(S)], [[] for _ in range(S)], [[] for _ in range(S)]
    seen = []

    def streams_now():
        if max_streams is not None:
            seen.append(eng.get_state('engine_streams'))
            assert seen[-1] <= max_streams, 'the engine owns %d HIP streams (calls so far: %s)' % (seen[-1], seen)
    streams_now()
    for c in list(range(CALLS)) + ([None] if pipelined else []):          # (pipelined: one empty call collects the last call's frames)
        parts = [d_sigs[i % DISTINCT][c * CHUNK:(c + 1) * CHUNK] if c is not None else d_sigs[0][:0] for i in range(S)]
        nb = eng.process_batch(dms, parts, outs)
        streams_now()
        host = torch.stack(outs).cpu().numpy()
        for i in range(S):
            data[i] += host[i, :nb[i]].tobytes()
            counts[i].append(int(nb[i]))
            stats[i] += [(s.pl_sync_best_match, s.detected_modcod, s.detected_shortframes, s.detected_pilots, s.coarse_freq_err, s.ldpc_trials, s.bch_corrections,
                          s.bbframe_bytes) for s in dms[i].stats()]
    eng.set_pipelined(False)
    for d in dms:
        d.close()
    eng.close()
    if pipelined:      # call k's frames come out of call k + 1: the first call delivers nothing
        assert all(x[0] == 0 for x in counts)
        counts = [x[1:] for x in counts]
    return [(bytes(data[i]), counts[i], stats[i]) for i in range(S)]


def _same(a, b):
    assert len(a) == len(b)
    for i, (x, y) in enumerate(zip(a, b)):
        assert x[1] == y[1], 'stream %d: byte counts per call differ' % i
        assert x[0] == y[0], 'stream %d: delivered bytes differ' % i
        assert x[2] == y[2], 'stream %d: per-frame statistics differ' % i


@pytest.fixture(scope='module')
def signals():
    import torch
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    return _signals()


@pytest.fixture(scope='module')
def sync_512(pkg, signals):
    ref = _run(pkg, signals, 512, False)
    assert all(len(x[0]) > 0 and len(x[2]) >= CALLS - 3 for x in ref), 'the synchronous run delivered too little to compare'
    return ref


@pytest.mark.parametrize('duty', [-1, 0, 7])
def test_big_bank_owns_three_streams_and_delivers_what_the_synchronous_mode_does(pkg, signals, sync_512, duty):
    """512 streams of 8PSK 3/4, 12 calls, forced iterations: balancer automatic (-1), share forced to 0 (post stages behind the last slice) and to 7 (front end critical)"""
    got = _run(pkg, signals, 512, True, duty=duty, max_streams=3)
    _same(got, sync_512)


def test_small_bank_delivers_what_the_synchronous_mode_does(pkg, signals):
    """2 streams: the small-bank flow keeps its streams; equality alone is asserted"""
    ref = _run(pkg, signals, 2, False)
    assert all(len(x[0]) > 0 for x in ref)
    _same(_run(pkg, signals, 2, True), ref)
