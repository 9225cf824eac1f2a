"""Calls whose pooled frame count is ODD, in the two flows that keep a table of device pointers behind per-frame arrays in one scratch buffer
(csrc/scratch_layout.h): the job buffer of a FEC job in parts, which an ACM/VCM bank (process_vcm_group) and a mixed-MODCOD bank (process_mixed) build
in either mode (build_parts_job: results | indices | destinations), and the mixed bank's per-frame table (LLR pointers | slot indices).  Three streams
each, one call with the whole signal, synchronous and pipelined; BBFRAMEs, trial counts and per-frame stats equal the oracle's."""
import numpy as np
import pytest
import orc

pytestmark = pytest.mark.gpu

S = 2           # PLS code bit: short frame
# per stream: the PLS codes its frames cycle over (ACM/VCM bank) / its one MODCOD (mixed bank, short frames, pilots as given) and its frame count
# (the oracle delivers 7 + 7 + 9 = 23 and 9 + 8 + 8 = 25 frames of them, the first ones undecodable while the loops settle: found by running bank() on the CPU)
VCM_STREAMS = [([(6 << 2) | S, (14 << 2) | S], 12), ([(4 << 2) | S, (12 << 2) | S | 1], 12), ([(14 << 2) | S | 1, (6 << 2) | S], 12)]
MIXED_STREAMS = [((4, 1, 0), 10), ((14, 1, 1), 9), ((6, 1, 0), 9)]


def stats_key(x, kind):
    """a frame's stats as the oracle (tap 4) or a GPU handle (stats()) reports them, the floats by bit pattern: the fields test_gpu_s2chain.py compares with
    the oracle's in the CCM and in the ACM/VCM mode (the BBFRAME size in the latter only)"""
    if hasattr(x, 'detect_modcod'):
        x = (x.best_match, x.fed_err, x.detect_modcod, x.detect_short, x.detect_pilots, x.ldpc_trials, x.bch_corr, x.bbframe_bytes)
    else:
        x = (x.pl_sync_best_match, x.coarse_freq_err, x.detected_modcod, x.detected_shortframes, x.detected_pilots, x.ldpc_trials, x.bch_corrections, x.bbframe_bytes)
    return tuple(int(np.float32(v).view(np.uint32)) for v in x[:2]) + x[2:8 if kind == 'vcm' else 7]


def bank(kind):
    """-> per stream (iq, demodulator configuration arguments, the oracle's BBFRAME bytes of the one call, its per-frame stats)"""
    out = []
    for k, (what, nframes) in enumerate(VCM_STREAMS if kind == 'vcm' else MIXED_STREAMS):
        common = dict(seed=900 + k, esn0_db=18.0, cfo=2e-4 * k, timing=0.1 * k, phase0=0.1, lead_symbols=300 + 10 * k)
        if kind == 'vcm':
            iq, _ = orc.transmit_vcm(what, nframes, **common)
            args, kw = (4, 1, 0), dict(acm_vcm=1)
        else:
            iq, _, _ = orc.transmit(*what, nframes=nframes, **common)
            args, kw = what, {}
        rx = orc.OracleRx(orc.default_cfg(*args, **kw))
        frames = rx.process(iq)
        out.append((iq, args, kw, np.concatenate([np.asarray(f).reshape(-1) for f in frames] + [np.zeros(0, np.uint8)]), [stats_key(x, kind) for x in rx.tap(4)]))
    return out


@pytest.mark.parametrize('kind', ['vcm', 'mixed'])
def test_odd_frame_count_per_call_equals_oracle(engine, pkg, kind):
    import torch
    streams = bank(kind)
    nf = sum(len(s[4]) for s in streams)
    print('frames per stream (oracle):', [len(s[4]) for s in streams])
    assert nf % 2 == 1 and nf >= 9 and all(len(s[4]) > 0 for s in streams), [len(s[4]) for s in streams]     # the subject: an odd pooled count, every stream in it
    cap = max(s[0].size for s in streams) // 2 + 100000
    for pipelined in (False, True):
        dms = [engine.demod(engine.default_cfg(a[0], bool(a[1]), bool(a[2]), **kw), max_samples=iq.size) for iq, a, kw, _, _ in streams]
        tout = [torch.zeros(cap, dtype=torch.uint8, device='cuda') for _ in streams]
        engine.set_pipelined(pipelined)
        try:
            nb = engine.process_batch(dms, [torch.from_numpy(s[0]).cuda() for s in streams], tout)
            if pipelined:       # the call's job is delivered by the next call
                assert sum(nb) == 0 and all(len(d.stats()) == 0 for d in dms)
                nb = engine.process_batch(dms, [torch.empty(0, dtype=torch.complex64, device='cuda') for _ in streams], tout)
            for i, (d, s) in enumerate(zip(dms, streams)):
                assert np.array_equal(tout[i][:nb[i]].cpu().numpy(), s[3]), (kind, pipelined, i)
                assert [stats_key(x, kind) for x in d.stats()] == s[4], (kind, pipelined, i)
        finally:
            engine.set_pipelined(False)
            for d in dms:
                d.close()
