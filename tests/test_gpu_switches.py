"""The throughput mode's calls against work the host puts on the legacy null stream between them."""
import pytest


@pytest.mark.gpu
def test_null_stream_work_of_the_host_between_pipelined_calls(pkg):
    """the throughput mode's streams are non-blocking, and each call starts behind the host's work on the legacy null stream: the same pipelined calls with a null-stream
    operation of the host (a torch default-stream kernel and a plain hipMemcpy-style copy) between every two calls deliver what the calls without it deliver"""
    import numpy as np
    import torch
    import orc
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    S, chunk = 6, 40000
    sigs = [orc.transmit(14, 1, 0, nframes=7, seed=90 + i, esn0_db=15.0, cfo=1e-4, timing=0.1 * i, phase0=0.2, lead_symbols=300 + 50 * i)[0] for i in range(S)]
    got = []
    for poke in (False, True):
        eng = pkg.Engine(0)
        cfg = eng.default_cfg(14, True, False, max_ldpc_trials=16)
        dms = [eng.demod(cfg, max_samples=chunk) for _ in range(S)]
        outs = [torch.zeros(1 << 18, dtype=torch.uint8, device='cuda') for _ in range(S)]
        eng.set_pipelined(True)
        per = [bytearray() for _ in range(S)]
        junk = torch.zeros(1 << 20, device='cuda')
        for a in list(range(0, max(x.size for x in sigs), chunk)) + [None]:
            parts = [torch.from_numpy(np.ascontiguousarray(x[a:a + chunk] if a is not None else x[:0])).cuda() for x in sigs]
            nb = eng.process_batch(dms, parts, outs)
            for i in range(S):
                per[i] += outs[i][:nb[i]].cpu().numpy().tobytes()
            if poke:
                junk.add_(1.0)                                  # a kernel on the null stream
                junk[:1024].copy_(torch.ones(1024))             # and a host -> device copy on it
        eng.set_pipelined(False)
        for d in dms:
            d.close()
        eng.close()
        got.append([bytes(x) for x in per])
    assert got[0] == got[1] and all(len(x) > 0 for x in got[0])
