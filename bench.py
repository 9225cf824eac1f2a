#!/usr/bin/env python3
"""Headline benchmark: Msymbols/s of the DVB-S2 demod + FEC hot path on MI355X.

Workload (BASELINE.json configs[2], the one the metric is quoted on): DVB-S2 8PSK 3/4 normal FECFRAME (MODCOD 14, PLFRAME
21 690 symbols, LDPC table B7, BCH t=12), pilots off, LDPC forced to exactly 50 layered iterations per frame (no early exit).
`--streams` independent transponder streams per GPU, each a continuous synthetic 27.5 Msym/s-class signal built by the
repo's own transmitter under the conditions of SURVEY 8(d): complex64 IQ at 2 samples/symbol, RRC 0.35, carrier offset
1e-3 rad/sample, timing offset 0.3 sample, sampling-clock error ~10 ppm, AWGN.  `--distinct` (64) different signal blocks
exist; every stream owns a PRIVATE copy in HBM, cyclically shifted by a stream-specific amount, so the streams' loops run in
different phases and the IQ (11 GB for 4096 streams x 8 frames) cannot be served from the Infinity Cache.  One step = one
dvbs2gpu_demod_process_batch call of `--frames` (8) PLFRAMEs per stream = the whole hot path
  IQ -> AGC -> NCO -> Gardner -> RRC -> /2 -> PL sync -> FED/PLL/PLHDR -> soft demap + de-interleave
     -> LDPC (50 it) -> BCH -> BB descramble -> BBFRAMEs
over every stream; the streams keep their loop state from step to step (the blocks are periodic, so the signals are
seamless).  value = PLFRAME symbols consumed per second, all GPUs.  No candidate blocks are discarded: the fraction of the
delivered frames that equal a transmitted BBFRAME is REPORTED (the reference's decision-directed loops, which the engine
reproduces bit for bit, lose frames at low SNR), and every delivered frame of every stream is compared on the device.

    python bench.py --gpus N --steps K --warmup W          (N>1: launched by torch.distributed.run)
    python bench.py --gpus N --steps K --warmup W --full   the same, plus every check and secondary measurement (below)
    python bench.py --config mixed64 [--gpus N]            BASELINE config 4 (64 mixed-MODCOD transponders, strong scaling)

Prints ONE JSON line on rank 0.  A plain run sets up, warms up, times the K steps and prints the headline (`value`, `ms_per_step`,
`stage_ms_per_step`: hipEvent pairs around every launch inside the timed steps).  `--dump-outputs DIR` writes what the last timed
step delivered as DIR/*.npy (see last_step_outputs).  `--full` adds the frame check of the last timed step + the pipeline flush, the
decoder self-check, `roofline` (dominant kernel = the LDPC decoder: the launches inside the timed steps plus stand-alone launches),
`cpu_baseline` (rank 0, N=1: the reference's own FEC code compiled into oracle/_ref when that build travelled, else the oracle
port, plus the oracle front end), `secondary` (configs 2, 5, D and the mixed-MODCOD batch) and the two config-4 lines.
"""
import argparse
import json
import os
import sys
import threading
import time

import numpy as np

# Mixed batches drive up to nine HIP streams side by side, HIP maps them onto GPU_MAX_HW_QUEUES hardware queues (default 4; 64 mixed transponders: 74 ... 85 ms per call on
# 4 queues, 48 on 6, 44 on 8; the DVB-S line late in a full run, with the S2 engine's streams still alive: 1 570 Msym/s on 8 queues, 2 230-2 350 on 12).  The library asks for
# 12 when it is loaded (csrc/capi.hip) -- but this process imports torch first, whose HIP runtime has read its environment by then: so here, and in any host that
# initialises HIP before it loads the plugin, the variable is set up front.
if not os.environ.get('DVBS2GPU_BENCH_DEFAULT_QUEUES'):          # (development aid: leave the runtime's default of 4 hardware queues)
    os.environ.setdefault('GPU_MAX_HW_QUEUES', '12')
ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

MODCOD = 14          # 8PSK 3/4
RATE, SHORT = 6, 0
PILOTS = 0
ITERS = 50
# SURVEY 8(d) asks for threshold + 1 dB (9 dB for 8PSK 3/4).  The reference receiver the engine reproduces (decision-directed PLL on a
# 256x256 LUT, AGC set point vs demapper prescale) delivers NO frame at 9 dB with a 1e-3 carrier offset -- the CPU oracle shows
# the same -- and all of them from 11 dB on: 11 dB is the lowest level at which the comparison with the transmitted frames means
# something.  The decoder's work does not depend on it (50 forced iterations).
ESN0_DB = 11.0
CFO = 1e-3           # rad/sample
PPM = 10.0           # sampling-clock error
HBM_PEAK_GBS = 8000.0
DISTINCT = 64
PREROLL_FRAMES = 24  # untimed frames per stream before the warm-up: loop acquisition (AGC, Gardner, PL sync, PLL)
WORKLOAD = ('DVB-S2 8PSK 3/4 normal FECFRAME (MODCOD 14), pilots off, 27.5 Msym/s-class streams at 2 sps, carrier offset 1e-3 rad/sample, '
            'clock error ~10 ppm, Es/N0 %.0f dB, 50 forced LDPC iterations, IQ in -> BBFRAMEs out' % ESN0_DB)


def ldpc_source_hash():
    """identifies the decoder build a set of PMC figures belongs to (tools/collect_profiles.py stores it with them)"""
    import hashlib
    h = hashlib.sha256()
    for n in ('ldpc_kernel.hip', 'ldpc_split_kernel.hip', 'ldpc_split_plan.h', 'ldpc_lane_common.h', 'ldpc_plan.h', 'ldpc_dev_common.h'):
        h.update(open(os.path.join(ROOT, 'sdrpp-dvbs-demodulator_amd', 'csrc', n), 'rb').read())
    return h.hexdigest()[:16]


def make_block(modcod, short, pilots, frames, seed, esn0_db, cfo=CFO, ppm=PPM):
    """one periodic IQ block from the repo's transmitter (oracle/s2chain.cpp, bench/test infrastructure): `frames` PLFRAMEs, resampled so
    that the sampling clock is ~ppm off, carrier offset rounded so that the block repeats seamlessly.  -> (iq, bbframes)"""
    import orc
    mp = orc.modcod_params(modcod, short, pilots)
    ns = frames * mp['plframe']
    nsamp = 2 * ns + (int(round(2 * ns * ppm * 1e-6)) if ppm else 0)
    c = 2 * np.pi * round(cfo * nsamp / (2 * np.pi)) / nsamp if cfo else 0.0
    iq, bb, _ = orc.transmit(modcod, short, pilots, nframes=frames, seed=seed, esn0_db=esn0_db, cfo=c, timing=0.3, phase0=0.1, lead_symbols=0,
                             circular=1, nsamples=nsamp if nsamp != 2 * ns else 0)
    return iq, bb


class FrameChecker:
    """device-side comparison of every delivered BBFRAME with the transmitted ones of its stream's block: a 64-bit hash finds the
    candidate, then the bytes are compared in full"""

    def __init__(self, torch, dev, sent, block_of_stream, kb, cap_frames):
        self.t, self.dev, self.kb, self.cap = torch, dev, kb, cap_frames
        g = torch.Generator(device='cpu'); g.manual_seed(1234)
        self.w = (torch.randint(1, 2 ** 62, (kb,), generator=g, dtype=torch.int64) | 1).to(dev)
        self.sent = torch.from_numpy(np.stack(sent)).to(dev)                      # [D, F, kb]
        self.hs = self._hash(self.sent)                                           # [D, F]
        self.block = torch.as_tensor(block_of_stream, dtype=torch.int64, device=dev)

    def _hash(self, frames):
        out = []
        for a in range(0, frames.shape[0], 256):                                  # (chunks bound the int64 temporary)
            out.append((frames[a:a + 256].to(self.t.int64) * self.w).sum(-1))
        return self.t.cat(out)

    def check(self, out_all, nbytes, want_mask=False):
        """out_all uint8 [S, cap*kb]; nbytes list -> dict(delivered, equal, out_of_order) [+ the per-frame masks `valid`, `good` with want_mask]"""
        t = self.t
        S = out_all.shape[0]
        fr = out_all.view(S, self.cap, self.kb)
        nfr = t.as_tensor(np.asarray(nbytes), dtype=t.int64, device=self.dev) // self.kb
        valid = t.arange(self.cap, device=self.dev)[None, :] < nfr[:, None]
        h = self._hash(fr)                                                        # [S, cap]
        hs = self.hs[self.block]                                                  # [S, F]
        eq = h[:, :, None] == hs[:, None, :]
        idx = eq.to(t.int8).argmax(-1)                                            # [S, cap]
        same = t.zeros_like(valid)
        for a in range(0, S, 256):
            exp = self.sent[self.block[a:a + 256, None], idx[a:a + 256]]          # [256, cap, kb]
            same[a:a + 256] = (exp == fr[a:a + 256]).all(-1)
        good = same & eq.any(-1) & valid
        F = hs.shape[1]
        both = good[:, 1:] & good[:, :-1]
        ooo = both & (idx[:, 1:] != (idx[:, :-1] + 1) % F)
        res = dict(delivered=int(valid.sum().item()), equal=int(good.sum().item()), out_of_order=int(ooo.sum().item()))
        if want_mask:
            res['valid'], res['good'] = valid.cpu().numpy(), good.cpu().numpy()
        return res


class S2Run:
    """S streams of one configuration: private IQ copies, demodulator handles, output buffers, checker"""

    def __init__(self, eng, pkg, dev, modcod, short, pilots, esn0_db, S, F, distinct, seed, iters=ITERS, force=True):
        import torch
        self.eng, self.dev, self.S, self.F = eng, dev, S, F
        info = pkg.modcod_info(modcod, bool(short), bool(pilots))
        self.info, self.sym, self.kb = info, info['plframe_symbols'], info['kbch'] // 8
        D = min(distinct, S)
        blocks = [make_block(modcod, short, pilots, F, 0xD5B2 + 1000 * seed + b, esn0_db) for b in range(D)]
        self.blocks_host = [b[0] for b in blocks]
        nsamp = blocks[0][0].size
        self.nsamp = nsamp
        d_blocks = [torch.from_numpy(b[0]).to(dev) for b in blocks]
        # private, cyclically shifted copy per stream (even shifts keep the 2-sps phase; the shift differs from stream to stream)
        self.iq = torch.empty((S, nsamp), dtype=torch.complex64, device=dev)
        for s in range(S):
            self.iq[s] = torch.roll(d_blocks[s % D], 2 * ((s // D) * 7919 % (nsamp // 2)))
        del d_blocks
        cfg = eng.default_cfg(modcod, bool(short), bool(pilots), force_ldpc_iters=iters if force else 0, max_ldpc_trials=iters)
        self.demods = [eng.demod(cfg, max_samples=nsamp) for _ in range(S)]
        self.tin = [self.iq[s] for s in range(S)]
        self.cap = F + 2
        self.out = torch.zeros((S, self.cap * self.kb), dtype=torch.uint8, device=dev)
        self.tout = [self.out[s] for s in range(S)]
        self.empty = [torch.empty(0, dtype=torch.complex64, device=dev) for _ in range(S)]
        self._step = eng.prepare_batch(self.demods, self.tin, self.tout)
        self._flush = eng.prepare_batch(self.demods, self.empty, self.tout)
        self.checker = FrameChecker(torch, dev, [b[1] for b in blocks], [s % D for s in range(S)], self.kb, self.cap)

    def step(self):
        return self._step()

    def flush(self):
        return self._flush()

    def check(self, nb, want_mask=False):
        return self.checker.check(self.out, nb, want_mask)

    def close(self):
        for d in self.demods:
            d.close()
        self.demods = []
        self.iq = self.out = None


def time_steps(run, steps, warmup, barrier, pipelined, prove_decoder=False, full=True, dump=False):
    """preroll + warm-up (untimed), then `steps` timed steps between barriers; with `full`, verifies the last timed step and the flush.
    -> (seconds, stage times, checks (None unless full), outputs of the last timed step (None unless dump))"""
    eng = run.eng
    eng.set_pipelined(pipelined)
    for _ in range(max(1, -(-PREROLL_FRAMES // run.F))):
        run.step()
    for _ in range(warmup):
        run.step()
    eng.stage_times()                      # reset the per-stage sums
    barrier()
    t0 = time.perf_counter()
    nb = None
    for _ in range(steps):
        nb = run.step()
    barrier()
    dt = time.perf_counter() - t0
    stages = eng.stage_times()
    outputs = last_step_outputs(run, nb) if dump else None      # (before the flush below writes into the same buffers)
    if not full:
        eng.set_pipelined(False)           # (drops the frames of the last timed step, which nobody collects here)
        return dt, stages, None, outputs
    balancer = {k: eng.get_state(k) for k in ('g_prio_duty', 'g_prio_auto', 'g_prio_hold', 'stage_pipeline_on', 'fec_part_on')}
    acc = run.check(nb)
    proof = None
    if pipelined:
        nb2 = run.flush()                  # the frames of the last timed step (delivered one call later)
        a2 = run.check(nb2, want_mask=prove_decoder)
        if prove_decoder:
            proof = decoder_self_check(run, nb2, a2.pop('valid'), a2.pop('good'))
        acc = {k: acc[k] + a2[k] for k in acc}
        eng.set_pipelined(False)
    acc['balancer'] = balancer
    acc['decoder_self_check'] = proof
    return dt, stages, acc, outputs


DUMP_BYTES = 48 << 20      # float32 bytes of the sampled output buffers (the whole dump stays under 64 MB)
DUMP_SEED = 2024


def last_step_outputs(run, nb):
    """What a caller of the timed path holds after the last timed step, as float arrays (uint8 -> float32 is exact):
      bytes_delivered   float64 [S]          byte counts the call returned, every stream
      frame_byte_sums   float64 [S, cap]     sum of the bytes of every delivered BBFRAME slot, every stream (0 where nothing was delivered)
      bbframes          float32 [n, cap*kb]  the output buffers of a fixed, seeded sample of n streams, bytes past the delivered count zeroed
      sample_streams    float64 [n]          which streams those are"""
    import torch
    torch.cuda.synchronize()
    S, cap, kb = run.S, run.cap, run.kb
    nbt = torch.as_tensor(np.asarray(nb, dtype=np.int64), device=run.out.device)
    valid = torch.arange(cap * kb, device=run.out.device)[None, :] < nbt[:, None]
    sums = torch.empty((S, cap), dtype=torch.float64, device=run.out.device)
    for a in range(0, S, 256):
        fr = run.out[a:a + 256] * valid[a:a + 256]
        sums[a:a + 256] = fr.view(-1, cap, kb).sum(-1, dtype=torch.int64).to(torch.float64)
    n = min(S, max(1, DUMP_BYTES // (cap * kb * 4)))
    pick = np.sort(np.random.default_rng(DUMP_SEED).choice(S, n, replace=False))
    pt = torch.as_tensor(pick, device=run.out.device)
    frames = (run.out[pt] * valid[pt]).to(torch.float32)
    return {'bytes_delivered': np.asarray(nb, dtype=np.float64), 'frame_byte_sums': sums.cpu().numpy(),
            'bbframes': frames.cpu().numpy(), 'sample_streams': pick.astype(np.float64)}


def dump_outputs(outdir, outputs):
    os.makedirs(outdir, exist_ok=True)
    for name, a in outputs.items():
        np.save(os.path.join(outdir, name + '.npy'), a)


def decoder_self_check(run, nb, valid, good, n_spread=40, n_odd=24):
    """The bench proves its own decoder at the headline shape: the LLRs of sampled frames of the LAST TIMED STEP -- streams spread over the whole bank, plus frames that are
    NOT equal to any transmitted frame (a decoder fault inside those would be invisible to the FrameChecker) -- are read back from the job's buffer
    (dvbs2gpu_debug_last_fec_job), decoded by the CPU oracle (oracle/: orc_fec_decode_frame, the job's own iteration setting) and compared byte for byte with the BBFRAMEs
    the engine delivered into the caller's output buffers.  Untimed."""
    import ctypes as C
    from concurrent.futures import ThreadPoolExecutor
    import orc
    eng = run.eng
    job = eng.last_fec_job(0)
    if not job['nf'] or job['n'] != run.S or [int(h or 0) for h in job['handles'][:4]] != [int(d.h.value or 0) for d in run.demods[:4]]:
        return {'error': 'the last delivered job is not this run\'s batch'}
    first, N, kb = job['first'], job['N'], job['kb']
    per_stream = first[1:] - first[:-1]
    assert np.array_equal(per_stream * kb, np.asarray(nb)), 'job frame table and delivered byte counts disagree'
    S, cap = valid.shape
    picks = []
    for s_ in np.linspace(0, S - 1, n_spread).astype(int):          # spread over the bank, alternating frame slots
        k = int(len(picks) % max(int(per_stream[s_]), 1))
        if per_stream[s_] > 0:
            picks.append((int(s_), k))
    odd = np.argwhere(valid & ~good)                                  # delivered, not a transmitted frame
    if len(odd):
        for i in np.linspace(0, len(odd) - 1, min(n_odd, len(odd))).astype(int):
            picks.append((int(odd[i][0]), int(odd[i][1])))
    picks = sorted(set(picks))
    hip = C.CDLL('libamdhip64.so')
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    out_host = {s_: run.out[s_].cpu().numpy() for s_ in {p_[0] for p_ in picks}}

    def one(pk):
        s_, k = pk
        f = int(first[s_]) + k
        llr = np.empty(N, np.int8)
        rc = hip.hipMemcpy(llr.ctypes.data, C.c_void_p(job['d_llr'] + f * N), N, 2)
        assert rc == 0, 'hipMemcpy'
        bbo = np.zeros(kb, np.uint8)
        c = np.zeros(1, np.int32)
        orc.lib().orc_fec_decode_frame(job['rate'], job['short'], llr, job['max_trials'], job['force'], bbo, c)
        return bool(np.array_equal(bbo, out_host[s_][k * kb:(k + 1) * kb]))
    with ThreadPoolExecutor(max_workers=min(32, os.cpu_count() or 1)) as ex:
        res = list(ex.map(one, picks))
    n_odd_checked = sum(1 for (s_, k) in picks if not good[s_, k])
    # the decoder ALONE on this very job's LLRs (frames that decode: the half-row decoder's speculative layers end after two passes, its chain layers skip their walk;
    # `kernel_ms_alone` of the roofline object is taken on noise that never converges -- their slow case)
    import torch
    nf_job = int(job['nf'])
    hard = torch.empty((nf_job, kb), dtype=torch.uint8, device=run.out[0].device)
    tri = torch.empty((nf_job,), dtype=torch.int32, device=run.out[0].device)
    alone_ms = None
    if job['force']:
        def go():
            eng._check(eng.lib.dvbs2gpu_ldpc_decode_batch(eng.h, job['rate'], job['short'], C.c_void_p(job['d_llr']), nf_job, job['max_trials'], 1, hard.data_ptr(), None, tri.data_ptr(), eng._stream()))
        go(); torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); go(); e1.record(); torch.cuda.synchronize()
        alone_ms = round(e0.elapsed_time(e1), 3)
    return {'frames_checked': len(picks), 'frames_equal_to_oracle_fec': int(sum(res)), 'of_which_not_transmitted_frames': n_odd_checked,
            'streams_spanned': [min(p_[0] for p_ in picks), max(p_[0] for p_ in picks)],
            'decoder_ms_alone_on_this_jobs_llrs': alone_ms, 'frames_of_the_job': nf_job,
            'how': 'LLRs of the last timed step read back from the decoder job\'s buffer, CPU oracle FEC (orc_fec_decode_frame, %d %s iterations), byte equality with the delivered BBFRAMEs'
                   % (job['max_trials'], 'forced' if job['force'] else 'max')}


def ldpc_alone(eng, info, rate, short, nfr, dev, iters=ITERS):
    """the decoder alone at the batch size of one step: forced mode and the normal mode on noise that never converges"""
    import torch
    llr = torch.randint(-40, 41, (nfr, info['ldpc_n']), dtype=torch.int8, device=dev)
    hard = torch.empty((nfr, info['ldpc_k'] // 8), dtype=torch.uint8, device=dev)
    tri = torch.empty((nfr,), dtype=torch.int32, device=dev)
    res = {}
    for name, force in (('forced', 1), ('normal', 0)):
        def go():
            eng._check(eng.lib.dvbs2gpu_ldpc_decode_batch(eng.h, rate, short, llr.data_ptr(), nfr, iters, force, hard.data_ptr(), None, tri.data_ptr(), eng._stream()))
        go()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        go()
        e1.record()
        torch.cuda.synchronize()
        res[name] = e0.elapsed_time(e1)
        res[name + '_all_ran'] = bool(((tri == -1) | (tri == iters)).all().item())
    return res


def cpu_info():
    model, phys = None, None
    try:
        cores = set()
        phys_id = core_id = None
        for line in open('/proc/cpuinfo'):
            if line.startswith('model name') and model is None:
                model = line.split(':', 1)[1].strip()
            elif line.startswith('physical id'):
                phys_id = line.split(':', 1)[1].strip()
            elif line.startswith('core id'):
                core_id = line.split(':', 1)[1].strip()
                cores.add((phys_id, core_id))
        phys = len(cores) or None
    except OSError:
        pass
    return model, phys


def cpu_baseline(block_iq, budget_s=12.0):
    """CPU path on this box's host cores.  FEC: the reference's own code (oracle/_ref) the way its library was designed to be used --
    a PERSISTENT decoder object per thread (tables built once), 16 frames in the 16 int8 SSE4.1 lanes of one call, 50 iterations on
    noise LLRs (never converges: the sweeps of the forced GPU run plus the reference's syndrome check before every iteration), then
    per frame the hard-decision repack, BCH and descrambler.  Without oracle/_ref: the oracle's scalar port.  Front end: the oracle
    restatement (the reference's float blocks need SDR++/VOLK, not buildable here).  Both legs run on all logical CPUs; the per-symbol
    times add."""
    import ctypes as C
    import orc
    p = orc.fec_params(RATE, SHORT)
    sym_per_frame = orc.modcod_params(MODCOD, SHORT, PILOTS)['plframe']
    ncpu = os.cpu_count() or 1
    model, phys = cpu_info()
    R = orc.ref()
    rng = np.random.default_rng(1)

    def run_threads(fn, seconds):
        counts = [0] * ncpu
        stop = time.time() + seconds

        def worker(i):
            while time.time() < stop:
                counts[i] += fn(i)
        t0 = time.time()
        th = [threading.Thread(target=worker, args=(i,)) for i in range(ncpu)]
        [t.start() for t in th]
        [t.join() for t in th]
        return sum(counts), time.time() - t0

    flags = None
    if R is not None and hasattr(R, 'ref_fec16_create'):
        kind = 'reference'
        flags = R.ref_build_flags().decode()
        lanes = np.ascontiguousarray(rng.integers(-40, 41, size=(p['N'], 16)).astype(np.int8))
        objs = [C.c_void_p(R.ref_fec16_create(RATE, SHORT)) for _ in range(ncpu)]

        def fec(i):
            R.ref_fec16_run(objs[i], lanes.ctypes.data, ITERS, None, 0)
            return 16
    else:
        kind = 'port'
        noise = rng.integers(-40, 41, size=(p['N'],)).astype(np.int8)

        def fec(i):
            bb = np.zeros(p['kbch'] // 8, np.uint8)
            c = np.zeros(1, np.int32)
            x = noise.copy()
            orc.lib().orc_fec_decode_frame(RATE, SHORT, x, ITERS, 1, bb, c)
            return 1
    nfec, tfec = run_threads(fec, budget_s * 0.6)
    fec_frames_per_s = nfec / tfec
    # ---- front-end leg (oracle; FEC skipped with force_ldpc_iters = -1)
    rxs = [orc.OracleRx(orc.default_cfg(MODCOD, SHORT, PILOTS, force_ldpc_iters=-1)) for _ in range(ncpu)]

    def fe(i):
        rxs[i].process(block_iq)
        return block_iq.size // 2
    nsym, tfe = run_threads(fe, budget_s * 0.4)
    fe_sym_per_s = nsym / tfe
    t_per_sym = 1.0 / fe_sym_per_s + 1.0 / (fec_frames_per_s * sym_per_frame)
    # kind: what the FEC leg ran (the ~97 % of the CPU time); the front-end leg is always the oracle restatement (SDR++ / VOLK are not available: unbuildable here)
    out = dict(value=round(1e-6 / t_per_sym, 4), unit='Msymbols/s', cores=ncpu, kind=kind, kind_fec=kind, kind_frontend='port', cpu_model=model, physical_cores=phys, logical_cpus=ncpu,
               compiler_flags=flags or 'oracle: g++ -std=c++17 -O3 -ffp-contract=off',
               sample='%d threads (one per logical CPU): FEC leg %d frames in %.1f s (%s LDPC 50 it + repack + BCH + descramble, persistent decoder '
                      'objects = %.3f Msym/s), front-end leg %d symbols in %.1f s (oracle AGC..demap = %.3f Msym/s); per-symbol times added'
                      % (ncpu, nfec, tfec, 'reference 16-lane SSE4.1' if kind == 'reference' else 'oracle scalar',
                         fec_frames_per_s * sym_per_frame / 1e6, nsym, tfe, fe_sym_per_s / 1e6),
               fec_only_msym_s=round(fec_frames_per_s * sym_per_frame / 1e6, 4), frontend_only_msym_s=round(fe_sym_per_s / 1e6, 4))
    if R is not None:
        # as-wired variant: one frame per decode call, single thread (bbframe_ldpc.cpp:123-139)
        b = rng.integers(-40, 41, size=(p['N'],)).astype(np.int8)
        t1 = time.time()
        n1 = 0
        while time.time() - t1 < 1.5:
            x = b.copy()
            R.ref_ldpc_decode(RATE, SHORT, x, ITERS)
            n1 += 1
        out['fec_as_wired_1thread_msym_s'] = round(n1 * sym_per_frame / (time.time() - t1) / 1e6, 4)
    return out


# ------------------------------------------------------------------------------------------------ secondary configurations
def secondary_s2(eng, pkg, dev, name, modcod, rate, short, pilots, esn0_db, S, F, steps, iters=ITERS, force=True):
    import torch
    run = S2Run(eng, pkg, dev, modcod, short, pilots, esn0_db, S, F, DISTINCT, seed=50 + modcod, iters=iters, force=force)

    def barrier():
        torch.cuda.synchronize()
    # untimed steps first: the pipelined mode's balancer (wave-priority share of the timing loop, stage pipeline on / off; the FEC partition stream) starts from zero for every new
    # configuration (s2_demod.hip) and moves one notch per two consistent calls: a front-end-bound configuration needs these steps to reach ITS setting -- 8 where the decoder
    # is the critical path (the setting stays near zero), 20 in the plugin's mode (seven notches + the partition rule: 16 calls; a receiver runs for hours)
    dt, stages, acc, _ = time_steps(run, steps, 8 if force else 20, barrier, True)
    k = ldpc_alone(eng, run.info, rate, short, S * F, dev)
    bpf = ITERS * 4 * run.info['ldpc_edges'] + run.info['ldpc_n'] + run.info['kbch'] // 8
    if not force:
        # the plugin's own mode (main.cpp:65: 16 trials, layered_decoder.hh:127: `while (bad() && --trials >= 0)`): the decoder's work depends on the
        # channel, so the decoder-alone figures (50 forced iterations on noise) do not belong to this line
        run.close()
        torch.cuda.empty_cache()
        return {'config': name, 'value': round(S * F * steps * run.sym / dt / 1e6, 1), 'unit': 'Msymbols/s', 'ms_per_step': round(dt / steps * 1e3, 2),
                'steps': steps, 'untimed_steps': 8 if force else 20, 'streams': S, 'frames_per_stream_per_step': F, 'esn0_db': esn0_db, 'max_ldpc_trials': iters, 'early_exit': True,
                'frames_delivered': acc['delivered'], 'frames_equal_to_transmitted': acc['equal'], 'balancer_final_state': acc['balancer'],
                'stage_ms_per_step': {name: round(v[0] / steps, 2) for name, v in stages.items()}}
    out = {'config': name, 'value': round(S * F * steps * run.sym / dt / 1e6, 1), 'unit': 'Msymbols/s', 'ms_per_step': round(dt / steps * 1e3, 2),
           'steps': steps, 'untimed_steps': 8 if force else 20, 'streams': S, 'frames_per_stream_per_step': F, 'esn0_db': esn0_db, 'frames_delivered': acc['delivered'],
           'frames_equal_to_transmitted': acc['equal'], 'balancer_final_state': acc['balancer'], 'stage_ms_per_step': {name: round(v[0] / steps, 2) for name, v in stages.items()},
           'ldpc_kernel_ms_alone': round(k['forced'], 3),
           'ldpc_nominal_hbm_frac': round(bpf * S * F / (k['forced'] * 1e-3) / 1e9 / HBM_PEAK_GBS, 4)}
    run.close()
    torch.cuda.empty_cache()
    return out


def secondary_dvbs(eng, pkg, dev):
    """BASELINE config D / 1: DVB-S QPSK 1/2, IQ -> TS PACKETS (DVBSDemod::process, module_dvbs_demod.cpp:78-117: QPSK_ALT front end, soft
    slicer, self-locking Viterbi, TS deframer, Forney de-interleaver, RS(204,188), energy dispersal).  GPU: a bank of 4096 carriers and ONE
    carrier, receiver bank + tail bank, a continuous signal in calls of 65 536 symbols; CPU (config 1): the oracle restatement of the same
    chain on one thread (kind "port": SDR++ / VOLK are not available; the tail stages are pinned against the reference's own sources)."""
    import torch
    import orc_dvbs as od
    import orc_dvbs_tail as ot
    npk, chunk_sym = 320, 65536
    obits, ts = ot.dvbs_outer_tx(npk, seed=5)
    enc = od.cc_encode(obits)
    nsym = enc.size // 2
    iq = np.zeros(2 * nsym, np.complex64)
    od.LF().orc_dvbs_modulate(od.P(np.ascontiguousarray(enc)), nsym, 12.0, 1e-3, 0.3, 0.2, 7, od.P(iq))
    sent = {bytes(p) for p in ts}
    ncalls = nsym // chunk_sym
    out = {'config': 'D / 1: DVB-S QPSK 1/2, 2 sps, IQ -> TS packets (receiver bank dvbs2gpu_dvbs_demod_* + tail bank dvbs2gpu_dvbs_tail_*), continuous signal of %d symbols in calls of %d, the first two calls (acquisition) untimed' % (ncalls * chunk_sym, chunk_sym)}
    d_iq = torch.from_numpy(iq).to(dev)
    for S in [int(x) for x in os.environ.get('DVBS2GPU_BENCH_DVBS_BANKS', '4096,1').split(',')]:          # (development aid: one of the two alone)
        bank = pkg.DvbsDemodBank(eng, S, max_samples=2 * chunk_sym)
        tail = pkg.DvbsTailBank(eng, S, max_bits=chunk_sym + 4 * 8192)
        bits = torch.zeros((S, 2 * chunk_sym + 4 * 8192), dtype=torch.uint8, device=dev)
        tso = torch.zeros((S, (chunk_sym // 1632 + 3) * 8 * 188), dtype=torch.uint8, device=dev)
        tbits, tts = [bits[i] for i in range(S)], [tso[i] for i in range(S)]
        got, hit = 0, 0

        def call(c, check):
            nonlocal got, hit
            part = d_iq[2 * c * chunk_sym:2 * (c + 1) * chunk_sym]
            nb = bank.process_batch([part for _ in range(S)], tbits)
            nts = tail.process_batch([tbits[i][:nb[i]] for i in range(S)], tts)
            if check:
                for i in (0, S - 1):
                    pk = tso[i, :nts[i]].cpu().numpy().reshape(-1, 188)
                    got += len(pk); hit += sum(bytes(x) in sent for x in pk)
        ACQ = 2                              # acquisition outside the timed calls: the loops settle in call 0, the Viterbi decoder's lock search (IDLE: 2 phases x 26
        for c in range(ACQ):                 # rate / shift hypotheses per block, ~17 ms for one carrier) runs on the first blocks of call 1; from call 2 on the receiver tracks
            call(c, False)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for c in range(ACQ, ncalls):
            call(c, False)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        bank.reset(); tail.reset()
        for c in range(ncalls):              # the same signal once more, untimed, with the TS packets of two carriers checked
            call(c, True)
        st = bank.stats()[0]
        out['bank_%d_msym_s' % S] = round(S * (ncalls - ACQ) * chunk_sym / dt / 1e6, 2)
        out['bank_%d_locked' % S] = bool(st.state == 1 and st.rate == 0)
        out['bank_%d_ts_packets_checked' % S] = got
        out['bank_%d_ts_packets_equal_to_transmitted' % S] = hit
        bank.close(); tail.close()
        del bits, tso
        torch.cuda.empty_cache()
    # CPU (config 1): the whole chain of the oracle, one stream, one thread, bounded sample
    from orc_dvbs_tail import OracleTail
    rx, o = od.OracleQpskAlt(), od.L()
    sl, vit, otail = od.VP(o.orc_dvbs_slicer_create()), od.OracleViterbi(), OracleTail()
    t0 = time.perf_counter()
    done = pk_cpu = hit_cpu = 0
    for c in range(ncalls):
        sy = np.ascontiguousarray(rx.process(iq[2 * c * chunk_sym:2 * (c + 1) * chunk_sym]))
        soft = np.zeros(2 * sy.size + 8192, np.int8)
        n = o.orc_dvbs_slicer_process(sl, sy.size, od.P(sy), od.P(soft))
        bl = []
        if n:
            eb, en, es = vit.work(soft[:n].reshape(-1, 8192))
            bl = [eb[b, :en[b]] for b in range(len(en))]
        tsb, nf = otail.process(np.concatenate(bl) if bl else np.zeros(0, np.uint8))
        pk = tsb.reshape(-1, 188)
        pk_cpu += len(pk); hit_cpu += sum(bytes(x) in sent for x in pk)
        done += chunk_sym
        if time.perf_counter() - t0 > 6.0:
            break
    out['cpu_config1_msym_s'] = round(done / (time.perf_counter() - t0) / 1e6, 3)
    out['cpu_config1_ts_packets'] = [pk_cpu, hit_cpu]
    out['cpu_config1_note'] = 'BASELINE config 1: oracle restatement of DVBSDemod::process, IQ -> TS packets, ONE stream on ONE host thread (kind "port"); [packets delivered, equal to transmitted ones]'
    return out


def small_batch(eng, pkg, dev, S=64, F=1):
    """latency of a small synchronous call (per-stream ceiling): `S` transponders x `F` PLFRAME(s) of 8PSK 3/4, early-exit LDPC;
    where the call's time goes (per-stage device times) and what the host adds on top (call time - sum of the stages)"""
    import torch
    run = S2Run(eng, pkg, dev, MODCOD, SHORT, PILOTS, 14.0, S, F, min(S, 16), seed=77, iters=16, force=False)
    eng.set_pipelined(False)
    for _ in range(PREROLL_FRAMES // F):
        run.step()
    torch.cuda.synchronize()
    reps = 10
    # the call time with the per-stage event pairs OFF (a small call is ~100 launches: the events around every stage cost it 10 %), then the
    # same calls once more with them on for the stage times
    eng.set_stage_timing(False)
    t0 = time.perf_counter()
    for _ in range(reps):
        nb = run.step()
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) / reps
    eng.set_stage_timing(True)
    eng.stage_times()
    for _ in range(reps):
        nb = run.step()
    torch.cuda.synchronize()
    st = eng.stage_times()
    acc = run.check(nb)
    run.close()
    return {'config': 'small batch: %d transponders x %d PLFRAME per call, 8PSK 3/4 normal, synchronous mode, LDPC with early exit' % (S, F),
            'ms_per_call': round(dt * 1e3, 3), 'msym_s_total': round(S * F * run.sym / dt / 1e6, 2), 'msym_s_per_stream': round(F * run.sym / dt / 1e6, 3),
            'stage_ms_per_call': {k: round(v[0] / reps, 3) for k, v in st.items()},
            'stage_note': 'per-stage device times overlap (the stages of a call run pipelined on several HIP streams): they do not add up to ms_per_call; ms_per_call is measured with the stage timers off, the stage times in a second pass with them on',
            'frames_delivered': acc['delivered'], 'frames_equal_to_transmitted': acc['equal']}


def dropin_calls(eng, pkg, dev, nsamples, seconds=2.0):
    """THE DROP-IN CALL: DVBS2Demod::process as SDR++ drives it (module_dvbs2_demod.h:66-76: whatever one VFO buffer holds, a few thousand samples) --
    dvbs2gpu_demod_process with HOST buffers, ONE stream, `nsamples` complex samples per call (2 sps): host -> device copy of the samples, every stage's
    launches, the read-back of the BBFRAMEs, the synchronisation.  8PSK 3/4 normal frames, the plugin's decoder mode (16 trials, early exit), synchronous.
    A continuous periodic signal is fed call after call; the first calls (loop acquisition) are untimed."""
    import torch
    iq, bb = make_block(MODCOD, SHORT, PILOTS, 8, 4242, 14.0)
    sent = {bytes(x) for x in bb}
    cfg = eng.default_cfg(MODCOD, bool(SHORT), bool(PILOTS), max_ldpc_trials=16)
    dm = eng.demod(cfg, max_samples=max(nsamples, 8192))
    eng.set_pipelined(False)
    eng.set_stage_timing(False)
    sig = np.concatenate([iq, iq[:nsamples]])           # (the block is periodic: a call that runs over its end continues at its start)
    pos = 0

    def call():
        nonlocal pos
        out = dm.process(sig[pos:pos + nsamples])
        pos = (pos + nsamples) % iq.size
        return out
    for _ in range(max(8, 4 * iq.size // nsamples)):       # acquisition + at least four blocks' worth of settled calls
        call()
    torch.cuda.synchronize()
    l0 = eng.get_state('kernel_launches')
    t0 = time.perf_counter()
    ncalls = nfr = nok = 0
    lat = []
    while time.perf_counter() - t0 < seconds or ncalls < 16:
        t1 = time.perf_counter()
        frames = call()
        lat.append(time.perf_counter() - t1)
        ncalls += 1
        nfr += len(frames); nok += sum(bytes(f) in sent for f in frames)
    dt = time.perf_counter() - t0
    launches = (eng.get_state('kernel_launches') - l0) / ncalls
    eng.set_stage_timing(True)
    dm.close()
    lat = np.sort(np.asarray(lat))
    return {'config': 'drop-in call: dvbs2gpu_demod_process, host buffers, ONE stream, %d samples per call (= %d symbols), 8PSK 3/4 normal, synchronous, 16 LDPC trials with early exit' % (nsamples, nsamples // 2),
            'ms_per_call': round(dt / ncalls * 1e3, 4), 'ms_per_call_median': round(float(lat[len(lat) // 2]) * 1e3, 4), 'ms_per_call_p99': round(float(lat[min(len(lat) - 1, int(0.99 * len(lat)))]) * 1e3, 4),
            'msym_s': round(ncalls * (nsamples // 2) / dt / 1e6, 4), 'kernel_launches_per_call': round(launches, 1), 'calls_timed': ncalls,
            'real_time_symbol_rate_this_call_size_sustains_msym_s': round((nsamples // 2) / (dt / ncalls) / 1e6, 4),
            'frames_delivered': nfr, 'frames_equal_to_transmitted': nok}


def secondary_vcm(eng, pkg, dev, S=64, frames_per_call=8, calls=10, distinct=4):
    """ACM/VCM in the throughput mode: `S` streams whose PLFRAMEs cycle over QPSK / 8PSK / 16APSK / 32APSK MODCODs, normal and short
    frames, with and without pilots, and a dummy PLFRAME (the reference only REPORTS the PLS code, dvbs2_plhdr_demod.cpp:43-64, and its GUI reconfigures:
    main.cpp:375-408; here the framing follows every frame's code).  Continuous signals fed in calls of ~`frames_per_call` cycles' worth of samples, 16 LDPC
    trials with early exit, one FEC job per LDPC code present in a call, collected by the next call."""
    import torch
    import orc
    pls = [(4 << 2) | 2, (14 << 2) | 2, (6 << 2) | 2 | 1, 0, (19 << 2) | 2, (27 << 2) | 2 | 1, 13 << 2, (12 << 2) | 2]
    nfr = len(pls) * frames_per_call * (calls + 3) // 8 * 8 // len(pls) * len(pls)
    sigs, sent = [], []
    for b in range(distinct):
        iq, bbs = orc.transmit_vcm(pls, nfr, seed=4000 + b, esn0_db=30.0, cfo=1e-4, timing=0.2, phase0=0.3, lead_symbols=500 + 1000 * b)
        sigs.append(torch.from_numpy(iq).to(dev))
        sent.append({bytes(x) for x in bbs if x is not None})
    nsym_total = (sigs[0].numel() // 2)
    chunk = (min(x.numel() for x in sigs) // (calls + 2)) & ~1
    cfg = eng.default_cfg(4, True, False, acm_vcm=1, max_ldpc_trials=16)
    dms = [eng.demod(cfg, max_samples=chunk) for _ in range(S)]
    cap = chunk // 2 + 100000
    out = torch.zeros((S, cap), dtype=torch.uint8, device=dev)
    tout = [out[i] for i in range(S)]
    eng.set_pipelined(True)
    try:
        def call(c):
            return eng.process_batch(dms, [sigs[i % distinct][c * chunk:(c + 1) * chunk] for i in range(S)], tout)
        call(0); call(1)                                    # acquisition outside the timed calls
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        nb = None
        for c in range(2, calls + 2):
            nb = call(c)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        # the frames the last timed call delivered, streams 0 and S - 1, against the transmitted BBFRAMEs (sizes from the per-frame stats)
        got = hit = 0
        for i in (0, S - 1):
            buf, pos = out[i, :nb[i]].cpu().numpy(), 0
            for st in dms[i].stats():
                if st.bbframe_bytes:
                    got += 1; hit += bytes(buf[pos:pos + st.bbframe_bytes]) in sent[i % distinct]
                    pos += st.bbframe_bytes
        eng.process_batch(dms, [torch.empty(0, dtype=torch.complex64, device=dev) for _ in dms], tout)
    finally:
        eng.set_pipelined(False)
        for d in dms:
            d.close()
    return {'config': 'ACM/VCM, throughput mode: %d streams, PLFRAMEs cycling over PLS codes %s (QPSK..32APSK, normal + short, +- pilots, a dummy PLFRAME), Es/N0 30 dB, carrier offset 1e-4 rad/sample (the reference PLL loses the 16APSK / 32APSK frames of such a cycle from ~2e-4 on), '
                      '16 LDPC trials with early exit, calls of %d samples per stream' % (S, pls, chunk),
            'value': round(S * calls * (chunk // 2) / dt / 1e6, 2), 'unit': 'Msymbols/s', 'ms_per_call': round(dt / calls * 1e3, 2), 'streams': S,
            'msym_s_per_stream': round(calls * (chunk // 2) / dt / 1e6, 3), 'frames_checked_last_call': got, 'frames_equal_to_transmitted': hit}


# ------------------------------------------------------------------------------------------------ config 4: 64 mixed transponders
MIXED_MODCODS = [4, 6, 7, 11, 12, 13, 14, 15]
MIXED_ESN0 = {4: 8.0, 6: 10.0, 7: 11.0, 11: 14.0, 12: 12.0, 13: 13.0, 14: 14.0, 15: 16.0}
MIXED_RATE = {4: 3, 6: 5, 7: 6, 11: 10, 12: 4, 13: 5, 14: 6, 15: 8}


def mixed64(eng, pkg, dev, dd, steps, warmup, nt=64, sub=64, F=1):
    """BASELINE config 4: `nt` table entries cycling over 8 QPSK / 8PSK MODCODs (normal frames, 50 forced iterations).  sub = 1: the config as it
    is named, 64 transponders = 64 streams.  sub > 1 (the GPU-sized variant): every entry stands for `sub` INDEPENDENT carriers of its MODCOD
    (nt x sub = 4096 continuous streams, each with its own loop state from step to step).  They are NOT sections of one fast transponder:
    cutting one carrier into concurrently processed segments costs a warm-up prefix per segment and a de-duplication of the frames at the
    seams (csrc/segrx.hip has that receiver; 8 warm-up frames per 10 own frames in its tests), which this line does not pay and does not
    claim.  STRONG scaling: the entry list is fixed and sharded
    over the ranks (MODCOD-grouped, weighted); rank 0 owns table + configuration and broadcasts them; after every step the BBFRAMEs
    and per-frame statistics are gathered to the egress rank 0, which reassembles them in transponder order and checks every frame."""
    import torch
    table = cfg = None
    if dd.rank == 0:
        table = []
        for t in range(nt):
            m = MIXED_MODCODS[t % len(MIXED_MODCODS)]
            info = pkg.modcod_info(m, False, False)
            table.append(dict(id=t, modcod=m, seed=900 + t, esn0_db=MIXED_ESN0[m], kb=info['kbch'] // 8, sym=info['plframe_symbols'],
                              weight=float(info['ldpc_edges']) * ITERS + 40.0 * info['plframe_symbols']))
        cfg = dict(sub=sub, frames=F, iters=ITERS, cfo=CFO, ppm=PPM)
    table = dd.broadcast_object(table)
    cfg = dd.broadcast_object(cfg)
    assign = pkg_distribute(pkg).assign_transponders(table, dd.world)
    mine = assign[dd.rank]
    kbmax = max(t['kb'] for t in table)
    cap = cfg['frames'] + 2
    # local streams: transponder-major, `sub` sub-streams each
    demods, tin, ids, kbs, syms, sent = [], [], [], [], [], []
    iq_keep = []
    for t in mine:
        e = table[t]
        iq, bb = make_block(e['modcod'], 0, 0, cfg['frames'], e['seed'], e['esn0_db'], cfg['cfo'], cfg['ppm'])
        d_iq = torch.from_numpy(iq).to(dev)
        c = eng.default_cfg(e['modcod'], False, False, force_ldpc_iters=cfg['iters'])
        for k in range(cfg['sub']):
            x = torch.roll(d_iq, 2 * (k * 7919 % (iq.size // 2)))
            iq_keep.append(x)
            demods.append(eng.demod(c, max_samples=iq.size))
            tin.append(x)
            ids.append(t * cfg['sub'] + k)
            kbs.append(e['kb']); syms.append(e['sym'])
        sent.append({bytes(x) for x in bb})
    nloc = len(demods)
    out = torch.zeros((max(nloc, 1), cap * kbmax), dtype=torch.uint8, device=dev)
    tout = [out[i] for i in range(nloc)]
    n_units = nt * cfg['sub']
    total_sym_per_step = sum(t['sym'] for t in table) * cfg['sub'] * cfg['frames']

    run_step = eng.prepare_batch(demods, tin, tout) if nloc else None

    def step():
        nb = run_step() if nloc else []
        # per-frame statistics of the step (LDPC trials, BCH corrections) travel with the frames
        res = dd.gather_units(ids, out[:nloc], torch.as_tensor(np.asarray(nb), dtype=torch.int32, device=dev), n_units)
        return nb, res

    def barrier():
        torch.cuda.synchronize()
        dd.barrier()
        torch.cuda.synchronize()

    eng.set_pipelined(True)
    for _ in range(PREROLL_FRAMES // cfg['frames'] + 2):
        step()
    for _ in range(warmup):
        step()
    barrier()
    t0 = time.perf_counter()
    for _ in range(steps):
        nb, (g_out, g_cnt) = step()
    torch.cuda.synchronize()
    t_steps_done = time.perf_counter()
    barrier()
    dt_local = time.perf_counter() - t0
    dt = dd.max_over_ranks(dt_local)
    # per-rank time of the timed steps WITHOUT the closing barrier's wait is what shows an uneven assignment: time to the last local step's return
    dt_ranks = dd.all_over_ranks(t_steps_done - t0)
    # egress check: every unit's frames are transmitted frames of ITS transponder (input order restored by the gather)
    bad = delivered = 0
    digest = None
    if dd.rank == dd.egress:
        import hashlib
        host = g_out.cpu().numpy()
        cnt = g_cnt.cpu().numpy()
        h = hashlib.sha256()
        for u in range(n_units):          # what the egress rank holds after the last step, in transponder order: equal for every number of ranks
            h.update(np.int32(cnt[u]).tobytes()); h.update(host[u, :cnt[u]].tobytes())
        digest = h.hexdigest()
        all_sent = {}
        for t in range(nt):
            e = table[t]
            _, bb = make_block(e['modcod'], 0, 0, cfg['frames'], e['seed'], e['esn0_db'], cfg['cfo'], cfg['ppm']) if t not in mine else (None, None)
            all_sent[t] = {bytes(x) for x in bb} if bb is not None else sent[mine.index(t)]
        for u in range(n_units):
            t = u // cfg['sub']
            kb = table[t]['kb']
            fr = host[u, :cnt[u]].reshape(-1, kb)
            delivered += len(fr)
            bad += sum(bytes(x) not in all_sent[t] for x in fr)
    if nloc:
        eng.process_batch(demods, [torch.empty(0, dtype=torch.complex64, device=dev) for _ in demods], tout)
    eng.set_pipelined(False)
    for d in demods:
        d.close()
    what = ('4 as named: %d transponders (one stream each), MODCODs %s cycled' % (nt, MIXED_MODCODS) if cfg['sub'] == 1 else
            '4, GPU-sized: %d independent carriers in %d MODCOD groups (%d table entries with MODCODs %s cycled, each standing for %d independent carriers of its MODCOD -- '
            'not sections of one transponder: no warm-up / de-duplication cost is paid or claimed)'
            % (nt * cfg['sub'], len(MIXED_MODCODS), nt, MIXED_MODCODS, cfg['sub']))
    res = {'config': what + ', normal frames, %d PLFRAME(s) per stream per step, 50 forced LDPC iterations' % cfg['frames'],
           'value': round(total_sym_per_step * steps / dt / 1e6, 1), 'unit': 'Msymbols/s', 'scaling': 'strong', 'n_gpus': dd.world,
           'ms_per_step': round(dt / steps * 1e3, 2), 'steps': steps, 'warmup': warmup, 'transponders_per_rank': [len(a) for a in assign],
           'load_per_rank_rel_to_average': [round(sum(table[i]['weight'] for i in a) * dd.world / sum(t['weight'] for t in table), 3) for a in assign],
           'ms_per_step_per_rank': [round(x / steps * 1e3, 2) for x in dt_ranks],
           'ms_per_step_rank_max_min': [round(max(dt_ranks) / steps * 1e3, 2), round(min(dt_ranks) / steps * 1e3, 2)],
           'modcods_per_rank': [sorted({table[i]['modcod'] for i in a}) for a in assign],
           'collectives': 'broadcast of table + configuration from rank 0; per step a gather of BBFRAMEs + byte counts to the egress rank 0 (in the timed region)',
           'frames_at_egress_last_step': delivered, 'frames_not_transmitted_ones': bad, 'egress_sha256': digest}
    return res


def pkg_distribute(pkg):
    import importlib
    return importlib.import_module(pkg.__name__ + '.distribute')


# ------------------------------------------------------------------------------------------------ main
def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--gpus', type=int, default=int(os.environ.get('WORLD_SIZE', '1')), help='ranks = GPUs of this node (default: WORLD_SIZE when a launcher set it, else 1)')
    ap.add_argument('--steps', type=int, default=40, help='timed steps (the timed region is bracketed by full synchronisations, so it holds one pipeline fill + drain: K calls cost about K + 1 step times)')
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--config', default='headline', choices=['headline', 'mixed64'])
    ap.add_argument('--streams', type=int, default=4096, help='transponder streams per GPU')
    ap.add_argument('--frames', type=int, default=8, help='PLFRAMEs per stream per step')
    ap.add_argument('--distinct', type=int, default=DISTINCT, help='distinct signal blocks (every stream gets a private, shifted copy)')
    ap.add_argument('--mixed-frames', type=int, default=4, help='config mixed64: PLFRAMEs per stream per step')
    ap.add_argument('--mixed-sub', type=int, default=64, help='config mixed64: independent carriers per table entry (1 = BASELINE config 4 as named: 64 streams)')
    ap.add_argument('--workload', default='', help='development aid: MODCOD,short,pilots,Es/N0,rate instead of the headline workload (e.g. 27,1,1,20,9 = the config 5 stand-in); the line then is NOT the headline')
    ap.add_argument('--plugin-mode', action='store_true', help='development aid: the main run with max_ldpc_trials 16 and early exit (the plugin\'s mode) instead of 50 forced iterations; the line then is NOT the headline')
    ap.add_argument('--no-cpu-baseline', action='store_true')
    ap.add_argument('--no-secondary', action='store_true', help='skip configs 2, 5, D and the mixed-MODCOD batch')
    ap.add_argument('--no-pipeline', action='store_true', help='run the FEC inside the call that produced the frames (no overlap with the next front end)')
    ap.add_argument('--full', action='store_true', help='besides the headline: frame check, decoder self-check, roofline, CPU baseline, secondary configs, config 4 lines '
                    '(--no-cpu-baseline / --no-secondary leave parts of it out)')
    ap.add_argument('--dump-outputs', metavar='DIR', help='write what the last timed headline step delivered as DIR/<name>.npy (rank 0; see last_step_outputs)')
    args = ap.parse_args()
    if args.dump_outputs and args.config != 'headline':
        ap.error('--dump-outputs: only the headline configuration')

    if args.gpus > 1 and 'WORLD_SIZE' not in os.environ:
        # `python bench.py --gpus N` on its own: start N ranks (one per GPU) as CHILD processes of this one, which has not touched the
        # GPU (nothing imported torch or the library yet; a process that has must never exec), and pass their exit code on
        import socket
        import subprocess
        with socket.socket() as so:
            so.bind(('127.0.0.1', 0))
            port = so.getsockname()[1]
        cmd = [sys.executable, '-m', 'torch.distributed.run', '--nnodes=1', '--nproc-per-node', str(args.gpus), '--master-addr', '127.0.0.1',
               '--master-port', str(port), os.path.abspath(__file__)] + sys.argv[1:]
        sys.exit(subprocess.call(cmd))

    import torch
    import __graft_entry__ as g
    pkg = g.load_package()

    rank = int(os.environ.get('RANK', '0'))
    local_rank = int(os.environ.get('LOCAL_RANK', '0'))
    world = int(os.environ.get('WORLD_SIZE', '1'))
    if world != args.gpus:
        raise SystemExit('bench.py: --gpus %d but WORLD_SIZE=%d (launch one rank per GPU, or run `python bench.py --gpus N` and let it start them)' % (args.gpus, world))
    dist = None
    backend = 'nccl'
    if world > 1:
        import torch.distributed as dist
        os.environ.setdefault('MASTER_ADDR', '127.0.0.1')
        # DVBS2GPU_BENCH_BACKEND=gloo: development aid to exercise the multi-rank path on a box with fewer GPUs than ranks
        backend = os.environ.get('DVBS2GPU_BENCH_BACKEND', 'nccl')
        if backend == 'nccl':
            torch.cuda.set_device(local_rank)
            dist.init_process_group('nccl', device_id=torch.device('cuda', local_rank))
        else:
            local_rank = local_rank % torch.cuda.device_count()
            torch.cuda.set_device(local_rank)
            dist.init_process_group(backend)
    else:
        local_rank = 0
        torch.cuda.set_device(0)
    dev = torch.device('cuda', local_rank)
    eng = pkg.Engine(local_rank)
    eng.set_stage_timing(True)
    dd = pkg_distribute(pkg).Distributor(dist, dev if backend == 'nccl' else 'cpu')

    def barrier():
        torch.cuda.synchronize()
        if dist is not None:
            dist.barrier()
        torch.cuda.synchronize()

    if args.config == 'mixed64':
        res = mixed64(eng, pkg, dev, dd, args.steps, args.warmup, sub=args.mixed_sub, F=args.mixed_frames)
        if rank == 0:
            line = {'metric': 'Msymbols/s demod+FEC, 64 mixed-MODCOD DVB-S2 transponders @50 LDPC iters (BASELINE config 4)', 'value': res['value'],
                    'unit': 'Msymbols/s', 'n_gpus': world, 'steps': args.steps, 'warmup': args.warmup, 'ms_per_step': res['ms_per_step'],
                    'higher_is_better': True, 'scaling': 'strong', 'vs_baseline': None, 'dtype': 'int8 (FEC) / f32 (demod)', 'data': 'synthetic',
                    'config': {'workload': res['config']}, 'mixed64': res}
            print(json.dumps(line))
        if dist is not None:
            dist.barrier()
            dist.destroy_process_group()
        eng.close()
        return

    S, F = args.streams, args.frames
    pipelined = not args.no_pipeline
    global MODCOD, SHORT, PILOTS, ESN0_DB, RATE, WORKLOAD
    if args.workload:
        w = args.workload.split(',')
        MODCOD, SHORT, PILOTS, ESN0_DB, RATE = int(w[0]), int(w[1]), int(w[2]), float(w[3]), int(w[4])
        WORKLOAD = 'development run, NOT the headline: MODCOD %d short %d pilots %d at %.1f dB' % (MODCOD, SHORT, PILOTS, ESN0_DB)
    if args.plugin_mode:
        WORKLOAD = 'development run, NOT the headline: ' + WORKLOAD + ' -- in the plugin\'s mode (16 trials, early exit)'
    t_start = time.perf_counter()
    run = S2Run(eng, pkg, dev, MODCOD, SHORT, PILOTS, ESN0_DB, S, F, args.distinct, seed=rank, **(dict(iters=16, force=False) if args.plugin_mode else {}))
    t_setup = time.perf_counter() - t_start
    dt, stages, acc, outputs = time_steps(run, args.steps, args.warmup, barrier, pipelined, prove_decoder=args.full and pipelined and rank == 0,
                                          full=args.full, dump=bool(args.dump_outputs) and rank == 0)
    dt = dd.max_over_ranks(dt)
    if outputs is not None:
        dump_outputs(args.dump_outputs, outputs)
    info, sym = run.info, run.sym
    block0 = run.blocks_host[0]
    iq_bytes = int(S) * run.nsamp * 8
    run.close()
    torch.cuda.empty_cache()

    value = world * S * F * args.steps * sym / dt / 1e6
    head = {
        'metric': 'Msymbols/s demod+FEC, DVB-S2 8PSK 3/4 normal-frame @50 LDPC iters',
        'value': round(value, 3), 'unit': 'Msymbols/s', 'n_gpus': world, 'steps': args.steps, 'warmup': args.warmup,
        'ms_per_step': round(dt / args.steps * 1e3, 4), 'higher_is_better': True, 'scaling': 'weak', 'vs_baseline': None,
        'dtype': 'int8 (FEC) / f32 (demod)', 'data': 'synthetic',
        'config': {'workload': WORKLOAD,
                   'streams_per_gpu': S, 'frames_per_stream_per_step': F, 'symbols_per_frame': sym, 'distinct_signal_blocks': min(args.distinct, S),
                   'private_iq_copy_per_stream_bytes_total': iq_bytes,
                   'parallelism': 'independent transponder streams sharded over GPUs, no data-path collective',
                   'fec_pipelined_across_steps': pipelined,
                   'setup_seconds_before_first_step': round(t_setup, 1),
                   'ranks_seen_by_backend': (dist.get_world_size() if dist is not None else 1), 'backend': (backend if dist is not None else 'none')},
        'stage_ms_per_step': {name: round(v[0] / args.steps, 3) for name, v in stages.items()},
    }
    if not args.full:
        if rank == 0:
            print(json.dumps(head))
        if dist is not None:
            dist.barrier()
            dist.destroy_process_group()
        eng.close()
        return

    nfr = S * F
    k = ldpc_alone(eng, info, RATE, SHORT, nfr, dev)
    bytes_per_frame = ITERS * 4 * info['ldpc_edges'] + info['ldpc_n'] + info['kbch'] // 8
    plan = eng.ldpc_plan_info(RATE, bool(SHORT))
    form = eng.ldpc_decoder_form(RATE, bool(SHORT))
    plan['decoder'] = ('lane per row, two frames per workgroup', 'wave per frame', 'half a row per lane, one frame per workgroup')[form]
    # the decoder's launches as they ran INSIDE the timed steps (hipEvent pairs on the FEC stream, dvbs2gpu_get_stage_times)
    l_ms, l_n, l_frames = stages['ldpc']
    in_step_ms = l_ms / max(l_n, 1)
    in_step_frames = l_frames / max(l_n, 1)
    achieved = bytes_per_frame * in_step_frames / (in_step_ms * 1e-3) / 1e9 if l_n else None
    achieved_alone = bytes_per_frame * nfr / (k['forced'] * 1e-3) / 1e9
    # PMC figures need rocprofv3 passes of their own (tools/profile_run.sh): the newest committed set is quoted, with a flag when the decoder
    # sources have changed since it was taken
    traffic, traffic_note, issue, wcf, traffic_current = None, None, None, None, None
    import glob
    cands = sorted(glob.glob(os.path.join(ROOT, 'profiles', 'r*_ldpc_traffic.json')))
    if cands:
        tj = json.load(open(cands[-1]))
        traffic = tj.get('traffic_bytes_per_frame', 0) * in_step_frames or None     # (measured on a 4096-frame launch; the kernel's traffic is per frame)
        traffic_note = tj.get('source')
        issue = tj.get('valu_per_simd_cycle', tj.get('valu_issue_fraction'))
        wcf = tj.get('wave_cycles_fraction')
        traffic_current = tj.get('kernel_source_sha16') == ldpc_source_hash()

    if rank == 0:
        line = {
            **head,
            # the same workload with the reference's check cadence (LDPCDecoder::operator(), layered_decoder.hh:121-133: bad() before EVERY iteration; the headline's forced mode
            # evaluates it once): `value` scaled by the decoder's own forced / normal time on input that never converges (all 50 iterations run), measured alone in this run
            'value_normal_mode': (round(value / (1.0 + (in_step_ms * l_n / (dt * 1e3)) * (k['normal'] / k['forced'] - 1.0)), 3) if k['normal_all_ran'] and l_n else None),
            'config': {**head['config'],
                       'frames_delivered_checked': acc['delivered'], 'frames_equal_to_transmitted': acc['equal'],
                       'fraction_equal_to_transmitted': round(acc['equal'] / max(acc['delivered'], 1), 5),
                       'frames_out_of_sequence': acc['out_of_order'],
                       'check': 'every delivered frame of every stream, last timed step + pipeline flush, on the device (hash + full byte compare)',
                       'decoder_self_check': acc['decoder_self_check'],
                       # where the pipelined mode's run-time balancer stood after the last timed step (s2_demod.hip: priority share of the timing loop 0..8, stage pipeline,
                       # decoder jobs on the 128-unit partition stream): two runs compare only at the same setting
                       'balancer_final_state': acc['balancer']},
            'roofline': {'bound': 'hbm',
                         'bound_note': 'NOMINAL: algorithmic bytes against the 8 TB/s HBM peak, as the contract asks for a byte / integer path -- the state is on-chip and what bounds the kernel is vector issue -- its instructions are packed 16-bit / DPP / byte-permute forms, which a SIMD issues at HALF rate (valu_note) -- plus what the layers with shared bits cost beyond a plain row update (profiles/r06_ldpc_split_layers.txt); the layers with shared bits are SPECULATIVE since round 6: their time depends on how far the frame has converged (kernel_ms_alone: noise; kernel_ms_alone_on_the_steps_llrs: the step\'s own frames), their result does not',
                         'kernel': ('ldpc_split_kernel<%d>' % plan['max_deg']) if form == 2 else 'ldpc_decode_kernel<%d,%d,%s>' % (plan['max_deg'], plan['rec_dwords'], 'true' if plan.get('irregular') else 'false'),
                         'achieved': round(achieved if achieved else achieved_alone, 1), 'peak': HBM_PEAK_GBS, 'unit': 'GB/s',
                         'frac': round((achieved if achieved else achieved_alone) / HBM_PEAK_GBS, 4),
                         'timing': 'average over the %d decoder launches inside the timed steps (hipEvent pairs on the FEC stream; the front end of the next step shares the CUs)' % l_n,
                         'kernel_ms_in_step': round(in_step_ms, 4), 'frames_per_launch': int(in_step_frames),
                         # alone, on NOISE that never converges (the slow case of the half-row decoder's speculative layers: 4-8 passes, every chain walked) ...
                         'kernel_ms_alone': round(k['forced'], 4), 'achieved_alone': round(achieved_alone, 1), 'frac_alone': round(achieved_alone / HBM_PEAK_GBS, 4),
                         # ... and alone on the very LLRs the last timed step decoded (frames that decode: two passes, no walks) -- the decoder's time depends on its data, its result does not
                         'kernel_ms_alone_on_the_steps_llrs': (acc['decoder_self_check'] or {}).get('decoder_ms_alone_on_this_jobs_llrs'),
                         'frac_alone_on_the_steps_llrs': (round(bytes_per_frame * (acc['decoder_self_check'] or {}).get('frames_of_the_job', 0) / ((acc['decoder_self_check'] or {}).get('decoder_ms_alone_on_this_jobs_llrs') * 1e-3) / 1e9 / HBM_PEAK_GBS, 4)
                                                          if (acc['decoder_self_check'] or {}).get('decoder_ms_alone_on_this_jobs_llrs') else None),
                         'kernel_ms_alone_normal_mode_same_iterations': round(k['normal'], 4) if k['normal_all_ran'] else None,
                         'traffic': traffic, 'traffic_taken_from_this_build': traffic_current, 'traffic_unit': 'bytes per launch (fabric-side FETCH_SIZE x2 + WRITE_SIZE, per frame x frames of the launch)', 'traffic_source': traffic_note,
                         'valu_per_simd_cycle': issue, 'valu_note': 'wave64 VALU instructions per SIMD and clock over the launch (PMC).  They are packed 16-bit / VOP3 / SDWA / DPP forms almost throughout, which a SIMD issues every 4.3 cycles (plain 32-bit VOP2: 2.3; tools/ubench/valu_tput.hip, profiles/r05_valu_rates.txt): x 4 = the share of the launch the vector ALUs are busy',
                         'wave_cycles_fraction': wcf,
                         'algorithmic_bytes_per_frame': bytes_per_frame, 'algorithmic_bytes_per_launch': int(bytes_per_frame * in_step_frames),
                         'ldpc_share_of_step': round(in_step_ms * l_n / (dt * 1e3), 3),
                         'syndrome_check': 'forced mode (the headline): evaluated once, after the last iteration; normal mode: before every iteration, as in the reference (bit-vector form, see DESIGN.md)',
                         'note': 'posteriors stay in LDS; the message records (132 MB live) bounce through the Infinity Cache, whose hits the fabric-side counters include',
                         'plan': plan},
        }
        if world == 1 and not args.no_cpu_baseline:
            cb = cpu_baseline(block0)
            line['cpu_baseline'] = cb
            # the GPU line against the CPU legs of the same run: `vs_cpu_baseline` uses the combined figure (FEC leg = the reference's own SSE4.1 code, front-end leg = the
            # unoptimised scalar oracle port, which halves it); `vs_fec_only` is the conservative ratio, against the reference's FEC code alone
            line['vs_cpu_baseline'] = round(value / cb['value'], 1) if cb.get('value') else None
            line['vs_fec_only'] = round(value / cb['fec_only_msym_s'], 1) if cb.get('fec_only_msym_s') else None
        if world == 1 and not args.no_secondary:
            sec = []
            try:
                # the small synchronous calls first: a small bank is a set of latency chains of a handful of waves, and late in this run -- after minutes of the
                # full-load configurations -- the same calls take ~10 % longer (1 x 4: 28.5 instead of 25.2 ms; 24 hardware queues change nothing: clocks?)
                sec.append(small_batch(eng, pkg, dev, 64, 1))
                sec.append(small_batch(eng, pkg, dev, 1, 4))
                for ns in (8192, 65536):
                    sec.append(dropin_calls(eng, pkg, dev, ns))
                sec.append(secondary_s2(eng, pkg, dev, 'headline workload in the PLUGIN\'s mode: 8PSK 3/4 normal FECFRAME, Es/N0 %.0f dB, max_ldpc_trials 16 with early exit '
                                        '(reference src/main.cpp:65, layered_decoder.hh:127), syndrome check before every iteration' % ESN0_DB, MODCOD, RATE, SHORT, PILOTS, ESN0_DB,
                                        S, F, 20, iters=16, force=False))
                sec.append(secondary_s2(eng, pkg, dev, '2: DVB-S2 QPSK 1/2 normal FECFRAME (MODCOD 4), same channel conditions, Es/N0 8 dB', 4, 3, 0, 0, 8.0, 4096, 4, 16))
                sec.append(secondary_s2(eng, pkg, dev, '5 stand-in: DVB-S2 32APSK 8/9 SHORT FECFRAME + pilots (MODCOD 27; 9/10 short does not exist), Es/N0 20 dB', 27, 9, 1, 1, 20.0, 2048, 16, 16))
                sec.append(secondary_dvbs(eng, pkg, dev))
                sec.append(secondary_vcm(eng, pkg, dev))
            except Exception as e:          # a secondary line must not take the headline down
                sec.append({'error': repr(e)})
            line['secondary'] = sec
    if not args.no_secondary:
        # BASELINE config 4 runs on every world size (strong scaling; at N = 1 it is the one-GPU number)
        # (an engine of their own for the mixed-batch lines when DVBS2GPU_BENCH_FRESH_ENGINE=1: development aid -- do the streams the earlier lines created cost these their hardware queues?)
        if os.environ.get('DVBS2GPU_BENCH_FRESH_ENGINE') == '1':
            eng.close()
            torch.cuda.empty_cache()
            eng = pkg.Engine(local_rank)
        try:
            m64 = mixed64(eng, pkg, dev, dd, 20, 2, F=args.mixed_frames)
        except Exception as e:
            m64 = {'error': repr(e)}
        if rank == 0:
            line['mixed64'] = m64
        # ... and BASELINE config 4 as it is named: 64 transponders, one stream each (4 PLFRAMEs per transponder and step)
        # (measured in either order: the GPU-sized variant loses 4 % behind this one, this one gains nothing in front)
        try:
            m64l = mixed64(eng, pkg, dev, dd, 20, 2, sub=1, F=4)
        except Exception as e:
            m64l = {'error': repr(e)}
        if rank == 0:
            line['config4_64_transponders'] = m64l
    if rank == 0:
        print(json.dumps(line))
    if dist is not None:
        dist.barrier()
        dist.destroy_process_group()
    eng.close()


if __name__ == '__main__':
    main()
