// Host side of the DVB-S receive path: mirror of dsp::dvbs::DVBSDemod (module_dvbs_demod.cpp:9-117) from the input samples up to
// and including vit.process -- demod::QPSK_ALT (a17), DVBSymToSoftBlock (a18), Viterbi_DVBS (a19) -- for a BANK of independent
// streams.  The TS deframer, Forney de-interleaver call, Reed-Solomon and energy dispersal that follow in the reference are the
// next rows; the de-interleaver kernel itself is exposed separately (dvbs2gpu_forney_*).
#include "ctx.h"
#include "../../include/dvbs2gpu_math.h"
#include <cmath>
#include <algorithm>

using namespace s2;

struct dvbs2gpu_dvbs_demod {
    dvbs2gpu_ctx* ctx = nullptr;
    dvbs2gpu_dvbs_cfg cfg{};
    DvbsLoopCoefs co{};
    int nstreams = 0, max_samples = 0, max_blocks = 0;
    size_t sym_cap = 0, soft_cap = 0;
    DevBuf<DvbsStreamState> d_state;
    DevBuf<cf32> d_buf_a;           // [nstreams][max_samples]
    DevBuf<cf32> d_buf_b;
    DevBuf<cf32> d_sym;             // [nstreams][sym_cap]
    DevBuf<int8_t> d_soft;          // [nstreams][soft_cap]
    DevBuf<cf32> d_in;              // staging for the host entry point (stream 0)
    DevBuf<uint8_t> d_out;
    DevBuf<uint8_t> d_ts;           // TS staging of dvbs2gpu_dvbs_process_ts
    size_t ts_cap = 0;
    DevBuf<DvbsVitState> d_vstate;
    DevBuf<uint8_t> d_vws;
    DevBuf<cf32> d_bandedge;
    float* d_rrc = nullptr;         // the context's table (get_rrc)
    std::vector<DvbsStreamState> init_state;
    int quality = 0;                // dvbs2gpu_dvbs_demod_set_quality
    DevBuf<DvbsQuality> d_qual;     // [nstreams], allocated on first use
    std::vector<DvbsQuality> qual;  // of the last call (empty: it ran with quality off)
};

namespace {

std::vector<cf32> make_bandedge(const dvbs2gpu_dvbs_cfg& c) {   // FLL::createBandedgeFilters, fll.cpp:61-95 (sym/samp rate are ints there)
    const int T = c.rrc_taps;
    const float PI_F = 3.14159265358979323846f;
    float sps = (float)((double)(int)c.samplerate / (double)(int)c.symbolrate);
    const int M = (int)(T / sps);
    float power = 0;
    std::vector<float> bb(T);
    auto sinc = [](double x) { return x == 0.0 ? 1.0 : sin(x) / x; };
    for (int i = 0; i < T; i++) {
        float k = -M + i * 2.0f / sps;
        float tap = (float)(sinc(c.rrc_alpha * k - 0.5f) + sinc(c.rrc_alpha * k + 0.5f));
        power += tap;
        bb[i] = tap;
    }
    std::vector<cf32> out(2 * T);
    int N = (int)((T - 1.0f) / 2.0f);
    for (int i = 0; i < T; i++) {
        float tap = bb[i] / power;
        float k = (-N + (int)i) / (2.0f * sps);
        float a1 = -2.0f * PI_F * (1.0f + c.rrc_alpha) * k, a2 = 2.0f * PI_F * (1.0f + c.rrc_alpha) * k;
        float s1, c1, s2, c2;   // the engine's own sin/cos (include/dvbs2gpu_math.h), like the oracle's tap builder
        dvbs2m::sincosf_det(a1, &s1, &c1);
        dvbs2m::sincosf_det(a2, &s2, &c2);
        out[T - i - 1] = cf32{c1 * tap, s1 * tap};
        out[T + T - i - 1] = cf32{c2 * tap, s2 * tap};
    }
    return out;
}

int vit_reset(dvbs2gpu_dvbs_demod* d) {
    std::vector<DvbsVitState> init(d->nstreams);
    memset(init.data(), 0, sizeof(DvbsVitState) * d->nstreams);
    for (auto& s : init) { s.ber = 10; s.dep_buf[0] = s.dep_buf[1] = 128; }
    HIP_TRY(hipMemcpy(d->d_vstate, init.data(), sizeof(DvbsVitState) * d->nstreams, hipMemcpyHostToDevice));
    HIP_TRY(hipMemset(d->d_vws, 0, (size_t)DVBS_VIT_WS_BYTES * d->nstreams));
    return 0;
}

}  // namespace

extern "C" {

void dvbs2gpu_dvbs_demod_default_cfg(dvbs2gpu_dvbs_cfg* c) {   // main.cpp:64-73,134-139
    if (!c) return;
    memset(c, 0, sizeof(*c));
    c->symbolrate = 2e6; c->samplerate = 4e6;
    c->agc_rate = 0.0001f; c->rrc_alpha = 0.35f; c->rrc_taps = 65; c->loop_bw = 0.00628f; c->fll_bw = 0.006f;
    float bw = 0.00628f, damp = 0.707f;
    float den = (1.0f + 2.0 * damp * bw + bw * bw);
    c->clock_mu_gain = (4.0f * damp * bw) / den;
    c->clock_omega_gain = (4.0f * bw * bw) / den;
    c->omega_rel_limit = 0.02f;
    c->viterbi_ber_threshold = 0.15f; c->viterbi_max_outsync = 20;   // module_dvbs_demod.cpp:23
}

int dvbs2gpu_dvbs_demod_create(dvbs2gpu_ctx* ctx, const dvbs2gpu_dvbs_cfg* cfg, int nstreams, int max_samples, dvbs2gpu_dvbs_demod** out) {
    if (!ctx || !cfg || !out || nstreams <= 0 || max_samples <= 0) return DVBS2GPU_ERR_ARG;
    // what a configuration may be: rx_cfg_rules.h.  The timing loop writes one symbol per a >= a_min = omega (1 - omega_rel_limit) - |clock_mu_gain| input
    // samples: the symbol / soft buffers are sized from that bound, and the kernel stages at most FD_TILE/2 + 72 symbols per 256-sample tile
    {
        const char* why = rxcfg::dvbs_loop_refusal(cfg->samplerate, cfg->symbolrate, cfg->rrc_taps, cfg->omega_rel_limit, cfg->clock_mu_gain, cfg->clock_omega_gain,
                                                   cfg->agc_rate, cfg->loop_bw, cfg->fll_bw);
        if (!why) why = rxcfg::rrc_refusal(cfg->rrc_taps, cfg->rrc_alpha, cfg->samplerate, cfg->symbolrate);
        if (why) { last_error() = why; return DVBS2GPU_ERR_ARG; }
    }
    HIP_TRY(hipSetDevice(ctx->device));
    std::unique_ptr<dvbs2gpu_dvbs_demod> d(new dvbs2gpu_dvbs_demod());
    d->ctx = ctx; d->cfg = *cfg; d->nstreams = nstreams; d->max_samples = max_samples;
    d->sym_cap = rxcfg::dvbs_sym_cap(max_samples, rxcfg::dvbs_a_min(cfg->samplerate / cfg->symbolrate, cfg->omega_rel_limit, cfg->clock_mu_gain));
    d->soft_cap = (size_t)2 * d->sym_cap + 2 * DVBS_SOFT_BLOCK + 128;
    d->max_blocks = (int)(d->soft_cap / DVBS_SOFT_BLOCK);
    const float PI_F = 3.14159265358979323846f;
    DvbsLoopCoefs& co = d->co;
    co.agc_rate = cfg->agc_rate;
    float a;
    critically_damped(cfg->fll_bw, &a, &co.fll_beta);
    co.fll_min_freq = -PI_F / 2.0f; co.fll_max_freq = PI_F / 2.0f;
    const float omega = (float)(cfg->samplerate / cfg->symbolrate);
    co.fd_alpha = cfg->clock_mu_gain; co.fd_beta = cfg->clock_omega_gain;
    co.fd_min_freq = (float)(omega * (1.0 - cfg->omega_rel_limit)); co.fd_max_freq = (float)(omega * (1.0 + cfg->omega_rel_limit));
    critically_damped(cfg->loop_bw, &co.cos_alpha, &co.cos_beta);
    co.cos_min_freq = -PI_F / 10.0f; co.cos_max_freq = PI_F / 10.0f;
    co.ntaps = cfg->rrc_taps;
    DvbsStreamState s0;
    memset(&s0, 0, sizeof(s0));
    s0.agc_gain = 1.0f; s0.fd_freq = omega;
    d->init_state.assign(nstreams, s0);
    {
        std::lock_guard<std::mutex> l(ctx->mtx);
        if (!ctx->d_fd_bank) RC_TRY(upload(make_polyphase_bank(FD_PHASES, FD_TAPS), ctx->d_fd_bank));
    }
    RC_TRY(upload(make_bandedge(*cfg), d->d_bandedge));
    RC_TRY(get_rrc(ctx, cfg->rrc_taps, cfg->rrc_alpha, cfg->samplerate / cfg->symbolrate, &d->d_rrc));
    const char* what = "hipMalloc(dvbs demod)";
    const size_t n = (size_t)nstreams;
    RC_TRY(d->d_state.alloc(n, false, what));
    RC_TRY(d->d_buf_a.alloc((size_t)max_samples * n, false, what));
    RC_TRY(d->d_buf_b.alloc((size_t)max_samples * n, false, what));
    RC_TRY(d->d_sym.alloc(d->sym_cap * n, false, what));
    RC_TRY(d->d_soft.alloc(d->soft_cap * n, false, what));
    RC_TRY(d->d_vstate.alloc(n, false, what));
    RC_TRY(d->d_vws.alloc((size_t)DVBS_VIT_WS_BYTES * n, false, what));
    RC_TRY(dvbs2gpu_dvbs_demod_reset(d.get()));
    *out = d.release();
    return 0;
}

int dvbs2gpu_dvbs_demod_reset(dvbs2gpu_dvbs_demod* d) {
    if (!d) return DVBS2GPU_ERR_ARG;
    HIP_TRY(hipSetDevice(d->ctx->device));
    HIP_TRY(hipMemcpy(d->d_state, d->init_state.data(), sizeof(DvbsStreamState) * d->nstreams, hipMemcpyHostToDevice));
    return vit_reset(d);
}

void dvbs2gpu_dvbs_demod_destroy(dvbs2gpu_dvbs_demod* d) { delete d; }


int dvbs2gpu_dvbs_demod_process_batch(dvbs2gpu_dvbs_demod* d, const float* const* d_iq, const int* counts, uint8_t* const* d_bits, int cap,
                                      int* out_counts) {
    if (!d || !d_iq || !counts || !d_bits || !out_counts || cap < 0) return DVBS2GPU_ERR_ARG;
    dvbs2gpu_ctx* ctx = d->ctx;
    CallGuard guard(ctx);                       // ws_dvbs[] are context-wide
    HIP_TRY(hipSetDevice(ctx->device));
    hipStream_t st = nullptr;
    const int n = d->nstreams;
    std::vector<DvbsStreamWork> work(n);
    int max_count = 0;
    for (int i = 0; i < n; ++i) {
        if (counts[i] < 0 || counts[i] > d->max_samples) { last_error() = "count exceeds max_samples"; return DVBS2GPU_ERR_ARG; }
        if (counts[i] > 0 && !d_iq[i]) return DVBS2GPU_ERR_ARG;
        work[i].in = (const cf32*)d_iq[i]; work[i].count = counts[i];
        work[i].buf_a = d->d_buf_a + (size_t)i * d->max_samples; work[i].buf_b = d->d_buf_b + (size_t)i * d->max_samples;
        work[i].sym = d->d_sym + (size_t)i * d->sym_cap; work[i].soft = d->d_soft + (size_t)i * d->soft_cap; work[i].st = d->d_state + i;
        max_count = std::max(max_count, counts[i]);
    }
    const int mb = d->max_blocks;
    Workspace& ws = ctx->ws_dvbs[0];
    ScratchLayout L;
    const auto l_work = L.add<DvbsStreamWork>(n); const auto l_ptr_in = L.add<const int8_t*>(n); const auto l_ptr_out = L.add<uint8_t*>(n);
    const auto l_nblk = L.add<int>(n); const auto l_cnt = L.add<int>(n); const auto l_blk0 = L.add<int>(n); const auto l_nbits = L.add<int>((size_t)n * mb);
    int rc;
    if ((rc = ws.ensure(L.bytes()))) return rc;
    Workspace& wsb = ctx->ws_dvbs[1];
    if ((rc = wsb.ensure((size_t)n * mb * DVBS_SOFT_BLOCK))) return rc;
    DvbsStreamWork* d_work = l_work(ws.p);
    const int8_t** d_ptr_in = l_ptr_in(ws.p); uint8_t** d_ptr_out = l_ptr_out(ws.p);
    std::vector<const int8_t*> pin(n);
    for (int i = 0; i < n; ++i) pin[i] = work[i].soft;
    HIP_TRY(hipMemcpyAsync(d_work, work.data(), sizeof(DvbsStreamWork) * n, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(d_ptr_in, pin.data(), sizeof(void*) * n, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(d_ptr_out, d_bits, sizeof(void*) * n, hipMemcpyHostToDevice, st));
    int *d_nblk = l_nblk(ws.p), *d_cnt = l_cnt(ws.p), *d_nbits = l_nbits(ws.p), *d_blk0 = l_blk0(ws.p);
    // The serial stages time-sliced over their own streams (s2_rx_kernels.hip, dvbs_frontend_launch): AGC, FLL + RRC, timing recovery, and --
    // behind every timing-recovery slice -- the slice's Costas loop, soft FIFO append and the Viterbi decoding of the blocks it completed.
    // One carrier then costs its slowest stage instead of the sum; a bank of thousands gains too (4096 carriers: 206 -> 146 ms per call),
    // because its lane-per-stream and four-streams-per-wave stages (AGC, Costas, FLL) are latency chains that leave the SIMDs to the
    // wave-per-stream ones (timing recovery, Viterbi, RRC).
    const int nsub = ctx->dvbs_fe_slices;
    dvbs2gpu_ctx::FeAux* fa = nullptr;
    if (nsub > 1) {
        std::lock_guard<std::mutex> l(ctx->mtx);
        fa = &ctx->fe_aux[st];
        if (!fa->dvbs_aux[0]) {
            for (int a = 0; a < (ctx->dvbs_agc_stream ? 3 : 2); ++a) HIP_TRY(hipStreamCreateWithFlags(&fa->dvbs_aux[a], hipStreamNonBlocking));
            for (int a = 0; a < 4; ++a)
                for (int i = 0; i <= DVBS_FE_MAX_SLICES; ++i) HIP_TRY(hipEventCreateWithFlags(&fa->dvbs_ev[a][i], hipEventDisableTiming));
        }
    }
    struct Hook : DvbsSliceHook {
        dvbs2gpu_dvbs_demod* d; dvbs2gpu_ctx::FeAux* fa; const DvbsStreamWork* d_work; const int8_t* const* d_in_ptrs; int n, max_count, nsub, mb;
        int* d_blk0; int* d_nblk; int* d_nbits; uint8_t* d_bits; hipStream_t st;
        hipError_t after_timing(int c) override {
            hipStream_t sv = fa->dvbs_aux[0];        // a bank: behind the AGC slices, which were all enqueued before the first timing-recovery slice
            hipError_t e;
            if ((e = hipEventRecord(fa->dvbs_ev[3][c], st)) != hipSuccess) return e;
            if ((e = hipStreamWaitEvent(sv, fa->dvbs_ev[3][c], 0)) != hipSuccess) return e;
            // (alternating the Costas slices between `st` and `sv`, which carry about the same load without them, was slower: every hand-over
            // between two streams costs tens of microseconds and ties the two chains together)
            if ((e = dvbs_costas_launch(d_work, n, d->co, c, nsub, sv)) != hipSuccess) return e;
            if ((e = dvbs_soft_slice_launch(d_work, n, max_count, c, nsub, d_blk0, d_nblk, sv)) != hipSuccess) return e;
            return dvbs_viterbi_launch(nullptr, d_in_ptrs, d_nblk, n, mb, d_bits, d_nbits, nullptr, d->d_vstate, d->d_vws, d->cfg.viterbi_ber_threshold,
                                       d->cfg.viterbi_max_outsync, sv, d_blk0);
        }
    } hook;
    hook.d = d; hook.fa = fa; hook.d_work = d_work; hook.d_in_ptrs = d_ptr_in; hook.n = n; hook.max_count = max_count;
    hook.nsub = nsub; hook.mb = mb; hook.d_blk0 = d_blk0; hook.d_nblk = d_nblk; hook.d_nbits = d_nbits; hook.d_bits = (uint8_t*)wsb.p; hook.st = st;
    // (tried: the Costas slices on the AGC's stream and the decoder alone on `sv` -- AGC + Costas then carry 0.94 ms per slice beside the FLL's 0.81: nothing gained)
    // (a few carriers: the AGC slices on a stream of their own -- one carrier 39.4 -> 36.7 ms per call; a bank keeps them ahead on the Viterbi stream)
    hipStream_t aux3[3] = {fa ? fa->dvbs_aux[0] : nullptr, fa ? fa->dvbs_aux[1] : nullptr, fa && n < ctx->dvbs_bank_min ? fa->dvbs_aux[2] : nullptr};
    HIP_TRY(dvbs_frontend_launch(d_work, n, max_count, d->co, d->d_bandedge, d->d_rrc, ctx->d_fd_bank, st, fa ? aux3 : nullptr,
                                 fa ? fa->dvbs_ev : nullptr, nsub, fa ? &hook : nullptr, ctx->dvbs_bank_min));
    if (fa) {
        // the last slice's decoder run ends the Viterbi stream's work for this call
        HIP_TRY(hipEventRecord(fa->dvbs_ev[3][DVBS_FE_MAX_SLICES], fa->dvbs_aux[0]));
        HIP_TRY(hipStreamWaitEvent(st, fa->dvbs_ev[3][DVBS_FE_MAX_SLICES], 0));
        HIP_TRY(dvbs_soft_count_launch(d_work, n, d_nblk, st));          // (FIFO fill and block count of the whole call, for the packing and the compaction)
    } else {
        HIP_TRY(dvbs_soft_count_launch(d_work, n, d_nblk, st));
        HIP_TRY(dvbs_viterbi_launch(nullptr, d_ptr_in, d_nblk, n, mb, (uint8_t*)wsb.p, d_nbits, nullptr, d->d_vstate,
                                    d->d_vws, d->cfg.viterbi_ber_threshold, d->cfg.viterbi_max_outsync, st));
    }
    HIP_TRY(dvbs_pack_bits_launch((const uint8_t*)wsb.p, d_nbits, d_nblk, n, mb, d_ptr_out, cap, d_cnt, st));
    HIP_TRY(dvbs_soft_compact_launch(d_work, n, st));
    // signal quality over the call's Costas output (quality.hip): one launch for the bank, behind the last Costas slice
    d->qual.clear();
    if (d->quality) {
        if (!d->d_qual) RC_TRY(d->d_qual.alloc(n, false, "hipMalloc(dvbs demod quality)"));
        d->qual.resize(n);
        HIP_TRY(dvbs_quality_launch(d_work, n, d->d_qual, st));
        HIP_TRY(hipMemcpyAsync(d->qual.data(), d->d_qual, sizeof(DvbsQuality) * n, hipMemcpyDeviceToHost, st));
    }
    HIP_TRY(hipMemcpyAsync(out_counts, d_cnt, sizeof(int) * n, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    return 0;
}

int dvbs2gpu_dvbs_demod_process(dvbs2gpu_dvbs_demod* d, int count, const float* h_iq, uint8_t* h_bits, int cap) {
    if (!d || d->nstreams != 1 || count < 0 || cap < 0 || (count > 0 && !h_iq) || (cap > 0 && !h_bits)) return DVBS2GPU_ERR_ARG;
    if (count > d->max_samples) { last_error() = "count exceeds max_samples"; return DVBS2GPU_ERR_ARG; }
    HIP_TRY(hipSetDevice(d->ctx->device));
    if (!d->d_in) RC_TRY(d->d_in.alloc((size_t)d->max_samples, false, "hipMalloc(dvbs demod staging)"));
    const size_t ocap = (size_t)d->max_blocks * DVBS_SOFT_BLOCK;
    if (!d->d_out) RC_TRY(d->d_out.alloc(ocap, false, "hipMalloc(dvbs demod staging)"));
    if (count) HIP_TRY(hipMemcpy(d->d_in, h_iq, sizeof(cf32) * (size_t)count, hipMemcpyHostToDevice));
    const float* pi = (const float*)d->d_in.get();
    uint8_t* po = d->d_out;
    int nb = 0;
    const int c2 = (int)std::min<size_t>((size_t)cap, ocap);
    int rc = dvbs2gpu_dvbs_demod_process_batch(d, &pi, &count, &po, c2, &nb);
    if (rc) return rc;
    if (nb) HIP_TRY(hipMemcpy(h_bits, d->d_out, (size_t)nb, hipMemcpyDeviceToHost));
    return nb;
}

// The whole of DVBSDemod::process (module_dvbs_demod.cpp:78-99) on host buffers: samples in, TS packets out; the decoded bits stay in HBM
int dvbs2gpu_dvbs_process_ts(dvbs2gpu_dvbs_demod* d, dvbs2gpu_dvbs_tail* t, int count, const float* h_iq, uint8_t* h_ts, int cap) {
    if (!d || !t || d->nstreams != 1 || count < 0 || cap < 0 || (count > 0 && !h_iq) || (cap > 0 && !h_ts)) return DVBS2GPU_ERR_ARG;
    if (count > d->max_samples) { last_error() = "count exceeds max_samples"; return DVBS2GPU_ERR_ARG; }
    HIP_TRY(hipSetDevice(d->ctx->device));
    if (!d->d_in) RC_TRY(d->d_in.alloc((size_t)d->max_samples, false, "hipMalloc(dvbs demod staging)"));
    const size_t ocap = (size_t)d->max_blocks * DVBS_SOFT_BLOCK;
    if (!d->d_out) RC_TRY(d->d_out.alloc(ocap, false, "hipMalloc(dvbs demod staging)"));
    if (!d->d_ts) {
        d->ts_cap = (ocap / 13056 + 2) * 8 * 188;                 // a deframer frame (8 packets) per 13056 bits, plus the carried ones
        RC_TRY(d->d_ts.alloc(d->ts_cap, false, "hipMalloc(dvbs demod staging)"));
    }
    if (count) HIP_TRY(hipMemcpy(d->d_in, h_iq, sizeof(cf32) * (size_t)count, hipMemcpyHostToDevice));
    const float* pi = (const float*)d->d_in.get();
    uint8_t* po = d->d_out;
    int nb = 0;
    int rc = dvbs2gpu_dvbs_demod_process_batch(d, &pi, &count, &po, (int)ocap, &nb);
    if (rc) return rc;
    const uint8_t* pb = d->d_out;
    uint8_t* pt = d->d_ts;
    int nbytes = 0;
    if ((rc = dvbs2gpu_dvbs_tail_process_batch(t, &pb, &nb, &pt, (int)std::min<size_t>(d->ts_cap, (size_t)cap), &nbytes, nullptr))) return rc;
    if (nbytes) HIP_TRY(hipMemcpy(h_ts, d->d_ts, (size_t)nbytes, hipMemcpyDeviceToHost));
    return nbytes;
}

int dvbs2gpu_dvbs_demod_get_stats(dvbs2gpu_dvbs_demod* d, dvbs2gpu_viterbi_stats* h_out) {
    if (!d || !h_out) return DVBS2GPU_ERR_ARG;
    HIP_TRY(hipSetDevice(d->ctx->device));
    std::vector<DvbsVitState> v(d->nstreams);
    HIP_TRY(hipMemcpy(v.data(), d->d_vstate, sizeof(DvbsVitState) * d->nstreams, hipMemcpyDeviceToHost));
    for (int i = 0; i < d->nstreams; ++i) {
        h_out[i].ber = v[i].ber; h_out[i].state = v[i].state; h_out[i].rate = v[i].rate; h_out[i].phase = v[i].phase; h_out[i].shift = v[i].shift;
    }
    return d->nstreams;
}

int dvbs2gpu_dvbs_demod_set_quality(dvbs2gpu_dvbs_demod* d, int on) {
    if (!d) return DVBS2GPU_ERR_ARG;
    CallGuard guard(d->ctx);
    d->quality = on ? 1 : 0;
    return 0;
}

int dvbs2gpu_dvbs_demod_get_quality(dvbs2gpu_dvbs_demod* d, dvbs2gpu_dvbs_quality* h_out) {
    if (!d) return DVBS2GPU_ERR_ARG;
    static_assert(sizeof(dvbs2gpu_dvbs_quality) == sizeof(DvbsQuality), "quality record layout");
    if (h_out && !d->qual.empty()) memcpy(h_out, d->qual.data(), sizeof(DvbsQuality) * d->qual.size());
    return (int)d->qual.size();
}

int dvbs2gpu_dvbs_demod_get_tap(dvbs2gpu_dvbs_demod* d, int stream, int which, void* h_dst, int cap) {
    if (!d || stream < 0 || stream >= d->nstreams || which < 0 || which > 1) return DVBS2GPU_ERR_ARG;
    HIP_TRY(hipSetDevice(d->ctx->device));
    DvbsStreamState s;
    HIP_TRY(hipMemcpy(&s, d->d_state + stream, sizeof(s), hipMemcpyDeviceToHost));
    if (which == 1) {   // loop state: agc gain, fll phase/freq, fd phase/freq/offset, costas phase/freq
        float v[8] = {s.agc_gain, s.fll_phase, s.fll_freq, s.fd_phase, s.fd_freq, (float)s.fd_offset, s.costas_phase, s.costas_freq};
        if (h_dst && cap >= 8) memcpy(h_dst, v, sizeof(v));
        return 8;
    }
    const int n = s.n_sym;
    if (h_dst && cap > 0) HIP_TRY(hipMemcpy(h_dst, d->d_sym + (size_t)stream * d->sym_cap, sizeof(cf32) * (size_t)std::min(n, cap), hipMemcpyDeviceToHost));
    return n;
}

}  // extern "C"
