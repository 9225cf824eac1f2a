// BBFRAME -> MPEG-TS / GSE parser bank: what the reference's sink handler runs on the demodulator's
// output (main.cpp:532-558 -> dsp::dvbs2::BBFrameTSParser::work, dvbs2/bbframe_ts_parser.cpp:104-390), for `nstreams`
// independent streams whose BBFRAMEs are already resident in HBM (they are the FEC's output).
//
// MPEG-TS frames (TS/GS = 11) never leave the device:
//   bbts_plan_kernel   one thread per stream walks its frames' 10-byte BBHEADERs in order -- CRC-8, DFL/SYNCD checks,
//                      resynchronisation, the carried partial packet -- and turns the reference's byte-by-byte loop into
//                      one copy descriptor per frame (the only serial part: a handful of integer operations per frame);
//   bbts_emit_kernel   one workgroup per (frame, stream) moves the bytes: 0x47 + 187 bytes per packet, the first packet of
//                      a frame completed from the tail of the previous one (HBM-bound byte movement, 2 x DFL/8 per frame).
// GSE frames (TS/GS = 01) stay on the device too (bbts_gse.hip): a stream that carries one in a call is parsed, for that call, by
// the four GSE kernels, which also emit the TS frames of a mixed call.  The native host parser (BbtsHostParser, bbts_host.h) is the
// second implementation of the same rules: it runs a stream's call when dvbs2gpu_bbts_set_gse_path chose it, when a frame has more
// packets than GSE_PKT_CAP records, or when one of its output-capacity rules would fire; it shares all state with the device path
// (gse_ctx_to_host / gse_ctx_to_device, bbts_common.h).  The two read a GSE packet header through the same gse_parse_packet
// (bbts_rules.h); the reassembly rule is stated once for the device (gse_apply_packet) and once for the host (GseHostCtx::apply).
#include "ctx.h"
#include "bbts_common.h"

#include <memory>

using namespace s2;
#define g_err last_error()

namespace s2 {

__global__ void bbts_plan_kernel(const uint8_t* const* __restrict__ in, const int* __restrict__ nframes, int nstreams, int fbytes, int max_dfl,
                                 int max_frames, BbtsDevState* __restrict__ state, BbtsFrameDesc* __restrict__ desc,
                                 BbtsStreamPlan* __restrict__ plan, int* __restrict__ out_bytes) {
    const int s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= nstreams) return;
    BbtsDevState st = state[s];
    const uint8_t* bb = in[s];
    const int nf = nframes[s];
    BbtsFrameDesc* d = desc + (size_t)s * max_frames;
    int synched = st.synched, pre_len = st.count, pre_src = -1, out_off = 0, proc = 0, needs_host = 0;
    for (int f = 0; f < nf; ++f) {
        BbtsFrameDesc e = {0, 0, 0, -1, 0, {0, 0, 0}};
        const int base = f * fbytes;
        uint8_t hb[10];
        for (int k = 0; k < 10; ++k) hb[k] = bb[base + k];
        HeaderFields h;
        if (!header_ok(hb, max_dfl, &h)) { synched = 0; d[f] = e; continue; }
        int df = h.v[8] / 8, pos = base + 10;
        if (!synched) {
            const int skip = h.v[10] / 8 + 1;
            pos += skip; df -= skip;
            pre_len = 0; synched = 1;
        }
        for (int k = 0; k < 11; ++k) st.hdr[k] = h.v[k];
        ++proc;
        if (h.v[0] == 1) { needs_host = GSE_SEEN; break; }
        if (h.v[0] == 3) {
            if (df >= TS) {
                // the reference's while loop (.cpp:178-199) in closed form: the first packet absorbs the carried partial
                const int d1 = pre_len > 0 ? df - (TS - pre_len) : df;
                const int n = (pre_len > 0 ? 1 : 0) + d1 / TS, rem = d1 % TS;
                e.src = pos; e.npk = n; e.pre_len = pre_len; e.pre_src = pre_src; e.out_off = out_off;
                out_off += n * TS;
                pre_len = rem; pre_src = pos + df - rem;
            } else if (df > 0) {
                pre_len = df; pre_src = pos;          // .cpp:201-205: a short data field REPLACES the partial
            }
        }
        d[f] = e;
    }
    BbtsStreamPlan p;
    p.needs_host = needs_host;
    if (needs_host) {
        for (int f = 0; f < nf; ++f) d[f].npk = 0;
        p.out_bytes = 0; p.fin_len = TS; p.fin_src = -1;
    } else {
        st.synched = synched; st.count = pre_len; st.last_cnt = nf; st.last_proc = proc;
        state[s] = st;
        p.out_bytes = out_off; p.fin_len = pre_len; p.fin_src = pre_src;
    }
    plan[s] = p;
    out_bytes[s] = p.out_bytes;
}

__global__ void __launch_bounds__(256) bbts_emit_kernel(const uint8_t* const* __restrict__ in, uint8_t* const* __restrict__ out,
                                                        const int* __restrict__ nframes, int max_frames,
                                                        const BbtsFrameDesc* __restrict__ desc, const BbtsStreamPlan* __restrict__ plan,
                                                        const uint8_t* __restrict__ reasm_old, uint8_t* __restrict__ reasm_new) {
    const int s = blockIdx.y, f = blockIdx.x;
    const uint8_t* bb = in[s];
    const uint8_t* old = reasm_old + (size_t)s * REASM_STRIDE;
    if (f == max_frames) {                      // the partial packet carried into the next call
        const BbtsStreamPlan p = plan[s];
        uint8_t* nw = reasm_new + (size_t)s * REASM_STRIDE;
        for (int i = threadIdx.x; i < p.fin_len; i += blockDim.x) nw[i] = p.fin_src < 0 ? old[i] : bb[p.fin_src + i];
        return;
    }
    if (f >= nframes[s]) return;
    const BbtsFrameDesc e = desc[(size_t)s * max_frames + f];
    if (e.npk == 0) return;
    bbts_emit_frame(bb, old, e, out[s] + e.out_off);
}

}  // namespace s2

struct dvbs2gpu_bbts {
    dvbs2gpu_ctx* ctx = nullptr;
    int nstreams = 0, kbch = 0, max_frames = 0;
    DevBuf<BbtsDevState> d_state;
    DevBuf<uint8_t> d_reasm[2];
    int cur = 0;
    DevBuf<BbtsFrameDesc> d_desc;
    DevBuf<BbtsStreamPlan> d_plan;
    DevBuf<uint8_t> d_args;                    // BankArgs(nstreams): [in ptrs][out ptrs][nframes][out bytes]
    Workspace in1, out1;                       // staging of the single-stream host-buffer entry point
    std::vector<std::unique_ptr<BbtsHostParser>> host;
    std::vector<BbtsStreamPlan> h_plan;
    std::vector<uint8_t> h_in, h_out;
    BbtsMa* ma = nullptr;                      // mode-adaptation mode (bbts_ma.hip); null while the mode is off
    BbtsGse* gse = nullptr;                    // GSE storage on the device (bbts_gse.hip); allocated when the bank first meets a GSE frame
    int gse_mode = 0;                          // dvbs2gpu_bbts_set_gse_path
    std::vector<GseStreamOut> h_sout;
    std::vector<int> nrows;                    // rows of the last call per stream; rows_host: they are in the host parser, not in HBM
    std::vector<char> rows_host;
    std::vector<long long> fb_records, fb_capacity;
};

namespace s2 {
BbtsBankView bbts_view(dvbs2gpu_bbts* b) { return {b->ctx, b->nstreams, b->kbch, b->max_frames, &b->ma}; }
dvbs2gpu_bbts* bbts_new_host_bank(int kbch_bits, int max_frames) {
    auto b = new dvbs2gpu_bbts();
    b->nstreams = 1; b->kbch = kbch_bits; b->max_frames = max_frames;
    return b;
}
int bbts_reset_reference_state(dvbs2gpu_bbts* b) {
    if (!b->ctx) return 0;
    HIP_TRY(hipSetDevice(b->ctx->device));
    HIP_TRY(hipMemset(b->d_state, 0, (size_t)b->nstreams * sizeof(BbtsDevState)));
    for (auto& h : b->host) h.reset();
    std::fill(b->nrows.begin(), b->nrows.end(), 0);
    std::fill(b->fb_records.begin(), b->fb_records.end(), 0);
    std::fill(b->fb_capacity.begin(), b->fb_capacity.end(), 0);
    return bbts_gse_reset(b->gse);
}

// The GSE context of one stream lives in HBM once the bank has its device storage; a call that the host parser runs takes it
// from there and returns it: slots, counters, the last CRC verdict, the bytes of the open reassemblies.
static int gse_state_to_host(dvbs2gpu_bbts* b, int i, BbtsHostParser& hp) {
    return gse_ctx_to_host(hp.gse, bbts_gse_state(b->gse) + i, bbts_gse_slot_data(b->gse, i, 0));
}
static int gse_state_to_device(dvbs2gpu_bbts* b, int i, const BbtsHostParser& hp) {
    return gse_ctx_to_device(hp.gse, bbts_gse_state(b->gse) + i, bbts_gse_slot_data(b->gse, i, 0));
}
// The context as it stands: in HBM once the bank has its device storage, until then with the stream's host parser if it has one.  The
// counters travel with it, so each call of a stream is counted once, by the parser that ran it.
static int bbts_gse_context(dvbs2gpu_bbts* b, int stream, GseDevState* gs) {
    if (!b->gse) {
        if (b->host[stream]) *gs = b->host[stream]->gse.g;
        return 0;
    }
    HIP_TRY(hipMemcpy(gs, bbts_gse_state(b->gse) + stream, sizeof(*gs), hipMemcpyDeviceToHost));
    return 0;
}
// 3 x 64 KiB of reassembly storage per stream and the record / row tables: only for a bank that meets a GSE frame
static int gse_storage(dvbs2gpu_bbts* b) {
    if (b->gse) return 0;
    int e = bbts_gse_create(b->nstreams, b->max_frames, &b->gse);
    for (int i = 0; i < b->nstreams && !e; ++i)     // streams the host parser has served so far (dvbs2gpu_bbts_set_gse_path)
        if (b->host[i]) e = gse_state_to_device(b, i, *b->host[i]);
    return e;
}
}  // namespace s2

extern "C" {

void dvbs2gpu_bbts_destroy(dvbs2gpu_bbts* b) {
    if (!b) return;
    bbts_ma_free(b->ma);
    bbts_gse_free(b->gse);
    delete b;
}

int dvbs2gpu_bbts_set_frame_size(dvbs2gpu_bbts* b, int kbch_bits) {
    if (!b || !b->ctx || kbch_bits < 88 || kbch_bits % 8 || kbch_bits > 65536) return DVBS2GPU_ERR_ARG;
    HIP_TRY(hipSetDevice(b->ctx->device));
    // setFrameSize (.cpp:31-42) forgets the synchronisation; header copy and counters stay, as do the GSE slots
    std::vector<BbtsDevState> st(b->nstreams);
    HIP_TRY(hipMemcpy(st.data(), b->d_state, st.size() * sizeof(BbtsDevState), hipMemcpyDeviceToHost));
    for (auto& s : st) { s.synched = 0; s.count = 0; }
    HIP_TRY(hipMemcpy(b->d_state, st.data(), st.size() * sizeof(BbtsDevState), hipMemcpyHostToDevice));
    b->kbch = kbch_bits;
    return 0;
}

int dvbs2gpu_bbts_create(dvbs2gpu_ctx* ctx, int nstreams, int kbch_bits, int max_frames, dvbs2gpu_bbts** out) {
    if (!ctx || !out || nstreams <= 0 || max_frames <= 0 || kbch_bits < 88 || kbch_bits % 8 || kbch_bits > 65536) return DVBS2GPU_ERR_ARG;
    HIP_TRY(hipSetDevice(ctx->device));
    std::unique_ptr<dvbs2gpu_bbts> b(new dvbs2gpu_bbts());
    b->ctx = ctx; b->nstreams = nstreams; b->kbch = kbch_bits; b->max_frames = max_frames;
    b->host.resize(nstreams);
    b->h_plan.resize(nstreams);
    b->h_sout.resize(nstreams);
    b->nrows.assign(nstreams, 0); b->rows_host.assign(nstreams, 0);
    b->fb_records.assign(nstreams, 0); b->fb_capacity.assign(nstreams, 0);
    const size_t n = (size_t)nstreams;
    const char* what = "hipMalloc(bbts)";
    RC_TRY(b->d_state.alloc(n, true, what));
    for (auto& r : b->d_reasm) RC_TRY(r.alloc(n * REASM_STRIDE, true, what));
    RC_TRY(b->d_desc.alloc(n * max_frames, true, what));
    RC_TRY(b->d_plan.alloc(n, true, what));
    RC_TRY(b->d_args.alloc(BankArgs(n).L.bytes(), true, what));
    *out = b.release();
    return 0;
}

int dvbs2gpu_bbts_process_batch(dvbs2gpu_bbts* b, const uint8_t* const* d_bb, const int* nframes, uint8_t* const* d_out, int cap,
                                int* out_bytes, void* stream) {
    if (!b || !b->ctx || !d_bb || !nframes || !d_out || !out_bytes || cap < 0) return DVBS2GPU_ERR_ARG;
    HIP_TRY(hipSetDevice(b->ctx->device));
    hipStream_t st = (hipStream_t)stream;
    const int n = b->nstreams, fbytes = b->kbch / 8;
    for (int i = 0; i < n; ++i) {
        if (nframes[i] < 0 || nframes[i] > b->max_frames) { g_err = "frame count exceeds max_frames"; return DVBS2GPU_ERR_ARG; }
        if (nframes[i] > 0 && (!d_bb[i] || !d_out[i])) return DVBS2GPU_ERR_ARG;
        // every TS packet is at most the bytes it was cut from + one carried partial; the reference additionally stops
        // when fewer than 189 bytes are left (.cpp:178,206): with this bound it never does
        if ((long)cap < (long)nframes[i] * fbytes + 2 * TS) { g_err = "cap must be >= nframes*kbch/8 + 376"; return DVBS2GPU_ERR_CAPACITY; }
    }
    const BankArgs a(n);
    const uint8_t** a_in = a.in(b->d_args); uint8_t** a_out = a.out(b->d_args);
    int *a_nf = a.cnt(b->d_args), *a_ob = a.ob(b->d_args);
    HIP_TRY(hipMemcpyAsync(a_in, d_bb, sizeof(void*) * n, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(a_out, d_out, sizeof(void*) * n, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(a_nf, nframes, sizeof(int) * n, hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(bbts_plan_kernel, dim3((n + 63) / 64), dim3(64), 0, st, a_in, a_nf, n, fbytes, b->kbch - 80, b->max_frames, b->d_state,
                       b->d_desc, b->d_plan, a_ob);
    hipLaunchKernelGGL(bbts_emit_kernel, dim3(b->max_frames + 1, n), dim3(256), 0, st, a_in, a_out, a_nf, b->max_frames, b->d_desc, b->d_plan,
                       b->d_reasm[b->cur], b->d_reasm[b->cur ^ 1]);
    HIP_TRY(hipGetLastError());
    b->cur ^= 1;
    // GSE on the device: four more launches behind the two above, for the streams whose plan met a GSE frame.  A bank that
    // has not met one yet learns it from the plan read-back, allocates its GSE storage and launches them then.
    const bool device_gse = b->gse_mode == 0;
    auto gse_pass = [&]() -> int {
        return bbts_gse_launch(b->gse, st, a_in, a_out, a_nf, a_ob, fbytes, b->kbch - 80, cap, b->d_state, b->d_desc, b->d_plan, b->d_reasm[b->cur]);
    };
    auto read_back = [&](bool with_gse) -> int {
        HIP_TRY(hipMemcpyAsync(out_bytes, a_ob, sizeof(int) * n, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipMemcpyAsync(b->h_plan.data(), b->d_plan, sizeof(BbtsStreamPlan) * n, hipMemcpyDeviceToHost, st));
        if (with_gse) HIP_TRY(hipMemcpyAsync(b->h_sout.data(), bbts_gse_stream_out(b->gse), sizeof(GseStreamOut) * n, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        return 0;
    };
    bool ran_gse = device_gse && b->gse;
    if (ran_gse) { const int e = gse_pass(); if (e) return e; }
    { const int e = read_back(ran_gse); if (e) return e; }
    if (device_gse && !b->gse) {
        bool seen = false;
        for (int i = 0; i < n; ++i) seen |= b->h_plan[i].needs_host == GSE_SEEN;
        if (seen) {
            int e = gse_storage(b);
            if (e || (e = gse_pass()) || (e = read_back(true))) return e;
            ran_gse = true;
        }
    }
    // streams left to the host parser: the whole call of that stream, all state taken from and returned to the device
    int rc = 0;
    for (int i = 0; i < n; ++i) {
        const int why = b->h_plan[i].needs_host;
        b->rows_host[i] = 0;
        b->nrows[i] = ran_gse && b->h_sout[i].ran ? b->h_sout[i].nrows : 0;
        if (!why) continue;
        if (why == GSE_FALLBACK_RECORDS) ++b->fb_records[i];
        if (why == GSE_FALLBACK_CAPACITY) ++b->fb_capacity[i];
        if (!b->host[i]) b->host[i].reset(new BbtsHostParser());
        BbtsHostParser& hp = *b->host[i];
        BbtsDevState ds;
        HIP_TRY(hipMemcpy(&ds, b->d_state + i, sizeof(ds), hipMemcpyDeviceToHost));
        HIP_TRY(hipMemcpy(hp.partial, b->d_reasm[b->cur] + (size_t)i * REASM_STRIDE, TS, hipMemcpyDeviceToHost));
        if (b->gse) { const int e = gse_state_to_host(b, i, hp); if (e) return e; }
        hp.synched = ds.synched; hp.count = ds.count;
        memcpy(hp.hdr, ds.hdr, sizeof(ds.hdr));
        b->h_in.resize((size_t)nframes[i] * fbytes);
        b->h_out.resize((size_t)cap);
        HIP_TRY(hipMemcpy(b->h_in.data(), d_bb[i], b->h_in.size(), hipMemcpyDeviceToHost));
        const int got = hp.run(b->h_in.data(), nframes[i], fbytes, b->kbch - 80, b->h_out.data(), cap);
        ds.synched = hp.synched; ds.count = hp.count; ds.last_cnt = hp.last_cnt; ds.last_proc = hp.last_proc;
        memcpy(ds.hdr, hp.hdr, sizeof(ds.hdr));
        HIP_TRY(hipMemcpy(b->d_state + i, &ds, sizeof(ds), hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(b->d_reasm[b->cur] + (size_t)i * REASM_STRIDE, hp.partial, TS, hipMemcpyHostToDevice));
        if (b->gse) { const int e = gse_state_to_device(b, i, hp); if (e) return e; }
        b->rows_host[i] = 1;
        b->nrows[i] = (int)hp.gse.rows.size();
        if (got < 0) { out_bytes[i] = 0; rc = got; g_err = "output buffer too small for the TS packets of a GSE-carrying call"; continue; }
        out_bytes[i] = got;
        if (got > 0) HIP_TRY(hipMemcpy(d_out[i], b->h_out.data(), got, hipMemcpyHostToDevice));
    }
    return rc;
}

int dvbs2gpu_bbts_work(dvbs2gpu_bbts* b, const uint8_t* h_bb, int cnt, uint8_t* h_ts, int cap) {
    if (!b || !b->ctx || b->nstreams != 1 || cnt < 0 || cnt > b->max_frames || cap < 0 || (cnt > 0 && (!h_bb || !h_ts))) return DVBS2GPU_ERR_ARG;
    HIP_TRY(hipSetDevice(b->ctx->device));
    const size_t fbytes = b->kbch / 8;
    if (const int e = b->in1.ensure((size_t)b->max_frames * 8192 + 64)) return e;
    HIP_TRY(hipMemcpy(b->in1.p, h_bb, cnt * fbytes, hipMemcpyHostToDevice));
    if (const int e = b->out1.ensure((size_t)cap + 64)) return e;
    uint8_t* d_out = static_cast<uint8_t*>(b->out1.p);
    const uint8_t* in_p = static_cast<const uint8_t*>(b->in1.p);
    int got = 0;
    int rc = dvbs2gpu_bbts_process_batch(b, &in_p, &cnt, &d_out, cap, &got, nullptr);
    if (rc == 0 && got > 0) {
        hipError_t e = hipMemcpy(h_ts, d_out, got, hipMemcpyDeviceToHost);
        if (e != hipSuccess) rc = fail_hip(e, "hipMemcpy(bbts out)");
    }
    return rc < 0 ? rc : got;
}

/* h_out15 = {ts_gs, sis_mis, ccm_acm, issyi, npd, ro, isi, upl, dfl, sync, syncd (last_header), last_gse_crc_err, last_bb_cnt,
 * last_bb_proc, last_ts_errs}; h_out15[15..16] = {synched, count} when 17 ints are asked for */
int dvbs2gpu_bbts_get_stats(dvbs2gpu_bbts* b, int stream, int32_t* h_out, int n_out) {
    if (!b || !b->ctx || stream < 0 || stream >= b->nstreams || !h_out || n_out < 15) return DVBS2GPU_ERR_ARG;
    HIP_TRY(hipSetDevice(b->ctx->device));
    BbtsDevState ds;
    HIP_TRY(hipMemcpy(&ds, b->d_state + stream, sizeof(ds), hipMemcpyDeviceToHost));
    for (int i = 0; i < 11; ++i) h_out[i] = ds.hdr[i];
    GseDevState gs = {};
    const int e = bbts_gse_context(b, stream, &gs);
    if (e) return e;
    h_out[11] = gs.crc_err;
    h_out[12] = ds.last_cnt; h_out[13] = ds.last_proc; h_out[14] = 0;
    if (n_out >= 17) { h_out[15] = ds.synched; h_out[16] = ds.count; }
    return 0;
}

int dvbs2gpu_bbts_set_gse_path(dvbs2gpu_bbts* b, int mode) {
    if (!b || !b->ctx || (mode != 0 && mode != 1)) return DVBS2GPU_ERR_ARG;
    b->gse_mode = mode;
    return 0;
}

int dvbs2gpu_bbts_get_gse_stats(dvbs2gpu_bbts* b, int stream, dvbs2gpu_gse_stats* out) {
    if (!b || !b->ctx || stream < 0 || stream >= b->nstreams || !out) return DVBS2GPU_ERR_ARG;
    HIP_TRY(hipSetDevice(b->ctx->device));
    static_assert(sizeof(GseCounters) == 9 * sizeof(int64_t) && sizeof(dvbs2gpu_gse_stats) == 12 * sizeof(int64_t), "layout");
    GseDevState gs = {};
    const int e = bbts_gse_context(b, stream, &gs);
    if (e) return e;
    memcpy(&out->frames, &gs.cnt, sizeof(GseCounters));
    out->fallback_records = b->fb_records[stream]; out->fallback_capacity = b->fb_capacity[stream];
    out->host_fallback_calls = out->fallback_records + out->fallback_capacity;
    return 0;
}

int dvbs2gpu_bbts_get_pdu_table(dvbs2gpu_bbts* b, int stream, dvbs2gpu_gse_pdu* h_rows, int cap, int* n) {
    if (!b || !b->ctx || stream < 0 || stream >= b->nstreams || !n || cap < 0 || (cap > 0 && !h_rows)) return DVBS2GPU_ERR_ARG;
    HIP_TRY(hipSetDevice(b->ctx->device));
    *n = b->nrows[stream];
    const int m = *n < cap ? *n : cap;
    if (m <= 0) return 0;
    if (b->rows_host[stream]) memcpy(h_rows, b->host[stream]->gse.rows.data(), m * sizeof(dvbs2gpu_gse_pdu));
    else HIP_TRY(hipMemcpy(h_rows, bbts_gse_rows(b->gse, stream), m * sizeof(dvbs2gpu_gse_pdu), hipMemcpyDeviceToHost));
    return 0;
}

int dvbs2gpu_bbts_get_pdu_table_device(dvbs2gpu_bbts* b, int stream, const dvbs2gpu_gse_pdu** d_rows, int* n) {
    if (!b || !b->ctx || stream < 0 || stream >= b->nstreams || !n || !d_rows) return DVBS2GPU_ERR_ARG;
    HIP_TRY(hipSetDevice(b->ctx->device));
    *n = b->nrows[stream];
    *d_rows = nullptr;
    if (*n == 0) return 0;
    if (b->rows_host[stream]) {                    // a call the host parser ran: its rows go to where the kernels put theirs
        const int e = gse_storage(b);
        if (e) return e;
        if (*n > b->max_frames * GSE_PKT_CAP) { g_err = "more rows than the device table holds"; return DVBS2GPU_ERR_CAPACITY; }
        HIP_TRY(hipMemcpy(bbts_gse_rows(b->gse, stream), b->host[stream]->gse.rows.data(), *n * sizeof(dvbs2gpu_gse_pdu), hipMemcpyHostToDevice));
    }
    *d_rows = (const dvbs2gpu_gse_pdu*)bbts_gse_rows(b->gse, stream);
    return 0;
}

uint32_t dvbs2gpu_crc32_mpeg_shift(uint32_t crc, uint32_t nbytes) {
    uint32_t r = crc;
    for (; nbytes >= (1u << 17); nbytes -= 1u << 16) r = crc32m_mulmod(r, crc32m_xpow(1u << 16));
    return crc32m_mulmod(r, crc32m_xpow(nbytes));
}

}  // extern "C"
