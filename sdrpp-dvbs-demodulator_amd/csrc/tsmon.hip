// TS monitor bank (own extension; include/dvbs2gpu.h): per-PID continuity checks, a per-call PID table and a PID
// filter for `nstreams` transport streams that the packetisers (bbts.hip, bbts_ma.hip, dvbs_capi.hip) have left in HBM.
// Every rule is in tsmon_rules.h; this file says how a call's packets are brought into per-PID order and who walks them.
//
//   tsmon_scan_kernel  one workgroup per stream.  Every packet's six header bytes are read once and classified; a trusted packet
//                      becomes the key PID << 13 | index and nine bits of header in LDS.  A bitonic sort of the keys puts the
//                      packets of a PID next to each other in input order, PIDs ascending: the sorted array IS the PID table's
//                      order.  One lane per PID present then walks its run with tsmon_row_add -- the sequential definition, from
//                      the PID's state byte in HBM -- and writes the row and the PID's new state.  A prefix sum over the run
//                      heads numbers the rows; the pass flags of the filter are counted for the capacity decision.
//                      Without output buffers nothing can fail for lack of room and the kernel stores the new states itself.
//   tsmon_emit_kernel  (calls with output buffers, once the host has seen that every stream's passing packets fit) one workgroup
//                      per stream: stores the new states of the rows' PIDs, recomputes the pass flags, numbers the passing
//                      packets by an exact prefix sum (a contiguous run of packets per thread, any packet count) and copies them
//                      in input order, a dword per lane.
// Two launches at most, whatever nstreams and the packet counts are; one device-to-host copy (TsmonCall per stream: bytes needed,
// rows, the call's counters).  The cumulative counters live on the host; the device keeps 8 KiB of continuity state per stream.
// TsmonHostStream below applies the same rules to host buffers, packet by packet (host-only banks; the kernels' yardstick).
// The header read, the prefix sum, the argument table, the count checks, the host staging and the table getters: ts_bank.h.
#include "ts_bank.h"

#include <map>
#include <memory>

using namespace s2;
#define g_err last_error()

namespace s2 {

constexpr int TSMON_MAX_PACKETS = 8192;          // per stream and call: key = PID << 13 | index, and the LDS of one workgroup
constexpr int TSMON_WG = 256;
constexpr unsigned TSMON_KEY_NONE = 0xffffffffu; // sorts behind every PID: untrusted packets and the padding to a power of two
static_assert(sizeof(TsmonRow) == sizeof(dvbs2gpu_tsmon_pid) && sizeof(TsmonRow) == 24, "row layout");
static_assert(sizeof(TsmonFilter) == sizeof(dvbs2gpu_tsmon_filter), "filter layout");
static_assert(TSMON_MAX_PACKETS <= 32 * TSMON_WG, "the emit kernel keeps a thread's pass flags in one 32-bit mask (ts_thread_run)");

// nine bits of a trusted packet's header for the walk
__device__ inline unsigned tsmon_pack(const TsmonHdr& h) { return h.cc | h.afc << 4 | h.di << 6 | h.pusi << 7 | (h.tsc != 0) << 8; }
__device__ inline TsmonHdr tsmon_unpack(unsigned v, int pid) {
    TsmonHdr h = {pid == TSMON_NULL_PID ? TSMON_NULL : TSMON_DATA, pid, (int)(v >> 7 & 1), (int)(v >> 8 & 1), (int)(v >> 4 & 3), (int)(v & 15),
                  (int)(v >> 6 & 1)};
    return h;
}

enum { TC_NULL = 0, TC_TEI, TC_SYNC, TC_CC, TC_DUP, TC_DISC, TC_SCR, TC_PASS, TC_FIRST, TC_COUNT };

// LDS: keys[npad_max] (dwords), then hdr[npad_max] (16 bits each)
__global__ void __launch_bounds__(TSMON_WG) tsmon_scan_kernel(const uint8_t* const* __restrict__ in, const int* __restrict__ nbytes, int max_packets,
                                                              int npad_max, int maxrows, const TsmonFilter* __restrict__ filt,
                                                              const uint32_t* __restrict__ maps, uint8_t* __restrict__ state,
                                                              TsmonRow* __restrict__ rows, uint8_t* __restrict__ newst,
                                                              TsmonCall* __restrict__ call, int commit) {
    extern __shared__ __attribute__((aligned(16))) unsigned tsmon_lds[];
    __shared__ int cnt[TC_COUNT], wsum[TSMON_WG / 64];
    unsigned* keys = tsmon_lds;
    uint16_t* hdr = reinterpret_cast<uint16_t*>(tsmon_lds + npad_max);
    const int s = blockIdx.x, tid = threadIdx.x;
    int n = nbytes[s] / TSMON_TS;
    if (n > max_packets) n = max_packets;            // (the host has refused such a call; the LDS arrays hold max_packets)
    if (n <= 0) {
        if (tid == 0) { const TsmonCall c = {}; call[s] = c; }
        return;
    }
    int npad = 1;
    while (npad < n) npad <<= 1;                     // <= npad_max
    if (tid < TC_COUNT) cnt[tid] = 0;
    __syncthreads();
    const uint8_t* ts = in[s];
    const TsmonFilter f = filt[s];
    const uint32_t* map = maps + (size_t)s * TSMON_MAP_WORDS;
    int c_null = 0, c_tei = 0, c_sync = 0, c_pass = 0;
    for (int k = tid; k < npad; k += TSMON_WG) {
        unsigned key = TSMON_KEY_NONE;
        if (k < n) {
            const TsmonHdr h = ts_load_header(ts, k);
            c_sync += h.cls == TSMON_SYNC_ERROR; c_tei += h.cls == TSMON_TEI; c_null += h.cls == TSMON_NULL;
            c_pass += tsmon_passes(h, f, map);
            if (h.cls >= TSMON_NULL) { key = (unsigned)h.pid << 13 | (unsigned)k; hdr[k] = (uint16_t)tsmon_pack(h); }
        }
        keys[k] = key;
    }
    if (c_null) atomicAdd(&cnt[TC_NULL], c_null);
    if (c_tei) atomicAdd(&cnt[TC_TEI], c_tei);
    if (c_sync) atomicAdd(&cnt[TC_SYNC], c_sync);
    if (c_pass) atomicAdd(&cnt[TC_PASS], c_pass);
    __syncthreads();
    // bitonic sort, ascending: PID major, input order within a PID
    for (int k2 = 2; k2 <= npad; k2 <<= 1)
        for (int j = k2 >> 1; j > 0; j >>= 1) {
            for (int i = tid; i < npad; i += TSMON_WG) {
                const int x = i ^ j;
                if (x > i) {
                    const unsigned a = keys[i], b = keys[x];
                    if ((a > b) == ((i & k2) == 0)) { keys[i] = b; keys[x] = a; }
                }
            }
            __syncthreads();
        }
    // a contiguous run of sorted positions per thread; the heads of the PID runs in it are this thread's rows
    const int chunk = (n + TSMON_WG - 1) / TSMON_WG, p0 = tid * chunk, p1 = p0 + chunk < n ? p0 + chunk : n;   // (ts_thread_run written out: through it four compares below come out unsigned)
    auto is_head = [&](int p) { return keys[p] != TSMON_KEY_NONE && (p == 0 || (keys[p - 1] >> 13) != (keys[p] >> 13)); };
    int heads = 0;
    for (int p = p0; p < p1; ++p) heads += is_head(p);
    int nrows;
    int rank = ts_block_scan<TSMON_WG>(heads, wsum, &nrows);
    int c_cc = 0, c_dup = 0, c_disc = 0, c_scr = 0, c_first = 0;
    for (int p = p0; p < p1; ++p) {
        if (!is_head(p)) continue;
        const int pid = (int)(keys[p] >> 13);
        uint8_t* sp = state + (size_t)s * TSMON_PIDS + pid;
        uint8_t st = *sp;
        TsmonRow r = {(uint16_t)pid, 0, 0, 0, 0, 0, 0};
        for (int q = p; q < n; ++q) {
            const unsigned key = keys[q];
            if ((int)(key >> 13) != pid) break;
            const int v = tsmon_row_add(&r, &st, tsmon_unpack(hdr[key & (TSMON_MAX_PACKETS - 1)], pid));
            c_disc += v == TSMON_DISC; c_first += v == TSMON_FIRST;
        }
        c_cc += r.cc_errors; c_dup += r.duplicates; c_scr += r.scrambled;
        if (rank < maxrows) {                          // (always: a call has at most min(packets, 8192) PIDs)
            rows[(size_t)s * maxrows + rank] = r;
            newst[(size_t)s * maxrows + rank] = st;
        }
        if (commit) *sp = st;
        ++rank;
    }
    if (c_cc) atomicAdd(&cnt[TC_CC], c_cc);
    if (c_dup) atomicAdd(&cnt[TC_DUP], c_dup);
    if (c_disc) atomicAdd(&cnt[TC_DISC], c_disc);
    if (c_scr) atomicAdd(&cnt[TC_SCR], c_scr);
    if (c_first) atomicAdd(&cnt[TC_FIRST], c_first);
    __syncthreads();
    if (tid == 0) {
        const TsmonCall c = {cnt[TC_PASS] * TSMON_TS, nrows, n, cnt[TC_NULL], cnt[TC_TEI], cnt[TC_SYNC], cnt[TC_CC], cnt[TC_DUP], cnt[TC_DISC],
                             cnt[TC_SCR], cnt[TC_PASS], cnt[TC_FIRST]};
        call[s] = c;
    }
}

// LDS: src[max_packets] (16 bits each): the input index of every passing packet, in output order
__global__ void __launch_bounds__(TSMON_WG) tsmon_emit_kernel(const uint8_t* const* __restrict__ in, uint8_t* const* __restrict__ out,
                                                              const int* __restrict__ nbytes, int max_packets, int maxrows, int cap,
                                                              const TsmonFilter* __restrict__ filt, const uint32_t* __restrict__ maps,
                                                              uint8_t* __restrict__ state, const TsmonRow* __restrict__ rows,
                                                              const uint8_t* __restrict__ newst, const TsmonCall* __restrict__ call) {
    extern __shared__ __attribute__((aligned(16))) unsigned tsmon_lds[];
    __shared__ int wsum[TSMON_WG / 64];
    uint16_t* src = reinterpret_cast<uint16_t*>(tsmon_lds);
    const int s = blockIdx.x, tid = threadIdx.x;
    int n = nbytes[s] / TSMON_TS;
    if (n > max_packets) n = max_packets;
    if (n <= 0) return;
    int nrows = call[s].nrows;
    if (nrows > maxrows) nrows = maxrows;
    for (int r = tid; r < nrows; r += TSMON_WG) {
        const int pid = rows[(size_t)s * maxrows + r].pid;
        state[(size_t)s * TSMON_PIDS + pid] = newst[(size_t)s * maxrows + r];       // (the null PID's byte stays 0: it is never stepped)
    }
    const uint8_t* ts = in[s];
    uint8_t* o = out[s];
    const TsmonFilter f = filt[s];
    const uint32_t* map = maps + (size_t)s * TSMON_MAP_WORDS;
    // a contiguous run of at most 32 packets per thread (8192 / 256): its pass flags in one word
    int k0, k1; ts_thread_run(n, TSMON_WG, &k0, &k1);
    unsigned mask = 0;
    for (int k = k0; k < k1; ++k) mask |= (unsigned)tsmon_passes(ts_load_header(ts, k), f, map) << (k - k0);
    int total;
    int at = ts_block_scan<TSMON_WG>(__popc(mask), wsum, &total);
    for (int k = k0; k < k1; ++k) if (mask >> (k - k0) & 1) src[at++] = (uint16_t)k;
    __syncthreads();
    if (total > cap / TSMON_TS) total = cap / TSMON_TS;  // (the host launches this kernel only when every stream fits)
    if (((reinterpret_cast<uintptr_t>(ts) | reinterpret_cast<uintptr_t>(o)) & 3) == 0) {
        const unsigned* i32 = reinterpret_cast<const unsigned*>(ts);
        unsigned* o32 = reinterpret_cast<unsigned*>(o);
        for (int w = tid; w < total * (TSMON_TS / 4); w += TSMON_WG) {
            const int d = w / (TSMON_TS / 4), j = w - d * (TSMON_TS / 4);
            o32[w] = i32[(size_t)src[d] * (TSMON_TS / 4) + j];
        }
    } else {
        for (int i = tid; i < total * TSMON_TS; i += TSMON_WG) {
            const int d = i / TSMON_TS, j = i - d * TSMON_TS;
            o[i] = ts[(size_t)src[d] * TSMON_TS + j];
        }
    }
}

// ------------------------------------------------------------------------------------------------- host bank
// The same rules for one stream in host memory, one packet at a time.
struct TsmonHostStream {
    uint8_t state[TSMON_PIDS] = {};
    std::vector<TsmonRow> rows;
    // needed < 0: the passing packets do not fit cap; nothing has changed then
    int run(const TsmonFilter& f, const uint32_t* map, const uint8_t* ts, int n, uint8_t* out, int cap, TsmonCall* c) {
        int pass = 0;
        for (int k = 0; k < n; ++k) pass += tsmon_passes(tsmon_parse(ts + (size_t)k * TSMON_TS), f, map);
        *c = TsmonCall{};
        c->needed = pass * TSMON_TS;
        if (out && c->needed > cap) return -1;
        std::map<int, TsmonRow> tab;
        int at = 0;
        for (int k = 0; k < n; ++k) {
            const uint8_t* p = ts + (size_t)k * TSMON_TS;
            const TsmonHdr h = tsmon_parse(p);
            ++c->packets;
            c->sync_byte_errors += h.cls == TSMON_SYNC_ERROR; c->tei_packets += h.cls == TSMON_TEI; c->null_packets += h.cls == TSMON_NULL;
            if (tsmon_passes(h, f, map)) {
                ++c->passed_packets;
                if (out) { memcpy(out + at, p, TSMON_TS); at += TSMON_TS; }
            }
            if (h.cls < TSMON_NULL) continue;
            TsmonRow& r = tab.emplace(h.pid, TsmonRow{(uint16_t)h.pid, 0, 0, 0, 0, 0, 0}).first->second;
            const int v = tsmon_row_add(&r, &state[h.pid], h);
            c->discontinuities += v == TSMON_DISC; c->first_seen += v == TSMON_FIRST;
        }
        rows.clear();
        for (const auto& kv : tab) {
            rows.push_back(kv.second);
            c->cc_errors += kv.second.cc_errors; c->duplicates += kv.second.duplicates; c->scrambled_packets += kv.second.scrambled;
        }
        c->nrows = (int)rows.size();
        return 0;
    }
};

}  // namespace s2

struct dvbs2gpu_tsmon {
    dvbs2gpu_ctx* ctx = nullptr;                   // null: a host-only bank (dvbs2gpu_tsmon_create_host)
    int nstreams = 0, max_packets = 0, maxrows = 0, npad_max = 1;
    std::vector<TsmonFilter> filt;
    std::vector<uint32_t> map;                     // nstreams x 256 words
    std::vector<dvbs2gpu_tsmon_stats> stats;       // since reset; the kernels report each call's share (TsmonCall)
    std::vector<int> nrows;                        // rows of the last call per stream
    std::vector<TsmonCall> h_call;
    std::vector<char> h_args;
    // device banks
    DevBuf<uint8_t> d_state;                       // nstreams x 8192 continuity bytes (tsmon_rules.h)
    DevBuf<TsmonFilter> d_filt;
    DevBuf<uint32_t> d_map;
    DevBuf<TsmonRow> d_rows;                       // nstreams x maxrows
    DevBuf<uint8_t> d_newst;                       // the state byte behind every row's last packet
    DevBuf<TsmonCall> d_call;
    DevBuf<uint8_t> d_args;                        // TsBankArgs(nstreams)
    TsHostStage stage;                             // of the host-buffer entry point
    // host-only banks
    std::vector<TsmonHostStream> host;
};

namespace s2 {
static void tsmon_account(dvbs2gpu_tsmon* m, int i, const TsmonCall& c) {
    dvbs2gpu_tsmon_stats& s = m->stats[i];
    s.packets += c.packets; s.null_packets += c.null_packets; s.tei_packets += c.tei_packets; s.sync_byte_errors += c.sync_byte_errors;
    s.cc_errors += c.cc_errors; s.duplicates += c.duplicates; s.discontinuities += c.discontinuities;
    s.scrambled_packets += c.scrambled_packets; s.passed_packets += c.passed_packets; s.pids_seen += c.first_seen;
    m->nrows[i] = c.nrows;
}
static std::unique_ptr<dvbs2gpu_tsmon> tsmon_new(dvbs2gpu_ctx* ctx, int nstreams, int max_packets) {
    std::unique_ptr<dvbs2gpu_tsmon> m(new dvbs2gpu_tsmon());
    m->ctx = ctx; m->nstreams = nstreams; m->max_packets = max_packets;
    m->maxrows = max_packets < TSMON_PIDS ? max_packets : TSMON_PIDS;
    while (m->npad_max < max_packets) m->npad_max <<= 1;
    m->filt.assign(nstreams, TsmonFilter{0, 0, 0, 0});
    m->map.assign((size_t)nstreams * TSMON_MAP_WORDS, 0);
    m->stats.assign(nstreams, dvbs2gpu_tsmon_stats{});
    m->nrows.assign(nstreams, 0);
    m->h_call.resize(nstreams);
    return m;
}
static bool tsmon_create_args_ok(int nstreams, int max_packets, dvbs2gpu_tsmon** out) {
    if (!out || nstreams <= 0 || max_packets <= 0) return false;
    if (max_packets > TSMON_MAX_PACKETS) { g_err = "TS monitor: max_packets is at most 8192 per stream and call"; return false; }
    return true;
}
}  // namespace s2

extern "C" {

void dvbs2gpu_tsmon_destroy(dvbs2gpu_tsmon* m) { delete m; }

int dvbs2gpu_tsmon_create(dvbs2gpu_ctx* ctx, int nstreams, int max_packets, dvbs2gpu_tsmon** out) {
    if (!ctx || !tsmon_create_args_ok(nstreams, max_packets, out)) return DVBS2GPU_ERR_ARG;
    HIP_TRY(hipSetDevice(ctx->device));
    auto m = tsmon_new(ctx, nstreams, max_packets);
    const size_t n = (size_t)nstreams;
    const char* what = "hipMalloc(tsmon)";             // (the rows, their states and the call records are written before they are read)
    RC_TRY(m->d_state.alloc(n * TSMON_PIDS, true, what));
    RC_TRY(m->d_filt.alloc(n, true, what));
    RC_TRY(m->d_map.alloc(n * TSMON_MAP_WORDS, true, what));
    RC_TRY(m->d_rows.alloc(n * m->maxrows, false, what));
    RC_TRY(m->d_newst.alloc(n * m->maxrows, false, what));
    RC_TRY(m->d_call.alloc(n, false, what));
    RC_TRY(m->d_args.alloc(TsBankArgs(n).L.bytes(), false, what));
    m->h_args.resize(TsBankArgs(n).L.bytes());
    *out = m.release();
    return 0;
}

int dvbs2gpu_tsmon_create_host(int nstreams, int max_packets, dvbs2gpu_tsmon** out) {
    if (!tsmon_create_args_ok(nstreams, max_packets, out)) return DVBS2GPU_ERR_ARG;
    auto m = tsmon_new(nullptr, nstreams, max_packets);
    m->host.resize(nstreams);
    *out = m.release();
    return 0;
}

int dvbs2gpu_tsmon_reset(dvbs2gpu_tsmon* m) {
    if (!m) return DVBS2GPU_ERR_ARG;
    if (m->ctx) {
        HIP_TRY(hipSetDevice(m->ctx->device));
        HIP_TRY(hipMemset(m->d_state, 0, (size_t)m->nstreams * TSMON_PIDS));
    }
    for (auto& h : m->host) { memset(h.state, 0, sizeof(h.state)); h.rows.clear(); }
    std::fill(m->stats.begin(), m->stats.end(), dvbs2gpu_tsmon_stats{});
    std::fill(m->nrows.begin(), m->nrows.end(), 0);
    return 0;
}

int dvbs2gpu_tsmon_set_filter(dvbs2gpu_tsmon* m, int stream, const dvbs2gpu_tsmon_filter* f, const uint16_t* pids, int n) {
    if (!m || stream < 0 || stream >= m->nstreams || !f || n < 0 || (n > 0 && !pids)) return DVBS2GPU_ERR_ARG;
    if (f->mode < 0 || f->mode > 2) { g_err = "TS monitor: filter mode is 0 (pass all), 1 (pass listed) or 2 (drop listed)"; return DVBS2GPU_ERR_ARG; }
    for (int k = 0; k < n; ++k) if (pids[k] >= TSMON_PIDS) { g_err = "TS monitor: a PID is at most 0x1FFF"; return DVBS2GPU_ERR_ARG; }
    uint32_t* map = m->map.data() + (size_t)stream * TSMON_MAP_WORDS;
    std::fill(map, map + TSMON_MAP_WORDS, 0u);
    for (int k = 0; k < n; ++k) map[pids[k] >> 5] |= 1u << (pids[k] & 31);
    m->filt[stream] = {f->mode, f->drop_null != 0, f->drop_tei != 0, f->drop_bad_sync != 0};
    if (m->ctx) {
        HIP_TRY(hipSetDevice(m->ctx->device));
        HIP_TRY(hipMemcpy(m->d_filt + stream, &m->filt[stream], sizeof(TsmonFilter), hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(m->d_map + (size_t)stream * TSMON_MAP_WORDS, map, TSMON_MAP_WORDS * sizeof(uint32_t), hipMemcpyHostToDevice));
    }
    return 0;
}

int dvbs2gpu_tsmon_process_batch(dvbs2gpu_tsmon* m, const uint8_t* const* d_ts, const int* nbytes, uint8_t* const* d_out, int cap,
                                 int* out_bytes, void* stream) {
    if (!m || !d_ts || !nbytes || cap < 0 || (d_out && !out_bytes)) return DVBS2GPU_ERR_ARG;
    if (!m->ctx) { g_err = "TS monitor: a host bank takes host buffers (dvbs2gpu_tsmon_work)"; return DVBS2GPU_ERR_ARG; }
    const int n = m->nstreams;
    for (int i = 0; i < n; ++i) {
        if (!ts_bank_check_counts("TS monitor: ", nbytes + i, 1, m->max_packets)) return DVBS2GPU_ERR_ARG;
        // only a stream that brings packets needs its buffers (the PSI bank wants an output pointer for every stream)
        if (nbytes[i] > 0 && (!d_ts[i] || (d_out && (!d_out[i] || d_out[i] == d_ts[i])))) {
            g_err = "TS monitor: null buffer, or an output buffer that is its stream's input";
            return DVBS2GPU_ERR_ARG;
        }
    }
    HIP_TRY(hipSetDevice(m->ctx->device));
    hipStream_t st = (hipStream_t)stream;
    const TsBankArgs a(n);
    a.fill(m->h_args.data(), n, d_ts, d_out, nbytes);
    HIP_TRY(hipMemcpyAsync(m->d_args, m->h_args.data(), m->h_args.size(), hipMemcpyHostToDevice, st));
    const size_t lds_scan = (size_t)m->npad_max * 6, lds_emit = ((size_t)m->max_packets * 2 + 15) / 16 * 16;   // <= 48 KiB
    hipLaunchKernelGGL(tsmon_scan_kernel, dim3(n), dim3(TSMON_WG), lds_scan, st, a.in(m->d_args), a.nbytes(m->d_args), m->max_packets, m->npad_max,
                       m->maxrows, m->d_filt, m->d_map, m->d_state, m->d_rows, m->d_newst, m->d_call, d_out ? 0 : 1);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(m->h_call.data(), m->d_call, sizeof(TsmonCall) * n, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    if (d_out) {
        bool fits = true;
        for (int i = 0; i < n; ++i) fits &= m->h_call[i].needed <= cap;
        if (!fits) {                                   // nothing has been stored: the same call may come again with more room
            for (int i = 0; i < n; ++i) { out_bytes[i] = m->h_call[i].needed; m->nrows[i] = 0; }
            g_err = "TS monitor: the passing packets of a stream do not fit cap (out_bytes holds the sizes)";
            return DVBS2GPU_ERR_CAPACITY;
        }
        hipLaunchKernelGGL(tsmon_emit_kernel, dim3(n), dim3(TSMON_WG), lds_emit, st, a.in(m->d_args), a.out(m->d_args), a.nbytes(m->d_args),
                           m->max_packets, m->maxrows, cap, m->d_filt, m->d_map, m->d_state, m->d_rows, m->d_newst, m->d_call);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipStreamSynchronize(st));
    }
    for (int i = 0; i < n; ++i) {
        tsmon_account(m, i, m->h_call[i]);
        if (out_bytes) out_bytes[i] = d_out ? m->h_call[i].needed : 0;
    }
    return 0;
}

int dvbs2gpu_tsmon_work(dvbs2gpu_tsmon* m, int stream, const uint8_t* h_ts, int nbytes, uint8_t* h_out, int cap) {
    if (!m || stream < 0 || stream >= m->nstreams || nbytes < 0 || cap < 0 || (nbytes > 0 && !h_ts)) return DVBS2GPU_ERR_ARG;
    if (!ts_bank_check_counts("TS monitor: ", &nbytes, 1, m->max_packets)) return DVBS2GPU_ERR_ARG;
    if (h_out && h_out == h_ts) { g_err = "TS monitor: the output buffer is the input"; return DVBS2GPU_ERR_ARG; }
    if (!m->ctx) {
        TsmonCall c;
        std::fill(m->nrows.begin(), m->nrows.end(), 0);    // as on the device: the table is of the LAST call, which brought the others nothing
        if (m->host[stream].run(m->filt[stream], m->map.data() + (size_t)stream * TSMON_MAP_WORDS, h_ts, nbytes / TSMON_TS, h_out, cap, &c) < 0) {
            m->nrows[stream] = 0;
            g_err = "TS monitor: the passing packets do not fit cap";
            return DVBS2GPU_ERR_CAPACITY;
        }
        tsmon_account(m, stream, c);
        return h_out ? c.needed : 0;
    }
    HIP_TRY(hipSetDevice(m->ctx->device));
    return ts_bank_work(m->stage, m->nstreams, stream, h_ts, nbytes, m->max_packets, h_out, cap, false, [&](const uint8_t* const* in, const int* nb, uint8_t* const* out, int* ob) {
        return dvbs2gpu_tsmon_process_batch(m, in, nb, out, cap, ob, nullptr);
    });
}

int dvbs2gpu_tsmon_get_stats(dvbs2gpu_tsmon* m, int stream, dvbs2gpu_tsmon_stats* h_out) {
    if (!m || stream < 0 || stream >= m->nstreams || !h_out) return DVBS2GPU_ERR_ARG;
    *h_out = m->stats[stream];
    return 0;
}

int dvbs2gpu_tsmon_get_pid_table(dvbs2gpu_tsmon* m, int stream, dvbs2gpu_tsmon_pid* h_rows, int cap, int* n) {
    return ts_bank_rows(m, &dvbs2gpu_tsmon::maxrows, stream, h_rows, cap, n);
}

int dvbs2gpu_tsmon_get_pid_table_device(dvbs2gpu_tsmon* m, int stream, const dvbs2gpu_tsmon_pid** d_rows, int* n) {
    return ts_bank_rows_device(m, &dvbs2gpu_tsmon::maxrows, stream, d_rows, n);
}

}  // extern "C"
