// IP-TS bank (own extension; include/dvbs2gpu.h): the UDP datagrams of up to four flows per stream among the IP
// datagrams that the MPE bank, the ULE bank or a GSE path left in HBM with one table row each, their UDP checksum verified, their
// payload recognised as raw TS or RTP/MP2T, an RTP sequence rule applied per flow, and their TS packets laid back to back per flow slot
// in a device buffer that the TS monitor, PSI, PCR, PES and T2-MI banks take as they take any transport stream.  Every rule is in
// ipts_rules.h, whose IptsHostStream is the sequential definition, the host bank and the kernels' yardstick.
//
//   ipts_scan_kernel    one workgroup per stream.
//     A  a wave per input row in turn.  The wave gathers the row's first 128 bytes, two per lane, and every lane evaluates
//        ipts_row_fields on them (rules 1 to 8), a byte read being a shuffle and the header sums a wave sum.  For a row of a watched
//        flow every lane sums its share of the UDP bytes -- a byte-wise lead-in up to a 16-byte boundary, 16-byte loads, a byte-wise
//        tail; the bytes at even and at odd places in two 32-bit sums, so that an odd lead-in only swaps them -- and the wave reduces
//        and folds.  The sync bytes are a lane per TS packet and a ballot, 64 packets a round.  Lane 0 writes the row.
//     B  the sequence rule: one lane per slot walks the slot's RTP rows in table order from the slot's stored state.
//     C  the rows no longer depend on each other: every thread accounts a run of rows, and one prefix sum per slot over the TS rows'
//        bytes gives their offsets.
//   ipts_commit_kernel  (once the host has seen that every slot's bytes fit) one workgroup per stream: a wave per TS row copies its
//     packets to their offset, with 16-byte accesses where source and destination agree modulo 16; then the slots' states are stored.
// Two launches per call and one device-to-host copy, of the call record per stream.  The kernels read nothing outside
// [offset, offset + bytes) of a row: rules 3, 5 and 8 bound every length by the row's byte count before a byte behind it is asked for.
// Static LDS: 0.4 KB.
#include "ip_wave.h"
#include "ipts_rules.h"

#include <memory>

using namespace s2;

static_assert(sizeof(IptsRow) == sizeof(dvbs2gpu_ipts_row) && sizeof(IptsRow) == 40 && IPTS.row_bytes == 40, "row layout");
static_assert(sizeof(IptsView) == sizeof(dvbs2gpu_ipts_view) && sizeof(IptsView) == 40 && IPTS.view_bytes == 40, "view layout");
static_assert(offsetof(IptsView, rows) == offsetof(dvbs2gpu_ipts_view, rows) && offsetof(IptsView, n) == offsetof(dvbs2gpu_ipts_view, n), "view layout");
static_assert(sizeof(IptsLayout) == sizeof(dvbs2gpu_ipts_layout), "layout layout");
static_assert(sizeof(IptsStreamCnt) == IPTS_NSTREAM_CNT * sizeof(int32_t) && sizeof(IptsSlotCnt) == IPTS_NSLOT_CNT * sizeof(int32_t), "counter order");
static_assert(sizeof(dvbs2gpu_ipts_stats) == (IPTS_NSTREAM_CNT + IPTS_NSLOT_CNT) * sizeof(int64_t), "stats order");
static_assert(sizeof(IptsFlow) == 24 && sizeof(IptsSeq) == 16, "flow and state layout");
static_assert(IPTS_KIND_RAW_IP == DVBS2GPU_IPTS_KIND_RAW_IP && IPTS_KIND_GRE == DVBS2GPU_IPTS_KIND_GRE && IPTS_TS == DVBS2GPU_IPTS_TS, "constants");
static_assert(IPTS.gre_header_bytes + 60 + IPTS.udp_header_bytes <= IPTS.head_bytes && IPTS.head_bytes == 128, "the head gather holds what rules 2 to 6 read");

namespace {

constexpr int IPTS_WG = 256, IPTS_WAVES = IPTS_WG / 64, IPTS_NCNT = IPTS_NSTREAM_CNT + IPTS_SLOTS * IPTS_NSLOT_CNT;
static_assert(IPTS_NCNT <= IPTS_WG, "a thread per counter");

// of one stream and call
struct IptsCall { int32_t needed[IPTS_SLOTS]; IptsStreamCnt scnt; IptsSlotCnt cnt[IPTS_SLOTS]; };
static_assert(sizeof(IptsCall) == (IPTS_SLOTS + IPTS_NCNT) * sizeof(int32_t), "the call record is the sizes and then the counters");

// a datagram in a wave: bytes 2 l and 2 l + 1 of its first 128 in lane l, the rest where it lies.  Every lane of the wave calls every
// member with the same arguments (but inside sum's f, where every index is below 128)
struct IptsWaveSrc {
    unsigned h; int lane; const uint8_t* p;
    __device__ unsigned rd(int i) const {
        const unsigned v = (unsigned)__shfl((int)h, (i >> 1) & 63) >> (8 * (i & 1)) & 255u;
        return i < IPTS.head_bytes ? v : p[i];
    }
    template <typename Fn> __device__ unsigned sum(int n, Fn f) const {
        unsigned v = f(lane < n ? lane : 0);
        if (lane >= n) v = 0;
        for (int k = 32; k > 0; k >>= 1) v += (unsigned)__shfl_xor((int)v, k);
        return v;
    }
    // the words' sum of [at, at + len), not folded (ip_wave.h)
    __device__ unsigned wsum(int at, int len) const {
        unsigned even = 0, odd = 0;
        ip_lanes_wsum(p + at, len, lane, 64, &even, &odd);
        return ip_wave_wsum_reduce(even, odd);
    }
    __device__ bool syncs(int at, int n) const {
        bool ok = true;
        for (int k0 = 0; k0 < n; k0 += 64) {
            const int k = k0 + lane;
            const bool bad = k < n && p[at + IPTS.ts_packet_bytes * k] != IPTS.ts_sync;
            ok &= __ballot(bad) == 0;
        }
        return ok;
    }
};

__device__ inline int ipts_row_i32(const IptsView& v, int r, int at) { return *reinterpret_cast<const int*>(v.rows + (size_t)r * v.stride + at); }

__global__ void __launch_bounds__(IPTS_WG) ipts_scan_kernel(const IptsView* __restrict__ views, int max_rows, const IptsFlow* __restrict__ flows,
                                                            const IptsSeq* __restrict__ state, IptsSeq* __restrict__ newst, IptsRow* __restrict__ rows_g,
                                                            IptsCall* __restrict__ call, int have_out) {
    __shared__ int cnt[IPTS_NCNT], wsum[IPTS_WAVES];
    __shared__ IptsFlow fl[IPTS_SLOTS];
    const int s = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const IptsView v = views[s];
    const int n = v.n < max_rows ? v.n : max_rows;   // (the host has refused a longer table)
    IptsRow* rows = rows_g + (size_t)s * max_rows;
    if (tid < IPTS_NCNT) cnt[tid] = 0;
    if (tid < IPTS_SLOTS) fl[tid] = flows[s * IPTS_SLOTS + tid];
    __syncthreads();
    // A: rules 1 to 8, a wave per row
    for (int r = wave; r < n; r += IPTS_WAVES) {
        const int off = ipts_row_i32(v, r, v.offset_at), nb = ipts_row_i32(v, r, v.bytes_at);
        const uint8_t* p = v.bytes + (off < 0 ? 0 : off);
        unsigned h = 0;
        if (off >= 0) {
            if (2 * lane < nb) h = p[2 * lane];
            if (2 * lane + 1 < nb) h |= (unsigned)p[2 * lane + 1] << 8;
        }
        const IptsRow row = ipts_row_fields(IptsWaveSrc{h, lane, p}, off, nb, v.kind, fl);
        if (lane == 0) rows[r] = row;
    }
    __syncthreads();
    // B: rule 9, a lane per slot
    if (tid < IPTS_SLOTS) {
        IptsSeq st = state[s * IPTS_SLOTS + tid];
        for (int r = 0; r < n; ++r) {
            if (rows[r].slot != tid || !(rows[r].flags & IPTS_RTP)) continue;
            IptsRow q = rows[r];
            ipts_seq_step(st, q);
            rows[r] = q;
        }
        newst[s * IPTS_SLOTS + tid] = st;
    }
    __syncthreads();
    // C: the counters, and rule 10: the offsets of the TS rows of each slot
    int r0, r1; ts_thread_run(n, IPTS_WG, &r0, &r1);
    int mine[IPTS_SLOTS] = {0, 0, 0, 0};
    for (int r = r0; r < r1; ++r) {
        const IptsRow q = rows[r];
        ipts_account(q, have_out != 0, [&](int c) { atomicAdd(&cnt[c], 1); },
                     [&](int c, int a) { atomicAdd(&cnt[IPTS_NSTREAM_CNT + IPTS_NSLOT_CNT * q.slot + c], a); });
        for (int k = 0; k < IPTS_SLOTS; ++k) mine[k] += have_out && (q.flags & IPTS_TS) && q.slot == k ? q.bytes : 0;
    }
    int needed[IPTS_SLOTS];
    for (int k = 0; k < IPTS_SLOTS; ++k) {
        int at = ts_block_scan<IPTS_WG>(mine[k], wsum, &needed[k]);
        if (mine[k] == 0) continue;
        for (int r = r0; r < r1; ++r)
            if ((rows[r].flags & IPTS_TS) && rows[r].slot == k) { rows[r].offset = at; at += rows[r].bytes; }
    }
    __syncthreads();
    int32_t* rec = reinterpret_cast<int32_t*>(call + s);
    if (tid < IPTS_SLOTS) rec[tid] = needed[tid];
    if (tid < IPTS_NCNT) rec[IPTS_SLOTS + tid] = cnt[tid];
}

__global__ void __launch_bounds__(IPTS_WG) ipts_commit_kernel(const IptsView* __restrict__ views, uint8_t* const* __restrict__ out, int max_rows, int cap,
                                                              IptsSeq* __restrict__ state, const IptsSeq* __restrict__ newst, const IptsRow* __restrict__ rows_g) {
    const int s = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const IptsView v = views[s];
    const int n = v.n < max_rows ? v.n : max_rows;
    const IptsRow* rows = rows_g + (size_t)s * max_rows;
    for (int r = wave; out && r < n; r += IPTS_WAVES) {
        const IptsRow q = rows[r];
        if (!(q.flags & IPTS_TS) || q.offset < 0 || q.bytes <= 0 || q.offset + q.bytes > cap) continue;
        uint8_t* o = out[s * IPTS_SLOTS + q.slot];
        if (!o) continue;
        ip_lanes_copy(o + q.offset, v.bytes + ipts_row_i32(v, r, v.offset_at) + q.ts_at, q.bytes, lane, 64);
    }
    if (tid < IPTS_SLOTS) state[s * IPTS_SLOTS + tid] = newst[s * IPTS_SLOTS + tid];
}

constexpr const char* BANK = "IP-TS bank: ";
int fail_arg(const char* text) { last_error() = std::string(BANK) + text; return DVBS2GPU_ERR_ARG; }

}  // namespace

struct dvbs2gpu_ipts {
    dvbs2gpu_ctx* ctx = nullptr;                   // null: a host-only bank (dvbs2gpu_ipts_create_host)
    int nstreams = 0, max_rows = 0;
    std::vector<IptsFlow> flow;                    // nstreams x 4
    std::vector<int64_t> stats;                    // nstreams x IPTS_NCNT, since reset (a slot's since its last set_flow), in the order of IptsCall's counters
    std::vector<int> nrows, need_bytes;            // of the last call: per stream, per (stream, slot)
    std::vector<IptsCall> h_call;
    std::vector<char> h_args;                      // IptsView x nstreams | uint8_t* x 4 nstreams
    // device banks
    DevBuf<IptsFlow> d_flow;
    DevBuf<IptsSeq> d_state, d_newst;
    DevBuf<IptsRow> d_rows;                        // nstreams x max_rows
    DevBuf<IptsCall> d_call;
    DevBuf<char> d_args;
    Workspace st_bytes, st_rows, st_out;           // of the host-buffer entry point
    // host-only banks
    std::vector<IptsHostStream> host;

    size_t out_at() const { return sizeof(IptsView) * (size_t)nstreams; }
    void account_call(int s, const IptsCall& c) {
        const int32_t* a = reinterpret_cast<const int32_t*>(&c.scnt);
        for (int k = 0; k < IPTS_NCNT; ++k) stats[(size_t)s * IPTS_NCNT + k] += a[k];
    }
};

namespace {

// the view of one stream as a call may hold it
bool view_ok(const dvbs2gpu_ipts* b, const dvbs2gpu_ipts_view& v) {
    if (v.n < 0 || v.n > b->max_rows) { fail_arg("a view has 0 .. max_rows rows"); return false; }
    if (v.kind != IPTS_KIND_RAW_IP && v.kind != IPTS_KIND_GRE) { fail_arg("a view's kind is RAW_IP or GRE"); return false; }
    if (v.n == 0) return true;
    const bool fields = v.stride >= 4 && v.stride % 4 == 0 && v.offset_at >= 0 && v.offset_at % 4 == 0 && v.offset_at + 4 <= v.stride && v.bytes_at >= 0 &&
                        v.bytes_at % 4 == 0 && v.bytes_at + 4 <= v.stride;
    if (!v.bytes || !v.rows || (reinterpret_cast<uintptr_t>(v.rows) & 3) || !fields) {
        fail_arg("a view with rows needs bytes, a row table at a multiple of 4 and two int32 fields at multiples of 4 inside the stride");
        return false;
    }
    return true;
}

// the device call: views and d_out (4 pointers per stream, or null) are host arrays
int ipts_batch(dvbs2gpu_ipts* b, const dvbs2gpu_ipts_view* views, uint8_t* const* d_out, int cap, int* out_bytes, int* out_rows, hipStream_t st) {
    const int n = b->nstreams, ns = n * IPTS_SLOTS;
    HIP_TRY(hipSetDevice(b->ctx->device));
    memcpy(b->h_args.data(), views, sizeof(IptsView) * (size_t)n);
    uint8_t** po = reinterpret_cast<uint8_t**>(b->h_args.data() + b->out_at());
    for (int g = 0; g < ns; ++g) po[g] = d_out ? d_out[g] : nullptr;
    HIP_TRY(hipMemcpyAsync(b->d_args, b->h_args.data(), b->h_args.size(), hipMemcpyHostToDevice, st));
    const IptsView* dv = reinterpret_cast<const IptsView*>(b->d_args.get());
    hipLaunchKernelGGL(ipts_scan_kernel, dim3(n), dim3(IPTS_WG), 0, st, dv, b->max_rows, b->d_flow, b->d_state, b->d_newst, b->d_rows, b->d_call, d_out ? 1 : 0);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(b->h_call.data(), b->d_call, sizeof(IptsCall) * (size_t)n, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    bool fits = true;
    for (int g = 0; g < ns; ++g) {
        const int need = b->h_call[g / IPTS_SLOTS].needed[g % IPTS_SLOTS];
        fits &= !d_out || need <= cap;
        b->need_bytes[g] = need;
        if (out_bytes) out_bytes[g] = need;
    }
    for (int i = 0; out_rows && i < n; ++i) out_rows[i] = views[i].n;
    if (!fits) {                                       // nothing has been stored: the same call may come again with more room
        std::fill(b->nrows.begin(), b->nrows.end(), 0);
        last_error() = std::string(BANK) + "the TS packets of a slot do not fit cap (out_bytes holds the sizes)";
        return DVBS2GPU_ERR_CAPACITY;
    }
    hipLaunchKernelGGL(ipts_commit_kernel, dim3(n), dim3(IPTS_WG), 0, st, dv, d_out ? reinterpret_cast<uint8_t* const*>(b->d_args.get() + b->out_at()) : nullptr,
                       b->max_rows, cap, b->d_state, b->d_newst, b->d_rows);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(st));
    for (int i = 0; i < n; ++i) { b->account_call(i, b->h_call[i]); b->nrows[i] = views[i].n; }
    return 0;
}

int ipts_create(dvbs2gpu_ctx* ctx, int nstreams, int max_rows, dvbs2gpu_ipts** out) {
    if (!out || nstreams <= 0 || max_rows <= 0) return DVBS2GPU_ERR_ARG;
    if (max_rows > IPTS_MAX_ROWS) return fail_arg("max_rows is at most 16384 per stream and call");
    if (ctx) HIP_TRY(hipSetDevice(ctx->device));
    std::unique_ptr<dvbs2gpu_ipts> b(new dvbs2gpu_ipts());
    const size_t n = (size_t)nstreams, ns = n * IPTS_SLOTS;
    b->ctx = ctx; b->nstreams = nstreams; b->max_rows = max_rows;
    b->flow.assign(ns, IptsFlow{});
    b->stats.assign(n * IPTS_NCNT, 0);
    b->nrows.assign(n, 0); b->need_bytes.assign(ns, 0);
    b->h_call.resize(n);
    if (!ctx) {
        b->host.resize(n);
        *out = b.release();
        return 0;
    }
    const char* what = "hipMalloc(ipts)";              // (zero-filled: the flows and the slots' states; the kernels write the rest before it is read)
    RC_TRY(b->d_flow.alloc(ns, true, what));
    RC_TRY(b->d_state.alloc(ns, true, what));
    RC_TRY(b->d_newst.alloc(ns, false, what));
    RC_TRY(b->d_rows.alloc(n * max_rows, false, what));
    RC_TRY(b->d_call.alloc(n, false, what));
    b->h_args.resize(b->out_at() + sizeof(uint8_t*) * ns);
    RC_TRY(b->d_args.alloc(b->h_args.size(), false, what));
    *out = b.release();
    return 0;
}

}  // namespace

extern "C" {

void dvbs2gpu_ipts_destroy(dvbs2gpu_ipts* b) { delete b; }
int dvbs2gpu_ipts_create(dvbs2gpu_ctx* ctx, int nstreams, int max_rows, dvbs2gpu_ipts** out) { return ctx ? ipts_create(ctx, nstreams, max_rows, out) : DVBS2GPU_ERR_ARG; }
int dvbs2gpu_ipts_create_host(int nstreams, int max_rows, dvbs2gpu_ipts** out) { return ipts_create(nullptr, nstreams, max_rows, out); }

int dvbs2gpu_ipts_reset(dvbs2gpu_ipts* b) {
    if (!b) return DVBS2GPU_ERR_ARG;
    if (b->ctx) {
        HIP_TRY(hipSetDevice(b->ctx->device));
        HIP_TRY(hipMemset(b->d_state, 0, (size_t)b->nstreams * IPTS_SLOTS * sizeof(IptsSeq)));
    }
    for (IptsHostStream& h : b->host) h.clear();
    std::fill(b->stats.begin(), b->stats.end(), 0);
    std::fill(b->nrows.begin(), b->nrows.end(), 0);
    return 0;
}

int dvbs2gpu_ipts_get_layout(dvbs2gpu_ipts_layout* h_out) {
    if (!h_out) return DVBS2GPU_ERR_ARG;
    memcpy(h_out, &IPTS, sizeof(IPTS));
    return 0;
}

int dvbs2gpu_ipts_set_flow(dvbs2gpu_ipts* b, int stream, int slot, int family, const uint8_t dst_addr[16], int dst_port) {
    if (!b || stream < 0 || stream >= b->nstreams || slot < 0 || slot >= IPTS_SLOTS) return DVBS2GPU_ERR_ARG;
    if (family != 0 && family != 4 && family != 6) return fail_arg("a flow's family is 4, 6 or 0 (the slot is empty)");
    if (family && (!dst_addr || dst_port < 0 || dst_port > 65535)) return fail_arg("a flow needs a destination address and a port 0..65535");
    const size_t at = (size_t)stream * IPTS_SLOTS + slot;
    IptsFlow f = {};
    if (family) {
        f.family = family; f.port = dst_port;
        memcpy(f.addr, dst_addr, family == 4 ? 4 : 16);
    }
    b->flow[at] = f;
    std::fill_n(b->stats.begin() + (size_t)stream * IPTS_NCNT + IPTS_NSTREAM_CNT + (size_t)slot * IPTS_NSLOT_CNT, IPTS_NSLOT_CNT, 0);
    if (b->ctx) {
        HIP_TRY(hipSetDevice(b->ctx->device));
        HIP_TRY(hipMemcpy(b->d_flow + at, &f, sizeof(f), hipMemcpyHostToDevice));
        HIP_TRY(hipMemset(b->d_state + at, 0, sizeof(IptsSeq)));
    } else {
        b->host[stream].flow[slot] = f;
        b->host[stream].seq[slot] = IptsSeq{};
    }
    return 0;
}

int dvbs2gpu_ipts_process_batch(dvbs2gpu_ipts* b, const dvbs2gpu_ipts_view* views, uint8_t* const* d_out, int cap, int* out_bytes, int* out_rows, void* stream) {
    if (!b || !views || cap < 0 || (d_out && !out_bytes)) return DVBS2GPU_ERR_ARG;
    if (!b->ctx) return fail_arg("a host bank takes host buffers (dvbs2gpu_ipts_work)");
    for (int i = 0; i < b->nstreams; ++i) {
        if (!view_ok(b, views[i])) return DVBS2GPU_ERR_ARG;
        // once d_out is given every slot with a flow needs its output pointer, one of a stream with an empty view too
        for (int k = 0; d_out && k < IPTS_SLOTS; ++k) {
            const uint8_t* o = d_out[i * IPTS_SLOTS + k];
            if ((b->flow[(size_t)i * IPTS_SLOTS + k].family && !o) || (o && o == views[i].bytes)) return fail_arg("null buffer, or an output buffer that is its stream's input");
        }
    }
    return ipts_batch(b, views, d_out, cap, out_bytes, out_rows, (hipStream_t)stream);
}

int dvbs2gpu_ipts_work(dvbs2gpu_ipts* b, int stream, const dvbs2gpu_ipts_view* h_view, uint8_t* const* h_out, int cap, int* out_bytes) {
    if (!b || stream < 0 || stream >= b->nstreams || !h_view || cap < 0 || !view_ok(b, *h_view)) return DVBS2GPU_ERR_ARG;
    for (int k = 0; h_out && k < IPTS_SLOTS; ++k)
        if (b->flow[(size_t)stream * IPTS_SLOTS + k].family && !h_out[k]) return fail_arg("null buffer of a slot with a flow");
    IptsView v;
    memcpy(&v, h_view, sizeof(v));
    int* need = b->need_bytes.data() + (size_t)stream * IPTS_SLOTS;
    if (!b->ctx) {
        IptsHostStream& h = b->host[stream];
        std::fill(b->nrows.begin(), b->nrows.end(), 0);        // the tables are of the LAST call, which brought the other streams nothing
        IptsSeq before[IPTS_SLOTS];
        memcpy(before, h.seq, sizeof(before));                 // what a capacity failure has to put back
        h.run(v, h_out != nullptr);
        bool fits = true;
        for (int k = 0; k < IPTS_SLOTS; ++k) {
            need[k] = (int)h.bytes[k].size();
            if (out_bytes) out_bytes[k] = need[k];
            fits &= need[k] <= cap;
        }
        if (!fits) {
            memcpy(h.seq, before, sizeof(before));
            h.clear_call();
            last_error() = std::string(BANK) + "the TS packets of a slot do not fit cap (dvbs2gpu_ipts_get_needed holds the sizes)";
            return DVBS2GPU_ERR_CAPACITY;
        }
        IptsCall c = {};
        c.scnt = h.scnt;
        memcpy(c.cnt, h.cnt, sizeof(c.cnt));
        b->account_call(stream, c);
        b->nrows[stream] = (int)h.rows.size();
        for (int k = 0; h_out && k < IPTS_SLOTS; ++k)
            if (!h.bytes[k].empty()) memcpy(h_out[k], h.bytes[k].data(), h.bytes[k].size());
        return 0;
    }
    // a device bank: the view's bytes, up to the end of its last row, and its table staged; the other streams take an empty view
    HIP_TRY(hipSetDevice(b->ctx->device));
    size_t extent = 0;
    for (int r = 0; r < v.n; ++r) {
        const int off = ipts_view_i32(v, r, v.offset_at), nb = ipts_view_i32(v, r, v.bytes_at);
        if (off >= 0 && nb > 0 && (size_t)off + nb > extent) extent = (size_t)off + nb;
    }
    const size_t slot_room = ((size_t)cap + 31) & ~(size_t)15;
    RC_TRY(b->st_bytes.ensure(extent + 16));
    RC_TRY(b->st_rows.ensure((size_t)v.n * v.stride + 16));
    if (h_out) RC_TRY(b->st_out.ensure(slot_room * IPTS_SLOTS));
    if (extent) HIP_TRY(hipMemcpy(b->st_bytes.p, v.bytes, extent, hipMemcpyHostToDevice));
    if (v.n) HIP_TRY(hipMemcpy(b->st_rows.p, v.rows, (size_t)v.n * v.stride, hipMemcpyHostToDevice));
    std::vector<dvbs2gpu_ipts_view> views(b->nstreams, dvbs2gpu_ipts_view{});
    views[stream] = *h_view;
    views[stream].bytes = static_cast<const uint8_t*>(b->st_bytes.p);
    views[stream].rows = b->st_rows.p;
    std::vector<uint8_t*> out((size_t)b->nstreams * IPTS_SLOTS, nullptr);
    for (int k = 0; h_out && k < IPTS_SLOTS; ++k) out[(size_t)stream * IPTS_SLOTS + k] = static_cast<uint8_t*>(b->st_out.p) + slot_room * k;
    std::vector<int> ob(out.size(), 0);
    const int rc = ipts_batch(b, views.data(), h_out ? out.data() : nullptr, cap, ob.data(), nullptr, nullptr);
    for (int k = 0; out_bytes && k < IPTS_SLOTS; ++k) out_bytes[k] = need[k];
    if (rc < 0) return rc;
    for (int k = 0; h_out && k < IPTS_SLOTS; ++k)
        if (need[k] > 0) HIP_TRY(hipMemcpy(h_out[k], out[(size_t)stream * IPTS_SLOTS + k], need[k], hipMemcpyDeviceToHost));
    return 0;
}

int dvbs2gpu_ipts_get_needed(dvbs2gpu_ipts* b, int stream, int slot, int* bytes) {
    if (!b || stream < 0 || stream >= b->nstreams || slot < 0 || slot >= IPTS_SLOTS || !bytes) return DVBS2GPU_ERR_ARG;
    *bytes = b->need_bytes[(size_t)stream * IPTS_SLOTS + slot];
    return 0;
}

int dvbs2gpu_ipts_get_stats(dvbs2gpu_ipts* b, int stream, int slot, dvbs2gpu_ipts_stats* h_out) {
    if (!b || stream < 0 || stream >= b->nstreams || slot < -1 || slot >= IPTS_SLOTS || !h_out) return DVBS2GPU_ERR_ARG;
    *h_out = dvbs2gpu_ipts_stats{};
    int64_t* d = reinterpret_cast<int64_t*>(h_out);
    const int64_t* a = b->stats.data() + (size_t)stream * IPTS_NCNT;
    for (int k = 0; slot < 0 && k < IPTS_NSTREAM_CNT; ++k) d[k] = a[k];
    for (int s = slot < 0 ? 0 : slot; s < (slot < 0 ? IPTS_SLOTS : slot + 1); ++s)
        for (int k = 0; k < IPTS_NSLOT_CNT; ++k) d[IPTS_NSTREAM_CNT + k] += a[IPTS_NSTREAM_CNT + s * IPTS_NSLOT_CNT + k];
    return 0;
}

int dvbs2gpu_ipts_get_row_table(dvbs2gpu_ipts* b, int stream, dvbs2gpu_ipts_row* h_rows, int cap, int* n) {
    return ts_bank_rows(b, &dvbs2gpu_ipts::max_rows, stream, h_rows, cap, n);
}
int dvbs2gpu_ipts_get_row_table_device(dvbs2gpu_ipts* b, int stream, const dvbs2gpu_ipts_row** d_rows, int* n) {
    return ts_bank_rows_device(b, &dvbs2gpu_ipts::max_rows, stream, d_rows, n);
}

}  // extern "C"
