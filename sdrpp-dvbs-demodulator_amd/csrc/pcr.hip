// PCR bank (own extension; include/dvbs2gpu.h): PCR interval, discontinuity and accuracy checks on up to 16 watched
// PIDs of each of `nstreams` transport streams in HBM.  Every rule is in pcr_rules.h, whose PcrHostStream is the sequential
// definition, the host bank and the kernel's yardstick; this file says how a call's packets are taken in parallel.
//
// What makes the parallel form possible: behind ANY record the slot's last_pcr is that record's own value (FIRST, ANNOUNCED, OK, LATE
// and JUMP store it, REPEATED found it equal), so a record's kind needs only the value of the record before it on its slot.  The one
// thing that reaches further is ref_n behind a run of REPEATED records: the position of the last record before it that was not one.
//
//   pcr_kernel  one workgroup per stream, one launch per call.
//     A  every packet's header is read once (ts_load_header, ts_bank.h); a packet with an adaptation field reads the field's flags
//        and one with the PCR flag one dword more (ts_load_header_dword).  Its PID is matched against the 16 watches.  The records --
//        well-formed PCR packets of watched PIDs -- are compacted in input order into LDS, one 64-bit word each (value, packet, slot,
//        DI): flags in a mask, ts_block_scan, scatter.  The input-order index is the row number.
//     B  a stable counting sort by slot: every thread counts the slots of a contiguous run of records, one prefix sum over the
//        16 x 256 counts in slot-major order gives every (slot, thread) its first place, and the threads place their records.  What
//        is sorted is a 16-bit index, the records stay where they are.
//     C  every thread takes a contiguous run of the sorted records.  The record before one in sorted order is its slot's previous
//        record, or the record is its slot's first of the call and takes the carried state.  A first pass finds the last record of
//        the thread's run that is not REPEATED, an exclusive maximum scan over the threads makes of it "the last record before mine
//        that is not REPEATED"; where that lies in the record's own slot run it gives ref_n, else the carried ref_n does.  The second
//        pass steps every record in its own lane (pcr_step), writes its row and sums the counters per thread and slot run, then into
//        LDS.  The slot's last record writes the slot's new state.
// No lane walks over packets or records of other lanes: the cost of a call does not depend on what the PCRs say.  One device-to-host
// copy of the per-stream call record (PcrCall).
#include "ts_bank.h"
#include "pcr_rules.h"

using namespace s2;
#define g_err last_error()

namespace s2 {

constexpr int PCR_MAX_PACKETS = 4096;            // per stream and call: 10 bytes of LDS per packet
constexpr int PCR_WG = 256;
static_assert(sizeof(PcrRow) == sizeof(dvbs2gpu_pcr_row) && sizeof(PcrRow) == 32, "row layout");
static_assert(PCR_MAX_PACKETS <= 16 * PCR_WG, "a thread's record flags are 16 bits of a mask, its slot counts 16-bit words (ts_thread_run)");
static_assert(PCR_MOD < (1ull << 42), "a record is a PCR value in 42 bits, the packet in 12, the slot in 4 and DI");
static_assert(PCR_ACCURACY_ERROR == DVBS2GPU_PCR_ACCURACY_ERROR && PCR_SATURATED == DVBS2GPU_PCR_SATURATED && PCR_JUMP == DVBS2GPU_PCR_JUMP, "public values");

struct PcrCall { PcrCallHead head; PcrCnt cnt[PCR_SLOTS]; };

// a record in LDS: P bits 0-41, packet k 42-53, slot 54-57, DI 58
__device__ inline uint64_t rec_p(uint64_t e) { return e & ((1ull << 42) - 1); }
__device__ inline int rec_k(uint64_t e) { return (int)(e >> 42 & 4095); }
__device__ inline int rec_slot(uint64_t e) { return (int)(e >> 54 & 15); }
__device__ inline int rec_di(uint64_t e) { return (int)(e >> 58 & 1); }

// what the kernel keeps in LDS beside the records; a multiple of 16 bytes in front of them
struct alignas(16) PcrShared {
    PcrCnt cnt[PCR_SLOTS];
    PcrState ss[PCR_SLOTS];                      // the slots' states before the call
    uint16_t place[PCR_SLOTS][PCR_WG];           // the counting sort's counts, then places
    int32_t w[PCR_SLOTS];
    int32_t start[PCR_SLOTS + 1];                // the slots' runs in sorted order
    int32_t wsum[PCR_WG / 64];
    int32_t unwatched; uint32_t first_unwatched; // (packet << 13 | PID) of the first one
    int64_t pos0;
    PcrRate rate;
};
static_assert(sizeof(PcrShared) % 16 == 0, "the records behind it are 64-bit words");

// packet k of the stream: PCR_NONE, or PCR_GOOD / PCR_MALFORMED with its PID; *slot: the watching slot or -1
__device__ inline int pcr_look(const uint8_t* __restrict__ ts, int k, const int32_t* w, uint64_t* P, int* slot, int* pid, int* di) {
    unsigned b4;
    const TsmonHdr h = ts_load_header(ts, k, &b4);
    if (h.cls != TSMON_DATA || !(h.afc & 2) || b4 < 1) return PCR_NONE;
    const unsigned w1 = ts_load_header_dword(ts, k, 1);
    if (!(w1 & 0x1000)) return PCR_NONE;
    const unsigned w2 = ts_load_header_dword(ts, k, 2);
    const uint8_t b[8] = {(uint8_t)w1, (uint8_t)(w1 >> 8), (uint8_t)(w1 >> 16), (uint8_t)(w1 >> 24), (uint8_t)w2, (uint8_t)(w2 >> 8), (uint8_t)(w2 >> 16), (uint8_t)(w2 >> 24)};
    *slot = -1;
    for (int s = 0; s < PCR_SLOTS; ++s) if (w[s] == h.pid) *slot = s;
    *pid = h.pid; *di = h.di;
    return pcr_parse(h.afc, b, P);
}

__device__ inline void pcr_flush(PcrCnt* d, const PcrCnt& a) {
    for (int i = 0; i < PCR_KINDS; ++i) if (a.kind[i]) atomicAdd(&d->kind[i], a.kind[i]);
    if (a.accuracy_measured) atomicAdd(&d->accuracy_measured, a.accuracy_measured);
    if (a.accuracy_errors) atomicAdd(&d->accuracy_errors, a.accuracy_errors);
    if (a.max_delta_ticks) atomicMax(&d->max_delta_ticks, a.max_delta_ticks);
    if (a.max_abs_accuracy) atomicMax(&d->max_abs_accuracy, a.max_abs_accuracy);
    if (a.sum_ticks) atomicAdd(reinterpret_cast<unsigned long long*>(&d->sum_ticks), (unsigned long long)a.sum_ticks);
    if (a.sum_packets) atomicAdd(reinterpret_cast<unsigned long long*>(&d->sum_packets), (unsigned long long)a.sum_packets);
    if (a.last_k >= 0) d->last_k = a.last_k;      // one lane per slot has it
}

// dynamic LDS: PcrShared, rec[max_packets] (64 bits each), order[max_packets] (16 bits each)
__global__ void __launch_bounds__(PCR_WG) pcr_kernel(const uint8_t* const* __restrict__ in, const int* __restrict__ nbytes, int max_packets, int max_rows,
                                                     const int32_t* __restrict__ watch, const PcrRate* __restrict__ rate, PcrState* __restrict__ state,
                                                     int64_t* __restrict__ pos, PcrRow* __restrict__ rows_g, PcrCall* __restrict__ call) {
    extern __shared__ __attribute__((aligned(16))) unsigned char pcr_lds[];
    PcrShared& sh = *reinterpret_cast<PcrShared*>(pcr_lds);
    uint64_t* rec = reinterpret_cast<uint64_t*>(pcr_lds + sizeof(PcrShared));
    uint16_t* order = reinterpret_cast<uint16_t*>(rec + max_packets);
    const int s = blockIdx.x, tid = threadIdx.x;
    int n = nbytes[s] / TSMON_TS;
    if (n > max_packets) n = max_packets;            // (the host has refused such a call)
    if (tid < PCR_SLOTS) {
        sh.w[tid] = watch[(size_t)s * PCR_SLOTS + tid];
        sh.ss[tid] = state[(size_t)s * PCR_SLOTS + tid];
        sh.cnt[tid] = pcr_cnt_zero();
    }
    if (tid == 0) { sh.unwatched = 0; sh.first_unwatched = 0xFFFFFFFFu; sh.pos0 = pos[s]; sh.rate = rate[s]; }
    __syncthreads();
    const uint8_t* ts = in[s];
    // A: the records, compacted in input order
    int W = 0;
    if (n > 0) {
        int k0, k1; ts_thread_run(n, PCR_WG, &k0, &k1);          // <= 16 packets per thread
        unsigned mask = 0, first_unw = 0xFFFFFFFFu;
        int unw = 0;
        for (int k = k0; k < k1; ++k) {
            uint64_t P; int slot, pid, di;
            const int v = pcr_look(ts, k, sh.w, &P, &slot, &pid, &di);
            if (v == PCR_NONE) continue;
            if (slot < 0) {
                if (v == PCR_GOOD && !unw++) first_unw = (unsigned)k << 13 | (unsigned)pid;
            } else if (v == PCR_MALFORMED) atomicAdd(&sh.cnt[slot].malformed, 1);
            else mask |= 1u << (k - k0);
        }
        if (unw) { atomicAdd(&sh.unwatched, unw); atomicMin(&sh.first_unwatched, first_unw); }
        int at = ts_block_scan<PCR_WG>(__popc(mask), sh.wsum, &W);
        for (int k = k0; k < k1; ++k) {
            if (!(mask >> (k - k0) & 1)) continue;
            uint64_t P = 0; int slot = 0, pid, di = 0;
            pcr_look(ts, k, sh.w, &P, &slot, &pid, &di);
            rec[at++] = P | (uint64_t)k << 42 | (uint64_t)slot << 54 | (uint64_t)di << 58;
        }
    }
    __syncthreads();
    if (W > 0) {
        // B: the stable counting sort by slot
        int r0, r1; ts_thread_run(W, PCR_WG, &r0, &r1);
        for (int q = 0; q < PCR_SLOTS; ++q) sh.place[q][tid] = 0;
        for (int r = r0; r < r1; ++r) ++sh.place[rec_slot(rec[r])][tid];
        __syncthreads();
        {
            uint16_t* flat = &sh.place[0][0] + PCR_SLOTS * tid;    // slot-major: 16 threads' counts of one slot
            int sum = 0, total;
            for (int i = 0; i < PCR_SLOTS; ++i) sum += flat[i];
            int at = ts_block_scan<PCR_WG>(sum, sh.wsum, &total);
            for (int i = 0; i < PCR_SLOTS; ++i) { const int c = flat[i]; flat[i] = (uint16_t)at; at += c; }
        }
        __syncthreads();
        if (tid < PCR_SLOTS) sh.start[tid] = sh.place[tid][0];
        if (tid == PCR_SLOTS) sh.start[PCR_SLOTS] = W;
        __syncthreads();
        for (int r = r0; r < r1; ++r) order[sh.place[rec_slot(rec[r])][tid]++] = (uint16_t)r;
        __syncthreads();
        // C: every record in its own lane
        const int64_t pos0 = sh.pos0;
        const PcrRate rt = sh.rate;
        int j0, j1; ts_thread_run(W, PCR_WG, &j0, &j1);
        // the state in front of sorted record j, but for ref_n
        auto before = [&](int j, uint64_t e) {
            const int slot = rec_slot(e);
            if (j == sh.start[slot]) return sh.ss[slot];
            return PcrState{rec_p(rec[order[j - 1]]), 0, 1, 0};
        };
        int mine = -1;
        for (int j = j0; j < j1; ++j) {
            const uint64_t e = rec[order[j]];
            const PcrState st = before(j, e);
            if (!(st.seen && !rec_di(e) && rec_p(e) == st.last_pcr)) mine = j;
        }
        int last = ts_block_scan_max(mine, sh.wsum);             // the last sorted record before j that is not REPEATED
        PcrCnt acc = pcr_cnt_zero();
        int acc_slot = -1;
        PcrRow* rows = rows_g + (size_t)s * max_rows;
        for (int j = j0; j < j1; ++j) {
            const int rank = order[j];
            const uint64_t e = rec[rank];
            const int slot = rec_slot(e), k = rec_k(e);
            PcrState st = before(j, e);
            st.ref_n = last >= sh.start[slot] ? pos0 + rec_k(rec[order[last]]) : sh.ss[slot].ref_n;
            PcrRow row = {(uint16_t)sh.w[slot], (uint8_t)slot, 0, 0, 0, k, rec_p(e), 0, 0, 0};
            const PcrState nx = pcr_step(st, rec_p(e), pos0 + k, rec_di(e), rt, &row);
            if (row.kind != PCR_REPEATED) last = j;
            if (slot != acc_slot) {
                if (acc_slot >= 0) pcr_flush(&sh.cnt[acc_slot], acc);
                acc = pcr_cnt_zero(); acc_slot = slot;
            }
            pcr_cnt_add(&acc, row, rt.tpp != 0);
            if (rank < max_rows) rows[rank] = row;
            if (j == sh.start[slot + 1] - 1) { state[(size_t)s * PCR_SLOTS + slot] = nx; acc.last_k = k; }
        }
        if (acc_slot >= 0) pcr_flush(&sh.cnt[acc_slot], acc);
        __syncthreads();
    }
    if (tid < PCR_SLOTS) call[s].cnt[tid] = sh.cnt[tid];
    if (tid == 0) {
        call[s].head = PcrCallHead{W, sh.unwatched, sh.unwatched ? (int32_t)(sh.first_unwatched & 0x1fff) : -1, 0};
        pos[s] = sh.pos0 + n;
    }
}

}  // namespace s2

struct dvbs2gpu_pcr {
    dvbs2gpu_ctx* ctx = nullptr;                   // null: a host-only bank (dvbs2gpu_pcr_create_host)
    int nstreams = 0, max_packets = 0, max_rows = 0;
    std::vector<int32_t> watch;                    // nstreams x 16
    std::vector<PcrRate> rate;
    std::vector<dvbs2gpu_pcr_stats> stats;         // nstreams x 16, since reset; the kernel reports each call's share (PcrCall)
    std::vector<dvbs2gpu_pcr_stream_stats> sstats; // packets_since_pcr holds the position of the slot's last record, -1: none
    std::vector<int> nrows, records;               // of the last call per stream: rows in the table, records in all
    std::vector<PcrCall> h_call;
    std::vector<char> h_args;
    // device banks
    DevBuf<int32_t> d_watch;
    DevBuf<PcrRate> d_rate;
    DevBuf<PcrState> d_state;
    DevBuf<int64_t> d_pos;
    DevBuf<PcrRow> d_rows;                         // nstreams x max_rows
    DevBuf<PcrCall> d_call;
    DevBuf<uint8_t> d_args;                        // TsBankArgs(nstreams)
    TsHostStage stage;                             // of the host-buffer entry point
    // host-only banks
    std::vector<PcrHostStream> host;
};

namespace s2 {
static_assert(sizeof(dvbs2gpu_pcr_stats) == 14 * sizeof(int64_t), "stats order");
// one stream's call into its statistics; `n` packets came
static void pcr_account(dvbs2gpu_pcr* b, int i, int n, const PcrCallHead& head, const PcrCnt* c) {
    dvbs2gpu_pcr_stream_stats& ss = b->sstats[i];
    for (int s = 0; s < PCR_SLOTS; ++s) {
        dvbs2gpu_pcr_stats& d = b->stats[(size_t)i * PCR_SLOTS + s];
        const PcrCnt& a = c[s];
        int64_t* dk[PCR_KINDS] = {&d.first, &d.announced, &d.repeated, &d.ok, &d.late, &d.jumps};
        for (int k = 0; k < PCR_KINDS; ++k) { *dk[k] += a.kind[k]; d.pcr_packets += a.kind[k]; }
        d.malformed += a.malformed; d.accuracy_measured += a.accuracy_measured; d.accuracy_errors += a.accuracy_errors;
        d.sum_ticks += (int64_t)a.sum_ticks; d.sum_packets += (int64_t)a.sum_packets;
        if ((int64_t)a.max_delta_ticks > d.max_delta_ticks) d.max_delta_ticks = a.max_delta_ticks;
        if ((int64_t)a.max_abs_accuracy > d.max_abs_accuracy) d.max_abs_accuracy = a.max_abs_accuracy;
        if (a.last_k >= 0) ss.packets_since_pcr[s] = ss.packets + a.last_k;
    }
    ss.packets += n;
    ss.unwatched_pcr_packets += head.unwatched;
    ss.first_unwatched_pid = head.first_unwatched_pid;
    if (head.records > b->max_rows) ss.rows_dropped += head.records - b->max_rows;
    b->records[i] = head.records;
    b->nrows[i] = head.records < b->max_rows ? head.records : b->max_rows;
}
static const dvbs2gpu_pcr_stream_stats PCR_NO_STREAM_STATS = {0, 0, 0, -1, 0, {-1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1}};
static bool pcr_create_args_ok(int nstreams, int max_packets, int max_rows, dvbs2gpu_pcr** out) {
    if (!out || nstreams <= 0 || max_packets <= 0 || max_rows <= 0) return false;
    if (max_packets > PCR_MAX_PACKETS) { g_err = "PCR bank: max_packets is at most 4096 per stream and call"; return false; }
    return true;
}
static std::unique_ptr<dvbs2gpu_pcr> pcr_new(dvbs2gpu_ctx* ctx, int nstreams, int max_packets, int max_rows) {
    std::unique_ptr<dvbs2gpu_pcr> b(new dvbs2gpu_pcr());
    b->ctx = ctx; b->nstreams = nstreams; b->max_packets = max_packets; b->max_rows = max_rows;
    b->watch.assign((size_t)nstreams * PCR_SLOTS, -1);
    b->rate.assign(nstreams, PcrRate{0, PCR_DEFAULT_LIMIT_Q6, 0});
    b->stats.assign((size_t)nstreams * PCR_SLOTS, dvbs2gpu_pcr_stats{});
    b->sstats.assign(nstreams, PCR_NO_STREAM_STATS);
    b->nrows.assign(nstreams, 0); b->records.assign(nstreams, 0);
    b->h_call.resize(nstreams);
    return b;
}
}  // namespace s2

extern "C" {

void dvbs2gpu_pcr_destroy(dvbs2gpu_pcr* b) { delete b; }

int dvbs2gpu_pcr_create(dvbs2gpu_ctx* ctx, int nstreams, int max_packets, int max_rows, dvbs2gpu_pcr** out) {
    if (!ctx || !pcr_create_args_ok(nstreams, max_packets, max_rows, out)) return DVBS2GPU_ERR_ARG;
    HIP_TRY(hipSetDevice(ctx->device));
    auto b = pcr_new(ctx, nstreams, max_packets, max_rows);
    const size_t n = (size_t)nstreams, ns = n * PCR_SLOTS;
    const char* what = "hipMalloc(pcr)";               // (zero-filled: the slots' states and the positions; the kernel writes rows and call records before they are read)
    RC_TRY(b->d_watch.alloc(ns, false, what));
    HIP_TRY(hipMemcpy(b->d_watch, b->watch.data(), ns * sizeof(int32_t), hipMemcpyHostToDevice));
    RC_TRY(b->d_rate.alloc(n, false, what));
    HIP_TRY(hipMemcpy(b->d_rate, b->rate.data(), n * sizeof(PcrRate), hipMemcpyHostToDevice));
    RC_TRY(b->d_state.alloc(ns, true, what));
    RC_TRY(b->d_pos.alloc(n, true, what));
    RC_TRY(b->d_rows.alloc(n * max_rows, false, what));
    RC_TRY(b->d_call.alloc(n, false, what));
    RC_TRY(b->d_args.alloc(TsBankArgs(n).L.bytes(), false, what));
    b->h_args.resize(TsBankArgs(n).L.bytes());
    *out = b.release();
    return 0;
}

int dvbs2gpu_pcr_create_host(int nstreams, int max_packets, int max_rows, dvbs2gpu_pcr** out) {
    if (!pcr_create_args_ok(nstreams, max_packets, max_rows, out)) return DVBS2GPU_ERR_ARG;
    auto b = pcr_new(nullptr, nstreams, max_packets, max_rows);
    b->host.resize(nstreams);
    *out = b.release();
    return 0;
}

int dvbs2gpu_pcr_reset(dvbs2gpu_pcr* b) {
    if (!b) return DVBS2GPU_ERR_ARG;
    if (b->ctx) {
        HIP_TRY(hipSetDevice(b->ctx->device));
        HIP_TRY(hipMemset(b->d_state, 0, (size_t)b->nstreams * PCR_SLOTS * sizeof(PcrState)));
        HIP_TRY(hipMemset(b->d_pos, 0, (size_t)b->nstreams * sizeof(int64_t)));
    }
    for (auto& h : b->host) h.reset();
    std::fill(b->stats.begin(), b->stats.end(), dvbs2gpu_pcr_stats{});
    std::fill(b->sstats.begin(), b->sstats.end(), PCR_NO_STREAM_STATS);
    std::fill(b->nrows.begin(), b->nrows.end(), 0);
    std::fill(b->records.begin(), b->records.end(), 0);
    return 0;
}

int dvbs2gpu_pcr_set_watch(dvbs2gpu_pcr* b, int stream, int slot, int pid) {
    if (!b || stream < 0 || stream >= b->nstreams || slot < 0 || slot >= PCR_SLOTS) return DVBS2GPU_ERR_ARG;
    if (pid < -1 || pid >= TSMON_NULL_PID) { g_err = "PCR bank: a watched PID is 0..0x1FFE (-1 clears the slot)"; return DVBS2GPU_ERR_ARG; }
    int32_t* w = b->watch.data() + (size_t)stream * PCR_SLOTS;
    for (int s = 0; s < PCR_SLOTS; ++s)
        if (pid >= 0 && s != slot && w[s] == pid) { g_err = "PCR bank: the PID is watched in another slot of the stream"; return DVBS2GPU_ERR_ARG; }
    const size_t at = (size_t)stream * PCR_SLOTS + slot;
    w[slot] = pid;
    b->stats[at] = dvbs2gpu_pcr_stats{};
    b->sstats[stream].packets_since_pcr[slot] = -1;
    if (b->ctx) {
        HIP_TRY(hipSetDevice(b->ctx->device));
        HIP_TRY(hipMemcpy(b->d_watch + at, &w[slot], sizeof(int32_t), hipMemcpyHostToDevice));
        HIP_TRY(hipMemset(b->d_state + at, 0, sizeof(PcrState)));
    } else {
        b->host[stream].watch[slot] = pid;
        b->host[stream].clear_slot(slot);
    }
    return 0;
}

int dvbs2gpu_pcr_set_rate(dvbs2gpu_pcr* b, int stream, uint64_t ticks_per_packet_q24, int limit_q6) {
    if (!b || stream < 0 || stream >= b->nstreams) return DVBS2GPU_ERR_ARG;
    if (ticks_per_packet_q24 >= PCR_MAX_TPP || limit_q6 < 0) {
        g_err = "PCR bank: ticks per packet (Q24.24) stay below 2^48, the accuracy limit is not negative";
        return DVBS2GPU_ERR_ARG;
    }
    b->rate[stream] = PcrRate{ticks_per_packet_q24, limit_q6, 0};
    if (b->ctx) {
        HIP_TRY(hipSetDevice(b->ctx->device));
        HIP_TRY(hipMemcpy(b->d_rate + stream, &b->rate[stream], sizeof(PcrRate), hipMemcpyHostToDevice));
    } else b->host[stream].rate = b->rate[stream];
    return 0;
}

int dvbs2gpu_pcr_process_batch(dvbs2gpu_pcr* b, const uint8_t* const* d_ts, const int* nbytes, int* out_rows, void* stream) {
    if (!b || !d_ts || !nbytes) return DVBS2GPU_ERR_ARG;
    if (!b->ctx) { g_err = "PCR bank: a host bank takes host buffers (dvbs2gpu_pcr_work)"; return DVBS2GPU_ERR_ARG; }
    const int n = b->nstreams;
    for (int i = 0; i < n; ++i) {
        if (!ts_bank_check_counts("PCR bank: ", nbytes + i, 1, b->max_packets)) return DVBS2GPU_ERR_ARG;
        if (nbytes[i] > 0 && !d_ts[i]) { g_err = "PCR bank: null buffer"; return DVBS2GPU_ERR_ARG; }
    }
    HIP_TRY(hipSetDevice(b->ctx->device));
    hipStream_t st = (hipStream_t)stream;
    const TsBankArgs a(n);
    a.fill(b->h_args.data(), n, d_ts, nullptr, nbytes);
    HIP_TRY(hipMemcpyAsync(b->d_args, b->h_args.data(), b->h_args.size(), hipMemcpyHostToDevice, st));
    const size_t lds = sizeof(PcrShared) + (size_t)b->max_packets * 10;      // <= 51 KiB
    hipLaunchKernelGGL(pcr_kernel, dim3(n), dim3(PCR_WG), lds, st, a.in(b->d_args), a.nbytes(b->d_args), b->max_packets, b->max_rows, b->d_watch, b->d_rate, b->d_state,
                       b->d_pos, b->d_rows, b->d_call);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(b->h_call.data(), b->d_call, sizeof(PcrCall) * n, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    for (int i = 0; i < n; ++i) {
        pcr_account(b, i, nbytes[i] / TSMON_TS, b->h_call[i].head, b->h_call[i].cnt);
        if (out_rows) out_rows[i] = b->records[i];
    }
    return 0;
}

int dvbs2gpu_pcr_work(dvbs2gpu_pcr* b, int stream, const uint8_t* h_ts, int nbytes) {
    if (!b || stream < 0 || stream >= b->nstreams || nbytes < 0 || (nbytes > 0 && !h_ts)) return DVBS2GPU_ERR_ARG;
    if (!ts_bank_check_counts("PCR bank: ", &nbytes, 1, b->max_packets)) return DVBS2GPU_ERR_ARG;
    if (!b->ctx) {
        for (int i = 0; i < b->nstreams; ++i) {        // the other streams receive an empty call
            PcrHostStream& h = b->host[i];
            const int np = i == stream ? nbytes / TSMON_TS : 0;
            h.run(h_ts, np, b->max_rows);
            pcr_account(b, i, np, h.head, h.cnt);
        }
        return b->records[stream];
    }
    HIP_TRY(hipSetDevice(b->ctx->device));
    const int rc = ts_bank_work(b->stage, b->nstreams, stream, h_ts, nbytes, b->max_packets, nullptr, 0, false, [&](const uint8_t* const* in, const int* nb, uint8_t* const*, int*) {
        return dvbs2gpu_pcr_process_batch(b, in, nb, nullptr, nullptr);
    });
    return rc < 0 ? rc : b->records[stream];
}

int dvbs2gpu_pcr_get_stats(dvbs2gpu_pcr* b, int stream, int slot, dvbs2gpu_pcr_stats* h_out) {
    if (!b || stream < 0 || stream >= b->nstreams || slot < -1 || slot >= PCR_SLOTS || !h_out) return DVBS2GPU_ERR_ARG;
    *h_out = dvbs2gpu_pcr_stats{};
    for (int s = slot < 0 ? 0 : slot; s < (slot < 0 ? PCR_SLOTS : slot + 1); ++s) {
        const dvbs2gpu_pcr_stats& a = b->stats[(size_t)stream * PCR_SLOTS + s];
        const int64_t* src = reinterpret_cast<const int64_t*>(&a);
        int64_t* d = reinterpret_cast<int64_t*>(h_out);
        for (int k = 0; k < 12; ++k) d[k] += src[k];   // the two maxima are the last two words
        if (a.max_delta_ticks > h_out->max_delta_ticks) h_out->max_delta_ticks = a.max_delta_ticks;
        if (a.max_abs_accuracy > h_out->max_abs_accuracy) h_out->max_abs_accuracy = a.max_abs_accuracy;
    }
    return 0;
}

int dvbs2gpu_pcr_get_stream_stats(dvbs2gpu_pcr* b, int stream, dvbs2gpu_pcr_stream_stats* h_out) {
    if (!b || stream < 0 || stream >= b->nstreams || !h_out) return DVBS2GPU_ERR_ARG;
    *h_out = b->sstats[stream];
    for (int s = 0; s < PCR_SLOTS; ++s)
        if (h_out->packets_since_pcr[s] >= 0) h_out->packets_since_pcr[s] = h_out->packets - h_out->packets_since_pcr[s];
    return 0;
}

int dvbs2gpu_pcr_get_rate(dvbs2gpu_pcr* b, int stream, int slot, double* bits_per_s) {
    dvbs2gpu_pcr_stats st;
    if (!bits_per_s) return DVBS2GPU_ERR_ARG;
    if (const int e = dvbs2gpu_pcr_get_stats(b, stream, slot, &st)) return e;
    *bits_per_s = st.sum_ticks > 0 ? 1504.0 * 27e6 * (double)st.sum_packets / (double)st.sum_ticks : 0.0;
    return 0;
}

int dvbs2gpu_pcr_get_row_table(dvbs2gpu_pcr* b, int stream, dvbs2gpu_pcr_row* h_rows, int cap, int* n) {
    return ts_bank_rows(b, &dvbs2gpu_pcr::max_rows, stream, h_rows, cap, n);
}

int dvbs2gpu_pcr_get_row_table_device(dvbs2gpu_pcr* b, int stream, const dvbs2gpu_pcr_row** d_rows, int* n) {
    return ts_bank_rows_device(b, &dvbs2gpu_pcr::max_rows, stream, d_rows, n);
}

}  // extern "C"
