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
#include "watch_bank.h"

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

// the host half is the watched-PID bank's (watch_bank.h); here what is the bank's own
struct PcrBankD {
    static constexpr int SLOTS = PCR_SLOTS, MAX_PACKETS = PCR_MAX_PACKETS;
    typedef PcrState State; typedef PcrRow Row; typedef PcrCall Call; typedef PcrHostStream HostStream;
    typedef dvbs2gpu_pcr_stats Stats; typedef dvbs2gpu_pcr_stream_stats StreamStats;
    static constexpr int SUMS = 12;                    // of dvbs2gpu_pcr_stats: the two maxima are the last two words
    // packets_since_pcr holds the position of the slot's last record, -1: none
    static constexpr StreamStats NO_STREAM_STATS = {0, 0, 0, -1, 0, {-1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1}};
    typedef PcrRate Config;                            // per stream
    static constexpr int CONFIGS = 1;
    static constexpr Config NO_CONFIG = {0, PCR_DEFAULT_LIMIT_Q6, 0};
    static constexpr const char *BANK = "PCR bank: ", *CNAME = "dvbs2gpu_pcr", *ALLOC = "hipMalloc(pcr)";

    // one stream's call into its statistics; `n` packets came
    static void account(WatchBank<PcrBankD>& b, int i, int n, const PcrCallHead& head, const PcrCnt* c) {
        dvbs2gpu_pcr_stream_stats& ss = b.sstats[i];
        for (int s = 0; s < PCR_SLOTS; ++s) {
            dvbs2gpu_pcr_stats& d = b.stats[(size_t)i * PCR_SLOTS + s];
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
        if (head.records > b.max_rows) ss.rows_dropped += head.records - b.max_rows;
        b.total[i] = head.records;
        b.nrows[i] = head.records < b.max_rows ? head.records : b.max_rows;
    }
    static void launch(WatchBank<PcrBankD>& b, const TsBankArgs& a, hipStream_t st) {
        const size_t lds = sizeof(PcrShared) + (size_t)b.max_packets * 10;      // <= 51 KiB
        hipLaunchKernelGGL(pcr_kernel, dim3(b.nstreams), dim3(PCR_WG), lds, st, a.in(b.d_args), a.nbytes(b.d_args), b.max_packets, b.max_rows, b.d_watch, b.d_cfg, b.d_state,
                           b.d_pos, b.d_rows, b.d_call);
    }
    static void fix_stream_stats(StreamStats* o) {
        for (int s = 0; s < PCR_SLOTS; ++s)
            if (o->packets_since_pcr[s] >= 0) o->packets_since_pcr[s] = o->packets - o->packets_since_pcr[s];
    }
};
static_assert(sizeof(dvbs2gpu_pcr_stats) == (PcrBankD::SUMS + 2) * sizeof(int64_t), "stats order");
struct dvbs2gpu_pcr : WatchBank<PcrBankD> {};

extern "C" {

void dvbs2gpu_pcr_destroy(dvbs2gpu_pcr* b) { delete b; }
int dvbs2gpu_pcr_create(dvbs2gpu_ctx* ctx, int nstreams, int max_packets, int max_rows, dvbs2gpu_pcr** out) { return watch_create(true, ctx, nstreams, max_packets, max_rows, out); }
int dvbs2gpu_pcr_create_host(int nstreams, int max_packets, int max_rows, dvbs2gpu_pcr** out) { return watch_create(false, nullptr, nstreams, max_packets, max_rows, out); }
int dvbs2gpu_pcr_reset(dvbs2gpu_pcr* b) { return watch_reset(b); }

int dvbs2gpu_pcr_set_watch(dvbs2gpu_pcr* b, int stream, int slot, int pid) {
    if (!watch_slot_ok(b, stream, slot, pid)) return DVBS2GPU_ERR_ARG;
    if (const int e = watch_set_watch(b, stream, slot, pid)) return e;
    b->sstats[stream].packets_since_pcr[slot] = -1;
    return 0;
}

int dvbs2gpu_pcr_set_rate(dvbs2gpu_pcr* b, int stream, uint64_t ticks_per_packet_q24, int limit_q6) {
    if (!b || stream < 0 || stream >= b->nstreams) return DVBS2GPU_ERR_ARG;
    if (ticks_per_packet_q24 >= PCR_MAX_TPP || limit_q6 < 0) {
        g_err = "PCR bank: ticks per packet (Q24.24) stay below 2^48, the accuracy limit is not negative";
        return DVBS2GPU_ERR_ARG;
    }
    b->cfg[stream] = PcrRate{ticks_per_packet_q24, limit_q6, 0};
    if (b->ctx) return watch_upload_config(b, stream);
    b->host[stream].rate = b->cfg[stream];
    return 0;
}

int dvbs2gpu_pcr_process_batch(dvbs2gpu_pcr* b, const uint8_t* const* d_ts, const int* nbytes, int* out_rows, void* stream) {
    return watch_process_batch(b, d_ts, nbytes, out_rows, stream);
}
int dvbs2gpu_pcr_work(dvbs2gpu_pcr* b, int stream, const uint8_t* h_ts, int nbytes) { return watch_work(b, stream, h_ts, nbytes); }
int dvbs2gpu_pcr_get_stats(dvbs2gpu_pcr* b, int stream, int slot, dvbs2gpu_pcr_stats* h_out) { return watch_get_stats(b, stream, slot, h_out); }
int dvbs2gpu_pcr_get_stream_stats(dvbs2gpu_pcr* b, int stream, dvbs2gpu_pcr_stream_stats* h_out) { return watch_get_stream_stats(b, stream, h_out); }

int dvbs2gpu_pcr_get_rate(dvbs2gpu_pcr* b, int stream, int slot, double* bits_per_s) {
    dvbs2gpu_pcr_stats st;
    if (!bits_per_s) return DVBS2GPU_ERR_ARG;
    if (const int e = dvbs2gpu_pcr_get_stats(b, stream, slot, &st)) return e;
    *bits_per_s = st.sum_ticks > 0 ? 1504.0 * 27e6 * (double)st.sum_packets / (double)st.sum_ticks : 0.0;
    return 0;
}

int dvbs2gpu_pcr_get_row_table(dvbs2gpu_pcr* b, int stream, dvbs2gpu_pcr_row* h_rows, int cap, int* n) { return watch_get_row_table(b, stream, h_rows, cap, n); }
int dvbs2gpu_pcr_get_row_table_device(dvbs2gpu_pcr* b, int stream, const dvbs2gpu_pcr_row** d_rows, int* n) { return watch_get_row_table_device(b, stream, d_rows, n); }

}  // extern "C"
