// PES bank (own extension; include/dvbs2gpu.h): PES packet starts, PTS / DTS and PES length checks on up to 16 watched
// PIDs of each of `nstreams` transport streams in HBM.  Every rule is in pes_rules.h, whose PesHostStream is the sequential
// definition, the host bank and the kernel's yardstick; this file says how a call's packets are taken in parallel.
//
// What makes the parallel form possible: behind any packet the continuity byte is the packet's own counter plus one bit, dup_used, and
// that bit is the parity of the packet's place in a run of equal counters; a PES packet's bytes, packets and GAP are sums over the
// packets between two starts; and a start's timestamp step needs only the slot's previous start that had a PTS.
//
//   pes_kernel  one workgroup per stream, one launch per call.
//     A-C  ts_watch.h, shared with the ES and audio banks: the trusted packets of watched PIDs compacted into LDS as one 32-bit word each
//        (packet, slot, counter, payload length, payload, PUSI, scrambled, DI), sorted by slot, and tsmon_step's verdict per packet
//        from the parity of its place in a run of equal counters.
//     D  two prefix sums over the accepted packets in sorted order -- payload bytes; packets and GAP marks -- make every PES
//        packet's byte count, packet count and GAP a difference of two prefix values.
//     E  the lanes that own starts read the first payload bytes (five unaligned dwords that stay inside the packet) and apply
//        pes_start; what a later start needs of them -- the declared length, "had a PTS" -- goes to LDS, the start's packet index
//        into a bitmap whose prefix population count is the row number.  Two more maximum scans give every start its slot's previous
//        start and previous start with a PTS.  Then pes_step per start in its own lane, against a state put together from the carried
//        one, the prefix values and the previous timestamp (read again from the packet that holds it), the row, and the counters
//        summed per thread and slot run, then into LDS.  The lane of the slot's last packet writes the slot's new state.
// No lane walks over packets of other lanes: the cost of a call does not depend on what the packets say.  One device-to-host copy of
// the per-stream call record (PesCall).
#include "ts_watch.h"
#include "watch_bank.h"

using namespace s2;
#define g_err last_error()

namespace s2 {

constexpr int PES_MAX_PACKETS = PW_MAX_PACKETS;           // per stream and call: 12 bytes of LDS per packet
constexpr int PES_WG = 256;
constexpr int PES_BM_WORDS = PES_MAX_PACKETS / 32;
static_assert(sizeof(PesRow) == sizeof(dvbs2gpu_pes_row) && sizeof(PesRow) == 48, "row layout");
static_assert(PES_MAX_PACKETS <= 16 * PES_WG, "a thread's verdicts are 16 bits of a mask, its slot counts 16-bit words (ts_thread_run)");
static_assert(PES_BM_WORDS <= PES_WG, "one thread per word of the start bitmap");
static_assert(PES_MAX_PACKETS * (TSMON_TS - 4) < (1 << 20) && PES_MAX_PACKETS < (1 << 13), "the prefix sums: bytes in an int, packets and GAP marks in 13 bits each");
static_assert(PES_HEADER == DVBS2GPU_PES_HEADER && PES_SCRAMBLED == DVBS2GPU_PES_SCRAMBLED && PES_MALFORMED == DVBS2GPU_PES_MALFORMED, "public values");
static_assert(PES_CLOSED == DVBS2GPU_PES_CLOSED && PES_UNBOUNDED_NONVIDEO == DVBS2GPU_PES_UNBOUNDED_NONVIDEO && PES_DTS_AFTER_PTS == DVBS2GPU_PES_DTS_AFTER_PTS, "public values");

struct PesCall { PesCallHead head; PesCnt cnt[PES_SLOTS]; };

// the packet words, their verdict bits and phases A-C: ts_watch.h.  Behind phase E's first pass bit 18 says that a start has a PTS
constexpr uint32_t PW_PTS = 1u << 18;

// what the kernel keeps in LDS beside the packets; a multiple of 16 bytes in front of them
struct alignas(16) PesShared {
    PesCnt cnt[PES_SLOTS];
    PesState ss[PES_SLOTS];                      // the slots' states before the call
    uint16_t place[PES_SLOTS][PES_WG];           // the counting sort's counts, then places; behind the sort the starts' declared lengths
    uint32_t bm[PES_BM_WORDS];                   // bit k: packet k is a start
    int32_t bmpre[PES_BM_WORDS];                 // the starts in the words before
    int32_t w[PES_SLOTS];
    int32_t start[PES_SLOTS + 1];                // the slots' runs in sorted order
    int32_t wsum[PES_WG / 64];
    uint8_t ncc[PES_SLOTS];                      // the slots' continuity bytes behind the call
    int64_t pos0;
    PesRate rate;
};
static_assert(sizeof(PesShared) % 16 == 0 && sizeof(PesShared::place) == PES_MAX_PACKETS * sizeof(uint16_t), "the packets behind it; a declared length per packet");
constexpr size_t pes_lds_bytes(int max_packets) { return sizeof(PesShared) + ((size_t)max_packets * 3 + 2) * sizeof(uint32_t); }
static_assert(pes_lds_bytes(PES_MAX_PACKETS) <= 64 * 1024, "dynamic LDS of a workgroup");

// the start in packet word e (pw_load_start: five dwords that stay inside the packet; pes_start looks at no byte behind its end)
__device__ inline PesHead pes_load_start(const uint8_t* __restrict__ ts, uint32_t e) {
    uint32_t w[5];
    pw_load_start(ts, e, w);
    return pes_start(w, pw_len(e), pw_scr(e));
}

__device__ inline void pes_flush(PesCnt* d, const PesCnt& a) {
#define PES_ADD(f) if (a.f) atomicAdd(&d->f, a.f)
    for (int i = 0; i < PES_KINDS; ++i) PES_ADD(kind[i]);
    PES_ADD(with_pts); PES_ADD(with_dts); PES_ADD(closed_ok); PES_ADD(closed_mismatch); PES_ADD(closed_gap); PES_ADD(closed_unchecked);
    PES_ADD(ts_backward); PES_ADD(ts_gap); PES_ADD(pts_late); PES_ADD(dts_after_pts);
#undef PES_ADD
    if (a.max_delta_packets) atomicMax(&d->max_delta_packets, a.max_delta_packets);
    if (a.last_k >= 0) d->last_k = a.last_k;      // one lane per slot has it
}

// dynamic LDS: PesShared, srt[max_packets], exb[max_packets + 1], exc[max_packets + 1] (32 bits each).  The compacted words lie in exb
// until they are sorted into srt
__global__ void __launch_bounds__(PES_WG) pes_kernel(const uint8_t* const* __restrict__ in, const int* __restrict__ nbytes, int max_packets, int max_rows,
                                                     const int32_t* __restrict__ watch, const PesRate* __restrict__ rate, PesState* __restrict__ state,
                                                     int64_t* __restrict__ pos, PesRow* __restrict__ rows_g, PesCall* __restrict__ call) {
    extern __shared__ __attribute__((aligned(16))) unsigned char pes_lds[];
    PesShared& sh = *reinterpret_cast<PesShared*>(pes_lds);
    uint32_t* srt = reinterpret_cast<uint32_t*>(pes_lds + sizeof(PesShared));
    uint32_t* exb = srt + max_packets;               // exclusive prefix: payload bytes of the accepted packets
    uint32_t* exc = exb + max_packets + 1;           // the same of (packets << 13 | GAP marks)
    uint32_t* rec = exb;
    uint16_t* decl = &sh.place[0][0];
    const int s = blockIdx.x, tid = threadIdx.x;
    int n = nbytes[s] / TSMON_TS;
    if (n > max_packets) n = max_packets;            // (the host has refused such a call)
    if (tid < PES_SLOTS) {
        sh.w[tid] = watch[(size_t)s * PES_SLOTS + tid];
        sh.ss[tid] = state[(size_t)s * PES_SLOTS + tid];
        sh.cnt[tid] = pes_cnt_zero();
    }
    if (tid < PES_BM_WORDS) sh.bm[tid] = 0;
    if (tid == 0) { sh.pos0 = pos[s]; sh.rate = rate[s]; }
    __syncthreads();
    const uint8_t* ts = in[s];
    // A: the watched packets, compacted in input order
    const int W = pw_compact<PES_WG>(ts, n, sh.w, sh.wsum, rec);
    int nstarts = 0;
    if (W > 0) {
        // B: the stable counting sort by slot
        int j0, j1;
        pw_sort<PES_WG>(rec, srt, W, sh.place, sh.start, sh.wsum, &j0, &j1);
        // C: the continuity verdicts
        unsigned dupm, gapm;
        pw_verdicts(srt, j0, j1, sh.start, [&](int slot) { return sh.ss[slot].cc; }, sh.wsum, sh.ncc,
                    [&](int slot, const PwPk& pk) { pw_flush_pk(&sh.cnt[slot], pk); }, &dupm, &gapm);
        __syncthreads();                                         // every counter has been read: the verdicts take their bits
        // D: the prefix sums over the accepted packets
        {
            int sb = 0, sc = 0;
            for (int j = j0; j < j1; ++j) {
                const uint32_t e = pw_with_verdict(srt[j], dupm >> (j - j0) & 1, gapm >> (j - j0) & 1);
                srt[j] = e;
                if (pw_counts(e)) { sb += pw_len(e); sc += 1 << 13; }
                sc += (e & PW_GAP) != 0;
            }
            int tb, tc;
            int ab = ts_block_scan<PES_WG>(sb, sh.wsum, &tb), ac = ts_block_scan<PES_WG>(sc, sh.wsum, &tc);
            for (int j = j0; j < j1; ++j) {
                const uint32_t e = srt[j];
                exb[j] = (uint32_t)ab; exc[j] = (uint32_t)ac;
                if (pw_counts(e)) { ab += pw_len(e); ac += 1 << 13; }
                ac += (e & PW_GAP) != 0;
            }
            if (tid == 0) { exb[W] = (uint32_t)tb; exc[W] = (uint32_t)tc; }
        }
        // E: the starts.  First what later starts need of each
        int last_start = -1, last_pts = -1;
        for (int j = j0; j < j1; ++j) {
            const uint32_t e = srt[j];
            if (!pw_start(e)) continue;
            const PesHead hd = pes_load_start(ts, e);
            decl[j] = (uint16_t)hd.declared;
            last_start = j;
            if (hd.kind == PES_HEADER && hd.pts != PES_NO_TS) { srt[j] = e | PW_PTS; last_pts = j; }
            atomicOr(&sh.bm[pw_k(e) >> 5], 1u << (pw_k(e) & 31));
        }
        __syncthreads();
        last_start = ts_block_scan_max(last_start, sh.wsum);     // the last sorted start before j,
        last_pts = ts_block_scan_max(last_pts, sh.wsum);         // and the last one with a PTS
        {
            const int at = ts_block_scan<PES_WG>(tid < PES_BM_WORDS ? __popc(sh.bm[tid]) : 0, sh.wsum, &nstarts);
            if (tid < PES_BM_WORDS) sh.bmpre[tid] = at;
        }
        __syncthreads();
        const int64_t pos0 = sh.pos0;
        const PesRate rt = sh.rate;
        // the slot's state where `bytes` payload bytes, `cg` (packets << 13 | GAP marks) have come since the call began, the last start
        // and the last start with a PTS before that place being ls and lp
        auto state_at = [&](int slot, uint32_t bytes, uint32_t cg, int ls, int lp) {
            const int head = sh.start[slot];
            PesState st = sh.ss[slot];
            uint32_t b0 = exb[head], c0 = exc[head];
            if (ls >= head) {
                const uint32_t ep = srt[ls];
                b0 = exb[ls]; c0 = exc[ls] + ((ep & PW_GAP) != 0);   // (a mark on the start itself went to the packet it closed)
                st.open = 1; st.gap = 0; st.declared = decl[ls]; st.bytes = 0; st.packets = 0;
            }
            st.bytes = pes_sat32((uint64_t)st.bytes + (bytes - b0));
            st.packets = pes_sat32((uint64_t)st.packets + ((cg >> 13) - (c0 >> 13)));
            if ((cg & 8191) != (c0 & 8191)) st.gap = 1;
            if (lp >= head) {
                const uint32_t ep = srt[lp];
                const PesHead hp = pes_load_start(ts, ep);
                st.seen = 1; st.last_t = hp.dts != PES_NO_TS ? hp.dts : hp.pts; st.ref_n = pos0 + pw_k(ep);
            }
            return st;
        };
        PesCnt acc = pes_cnt_zero();
        int acc_slot = -1;
        PesRow* rows = rows_g + (size_t)s * max_rows;
        for (int j = j0; j < j1; ++j) {
            const uint32_t e = srt[j];
            const int slot = pw_slot(e), k = pw_k(e);
            if (slot != acc_slot) {
                if (acc_slot >= 0) pes_flush(&sh.cnt[acc_slot], acc);
                acc = pes_cnt_zero(); acc_slot = slot;
            }
            if (pw_start(e)) {
                const PesState st = state_at(slot, exb[j], exc[j] + ((e & PW_GAP) != 0), last_start, last_pts);
                PesRow row = {(uint16_t)sh.w[slot], (uint8_t)slot, 0, 0, 0, 0, k, 0, 0, 0, 0, 0, 0, 0};
                pes_step(st, pes_load_start(ts, e), pw_len(e), pos0 + k, rt, &row);
                pes_cnt_add(&acc, row);
                const int rank = sh.bmpre[k >> 5] + __popc(sh.bm[k >> 5] & ((1u << (k & 31)) - 1));
                if (rank < max_rows) rows[rank] = row;
                last_start = j;
                if (e & PW_PTS) last_pts = j;
            }
            if (j == sh.start[slot + 1] - 1) {
                PesState nx = state_at(slot, exb[j + 1], exc[j + 1], last_start, last_pts);
                nx.cc = sh.ncc[slot];
                state[(size_t)s * PES_SLOTS + slot] = nx;
                if (last_start >= sh.start[slot]) acc.last_k = pw_k(srt[last_start]);
            }
        }
        if (acc_slot >= 0) pes_flush(&sh.cnt[acc_slot], acc);
        __syncthreads();
    }
    if (tid < PES_SLOTS) call[s].cnt[tid] = sh.cnt[tid];
    if (tid == 0) {
        call[s].head = PesCallHead{nstarts, {0, 0, 0}};
        pos[s] = sh.pos0 + n;
    }
}

}  // namespace s2

// the host half is the watched-PID bank's (watch_bank.h); here what is the bank's own
struct PesBankD {
    static constexpr int SLOTS = PES_SLOTS, MAX_PACKETS = PES_MAX_PACKETS;
    typedef PesState State; typedef PesRow Row; typedef PesCall Call; typedef PesHostStream HostStream;
    typedef dvbs2gpu_pes_stats Stats; typedef dvbs2gpu_pes_stream_stats StreamStats;
    static constexpr int SUMS = 23;                    // of dvbs2gpu_pes_stats: the counters in front of the maximum
    // packets_since_start holds the position of the slot's last start, -1: none
    static constexpr StreamStats NO_STREAM_STATS = {0, 0, {-1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1}};
    typedef PesRate Config;                            // per stream
    static constexpr int CONFIGS = 1;
    static constexpr Config NO_CONFIG = {0, 0};
    static constexpr const char *BANK = "PES bank: ", *CNAME = "dvbs2gpu_pes", *ALLOC = "hipMalloc(pes)";

    // one stream's call into its statistics; `n` packets came
    static void account(WatchBank<PesBankD>& b, int i, int n, const PesCallHead& head, const PesCnt* c) {
        dvbs2gpu_pes_stream_stats& ss = b.sstats[i];
        for (int s = 0; s < PES_SLOTS; ++s) {
            const PesCnt& a = c[s];
            if (!a.packets) continue;                      // (no packet of the slot's PID came: every counter is 0)
            dvbs2gpu_pes_stats& d = b.stats[(size_t)i * PES_SLOTS + s];
            d.packets += a.packets; d.payload_bytes += a.payload_bytes; d.duplicates += a.duplicates; d.cc_errors += a.cc_errors;
            d.scrambled_packets += a.scrambled_packets; d.malformed_packets += a.malformed_packets;
            int64_t* dk[PES_KINDS] = {&d.starts_scrambled, &d.starts_short, &d.starts_bad_start, &d.starts_plain, &d.starts_malformed, &d.starts_header};
            for (int k = 0; k < PES_KINDS; ++k) { *dk[k] += a.kind[k]; d.starts += a.kind[k]; }
            d.with_pts += a.with_pts; d.with_dts += a.with_dts;
            d.closed_ok += a.closed_ok; d.closed_mismatch += a.closed_mismatch; d.closed_gap += a.closed_gap; d.closed_unchecked += a.closed_unchecked;
            d.ts_backward += a.ts_backward; d.ts_gap += a.ts_gap; d.pts_late += a.pts_late; d.dts_after_pts += a.dts_after_pts;
            if ((int64_t)a.max_delta_packets > d.max_delta_packets) d.max_delta_packets = a.max_delta_packets;
            if (a.last_k >= 0) ss.packets_since_start[s] = ss.packets + a.last_k;
        }
        ss.packets += n;
        if (head.starts > b.max_rows) ss.rows_dropped += head.starts - b.max_rows;
        b.total[i] = head.starts;
        b.nrows[i] = head.starts < b.max_rows ? head.starts : b.max_rows;
    }
    static void launch(WatchBank<PesBankD>& b, const TsBankArgs& a, hipStream_t st) {
        const size_t lds = pes_lds_bytes(b.max_packets);       // <= 59.2 KiB
        hipLaunchKernelGGL(pes_kernel, dim3(b.nstreams), dim3(PES_WG), lds, st, a.in(b.d_args), a.nbytes(b.d_args), b.max_packets, b.max_rows, b.d_watch, b.d_cfg, b.d_state,
                           b.d_pos, b.d_rows, b.d_call);
    }
    static void fix_stream_stats(StreamStats* o) {
        for (int s = 0; s < PES_SLOTS; ++s)
            if (o->packets_since_start[s] >= 0) o->packets_since_start[s] = o->packets - o->packets_since_start[s];
    }
};
static_assert(sizeof(dvbs2gpu_pes_stats) == (PesBankD::SUMS + 1) * sizeof(int64_t), "stats order");
struct dvbs2gpu_pes : WatchBank<PesBankD> {};

extern "C" {

void dvbs2gpu_pes_destroy(dvbs2gpu_pes* b) { delete b; }
int dvbs2gpu_pes_create(dvbs2gpu_ctx* ctx, int nstreams, int max_packets, int max_rows, dvbs2gpu_pes** out) { return watch_create(true, ctx, nstreams, max_packets, max_rows, out); }
int dvbs2gpu_pes_create_host(int nstreams, int max_packets, int max_rows, dvbs2gpu_pes** out) { return watch_create(false, nullptr, nstreams, max_packets, max_rows, out); }
int dvbs2gpu_pes_reset(dvbs2gpu_pes* b) { return watch_reset(b); }

int dvbs2gpu_pes_set_watch(dvbs2gpu_pes* b, int stream, int slot, int pid) {
    if (!watch_slot_ok(b, stream, slot, pid)) return DVBS2GPU_ERR_ARG;
    if (const int e = watch_set_watch(b, stream, slot, pid)) return e;
    b->sstats[stream].packets_since_start[slot] = -1;
    return 0;
}

int dvbs2gpu_pes_set_rate(dvbs2gpu_pes* b, int stream, uint64_t ticks_per_packet_q24) {
    if (!b || stream < 0 || stream >= b->nstreams) return DVBS2GPU_ERR_ARG;
    if (ticks_per_packet_q24 >= PES_MAX_TPP) { g_err = "PES bank: ticks per packet (Q24.24) stay below 2^48"; return DVBS2GPU_ERR_ARG; }
    b->cfg[stream] = pes_rate(ticks_per_packet_q24);
    if (b->ctx) return watch_upload_config(b, stream);
    b->host[stream].rate = b->cfg[stream];
    return 0;
}

int dvbs2gpu_pes_process_batch(dvbs2gpu_pes* b, const uint8_t* const* d_ts, const int* nbytes, int* out_rows, void* stream) {
    return watch_process_batch(b, d_ts, nbytes, out_rows, stream);
}
int dvbs2gpu_pes_work(dvbs2gpu_pes* b, int stream, const uint8_t* h_ts, int nbytes) { return watch_work(b, stream, h_ts, nbytes); }
int dvbs2gpu_pes_get_stats(dvbs2gpu_pes* b, int stream, int slot, dvbs2gpu_pes_stats* h_out) { return watch_get_stats(b, stream, slot, h_out); }
int dvbs2gpu_pes_get_stream_stats(dvbs2gpu_pes* b, int stream, dvbs2gpu_pes_stream_stats* h_out) { return watch_get_stream_stats(b, stream, h_out); }
int dvbs2gpu_pes_get_row_table(dvbs2gpu_pes* b, int stream, dvbs2gpu_pes_row* h_rows, int cap, int* n) { return watch_get_row_table(b, stream, h_rows, cap, n); }
int dvbs2gpu_pes_get_row_table_device(dvbs2gpu_pes* b, int stream, const dvbs2gpu_pes_row** d_rows, int* n) { return watch_get_row_table_device(b, stream, d_rows, n); }

}  // extern "C"
