// PES bank (own extension; include/dvbs2gpu.h): PES packet starts, PTS / DTS and PES length checks on up to 16 watched
// PIDs of each of `nstreams` transport streams in HBM.  Every rule is in pes_rules.h, whose PesHostStream is the sequential
// definition, the host bank and the kernel's yardstick; this file says how a call's packets are taken in parallel.
//
// What makes the parallel form possible: behind any packet the continuity byte is the packet's own counter plus one bit, dup_used, and
// that bit is the parity of the packet's place in a run of equal counters; a PES packet's bytes, packets and GAP are sums over the
// packets between two starts; and a start's timestamp step needs only the slot's previous start that had a PTS.
//
//   pes_kernel  one workgroup per stream, one launch per call.
//     A-C  ts_watch.h, shared with the ES bank: the trusted packets of watched PIDs compacted into LDS as one 32-bit word each
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

// the packet counters of phase C, per thread and slot run
__device__ inline void pes_flush_pk(PesCnt* d, const PwPk& a) {
    atomicAdd(&d->packets, a.packets);
    if (a.payload_bytes) atomicAdd(&d->payload_bytes, a.payload_bytes);
    if (a.duplicates) atomicAdd(&d->duplicates, a.duplicates);
    if (a.cc_errors) atomicAdd(&d->cc_errors, a.cc_errors);
    if (a.scrambled) atomicAdd(&d->scrambled_packets, a.scrambled);
    if (a.malformed) atomicAdd(&d->malformed_packets, a.malformed);
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
                    [&](int slot, const PwPk& pk) { pes_flush_pk(&sh.cnt[slot], pk); }, &dupm, &gapm);
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

struct dvbs2gpu_pes {
    dvbs2gpu_ctx* ctx = nullptr;                   // null: a host-only bank (dvbs2gpu_pes_create_host)
    int nstreams = 0, max_packets = 0, max_rows = 0;
    std::vector<int32_t> watch;                    // nstreams x 16
    std::vector<PesRate> rate;
    std::vector<dvbs2gpu_pes_stats> stats;         // nstreams x 16, since reset; the kernel reports each call's share (PesCall)
    std::vector<dvbs2gpu_pes_stream_stats> sstats; // packets_since_start holds the position of the slot's last start, -1: none
    std::vector<int> nrows, starts;                // of the last call per stream: rows in the table, starts in all
    std::vector<PesCall> h_call;
    std::vector<char> h_args;
    // device banks
    DevBuf<int32_t> d_watch;
    DevBuf<PesRate> d_rate;
    DevBuf<PesState> d_state;
    DevBuf<int64_t> d_pos;
    DevBuf<PesRow> d_rows;                         // nstreams x max_rows
    DevBuf<PesCall> d_call;
    DevBuf<uint8_t> d_args;                        // TsBankArgs(nstreams)
    TsHostStage stage;                             // of the host-buffer entry point
    // host-only banks
    std::vector<PesHostStream> host;
};

namespace s2 {
constexpr int PES_STATS_SUMS = 23;                 // of dvbs2gpu_pes_stats: the counters in front of the maximum
static_assert(sizeof(dvbs2gpu_pes_stats) == (PES_STATS_SUMS + 1) * sizeof(int64_t), "stats order");
// one stream's call into its statistics; `n` packets came
static void pes_account(dvbs2gpu_pes* b, int i, int n, const PesCallHead& head, const PesCnt* c) {
    dvbs2gpu_pes_stream_stats& ss = b->sstats[i];
    for (int s = 0; s < PES_SLOTS; ++s) {
        const PesCnt& a = c[s];
        if (!a.packets) continue;                      // (no packet of the slot's PID came: every counter is 0)
        dvbs2gpu_pes_stats& d = b->stats[(size_t)i * PES_SLOTS + s];
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
    if (head.starts > b->max_rows) ss.rows_dropped += head.starts - b->max_rows;
    b->starts[i] = head.starts;
    b->nrows[i] = head.starts < b->max_rows ? head.starts : b->max_rows;
}
static const dvbs2gpu_pes_stream_stats PES_NO_STREAM_STATS = {0, 0, {-1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1}};
static bool pes_create_args_ok(int nstreams, int max_packets, int max_rows, dvbs2gpu_pes** out) {
    if (!out || nstreams <= 0 || max_packets <= 0 || max_rows <= 0) return false;
    if (max_packets > PES_MAX_PACKETS) { g_err = "PES bank: max_packets is at most 4096 per stream and call"; return false; }
    return true;
}
static std::unique_ptr<dvbs2gpu_pes> pes_new(dvbs2gpu_ctx* ctx, int nstreams, int max_packets, int max_rows) {
    std::unique_ptr<dvbs2gpu_pes> b(new dvbs2gpu_pes());
    b->ctx = ctx; b->nstreams = nstreams; b->max_packets = max_packets; b->max_rows = max_rows;
    b->watch.assign((size_t)nstreams * PES_SLOTS, -1);
    b->rate.assign(nstreams, PesRate{0, 0});
    b->stats.assign((size_t)nstreams * PES_SLOTS, dvbs2gpu_pes_stats{});
    b->sstats.assign(nstreams, PES_NO_STREAM_STATS);
    b->nrows.assign(nstreams, 0); b->starts.assign(nstreams, 0);
    b->h_call.resize(nstreams);
    return b;
}
}  // namespace s2

extern "C" {

void dvbs2gpu_pes_destroy(dvbs2gpu_pes* b) { delete b; }

int dvbs2gpu_pes_create(dvbs2gpu_ctx* ctx, int nstreams, int max_packets, int max_rows, dvbs2gpu_pes** out) {
    if (!ctx || !pes_create_args_ok(nstreams, max_packets, max_rows, out)) return DVBS2GPU_ERR_ARG;
    HIP_TRY(hipSetDevice(ctx->device));
    auto b = pes_new(ctx, nstreams, max_packets, max_rows);
    const size_t n = (size_t)nstreams, ns = n * PES_SLOTS;
    const char* what = "hipMalloc(pes)";               // (zero-filled: the slots' states, the positions and the rates; the kernel writes rows and call records before they are read)
    RC_TRY(b->d_watch.alloc(ns, false, what));
    HIP_TRY(hipMemcpy(b->d_watch, b->watch.data(), ns * sizeof(int32_t), hipMemcpyHostToDevice));
    RC_TRY(b->d_rate.alloc(n, true, what));
    RC_TRY(b->d_state.alloc(ns, true, what));
    RC_TRY(b->d_pos.alloc(n, true, what));
    RC_TRY(b->d_rows.alloc(n * max_rows, false, what));
    RC_TRY(b->d_call.alloc(n, false, what));
    RC_TRY(b->d_args.alloc(TsBankArgs(n).L.bytes(), false, what));
    b->h_args.resize(TsBankArgs(n).L.bytes());
    *out = b.release();
    return 0;
}

int dvbs2gpu_pes_create_host(int nstreams, int max_packets, int max_rows, dvbs2gpu_pes** out) {
    if (!pes_create_args_ok(nstreams, max_packets, max_rows, out)) return DVBS2GPU_ERR_ARG;
    auto b = pes_new(nullptr, nstreams, max_packets, max_rows);
    b->host.resize(nstreams);
    *out = b.release();
    return 0;
}

int dvbs2gpu_pes_reset(dvbs2gpu_pes* b) {
    if (!b) return DVBS2GPU_ERR_ARG;
    if (b->ctx) {
        HIP_TRY(hipSetDevice(b->ctx->device));
        HIP_TRY(hipMemset(b->d_state, 0, (size_t)b->nstreams * PES_SLOTS * sizeof(PesState)));
        HIP_TRY(hipMemset(b->d_pos, 0, (size_t)b->nstreams * sizeof(int64_t)));
    }
    for (auto& h : b->host) h.reset();
    std::fill(b->stats.begin(), b->stats.end(), dvbs2gpu_pes_stats{});
    std::fill(b->sstats.begin(), b->sstats.end(), PES_NO_STREAM_STATS);
    std::fill(b->nrows.begin(), b->nrows.end(), 0);
    std::fill(b->starts.begin(), b->starts.end(), 0);
    return 0;
}

int dvbs2gpu_pes_set_watch(dvbs2gpu_pes* b, int stream, int slot, int pid) {
    if (!b || stream < 0 || stream >= b->nstreams || slot < 0 || slot >= PES_SLOTS) return DVBS2GPU_ERR_ARG;
    if (pid < -1 || pid >= TSMON_NULL_PID) { g_err = "PES bank: a watched PID is 0..0x1FFE (-1 clears the slot)"; return DVBS2GPU_ERR_ARG; }
    int32_t* w = b->watch.data() + (size_t)stream * PES_SLOTS;
    for (int s = 0; s < PES_SLOTS; ++s)
        if (pid >= 0 && s != slot && w[s] == pid) { g_err = "PES bank: the PID is watched in another slot of the stream"; return DVBS2GPU_ERR_ARG; }
    const size_t at = (size_t)stream * PES_SLOTS + slot;
    w[slot] = pid;
    b->stats[at] = dvbs2gpu_pes_stats{};
    b->sstats[stream].packets_since_start[slot] = -1;
    if (b->ctx) {
        HIP_TRY(hipSetDevice(b->ctx->device));
        HIP_TRY(hipMemcpy(b->d_watch + at, &w[slot], sizeof(int32_t), hipMemcpyHostToDevice));
        HIP_TRY(hipMemset(b->d_state + at, 0, sizeof(PesState)));
    } else {
        b->host[stream].watch[slot] = pid;
        b->host[stream].clear_slot(slot);
    }
    return 0;
}

int dvbs2gpu_pes_set_rate(dvbs2gpu_pes* b, int stream, uint64_t ticks_per_packet_q24) {
    if (!b || stream < 0 || stream >= b->nstreams) return DVBS2GPU_ERR_ARG;
    if (ticks_per_packet_q24 >= PES_MAX_TPP) { g_err = "PES bank: ticks per packet (Q24.24) stay below 2^48"; return DVBS2GPU_ERR_ARG; }
    b->rate[stream] = pes_rate(ticks_per_packet_q24);
    if (b->ctx) {
        HIP_TRY(hipSetDevice(b->ctx->device));
        HIP_TRY(hipMemcpy(b->d_rate + stream, &b->rate[stream], sizeof(PesRate), hipMemcpyHostToDevice));
    } else b->host[stream].rate = b->rate[stream];
    return 0;
}

int dvbs2gpu_pes_process_batch(dvbs2gpu_pes* b, const uint8_t* const* d_ts, const int* nbytes, int* out_rows, void* stream) {
    if (!b || !d_ts || !nbytes) return DVBS2GPU_ERR_ARG;
    if (!b->ctx) { g_err = "PES bank: a host bank takes host buffers (dvbs2gpu_pes_work)"; return DVBS2GPU_ERR_ARG; }
    const int n = b->nstreams;
    for (int i = 0; i < n; ++i) {
        if (!ts_bank_check_counts("PES bank: ", nbytes + i, 1, b->max_packets)) return DVBS2GPU_ERR_ARG;
        if (nbytes[i] > 0 && !d_ts[i]) { g_err = "PES bank: null buffer"; return DVBS2GPU_ERR_ARG; }
    }
    HIP_TRY(hipSetDevice(b->ctx->device));
    hipStream_t st = (hipStream_t)stream;
    const TsBankArgs a(n);
    a.fill(b->h_args.data(), n, d_ts, nullptr, nbytes);
    HIP_TRY(hipMemcpyAsync(b->d_args, b->h_args.data(), b->h_args.size(), hipMemcpyHostToDevice, st));
    const size_t lds = pes_lds_bytes(b->max_packets);      // <= 59.2 KiB
    hipLaunchKernelGGL(pes_kernel, dim3(n), dim3(PES_WG), lds, st, a.in(b->d_args), a.nbytes(b->d_args), b->max_packets, b->max_rows, b->d_watch, b->d_rate, b->d_state,
                       b->d_pos, b->d_rows, b->d_call);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(b->h_call.data(), b->d_call, sizeof(PesCall) * n, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    for (int i = 0; i < n; ++i) {
        pes_account(b, i, nbytes[i] / TSMON_TS, b->h_call[i].head, b->h_call[i].cnt);
        if (out_rows) out_rows[i] = b->starts[i];
    }
    return 0;
}

int dvbs2gpu_pes_work(dvbs2gpu_pes* b, int stream, const uint8_t* h_ts, int nbytes) {
    if (!b || stream < 0 || stream >= b->nstreams || nbytes < 0 || (nbytes > 0 && !h_ts)) return DVBS2GPU_ERR_ARG;
    if (!ts_bank_check_counts("PES bank: ", &nbytes, 1, b->max_packets)) return DVBS2GPU_ERR_ARG;
    if (!b->ctx) {
        for (int i = 0; i < b->nstreams; ++i) {        // the other streams receive an empty call
            PesHostStream& h = b->host[i];
            const int np = i == stream ? nbytes / TSMON_TS : 0;
            h.run(h_ts, np, b->max_rows);
            pes_account(b, i, np, h.head, h.cnt);
        }
        return b->starts[stream];
    }
    HIP_TRY(hipSetDevice(b->ctx->device));
    const int rc = ts_bank_work(b->stage, b->nstreams, stream, h_ts, nbytes, b->max_packets, nullptr, 0, false, [&](const uint8_t* const* in, const int* nb, uint8_t* const*, int*) {
        return dvbs2gpu_pes_process_batch(b, in, nb, nullptr, nullptr);
    });
    return rc < 0 ? rc : b->starts[stream];
}

int dvbs2gpu_pes_get_stats(dvbs2gpu_pes* b, int stream, int slot, dvbs2gpu_pes_stats* h_out) {
    if (!b || stream < 0 || stream >= b->nstreams || slot < -1 || slot >= PES_SLOTS || !h_out) return DVBS2GPU_ERR_ARG;
    *h_out = dvbs2gpu_pes_stats{};
    for (int s = slot < 0 ? 0 : slot; s < (slot < 0 ? PES_SLOTS : slot + 1); ++s) {
        const dvbs2gpu_pes_stats& a = b->stats[(size_t)stream * PES_SLOTS + s];
        const int64_t* src = reinterpret_cast<const int64_t*>(&a);
        int64_t* d = reinterpret_cast<int64_t*>(h_out);
        for (int k = 0; k < PES_STATS_SUMS; ++k) d[k] += src[k];   // the maximum is the last word
        if (a.max_delta_packets > h_out->max_delta_packets) h_out->max_delta_packets = a.max_delta_packets;
    }
    return 0;
}

int dvbs2gpu_pes_get_stream_stats(dvbs2gpu_pes* b, int stream, dvbs2gpu_pes_stream_stats* h_out) {
    if (!b || stream < 0 || stream >= b->nstreams || !h_out) return DVBS2GPU_ERR_ARG;
    *h_out = b->sstats[stream];
    for (int s = 0; s < PES_SLOTS; ++s)
        if (h_out->packets_since_start[s] >= 0) h_out->packets_since_start[s] = h_out->packets - h_out->packets_since_start[s];
    return 0;
}

int dvbs2gpu_pes_get_row_table(dvbs2gpu_pes* b, int stream, dvbs2gpu_pes_row* h_rows, int cap, int* n) {
    return ts_bank_rows(b, &dvbs2gpu_pes::max_rows, stream, h_rows, cap, n);
}

int dvbs2gpu_pes_get_row_table_device(dvbs2gpu_pes* b, int stream, const dvbs2gpu_pes_row** d_rows, int* n) {
    return ts_bank_rows_device(b, &dvbs2gpu_pes::max_rows, stream, d_rows, n);
}

}  // extern "C"
