// Shared by the banks that read the elementary streams of up to 16 watched PIDs per stream (es.hip: the video start codes; aud.hip:
// the audio frames).  It sits on ts_watch.h as ts_watch.h sits on ts_bank.h, and holds what such a kernel does before
// and after it looks at the elementary-stream bytes themselves, and what the bank is on the host beside watch_bank.h:
//     front()  the kernel's set-up and phases A-E: the trusted packets of watched PIDs sorted by slot with their verdicts (A-C,
//        ts_watch.h); the starts' plans, valid or not into bit 18 of the word (D); every packet's segment of ES bytes from its slot's
//        last start, the ES positions by one prefix sum (exs), the reset marks (E).
//     rows()   the skeleton of the last phase: a prefix sum over the rows per packet in INPUT order gives every packet its place in the
//        table, a maximum scan the slot's last row-bearing packet before one (RESYNC: a reset mark behind it); the PES rows are written;
//        the lane of the slot's last packet writes the slot's new state.
//     finish() the call record and the stream's position.
// A bank supplies a traits type T:
//   State, Cnt, Row, Shared           the slot's carried state (es_count, tail, have, cc), the counters (they begin with EsStreamCnt),
//                                     the row, what the kernel keeps in LDS (EsStreamShared<Cnt, State> or a struct derived from it)
//   flush(Cnt*, const Cnt&)           a thread's counters of one slot run into LDS
//   synced(State), lost(State), set_synced_lost(State&, bool, bool)     where the two bits are kept
//   pes_row(pid, slot, k, plan, es_pos, lost)                           the row of a start
// and its own callables: for front() a per-packet hook with placed(j) (phase D: the sorted place j holds its word), first(j, e, len)
// and second(j, e, len) (the two loops of phase E) and between(wsum) (the block scans between them); for rows() "write the other rows
// of sorted packet j from `rank`, the first with RESYNC if `lost`" and "finish the slot's new state behind its last packet j".  What a
// bank does between front() and rows() -- how it finds and counts its rows, rc[k] per INPUT packet -- is its own.
// Behind them the descriptor half that the two banks share on the host (EsStreamBankD) and the body of set_watch.
// aud_kernel is written on all of it.  es_kernel uses the types, the predicates and the host half, but keeps its own text of front()
// and rows(): on EsStream it was measurably slower for no reason that was found (the note at the kernel, es.hip).
// Vector stores and plain C++ only.
#pragma once
#include "ts_watch.h"
#include "watch_bank.h"
#include "es_rules.h"

namespace s2 {

constexpr int ES_MAX_PACKETS = PW_MAX_PACKETS;             // per stream and call
constexpr int ES_WG = 256;
static_assert(ES_MAX_PACKETS <= 16 * ES_WG, "a thread's verdicts are 16 bits of a mask, its slot counts 16-bit words (ts_thread_run)");
static_assert(ES_MAX_PACKETS * (TSMON_TS - 4) < (1 << 20), "the prefix sum of segment bytes in an int");

// behind phase D bit 18 of a start's word says that the start is valid
constexpr uint32_t PW_VALID = 1u << 18;
__device__ inline bool es_invalid_start(uint32_t e) { return pw_start(e) && !(e & PW_VALID); }
// the packet's reset in front of its row and segment; its reset mark (an invalid start resets once more, behind its row)
__device__ inline bool es_reset_front(uint32_t e) { return (e & PW_GAP) || (pw_counts(e) && pw_scr(e)); }
__device__ inline bool es_reset_mark(uint32_t e) { return es_reset_front(e) || es_invalid_start(e); }

// a stream's call record
template <typename Cnt>
struct EsStreamCall { EsCallHead head; Cnt cnt[ES_SLOTS]; };

// what the kernel keeps in LDS beside the packets (a bank may add to it); a multiple of 16 bytes in front of them
template <typename Cnt, typename State>
struct alignas(16) EsStreamShared {
    Cnt cnt[ES_SLOTS];
    State ss[ES_SLOTS];                          // the slots' states before the call
    uint16_t place[ES_SLOTS][ES_WG];             // the counting sort's counts, then places; behind the sort the bank's: an index per sorted packet
    int32_t tbase[ES_WG];                        // the rows in front of a thread's run of input packets
    int32_t w[ES_SLOTS], codec[ES_SLOTS];
    int32_t start[ES_SLOTS + 1];                 // the slots' runs in sorted order
    int32_t wsum[ES_WG / 64];
    uint8_t ncc[ES_SLOTS];                       // the slots' continuity bytes behind the call
    int64_t pos0;
};

// counters summed per thread and slot run
template <typename T>
struct EsStreamAcc {
    typename T::Cnt c; int slot; typename T::Cnt* dst;
    __device__ __forceinline__ EsStreamAcc(typename T::Cnt* d) : c{}, slot(-1), dst(d) {}
    __device__ __forceinline__ void at(int s) { if (s != slot) { done(); c = typename T::Cnt{}; slot = s; } }
    __device__ __forceinline__ void done() { if (slot >= 0) T::flush(&dst[slot], c); slot = -1; }
};

// One workgroup's call.  Dynamic LDS: T::Shared, srt[max_packets], exs[max_packets + 2] (32 bits each), then the bank's own.  The
// phases are parts of one kernel: forced inline, since a call would put the kernel's registers through the stack
template <typename T>
struct EsStream {
    typedef typename T::State State;
    typename T::Shared& sh;
    uint32_t* srt;                               // the sorted words
    uint32_t* exs;                               // a segment's length, then the exclusive prefix: the ES bytes of the call in front of it; exs[W] the call's
    const uint8_t* __restrict__ ts;
    int s, tid, n, max_rows;
    int W, j0, j1;                               // the watched packets; the thread's run of sorted places
    int ls0, lr0;                                // the last sorted start / packet with a reset mark before the thread's run

    __device__ __forceinline__ EsStream(unsigned char* lds, const uint8_t* const* __restrict__ in, const int* __restrict__ nbytes, int max_packets, int max_rows_)
        : sh(*reinterpret_cast<typename T::Shared*>(lds)), srt(reinterpret_cast<uint32_t*>(lds + sizeof(typename T::Shared))), exs(srt + max_packets),
          ts(in[blockIdx.x]), s(blockIdx.x), tid(threadIdx.x), n(nbytes[blockIdx.x] / TSMON_TS), max_rows(max_rows_), W(0), j0(0), j1(0), ls0(-1), lr0(-1) {
        if (n > max_packets) n = max_packets;        // (the host has refused such a call)
    }
    // the slot's synced bit behind its start ls (or none in this call)
    __device__ __forceinline__ bool synced_at(int slot, int ls) const { return ls >= sh.start[slot] ? (srt[ls] & PW_VALID) != 0 : T::synced(sh.ss[slot]); }
    // the slot's lost bit where its last row-bearing packet is p and its last reset mark r (both before the place, -1 or another slot's: none)
    __device__ __forceinline__ bool lost_behind(int slot, int p, int r) const {
        const int head = sh.start[slot];
        if (p >= head) return r > p || (r == p && es_invalid_start(srt[p]));
        return T::lost(sh.ss[slot]) || r >= head;
    }

    // The set-up and phases A-E; every thread of the workgroup calls it (what the kernel wrote to LDS before is behind a barrier here)
    // -> W > 0.  Then srt, exs, [j0, j1), ls0 and lr0 stand, and acc holds the thread's counters so far
    template <typename Hook>
    __device__ __forceinline__ bool front(const int32_t* __restrict__ watch, const int32_t* __restrict__ codec, const State* __restrict__ state, const int64_t* __restrict__ pos,
                          EsStreamAcc<T>& acc, Hook& hook) {
        if (tid < ES_SLOTS) {
            sh.w[tid] = watch[(size_t)s * ES_SLOTS + tid];
            sh.codec[tid] = codec[(size_t)s * ES_SLOTS + tid];
            sh.ss[tid] = state[(size_t)s * ES_SLOTS + tid];
            sh.cnt[tid] = typename T::Cnt{};
        }
        if (tid == 0) sh.pos0 = pos[s];
        __syncthreads();
        // A: the watched packets, compacted in input order
        uint32_t* rec = exs;
        W = pw_compact<ES_WG>(ts, n, sh.w, sh.wsum, rec);
        if (W <= 0) return false;
        // B: the stable counting sort by slot
        pw_sort<ES_WG>(rec, srt, W, sh.place, sh.start, sh.wsum, &j0, &j1);
        // C: the continuity verdicts
        unsigned dupm, gapm;
        pw_verdicts(srt, j0, j1, sh.start, [&](int slot) { return sh.ss[slot].cc; }, sh.wsum, sh.ncc,
                    [&](int slot, const PwPk& pk) { pw_flush_pk(&sh.cnt[slot], pk); }, &dupm, &gapm);
        __syncthreads();                                         // every counter has been read: the verdicts take their bits
        // D: the starts: valid or not, and their segments
        int last_start = -1;
        for (int j = j0; j < j1; ++j) {
            uint32_t e = pw_with_verdict(srt[j], dupm >> (j - j0) & 1, gapm >> (j - j0) & 1);
            if (pw_start(e)) {
                uint32_t w5[5];
                pw_load_start(ts, e, w5);
                const EsPlan pl = es_packet_plan(w5, pw_len(e), pw_scr(e), 1, false, false);
                if (pl.valid) e |= PW_VALID;
                exs[j] = (uint32_t)pl.seg_len;
                acc.at(pw_slot(e));
                es_cnt_start(&acc.c, pl);
                last_start = j;
            }
            srt[j] = e;
            hook.placed(j);
        }
        __syncthreads();
        ls0 = ts_block_scan_max(last_start, sh.wsum);
        // E: the segment lengths, the reset marks
        int ls = ls0, sum = 0, lr = -1;
        for (int j = j0; j < j1; ++j) {
            const uint32_t e = srt[j];
            const int slot = pw_slot(e);
            acc.at(slot);
            int len = 0;
            if (pw_start(e)) { len = (int)exs[j]; ls = j; }
            else if (pw_counts(e) && !pw_scr(e)) {
                if (synced_at(slot, ls)) len = pw_len(e); else acc.c.bytes_unsynced += pw_len(e);
            }
            exs[j] = (uint32_t)len;
            sum += len;
            acc.c.es_bytes += len;
            if (es_reset_mark(e)) { lr = j; ++acc.c.resets; }
            hook.first(j, e, len);
        }
        int total;
        int at = ts_block_scan<ES_WG>(sum, sh.wsum, &total);
        lr0 = ts_block_scan_max(lr, sh.wsum);
        hook.between(sh.wsum);
        for (int j = j0; j < j1; ++j) {
            const int len = (int)exs[j];
            exs[j] = (uint32_t)at; at += len;
            hook.second(j, srt[j], len);
        }
        if (tid == 0) exs[W] = (uint32_t)total;
        __syncthreads();
        return true;
    }

    // The last phase, behind a barrier that follows the bank's counting of rc[k], the rows of INPUT packet k: the rows' places in input
    // order, the slot's last row-bearing packet (last_row: the thread's own last one, -1: none), the PES rows and the new states -> the
    // rows of the call.  other_rows(j, e, es_pos, lr, rank, lost): the rows of sorted packet j beyond its PES row, lr the last reset mark
    // before j; finish(nx, slot, j, lr): the bank's part of the state behind the slot's last packet j, lr the last reset mark up to j
    template <typename Rc, typename OtherRows, typename Finish>
    __device__ __forceinline__ int rows(const Rc* rc, int last_row, typename T::Row* __restrict__ rows_g, State* __restrict__ state, OtherRows other_rows, Finish finish) {
        const int chunk = (n + ES_WG - 1) / ES_WG;
        int nrows;
        {
            int k0, k1; ts_thread_run(n, ES_WG, &k0, &k1);
            int sum = 0;
            for (int k = k0; k < k1; ++k) sum += rc[k];
            sh.tbase[tid] = ts_block_scan<ES_WG>(sum, sh.wsum, &nrows);
        }
        int lp = ts_block_scan_max(last_row, sh.wsum);
        __syncthreads();
        typename T::Row* rows = rows_g + (size_t)s * max_rows;
        int lr = lr0, ls = ls0;
        for (int j = j0; j < j1; ++j) {
            const uint32_t e = srt[j];
            const int slot = pw_slot(e), k = pw_k(e), head = sh.start[slot];
            const uint64_t es_pos = sh.ss[slot].es_count + (exs[j] - exs[head]);
            const int nr = rc[k];
            if (nr) {
                bool lost = es_reset_front(e) || lost_behind(slot, lp, lr);
                int rank = sh.tbase[k / chunk];
                for (int q = (k / chunk) * chunk; q < k; ++q) rank += rc[q];
                if (pw_start(e)) {
                    uint32_t w5[5];
                    pw_load_start(ts, e, w5);
                    const EsPlan pl = es_packet_plan(w5, pw_len(e), pw_scr(e), 1, false, false);
                    if (rank < max_rows) rows[rank] = T::pes_row(sh.w[slot], slot, k, pl, es_pos, lost);
                    lost = false;
                    ++rank;
                }
                if (nr > pw_start(e)) other_rows(j, e, es_pos, lr, rank, lost);
                lp = j;
            }
            if (es_reset_mark(e)) lr = j;
            if (pw_start(e)) ls = j;
            if (j == sh.start[slot + 1] - 1) {
                State nx = sh.ss[slot];
                nx.es_count += exs[j + 1] - exs[head];
                nx.cc = sh.ncc[slot];
                T::set_synced_lost(nx, synced_at(slot, ls), lost_behind(slot, lp, lr));
                finish(nx, slot, j, lr);
                state[(size_t)s * ES_SLOTS + slot] = nx;
            }
        }
        __syncthreads();
        return nrows;
    }

    // the call record and the stream's position; every thread calls it, with the rows of the call (0 where W == 0)
    __device__ __forceinline__ void finish(EsStreamCall<typename T::Cnt>* __restrict__ call, int64_t* __restrict__ pos, int nrows) {
        if (tid < ES_SLOTS) call[s].cnt[tid] = sh.cnt[tid];
        if (tid == 0) {
            call[s].head = EsCallHead{nrows, {0, 0, 0}};
            pos[s] = sh.pos0 + n;
        }
    }
};

// ------------------------------------------------------------------------------------------------- the host half
// What the two banks' descriptions for watch_bank.h share: a codec per slot as the configuration, account() and launch().  D, the
// bank's description, derives from it and names the rest; KERNEL, LDS_BYTES: the kernel and its dynamic LDS for max_packets;
// COUNTERS: the words of the bank's counters, every one a sum
template <typename D, typename T, void (*KERNEL)(const uint8_t* const*, const int*, int, int, const int32_t*, const int32_t*, typename T::State*, int64_t*, typename T::Row*,
                                                  EsStreamCall<typename T::Cnt>*),
          size_t (*LDS_BYTES)(int), int COUNTERS>
struct EsStreamBankD {
    static constexpr int SLOTS = ES_SLOTS, MAX_PACKETS = ES_MAX_PACKETS;
    typedef typename T::State State; typedef typename T::Row Row; typedef EsStreamCall<typename T::Cnt> Call;
    static constexpr int SUMS = COUNTERS;              // every word of the bank's statistics is a counter
    typedef int32_t Config;                            // the codec, per slot
    static constexpr int CONFIGS = ES_SLOTS;
    static constexpr Config NO_CONFIG = 0;

    // one stream's call into its statistics; `n` packets came
    static void account(WatchBank<D>& b, int i, int n, const EsCallHead& head, const typename T::Cnt* c) {
        for (int s = 0; s < ES_SLOTS; ++s) {
            if (!c[s].packets) continue;                   // (no packet of the slot's PID came: every counter is 0)
            const int32_t* a = reinterpret_cast<const int32_t*>(&c[s]);
            int64_t* d = reinterpret_cast<int64_t*>(&b.stats[(size_t)i * ES_SLOTS + s]);
            for (int k = 0; k < COUNTERS; ++k) d[k] += a[k];
        }
        b.sstats[i].packets += n;
        if (head.rows > b.max_rows) b.sstats[i].rows_dropped += head.rows - b.max_rows;
        b.total[i] = head.rows;
        b.nrows[i] = head.rows < b.max_rows ? head.rows : b.max_rows;
    }
    static void launch(WatchBank<D>& b, const TsBankArgs& a, hipStream_t st) {
        hipLaunchKernelGGL(KERNEL, dim3(b.nstreams), dim3(ES_WG), LDS_BYTES(b.max_packets), st, a.in(b.d_args), a.nbytes(b.d_args), b.max_packets, b.max_rows, b.d_watch, b.d_cfg,
                           b.d_state, b.d_pos, b.d_rows, b.d_call);
    }
    template <typename S> static void fix_stream_stats(S*) {}
};

// the body of set_watch: the codec is 1 .. codecs, or `text` is the error
template <typename H>
int es_stream_set_watch(H* b, int stream, int slot, int pid, int codec, int codecs, const char* text) {
    if (!watch_slot_ok(b, stream, slot, pid)) return DVBS2GPU_ERR_ARG;
    if (pid >= 0 && (codec < 1 || codec > codecs)) { last_error() = text; return DVBS2GPU_ERR_ARG; }
    if (const int e = watch_set_watch(b, stream, slot, pid)) return e;
    const size_t at = (size_t)stream * ES_SLOTS + slot;
    b->cfg[at] = pid >= 0 ? codec : 0;
    if (b->ctx) return watch_upload_config(b, at);
    b->host[stream].codec[slot] = b->cfg[at];
    return 0;
}

}  // namespace s2
