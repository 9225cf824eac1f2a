// ES bank (own extension; include/dvbs2gpu.h): picture, GOP and parameter-set index of up to 16 watched video PIDs
// (MPEG-2, H.264, H.265) of each of `nstreams` transport streams in HBM -- the first TS bank that reads every payload byte.  Every rule
// is in es_rules.h, whose EsHostStream is the sequential definition, the host bank and the kernel's yardstick; this file says how a
// call's packets and their bytes are taken in parallel.
//
// What makes the parallel form possible: whether a slot is synced in front of a packet is the validity of its last start; with it every
// packet's segment of ES bytes is known from its own bytes, so a segment's ES position is a prefix sum and the bytes since the last
// reset a difference of two prefix values; and a code is a pure function of the last 8 ES bytes, so the lane of a packet needs, beside
// its own segment, only the 7 bytes in front of it, which lie at the END of the slot's previous non-empty segments.
//
//   es_kernel  one workgroup per stream, one launch per call.
//     A-E  es_stream.h, shared with the audio bank (A-C: ts_watch.h, shared with the PES bank too): the trusted packets of watched PIDs
//        as one word each, sorted by slot, with the continuity verdict; the starts' plans (es_packet_plan: valid or not into the word);
//        every packet's segment of ES bytes from its slot's last start (synced = that start was valid, or the carried bit), the ES
//        positions by one prefix sum, the last packet with a reset mark before a packet.  This bank's hook adds the last non-empty
//        segment before a packet.
//     F  every lane rolls the 64-bit window over its packets' segments (dwords at fixed places inside the packet), starting from the 7
//        bytes in front: at most 7 hops back over non-empty segments (a payload may be one byte), then the carried tail.  Codes are
//        counted and classified, rows counted per packet.
//     G  es_stream.h: a prefix sum over the rows per packet in INPUT order gives every packet its place in the table; a maximum scan
//        the slot's last row-bearing packet before one (RESYNC: a reset mark behind it).  The PES rows are written; a packet with code
//        rows is scanned once more to write them.  The lane of the slot's last packet writes the slot's new state: here its window.
// No lane walks over packets of other lanes beyond the 7 hops: the cost of a call does not depend on what the packets say, but for the
// second scan of packets that hold codes with rows.  One device-to-host copy of the per-stream call record (EsCall).
// Vector stores and plain C++ only.
#include "es_stream.h"

using namespace s2;

namespace s2 {

static_assert(sizeof(EsRow) == sizeof(dvbs2gpu_es_row) && sizeof(EsRow) == 48, "row layout");
static_assert(sizeof(EsCnt) * 2 == sizeof(dvbs2gpu_es_stats), "stats order");
static_assert(sizeof(EsState) == 24, "state layout");
static_assert(ES_NONE == 0 && ES_MPEG2 == DVBS2GPU_ES_MPEG2 && ES_H264 == DVBS2GPU_ES_H264 && ES_H265 == DVBS2GPU_ES_H265, "public values");
static_assert(ES_PES == DVBS2GPU_ES_UNIT_PES && ES_PICTURE == DVBS2GPU_ES_UNIT_PICTURE && ES_END == DVBS2GPU_ES_UNIT_END, "public values");
static_assert(ES_KEY == DVBS2GPU_ES_KEY && ES_RESYNC == DVBS2GPU_ES_RESYNC && ES_UNSYNCED == DVBS2GPU_ES_UNSYNCED && ES_SPLIT_HEADER == DVBS2GPU_ES_SPLIT_HEADER, "public values");

// what the bank is to es_stream.h
struct EsT {
    typedef EsState State; typedef EsCnt Cnt; typedef EsRow Row;
    typedef EsStreamShared<EsCnt, EsState> Shared;   // place[]: behind the sort the last non-empty segment before each sorted packet
    __device__ static void flush(EsCnt* d, const EsCnt& a) {
#define ES_ADD(f) if (a.f) atomicAdd(&d->f, a.f)
        ES_ADD(es_bytes); ES_ADD(bytes_unsynced); ES_ADD(resets); ES_ADD(pes_starts); ES_ADD(pes_invalid); ES_ADD(split_headers);
        ES_ADD(codes); ES_ADD(pictures); ES_ADD(pictures_i); ES_ADD(pictures_p); ES_ADD(pictures_b); ES_ADD(key_pictures); ES_ADD(sequences); ES_ADD(gops);
        ES_ADD(params); ES_ADD(auds); ES_ADD(ends); ES_ADD(slices); ES_ADD(other_codes); ES_ADD(bad_codes);
#undef ES_ADD
    }
    __device__ static bool synced(const EsState& st) { return st.synced != 0; }
    __device__ static bool lost(const EsState& st) { return st.lost != 0; }
    __device__ static void set_synced_lost(EsState& st, bool synced, bool lost) { st.synced = synced; st.lost = lost; }
    __device__ static EsRow pes_row(int pid, int slot, int k, const EsPlan& pl, uint64_t es_pos, bool lost) { return es_pes_row(pid, slot, k, pl, es_pos, lost); }
};
typedef EsT::Shared EsShared;
typedef EsStreamCall<EsCnt> EsCall;
static_assert(sizeof(EsShared) % 16 == 0 && sizeof(EsShared::place) == ES_MAX_PACKETS * sizeof(uint16_t), "the packets behind it; an index per packet");
// dynamic LDS: EsShared, srt[max_packets], exs[max_packets + 1] (32 bits each), rc[max_packets] (16 bits): 10 bytes per packet
constexpr size_t es_lds_bytes(int max_packets) { return sizeof(EsShared) + ((size_t)max_packets * 2 + 2) * sizeof(uint32_t) + (((size_t)max_packets + 1) & ~(size_t)1) * sizeof(uint16_t); }
static_assert(es_lds_bytes(ES_MAX_PACKETS) <= 64 * 1024, "dynamic LDS of a workgroup");        // 51.3 KiB

constexpr uint16_t ES_NO_PREV = 0xFFFF;

// the last 8 bytes of packet k, the packet's last byte in the low byte: two dwords that lie inside the packet
__device__ inline uint64_t es_packet_end(const uint8_t* __restrict__ ts, int k) {
    const uint8_t* p = ts + (size_t)k * TSMON_TS + TSMON_TS - 8;
    const uint32_t lo = *reinterpret_cast<const ts_unaligned_u32*>(p), hi = *reinterpret_cast<const ts_unaligned_u32*>(p + 4);
    return (uint64_t)__builtin_bswap32(lo) << 32 | __builtin_bswap32(hi);
}
__device__ inline uint64_t es_low_bytes(uint64_t v, int t) { return t >= 8 ? v : v & ((1ull << (8 * t)) - 1); }

// The segment of the packet k: its last `len` bytes, at ES position `pos`, scanned from the window (win, since) in front of it.  The
// dwords are read at multiples of 4 inside the packet.  ROWS false: the codes are counted into *c -> the codes with a row.  ROWS
// true: the rows are written at rows[rank ..] below max_rows, the first with RESYNC if `lost` -> the codes with a row
template <bool ROWS>
__device__ inline int es_scan_segment(const uint8_t* __restrict__ ts, int k, int len, uint64_t pos, uint64_t win, uint32_t since, int codec, EsCnt* c, int pid, int slot,
                                      bool lost, EsRow* rows, int rank, int max_rows) {
    const uint8_t* p = ts + (size_t)k * TSMON_TS;
    const int a = TSMON_TS - len;
    int nrows = 0;
    for (int d = a >> 2; d < TSMON_TS / 4; ++d) {
        const uint32_t v = *reinterpret_cast<const ts_unaligned_u32*>(p + 4 * d);
#pragma unroll
        for (int b = 0; b < 4; ++b) {
            const int idx = 4 * d + b;
            if (idx < a) continue;
            uint32_t code, head;
            if (!es_scan_byte(&win, &since, v >> (8 * b) & 255, &code, &head)) continue;
            const EsCode e = es_classify(codec, code, head);
            if (!ROWS) es_cnt_code(c, e);
            if (e.unit >= ES_UNITS) continue;
            if (ROWS) {
                if (rank + nrows < max_rows) rows[rank + nrows] = es_code_row(pid, slot, k, e, code, head, pos + (uint64_t)(idx - a) - 7, lost);
                lost = false;
            }
            ++nrows;
        }
    }
    return nrows;
}

// The kernel keeps its own text of the set-up, phases A-E and the skeleton of G, which aud_kernel takes from es_stream.h (EsStream):
// written on EsStream, with all but identical instructions, this kernel took 0.80 ms where this text takes 0.70 ms (4096 streams x 309
// packets), and the cause was not found.  A change to either text belongs in the other too; the word predicates,
// the accumulator, the LDS struct, the call record and the host half are es_stream.h's
__global__ void __launch_bounds__(ES_WG) es_kernel(const uint8_t* const* __restrict__ in, const int* __restrict__ nbytes, int max_packets, int max_rows,
                                                   const int32_t* __restrict__ watch, const int32_t* __restrict__ codec, EsState* __restrict__ state,
                                                   int64_t* __restrict__ pos, EsRow* __restrict__ rows_g, EsCall* __restrict__ call) {
    extern __shared__ __attribute__((aligned(16))) unsigned char es_lds[];
    EsShared& sh = *reinterpret_cast<EsShared*>(es_lds);
    uint32_t* srt = reinterpret_cast<uint32_t*>(es_lds + sizeof(EsShared));
    uint32_t* exs = srt + max_packets;               // a segment's length, then the exclusive prefix: the ES bytes of the call in front of it
    uint16_t* rc = reinterpret_cast<uint16_t*>(exs + max_packets + 2);   // rows per INPUT packet
    uint32_t* rec = exs;
    uint16_t* prevne = &sh.place[0][0];
    const int s = blockIdx.x, tid = threadIdx.x;
    int n = nbytes[s] / TSMON_TS;
    if (n > max_packets) n = max_packets;            // (the host has refused such a call)
    if (tid < ES_SLOTS) {
        sh.w[tid] = watch[(size_t)s * ES_SLOTS + tid];
        sh.codec[tid] = codec[(size_t)s * ES_SLOTS + tid];
        sh.ss[tid] = state[(size_t)s * ES_SLOTS + tid];
        sh.cnt[tid] = es_cnt_zero();
    }
    for (int k = tid; k < n; k += ES_WG) rc[k] = 0;
    if (tid == 0) sh.pos0 = pos[s];
    __syncthreads();
    const uint8_t* ts = in[s];
    // A: the watched packets, compacted in input order
    const int W = pw_compact<ES_WG>(ts, n, sh.w, sh.wsum, rec);
    int nrows = 0;
    if (W > 0) {
        // B: the stable counting sort by slot
        int j0, j1;
        pw_sort<ES_WG>(rec, srt, W, sh.place, sh.start, sh.wsum, &j0, &j1);
        // C: the continuity verdicts
        unsigned dupm, gapm;
        pw_verdicts(srt, j0, j1, sh.start, [&](int slot) { return sh.ss[slot].cc; }, sh.wsum, sh.ncc,
                    [&](int slot, const PwPk& pk) { pw_flush_pk(&sh.cnt[slot], pk); }, &dupm, &gapm);
        __syncthreads();                                         // every counter has been read: the verdicts take their bits
        EsStreamAcc<EsT> acc(sh.cnt);
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
        }
        __syncthreads();
        const int ls0 = ts_block_scan_max(last_start, sh.wsum);   // the last sorted start before the thread's run
        // the slot's synced bit behind its start ls (or none in this call)
        auto synced_at = [&](int slot, int ls) { return ls >= sh.start[slot] ? (srt[ls] & PW_VALID) != 0 : sh.ss[slot].synced != 0; };
        // E: the segment lengths, the reset marks
        int lr0 = -1, ne0 = -1;
        {
            int ls = ls0, sum = 0, lr = -1, ne = -1;
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
                if (len > 0) ne = j;
            }
            int total;
            int at = ts_block_scan<ES_WG>(sum, sh.wsum, &total);
            lr0 = ts_block_scan_max(lr, sh.wsum);                // the last sorted packet with a reset mark before the run,
            ne0 = ts_block_scan_max(ne, sh.wsum);                // and the last one with a non-empty segment
            ne = ne0;
            for (int j = j0; j < j1; ++j) {
                const int len = (int)exs[j];
                exs[j] = (uint32_t)at; at += len;
                prevne[j] = ne >= 0 ? (uint16_t)ne : ES_NO_PREV;
                if (len > 0) ne = j;
            }
            if (tid == 0) exs[W] = (uint32_t)total;
        }
        __syncthreads();
        // the window in front of sorted place j of `slot` (j may be the end of the slot's run): lr the last reset mark before or at j,
        // pne the last non-empty segment before j
        auto window = [&](int slot, int j, int lr, int pne, uint64_t* win, uint32_t* since) {
            const int head = sh.start[slot];
            const uint32_t sn = lr >= head ? exs[j] - exs[lr] : (uint32_t)sh.ss[slot].have + (exs[j] - exs[head]);
            const int need = sn < 7 ? (int)sn : 7;
            uint64_t v = 0;
            int got = 0, jj = pne;
            for (int hop = 0; hop < 7 && got < need; ++hop) {
                if (jj < head) break;
                const int len = (int)(exs[jj + 1] - exs[jj]), t = len < need - got ? len : need - got;
                v |= es_low_bytes(es_packet_end(ts, pw_k(srt[jj])), t) << (8 * got);
                got += t;
                jj = prevne[jj] == ES_NO_PREV ? -1 : (int)prevne[jj];
            }
            if (got < need) v |= es_low_bytes(sh.ss[slot].tail, need - got) << (8 * got);
            *win = v; *since = (uint32_t)need;
        };
        // F: the codes, counted; the rows per packet
        int last_row = -1;
        {
            int lr = lr0, ne = ne0;
            for (int j = j0; j < j1; ++j) {
                const uint32_t e = srt[j];
                const int slot = pw_slot(e), k = pw_k(e), len = (int)(exs[j + 1] - exs[j]);
                acc.at(slot);
                if (es_reset_mark(e)) lr = j;
                int nr = pw_start(e);
                if (len > 0) {
                    uint64_t win; uint32_t since;
                    window(slot, j, lr, ne, &win, &since);
                    nr += es_scan_segment<false>(ts, k, len, 0, win, since, sh.codec[slot], &acc.c, 0, 0, false, nullptr, 0, 0);
                    ne = j;
                }
                if (nr) { rc[k] = (uint16_t)nr; last_row = j; }
            }
        }
        acc.done();
        __syncthreads();
        // G: the rows' places in input order, the slot's last row-bearing packet, the rows and the new states
        const int chunk = (n + ES_WG - 1) / ES_WG;
        {
            int k0, k1; ts_thread_run(n, ES_WG, &k0, &k1);
            int sum = 0;
            for (int k = k0; k < k1; ++k) sum += rc[k];
            sh.tbase[tid] = ts_block_scan<ES_WG>(sum, sh.wsum, &nrows);
        }
        int lp = ts_block_scan_max(last_row, sh.wsum);
        __syncthreads();
        EsRow* rows = rows_g + (size_t)s * max_rows;
        int lr = lr0, ne = ne0, ls = ls0;
        // the slot's lost bit where its last row-bearing packet is p and its last reset mark r (both before the place, -1 or another slot's: none)
        auto lost_behind = [&](int slot, int p, int r) {
            const int head = sh.start[slot];
            if (p >= head) return r > p || (r == p && es_invalid_start(srt[p]));
            return sh.ss[slot].lost != 0 || r >= head;
        };
        for (int j = j0; j < j1; ++j) {
            const uint32_t e = srt[j];
            const int slot = pw_slot(e), k = pw_k(e), head = sh.start[slot], len = (int)(exs[j + 1] - exs[j]);
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
                    if (rank < max_rows) rows[rank] = es_pes_row(sh.w[slot], slot, k, pl, es_pos, lost);
                    lost = false;
                    ++rank;
                }
                if (nr > pw_start(e)) {
                    uint64_t win; uint32_t since;
                    window(slot, j, es_reset_mark(e) ? j : lr, ne, &win, &since);
                    es_scan_segment<true>(ts, k, len, es_pos, win, since, sh.codec[slot], nullptr, sh.w[slot], slot, lost, rows, rank, max_rows);
                }
                lp = j;
            }
            if (es_reset_mark(e)) lr = j;
            if (len > 0) ne = j;
            if (pw_start(e)) ls = j;
            if (j == sh.start[slot + 1] - 1) {
                EsState nx = sh.ss[slot];
                uint64_t win; uint32_t since;
                window(slot, j + 1, lr, ne, &win, &since);
                nx.es_count += exs[j + 1] - exs[head];
                nx.tail = win; nx.have = (uint8_t)since;
                nx.cc = sh.ncc[slot];
                nx.synced = synced_at(slot, ls);
                nx.lost = lost_behind(slot, lp, lr);
                state[(size_t)s * ES_SLOTS + slot] = nx;
            }
        }
        __syncthreads();
    }
    if (tid < ES_SLOTS) call[s].cnt[tid] = sh.cnt[tid];
    if (tid == 0) {
        call[s].head = EsCallHead{nrows, {0, 0, 0}};
        pos[s] = sh.pos0 + n;
    }
}

}  // namespace s2

// the host half is the watched-PID bank's (watch_bank.h) with what es_stream.h adds for a bank with a codec per slot; here what is the bank's own
struct EsBankD : EsStreamBankD<EsBankD, EsT, es_kernel, es_lds_bytes, ES_COUNTERS> {
    typedef EsHostStream HostStream; typedef dvbs2gpu_es_stats Stats; typedef dvbs2gpu_es_stream_stats StreamStats;
    static constexpr StreamStats NO_STREAM_STATS = {};
    static constexpr const char *BANK = "ES bank: ", *CNAME = "dvbs2gpu_es", *ALLOC = "hipMalloc(es)";
};
struct dvbs2gpu_es : WatchBank<EsBankD> {};

extern "C" {

void dvbs2gpu_es_destroy(dvbs2gpu_es* b) { delete b; }
int dvbs2gpu_es_create(dvbs2gpu_ctx* ctx, int nstreams, int max_packets, int max_rows, dvbs2gpu_es** out) { return watch_create(true, ctx, nstreams, max_packets, max_rows, out); }
int dvbs2gpu_es_create_host(int nstreams, int max_packets, int max_rows, dvbs2gpu_es** out) { return watch_create(false, nullptr, nstreams, max_packets, max_rows, out); }
int dvbs2gpu_es_reset(dvbs2gpu_es* b) { return watch_reset(b); }

int dvbs2gpu_es_set_watch(dvbs2gpu_es* b, int stream, int slot, int pid, int codec) {
    return es_stream_set_watch(b, stream, slot, pid, codec, ES_H265, "ES bank: the codec is DVBS2GPU_ES_MPEG2, _H264 or _H265");
}

int dvbs2gpu_es_process_batch(dvbs2gpu_es* b, const uint8_t* const* d_ts, const int* nbytes, int* out_rows, void* stream) {
    return watch_process_batch(b, d_ts, nbytes, out_rows, stream);
}
int dvbs2gpu_es_work(dvbs2gpu_es* b, int stream, const uint8_t* h_ts, int nbytes) { return watch_work(b, stream, h_ts, nbytes); }
int dvbs2gpu_es_get_stats(dvbs2gpu_es* b, int stream, int slot, dvbs2gpu_es_stats* h_out) { return watch_get_stats(b, stream, slot, h_out); }
int dvbs2gpu_es_get_stream_stats(dvbs2gpu_es* b, int stream, dvbs2gpu_es_stream_stats* h_out) { return watch_get_stream_stats(b, stream, h_out); }
int dvbs2gpu_es_get_row_table(dvbs2gpu_es* b, int stream, dvbs2gpu_es_row* h_rows, int cap, int* n) { return watch_get_row_table(b, stream, h_rows, cap, n); }
int dvbs2gpu_es_get_row_table_device(dvbs2gpu_es* b, int stream, const dvbs2gpu_es_row** d_rows, int* n) { return watch_get_row_table_device(b, stream, d_rows, n); }

}  // extern "C"
