// T2-MI bank (own extension; include/dvbs2gpu.h): the T2-MI packets of a PID of each of `nstreams` transport streams
// in HBM, reassembled, checked (CRC-32, packet count) and the BBFRAMEs of the chosen PLP laid back to back for the mode-adaptation
// packetiser.  Every rule is in t2mi_rules.h, whose T2miHostStream is the sequential definition, the host bank and the kernels'
// yardstick; this file says how a call's packets are cut into independent pieces.
//
// What makes the parallel form possible is the section bank's observation (psi.hip): a T2-MI packet STARTS only behind the pointer
// field of a PUSI packet, so the chain of headers of a TS packet starts at its own pointer and never leaves it; only the LAST T2-MI
// packet begun in a PUSI packet reaches into later TS packets, at most to the pointer bytes of the slot's next PUSI packet.
//
//   t2mi_scan_kernel    one workgroup per (stream, slot): the slots are independent reassemblers, an empty one returns at once, and
//                       a slot sees one PID, so there is no sort by slot.
//     A  every header is read once (ts_load_header) and the slot's packets are compacted in input order into LDS with payload start
//        and pointer byte.
//     B  one lane takes the continuity steps in order and classes each packet: SKIP, CUT, CONT, PUSI, PUSI behind a break.
//     C  one lane per PUSI packet hops from header to header inside its packet and follows the T2-MI packet that the TS packet's end
//        cuts (a header split after 1 to 5 bytes too) until it is complete, dropped or the call ends; one lane does the same for the
//        packet carried in.  Count, prefix sum, then one record per row.
//     D  one wave per row: each lane takes the CRC of one PIECE of the packet (its bytes in one TS payload, at most 184; 46 pieces at
//        8202 bytes, 64 a round) from a zero register, reading the bytes from the TS payloads where they lie (a gathered copy of
//        4 x 8202 bytes beside the packet list would not leave two workgroups per CU their LDS), the registers are shifted to the
//        packet's end (crc32m_mulmod, crc32m_xpow) and summed; lane 0 reads the nine bytes the row needs.
//     E  COUNT_ERROR: "the last valid row before mine" is an exclusive maximum scan over the rows; two prefix sums over the delivered
//        rows give their offsets and their places in the frame-size list.
//   t2mi_commit_kernel  (once the host has seen that every slot's bytes and rows fit) one workgroup per (stream, slot): a wave per
//     delivered row copies the BBFRAME's pieces to its offset, a dword per lane behind the unaligned head; then the open packet goes
//     to the slot's 8208-byte buffer and the state is stored.
// Two launches per call and one device-to-host copy, of the call record per (stream, slot).
#include "ts_bank.h"
#include "t2mi_rules.h"

#include <memory>

using namespace s2;
#define g_err last_error()

namespace s2 {

constexpr int T2_MAX_PACKETS = 4096;             // per stream and call: 10 bytes of LDS per packet
constexpr int T2_WG = 256, T2_WAVES = T2_WG / 64;
static_assert(sizeof(T2miRow) == sizeof(dvbs2gpu_t2mi_row) && sizeof(T2miRow) == 32, "row layout");
static_assert(sizeof(T2miLayout) == sizeof(dvbs2gpu_t2mi_layout), "layout layout");
static_assert(T2_MAX_PACKETS <= 32 * T2_WG, "t2_collect keeps a thread's match flags in one 32-bit mask (ts_thread_run)");
static_assert(sizeof(T2miCnt) == T2MI_NCNT * sizeof(int32_t), "counter order");
static_assert(sizeof(dvbs2gpu_t2mi_stats) == T2MI_NCNT * sizeof(int64_t), "stats order");
static_assert(T2MI.max_packet_bytes <= T2MI_BUF && T2MI.max_packet_bytes < (1 << 17), "crc32m_xpow takes 17 bits of length");

enum { T2K_SKIP = 0, T2K_CUT, T2K_CONT, T2K_PUSI, T2K_PUSI_BRK };
enum { T2C_PACKETS = 0, T2C_T2MI, T2C_CRC, T2C_COUNT, T2C_BB, T2C_BADPAY, T2C_DELIVERED, T2C_BYTES, T2C_DROPPED, T2C_MALPKT, T2C_SCR, T2C_SLACK };

struct T2DevSlot { int32_t fill; uint8_t cont, has_count, last_count, pad; };
// a T2-MI packet of the call: its first byte at offset `at` of the slot's packet j0 (j0 -1: carried in, the slot's buffer comes first),
// its last byte in the slot's packet j1.  As the open packet of a slot: j0 -2 none, total the bytes so far
struct T2Rec { int32_t j0, j1, at, total; };
struct T2Call { int32_t needed, nrows, watched, ndelivered; T2miCnt cnt; };

// a packet of the slot in LDS.  wa: index k bits 0-12, class 13-15 (after the walk); before it CC 16-19, AFC 20-21, DI 22, PUSI 23,
// scrambled 24.  wb: payload start (188: none) | pointer byte << 8
__device__ inline int t2_k(unsigned e) { return (int)(e & 0x1fff); }
__device__ inline int t2_kind(unsigned e) { return (int)(e >> 13 & 7); }

struct T2View {                                  // what the packet walkers read of one (stream, slot)
    const uint8_t* ts; const unsigned* wa; const uint16_t* wb; int W;
    const uint8_t* sbuf;                         // the slot's packet buffer
    int fill0;                                   // its bytes before the call
};
struct T2Out { int* rc; T2Rec* rec; T2Rec* open; T2DevSlot* nss; int* cnt; int max_rows; };

// the pieces of packet r that hold its bytes [0, limit), in order: f(position in the packet, source, bytes)
template <typename F>
__device__ inline void t2_pieces(const T2Rec& r, const T2View& v, int limit, F f) {
    const int total = r.total < limit ? r.total : limit;
    int pos, jn = 0;
    if (r.j0 < 0) {
        pos = v.fill0 < total ? v.fill0 : total;
        f(0, v.sbuf, pos);
    } else {
        pos = TSMON_TS - r.at < total ? TSMON_TS - r.at : total;
        f(0, v.ts + (size_t)t2_k(v.wa[r.j0]) * TSMON_TS + r.at, pos);
        jn = r.j0 + 1;
    }
    for (int j = jn; pos < total && j < v.W; ++j) {
        const unsigned e = v.wa[j];
        const int kind = t2_kind(e);
        if (kind == T2K_SKIP) continue;
        if (kind != T2K_CONT && kind != T2K_PUSI) break;
        const int ps = v.wb[j] & 255, lo = kind == T2K_PUSI ? ps + 1 : ps, avail = kind == T2K_PUSI ? v.wb[j] >> 8 : TSMON_TS - ps;
        const int len = avail < total - pos ? avail : total - pos;
        f(pos, v.ts + (size_t)t2_k(e) * TSMON_TS + lo, len);
        pos += len;
    }
}

// The open packet -- `fill` bytes so far, header bytes b4, b5 where fill reaches them, first byte at (j0, at) -- through the slot's
// packets from jn on: rules 4 and 5.  One lane.
template <bool WRITE>
__device__ void t2_resolve(const T2View& v, const T2Out& o, int j0, int at, int fill, unsigned b4, unsigned b5, int jn) {
    enum { R_OPEN, R_DONE, R_DROPPED };
    int outcome = R_OPEN, endj = -1, total = 0;
    bool slack = false;
    for (int j = jn; j < v.W; ++j) {
        const unsigned e = v.wa[j];
        const int kind = t2_kind(e);
        if (kind == T2K_SKIP) continue;
        if (kind == T2K_CUT || kind == T2K_PUSI_BRK) { outcome = R_DROPPED; break; }
        const int ps = v.wb[j] & 255, lo = kind == T2K_PUSI ? ps + 1 : ps, avail = kind == T2K_PUSI ? v.wb[j] >> 8 : TSMON_TS - ps;
        const uint8_t* p = v.ts + (size_t)t2_k(e) * TSMON_TS + lo;
        int used = 0;
        while (fill < T2MI.header_bytes && used < avail) {
            const unsigned byte = p[used++];
            if (fill == 4) b4 = byte; else if (fill == 5) b5 = byte;
            ++fill;
        }
        if (fill >= T2MI.header_bytes) {
            total = t2mi_total(b4, b5);
            const int take = avail - used < total - fill ? avail - used : total - fill;
            fill += take; used += take;
            if (fill == total) { outcome = R_DONE; endj = j; slack = kind == T2K_PUSI && used < avail; break; }
        }
        if (kind == T2K_PUSI) { outcome = R_DROPPED; break; }
    }
    if (outcome == R_DONE) {
        if (!WRITE) atomicAdd(&o.rc[endj], 1);
        else {
            const int r = o.rc[endj] >> 1;
            if (r < o.max_rows) { const T2Rec rec = {j0, endj, at, total}; o.rec[r] = rec; }
            if (slack) atomicAdd(&o.cnt[T2C_SLACK], 1);
        }
    } else if (WRITE) {
        if (outcome == R_DROPPED) atomicAdd(&o.cnt[T2C_DROPPED], 1);
        else { const T2Rec rec = {j0, v.W, at, fill}; *o.open = rec; o.nss->fill = fill; }
    }
}

// the slot's packet j, a PUSI packet: the T2-MI packets that start behind its pointer (rule 6).  One lane.
template <bool WRITE>
__device__ void t2_pusi_job(const T2View& v, const T2Out& o, int j) {
    const unsigned e = v.wa[j];
    const int ps = v.wb[j] & 255, ptr = v.wb[j] >> 8;
    const uint8_t* p = v.ts + (size_t)t2_k(e) * TSMON_TS;
    const int base = WRITE ? (o.rc[j] >> 1) + (o.rc[j] & 1) : 0;
    int at = ps + 1 + ptr, i = 0;
    while (at < TSMON_TS) {
        const int have = TSMON_TS - at;
        if (have >= T2MI.header_bytes) {
            const int total = t2mi_total(p[at + 4], p[at + 5]);
            if (total <= have) {
                if (WRITE && base + i < o.max_rows) { const T2Rec rec = {j, j, at, total}; o.rec[base + i] = rec; }
                ++i;
                at += total;
                continue;
            }
        }
        t2_resolve<WRITE>(v, o, j, at, have, have >= 5 ? p[at + 4] : 0, have >= 6 ? p[at + 5] : 0, j + 1);
        break;
    }
    if (!WRITE && i) atomicAdd(&o.rc[j], 2 * i);
}

template <bool WRITE>
__device__ void t2_jobs(const T2View& v, const T2Out& o) {
    for (int t = threadIdx.x; t < v.W + 1; t += T2_WG) {
        if (t == 0) {
            if (v.fill0 > 0) t2_resolve<WRITE>(v, o, -1, 0, v.fill0, v.fill0 >= 5 ? v.sbuf[4] : 0, v.fill0 >= 6 ? v.sbuf[5] : 0, 0);
        } else if (t2_kind(v.wa[t - 1]) >= T2K_PUSI) t2_pusi_job<WRITE>(v, o, t - 1);
    }
}

// phase A: the slot's packets of the stream into wa / wb, in input order; returns their number
__device__ int t2_collect(const uint8_t* __restrict__ ts, int n, int pid, unsigned* wa, uint16_t* wb, int* wsum) {
    int k0, k1; ts_thread_run(n, T2_WG, &k0, &k1);               // <= 16 packets per thread
    unsigned mask = 0;
    for (int k = k0; k < k1; ++k) {
        const TsmonHdr h = ts_load_header(ts, k);
        mask |= (unsigned)(h.cls == TSMON_DATA && h.pid == pid) << (k - k0);
    }
    int W;
    int at = ts_block_scan<T2_WG>(__popc(mask), wsum, &W);
    for (int k = k0; k < k1; ++k) {
        if (!(mask >> (k - k0) & 1)) continue;
        unsigned b4;
        const TsmonHdr h = ts_load_header(ts, k, &b4);
        int ps = t2mi_payload_start(h.afc, b4);
        if (ps > TSMON_TS) ps = TSMON_TS;
        const unsigned ptr = (h.pusi && (h.afc & 1) && ps < TSMON_TS) ? ts[(size_t)k * TSMON_TS + ps] : 0;
        wa[at] = (unsigned)k | (unsigned)h.cc << 16 | (unsigned)h.afc << 20 | (unsigned)h.di << 22 | (unsigned)h.pusi << 23 | (unsigned)(h.tsc != 0) << 24;
        wb[at] = (uint16_t)(ps | ptr << 8);
        ++at;
    }
    __syncthreads();
    return W;
}

// dynamic LDS: wa[max_packets] (dwords), rc[max_packets] (dwords), wb[max_packets] (16 bits each).  only >= 0: the one (stream, slot)
// that receives its stream's packets (the single-slot entry point); the others take an empty call
__global__ void __launch_bounds__(T2_WG) t2mi_scan_kernel(const uint8_t* const* __restrict__ in, const int* __restrict__ nbytes, int max_packets, int max_rows,
                                                          int only, const T2miWatch* __restrict__ watch, const T2DevSlot* __restrict__ state,
                                                          T2DevSlot* __restrict__ newst, const uint8_t* __restrict__ bufs, unsigned* __restrict__ wa_g,
                                                          uint16_t* __restrict__ wb_g, T2Rec* __restrict__ recs, T2Rec* __restrict__ opens,
                                                          T2miRow* __restrict__ rows_g, int* __restrict__ fb_g, T2Call* __restrict__ call, int have_out) {
    extern __shared__ __attribute__((aligned(16))) unsigned t2_lds[];
    __shared__ int cnt[T2MI_NCNT], wsum[T2_WAVES], last_valid;
    __shared__ T2DevSlot nss;
    const int g = blockIdx.x, s = g / T2MI_SLOTS, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const T2miWatch w = watch[g];
    if (w.pid < 0) {                                 // an empty slot: nothing carried, nothing to do
        if (tid == 0) {
            T2Call c = {};
            call[g] = c;
            const T2Rec none = {-2, 0, 0, 0};
            opens[g] = none;
            newst[g] = state[g];
        }
        return;
    }
    unsigned* wa = t2_lds;
    int* rc = reinterpret_cast<int*>(t2_lds + max_packets);
    uint16_t* wb = reinterpret_cast<uint16_t*>(t2_lds + 2 * (size_t)max_packets);
    int n = (only >= 0 && only != g) ? 0 : nbytes[s] / TSMON_TS;
    if (n > max_packets) n = max_packets;            // (the host has refused such a call)
    const T2DevSlot ss = state[g];
    if (tid == 0) {
        nss = ss;
        last_valid = -1;
        const T2Rec none = {-2, 0, 0, 0};
        opens[g] = none;
    }
    if (tid < T2MI_NCNT) cnt[tid] = 0;
    __syncthreads();
    const uint8_t* ts = in[s];
    const int W = n > 0 ? t2_collect(ts, n, w.pid, wa, wb, wsum) : 0;
    // B: the continuity walk, one lane
    if (tid == 0) {
        uint8_t st = ss.cont;
        int c_scr = 0, c_mal = 0;
        for (int j = 0; j < W; ++j) {
            const unsigned e = wa[j];
            const int cc = e >> 16 & 15, afc = e >> 20 & 3, di = e >> 22 & 1, pusi = e >> 23 & 1, ps = wb[j] & 255, ptr = wb[j] >> 8;
            int kind;
            const int v = tsmon_step(&st, afc, cc, di);
            const bool brk = v == TSMON_CC_ERROR || v == TSMON_DISC;
            if (e >> 24 & 1) { ++c_scr; kind = T2K_CUT; }
            else if (v == TSMON_DUPLICATE) kind = T2K_SKIP;
            else if (!(afc & 1)) kind = brk ? T2K_CUT : T2K_SKIP;
            else if (ps >= TSMON_TS || (pusi && ptr > TSMON_TS - ps - 1)) { ++c_mal; kind = T2K_CUT; }
            else if (pusi) kind = brk ? T2K_PUSI_BRK : T2K_PUSI;
            else kind = brk ? T2K_CUT : T2K_CONT;
            wa[j] = (e & 0x1fffu) | (unsigned)kind << 13;
        }
        nss.cont = st;
        nss.fill = 0;
        cnt[T2C_PACKETS] = W; cnt[T2C_SCR] = c_scr; cnt[T2C_MALPKT] = c_mal;
    }
    for (int j = tid; j < W; j += T2_WG) rc[j] = 0;
    __syncthreads();
    // C: T2-MI packets
    const T2View v = {ts, wa, wb, W, bufs + (size_t)g * T2MI_BUF, ss.fill};
    T2Rec* rec = recs + (size_t)g * max_rows;
    const T2Out o = {rc, rec, opens + g, &nss, cnt, max_rows};
    t2_jobs<false>(v, o);
    __syncthreads();
    int nrows;
    {
        int j0, j1; ts_thread_run(W, T2_WG, &j0, &j1);
        int mine = 0;
        for (int j = j0; j < j1; ++j) mine += (rc[j] >> 1) + (rc[j] & 1);
        int run = ts_block_scan<T2_WG>(mine, wsum, &nrows);
        for (int j = j0; j < j1; ++j) { const int c = rc[j]; rc[j] = run << 1 | (c & 1); run += (c >> 1) + (c & 1); }
    }
    __syncthreads();
    const bool fits = nrows <= max_rows;
    T2miRow* rows = rows_g + (size_t)g * max_rows;
    int needed = fits ? 0 : -1, ndelivered = 0;
    if (fits) {
        t2_jobs<true>(v, o);
        __syncthreads();
        // D: a wave per row
        for (int r = wave; r < nrows; r += T2_WAVES) {
            const T2Rec q = rec[r];
            // A lane per PIECE (the packet's bytes in one TS payload, at most 184), 64 pieces a round: the walk only notes the lane's
            // piece, and the CRC loops of all lanes then run side by side.  (A lane per 64th of the packet, taken inside the walk,
            // has two or three lanes at work in each of the packet's pieces: 26 ms per call of tools/t2mi_bench.py)
            const int total = q.total;
            uint32_t x = lane == 0 ? crc32m_mulmod(0xFFFFFFFFu, crc32m_xpow((uint32_t)total)) : 0;
            for (int base = 0;; base += 64) {
                int idx = 0, ppos = 0, plen = 0;                                   // idx: the same in every lane
                const uint8_t* psrc = nullptr;
                t2_pieces(q, v, total, [&](int pos, const uint8_t* src, int len) {
                    if (idx == base + lane) { ppos = pos; psrc = src; plen = len; }
                    ++idx;
                });
                uint32_t c = 0;
                int i = 0;
                for (; i + 4 <= plen; i += 4) {                                    // an unaligned dword inside the piece
                    const unsigned d = *reinterpret_cast<const ts_unaligned_u32*>(psrc + i);
                    for (int k = 0; k < 4; ++k) c = crc32m_byte(c, d >> (8 * k) & 255);
                }
                for (; i < plen; ++i) c = crc32m_byte(c, psrc[i]);
                if (plen > 0) x ^= crc32m_mulmod(c, crc32m_xpow((uint32_t)(total - ppos - plen)));
                if (idx <= base + 64) break;
            }
            for (int k = 32; k > 0; k >>= 1) x ^= __shfl_xor(x, k);
            if (lane == 0) {
                unsigned long long h8 = 0;
                unsigned h9 = 0;
                t2_pieces(q, v, 9, [&](int pos, const uint8_t* src, int len) {
                    for (int i = 0; i < len; ++i) {
                        const int at = pos + i;
                        if (at < 8) h8 |= (unsigned long long)src[i] << (8 * at); else h9 = src[i];
                    }
                });
                auto rd = [&](int i) { return i < 8 ? (unsigned)(h8 >> (8 * i) & 255) : h9; };
                rows[r] = t2mi_row_fields(rd, total, x == 0, q.j0 < 0 ? -1 : t2_k(wa[q.j0]), t2_k(wa[q.j1]));
            }
        }
        __syncthreads();
        // E: COUNT_ERROR from the last valid row before each, then the offsets of the delivered rows
        int r0, r1; ts_thread_run(nrows, T2_WG, &r0, &r1);
        {
            int lastv = -1;
            for (int r = r0; r < r1; ++r) if (!(rows[r].flags & T2MI_CRC_ERROR)) lastv = r;
            const int prev = ts_block_scan_max(lastv, wsum);
            int has = prev >= 0 ? 1 : ss.has_count, last = prev >= 0 ? rows[prev].packet_count : ss.last_count;
            int c_crc = 0, c_cnt = 0, c_bb = 0, c_bad = 0;
            for (int r = r0; r < r1; ++r) {
                const T2miRow row = rows[r];
                if (row.flags & T2MI_CRC_ERROR) { ++c_crc; continue; }
                if (has && row.packet_count != ((last + 1) & 255)) { rows[r].flags = row.flags | T2MI_COUNT_ERROR; ++c_cnt; }
                has = 1; last = row.packet_count;
                c_bb += (row.flags & T2MI_BBFRAME) != 0; c_bad += (row.flags & T2MI_BAD_PAYLOAD) != 0;
            }
            if (c_crc) atomicAdd(&cnt[T2C_CRC], c_crc);
            if (c_cnt) atomicAdd(&cnt[T2C_COUNT], c_cnt);
            if (c_bb) atomicAdd(&cnt[T2C_BB], c_bb);
            if (c_bad) atomicAdd(&cnt[T2C_BADPAY], c_bad);
            if (lastv >= 0) atomicMax(&last_valid, lastv);
        }
        {
            auto bytes_of = [&](int r) { return have_out && t2mi_delivers(rows[r], w.plp) ? rows[r].bbframe_bytes : 0; };
            int mine = 0, mine_n = 0;
            for (int r = r0; r < r1; ++r) { const int b = bytes_of(r); mine += b; mine_n += b > 0; }
            int at = ts_block_scan<T2_WG>(mine, wsum, &needed);
            int idx = ts_block_scan<T2_WG>(mine_n, wsum, &ndelivered);
            int* fb = fb_g + (size_t)g * max_rows;
            for (int r = r0; r < r1; ++r) {
                const int b = bytes_of(r);
                rows[r].offset = b ? at : -1;
                if (b) fb[idx++] = b;
                at += b;
            }
        }
        __syncthreads();
        if (tid == 0) {
            cnt[T2C_T2MI] = nrows; cnt[T2C_DELIVERED] = ndelivered; cnt[T2C_BYTES] = needed;
            if (last_valid >= 0) { nss.has_count = 1; nss.last_count = rows[last_valid].packet_count; }
        }
    }
    for (int j = tid; j < W; j += T2_WG) { wa_g[(size_t)g * max_packets + j] = wa[j]; wb_g[(size_t)g * max_packets + j] = wb[j]; }
    __syncthreads();
    if (tid == 0) {
        newst[g] = nss;
        T2Call c;
        c.needed = needed; c.nrows = nrows; c.watched = W; c.ndelivered = ndelivered;
        int32_t* dst = reinterpret_cast<int32_t*>(&c.cnt);
        for (int k = 0; k < T2MI_NCNT; ++k) dst[k] = cnt[k];
        call[g] = c;
    }
}

// n bytes from s to d, all 64 lanes of a wave: a dword per lane behind d's unaligned head
__device__ inline void t2_copy(uint8_t* d, const uint8_t* s, int n, int lane) {
    int head = (int)((4 - (reinterpret_cast<uintptr_t>(d) & 3)) & 3);
    if (head > n) head = n;
    const int nd = (n - head) / 4;
    if (lane < head) d[lane] = s[lane];
    for (int i = lane; i < nd; i += 64) *reinterpret_cast<unsigned*>(d + head + 4 * i) = *reinterpret_cast<const ts_unaligned_u32*>(s + head + 4 * i);
    const int tail = head + 4 * nd;
    if (lane < n - tail) d[tail + lane] = s[tail + lane];
}

__global__ void __launch_bounds__(T2_WG) t2mi_commit_kernel(const uint8_t* const* __restrict__ in, uint8_t* const* __restrict__ out, int max_packets, int max_rows,
                                                            int cap, T2DevSlot* __restrict__ state, const T2DevSlot* __restrict__ newst,
                                                            uint8_t* __restrict__ bufs, const unsigned* __restrict__ wa_g, const uint16_t* __restrict__ wb_g,
                                                            const T2Rec* __restrict__ recs, const T2Rec* __restrict__ opens, const T2miRow* __restrict__ rows_g,
                                                            const T2Call* __restrict__ call) {
    const int g = blockIdx.x, s = g / T2MI_SLOTS, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int W = call[g].watched, nrows = call[g].nrows;
    if (W > max_packets) W = max_packets;
    if (nrows > max_rows) nrows = max_rows;
    const T2Rec q = opens[g];
    if (nrows == 0 && q.j0 == -2 && W == 0) return;  // (an empty slot, or an empty call with nothing open: the state is what it was)
    uint8_t* sbuf = bufs + (size_t)g * T2MI_BUF;
    const T2View v = {in[s], wa_g + (size_t)g * max_packets, wb_g + (size_t)g * max_packets, W, sbuf, state[g].fill};
    const T2Rec* rec = recs + (size_t)g * max_rows;
    const T2miRow* rows = rows_g + (size_t)g * max_rows;
    uint8_t* o = out ? out[g] : nullptr;
    const int skip = T2MI.header_bytes + T2MI.bbframe_prefix_bytes;
    for (int r = wave; o && r < nrows; r += T2_WAVES) {
        const int off = rows[r].offset, bb = rows[r].bbframe_bytes;
        if (off < 0 || bb <= 0 || off + bb > cap) continue;
        t2_pieces(rec[r], v, skip + bb, [&](int pos, const uint8_t* src, int len) {
            const int a = pos > skip ? pos : skip, b = pos + len;
            if (b > a) t2_copy(o + off + (a - skip), src + (a - pos), b - a, lane);
        });
    }
    __syncthreads();                                 // the carried rows have read the buffer
    if (wave == 0 && q.j0 > -2)                      // the open packet: what the buffer holds already (a packet carried in and on) stays where it is
        t2_pieces(q, v, T2MI_BUF, [&](int pos, const uint8_t* src, int len) {
            if (src != sbuf) for (int i = lane; i < len; i += 64) sbuf[pos + i] = src[i];
        });
    if (tid == 0) state[g] = newst[g];
}

}  // namespace s2

struct dvbs2gpu_t2mi {
    dvbs2gpu_ctx* ctx = nullptr;                   // null: a host-only bank (dvbs2gpu_t2mi_create_host)
    int nstreams = 0, max_packets = 0, max_rows = 0;
    std::vector<T2miWatch> watch;                  // nstreams x 4
    std::vector<dvbs2gpu_t2mi_stats> stats;        // nstreams x 4, since reset; the kernels report each call's share (T2Call)
    std::vector<int> nrows, need_bytes, need_rows, ndelivered;   // of the last call per (stream, slot)
    std::vector<T2Call> h_call;
    std::vector<char> h_args;
    // device banks
    DevBuf<T2miWatch> d_watch;
    DevBuf<T2DevSlot> d_state, d_newst;
    DevBuf<uint8_t> d_bufs;                        // nstreams x 4 x 8208
    DevBuf<unsigned> d_wa;                         // nstreams x 4 x max_packets: the slots' packets of the last call
    DevBuf<uint16_t> d_wb;
    DevBuf<T2Rec> d_recs, d_opens;
    DevBuf<T2miRow> d_rows;                        // nstreams x 4 x max_rows
    DevBuf<int> d_fb;                              // the sizes of the delivered BBFRAMEs, nstreams x 4 x max_rows
    DevBuf<T2Call> d_call;
    DevBuf<uint8_t> d_args;                        // input pointers | output pointers (4 per stream) | byte counts
    Workspace stage_in, stage_out;                 // of the host-buffer entry point
    // host-only banks
    std::vector<T2miHostStream> host;              // nstreams x 4
};

namespace s2 {
// the argument table of a call: n input pointers | 4 n output pointers | n byte counts
struct T2Args {
    ScratchLayout L;
    ScratchPart<const uint8_t*> in; ScratchPart<uint8_t*> out; ScratchPart<int> nbytes;
    explicit T2Args(size_t n) : in(L.add<const uint8_t*>(n)), out(L.add<uint8_t*>(n * T2MI_SLOTS)), nbytes(L.add<int>(n)) {}
};
static void t2_account(dvbs2gpu_t2mi* b, int g, const T2miCnt& c) {
    int64_t* d = reinterpret_cast<int64_t*>(&b->stats[g]);
    const int32_t* a = reinterpret_cast<const int32_t*>(&c);
    for (int k = 0; k < T2MI_NCNT; ++k) d[k] += a[k];
}
static bool t2_create_args_ok(int nstreams, int max_packets, int max_rows, dvbs2gpu_t2mi** out) {
    if (!out || nstreams <= 0 || max_packets <= 0 || max_rows <= 0) return false;
    if (max_packets > T2_MAX_PACKETS) { g_err = "T2-MI bank: max_packets is at most 4096 per stream and call"; return false; }
    return true;
}
static std::unique_ptr<dvbs2gpu_t2mi> t2_new(dvbs2gpu_ctx* ctx, int nstreams, int max_packets, int max_rows) {
    std::unique_ptr<dvbs2gpu_t2mi> b(new dvbs2gpu_t2mi());
    const size_t ns = (size_t)nstreams * T2MI_SLOTS;
    b->ctx = ctx; b->nstreams = nstreams; b->max_packets = max_packets; b->max_rows = max_rows;
    b->watch.assign(ns, T2miWatch{-1, -1});
    b->stats.assign(ns, dvbs2gpu_t2mi_stats{});
    b->nrows.assign(ns, 0); b->need_bytes.assign(ns, 0); b->need_rows.assign(ns, 0); b->ndelivered.assign(ns, 0);
    b->h_call.resize(ns);
    return b;
}
static bool t2_slot_ok(const dvbs2gpu_t2mi* b, int stream, int slot) { return b && stream >= 0 && stream < b->nstreams && slot >= 0 && slot < T2MI_SLOTS; }

// the device call: d_out 4 pointers per stream or null; only: the one (stream, slot) index that is served, -1: all
static int t2_batch(dvbs2gpu_t2mi* b, const uint8_t* const* d_ts, const int* nbytes, uint8_t* const* d_out, int cap, int* out_bytes, int* out_rows, int only,
                    hipStream_t st) {
    const int n = b->nstreams, ns = n * T2MI_SLOTS;
    HIP_TRY(hipSetDevice(b->ctx->device));
    const T2Args a(n);
    {
        const uint8_t** pi = a.in(b->h_args.data()); uint8_t** po = a.out(b->h_args.data()); int* pn = a.nbytes(b->h_args.data());
        for (int i = 0; i < n; ++i) { pi[i] = d_ts[i]; pn[i] = nbytes[i]; }
        for (int g = 0; g < ns; ++g) po[g] = d_out ? d_out[g] : nullptr;
    }
    HIP_TRY(hipMemcpyAsync(b->d_args, b->h_args.data(), b->h_args.size(), hipMemcpyHostToDevice, st));
    const size_t lds = (size_t)b->max_packets * 10 + 16;               // <= 40 KiB
    hipLaunchKernelGGL(t2mi_scan_kernel, dim3(ns), dim3(T2_WG), lds, st, a.in(b->d_args), a.nbytes(b->d_args), b->max_packets, b->max_rows, only, b->d_watch, b->d_state,
                       b->d_newst, b->d_bufs, b->d_wa, b->d_wb, b->d_recs, b->d_opens, b->d_rows, b->d_fb, b->d_call, d_out ? 1 : 0);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(b->h_call.data(), b->d_call, sizeof(T2Call) * ns, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    bool fits = true;
    for (int g = 0; g < ns; ++g) {
        const T2Call& c = b->h_call[g];
        fits &= c.nrows <= b->max_rows && (!d_out || c.needed <= cap);
        b->need_bytes[g] = c.needed; b->need_rows[g] = c.nrows;
        if (out_bytes) out_bytes[g] = c.needed;
        if (out_rows) out_rows[g] = c.nrows;
    }
    if (!fits) {                                       // nothing has been stored: the same call may come again with more room
        std::fill(b->nrows.begin(), b->nrows.end(), 0);
        std::fill(b->ndelivered.begin(), b->ndelivered.end(), 0);
        g_err = "T2-MI bank: the BBFRAMEs of a slot do not fit cap, or its rows max_rows (out_bytes / out_rows hold the sizes)";
        return DVBS2GPU_ERR_CAPACITY;
    }
    hipLaunchKernelGGL(t2mi_commit_kernel, dim3(ns), dim3(T2_WG), 0, st, a.in(b->d_args), d_out ? a.out(b->d_args) : nullptr, b->max_packets, b->max_rows, cap, b->d_state,
                       b->d_newst, b->d_bufs, b->d_wa, b->d_wb, b->d_recs, b->d_opens, b->d_rows, b->d_call);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(st));
    for (int g = 0; g < ns; ++g) { t2_account(b, g, b->h_call[g].cnt); b->nrows[g] = b->h_call[g].nrows; b->ndelivered[g] = b->h_call[g].ndelivered; }
    return 0;
}
}  // namespace s2

extern "C" {

void dvbs2gpu_t2mi_destroy(dvbs2gpu_t2mi* b) { delete b; }

int dvbs2gpu_t2mi_create(dvbs2gpu_ctx* ctx, int nstreams, int max_packets, int max_rows, dvbs2gpu_t2mi** out) {
    if (!ctx || !t2_create_args_ok(nstreams, max_packets, max_rows, out)) return DVBS2GPU_ERR_ARG;
    HIP_TRY(hipSetDevice(ctx->device));
    auto b = t2_new(ctx, nstreams, max_packets, max_rows);
    const size_t n = (size_t)nstreams, ns = n * T2MI_SLOTS;
    const char* what = "hipMalloc(t2mi)";              // (zero-filled: the slots' states; the kernels write the rest before it is read)
    RC_TRY(b->d_watch.alloc(ns, false, what));
    HIP_TRY(hipMemcpy(b->d_watch, b->watch.data(), ns * sizeof(T2miWatch), hipMemcpyHostToDevice));
    RC_TRY(b->d_state.alloc(ns, true, what));
    RC_TRY(b->d_newst.alloc(ns, false, what));
    RC_TRY(b->d_bufs.alloc(ns * T2MI_BUF, false, what));
    RC_TRY(b->d_wa.alloc(ns * max_packets, false, what));
    RC_TRY(b->d_wb.alloc(ns * max_packets, false, what));
    RC_TRY(b->d_recs.alloc(ns * max_rows, false, what));
    RC_TRY(b->d_opens.alloc(ns, false, what));
    RC_TRY(b->d_rows.alloc(ns * max_rows, false, what));
    RC_TRY(b->d_fb.alloc(ns * max_rows, false, what));
    RC_TRY(b->d_call.alloc(ns, false, what));
    RC_TRY(b->d_args.alloc(T2Args(n).L.bytes(), false, what));
    b->h_args.resize(T2Args(n).L.bytes());
    *out = b.release();
    return 0;
}

int dvbs2gpu_t2mi_create_host(int nstreams, int max_packets, int max_rows, dvbs2gpu_t2mi** out) {
    if (!t2_create_args_ok(nstreams, max_packets, max_rows, out)) return DVBS2GPU_ERR_ARG;
    auto b = t2_new(nullptr, nstreams, max_packets, max_rows);
    b->host.resize((size_t)nstreams * T2MI_SLOTS);
    *out = b.release();
    return 0;
}

int dvbs2gpu_t2mi_reset(dvbs2gpu_t2mi* b) {
    if (!b) return DVBS2GPU_ERR_ARG;
    if (b->ctx) {
        HIP_TRY(hipSetDevice(b->ctx->device));
        HIP_TRY(hipMemset(b->d_state, 0, (size_t)b->nstreams * T2MI_SLOTS * sizeof(T2DevSlot)));
    }
    for (auto& h : b->host) h.clear();
    std::fill(b->stats.begin(), b->stats.end(), dvbs2gpu_t2mi_stats{});
    std::fill(b->nrows.begin(), b->nrows.end(), 0);
    std::fill(b->ndelivered.begin(), b->ndelivered.end(), 0);
    return 0;
}

int dvbs2gpu_t2mi_get_layout(dvbs2gpu_t2mi_layout* h_out) {
    if (!h_out) return DVBS2GPU_ERR_ARG;
    memcpy(h_out, &T2MI, sizeof(T2MI));
    return 0;
}

int dvbs2gpu_t2mi_set_watch(dvbs2gpu_t2mi* b, int stream, int slot, int pid, int plp) {
    if (!t2_slot_ok(b, stream, slot)) return DVBS2GPU_ERR_ARG;
    if (pid < -1 || pid >= TSMON_NULL_PID || plp < -1 || plp > 255) {
        g_err = "T2-MI bank: a slot's PID is 0..0x1FFE (-1 empties the slot), its PLP 0..255 or -1 for every PLP";
        return DVBS2GPU_ERR_ARG;
    }
    const size_t at = (size_t)stream * T2MI_SLOTS + slot;
    b->watch[at] = {pid, pid < 0 ? -1 : plp};
    b->stats[at] = dvbs2gpu_t2mi_stats{};
    b->nrows[at] = 0; b->ndelivered[at] = 0;
    if (b->ctx) {
        HIP_TRY(hipSetDevice(b->ctx->device));
        HIP_TRY(hipMemcpy(b->d_watch + at, &b->watch[at], sizeof(T2miWatch), hipMemcpyHostToDevice));
        HIP_TRY(hipMemset(b->d_state + at, 0, sizeof(T2DevSlot)));
    } else {
        b->host[at].clear();
        b->host[at].watch = b->watch[at];
    }
    return 0;
}

int dvbs2gpu_t2mi_process_batch(dvbs2gpu_t2mi* b, const uint8_t* const* d_ts, const int* nbytes, uint8_t* const* d_out, int cap, int* out_bytes, int* out_rows,
                                void* stream) {
    if (!b || !d_ts || !nbytes || cap < 0 || (d_out && !out_bytes)) return DVBS2GPU_ERR_ARG;
    if (!b->ctx) { g_err = "T2-MI bank: a host bank takes host buffers (dvbs2gpu_t2mi_work)"; return DVBS2GPU_ERR_ARG; }
    for (int i = 0; i < b->nstreams; ++i) {
        if (!ts_bank_check_counts("T2-MI bank: ", nbytes + i, 1, b->max_packets)) return DVBS2GPU_ERR_ARG;
        bool bad = nbytes[i] > 0 && !d_ts[i];
        // once d_out is given every watching slot needs its output pointer, one of an empty stream too
        for (int k = 0; d_out && k < T2MI_SLOTS; ++k) {
            uint8_t* o = d_out[i * T2MI_SLOTS + k];
            bad |= (b->watch[(size_t)i * T2MI_SLOTS + k].pid >= 0 && !o) || (o && o == d_ts[i]);
        }
        if (bad) { g_err = "T2-MI bank: null buffer, or an output buffer that is its stream's input"; return DVBS2GPU_ERR_ARG; }
    }
    return t2_batch(b, d_ts, nbytes, d_out, cap, out_bytes, out_rows, -1, (hipStream_t)stream);
}

int dvbs2gpu_t2mi_work(dvbs2gpu_t2mi* b, int stream, int slot, const uint8_t* h_ts, int nbytes, uint8_t* h_out, int cap) {
    if (!t2_slot_ok(b, stream, slot) || nbytes < 0 || cap < 0 || (nbytes > 0 && !h_ts)) return DVBS2GPU_ERR_ARG;
    if (!ts_bank_check_counts("T2-MI bank: ", &nbytes, 1, b->max_packets)) return DVBS2GPU_ERR_ARG;
    if (h_out && h_out == h_ts) { g_err = "T2-MI bank: the output buffer is the input"; return DVBS2GPU_ERR_ARG; }
    const int g = stream * T2MI_SLOTS + slot;
    if (!b->ctx) {
        T2miHostStream& h = b->host[g];
        // The tables are of the LAST call, which brought the others nothing.  An empty call changes no state (run() with no packet
        // is the identity), so the other slots are not run: their tables are emptied by count alone.  host[].rows and .bytes of those
        // slots keep what their own last call left; every getter reads them through nrows / ndelivered, which are 0.
        std::fill(b->nrows.begin(), b->nrows.end(), 0);
        std::fill(b->ndelivered.begin(), b->ndelivered.end(), 0);
        const std::unique_ptr<T2miState> before(new T2miState(h.st));  // what a capacity failure has to put back
        h.run(h_ts, nbytes / TSMON_TS, h_out != nullptr);
        const bool rows_fit = (int)h.rows.size() <= b->max_rows;
        b->need_rows[g] = (int)h.rows.size();
        b->need_bytes[g] = rows_fit ? (int)h.bytes.size() : -1;
        if (!rows_fit || (h_out && (int)h.bytes.size() > cap)) {
            h.st = *before;
            h.rows.clear(); h.bytes.clear();
            g_err = "T2-MI bank: the BBFRAMEs do not fit cap, or the rows max_rows (dvbs2gpu_t2mi_get_needed holds the sizes)";
            return DVBS2GPU_ERR_CAPACITY;
        }
        t2_account(b, g, h.cnt);
        b->nrows[g] = (int)h.rows.size();
        b->ndelivered[g] = h.cnt.bbframes_delivered;
        if (h_out && !h.bytes.empty()) memcpy(h_out, h.bytes.data(), h.bytes.size());
        return (int)h.bytes.size();
    }
    HIP_TRY(hipSetDevice(b->ctx->device));
    if (const int e = b->stage_in.ensure((size_t)b->max_packets * TSMON_TS)) return e;
    if (nbytes > 0) HIP_TRY(hipMemcpy(b->stage_in.p, h_ts, nbytes, hipMemcpyHostToDevice));
    if (const int e = h_out ? b->stage_out.ensure((size_t)cap + 4) : 0) return e;
    const size_t ns = (size_t)b->nstreams * T2MI_SLOTS;
    std::vector<const uint8_t*> in(b->nstreams, nullptr);
    std::vector<uint8_t*> out(ns, nullptr);
    std::vector<int> nb(b->nstreams, 0), ob(ns, 0);
    in[stream] = static_cast<const uint8_t*>(b->stage_in.p); out[g] = static_cast<uint8_t*>(b->stage_out.p); nb[stream] = nbytes;
    const int rc = t2_batch(b, in.data(), nb.data(), h_out ? out.data() : nullptr, cap, ob.data(), nullptr, g, nullptr);
    if (rc < 0) return rc;
    if (h_out && ob[g] > 0) HIP_TRY(hipMemcpy(h_out, b->stage_out.p, ob[g], hipMemcpyDeviceToHost));
    return ob[g];
}

/* the byte and row sizes the slot's last call needed, whether it succeeded or failed for capacity (bytes -1: the rows did not fit) */
int dvbs2gpu_t2mi_get_needed(dvbs2gpu_t2mi* b, int stream, int slot, int* bytes, int* rows) {
    if (!t2_slot_ok(b, stream, slot) || !bytes || !rows) return DVBS2GPU_ERR_ARG;
    *bytes = b->need_bytes[stream * T2MI_SLOTS + slot]; *rows = b->need_rows[stream * T2MI_SLOTS + slot];
    return 0;
}

int dvbs2gpu_t2mi_get_stats(dvbs2gpu_t2mi* b, int stream, int slot, dvbs2gpu_t2mi_stats* h_out) {
    if (!b || stream < 0 || stream >= b->nstreams || slot < -1 || slot >= T2MI_SLOTS || !h_out) return DVBS2GPU_ERR_ARG;
    *h_out = dvbs2gpu_t2mi_stats{};
    int64_t* d = reinterpret_cast<int64_t*>(h_out);
    for (int s = slot < 0 ? 0 : slot; s < (slot < 0 ? T2MI_SLOTS : slot + 1); ++s) {
        const int64_t* a = reinterpret_cast<const int64_t*>(&b->stats[(size_t)stream * T2MI_SLOTS + s]);
        for (int k = 0; k < T2MI_NCNT; ++k) d[k] += a[k];
    }
    return 0;
}

int dvbs2gpu_t2mi_get_row_table(dvbs2gpu_t2mi* b, int stream, int slot, dvbs2gpu_t2mi_row* h_rows, int cap, int* n) {
    if (!t2_slot_ok(b, stream, slot) || !n || cap < 0 || (cap > 0 && !h_rows)) return DVBS2GPU_ERR_ARG;
    const int g = stream * T2MI_SLOTS + slot;
    const int k = (*n = b->nrows[g]) < cap ? *n : cap;
    if (k <= 0) return 0;
    if (!b->ctx) { memcpy(h_rows, b->host[g].rows.data(), k * sizeof(T2miRow)); return 0; }
    HIP_TRY(hipSetDevice(b->ctx->device));
    HIP_TRY(hipMemcpy(h_rows, b->d_rows + (size_t)g * b->max_rows, k * sizeof(T2miRow), hipMemcpyDeviceToHost));
    return 0;
}

int dvbs2gpu_t2mi_get_row_table_device(dvbs2gpu_t2mi* b, int stream, int slot, const dvbs2gpu_t2mi_row** d_rows, int* n) {
    if (!t2_slot_ok(b, stream, slot) || !b->ctx || !n || !d_rows) return DVBS2GPU_ERR_ARG;
    const int g = stream * T2MI_SLOTS + slot;
    *n = b->nrows[g]; *d_rows = *n ? reinterpret_cast<const dvbs2gpu_t2mi_row*>(b->d_rows + (size_t)g * b->max_rows) : nullptr;
    return 0;
}

int dvbs2gpu_t2mi_get_frame_bytes(dvbs2gpu_t2mi* b, int stream, int slot, int* h_sizes, int cap, int* n) {
    if (!t2_slot_ok(b, stream, slot) || !n || cap < 0 || (cap > 0 && !h_sizes)) return DVBS2GPU_ERR_ARG;
    const int g = stream * T2MI_SLOTS + slot;
    const int k = (*n = b->ndelivered[g]) < cap ? *n : cap;
    if (k <= 0) return 0;
    if (!b->ctx) {
        int i = 0;
        for (const T2miRow& r : b->host[g].rows)
            if (r.offset >= 0 && i < k) h_sizes[i++] = r.bbframe_bytes;
        return 0;
    }
    HIP_TRY(hipSetDevice(b->ctx->device));
    HIP_TRY(hipMemcpy(h_sizes, b->d_fb + (size_t)g * b->max_rows, k * sizeof(int), hipMemcpyDeviceToHost));
    return 0;
}

}  // extern "C"
