// The device side of the banks that reassemble length-prefixed units from the payloads of a PID (psi.hip: PSI sections; dgram_bank.h:
// the datagram banks -- T2-MI packets, MPE sections, ULE SNDUs; rules and sequential definition in ts_reasm_rules.h; DESIGN section
// 9), stated once.
//
// What makes the parallel form possible: a unit STARTS only behind the pointer field of a PUSI packet, so the chain of unit headers of
// a TS packet starts at its own pointer and never leaves the packet; only the LAST unit begun in a PUSI packet can reach into the
// slot's later packets, and it ends at the latest in the pointer bytes of the slot's next PUSI packet.  Hence, in a bank's scan kernel:
//   A  reasm_collect     the packets that a matcher gives a slot, compacted in input order into LDS (wa / wb below);
//   B  reasm_classify    one lane per slot takes the continuity steps in order and classes each packet (ts_packet_class);
//   C  reasm_jobs        one lane per PUSI packet hops from header to header inside its packet (reasm_pusi_job) and follows the unit
//                        that the packet's end cuts -- a split header too -- through the slot's next packets until it is complete,
//                        dropped or the call ends (reasm_resolve); one lane per slot does the same for the unit carried in.  A first
//                        pass (WRITE false) counts the rows that every packet ends, reasm_number_rows numbers them in input order --
//                        the row order of the rules -- and the second pass writes one ReasmRec per row, the open unit's and the counters;
//   D, E and the commit kernel are the bank's own; they read a unit's bytes where they lie through reasm_pieces.
//
// A format is a traits type F:
//   WG, SLOTS       threads per workgroup; slots that a workgroup serves (1: the slot compares compile out of every loop)
//   State, BUF      a slot's state with members `fill` (bytes of the unit carried in) and `cont`; bytes of a slot's buffer
//   HEADER, LEN_A, LEN_B, total(bA, bB)
//                   the header's bytes, the indices of the two that carry the length, the unit's bytes from them (< 0: a bad length,
//                   which ends the packet's chain)
//   STUFFING        the byte in a unit's first place that ends a packet's chain, -1: none
//   is_row(bA, total)   is a finished unit a row; one that is not is counted in C_BAD_UNIT, as a bad length is
//   NCNT, C_DROPPED, C_BAD_UNIT, C_SLACK   the counters of a slot and the indices of these three (-1: the format has no such counter)
#pragma once
#include "ts_bank.h"
#include "ts_reasm_rules.h"

namespace s2 {

// a unit of the call: its first byte at offset `at` of the slot's packet j0 (j0 -1: carried in, the slot's buffer comes first), its last
// byte in packet j1 (indices into wa).  As the open unit of a slot: j0 -2 none, total the bytes so far
struct ReasmRec { int32_t j0, j1; uint16_t at, slot; int32_t total; };
static_assert(sizeof(ReasmRec) == 16, "record layout");

// a slot's packet in LDS.  wa: index k bits 0-12, slot 13-16, class 17-19 (after reasm_classify); before it CC 20-23, AFC 24-25,
// DI 26, PUSI 27, scrambled 28.  wb: payload start (188: none) | pointer byte << 8
__device__ inline int wa_k(unsigned e) { return (int)(e & 0x1fff); }
template <typename F> __device__ inline int wa_slot(unsigned e) { return F::SLOTS > 1 ? (int)(e >> 13 & 15) : 0; }
__device__ inline int wa_kind(unsigned e) { return (int)(e >> 17 & 7); }
// the bytes that a CONT or PUSI packet has for the open unit, from offset *lo of the packet on: of a PUSI packet its pointer bytes
__device__ inline int wa_avail(unsigned e, unsigned b, int* lo) {
    const int ps = b & 255, pusi = wa_kind(e) == PK_PUSI;
    *lo = ps + pusi;
    return pusi ? (int)(b >> 8) : TSMON_TS - ps;
}

template <typename F> struct ReasmView {         // what the walkers read of one workgroup's slots
    const uint8_t* ts; const unsigned* wa; const uint16_t* wb; int W;
    const uint8_t* sbuf;                         // the slots' buffers, F::BUF bytes each
    const typename F::State* ss;                 // the slots' states before the call
};
template <typename F> struct ReasmOut { int* rc; ReasmRec* rec; ReasmRec* open; typename F::State* nss; int (*cnt)[F::NCNT]; int max_rows; };
// one more in counter C of the slot (C -1: the format has no such counter)
template <int C, typename F> __device__ inline void reasm_count(const ReasmOut<F>& o, int slot) { if constexpr (C >= 0) atomicAdd(&o.cnt[slot][C], 1); }

// phase A: the packets for which match(header) gives a slot (-1: none) into wa / wb, in input order; returns their number
template <int WG, typename M>
__device__ int reasm_collect(const uint8_t* __restrict__ ts, int n, M match, unsigned* wa, uint16_t* wb, int* wsum) {
    int k0, k1; ts_thread_run(n, WG, &k0, &k1);
    unsigned mask = 0;
    for (int k = k0; k < k1; ++k) mask |= (unsigned)(match(ts_load_header(ts, k)) >= 0) << (k - k0);
    int W;
    int at = ts_block_scan<WG>(__popc(mask), wsum, &W);
    for (int k = k0; k < k1; ++k) {
        if (!(mask >> (k - k0) & 1)) continue;
        unsigned b4;
        const TsmonHdr h = ts_load_header(ts, k, &b4);
        int ps = ts_payload_start(h.afc, b4);
        if (ps > TSMON_TS) ps = TSMON_TS;
        const unsigned ptr = (h.pusi && (h.afc & 1) && ps < TSMON_TS) ? ts[(size_t)k * TSMON_TS + ps] : 0;
        wa[at] = (unsigned)k | (unsigned)match(h) << 13 | (unsigned)h.cc << 20 | (unsigned)h.afc << 24 | (unsigned)h.di << 26 |
                 (unsigned)h.pusi << 27 | (unsigned)(h.tsc != 0) << 28;
        wb[at] = (uint16_t)(ps | ptr << 8);
        ++at;
    }
    __syncthreads();
    return W;
}

// phase B: the continuity walk of `slot` from its state byte, one lane; every packet of the slot gets its class
struct ReasmWalk { int packets, scrambled, malformed; };
template <typename F>
__device__ inline ReasmWalk reasm_classify(unsigned* wa, const uint16_t* wb, int W, int slot, uint8_t* cont) {
    ReasmWalk c = {0, 0, 0};
    for (int j = 0; j < W; ++j) {
        const unsigned e = wa[j];
        if (F::SLOTS > 1 && wa_slot<F>(e) != slot) continue;
        const int v = tsmon_step(cont, e >> 24 & 3, e >> 20 & 15, e >> 26 & 1);
        const TsPacketClass pc = ts_packet_class(v, e >> 28 & 1, e >> 24 & 3, wb[j] & 255, e >> 27 & 1, wb[j] >> 8);
        ++c.packets; c.scrambled += pc.scrambled; c.malformed += pc.malformed;
        wa[j] = (e & 0x1ffffu) | (unsigned)pc.kind << 17;   // (the other slots' lanes read this word for its slot bits only, which stay)
    }
    return c;
}

// the pieces of unit r that hold its bytes [0, limit), in order: f(position in the unit, source, bytes)
template <typename F, typename Fn>
__device__ inline void reasm_pieces(const ReasmRec& r, const ReasmView<F>& v, int limit, Fn f) {
    const int total = r.total < limit ? r.total : limit, slot = F::SLOTS > 1 ? r.slot : 0;
    int pos, jn = 0;
    if (r.j0 < 0) {
        pos = v.ss[slot].fill < total ? v.ss[slot].fill : total;
        f(0, v.sbuf + (size_t)slot * F::BUF, pos);
    } else {
        pos = TSMON_TS - r.at < total ? TSMON_TS - r.at : total;
        f(0, v.ts + (size_t)wa_k(v.wa[r.j0]) * TSMON_TS + r.at, pos);
        jn = r.j0 + 1;
    }
    for (int j = jn; pos < total && j < v.W; ++j) {
        const unsigned e = v.wa[j];
        if ((F::SLOTS > 1 && wa_slot<F>(e) != slot) || wa_kind(e) == PK_SKIP) continue;
        if (wa_kind(e) != PK_CONT && wa_kind(e) != PK_PUSI) break;
        int lo;
        const int avail = wa_avail(e, v.wb[j], &lo), len = avail < total - pos ? avail : total - pos;
        f(pos, v.ts + (size_t)wa_k(e) * TSMON_TS + lo, len);
        pos += len;
    }
}

// The open unit of `slot` -- `fill` bytes so far, length bytes bA, bB where fill reaches them, first byte at (j0, at) -- through the
// slot's packets from jn on.  One lane.
template <bool WRITE, typename F>
__device__ void reasm_resolve(const ReasmView<F>& v, const ReasmOut<F>& o, int slot, int j0, int at, int fill, unsigned bA, unsigned bB, int jn) {
    enum { R_OPEN, R_DONE, R_DROPPED, R_BAD_LENGTH };
    int outcome = R_OPEN, endj = -1, total = 0;
    bool slack = false;
    for (int j = jn; j < v.W; ++j) {
        const unsigned e = v.wa[j];
        const int kind = wa_kind(e);
        if ((F::SLOTS > 1 && wa_slot<F>(e) != slot) || kind == PK_SKIP) continue;
        if (kind == PK_CUT || kind == PK_PUSI_BRK) { outcome = R_DROPPED; break; }
        int lo, used = 0;
        const int avail = wa_avail(e, v.wb[j], &lo);
        const uint8_t* p = v.ts + (size_t)wa_k(e) * TSMON_TS + lo;
        while (fill < F::HEADER && used < avail) {
            const unsigned byte = p[used++];
            if (fill == F::LEN_A) bA = byte; else if (fill == F::LEN_B) bB = byte;
            ++fill;
        }
        if (fill >= F::HEADER) {
            total = F::total(bA, bB);
            if (total < 0) { outcome = R_BAD_LENGTH; break; }
            const int take = avail - used < total - fill ? avail - used : total - fill;
            fill += take; used += take;
            if (fill == total) { outcome = R_DONE; endj = j; slack = kind == PK_PUSI && used < avail; break; }
        }
        if (kind == PK_PUSI) { outcome = R_DROPPED; break; }
    }
    if (outcome == R_DONE) {
        const bool row = F::is_row(bA, total);
        if (!WRITE) { if (row) atomicAdd(&o.rc[endj], 1); }
        else {
            const int r = o.rc[endj] >> 1;
            if (!row) reasm_count<F::C_BAD_UNIT>(o, slot);
            else if (r < o.max_rows) { const ReasmRec rec = {j0, endj, (uint16_t)at, (uint16_t)slot, total}; o.rec[r] = rec; }
            if (slack) reasm_count<F::C_SLACK>(o, slot);
        }
    } else if (WRITE) {
        if (outcome == R_DROPPED) reasm_count<F::C_DROPPED>(o, slot);
        else if (outcome == R_BAD_LENGTH) reasm_count<F::C_BAD_UNIT>(o, slot);
        else { const ReasmRec rec = {j0, v.W, (uint16_t)at, (uint16_t)slot, fill}; o.open[slot] = rec; o.nss[slot].fill = fill; }
    }
}

// packet j of wa, a PUSI packet: the units that start behind its pointer.  One lane.
template <bool WRITE, typename F>
__device__ void reasm_pusi_job(const ReasmView<F>& v, const ReasmOut<F>& o, int j) {
    const unsigned e = v.wa[j];
    const int slot = wa_slot<F>(e), ps = v.wb[j] & 255, ptr = v.wb[j] >> 8;
    const uint8_t* p = v.ts + (size_t)wa_k(e) * TSMON_TS;
    const int base = WRITE ? (o.rc[j] >> 1) + (o.rc[j] & 1) : 0;
    int at = ps + 1 + ptr, i = 0;
    while (at < TSMON_TS) {
        if (F::STUFFING >= 0 && p[at] == F::STUFFING) break;
        const int have = TSMON_TS - at;
        const unsigned bA = have > F::LEN_A ? p[at + F::LEN_A] : 0, bB = have > F::LEN_B ? p[at + F::LEN_B] : 0;
        if (have >= F::HEADER) {
            const int total = F::total(bA, bB);
            if (total < 0) { if (WRITE) reasm_count<F::C_BAD_UNIT>(o, slot); break; }
            if (total <= have) {
                if (!F::is_row(bA, total)) { if (WRITE) reasm_count<F::C_BAD_UNIT>(o, slot); }
                else {
                    if (WRITE && base + i < o.max_rows) { const ReasmRec rec = {j, j, (uint16_t)at, (uint16_t)slot, total}; o.rec[base + i] = rec; }
                    ++i;
                }
                at += total;
                continue;
            }
        }
        reasm_resolve<WRITE>(v, o, slot, j, at, have, bA, bB, j + 1);
        break;
    }
    if (!WRITE && i) atomicAdd(&o.rc[j], 2 * i);
}

// phase C, one pass: a lane per slot with a unit carried in (an empty slot's state is zero: it carries nothing) and per PUSI packet.
// Pass one leaves in rc[j] twice the units that start and end in packet j, plus one if a unit from before ends in it
template <bool WRITE, typename F>
__device__ void reasm_jobs(const ReasmView<F>& v, const ReasmOut<F>& o) {
    for (int t = threadIdx.x; t < v.W + F::SLOTS; t += F::WG) {
        if (t < F::SLOTS) {
            const int fill = v.ss[t].fill;
            const uint8_t* sb = v.sbuf + (size_t)t * F::BUF;
            if (fill > 0) reasm_resolve<WRITE>(v, o, t, -1, 0, fill, fill > F::LEN_A ? sb[F::LEN_A] : 0, fill > F::LEN_B ? sb[F::LEN_B] : 0, 0);
        } else if (wa_kind(v.wa[t - F::SLOTS]) >= PK_PUSI) reasm_pusi_job<WRITE>(v, o, t - F::SLOTS);
    }
}

// between the passes: rc[j] becomes (the first row that packet j ends) << 1 | (a unit from before ends in it, and takes that row);
// returns the number of rows.  Whole workgroup
template <int WG>
__device__ inline int reasm_number_rows(int* rc, int W, int* wsum) {
    int j0, j1; ts_thread_run(W, WG, &j0, &j1);
    int mine = 0, nrows;
    for (int j = j0; j < j1; ++j) mine += (rc[j] >> 1) + (rc[j] & 1);
    int run = ts_block_scan<WG>(mine, wsum, &nrows);
    for (int j = j0; j < j1; ++j) { const int c = rc[j]; rc[j] = run << 1 | (c & 1); run += (c >> 1) + (c & 1); }
    __syncthreads();
    return nrows;
}

// n bytes to d, all 64 lanes of a wave: a dword per lane behind d's unaligned head.  s.u8(i): source byte i; s.u32(i): bytes i .. i + 3
struct TsBytes {                                 // a source in memory
    const uint8_t* p;
    __device__ unsigned u8(int i) const { return p[i]; }
    __device__ unsigned u32(int i) const { return *reinterpret_cast<const ts_unaligned_u32*>(p + i); }
};
template <typename Src>
__device__ inline void ts_wave_copy(uint8_t* d, Src s, int n, int lane) {
    int head = (int)((4 - (reinterpret_cast<uintptr_t>(d) & 3)) & 3);
    if (head > n) head = n;
    const int nd = (n - head) / 4;
    if (lane < head) d[lane] = (uint8_t)s.u8(lane);
    for (int i = lane; i < nd; i += 64) *reinterpret_cast<unsigned*>(d + head + 4 * i) = s.u32(head + 4 * i);
    const int tail = head + 4 * nd;
    if (lane < n - tail) d[tail + lane] = (uint8_t)s.u8(tail + lane);
}

}  // namespace s2
