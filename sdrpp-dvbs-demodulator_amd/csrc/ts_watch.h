// Shared by the banks that follow up to 16 watched PIDs per stream packet by packet with one workgroup per stream (pes.hip: the PES
// packets; es.hip and aud.hip through es_stream.h: the elementary streams): the first three phases of their kernels,
// which turn a call's packets into one 32-bit word per trusted packet of a watched PID, sorted by slot, with the TS monitor's
// continuity verdict in it.
//     A  every packet's header is read once (ts_load_header, ts_bank.h) and its PID matched against the 16 watches.  The trusted
//        packets of watched PIDs are compacted in input order into LDS, one word each: flags in a mask, ts_block_scan, scatter.
//     B  the PCR bank's stable counting sort by slot; the words themselves are placed.
//     C  every thread takes a contiguous run of the sorted words.  The word before one in sorted order is its slot's previous packet,
//        or the word is its slot's first of the call and takes the carried continuity byte.  A packet is "eligible" when it could be
//        a duplicate (payload, no DI, the counter of the packet before it); an exclusive maximum scan over the threads
//        (ts_block_scan_max) gives every packet the last one before it that is not eligible, the distance to it is its place in the
//        run of equal counters and the parity of that place is dup_used.  With it tsmon_step's verdict follows per packet.
// What a bank does with a verdict beyond these counters is its own.  Device code only.
#pragma once
#include "ts_bank.h"
#include "pes_rules.h"

namespace s2 {

constexpr int PW_SLOTS = PES_SLOTS;
constexpr int PW_MAX_PACKETS = 4096;             // per stream and call: 12 bits of a word, 16 packets per thread of 256

// a packet in LDS: packet k bits 0-11, slot 12-15, continuity counter 16-19, payload bytes L 20-27 (0 with payload: malformed),
// payload 28, PUSI 29, scrambled 30, DI 31.  Behind phase C the counter's bits hold the verdict: DUPLICATE 16, a GAP mark 17 (CC_ERROR,
// DISC or malformed); bits 18 and 19 are the bank's
__device__ inline int pw_k(uint32_t e) { return (int)(e & 4095); }
__device__ inline int pw_slot(uint32_t e) { return (int)(e >> 12 & 15); }
__device__ inline int pw_cc(uint32_t e) { return (int)(e >> 16 & 15); }
__device__ inline int pw_len(uint32_t e) { return (int)(e >> 20 & 255); }
__device__ inline int pw_pay(uint32_t e) { return (int)(e >> 28 & 1); }
__device__ inline int pw_pusi(uint32_t e) { return (int)(e >> 29 & 1); }
__device__ inline int pw_scr(uint32_t e) { return (int)(e >> 30 & 1); }
__device__ inline int pw_di(uint32_t e) { return (int)(e >> 31); }
constexpr uint32_t PW_VERDICT = 15u << 16, PW_DUP = 1u << 16, PW_GAP = 1u << 17;
// behind phase C: an accepted packet with payload bytes; a start
__device__ inline bool pw_counts(uint32_t e) { return !(e & PW_DUP) && pw_len(e) > 0; }
__device__ inline bool pw_start(uint32_t e) { return pw_counts(e) && pw_pusi(e); }
// a word with its verdict in the counter's place
__device__ inline uint32_t pw_with_verdict(uint32_t e, bool dup, bool gap) { return (e & ~PW_VERDICT) | (dup ? PW_DUP : 0) | (gap ? PW_GAP : 0); }

// packet k of the stream: false, or a trusted packet of a watched PID as its word
__device__ inline bool pw_look(const uint8_t* __restrict__ ts, int k, const int32_t* w, uint32_t* word) {
    unsigned b4;
    const TsmonHdr h = ts_load_header(ts, k, &b4);
    if (h.cls != TSMON_DATA) return false;
    int slot = -1;
    for (int s = 0; s < PW_SLOTS; ++s) if (w[s] == h.pid) slot = s;
    if (slot < 0) return false;
    const int L = pes_payload_len(h.afc, b4);
    *word = (uint32_t)k | (uint32_t)slot << 12 | (uint32_t)h.cc << 16 | (uint32_t)(L > 0 ? L : 0) << 20 | (uint32_t)(L >= 0) << 28 | (uint32_t)h.pusi << 29 |
            (uint32_t)(h.tsc != 0) << 30 | (uint32_t)h.di << 31;
    return true;
}

// the first payload bytes of the packet in word e as five dwords (byte i in bits 8 (i & 3).. of w[i >> 2]: what pes_start takes), each
// read where it still lies inside the packet and shifted down; bytes behind the packet's end read as 0.  A scrambled payload is not read
__device__ inline void pw_load_start(const uint8_t* __restrict__ ts, uint32_t e, uint32_t* w) {
    const int L = pw_len(e), o = TSMON_TS - L;
#pragma unroll
    for (int i = 0; i < 5; ++i) w[i] = 0;
    if (pw_scr(e)) return;
    const uint8_t* p = ts + (size_t)pw_k(e) * TSMON_TS;
#pragma unroll
    for (int i = 0; i < 5; ++i) {
        const int a = o + 4 * i, c = a > TSMON_TS - 4 ? TSMON_TS - 4 : a;
        const uint32_t v = *reinterpret_cast<const ts_unaligned_u32*>(p + c);
        w[i] = a - c >= 4 ? 0u : v >> (8 * (a - c));
    }
}

// the packet counters of phase C, per thread and slot run
struct PwPk { int packets, payload_bytes, duplicates, cc_errors, scrambled, malformed; };
// into the slot's counters in LDS (Cnt: PesCnt, EsCnt, AudCnt: each has the six fields)
template <typename Cnt>
__device__ inline void pw_flush_pk(Cnt* d, const PwPk& a) {
    atomicAdd(&d->packets, a.packets);
    if (a.payload_bytes) atomicAdd(&d->payload_bytes, a.payload_bytes);
    if (a.duplicates) atomicAdd(&d->duplicates, a.duplicates);
    if (a.cc_errors) atomicAdd(&d->cc_errors, a.cc_errors);
    if (a.scrambled) atomicAdd(&d->scrambled_packets, a.scrambled);
    if (a.malformed) atomicAdd(&d->malformed_packets, a.malformed);
}

// A: the watched packets of ts[0 .. n), compacted in input order into rec -> how many.  w: the 16 watches (LDS).  Every thread of the
// workgroup calls it, whatever n is
template <int WG>
__device__ inline int pw_compact(const uint8_t* __restrict__ ts, int n, const int32_t* w, int* wsum, uint32_t* rec) {
    int W = 0;
    if (n > 0) {
        int k0, k1; ts_thread_run(n, WG, &k0, &k1);              // <= 16 packets per thread
        unsigned mask = 0;
        uint32_t word;
        for (int k = k0; k < k1; ++k) if (pw_look(ts, k, w, &word)) mask |= 1u << (k - k0);
        int at = ts_block_scan<WG>(__popc(mask), wsum, &W);
        for (int k = k0; k < k1; ++k) {
            if (!(mask >> (k - k0) & 1)) continue;
            pw_look(ts, k, w, &word);
            rec[at++] = word;
        }
    }
    __syncthreads();
    return W;
}

// B: the stable counting sort by slot of rec[0 .. W), W > 0, into srt.  place: 16 x WG counts (LDS); start[slot], start[16] = W: the
// slots' runs in sorted order.  [*j0, *j1): the thread's run, of rec and of srt alike
template <int WG>
__device__ inline void pw_sort(const uint32_t* rec, uint32_t* srt, int W, uint16_t (*place)[WG], int32_t* start, int* wsum, int* j0p, int* j1p) {
    const int tid = threadIdx.x;
    int j0, j1; ts_thread_run(W, WG, &j0, &j1);
    for (int q = 0; q < PW_SLOTS; ++q) place[q][tid] = 0;
    for (int r = j0; r < j1; ++r) ++place[pw_slot(rec[r])][tid];
    __syncthreads();
    {
        uint16_t* flat = &place[0][0] + PW_SLOTS * tid;          // slot-major: 16 threads' counts of one slot
        int sum = 0, total;
        for (int i = 0; i < PW_SLOTS; ++i) sum += flat[i];
        int at = ts_block_scan<WG>(sum, wsum, &total);
        for (int i = 0; i < PW_SLOTS; ++i) { const int c = flat[i]; flat[i] = (uint16_t)at; at += c; }
    }
    __syncthreads();
    if (tid < PW_SLOTS) start[tid] = place[tid][0];
    if (tid == PW_SLOTS) start[PW_SLOTS] = W;
    __syncthreads();
    for (int r = j0; r < j1; ++r) { const uint32_t e = rec[r]; srt[place[pw_slot(e)][tid]++] = e; }
    __syncthreads();
    *j0p = j0; *j1p = j1;
}

// C: the continuity verdicts of srt[j0 .. j1).  cc0(slot): the slot's carried continuity byte; flush(slot, pk): the packet counters of
// one slot run of this thread; ncc[slot]: the slot's continuity byte behind the call, written by the lane of its last packet.
// *dupm / *gapm: bit j - j0 says DUPLICATE / a GAP mark.  The words are left as they are: every thread still reads its neighbour's counter
template <typename Cc0, typename Flush>
__device__ inline void pw_verdicts(const uint32_t* srt, int j0, int j1, const int32_t* start, Cc0 cc0, int* wsum, uint8_t* ncc, Flush flush, unsigned* dupm_out,
                                   unsigned* gapm_out) {
    // seen / last: the continuity state in front of sorted packet j
    auto front_cc = [&](int j, uint32_t e, bool* seen) {
        const int slot = pw_slot(e);
        if (j != start[slot]) { *seen = true; return pw_cc(srt[j - 1]); }
        const uint8_t c = cc0(slot);
        *seen = (c & TSMON_ST_SEEN) != 0;
        return c & 15;
    };
    auto eligible = [&](uint32_t e, bool seen, int last) { return seen && !pw_di(e) && pw_pay(e) && pw_cc(e) == last; };
    int mine = -1;
    for (int j = j0; j < j1; ++j) {
        const uint32_t e = srt[j];
        bool seen;
        const int last = front_cc(j, e, &seen);
        if (!eligible(e, seen, last)) mine = j;
    }
    int brk = ts_block_scan_max(mine, wsum);                     // the last sorted packet before j that is not eligible
    unsigned dupm = 0, gapm = 0;
    PwPk pk = {0, 0, 0, 0, 0, 0};
    int pk_slot = -1;
    for (int j = j0; j < j1; ++j) {
        const uint32_t e = srt[j];
        const int slot = pw_slot(e), head = start[slot], cc = pw_cc(e);
        bool seen;
        const int last = front_cc(j, e, &seen);
        int v = TSMON_CC_ERROR;
        if (!seen) v = TSMON_FIRST;
        else if (pw_di(e)) v = TSMON_DISC;
        else if (!pw_pay(e)) v = cc != last ? TSMON_CC_ERROR : TSMON_OK;
        else if (cc == ((last + 1) & 15)) v = TSMON_OK;
        else if (cc == last) {
            // its place in the run of equal counters; a run that reaches the slot's head goes on from the carried dup_used
            const int dup = brk >= head ? (j - brk) & 1 : ((cc0(slot) & TSMON_ST_DUP) != 0) ^ ((j - head + 1) & 1);
            v = dup ? TSMON_DUPLICATE : TSMON_CC_ERROR;
        }
        if (!eligible(e, seen, last)) brk = j;
        if (slot != pk_slot) {
            if (pk_slot >= 0) flush(pk_slot, pk);
            pk = PwPk{0, 0, 0, 0, 0, 0}; pk_slot = slot;
        }
        ++pk.packets;
        const bool dup = v == TSMON_DUPLICATE, malformed = !dup && pw_pay(e) && pw_len(e) == 0;
        pk.duplicates += dup; pk.cc_errors += v == TSMON_CC_ERROR; pk.malformed += malformed;
        if (!dup) { pk.payload_bytes += pw_len(e); pk.scrambled += pw_len(e) > 0 && pw_scr(e); }
        if (dup) dupm |= 1u << (j - j0);
        if (v == TSMON_CC_ERROR || v == TSMON_DISC || malformed) gapm |= 1u << (j - j0);
        if (j == start[slot + 1] - 1) ncc[slot] = (uint8_t)(TSMON_ST_SEEN | (dup ? TSMON_ST_DUP : 0) | cc);
    }
    if (pk_slot >= 0) flush(pk_slot, pk);
    *dupm_out = dupm; *gapm_out = gapm;
}

}  // namespace s2
