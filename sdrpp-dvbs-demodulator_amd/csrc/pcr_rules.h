// The rules of the PCR bank (own extension; include/dvbs2gpu.h), each stated once and shared by the kernel (pcr.hip),
// the native host bank (PcrHostStream below, behind dvbs2gpu_pcr_create_host) and a plain C++ test program: which packet carries a
// PCR and when it is malformed, the step of one watched PID's clock state for a (PCR value, packet position) pair, the accuracy
// of a pair against the stream's rate, and what a step adds to its slot's counters.
//
// The sequential form -- PcrHostStream::run, packet by packet -- IS the definition; every other form must give its results for every
// cut of a stream into calls.  Everything is integer arithmetic on (P, n): P the 27 MHz PCR value modulo PCR_MOD, n the packet's
// position in the stream.  PCR syntax as in ISO/IEC 13818-1 2.4.3.4 / 2.4.3.5, limits as in ETSI TR 101 290 2.3a, 2.3b, 2.4.
// Standard headers only: the host tests compile this file with a plain C++ compiler.
#pragma once
#include "tsmon_rules.h"

#include <cstddef>
#include <vector>

#ifdef __HIPCC__
#define PCR_HD __host__ __device__
#else
#define PCR_HD
#endif

namespace s2 {

constexpr int PCR_SLOTS = 16;
constexpr uint64_t PCR_MOD = (1ull << 33) * 300;            // 2 576 980 377 600: P = base * 300 + ext
constexpr uint32_t PCR_LATE_TICKS = 1080000;                // 40 ms: more is LATE (TR 101 290 2.3a)
constexpr uint32_t PCR_JUMP_TICKS = 2700000;                // 100 ms: more is JUMP (2.3b); a backward step lands here
constexpr int64_t PCR_MAX_DN = 32767;                       // packets between the two PCRs of a measured pair; more is SATURATED
constexpr int32_t PCR_DEFAULT_LIMIT_Q6 = 864;               // 13.5 ticks = 500 ns in 1/64 tick (2.4)
constexpr uint64_t PCR_MAX_TPP = 1ull << 48;                // ticks per packet in Q24.24 stay below this
enum PcrKind { PCR_FIRST = 0, PCR_ANNOUNCED = 1, PCR_REPEATED = 2, PCR_OK = 3, PCR_LATE = 4, PCR_JUMP = 5, PCR_KINDS = 6 };
constexpr int PCR_ACCURACY_ERROR = 1, PCR_SATURATED = 2;    // row flags (DVBS2GPU_PCR_*)

// bytes 4..11 of a packet whose adaptation field control says that an adaptation field follows (b[0]: adaptation_field_length,
// b[1]: its flags, b[2..7]: program_clock_reference_base 33, 6 reserved, extension 9)
enum { PCR_NONE = 0, PCR_GOOD = 1, PCR_MALFORMED = 2 };
PCR_HD inline int pcr_parse(int afc, const uint8_t* b, uint64_t* P) {
    if (!(afc & 2) || b[0] < 1 || !(b[1] & 0x10)) return PCR_NONE;
    const unsigned ext = (b[6] & 1u) << 8 | b[7];
    if (b[0] < 7 || b[0] > (afc == 3 ? 182 : 183) || ext > 299) return PCR_MALFORMED;
    const uint64_t base = (uint64_t)b[2] << 25 | (uint64_t)b[3] << 17 | (uint64_t)b[4] << 9 | (uint64_t)b[5] << 1 | b[6] >> 7;
    *P = base * 300 + ext;
    return PCR_GOOD;
}

struct PcrRate { uint64_t tpp; int32_t limit, pad; };       // tpp: 27 MHz ticks per packet in Q24.24, 0: not set; limit in 1/64 tick

#pragma pack(push, 4)
struct PcrRow {                                             // the layout of dvbs2gpu_pcr_row: 32 bytes, pcr at offset 12
    uint16_t pid; uint8_t slot, kind; uint16_t flags, reserved;
    int32_t packet;
    uint64_t pcr;
    uint32_t delta_ticks, delta_packets;
    int32_t accuracy;
};
#pragma pack(pop)

// The state of one slot: seen; the last PCR value; ref_n, the position that the next interval is measured from
struct PcrState { uint64_t last_pcr; int64_t ref_n; uint32_t seen, pad; };

PCR_HD inline uint32_t pcr_sat32(uint64_t v) { return v > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)v; }

// One step: the record (P, n, di) against the state before it.  Fills kind, flags, delta_ticks, delta_packets and accuracy of *r and
// returns the state behind it.  A REPEATED record leaves the state as it is: the pair after a run of equal values is measured from
// the run's first packet.
PCR_HD inline PcrState pcr_step(const PcrState& st, uint64_t P, int64_t n, int di, const PcrRate& rt, PcrRow* r) {
    const PcrState next = {P, n, 1, 0};
    r->flags = 0; r->delta_ticks = 0; r->delta_packets = 0; r->accuracy = 0;
    if (!st.seen) { r->kind = PCR_FIRST; return next; }
    if (di) { r->kind = PCR_ANNOUNCED; return next; }
    if (P == st.last_pcr) { r->kind = PCR_REPEATED; return st; }
    const uint64_t dP = P >= st.last_pcr ? P - st.last_pcr : P + PCR_MOD - st.last_pcr;
    const int64_t dN = n - st.ref_n;
    r->delta_ticks = pcr_sat32(dP); r->delta_packets = pcr_sat32((uint64_t)dN);
    if (dP > PCR_JUMP_TICKS) { r->kind = PCR_JUMP; return next; }
    r->kind = dP > PCR_LATE_TICKS ? PCR_LATE : PCR_OK;
    if (rt.tpp) {
        // dP < 2^22 and min(dN, 32767) * tpp < 2^63: e fits
        const int64_t e = (int64_t)(dP << 24) - (dN < PCR_MAX_DN ? dN : PCR_MAX_DN) * (int64_t)rt.tpp;
        const int64_t a = e >> 18, lim = 0x7FFFFFFF;
        r->accuracy = (int32_t)(a > lim ? lim : (a < -lim ? -lim : a));
        if ((r->accuracy < 0 ? -(int64_t)r->accuracy : (int64_t)r->accuracy) > rt.limit) r->flags |= PCR_ACCURACY_ERROR;
        if (dN > PCR_MAX_DN) r->flags |= PCR_SATURATED;
    }
    return next;
}

// what one call adds to a slot's statistics.  last_k: the index in the call of the slot's last record, -1: none
struct PcrCnt {
    int32_t kind[PCR_KINDS];
    int32_t malformed, accuracy_measured, accuracy_errors;
    uint32_t max_delta_ticks, max_abs_accuracy;
    int32_t last_k;
    uint64_t sum_ticks, sum_packets;
};
PCR_HD inline PcrCnt pcr_cnt_zero() { return PcrCnt{{0, 0, 0, 0, 0, 0}, 0, 0, 0, 0, 0, -1, 0, 0}; }
// a stepped record into its slot's counters
PCR_HD inline void pcr_cnt_add(PcrCnt* c, const PcrRow& r, bool rate_set) {
    for (int i = 0; i < PCR_KINDS; ++i) c->kind[i] += r.kind == i;      // (no run-time index: the kernel keeps *c in registers)
    if (r.kind != PCR_LATE && r.kind != PCR_OK) return;
    if (r.delta_ticks > c->max_delta_ticks) c->max_delta_ticks = r.delta_ticks;
    if (!(r.flags & PCR_SATURATED)) { c->sum_ticks += r.delta_ticks; c->sum_packets += r.delta_packets; }
    if (!rate_set) return;
    ++c->accuracy_measured;
    c->accuracy_errors += r.flags & PCR_ACCURACY_ERROR;
    const uint32_t a = r.accuracy < 0 ? (uint32_t)-(int64_t)r.accuracy : (uint32_t)r.accuracy;
    if (a > c->max_abs_accuracy) c->max_abs_accuracy = a;
}
// the header of a stream's call record; the slots' PcrCnt follow it (PcrCall in pcr.hip)
struct PcrCallHead { int32_t records, unwatched, first_unwatched_pid, pad; };

// ------------------------------------------------------------------------------------------------- the sequential definition
struct PcrHostStream {
    int32_t watch[PCR_SLOTS];                               // -1: the slot watches nothing
    PcrRate rate = {0, PCR_DEFAULT_LIMIT_Q6, 0};
    PcrState slot[PCR_SLOTS];
    int64_t packets = 0;                                    // the position of the next call's first packet
    // of the last call
    std::vector<PcrRow> rows;                               // the first max_rows
    PcrCnt cnt[PCR_SLOTS];
    PcrCallHead head = {0, 0, -1, 0};

    PcrHostStream() {
        for (int s = 0; s < PCR_SLOTS; ++s) { watch[s] = -1; slot[s] = PcrState{0, 0, 0, 0}; cnt[s] = pcr_cnt_zero(); }
    }
    void clear_slot(int s) { slot[s] = PcrState{0, 0, 0, 0}; }
    void reset() {
        for (int s = 0; s < PCR_SLOTS; ++s) clear_slot(s);
        packets = 0; rows.clear(); head = {0, 0, -1, 0};
    }
    // one call: n packets
    void run(const uint8_t* ts, int n, int max_rows) {
        rows.clear();
        head = {0, 0, -1, 0};
        for (int s = 0; s < PCR_SLOTS; ++s) cnt[s] = pcr_cnt_zero();
        for (int k = 0; k < n; ++k) {
            const uint8_t* p = ts + (size_t)k * TSMON_TS;
            const TsmonHdr h = tsmon_parse(p);
            if (h.cls != TSMON_DATA || !(h.afc & 2)) continue;
            uint64_t P = 0;
            const int v = pcr_parse(h.afc, p + 4, &P);
            if (v == PCR_NONE) continue;
            int s = 0;
            while (s < PCR_SLOTS && watch[s] != h.pid) ++s;
            if (s == PCR_SLOTS) {
                if (v != PCR_GOOD) continue;
                if (!head.unwatched++) head.first_unwatched_pid = h.pid;
                continue;
            }
            if (v == PCR_MALFORMED) { ++cnt[s].malformed; continue; }
            PcrRow r = {(uint16_t)h.pid, (uint8_t)s, 0, 0, 0, k, P, 0, 0, 0};
            slot[s] = pcr_step(slot[s], P, packets + k, h.di, rate, &r);
            pcr_cnt_add(&cnt[s], r, rate.tpp != 0);
            cnt[s].last_k = k;
            if (head.records++ < max_rows) rows.push_back(r);
        }
        packets += n;
    }
};

}  // namespace s2
