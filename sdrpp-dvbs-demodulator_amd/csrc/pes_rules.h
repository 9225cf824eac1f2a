// The rules of the PES bank (own extension; include/dvbs2gpu.h), each stated once and shared by the kernel (pes.hip),
// the native host bank (PesHostStream below, behind dvbs2gpu_pes_create_host) and a plain C++ test program: where a packet's payload
// lies, what the first bytes of a PES packet say (pes_start), the step of one watched PID's state for a start (pes_step: what the
// start closes, what it opens, its timestamp against the one before), and what a row adds to its slot's counters.
//
// The sequential form -- PesHostStream::run, packet by packet -- IS the definition; every other form must give its results for every
// cut of a stream into calls.  Everything is integer arithmetic: byte and packet counts, 33-bit timestamps at 90 kHz modulo 2^33 and
// the packet's position n in the stream.  PES syntax as in ISO/IEC 13818-1 2.4.3.6 / 2.4.3.7, limits as in ETSI TR 101 290 2.5.
// Standard headers only: the host tests compile this file with a plain C++ compiler.
#pragma once
#include "tsmon_rules.h"

#include <cstddef>
#include <vector>

#ifdef __HIPCC__
#define PES_HD __host__ __device__
#else
#define PES_HD
#endif

namespace s2 {

constexpr int PES_SLOTS = 16;
constexpr uint64_t PES_TS_MOD = 1ull << 33, PES_TS_HALF = 1ull << 32, PES_NO_TS = ~0ull;
constexpr uint32_t PES_GAP_TICKS = 63000;                   // 0.7 s at 90 kHz: a larger step of the timestamps is TS_GAP
constexpr uint64_t PES_LATE_TICKS = 18900000;               // 0.7 s at 27 MHz: more between two PTS is PTS_LATE (TR 101 290 2.5)
constexpr uint64_t PES_MAX_TPP = 1ull << 48;                // ticks per packet in Q24.24 stay below this (the PCR bank's quantity)
constexpr int PES_HEAD_BYTES = 19;                          // of a PES packet, all that is read: up to the DTS
enum PesKind { PES_SCRAMBLED = 0, PES_SHORT = 1, PES_BAD_START = 2, PES_PLAIN = 3, PES_MALFORMED = 4, PES_HEADER = 5, PES_KINDS = 6 };
// row flags (DVBS2GPU_PES_*)
constexpr int PES_CLOSED = 1, PES_CLOSED_GAP = 2, PES_CLOSED_MISMATCH = 4, PES_CLOSED_UNCHECKED = 8, PES_UNBOUNDED_NONVIDEO = 16, PES_TS_FIRST = 32,
              PES_TS_BACKWARD = 64, PES_TS_GAP = 128, PES_PTS_LATE = 256, PES_DTS_AFTER_PTS = 512;

// the payload bytes L of a trusted packet: -1 none (AFC&1 clear), 0 malformed (AFC 3 with an adaptation field that leaves no
// payload byte), else 184 or 183 - b4; the payload starts at 188 - L.  b4 is read only with AFC 3
PES_HD inline int pes_payload_len(int afc, unsigned b4) {
    if (!(afc & 1)) return -1;
    if (afc == 1) return TSMON_TS - 4;
    return b4 > 182 ? 0 : TSMON_TS - 5 - (int)b4;
}

// The rate of a stream: tpp, 27 MHz ticks per packet in Q24.24 (0: not set), and the packets that 0.7 s hold at it
struct PesRate { uint64_t tpp; int64_t late_packets; };
inline PesRate pes_rate(uint64_t tpp) { return PesRate{tpp, tpp ? (int64_t)((PES_LATE_TICKS << 24) / tpp) : 0}; }

#pragma pack(push, 4)
struct PesRow {                                             // the layout of dvbs2gpu_pes_row: 48 bytes, pts at offset 16
    uint16_t pid; uint8_t slot, kind; uint16_t flags; uint8_t stream_id, reserved;
    int32_t packet; uint32_t declared;
    uint64_t pts, dts;
    uint32_t closed_bytes, closed_packets, delta_packets;
    int32_t delta_ts;
};
#pragma pack(pop)

// what the first bytes of a PES packet say
struct PesHead { uint32_t kind, stream_id, declared, unbounded; uint64_t pts, dts; };

// a 33-bit timestamp in the five bytes b0..b4; false: a marker bit is 0 or the 4-bit prefix is not `prefix`
PES_HD inline bool pes_timestamp(unsigned b0, unsigned b1, unsigned b2, unsigned b3, unsigned b4, unsigned prefix, uint64_t* t) {
    *t = (uint64_t)(b0 >> 1 & 7) << 30 | (uint64_t)b1 << 22 | (uint64_t)(b2 >> 1) << 15 | (uint64_t)b3 << 7 | b4 >> 1;
    return b0 >> 4 == prefix && (b0 & 1) && (b2 & 1) && (b4 & 1);
}

// A start: the first min(L, 19) payload bytes of a packet with PUSI, byte i in bits 8 (i & 3).. of w[i >> 2] (the rest 0), the
// payload's length L >= 1 and the packet's transport_scrambling_control.  The kinds are decided in the order of the header's table.
PES_HD inline PesHead pes_start(const uint32_t* w, int L, int tsc) {
#define PES_B(i) ((w[(i) >> 2] >> (8 * ((i) & 3))) & 255u)
    PesHead h = {PES_SCRAMBLED, 0, 0, 0, PES_NO_TS, PES_NO_TS};
    if (tsc) return h;
    h.kind = PES_SHORT;
    if (L < 6) return h;
    const unsigned sid = PES_B(3);
    h.stream_id = sid;
    if (PES_B(0) != 0 || PES_B(1) != 0 || PES_B(2) != 1) { h.kind = PES_BAD_START; return h; }
    h.declared = PES_B(4) << 8 | PES_B(5);
    if (sid == 0xBC || sid == 0xBE || sid == 0xBF || sid == 0xF0 || sid == 0xF1 || sid == 0xF2 || sid == 0xF8 || sid == 0xFF) { h.kind = PES_PLAIN; return h; }
    if (L < 9) return h;
    const unsigned fl = PES_B(7) >> 6, hdl = PES_B(8);
    if ((PES_B(6) & 0xC0) != 0x80 || fl == 1 || (fl == 2 && hdl < 5) || (fl == 3 && hdl < 10)) { h.kind = PES_MALFORMED; return h; }
    if ((fl == 2 && L < 14) || (fl == 3 && L < 19)) return h;                      // the header is split over packets: not parsed
    uint64_t pts = PES_NO_TS, dts = PES_NO_TS;
    bool good = true;
    if (fl >= 2) good = pes_timestamp(PES_B(9), PES_B(10), PES_B(11), PES_B(12), PES_B(13), fl, &pts);
    if (fl == 3) good = pes_timestamp(PES_B(14), PES_B(15), PES_B(16), PES_B(17), PES_B(18), 1, &dts) && good;
    if (!good) { h.kind = PES_MALFORMED; return h; }
    h.kind = PES_HEADER; h.pts = pts; h.dts = dts;
    h.unbounded = h.declared == 0 && (sid < 0xE0 || sid > 0xEF);
    return h;
#undef PES_B
}

// The state of one slot.  cc: the TS monitor's continuity byte.  The open PES packet: open, its declared PES_packet_length, the
// payload bytes and packets it has had (saturating), gap (marked GAP).  The timestamps: seen, the last T, ref_n its position.
struct PesState { uint64_t last_t; int64_t ref_n; uint32_t bytes, packets, declared; uint8_t cc, open, gap, seen; };

PES_HD inline uint32_t pes_sat32(uint64_t v) { return v > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)v; }

// One step: the start `h` of L payload bytes at position n against the state before it.  Fills everything of *r but pid, slot and
// packet and returns the state behind it (cc as it was).
PES_HD inline PesState pes_step(const PesState& st, const PesHead& h, int L, int64_t n, const PesRate& rt, PesRow* r) {
    PesState nx = st;
    r->kind = (uint8_t)h.kind; r->stream_id = (uint8_t)h.stream_id; r->reserved = 0; r->declared = h.declared;
    r->pts = h.pts; r->dts = h.dts;
    r->closed_bytes = 0; r->closed_packets = 0; r->delta_packets = 0; r->delta_ts = 0;
    unsigned f = h.unbounded ? PES_UNBOUNDED_NONVIDEO : 0;
    if (st.open) {
        r->closed_bytes = st.bytes; r->closed_packets = st.packets;
        f |= PES_CLOSED;
        if (st.gap) f |= PES_CLOSED_GAP;
        else if (st.declared == 0) f |= PES_CLOSED_UNCHECKED;
        else if (st.bytes != st.declared + 6) f |= PES_CLOSED_MISMATCH;
    }
    nx.open = 1; nx.gap = 0; nx.declared = h.declared; nx.bytes = (uint32_t)L; nx.packets = 1;
    if (h.kind == PES_HEADER && h.pts != PES_NO_TS) {
        const uint64_t T = h.dts != PES_NO_TS ? h.dts : h.pts;
        if (h.dts != PES_NO_TS && ((h.pts - h.dts) & (PES_TS_MOD - 1)) >= PES_TS_HALF) f |= PES_DTS_AFTER_PTS;
        if (!st.seen) f |= PES_TS_FIRST;
        else {
            const uint64_t dT = (T - st.last_t) & (PES_TS_MOD - 1);
            const int64_t dN = n - st.ref_n;
            if (dT >= PES_TS_HALF) f |= PES_TS_BACKWARD;
            else if (dT > PES_GAP_TICKS) f |= PES_TS_GAP;
            if (rt.tpp && dN > rt.late_packets) f |= PES_PTS_LATE;
            const int64_t d = dT >= PES_TS_HALF ? (int64_t)dT - (int64_t)PES_TS_MOD : (int64_t)dT, lim = 0x7FFFFFFF;
            r->delta_ts = (int32_t)(d > lim ? lim : (d < -lim - 1 ? -lim - 1 : d));
            r->delta_packets = pes_sat32((uint64_t)dN);
        }
        nx.seen = 1; nx.last_t = T; nx.ref_n = n;
    }
    r->flags = (uint16_t)f;
    return nx;
}

// what one call adds to a slot's statistics.  last_k: the index in the call of the slot's last start, -1: none
struct PesCnt {
    int32_t packets, payload_bytes, duplicates, cc_errors, scrambled_packets, malformed_packets;
    int32_t kind[PES_KINDS];
    int32_t with_pts, with_dts, closed_ok, closed_mismatch, closed_gap, closed_unchecked, ts_backward, ts_gap, pts_late, dts_after_pts;
    uint32_t max_delta_packets;
    int32_t last_k;
};
PES_HD inline PesCnt pes_cnt_zero() { return PesCnt{0, 0, 0, 0, 0, 0, {0, 0, 0, 0, 0, 0}, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, -1}; }
// a start's row into its slot's counters
PES_HD inline void pes_cnt_add(PesCnt* c, const PesRow& r) {
    for (int i = 0; i < PES_KINDS; ++i) c->kind[i] += r.kind == i;        // (no run-time index: the kernel keeps *c in registers)
    const unsigned f = r.flags;
    c->with_pts += r.kind == PES_HEADER && r.pts != PES_NO_TS; c->with_dts += r.kind == PES_HEADER && r.dts != PES_NO_TS;
    c->closed_ok += (f & (PES_CLOSED | PES_CLOSED_GAP | PES_CLOSED_MISMATCH | PES_CLOSED_UNCHECKED)) == PES_CLOSED;
    c->closed_mismatch += (f & PES_CLOSED_MISMATCH) != 0; c->closed_gap += (f & PES_CLOSED_GAP) != 0; c->closed_unchecked += (f & PES_CLOSED_UNCHECKED) != 0;
    c->ts_backward += (f & PES_TS_BACKWARD) != 0; c->ts_gap += (f & PES_TS_GAP) != 0; c->pts_late += (f & PES_PTS_LATE) != 0;
    c->dts_after_pts += (f & PES_DTS_AFTER_PTS) != 0;
    if (r.delta_packets > c->max_delta_packets) c->max_delta_packets = r.delta_packets;
}
// the header of a stream's call record; the slots' PesCnt follow it (PesCall in pes.hip)
struct PesCallHead { int32_t starts, pad[3]; };

// ------------------------------------------------------------------------------------------------- the sequential definition
struct PesHostStream {
    int32_t watch[PES_SLOTS];                               // -1: the slot watches nothing
    PesRate rate = {0, 0};
    PesState slot[PES_SLOTS];
    int64_t packets = 0;                                    // the position of the next call's first packet
    // of the last call
    std::vector<PesRow> rows;                               // the first max_rows
    PesCnt cnt[PES_SLOTS];
    PesCallHead head = {0, {0, 0, 0}};

    PesHostStream() {
        for (int s = 0; s < PES_SLOTS; ++s) { watch[s] = -1; clear_slot(s); cnt[s] = pes_cnt_zero(); }
    }
    void clear_slot(int s) { slot[s] = PesState{0, 0, 0, 0, 0, 0, 0, 0, 0}; }
    void reset() {
        for (int s = 0; s < PES_SLOTS; ++s) clear_slot(s);
        packets = 0; rows.clear(); head = {0, {0, 0, 0}};
    }
    // one call: n packets
    void run(const uint8_t* ts, int n, int max_rows) {
        rows.clear();
        head = {0, {0, 0, 0}};
        for (int s = 0; s < PES_SLOTS; ++s) cnt[s] = pes_cnt_zero();
        for (int k = 0; k < n; ++k) {
            const uint8_t* p = ts + (size_t)k * TSMON_TS;
            const TsmonHdr h = tsmon_parse(p);
            if (h.cls != TSMON_DATA) continue;
            int s = 0;
            while (s < PES_SLOTS && watch[s] != h.pid) ++s;
            if (s == PES_SLOTS) continue;
            PesState& st = slot[s];
            PesCnt& c = cnt[s];
            ++c.packets;
            const int v = tsmon_step(&st.cc, h.afc, h.cc, h.di);
            if (v == TSMON_DUPLICATE) { ++c.duplicates; continue; }
            c.cc_errors += v == TSMON_CC_ERROR;
            if (v == TSMON_CC_ERROR || v == TSMON_DISC) st.gap = 1;
            const int L = pes_payload_len(h.afc, h.afc == 3 ? p[4] : 0);
            if (L < 0) continue;
            if (L == 0) { ++c.malformed_packets; st.gap = 1; continue; }
            c.payload_bytes += L;
            c.scrambled_packets += h.tsc != 0;
            if (!h.pusi) { st.bytes = pes_sat32((uint64_t)st.bytes + L); st.packets = pes_sat32((uint64_t)st.packets + 1); continue; }
            uint32_t w[5] = {0, 0, 0, 0, 0};
            const uint8_t* pay = p + TSMON_TS - L;
            for (int i = 0; i < L && i < PES_HEAD_BYTES; ++i) w[i >> 2] |= (uint32_t)pay[i] << (8 * (i & 3));
            PesRow r = {(uint16_t)h.pid, (uint8_t)s, 0, 0, 0, 0, k, 0, 0, 0, 0, 0, 0, 0};
            st = pes_step(st, pes_start(w, L, h.tsc), L, packets + k, rate, &r);
            pes_cnt_add(&c, r);
            c.last_k = k;
            if (head.starts++ < max_rows) rows.push_back(r);
        }
        packets += n;
    }
};

}  // namespace s2
