// The rules that the banks share which reassemble length-prefixed units from the payloads of one PID (psi_rules.h: PSI sections;
// dgram_rules.h: the datagram banks -- T2-MI packets, MPE sections, ULE SNDUs), each stated once for the kernels (ts_reasm.h), the host banks and the plain C++ test
// programs.  A unit STARTS only behind the pointer field of a PUSI packet; a packet without PUSI only continues the open unit and
// ignores what is left of its payload; scrambling, a continuity break or a malformed packet drops the open unit.
//
// ts_reasm_run, packet by packet, IS the definition.  A format supplies to it (F below; PsiHostStream and DgramHostStream each wrap
// themselves in one):
//   slot_of(pid)                      the slot that takes the PID, -1: none
//   state(s)  .cont .fill             tsmon_step's byte; the bytes of the open unit, 0: none is open
//   cnt(s)    .packets .scrambled_packets .malformed_packets
//   drop(s)                           the open unit, if there is one, is lost and counted
//   feed(s, b, n, &used, k, want)     n bytes for the slot's unit (open, or starting with them) in packet k; stops behind the unit's last
//                                     byte; true: the unit was completed and emitted (the format's own header, length and row rules)
//   begin(s, k)                       a unit starts in packet k
//   slack(s)                          the pointer bytes of a PUSI packet reached beyond the end of the open unit
//   stuffing(byte)                    the byte in a unit's first place that ends the packet's chain of units
// Standard headers only.
#pragma once
#include "bbts_rules.h"
#include "tsmon_rules.h"

#include <cstddef>

namespace s2 {

#ifdef __HIPCC__
#define TS_HD __host__ __device__
#else
#define TS_HD
#endif

// the payload's first byte: 4, or 5 + adaptation_field_length; >= 188 is malformed
TS_HD inline int ts_payload_start(int afc, unsigned b4) { return (afc & 2) ? 5 + (int)b4 : 4; }
// CRC-32/MPEG of a whole unit from the initial value 0xFFFFFFFF: 0 for an intact one
TS_HD inline uint32_t ts_crc32(const uint8_t* b, int n) {
    uint32_t c = 0xFFFFFFFFu;
    for (int i = 0; i < n; ++i) c = crc32m_byte(c, b[i]);
    return c;
}

// What a packet of a slot's PID is to the open unit (the parallel form's restatement of the loop below, packet by packet): SKIP brings
// nothing and changes nothing (a duplicate, no payload); CUT drops it and brings nothing; CONT continues it; PUSI completes or drops it
// in its pointer bytes and starts units behind them; PUSI_BRK: a PUSI packet behind a continuity break, the open unit is dropped first.
enum { PK_SKIP = 0, PK_CUT, PK_CONT, PK_PUSI, PK_PUSI_BRK };
struct TsPacketClass { int kind; bool scrambled, malformed; };
// verdict: tsmon_step's for the packet; ps: ts_payload_start; ptr: the byte at ps of a PUSI packet with payload
TS_HD inline TsPacketClass ts_packet_class(int verdict, bool scrambled, int afc, int ps, int pusi, int ptr) {
    const bool brk = verdict == TSMON_CC_ERROR || verdict == TSMON_DISC;
    if (scrambled) return {PK_CUT, true, false};
    if (verdict == TSMON_DUPLICATE) return {PK_SKIP, false, false};
    if (!(afc & 1)) return {brk ? PK_CUT : PK_SKIP, false, false};
    if (ps >= TSMON_TS || (pusi && ptr > TSMON_TS - ps - 1)) return {PK_CUT, false, true};
    if (pusi) return {brk ? PK_PUSI_BRK : PK_PUSI, false, false};
    return {brk ? PK_CUT : PK_CONT, false, false};
}

// one call: n packets
template <typename F>
inline void ts_reasm_run(F f, const uint8_t* ts, int n, bool want_bytes) {
    for (int k = 0; k < n; ++k) {
        const uint8_t* p = ts + (size_t)k * TSMON_TS;
        const TsmonHdr h = tsmon_parse(p);
        if (h.cls != TSMON_DATA) continue;
        const int s = f.slot_of(h.pid);
        if (s < 0) continue;
        auto& sl = f.state(s);
        ++f.cnt(s).packets;
        if (h.tsc) { ++f.cnt(s).scrambled_packets; f.drop(s); tsmon_step(&sl.cont, h.afc, h.cc, h.di); continue; }
        const int v = tsmon_step(&sl.cont, h.afc, h.cc, h.di);
        if (v == TSMON_DUPLICATE) continue;
        if (v == TSMON_CC_ERROR || v == TSMON_DISC) f.drop(s);
        if (!(h.afc & 1)) continue;
        const int ps = ts_payload_start(h.afc, p[4]);
        if (ps >= TSMON_TS) { ++f.cnt(s).malformed_packets; f.drop(s); continue; }
        int used = 0;
        if (!h.pusi) {
            if (sl.fill > 0) f.feed(s, p + ps, TSMON_TS - ps, &used, k, want_bytes);
            continue;
        }
        const int ptr = p[ps];
        if (ptr > TSMON_TS - ps - 1) { ++f.cnt(s).malformed_packets; f.drop(s); continue; }
        if (sl.fill > 0) {
            if (!f.feed(s, p + ps + 1, ptr, &used, k, want_bytes)) f.drop(s);
            else if (used < ptr) f.slack(s);
        }
        for (int at = ps + 1 + ptr; at < TSMON_TS && !f.stuffing(p[at]); at += used) {
            f.begin(s, k);
            if (!f.feed(s, p + at, TSMON_TS - at, &used, k, want_bytes)) break;
        }
    }
}

}  // namespace s2
