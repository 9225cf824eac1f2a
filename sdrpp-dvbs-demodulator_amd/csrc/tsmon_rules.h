// The rules of the TS monitor bank (own extension; include/dvbs2gpu.h), each stated once and shared by the kernels
// (tsmon.hip), the native host bank (tsmon.hip, TsmonHostStream) and a plain C++ test program: the six header bytes that matter,
// the classification of a packet, the continuity automaton of one (stream, PID), and the PID filter.
//
// A packet is 188 bytes at offset 188 k of a stream's input: the engine's packetisers emit whole packets from offset 0, there is no
// sync search.  Header fields as in ISO/IEC 13818-1 2.4.3.2.  Classification, in this order:
//   1. b0 != 0x47: a sync-byte error, nothing else of the packet is read;
//   2. TEI set: a TEI packet, its header is not trusted (no PID row, no continuity step);
//   3. PID 0x1FFF: a null packet (a PID row, no continuity step);
//   4. otherwise the packet takes the continuity step of its PID (tsmon_step below: the definition).
// A duplicate is recognised by its continuity counter ALONE: the 188 bytes of the two packets are not compared (the kernels read
// six bytes of a packet, not the packet).
// Standard headers only: the host tests compile this file with a plain C++ compiler.
#pragma once
#include <cstdint>

#ifdef __HIPCC__
#define TSMON_HD __host__ __device__
#else
#define TSMON_HD
#endif

namespace s2 {

constexpr int TSMON_TS = 188, TSMON_PIDS = 8192, TSMON_NULL_PID = 0x1FFF;
constexpr int TSMON_HDR_BYTES = 6;                       // of a packet, all the monitor's statistics read
// flags of a PID row (dvbs2gpu_tsmon_pid.flags)
constexpr int TSMON_FIRST_SEEN = 1, TSMON_DISCONTINUITY = 2;

enum TsmonClass { TSMON_SYNC_ERROR = 0, TSMON_TEI = 1, TSMON_NULL = 2, TSMON_DATA = 3 };

struct TsmonHdr { int cls, pid, pusi, tsc, afc, cc, di; };
// b: at least 4 readable bytes; b[4], b[5] are read only when the adaptation field control says that an adaptation field follows
TSMON_HD inline TsmonHdr tsmon_parse(const uint8_t* b) {
    TsmonHdr h = {TSMON_SYNC_ERROR, 0, 0, 0, 0, 0, 0};
    if (b[0] != 0x47) return h;
    h.pusi = (b[1] >> 6) & 1; h.pid = (b[1] & 0x1f) << 8 | b[2];
    h.tsc = b[3] >> 6; h.afc = (b[3] >> 4) & 3; h.cc = b[3] & 15;
    if (b[1] >> 7) { h.cls = TSMON_TEI; return h; }
    if ((h.afc & 2) && b[4] > 0) h.di = b[5] >> 7;
    h.cls = h.pid == TSMON_NULL_PID ? TSMON_NULL : TSMON_DATA;
    return h;
}

// The continuity state of one (stream, PID) in a byte: last CC in bits 0-3, dup_used bit 4, seen bit 5.  0: never seen.
constexpr uint8_t TSMON_ST_DUP = 0x10, TSMON_ST_SEEN = 0x20;
enum TsmonVerdict { TSMON_NO_VERDICT = 0, TSMON_OK = 1, TSMON_DUPLICATE = 2, TSMON_CC_ERROR = 3, TSMON_FIRST = 4, TSMON_DISC = 5 };
// One step of the automaton: the sequential form IS the definition; every other form must give its results for every cut of a
// stream into calls.
TSMON_HD inline int tsmon_step(uint8_t* state, int afc, int cc, int di) {
    const uint8_t st = *state;
    const int last = st & 15;
    if (!(st & TSMON_ST_SEEN)) { *state = (uint8_t)(TSMON_ST_SEEN | cc); return TSMON_FIRST; }
    if (di) { *state = (uint8_t)(TSMON_ST_SEEN | cc); return TSMON_DISC; }
    if (!(afc & 1)) {                                    // no payload: the counter does not advance
        *state = (uint8_t)(TSMON_ST_SEEN | cc);
        return cc != last ? TSMON_CC_ERROR : TSMON_OK;
    }
    if (cc == ((last + 1) & 15)) { *state = (uint8_t)(TSMON_ST_SEEN | cc); return TSMON_OK; }
    if (cc == last && !(st & TSMON_ST_DUP)) { *state = (uint8_t)(TSMON_ST_SEEN | TSMON_ST_DUP | cc); return TSMON_DUPLICATE; }
    *state = (uint8_t)(TSMON_ST_SEEN | cc);
    return TSMON_CC_ERROR;
}

// A PID row of one call as it grows; the layout of dvbs2gpu_tsmon_pid (include/dvbs2gpu.h; tsmon.hip asserts it)
struct TsmonRow { uint16_t pid, flags; uint32_t packets, cc_errors, duplicates, scrambled, pusi; };
// one trusted packet (TSMON_NULL or TSMON_DATA) enters its PID's row and, unless it is a null packet, steps the PID's state;
// returns the step's verdict (TSMON_NO_VERDICT for a null packet)
TSMON_HD inline int tsmon_row_add(TsmonRow* r, uint8_t* state, const TsmonHdr& h) {
    ++r->packets;
    r->scrambled += h.tsc != 0; r->pusi += h.pusi;
    if (h.cls != TSMON_DATA) return TSMON_NO_VERDICT;
    const int v = tsmon_step(state, h.afc, h.cc, h.di);
    r->cc_errors += v == TSMON_CC_ERROR; r->duplicates += v == TSMON_DUPLICATE;
    if (v == TSMON_FIRST) r->flags |= TSMON_FIRST_SEEN;
    if (v == TSMON_DISC) r->flags |= TSMON_DISCONTINUITY;
    return v;
}

// The PID filter of one stream.  mode 0: every PID passes; 1: the listed ones; 2: all but the listed ones.  The list is a bitmap
// of 8192 bits.  drop_null / drop_tei / drop_bad_sync take those packets out whatever the list says; a TEI packet or one with a
// bad sync byte has no trusted PID and passes unless its flag drops it.
struct TsmonFilter { int32_t mode, drop_null, drop_tei, drop_bad_sync; };
constexpr int TSMON_MAP_WORDS = TSMON_PIDS / 32;
TSMON_HD inline bool tsmon_passes(const TsmonHdr& h, const TsmonFilter& f, const uint32_t* map) {
    if (h.cls == TSMON_SYNC_ERROR) return !f.drop_bad_sync;
    if (h.cls == TSMON_TEI) return !f.drop_tei;
    if (h.cls == TSMON_NULL && f.drop_null) return false;
    if (f.mode == 0) return true;
    const bool listed = (map[h.pid >> 5] >> (h.pid & 31)) & 1;
    return f.mode == 1 ? listed : !listed;
}

// the counters one call adds to a stream's statistics (dvbs2gpu_tsmon_stats); needed: bytes of the passing packets
struct TsmonCall { int32_t needed, nrows, packets, null_packets, tei_packets, sync_byte_errors, cc_errors, duplicates, discontinuities,
                           scrambled_packets, passed_packets, first_seen; };

}  // namespace s2
