// The rules of the PSI section bank (own extension; include/dvbs2gpu.h), each stated once and shared by the kernels
// (psi.hip), the native host bank (PsiHostStream below, behind dvbs2gpu_psi_create_host) and a plain C++ test program: the section
// syntax as one struct of offsets (PsiLayout), what a packet of a watched PID does to its slot, what an emitted section's row says,
// and the PAT / PMT parsers of the decoded views.
//
// The sequential form -- PsiHostStream::run, packet by packet -- IS the definition; every other form must give its results for every
// cutting of a stream into calls.  The section syntax is written from memory of ISO/IEC 13818-1 2.4.4: every offset and limit the
// code relies on is a field of PsiLayout, reported through dvbs2gpu_psi_get_layout and compared with the tests' model.
// Standard headers only: the host tests compile this file with a plain C++ compiler.
#pragma once
#include "ts_reasm_rules.h"

#include <cstring>
#include <vector>

namespace s2 {

struct PsiLayout {                     // the layout of dvbs2gpu_psi_layout (psi.hip asserts it)
    int32_t header_bytes;              // table_id, then 4 flag bits and the 12-bit section_length: 3
    int32_t length_mask;               // of (b1 << 8 | b2): 0x0FFF
    int32_t max_section_length;        // 4093: a section is at most 4096 bytes
    int32_t max_section_bytes;         // 4096
    int32_t min_long_section;          // a section with section_syntax_indicator holds the long header and a CRC: 12 bytes
    int32_t ext_at;                    // table_id_extension, 2 bytes
    int32_t version_at;                // (b >> 1) & 31; current_next_indicator b & 1
    int32_t section_number_at, last_section_number_at;
    int32_t long_header_bytes;         // 8
    int32_t crc_bytes;                 // 4
    int32_t pat_loop_at, pat_stride;   // {program_number 16, 3 reserved, PID 13}
    int32_t pmt_pcr_at;                // 3 reserved, PCR_PID 13
    int32_t pmt_info_length_at;        // 4 reserved, program_info_length 12
    int32_t pmt_loop_at, pmt_stride;   // {stream_type 8, 3 + PID 13, 4 + ES_info_length 12} then ES_info_length bytes
};
constexpr PsiLayout PSI = {3, 0x0FFF, 4093, 4096, 12, 3, 5, 6, 7, 8, 4, 8, 4, 8, 10, 12, 5};

constexpr int PSI_SLOTS = 16, PSI_BUF = 4096;
constexpr int PSI_CRC_ERROR = 1, PSI_CHANGED = 2;          // row flags (DVBS2GPU_PSI_*)

struct PsiWatch { int32_t pid, expect; };                  // pid -1: the slot watches nothing; expect -1: any table_id
// the counters one call adds to a slot's statistics (the first eleven words of dvbs2gpu_psi_stats, as 32-bit shares)
struct PsiCnt { int32_t packets, sections, valid, changed, crc_errors, dropped_sections, malformed_sections, malformed_packets, scrambled_packets,
                        unexpected_table_id, bytes_delivered; };
constexpr int PSI_NCNT = 11;
// one emitted section; the layout of dvbs2gpu_psi_section
struct PsiRow {
    uint16_t pid, flags;
    uint8_t table_id, ssi, version, current_next, section_number, last_section_number;
    uint16_t table_id_ext;
    int32_t length, offset, first_packet;
};

// section_length from the second and third header byte; the section's bytes are PSI.header_bytes more
TS_HD inline int psi_section_length(unsigned b1, unsigned b2) { return (int)((b1 << 8 | b2) & (unsigned)PSI.length_mask); }
// ts_payload_start under the name that the stand-alone test program of these rules calls
inline int psi_payload_start(int afc, unsigned b4) { return ts_payload_start(afc, b4); }
// the last four bytes, big-endian; of a shorter section all its bytes
TS_HD inline uint32_t psi_last4(const uint8_t* b, int n) {
    uint32_t v = 0;
    for (int i = n < 4 ? 0 : n - 4; i < n; ++i) v = v << 8 | b[i];
    return v;
}
// the row of an emitted section from its bytes (flags: PSI_CRC_ERROR only, offset -1); rd(i): byte i
template <typename Rd>
TS_HD inline PsiRow psi_row_fields(Rd rd, int total, int pid, bool valid, int first_packet) {
    PsiRow r = {(uint16_t)pid, (uint16_t)(valid ? 0 : PSI_CRC_ERROR), (uint8_t)rd(0), (uint8_t)(rd(1) >> 7), 0, 0, 0, 0, 0, total, -1, first_packet};
    if (r.ssi) {                                           // total >= PSI.min_long_section
        r.table_id_ext = (uint16_t)(rd(PSI.ext_at) << 8 | rd(PSI.ext_at + 1));
        r.version = (uint8_t)((rd(PSI.version_at) >> 1) & 31); r.current_next = (uint8_t)(rd(PSI.version_at) & 1);
        r.section_number = (uint8_t)rd(PSI.section_number_at); r.last_section_number = (uint8_t)rd(PSI.last_section_number_at);
    }
    return r;
}
// a valid changed section that the host keeps as the slot's decoded view: a current PAT or PMT
TS_HD inline bool psi_is_view(const PsiRow& r) {
    return (r.flags & PSI_CHANGED) && r.ssi && (r.table_id == 0 || r.table_id == 2) && r.current_next;
}

// ------------------------------------------------------------------------------------------------- decoded views (host)
struct PsiProgram { uint16_t program_number, pid; };               // dvbs2gpu_psi_program
struct PsiPatHeader { int32_t transport_stream_id, version, malformed; };          // dvbs2gpu_psi_pat (-1, -1, 0: no PAT held)
struct PsiEs { uint16_t stream_type, elementary_pid; };            // dvbs2gpu_psi_es
struct PsiPmtHeader { int32_t program_number, version, pcr_pid, malformed; };      // dvbs2gpu_psi_pmt (-1, ...: no PMT held)
// b[n]: a whole valid section with table_id 0.  No byte outside it is read; a loop that does not end at the CRC makes the view empty.
inline PsiPatHeader psi_parse_pat(const uint8_t* b, int n, std::vector<PsiProgram>* out) {
    out->clear();
    PsiPatHeader h = {-1, -1, 0};
    if (n < PSI.min_long_section) { h.malformed = 1; return h; }
    h.transport_stream_id = b[PSI.ext_at] << 8 | b[PSI.ext_at + 1]; h.version = (b[PSI.version_at] >> 1) & 31;
    const int end = n - PSI.crc_bytes;
    if ((end - PSI.pat_loop_at) % PSI.pat_stride) { h.malformed = 1; return h; }
    for (int i = PSI.pat_loop_at; i + PSI.pat_stride <= end; i += PSI.pat_stride)
        out->push_back({(uint16_t)(b[i] << 8 | b[i + 1]), (uint16_t)((b[i + 2] & 0x1f) << 8 | b[i + 3])});
    return h;
}
inline PsiPmtHeader psi_parse_pmt(const uint8_t* b, int n, std::vector<PsiEs>* out) {
    out->clear();
    PsiPmtHeader h = {-1, -1, -1, 0};
    if (n < PSI.pmt_loop_at + PSI.crc_bytes) { h.malformed = 1; return h; }
    h.program_number = b[PSI.ext_at] << 8 | b[PSI.ext_at + 1]; h.version = (b[PSI.version_at] >> 1) & 31;
    h.pcr_pid = (b[PSI.pmt_pcr_at] & 0x1f) << 8 | b[PSI.pmt_pcr_at + 1];
    const int end = n - PSI.crc_bytes;
    int i = PSI.pmt_loop_at + ((b[PSI.pmt_info_length_at] & 0x0f) << 8 | b[PSI.pmt_info_length_at + 1]);
    while (i < end) {
        if (i + PSI.pmt_stride > end) break;
        const PsiEs e = {b[i], (uint16_t)((b[i + 1] & 0x1f) << 8 | b[i + 2])};
        i += PSI.pmt_stride + ((b[i + 3] & 0x0f) << 8 | b[i + 4]);
        if (i > end) break;
        out->push_back(e);
    }
    if (i != end) { out->clear(); h.malformed = 1; }
    return h;
}

// ------------------------------------------------------------------------------------------------- the sequential definition
struct PsiSlot {
    uint8_t cont = 0, has_last = 0;                        // tsmon_step's byte; there has been a valid section
    int fill = 0;                                          // bytes buffered; 0: no section is open
    uint32_t last4 = 0;                                    // psi_last4 of the last valid section
    int first_packet = -1;                                 // of the open section, in this call
    uint8_t buf[PSI_BUF];
};

struct PsiHostStream {
    PsiWatch watch[PSI_SLOTS];
    int deliver = 0;
    std::vector<PsiSlot> slot = std::vector<PsiSlot>(PSI_SLOTS);
    std::vector<uint8_t> view[PSI_SLOTS];                  // the slot's last valid changed current PAT / PMT section
    // of the last call
    std::vector<PsiRow> rows;
    std::vector<uint8_t> bytes;
    PsiCnt cnt[PSI_SLOTS];
    bool view_new[PSI_SLOTS];

    PsiHostStream() {
        for (auto& w : watch) w = {-1, -1};
        watch[0] = {0, 0};
    }
    void clear_slot(int s) { slot[s] = PsiSlot(); view[s].clear(); }

    void drop(int s) {
        if (slot[s].fill > 0) ++cnt[s].dropped_sections;
        slot[s].fill = 0;
    }
    void emit(int s, bool want_bytes) {
        PsiSlot& sl = slot[s];
        const uint8_t* b = sl.buf;
        const int total = sl.fill;
        if ((b[1] >> 7) && total < PSI.min_long_section) { ++cnt[s].malformed_sections; return; }
        ++cnt[s].sections;
        if (watch[s].expect >= 0 && b[0] != watch[s].expect) ++cnt[s].unexpected_table_id;
        const bool valid = !(b[1] >> 7) || ts_crc32(b, total) == 0;
        PsiRow r = psi_row_fields([&](int i) { return (unsigned)b[i]; }, total, watch[s].pid, valid, sl.first_packet);
        if (!valid) ++cnt[s].crc_errors;
        else {
            ++cnt[s].valid;
            const uint32_t l4 = psi_last4(b, total);
            if (!sl.has_last || l4 != sl.last4) { r.flags |= PSI_CHANGED; ++cnt[s].changed; }
            sl.has_last = 1; sl.last4 = l4;
        }
        if (psi_is_view(r)) { view[s].assign(b, b + total); view_new[s] = true; }
        if (want_bytes && (deliver == 0 || (r.flags & PSI_CHANGED))) {
            r.offset = (int32_t)bytes.size();
            bytes.insert(bytes.end(), b, b + total);
            cnt[s].bytes_delivered += total;
        }
        rows.push_back(r);
    }
    enum { OPEN = 0, DONE = 1, BAD_LENGTH = 2 };
    // n bytes for the slot's section (open, or starting with them): stops behind the section's last byte
    int feed(int s, const uint8_t* b, int n, int* used, bool want_bytes) {
        PsiSlot& sl = slot[s];
        int i = 0, st = OPEN;
        while (i < n) {
            if (sl.fill < PSI.header_bytes) {
                sl.buf[sl.fill++] = b[i++];
                if (sl.fill < PSI.header_bytes) continue;
                if (psi_section_length(sl.buf[1], sl.buf[2]) > PSI.max_section_length) {
                    ++cnt[s].malformed_sections; sl.fill = 0; st = BAD_LENGTH;
                    break;
                }
            } else {
                const int total = PSI.header_bytes + psi_section_length(sl.buf[1], sl.buf[2]);
                const int take = n - i < total - sl.fill ? n - i : total - sl.fill;
                memcpy(sl.buf + sl.fill, b + i, (size_t)take);
                sl.fill += take; i += take;
            }
            if (sl.fill == PSI.header_bytes + psi_section_length(sl.buf[1], sl.buf[2])) {
                emit(s, want_bytes); sl.fill = 0; st = DONE;
                break;
            }
        }
        *used = i;
        return st;
    }
    // what the shared packet loop asks of a format (ts_reasm_rules.h)
    struct Format {
        PsiHostStream& h;
        int slot_of(int pid) const { int s = 0; while (s < PSI_SLOTS && h.watch[s].pid != pid) ++s; return s < PSI_SLOTS ? s : -1; }
        PsiSlot& state(int s) { return h.slot[s]; }
        PsiCnt& cnt(int s) { return h.cnt[s]; }
        void drop(int s) { h.drop(s); }
        bool feed(int s, const uint8_t* b, int n, int* used, int, bool want_bytes) { return h.feed(s, b, n, used, want_bytes) == DONE; }
        void begin(int s, int k) { h.slot[s].first_packet = k; }
        void slack(int) {}
        bool stuffing(uint8_t b) const { return b == 0xFF; }
    };
    // one call: n packets.  The caller keeps a copy of `slot` and `view` if the call may have to be undone.
    void run(const uint8_t* ts, int n, bool want_bytes) {
        rows.clear(); bytes.clear();
        for (int s = 0; s < PSI_SLOTS; ++s) { cnt[s] = PsiCnt{}; view_new[s] = false; slot[s].first_packet = -1; }
        ts_reasm_run(Format{*this}, ts, n, want_bytes);
    }
};

}  // namespace s2
