// The rules of the T2-MI bank (own extension; include/dvbs2gpu.h), each stated once and shared by the kernels
// (t2mi.hip), the native host bank (T2miHostStream below, behind dvbs2gpu_t2mi_create_host) and a plain C++ test program: the T2-MI
// packet layout as one struct (T2miLayout), what a TS packet of a slot's PID does to the slot, and what an emitted packet's row says.
//
// The sequential form -- T2miHostStream::run, packet by packet -- IS the definition; every other form must give its results for every
// cutting of a stream into calls.  The packet syntax is written from memory of ETSI TS 102 773: every offset and limit the code relies
// on is a field of T2miLayout, reported through dvbs2gpu_t2mi_get_layout and compared with the tests' model.
// Standard headers only: the host tests compile this file with a plain C++ compiler.
#pragma once
#include "ts_reasm_rules.h"

#include <cstring>
#include <vector>

namespace s2 {

struct T2miLayout {                    // the layout of dvbs2gpu_t2mi_layout (t2mi.hip asserts it)
    int32_t header_bytes;              // packet_type, packet_count, superframe_idx 4 | rfu, rfu 5 | t2mi_stream_id 3, payload_bits 16: 6
    int32_t crc_bytes;                 // 4
    int32_t min_packet_bytes;          // 10
    int32_t max_packet_bytes;          // 6 + 8192 + 4 = 8202
    int32_t bbframe_type;              // packet_type 0x00
    int32_t bbframe_prefix_bytes;      // frame_idx, plp_id, intl_frame_start 1 | rfu 7: 3
    int32_t min_bbframe_bytes;         // a BBHEADER: 10
    int32_t max_bbframe_bytes;         // Kbch 58 192 bits: 7274
    int32_t stream_id_mask;            // of b3: 7
};
constexpr T2miLayout T2MI = {6, 4, 10, 8202, 0, 3, 10, 7274, 7};

constexpr int T2MI_SLOTS = 4, T2MI_BUF = 8208;
// row flags (DVBS2GPU_T2MI_*)
constexpr int T2MI_CRC_ERROR = 1, T2MI_COUNT_ERROR = 2, T2MI_BBFRAME = 4, T2MI_INTL_FRAME_START = 8, T2MI_BAD_PAYLOAD = 16;

struct T2miWatch { int32_t pid, plp; };                    // pid -1: the slot is empty; plp -1: every PLP
// the counters one call adds to a slot's statistics (dvbs2gpu_t2mi_stats, as 32-bit shares)
struct T2miCnt { int32_t packets, t2mi_packets, crc_errors, count_errors, bbframes, bad_payload, bbframes_delivered, bytes_delivered, dropped_packets,
                         malformed_packets, scrambled_packets, pointer_slack; };
constexpr int T2MI_NCNT = 12;
// one emitted T2-MI packet; the layout of dvbs2gpu_t2mi_row
struct T2miRow {
    uint8_t packet_type, packet_count, superframe_idx, stream_id;
    uint16_t flags;
    uint8_t plp_id, frame_idx;
    uint32_t payload_bits;
    int32_t length, offset, bbframe_bytes, first_packet, last_packet;
};

// a T2-MI packet's bytes from the fifth and sixth header byte: header, payload with its pad bits, CRC
TS_HD inline int t2mi_total(unsigned b4, unsigned b5) { return T2MI.header_bytes + (int)(((b4 << 8 | b5) + 7) >> 3) + T2MI.crc_bytes; }
// ts_payload_start under the name that the stand-alone test program of these rules calls
inline int t2mi_payload_start(int afc, unsigned b4) { return ts_payload_start(afc, b4); }
// the row of an emitted packet from its first nine bytes (total >= 10); rd(i): byte i.  COUNT_ERROR and the offset are the caller's.
template <typename Rd>
TS_HD inline T2miRow t2mi_row_fields(Rd rd, int total, bool valid, int first_packet, int last_packet) {
    T2miRow r = {(uint8_t)rd(0), (uint8_t)rd(1), (uint8_t)(rd(2) >> 4), (uint8_t)(rd(3) & (unsigned)T2MI.stream_id_mask), (uint16_t)(valid ? 0 : T2MI_CRC_ERROR), 0, 0,
                 (uint32_t)(rd(4) << 8 | rd(5)), total, -1, 0, first_packet, last_packet};
    if (!valid || r.packet_type != T2MI.bbframe_type) return r;
    const int bits = (int)r.payload_bits, prefix = 8 * T2MI.bbframe_prefix_bytes;
    if (bits >= prefix) { r.frame_idx = (uint8_t)rd(6); r.plp_id = (uint8_t)rd(7); }
    if (bits < prefix + 8 * T2MI.min_bbframe_bytes || (bits - prefix) % 8 || (bits - prefix) / 8 > T2MI.max_bbframe_bytes) { r.flags |= T2MI_BAD_PAYLOAD; return r; }
    r.flags |= T2MI_BBFRAME | ((rd(8) >> 7) ? T2MI_INTL_FRAME_START : 0);
    r.bbframe_bytes = (bits - prefix) / 8;
    return r;
}
// does the slot deliver the BBFRAME of this row
TS_HD inline bool t2mi_delivers(const T2miRow& r, int plp) { return (r.flags & T2MI_BBFRAME) && (plp < 0 || plp == r.plp_id); }

// ------------------------------------------------------------------------------------------------- the sequential definition
struct T2miState {
    uint8_t cont = 0, has_count = 0, last_count = 0;       // tsmon_step's byte; there has been a valid packet; its packet_count
    int fill = 0;                                          // bytes buffered; 0: no packet is open
    uint8_t buf[T2MI_BUF];
};

// one slot of one stream: a complete reassembler
struct T2miHostStream {
    T2miWatch watch = {-1, -1};
    T2miState st;
    int first_packet = -1;                                 // of the open packet, in this call
    // of the last call
    std::vector<T2miRow> rows;
    std::vector<uint8_t> bytes;
    T2miCnt cnt = {};

    void clear() { st = T2miState(); rows.clear(); bytes.clear(); }

    void drop() {
        if (st.fill > 0) ++cnt.dropped_packets;
        st.fill = 0;
    }
    void emit(int k, bool want_bytes) {
        const uint8_t* b = st.buf;
        const int total = st.fill;
        ++cnt.t2mi_packets;
        const bool valid = ts_crc32(b, total) == 0;
        T2miRow r = t2mi_row_fields([&](int i) { return (unsigned)b[i]; }, total, valid, first_packet, k);
        if (!valid) ++cnt.crc_errors;
        else {
            if (st.has_count && r.packet_count != ((st.last_count + 1) & 255)) { r.flags |= T2MI_COUNT_ERROR; ++cnt.count_errors; }
            st.has_count = 1; st.last_count = r.packet_count;
            if (r.flags & T2MI_BAD_PAYLOAD) ++cnt.bad_payload;
            if (r.flags & T2MI_BBFRAME) ++cnt.bbframes;
            if (want_bytes && t2mi_delivers(r, watch.plp)) {
                const uint8_t* f = b + T2MI.header_bytes + T2MI.bbframe_prefix_bytes;
                r.offset = (int32_t)bytes.size();
                bytes.insert(bytes.end(), f, f + r.bbframe_bytes);
                ++cnt.bbframes_delivered; cnt.bytes_delivered += r.bbframe_bytes;
            }
        }
        rows.push_back(r);
    }
    // n bytes for the slot's packet (open, or starting with them): stops behind the packet's last byte.  true: it was emitted
    bool feed(const uint8_t* b, int n, int* used, int k, bool want_bytes) {
        int i = 0;
        bool done = false;
        while (i < n) {
            if (st.fill < T2MI.header_bytes) { st.buf[st.fill++] = b[i++]; continue; }
            const int total = t2mi_total(st.buf[4], st.buf[5]);
            const int take = n - i < total - st.fill ? n - i : total - st.fill;
            memcpy(st.buf + st.fill, b + i, (size_t)take);
            st.fill += take; i += take;
            if (st.fill == total) { emit(k, want_bytes); st.fill = 0; done = true; break; }
        }
        *used = i;
        return done;
    }
    // what the shared packet loop asks of a format (ts_reasm_rules.h): one slot, no stuffing, the pointer slack counted
    struct Format {
        T2miHostStream& h;
        int slot_of(int pid) const { return pid == h.watch.pid ? 0 : -1; }
        T2miState& state(int) { return h.st; }
        T2miCnt& cnt(int) { return h.cnt; }
        void drop(int) { h.drop(); }
        bool feed(int, const uint8_t* b, int n, int* used, int k, bool want_bytes) { return h.feed(b, n, used, k, want_bytes); }
        void begin(int, int k) { h.first_packet = k; }
        void slack(int) { ++h.cnt.pointer_slack; }
        bool stuffing(uint8_t) const { return false; }
    };
    // one call: n packets.  The caller keeps a copy of `st` if the call may have to be undone.
    void run(const uint8_t* ts, int n, bool want_bytes) {
        rows.clear(); bytes.clear();
        cnt = T2miCnt{};
        first_packet = -1;
        if (watch.pid >= 0) ts_reasm_run(Format{*this}, ts, n, want_bytes);
    }
};

}  // namespace s2
