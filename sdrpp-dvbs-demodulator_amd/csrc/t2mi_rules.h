// The rules of the T2-MI bank (own extension; include/dvbs2gpu.h), each stated once and shared by the kernels
// (t2mi.hip), the native host bank (T2miHostStream below, behind dvbs2gpu_t2mi_create_host) and a plain C++ test program: the T2-MI
// packet layout as one struct (T2miLayout), what an emitted packet's row says and the packet-count rule.  What a TS packet of a slot's
// PID does to the slot is the datagram banks' sequential stream (dgram_rules.h, shared with mpe_rules.h and ule_rules.h) with T2miRules.
//
// The sequential form -- T2miHostStream::run, packet by packet -- IS the definition; every other form must give its results for every
// cutting of a stream into calls.  The packet syntax is written from memory of ETSI TS 102 773: every offset and limit the code relies
// on is a field of T2miLayout, reported through dvbs2gpu_t2mi_get_layout and compared with the tests' model.
// Standard headers only: the host tests compile this file with a plain C++ compiler.
#pragma once
#include "dgram_rules.h"

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

// the packet-count rule on what a slot carries from packet to packet -- own[0]: there has been a valid packet, own[1]: its packet_count:
// a valid packet whose count is not the last one's plus one has COUNT_ERROR, and steps the pair
enum { T2S_HAS_COUNT = 0, T2S_LAST_COUNT = 1 };
TS_HD inline void t2mi_sequence(T2miRow& r, uint8_t* own) {
    if (r.flags & T2MI_CRC_ERROR) return;
    if (own[T2S_HAS_COUNT] && r.packet_count != ((own[T2S_LAST_COUNT] + 1) & 255)) r.flags |= T2MI_COUNT_ERROR;
    own[T2S_HAS_COUNT] = 1; own[T2S_LAST_COUNT] = r.packet_count;
}
// the counters that a row steps, but for the delivery's: add(index into T2miCnt)
enum { T2C_PACKETS = 0, T2C_T2MI, T2C_CRC, T2C_COUNT, T2C_BB, T2C_BADPAY, T2C_DELIVERED, T2C_BYTES, T2C_DROPPED, T2C_MALPKT, T2C_SCR, T2C_SLACK };
template <typename Add>
TS_HD inline void t2mi_account(unsigned flags, Add add) {
    add(T2C_T2MI);
    if (flags & T2MI_CRC_ERROR) add(T2C_CRC);
    if (flags & T2MI_COUNT_ERROR) add(T2C_COUNT);
    if (flags & T2MI_BBFRAME) add(T2C_BB);
    if (flags & T2MI_BAD_PAYLOAD) add(T2C_BADPAY);
}

// ------------------------------------------------------------------------------------------------- what the shared code asks of the bank
// (dgram_rules.h: the sequential stream; dgram_bank.h: the kernels and the handle)
struct T2miRules {
    typedef T2miRow Row; typedef T2miWatch Watch; typedef T2miCnt Cnt;
    static constexpr T2miWatch NO_WATCH = {-1, -1};
    static constexpr int SLOTS = T2MI_SLOTS, BUF = T2MI_BUF, NCNT = T2MI_NCNT;
    // a 6-byte header with payload_bits in bytes 4 and 5; no stuffing and no bad length; what a PUSI packet's pointer bytes hold beyond
    // the open packet's end is counted
    static constexpr int HEADER = T2MI.header_bytes, LEN_A = 4, LEN_B = 5, STUFFING = -1;
    static constexpr int C_PACKETS = T2C_PACKETS, C_SCR = T2C_SCR, C_MALPKT = T2C_MALPKT, C_DELIVERED = T2C_DELIVERED, C_BYTES = T2C_BYTES;
    static constexpr int C_DROPPED = T2C_DROPPED, C_BAD_UNIT = -1, C_SLACK = T2C_SLACK;
    static constexpr auto total = &t2mi_total;
    static constexpr auto sequence = &t2mi_sequence;
    TS_HD static bool takes_crc(unsigned, unsigned, int) { return true; }      // there is no unchecked packet
    template <typename Src> TS_HD static T2miRow row_fields(const Src& s, int total, bool crc_ok, const T2miWatch&, int first_packet, int last_packet) {
        return t2mi_row_fields([&](int i) { return s.rd(i); }, total, crc_ok, first_packet, last_packet);
    }
    template <typename Add> TS_HD static void account(unsigned flags, Add add) { t2mi_account(flags, add); }
    // the BBFRAME of a row lies behind the packet's header and the BBFRAME prefix
    TS_HD static bool delivers(const T2miRow& r, const T2miWatch& w) { return t2mi_delivers(r, w.plp); }
    TS_HD static int bytes_of(const T2miRow& r) { return r.bbframe_bytes; }
    TS_HD static int ip_at(const T2miRow&) { return T2MI.header_bytes + T2MI.bbframe_prefix_bytes; }
};
// the sequential definition: one slot of one stream
typedef DgramHostStream<T2miRules> T2miHostStream;

}  // namespace s2
