// The rules of the ULE bank (own extension; include/dvbs2gpu.h), each stated once and shared by the kernels
// (ule.hip), the native host bank (UleHostStream, behind dvbs2gpu_ule_create_host) and a plain C++ test program: the layout of a
// ULE SNDU (Unidirectional Lightweight Encapsulation), of its extension headers and of a bridged frame as one struct (UleLayout), what
// a TS packet of a slot's PID does to the slot, and what an emitted SNDU's row says.  The IP header rules behind them are ip_rules.h,
// shared with the MPE bank.
//
// The sequential form -- UleHostStream::run, which is DgramHostStream (dgram_rules.h) with these rules -- IS the definition; every other form must give
// its results for every cutting of a stream into calls.  The syntax is written from memory of RFC 4326 and RFC 5163 and is pinned to
// no test vector of theirs: every offset and limit the code relies on is a field of UleLayout, reported through dvbs2gpu_ule_get_layout
// and compared with the tests' model.
// Departures from RFC 4326, all of them the shared packet rules' (ts_reasm_rules.h): a payload pointer that reaches BEYOND the end of
// the open SNDU emits the SNDU and counts `slack` where the RFC discards it and waits for the next PUSI; a TS packet without PUSI
// ignores what is left of its payload behind the open SNDU's end (the RFC requires PUSI in a packet in which an SNDU starts, so nothing
// legal is lost); SNDUs above 4096 bytes are the bad length.
// Standard headers, ip_rules.h, dgram_rules.h and ts_reasm_rules.h only: the host tests compile this file with a plain C++ compiler.
#pragma once
#include "dgram_rules.h"
#include "ip_rules.h"

namespace s2 {

struct UleLayout {                     // the layout of dvbs2gpu_ule_layout (ule.hip asserts it)
    int32_t header_bytes;              // D and the 15-bit Length, then the 16-bit Type: 4
    int32_t length_bytes;              // the bytes that carry the Length, the first two: 2
    int32_t d_bit;                     // of byte 0, "destination address absent": 0x80
    int32_t length_mask;               // of (b0 << 8 | b1): 0x7FFF
    int32_t max_length;                // 4092: an SNDU is Length + 4 bytes and at most 4096
    int32_t max_sndu_bytes;            // 4096
    int32_t type_at;                   // 2
    int32_t npa_bytes;                 // the destination address behind Type when D = 0: 6
    int32_t crc_bytes;                 // CRC-32 over the whole SNDU: 4
    int32_t min_length_d1, min_length_d0;                  // 4 (the CRC), 10 (NPA and CRC)
    int32_t type_test, type_bridged, type_ts_concat, type_priv_concat;   // 0, 1, 2, 3
    int32_t ethertype_floor;           // 1536: a Type from here on is an EtherType, one below an extension header
    int32_t hlen_shift, hlen_mask;     // H-LEN = Type >> 8 & 7; 0: a mandatory header, 1..5: an optional one of 2 H-LEN bytes
    int32_t max_hlen;                  // 5
    int32_t max_extension_bytes;       // of optional headers that are followed, in all: 40
    int32_t mac_header_bytes;          // of a bridged frame -- destination, source, EtherType: 14
    int32_t bridged_ethertype_at;      // 12
    int32_t ethertype_ipv4, ethertype_ipv6;
    int32_t ipv4_min_header, ipv4_total_length_at, ipv4_fragment_at, ipv4_protocol_at, ipv4_src_at, ipv4_dst_at;
    int32_t ipv6_header, ipv6_payload_length_at, ipv6_next_header_at;
    int32_t head_bytes;                // a row is decided from the first 4 + 6 + 40 + 14 + 60 + 4 = 128 bytes of its SNDU at most
};
constexpr UleLayout ULE = {4, 2, 0x80, 0x7FFF, 4092, 4096, 2, 6, 4, 4, 10, 0, 1, 2, 3, 1536, 8, 7, 5, 40, 14, 12, IP.ethertype_ipv4, IP.ethertype_ipv6,
                           IP.ipv4_min_header, IP.ipv4_total_length_at, IP.ipv4_fragment_at, IP.ipv4_protocol_at, IP.ipv4_src_at, IP.ipv4_dst_at, IP.ipv6_header,
                           IP.ipv6_payload_length_at, IP.ipv6_next_header_at, 128};
static_assert(ULE.head_bytes == ULE.header_bytes + ULE.npa_bytes + ULE.max_extension_bytes + ULE.mac_header_bytes + IP_HEAD_BYTES, "what a row reads at most");
static_assert((ULE.max_hlen << ULE.hlen_shift | 0xFF) < ULE.ethertype_floor && ((ULE.max_hlen + 1) << ULE.hlen_shift) >= ULE.ethertype_floor, "H-LEN of a Type below 1536 is 0..5");

constexpr int ULE_SLOTS = 4, ULE_BUF = 4096;
// row flags (DVBS2GPU_ULE_*); NO_ADDRESS and BRIDGED are information, the others end the rule list
constexpr int ULE_MALFORMED = 1, ULE_CRC_ERROR = 2, ULE_FILTERED = 4, ULE_NO_ADDRESS = 8, ULE_TEST = 16, ULE_BRIDGED = 32, ULE_EXTENSION = 64, ULE_OTHER_PROTOCOL = 128,
              ULE_BAD_IP = 256, ULE_DATAGRAM = 512;

// pid -1: the slot is empty; an all-zero mask: every address; accept_unaddressed: SNDUs with D = 1 pass the filter
struct UleWatch { int32_t pid; uint8_t npa_value[6], npa_mask[6]; int32_t accept_unaddressed; };
// the counters one call adds to a slot's statistics (dvbs2gpu_ule_stats, as 32-bit shares)
struct UleCnt { int32_t packets, sndus, crc_errors, filtered, no_address, test, bridged, extension, other_protocol, bad_ip, datagrams, datagrams_delivered,
                        bytes_delivered, dropped_sndus, malformed_sndus, slack, malformed_packets, scrambled_packets; };
constexpr int ULE_NCNT = 18;
enum { ULC_PACKETS = 0, ULC_SNDUS, ULC_CRC, ULC_FILTERED, ULC_NO_ADDRESS, ULC_TEST, ULC_BRIDGED, ULC_EXTENSION, ULC_OTHER_PROTOCOL, ULC_BAD_IP, ULC_DATAGRAMS,
       ULC_DELIVERED, ULC_BYTES, ULC_DROPPED, ULC_MALSNDU, ULC_SLACK, ULC_MALPKT, ULC_SCR };
// one emitted SNDU; the layout of dvbs2gpu_ule_row
struct UleRow {
    uint16_t flags;
    uint8_t family, protocol;
    uint8_t mac[6];
    uint8_t ip_at, extension_bytes;
    uint16_t src_port, dst_port;
    uint32_t src4, dst4;
    int32_t length, offset, bytes, first_packet, last_packet;
    uint16_t ethertype, stuffing;
};

// an SNDU's bytes from its first two; -1: Length is beyond 4092, the bad length (so 0xFF never is a legal first byte)
TS_HD inline int ule_total(unsigned b0, unsigned b1) {
    const int n = (int)((b0 << 8 | b1) & (unsigned)ULE.length_mask);
    return n > ULE.max_length ? -1 : ULE.header_bytes + n;
}

// The row of an emitted SNDU.  s: its leading bytes and the reductions the rules take over them, as in mpe_row_fields --  s.rd(i): byte
// i, asked for i < total only;  s.any(n, f);  s.sum(n, f); n <= 64.  crc_ok: the CRC-32 over the SNDU is 0.  The offset is the caller's.
// The extension-header walk is data dependent but reads through s.rd alone: a wave in which every lane holds the same source walks it
// without diverging.
template <typename Src>
TS_HD inline UleRow ule_row_fields(const Src& s, int total, bool crc_ok, const UleWatch& w, int first_packet, int last_packet) {
    UleRow r = {};
    r.length = total; r.offset = -1; r.first_packet = first_packet; r.last_packet = last_packet;
    const bool d = (s.rd(0) & (unsigned)ULE.d_bit) != 0;
    if (total - ULE.header_bytes < (d ? ULE.min_length_d1 : ULE.min_length_d0)) { r.flags = ULE_MALFORMED; return r; }
    if (!crc_ok) { r.flags = ULE_CRC_ERROR; return r; }
    int at = ULE.header_bytes;
    const int end = total - ULE.crc_bytes;                 // the body is [at, end)
    if (d) {
        r.flags = ULE_NO_ADDRESS;
        if (!w.accept_unaddressed) { r.flags |= ULE_FILTERED; return r; }
    } else {
        for (int k = 0; k < 6; ++k) r.mac[k] = (uint8_t)s.rd(at + k);
        if (s.any(6, [&](int k) { return ((s.rd(ULE.header_bytes + k) ^ w.npa_value[k]) & w.npa_mask[k]) != 0; })) { r.flags |= ULE_FILTERED; return r; }
        at += ULE.npa_bytes;
    }
    unsigned type = s.rd(ULE.type_at) << 8 | s.rd(ULE.type_at + 1);
    // optional extension headers: 2 H-LEN bytes each, the last two the next Type
    int ext = 0;
    while ((int)type < ULE.ethertype_floor && (type >> ULE.hlen_shift & (unsigned)ULE.hlen_mask) != 0) {
        const int n = 2 * (int)(type >> ULE.hlen_shift & (unsigned)ULE.hlen_mask);
        ext += n;
        if (ext > ULE.max_extension_bytes || at + n > end) { r.flags |= ULE_EXTENSION; r.ethertype = (uint16_t)type; return r; }
        at += n;
        type = s.rd(at - 2) << 8 | s.rd(at - 1);
    }
    r.extension_bytes = (uint8_t)ext;
    if ((int)type < ULE.ethertype_floor) {                 // a mandatory extension header
        if ((int)type == ULE.type_test) { r.flags |= ULE_TEST; return r; }
        if ((int)type != ULE.type_bridged || end - at < ULE.mac_header_bytes) { r.flags |= ULE_EXTENSION; r.ethertype = (uint16_t)type; return r; }
        r.flags |= ULE_BRIDGED;
        if (d) for (int k = 0; k < 6; ++k) r.mac[k] = (uint8_t)s.rd(at + k);
        type = s.rd(at + ULE.bridged_ethertype_at) << 8 | s.rd(at + ULE.bridged_ethertype_at + 1);
        at += ULE.mac_header_bytes;
    }
    r.ethertype = (uint16_t)type;
    // (an EtherType field below 1536 in a bridged frame is an LLC length: another protocol)
    const int family = type == (unsigned)ULE.ethertype_ipv4 ? 4 : type == (unsigned)ULE.ethertype_ipv6 ? 6 : 0;
    const int ip = ip_row_fields(s, at, end, family, r);
    r.flags |= ip == IP_IS_DATAGRAM ? ULE_DATAGRAM : ip == IP_IS_BAD ? ULE_BAD_IP : ULE_OTHER_PROTOCOL;
    if (ip == IP_IS_DATAGRAM) r.ip_at = (uint8_t)at;
    return r;
}
// where the datagram of a DATAGRAM row starts in its SNDU: behind the base header, the NPA, the optional headers and a bridged MAC header
TS_HD inline int ule_ip_at(const UleRow& r) { return r.ip_at; }
// the counters that a row steps, but for the delivery's: add(index into UleCnt)
template <typename Add>
TS_HD inline void ule_account(unsigned flags, Add add) {
    add(ULC_SNDUS);
    constexpr int of_flag[10] = {ULC_MALSNDU, ULC_CRC, ULC_FILTERED, ULC_NO_ADDRESS, ULC_TEST, ULC_BRIDGED, ULC_EXTENSION, ULC_OTHER_PROTOCOL, ULC_BAD_IP, ULC_DATAGRAMS};
    for (int k = 0; k < 10; ++k) if (flags >> k & 1) add(of_flag[k]);
}

// ------------------------------------------------------------------------------------------------- what the shared code asks of the bank
// (dgram_rules.h: the sequential stream; dgram_bank.h: the kernels and the handle)
struct UleRules {
    typedef UleRow Row; typedef UleWatch Watch; typedef UleCnt Cnt;
    static constexpr UleWatch NO_WATCH = {-1, {0, 0, 0, 0, 0, 0}, {0, 0, 0, 0, 0, 0}, 0};
    static constexpr int SLOTS = ULE_SLOTS, BUF = ULE_BUF, NCNT = ULE_NCNT;
    // the length is known from the first two bytes (D and the 15-bit Length), a Length beyond 4092 is bad; 0xFF in an SNDU's first place
    // is the End Indicator or padding
    static constexpr int HEADER = ULE.length_bytes, LEN_A = 0, LEN_B = 1, STUFFING = 0xFF;
    static constexpr int C_PACKETS = ULC_PACKETS, C_SCR = ULC_SCR, C_MALPKT = ULC_MALPKT, C_DELIVERED = ULC_DELIVERED, C_BYTES = ULC_BYTES;
    static constexpr int C_DROPPED = ULC_DROPPED, C_BAD_UNIT = ULC_MALSNDU, C_SLACK = ULC_SLACK;
    // the rules above under the names the shared code calls them by: constant function pointers, not forwarding members (a row returned through one
    // more call level costs the scan kernel registers: profiles/ts_reasm_resources.txt)
    static constexpr auto total = &ule_total;
    static constexpr auto ip_at = &ule_ip_at;
    template <typename Src> static constexpr auto row_fields = &ule_row_fields<Src>;
    template <typename Add> TS_HD static void account(unsigned flags, Add add) { ule_account(flags, add); }
    TS_HD static bool takes_crc(unsigned, unsigned, int) { return true; }      // there is no unchecked SNDU
    // nothing is carried from SNDU to SNDU; a DATAGRAM row's datagram is delivered
    TS_HD static void sequence(UleRow&, uint8_t*) {}
    TS_HD static bool delivers(const UleRow& r, const UleWatch&) { return r.flags & ULE_DATAGRAM; }
    TS_HD static int bytes_of(const UleRow& r) { return r.bytes; }
};
// the sequential definition: one slot of one stream
typedef DgramHostStream<UleRules> UleHostStream;

}  // namespace s2
