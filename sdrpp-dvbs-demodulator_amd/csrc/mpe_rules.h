// The rules of the MPE bank (own extension; include/dvbs2gpu.h), each stated once and shared by the kernels
// (mpe.hip), the native host bank (MpeHostStream, behind dvbs2gpu_mpe_create_host) and a plain C++ test program: the layout of a
// DSM-CC datagram_section and of the IP headers behind it as one struct (MpeLayout), what a TS packet of a slot's PID does to the slot,
// and what an emitted section's row says.  The IP header rules behind the MPE header are ip_rules.h, shared with the ULE bank.
//
// The sequential form -- MpeHostStream::run, which is DgramHostStream (dgram_rules.h) with these rules -- IS the definition; every other form must give
// its results for every cutting of a stream into calls.  The syntax is written from memory of ETSI EN 301 192 (section 7), RFC 791,
// RFC 8200 and RFC 1042: every offset and limit the code relies on is a field of MpeLayout, reported through dvbs2gpu_mpe_get_layout
// and compared with the tests' model.
// Standard headers, ip_rules.h, dgram_rules.h and ts_reasm_rules.h only: the host tests compile this file with a plain C++ compiler.
#pragma once
#include "dgram_rules.h"
#include "ip_rules.h"

namespace s2 {

struct MpeLayout {                     // the layout of dvbs2gpu_mpe_layout (mpe.hip asserts it)
    int32_t header_bytes;              // table_id, then 4 flag bits and the 12-bit section_length: 3
    int32_t length_mask;               // of (b1 << 8 | b2): 0x0FFF
    int32_t max_section_length;        // 4093: a section is at most 4096 bytes
    int32_t max_section_bytes;         // 4096
    int32_t table_id;                  // datagram_section: 0x3E
    int32_t mpe_header_bytes;          // up to and with last_section_number: 12
    int32_t crc_bytes;                 // CRC-32 or checksum: 4
    int32_t min_section_bytes;         // 16
    int32_t mac_at[6];                 // MAC_address_1 .. MAC_address_6 (network order): 11, 10, 9, 8, 4, 3
    int32_t flags_at;                  // 2 reserved, payload_scrambling 2, address_scrambling 2, LLC_SNAP_flag, current_next: 5
    int32_t section_number_at, last_section_number_at;     // 6, 7
    int32_t llc_snap_bytes;            // AA AA 03 00 00 00 and the EtherType: 8
    int32_t ethertype_at;              // in the LLC/SNAP header: 6
    int32_t ethertype_ipv4, ethertype_ipv6;                // 0x0800, 0x86DD
    int32_t ipv4_min_header;           // 20
    int32_t ipv4_total_length_at, ipv4_fragment_at, ipv4_protocol_at, ipv4_src_at, ipv4_dst_at;   // 2, 6, 9, 12, 16
    int32_t ipv6_header;               // 40
    int32_t ipv6_payload_length_at, ipv6_next_header_at;   // 4, 6
    int32_t head_bytes;                // a row is decided from the first 12 + 8 + 60 + 4 = 84 bytes of its section at most
};
constexpr MpeLayout MPE = {3, 0x0FFF, 4093, 4096, 0x3E, 12, 4, 16, {11, 10, 9, 8, 4, 3}, 5, 6, 7, 8, 6, IP.ethertype_ipv4, IP.ethertype_ipv6, IP.ipv4_min_header,
                           IP.ipv4_total_length_at, IP.ipv4_fragment_at, IP.ipv4_protocol_at, IP.ipv4_src_at, IP.ipv4_dst_at, IP.ipv6_header, IP.ipv6_payload_length_at,
                           IP.ipv6_next_header_at, 84};

constexpr int MPE_SLOTS = 4, MPE_BUF = 4096;
// row flags (DVBS2GPU_MPE_*)
constexpr int MPE_OTHER_TABLE = 1, MPE_MALFORMED = 2, MPE_CRC_ERROR = 4, MPE_UNCHECKED = 8, MPE_SCRAMBLED = 16, MPE_FILTERED = 32, MPE_FRAGMENT = 64,
              MPE_OTHER_PROTOCOL = 128, MPE_BAD_IP = 256, MPE_DATAGRAM = 512;

struct MpeWatch { int32_t pid; uint8_t mac_value[6], mac_mask[6]; };       // pid -1: the slot is empty; an all-zero mask: every address
// the counters one call adds to a slot's statistics (dvbs2gpu_mpe_stats, as 32-bit shares)
struct MpeCnt { int32_t packets, sections, other_table, crc_errors, unchecked, scrambled_sections, filtered, fragments, other_protocol, bad_ip, datagrams,
                        datagrams_delivered, bytes_delivered, dropped_sections, malformed_sections, malformed_packets, scrambled_packets; };
constexpr int MPE_NCNT = 17;
enum { MPC_PACKETS = 0, MPC_SECTIONS, MPC_OTHER_TABLE, MPC_CRC, MPC_UNCHECKED, MPC_SCR_SECTIONS, MPC_FILTERED, MPC_FRAGMENTS, MPC_OTHER_PROTOCOL, MPC_BAD_IP,
       MPC_DATAGRAMS, MPC_DELIVERED, MPC_BYTES, MPC_DROPPED, MPC_MALSEC, MPC_MALPKT, MPC_SCR };
// one emitted section; the layout of dvbs2gpu_mpe_row
struct MpeRow {
    uint16_t flags;
    uint8_t family, protocol;
    uint8_t mac[6];
    uint8_t section_number, last_section_number;
    uint16_t src_port, dst_port;
    uint32_t src4, dst4;
    int32_t length, offset, bytes, first_packet, last_packet;
    uint16_t ethertype, stuffing;
};

// a section's bytes from its second and third byte; -1: section_length is beyond 4093, the bad length
TS_HD inline int mpe_total(unsigned b1, unsigned b2) {
    const int n = (int)((b1 << 8 | b2) & (unsigned)MPE.length_mask);
    return n > MPE.max_section_length ? -1 : MPE.header_bytes + n;
}
// is the CRC-32 of an emitted section taken: not of another table, not of one too short, not with section_syntax_indicator clear
TS_HD inline bool mpe_takes_crc(unsigned b0, unsigned b1, int total) { return (int)b0 == MPE.table_id && total >= MPE.min_section_bytes && (b1 >> 7); }

// The row of an emitted section.  s: its leading bytes and the two reductions the rules take over them, so that a wave can take them
// with a lane per term --  s.rd(i): byte i, asked for i < total only;  s.any(n, f): is f(k) true for a k in [0, n);  s.sum(n, f): the
// sum of f(k) over [0, n); n <= 64.  crc_ok: the CRC-32 over the section is 0 (looked at where mpe_takes_crc).  The offset is the caller's.
template <typename Src>
TS_HD inline MpeRow mpe_row_fields(const Src& s, int total, bool crc_ok, const MpeWatch& w, int first_packet, int last_packet) {
    MpeRow r = {};
    r.length = total; r.offset = -1; r.first_packet = first_packet; r.last_packet = last_packet;
    if ((int)s.rd(0) != MPE.table_id) { r.flags = MPE_OTHER_TABLE; return r; }
    if (total < MPE.min_section_bytes) { r.flags = MPE_MALFORMED; return r; }
    if (!(s.rd(1) >> 7)) r.flags = MPE_UNCHECKED;
    else if (!crc_ok) { r.flags = MPE_CRC_ERROR; return r; }
    for (int k = 0; k < 6; ++k) r.mac[k] = (uint8_t)s.rd(MPE.mac_at[k]);
    const unsigned fl = s.rd(MPE.flags_at);
    r.section_number = (uint8_t)s.rd(MPE.section_number_at); r.last_section_number = (uint8_t)s.rd(MPE.last_section_number_at);
    if ((fl >> 4 & 3) || (fl >> 2 & 3)) { r.flags |= MPE_SCRAMBLED; return r; }
    if (s.any(6, [&](int k) { return ((s.rd(MPE.mac_at[k]) ^ w.mac_value[k]) & w.mac_mask[k]) != 0; })) { r.flags |= MPE_FILTERED; return r; }
    if (r.section_number || r.last_section_number) { r.flags |= MPE_FRAGMENT; return r; }
    int at = MPE.mpe_header_bytes, family;
    const int end = total - MPE.crc_bytes;                 // the body is [at, end)
    if (fl >> 1 & 1) {
        if (end - at < MPE.llc_snap_bytes || s.rd(at) != 0xAA || s.rd(at + 1) != 0xAA || s.rd(at + 2) != 0x03 || s.rd(at + 3) || s.rd(at + 4) || s.rd(at + 5)) {
            r.flags |= MPE_OTHER_PROTOCOL;
            return r;
        }
        r.ethertype = (uint16_t)(s.rd(at + MPE.ethertype_at) << 8 | s.rd(at + MPE.ethertype_at + 1));
        family = r.ethertype == IP.ethertype_ipv4 ? 4 : r.ethertype == IP.ethertype_ipv6 ? 6 : 0;
        at += MPE.llc_snap_bytes;
    } else {
        family = end > at ? (int)(s.rd(at) >> 4) : 0;
    }
    // the IP header behind it: ip_rules.h, shared with the ULE bank
    const int ip = ip_row_fields(s, at, end, family, r);
    r.flags |= ip == IP_IS_DATAGRAM ? MPE_DATAGRAM : ip == IP_IS_BAD ? MPE_BAD_IP : MPE_OTHER_PROTOCOL;
    return r;
}
// where the datagram of a DATAGRAM row starts in its section: behind the MPE header, and behind LLC/SNAP where there was one
TS_HD inline int mpe_ip_at(const MpeRow& r) { return MPE.mpe_header_bytes + (r.ethertype ? MPE.llc_snap_bytes : 0); }
// the counters that a row steps, but for the delivery's: add(index into MpeCnt)
template <typename Add>
TS_HD inline void mpe_account(unsigned flags, Add add) {
    add(MPC_SECTIONS);
    constexpr int of_flag[10] = {MPC_OTHER_TABLE, MPC_MALSEC, MPC_CRC, MPC_UNCHECKED, MPC_SCR_SECTIONS, MPC_FILTERED, MPC_FRAGMENTS, MPC_OTHER_PROTOCOL, MPC_BAD_IP,
                                 MPC_DATAGRAMS};
    for (int k = 0; k < 10; ++k) if (flags >> k & 1) add(of_flag[k]);
}

// ------------------------------------------------------------------------------------------------- what the shared code asks of the bank
// (dgram_rules.h: the sequential stream; dgram_bank.h: the kernels and the handle)
struct MpeRules {
    typedef MpeRow Row; typedef MpeWatch Watch; typedef MpeCnt Cnt;
    static constexpr MpeWatch NO_WATCH = {-1, {0, 0, 0, 0, 0, 0}, {0, 0, 0, 0, 0, 0}};
    static constexpr int SLOTS = MPE_SLOTS, BUF = MPE_BUF, NCNT = MPE_NCNT;
    // a 3-byte header with section_length in bytes 1 and 2, a length beyond 4093 is bad; 0xFF in a section's first place is stuffing
    static constexpr int HEADER = MPE.header_bytes, LEN_A = 1, LEN_B = 2, STUFFING = 0xFF;
    static constexpr int C_PACKETS = MPC_PACKETS, C_SCR = MPC_SCR, C_MALPKT = MPC_MALPKT, C_DELIVERED = MPC_DELIVERED, C_BYTES = MPC_BYTES;
    static constexpr int C_DROPPED = MPC_DROPPED, C_BAD_UNIT = MPC_MALSEC, C_SLACK = -1;
    // the rules above under the names the shared code calls them by: constant function pointers, not forwarding members (a row returned through one
    // more call level costs the scan kernel registers: profiles/ts_reasm_resources.txt)
    static constexpr auto total = &mpe_total;
    static constexpr auto takes_crc = &mpe_takes_crc;
    static constexpr auto ip_at = &mpe_ip_at;
    template <typename Src> static constexpr auto row_fields = &mpe_row_fields<Src>;
    template <typename Add> TS_HD static void account(unsigned flags, Add add) { mpe_account(flags, add); }
    // nothing is carried from section to section; a DATAGRAM row's datagram is delivered
    TS_HD static void sequence(MpeRow&, uint8_t*) {}
    TS_HD static bool delivers(const MpeRow& r, const MpeWatch&) { return r.flags & MPE_DATAGRAM; }
    TS_HD static int bytes_of(const MpeRow& r) { return r.bytes; }
};
// the sequential definition: one slot of one stream
typedef DgramHostStream<MpeRules> MpeHostStream;

}  // namespace s2
