// The IP header rules of the banks that deliver IP datagrams (mpe_rules.h: MPE sections; ule_rules.h: ULE SNDUs; include/dvbs2gpu.h,
// DESIGN section 9), stated once: what the bytes behind an encapsulation header say of the row -- IPv4 IHL, total_length and header
// checksum, IPv6 payload_length, the protocol, addresses and ports of an unfragmented TCP / UDP datagram, and the body bytes behind the
// datagram.  Written from memory of RFC 791 and RFC 8200: every offset is a field of IpLayout, which the banks' layouts repeat.
// Standard headers only.
#pragma once
#include "ts_reasm_rules.h"

namespace s2 {

struct IpLayout {
    int32_t ethertype_ipv4, ethertype_ipv6;                // 0x0800, 0x86DD
    int32_t ipv4_min_header;           // 20
    int32_t ipv4_total_length_at, ipv4_fragment_at, ipv4_protocol_at, ipv4_src_at, ipv4_dst_at;   // 2, 6, 9, 12, 16
    int32_t ipv6_header;               // 40
    int32_t ipv6_payload_length_at, ipv6_next_header_at;   // 4, 6
};
constexpr IpLayout IP = {0x0800, 0x86DD, 20, 2, 6, 9, 12, 16, 40, 4, 6};
constexpr int IP_HEAD_BYTES = 60 + 4;                      // the longest IPv4 header and the ports: what the rules read at most

enum { IP_IS_DATAGRAM = 0, IP_IS_OTHER_PROTOCOL, IP_IS_BAD };

// The datagram in the unit's bytes [at, end), of the family (4, 6, else: neither) that the encapsulation named.  s: the unit's leading
// bytes and the reductions over them --  s.rd(i): byte i;  s.sum(n, f): the sum of f(k) over [0, n), n <= 64  (and s.any, which these
// rules do not use).  Fills family, protocol, src4, dst4, src_port, dst_port, bytes and stuffing of a row that is a datagram and nothing
// of any other; the flag is the caller's.
template <typename Src, typename Row>
TS_HD inline int ip_row_fields(const Src& s, int at, int end, int family, Row& r) {
    if (family != 4 && family != 6) return IP_IS_OTHER_PROTOCOL;
    const int avail = end - at;
    int ports_at = -1;
    if (family == 4) {
        const int hl = avail >= IP.ipv4_min_header ? 4 * (int)(s.rd(at) & 15) : 0;
        const int tl = hl ? (int)(s.rd(at + IP.ipv4_total_length_at) << 8 | s.rd(at + IP.ipv4_total_length_at + 1)) : 0;
        if (hl < IP.ipv4_min_header || hl > avail || tl < hl || tl > avail) return IP_IS_BAD;
        unsigned sum = s.sum(hl / 2, [&](int k) { return s.rd(at + 2 * k) << 8 | s.rd(at + 2 * k + 1); });
        sum = (sum & 0xFFFF) + (sum >> 16); sum = (sum & 0xFFFF) + (sum >> 16);
        if (sum != 0xFFFF) return IP_IS_BAD;
        auto be32 = [&](int i) { return (uint32_t)(s.rd(i) << 24 | s.rd(i + 1) << 16 | s.rd(i + 2) << 8 | s.rd(i + 3)); };
        r.bytes = tl; r.protocol = (uint8_t)s.rd(at + IP.ipv4_protocol_at);
        r.src4 = be32(at + IP.ipv4_src_at); r.dst4 = be32(at + IP.ipv4_dst_at);
        const unsigned frag = (s.rd(at + IP.ipv4_fragment_at) << 8 | s.rd(at + IP.ipv4_fragment_at + 1)) & 0x1FFF;
        if (frag == 0 && tl >= hl + 4) ports_at = at + hl;
    } else {
        const int pl = avail >= IP.ipv6_header ? (int)(s.rd(at + IP.ipv6_payload_length_at) << 8 | s.rd(at + IP.ipv6_payload_length_at + 1)) : 0;
        if (avail < IP.ipv6_header || IP.ipv6_header + pl > avail) return IP_IS_BAD;
        r.bytes = IP.ipv6_header + pl; r.protocol = (uint8_t)s.rd(at + IP.ipv6_next_header_at);
        if (pl >= 4) ports_at = at + IP.ipv6_header;
    }
    r.family = (uint8_t)family; r.stuffing = (uint16_t)(avail - r.bytes);
    if (ports_at >= 0 && (r.protocol == 6 || r.protocol == 17)) {
        r.src_port = (uint16_t)(s.rd(ports_at) << 8 | s.rd(ports_at + 1)); r.dst_port = (uint16_t)(s.rd(ports_at + 2) << 8 | s.rd(ports_at + 3));
    }
    return IP_IS_DATAGRAM;
}

}  // namespace s2
