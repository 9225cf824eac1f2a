// The rules of the IP-TS bank (own extension; include/dvbs2gpu.h), each stated once and shared by the kernels
// (ipts.hip), the native host bank (IptsHostStream, behind dvbs2gpu_ipts_create_host) and a plain C++ test program: which rows of a
// table of IP datagrams are UDP datagrams of a watched flow, whether their UDP checksum holds, whether their payload is raw TS or
// RTP/MP2T, what the RTP sequence rule says of them, and where their TS packets go.  The IP header rules are ip_rules.h, unchanged and
// shared with the MPE and ULE banks.
//
// The sequential form -- IptsHostStream::run, row by row -- IS the definition; every other form must give its results for every
// cutting of a datagram sequence into calls.  The syntax is written from memory of RFC 768, RFC 791, RFC 8200, RFC 3550 and RFC 2250
// and pinned to no vector of theirs: every offset and constant the code relies on is a field of IptsLayout, reported through
// dvbs2gpu_ipts_get_layout and compared with the tests' model.
// Standard headers and ip_rules.h only: the host tests compile this file with a plain C++ compiler.
#pragma once
#include "ip_rules.h"

#include <cstring>
#include <vector>

namespace s2 {

struct IptsLayout {                    // the layout of dvbs2gpu_ipts_layout (ipts.hip asserts it)
    int32_t gre_header_bytes;          // 00 00 and the protocol type: 4
    int32_t ipv4_src_at, ipv6_src_at, ipv6_dst_at;         // 12, 8, 24 (the IPv4 destination: ipv4_dst_at of the IP layout, 16)
    int32_t ipv4_more_fragments;       // of the 16 bits at ipv4_fragment_at: 0x2000
    int32_t udp_protocol;              // 17
    int32_t udp_header_bytes, udp_length_at, udp_checksum_at;          // 8, 4, 6
    int32_t ts_packet_bytes, ts_sync;  // 188, 0x47
    int32_t rtp_min_header, rtp_version, rtp_payload_type_mp2t;        // 12, 2, 33
    int32_t rtp_seq_at, rtp_timestamp_at, rtp_ssrc_at;     // 2, 4, 8
    int32_t late_from;                 // (seq - last_seq - 1) mod 65536 from here on is a late packet: 0x8000
    int32_t head_bytes;                // rules 2 to 6 read the first 4 + 60 + 8 = 72 bytes of a row at most; a wave keeps 128
    int32_t slots, row_bytes, view_bytes;                  // 4, 40, 40
};
constexpr IptsLayout IPTS = {4, 12, 8, 24, 0x2000, 17, 8, 4, 6, 188, 0x47, 12, 2, 33, 2, 4, 8, 0x8000, 128, 4, 40, 40};

constexpr int IPTS_SLOTS = 4, IPTS_MAX_ROWS = 16384;
constexpr int IPTS_KIND_RAW_IP = 0, IPTS_KIND_GRE = 1;
// row flags (DVBS2GPU_IPTS_*), in the order of the rules
constexpr unsigned IPTS_NOT_DELIVERED = 1, IPTS_NOT_IP = 2, IPTS_BAD_IP = 4, IPTS_FRAGMENT = 8, IPTS_OTHER_PROTOCOL = 16, IPTS_BAD_UDP = 32, IPTS_UNWATCHED = 64,
                   IPTS_BAD_CHECKSUM = 128, IPTS_NO_CHECKSUM = 256, IPTS_BAD_PAYLOAD = 512, IPTS_OTHER_PAYLOAD = 1024, IPTS_RAW = 2048, IPTS_RTP = 4096,
                   IPTS_NEW_SOURCE = 8192, IPTS_LOSS = 16384, IPTS_LATE = 32768, IPTS_TS = 65536;

// one call's view of one stream's datagrams; the layout of dvbs2gpu_ipts_view
struct IptsView {
    const uint8_t* bytes;
    const uint8_t* rows;               // n rows of `stride` bytes; a row keeps an int32 offset into `bytes` at offset_at and an int32 byte count at bytes_at
    int32_t stride, offset_at, bytes_at, kind, n, reserved;
};
struct IptsFlow { int32_t family, port; uint8_t addr[16]; };           // family 0: the slot is empty; an IPv4 address in addr[0..3]
struct IptsSeq { int32_t has; uint32_t last_seq, ssrc; int32_t pad; };  // a slot's RTP state
// one input row; the layout of dvbs2gpu_ipts_row
struct IptsRow {
    uint32_t flags;
    int8_t slot;
    uint8_t family, payload_type, reserved;
    uint16_t src_port, dst_port;
    uint16_t rtp_seq, ts_at;
    uint32_t rtp_timestamp, rtp_ssrc;
    int32_t packets, lost, offset, bytes;
};
// the counters one call adds to a stream's and to a slot's statistics (dvbs2gpu_ipts_stats, as 32-bit shares)
struct IptsStreamCnt { int32_t rows, not_delivered, not_ip, bad_ip, fragments, other_protocol, bad_udp, unwatched; };
struct IptsSlotCnt { int32_t matched, bad_checksum, no_checksum, bad_payload, other_payload, raw, rtp, new_source, loss_events, late, ts, ts_packets,
                             bytes_delivered, lost; };
constexpr int IPTS_NSTREAM_CNT = 8, IPTS_NSLOT_CNT = 14;
enum { IPC_ROWS = 0, IPC_MATCHED = 0, IPC_TS_PACKETS = 11, IPC_BYTES = 12, IPC_LOST = 13 };

// what ip_row_fields fills of a row
struct IptsIp { uint8_t family, protocol; uint16_t stuffing, src_port, dst_port; uint32_t src4, dst4; int32_t bytes; };

// Rules 1 to 8 of one row: the row but for the sequence rule (9) and its offset (10); a RAW row is a TS row already.  off, nbytes: what
// the input row says.  s: the datagram's bytes and the reductions over them, so that a wave can take them with its lanes --
//   s.rd(i): byte i, asked for i < nbytes only;  s.sum(n, f): the sum of f(k) over [0, n), n <= 64 (as ip_rules.h asks);
//   s.wsum(at, len): the sum of the bytes [at, at + len) as big-endian 16-bit words, an odd last byte padded with a zero byte, not
//   folded (len < 65536: it fits 32 bits);  s.syncs(at, n): is byte at + 188 k the sync byte for every k in [0, n).
// Nothing is read at or beyond nbytes.
template <typename Src>
TS_HD inline IptsRow ipts_row_fields(const Src& s, int off, int nbytes, int kind, const IptsFlow* flows) {
    IptsRow r = {};
    r.slot = -1; r.offset = -1;
    if (off < 0) { r.flags = IPTS_NOT_DELIVERED; return r; }
    if (nbytes < 0) nbytes = 0;
    auto be16 = [&](int i) { return s.rd(i) << 8 | s.rd(i + 1); };
    auto be32 = [&](int i) { return (uint32_t)(be16(i) << 16 | be16(i + 2)); };
    // 2: GRE, or the version nibble
    int at = 0, family;
    if (kind == IPTS_KIND_GRE) {
        at = IPTS.gre_header_bytes;
        const unsigned type = nbytes >= at && !s.rd(0) && !s.rd(1) ? be16(2) : 0;
        family = type == (unsigned)IP.ethertype_ipv4 ? 4 : type == (unsigned)IP.ethertype_ipv6 ? 6 : 0;
    } else {
        family = nbytes > 0 ? (int)(s.rd(0) >> 4) : 0;
    }
    if (family != 4 && family != 6) { r.flags = IPTS_NOT_IP; return r; }
    // 3: the IP header (ip_rules.h)
    IptsIp ip = {};
    if (ip_row_fields(s, at, nbytes, family, ip) != IP_IS_DATAGRAM) { r.flags = IPTS_BAD_IP; return r; }
    r.family = (uint8_t)family;
    // 4: fragments and protocol
    const int hl = family == 4 ? 4 * (int)(s.rd(at) & 15) : IP.ipv6_header;
    if (family == 4 && (be16(at + IP.ipv4_fragment_at) & (unsigned)(IPTS.ipv4_more_fragments | 0x1FFF))) { r.flags = IPTS_FRAGMENT; return r; }
    if (ip.protocol != IPTS.udp_protocol) { r.flags = IPTS_OTHER_PROTOCOL; return r; }
    // 5: the UDP length
    const int u = at + hl, room = ip.bytes - hl;
    const int L = room >= IPTS.udp_header_bytes ? (int)be16(u + IPTS.udp_length_at) : 0;
    if (L < IPTS.udp_header_bytes || L > room) { r.flags = IPTS_BAD_UDP; return r; }
    r.src_port = (uint16_t)be16(u); r.dst_port = (uint16_t)be16(u + 2);
    // 6: the flow slots, the lowest first
    const int dst_at = at + (family == 4 ? IP.ipv4_dst_at : IPTS.ipv6_dst_at), alen = family == 4 ? 4 : 16;
    int slot = -1;
    for (int k = 0; k < IPTS_SLOTS && slot < 0; ++k) {
        if (flows[k].family != family || flows[k].port != (int)r.dst_port) continue;
        bool same = true;
        for (int i = 0; i < alen; ++i) same &= s.rd(dst_at + i) == (unsigned)flows[k].addr[i];
        if (same) slot = k;
    }
    if (slot < 0) { r.flags = IPTS_UNWATCHED; return r; }
    r.slot = (int8_t)slot;
    // 7: the checksum over the pseudo-header (the addresses, the protocol, the UDP length) and the L UDP bytes
    if (be16(u + IPTS.udp_checksum_at) == 0) {
        if (family == 6) { r.flags = IPTS_BAD_CHECKSUM; return r; }
        r.flags = IPTS_NO_CHECKSUM;
    } else {
        const int src_at = at + (family == 4 ? IPTS.ipv4_src_at : IPTS.ipv6_src_at);
        unsigned sum = s.sum(alen, [&](int k) { return be16(src_at + 2 * k); }) + (unsigned)IPTS.udp_protocol + (unsigned)L + s.wsum(u, L);
        sum = (sum & 0xFFFF) + (sum >> 16); sum = (sum & 0xFFFF) + (sum >> 16);
        if (sum != 0xFFFF) { r.flags = IPTS_BAD_CHECKSUM; return r; }
    }
    // 8: raw TS, or RTP with payload type 33
    const int pay = u + IPTS.udp_header_bytes, plen = L - IPTS.udp_header_bytes, TSB = IPTS.ts_packet_bytes;
    if (plen > 0 && plen % TSB == 0 && s.syncs(pay, plen / TSB)) {
        r.flags |= IPTS_RAW | IPTS_TS;
        r.ts_at = (uint16_t)pay; r.packets = plen / TSB; r.bytes = plen;
        return r;
    }
    const unsigned b0 = plen >= IPTS.rtp_min_header ? s.rd(pay) : 0;
    if ((int)(b0 >> 6) != IPTS.rtp_version) { r.flags |= IPTS_BAD_PAYLOAD; return r; }      // (fewer than 12 bytes, too)
    int hdr = IPTS.rtp_min_header + 4 * (int)(b0 & 15), pad = 0;
    bool fits = hdr <= plen;
    if (fits && (b0 >> 4 & 1)) {
        fits = hdr + 4 <= plen;
        if (fits) { hdr += 4 + 4 * (int)be16(pay + hdr + 2); fits = hdr <= plen; }
    }
    if (fits && (b0 >> 5 & 1)) {
        pad = (int)s.rd(pay + plen - 1);
        fits = pad >= 1 && hdr + pad <= plen;
    }
    if (!fits) { r.flags |= IPTS_BAD_PAYLOAD; return r; }
    r.payload_type = (uint8_t)(s.rd(pay + 1) & 127);
    if (r.payload_type != IPTS.rtp_payload_type_mp2t) { r.flags |= IPTS_OTHER_PAYLOAD; return r; }
    const int left = plen - hdr - pad;
    if (left <= 0 || left % TSB || !s.syncs(pay + hdr, left / TSB)) { r.flags |= IPTS_BAD_PAYLOAD; return r; }
    r.flags |= IPTS_RTP;
    r.rtp_seq = (uint16_t)be16(pay + IPTS.rtp_seq_at); r.rtp_timestamp = be32(pay + IPTS.rtp_timestamp_at); r.rtp_ssrc = be32(pay + IPTS.rtp_ssrc_at);
    r.ts_at = (uint16_t)(pay + hdr); r.packets = left / TSB; r.bytes = left;
    return r;
}

// 9: the sequence rule of a slot on an RTP row, in table order
TS_HD inline void ipts_seq_step(IptsSeq& st, IptsRow& r) {
    // (as selects, not branches: the one lane per slot that walks the rows on the device diverges from its neighbours row by row)
    const bool known = st.has && st.ssrc == r.rtp_ssrc;
    const unsigned d = known ? ((unsigned)r.rtp_seq - st.last_seq - 1u) & 0xFFFFu : 0u;
    const bool late = d >= (unsigned)IPTS.late_from;
    r.flags |= late ? IPTS_LATE : IPTS_TS | (d ? IPTS_LOSS : 0u) | (st.has && !known ? IPTS_NEW_SOURCE : 0u);
    r.lost = late ? 0 : (int32_t)d;
    r.packets = late ? 0 : r.packets; r.bytes = late ? 0 : r.bytes;
    st.last_seq = late ? st.last_seq : r.rtp_seq; st.ssrc = late ? st.ssrc : r.rtp_ssrc;
    st.has = 1;
}

// the counters that a finished row steps: stream(index into IptsStreamCnt), slot(index into IptsSlotCnt, amount) of the row's slot
template <typename AddStream, typename AddSlot>
TS_HD inline void ipts_account(const IptsRow& r, bool delivered, AddStream stream, AddSlot slot) {
    stream(IPC_ROWS);
    for (int k = 0; k < 7; ++k) if (r.flags >> k & 1) stream(1 + k);
    if (r.slot < 0) return;
    slot(IPC_MATCHED, 1);
    for (int k = 0; k < 10; ++k) if (r.flags >> (7 + k) & 1) slot(1 + k, 1);
    if (r.flags & IPTS_LOSS) slot(IPC_LOST, r.lost);
    if (r.flags & IPTS_TS) {
        slot(IPC_TS_PACKETS, r.packets);
        if (delivered) slot(IPC_BYTES, r.bytes);
    }
}

// a datagram's bytes in memory, the reductions as loops
struct IptsHostSrc {
    const uint8_t* b;
    unsigned rd(int i) const { return b[i]; }
    template <typename Fn> unsigned sum(int n, Fn f) const { unsigned v = 0; for (int k = 0; k < n; ++k) v += f(k); return v; }
    unsigned wsum(int at, int len) const {
        unsigned v = 0;
        for (int i = 0; i < len; i += 2) v += (unsigned)b[at + i] << 8 | (i + 1 < len ? b[at + i + 1] : 0u);
        return v;
    }
    bool syncs(int at, int n) const { for (int k = 0; k < n; ++k) if (b[at + IPTS.ts_packet_bytes * k] != IPTS.ts_sync) return false; return true; }
};

inline int32_t ipts_view_i32(const IptsView& v, int r, int at) { int32_t x; memcpy(&x, v.rows + (size_t)r * v.stride + at, 4); return x; }

// one stream: four flow slots with their RTP states
struct IptsHostStream {
    IptsFlow flow[IPTS_SLOTS] = {};
    IptsSeq seq[IPTS_SLOTS] = {};
    // of the last call
    std::vector<IptsRow> rows;
    std::vector<uint8_t> bytes[IPTS_SLOTS];
    IptsStreamCnt scnt = {};
    IptsSlotCnt cnt[IPTS_SLOTS] = {};

    void clear() { for (IptsSeq& q : seq) q = IptsSeq{}; clear_call(); }
    void clear_call() { rows.clear(); for (auto& b : bytes) b.clear(); scnt = IptsStreamCnt{}; for (IptsSlotCnt& c : cnt) c = IptsSlotCnt{}; }
    // one call: the view's rows in table order.  The caller keeps a copy of `seq` if the call may have to be undone.
    void run(const IptsView& v, bool want_bytes) {
        clear_call();
        for (int i = 0; i < v.n; ++i) {
            const int off = ipts_view_i32(v, i, v.offset_at), nb = ipts_view_i32(v, i, v.bytes_at);
            const uint8_t* d = off < 0 ? nullptr : v.bytes + off;
            IptsRow r = ipts_row_fields(IptsHostSrc{d}, off, nb, v.kind, flow);
            if (r.flags & IPTS_RTP) ipts_seq_step(seq[r.slot], r);
            if (want_bytes && (r.flags & IPTS_TS)) {
                std::vector<uint8_t>& o = bytes[r.slot];
                r.offset = (int32_t)o.size();
                o.insert(o.end(), d + r.ts_at, d + r.ts_at + r.bytes);
            }
            ipts_account(r, want_bytes, [&](int c) { ++reinterpret_cast<int32_t*>(&scnt)[c]; },
                         [&](int c, int n) { reinterpret_cast<int32_t*>(&cnt[r.slot])[c] += n; });
            rows.push_back(r);
        }
    }
};

}  // namespace s2
