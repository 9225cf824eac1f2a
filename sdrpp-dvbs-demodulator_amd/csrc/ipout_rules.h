// The rules of the IP output bank (own extension; include/dvbs2gpu.h), each stated once and shared by the kernels
// (ipout.hip), the native host bank (IpoutHostStream, behind dvbs2gpu_ipout_create_host) and a plain C++ test program: which packets
// of a transport stream enter which of four flow slots, the 90 kHz tick value of a packet, how a slot's packets are grouped into
// datagrams over the calls, and the IPv4 / IPv6, UDP and RTP headers with their checksums.  It is the IP-TS bank's direction reversed:
// what this file writes, ipts_rules.h reads back.
//
// The sequential form -- IpoutHostStream::run, packet by packet -- IS the definition; every other form must give its results for every
// cutting of a stream into calls.  The syntax is written from memory of RFC 768, RFC 791, RFC 8200, RFC 3550 and RFC 2250 and pinned to
// no vector of theirs: the offsets are those of IpLayout (ip_rules.h) and IptsLayout (ipts_rules.h), and what those two do not name is
// a field of IpoutLayout, reported through dvbs2gpu_ipout_get_layout and compared with the tests' model.
// Standard headers, ip_rules.h and ipts_rules.h only: the host tests compile this file with a plain C++ compiler.
#pragma once
#include "ipts_rules.h"

namespace s2 {

struct IpoutLayout {                   // the layout of dvbs2gpu_ipout_layout (ipout.hip asserts it)
    int32_t ipv4_version_ihl, ipv4_tos_at, ipv4_id_at, ipv4_dont_fragment, ipv4_ttl_at, ipv4_checksum_at;  // 0x45, 1, 4, 0x4000, 8, 10
    int32_t ipv6_hop_limit_at;         // 7
    int32_t rtp_first_byte;            // version 2, no padding, no extension, no CSRC: 0x80
    int32_t tick_divisor;              // 27 MHz ticks per tick of the RTP clock: 300
    int32_t max_packets_per_datagram, held_packets;        // 7, 6
    int32_t pid_map_bytes;             // 1024
    int32_t slots, row_bytes, flow_bytes;                  // 4, 24, 56
};
constexpr IpoutLayout IPOUT = {0x45, 1, 4, 0x4000, 8, 10, 7, 0x80, 300, 7, 6, 1024, 4, 24, 56};

constexpr int IPOUT_SLOTS = 4, IPOUT_MAX_PACKETS = 8192, IPOUT_TS = 188, IPOUT_HELD_BYTES = 6 * 188, IPOUT_MAP_WORDS = 256, IPOUT_MAX_HEADER = 40 + 8 + 12;
constexpr int IPOUT_MODE_RAW = 0, IPOUT_MODE_RTP = 1;
constexpr unsigned IPOUT_RTP = 1, IPOUT_SHORT = 2, IPOUT_CARRIED = 4;   // row flags (DVBS2GPU_IPOUT_*)
constexpr uint64_t IPOUT_TICK_D = 300ull << 24;

// a flow slot; the layout of dvbs2gpu_ipout_flow
struct IpoutFlow {
    int32_t family;                    // 0: the slot is empty
    uint8_t src_addr[16], dst_addr[16];
    uint16_t src_port, dst_port;
    uint8_t ttl, dscp, mode, packets_per_datagram;
    uint32_t ssrc, timestamp_base;
    uint16_t seq_base;
    uint8_t pid_mode, drop_null;
};
// one datagram; the layout of dvbs2gpu_ipout_row
struct IpoutRow {
    int32_t offset, bytes;
    uint32_t rtp_timestamp;
    uint16_t rtp_seq;
    uint8_t packets, flags;
    int32_t first_packet;
    uint16_t udp_checksum, reserved;
};
struct IpoutClock { uint64_t r; uint32_t q, pad; };                      // a stream's (q, r)
struct IpoutSlot { uint32_t dgrams, held_tick; int32_t held, pad; };     // a slot's state: datagrams so far mod 2^32, and what it holds

// does a packet with a good sync byte enter the slot: the monitor's filter form (tsmon_rules.h) without its TEI and sync switches
TS_HD inline bool ipout_passes(int pid, const IpoutFlow& f, const uint32_t* map) {
    if (pid == TSMON_NULL_PID && f.drop_null) return false;
    if (f.pid_mode == 0) return true;
    const bool listed = (map[pid >> 5] >> (pid & 31)) & 1;
    return f.pid_mode == 1 ? listed : !listed;
}
TS_HD inline int ipout_pid(unsigned b1, unsigned b2) { return (int)((b1 & 0x1f) << 8 | b2); }

// the clock: the tick value of packet k of a call that starts at c, and c behind n packets (n <= 8192, tpp < 2^48: below 2^62)
TS_HD inline uint32_t ipout_tick(const IpoutClock& c, uint64_t tpp, int k) { return (uint32_t)(c.q + (c.r + (uint64_t)k * tpp) / IPOUT_TICK_D); }
TS_HD inline IpoutClock ipout_advance(const IpoutClock& c, uint64_t tpp, int n) {
    const uint64_t r = c.r + (uint64_t)n * tpp;
    return IpoutClock{r % IPOUT_TICK_D, (uint32_t)(c.q + r / IPOUT_TICK_D), 0};
}

TS_HD inline int ipout_header_bytes(const IpoutFlow& f) {
    return (f.family == 4 ? IP.ipv4_min_header : IP.ipv6_header) + IPTS.udp_header_bytes + (f.mode == IPOUT_MODE_RTP ? IPTS.rtp_min_header : 0);
}

// what a call makes of a slot that held `held` packets and takes `passed` more: nd datagrams, the first nfull of them of P packets, a
// last one of last (< P) under flush; bytes; and what it holds afterwards
struct IpoutPlan { int nd, nfull, last, held, bytes; };
TS_HD inline IpoutPlan ipout_plan(const IpoutFlow& f, int held, int passed, bool flush) {
    const int P = f.packets_per_datagram, total = held + passed, hb = ipout_header_bytes(f);
    IpoutPlan p = {total / P, total / P, 0, total % P, 0};
    if (flush && p.held) { p.last = p.held; p.held = 0; ++p.nd; }
    p.bytes = p.nfull * (hb + IPOUT_TS * P) + (p.last ? hb + IPOUT_TS * p.last : 0);
    return p;
}

// The headers of a datagram of npk packets into h (at most 60 bytes); returns their length.  paysum: the sum of the TS bytes as
// big-endian 16-bit words, not folded (every packet starts at an even place of the UDP bytes; below 2^27).  *sent: the UDP checksum as sent
TS_HD inline int ipout_headers(uint8_t* h, const IpoutFlow& f, int npk, unsigned seq, uint32_t timestamp, unsigned paysum, uint16_t* sent) {
    const bool rtp = f.mode == IPOUT_MODE_RTP;
    const int iph = f.family == 4 ? IP.ipv4_min_header : IP.ipv6_header;
    const unsigned L = (unsigned)(IPTS.udp_header_bytes + (rtp ? IPTS.rtp_min_header : 0) + IPOUT_TS * npk);
    auto put16 = [&](int at, unsigned v) { h[at] = (uint8_t)(v >> 8); h[at + 1] = (uint8_t)v; };
    auto be16 = [&](int at) { return (unsigned)h[at] << 8 | h[at + 1]; };
    auto fold = [](unsigned v) { v = (v & 0xFFFF) + (v >> 16); return (v & 0xFFFF) + (v >> 16); };
    unsigned sum = (unsigned)IPTS.udp_protocol + L;       // the pseudo-header: the addresses, the protocol, the UDP length
    if (f.family == 4) {
        h[0] = (uint8_t)IPOUT.ipv4_version_ihl; h[IPOUT.ipv4_tos_at] = (uint8_t)(f.dscp << 2);
        put16(IP.ipv4_total_length_at, iph + L); put16(IPOUT.ipv4_id_at, 0); put16(IP.ipv4_fragment_at, IPOUT.ipv4_dont_fragment);
        h[IPOUT.ipv4_ttl_at] = f.ttl; h[IP.ipv4_protocol_at] = (uint8_t)IPTS.udp_protocol; put16(IPOUT.ipv4_checksum_at, 0);
        for (int i = 0; i < 4; ++i) { h[IP.ipv4_src_at + i] = f.src_addr[i]; h[IP.ipv4_dst_at + i] = f.dst_addr[i]; }
        unsigned hs = 0;
        for (int k = 0; k < iph / 2; ++k) hs += be16(2 * k);
        put16(IPOUT.ipv4_checksum_at, ~fold(hs) & 0xFFFF);
        for (int k = 0; k < 4; ++k) sum += be16(IP.ipv4_src_at + 2 * k);
    } else {
        const unsigned tc = (unsigned)f.dscp << 2;
        h[0] = (uint8_t)(0x60 | tc >> 4); h[1] = (uint8_t)(tc << 4); h[2] = 0; h[3] = 0;
        put16(IP.ipv6_payload_length_at, L); h[IP.ipv6_next_header_at] = (uint8_t)IPTS.udp_protocol; h[IPOUT.ipv6_hop_limit_at] = f.ttl;
        for (int i = 0; i < 16; ++i) { h[IPTS.ipv6_src_at + i] = f.src_addr[i]; h[IPTS.ipv6_dst_at + i] = f.dst_addr[i]; }
        for (int k = 0; k < 16; ++k) sum += be16(IPTS.ipv6_src_at + 2 * k);
    }
    const int u = iph;
    put16(u, f.src_port); put16(u + 2, f.dst_port); put16(u + IPTS.udp_length_at, L); put16(u + IPTS.udp_checksum_at, 0);
    int hb = u + IPTS.udp_header_bytes;
    if (rtp) {
        h[hb] = (uint8_t)IPOUT.rtp_first_byte; h[hb + 1] = (uint8_t)IPTS.rtp_payload_type_mp2t;
        put16(hb + IPTS.rtp_seq_at, seq & 0xFFFF);
        put16(hb + IPTS.rtp_timestamp_at, timestamp >> 16); put16(hb + IPTS.rtp_timestamp_at + 2, timestamp & 0xFFFF);
        put16(hb + IPTS.rtp_ssrc_at, f.ssrc >> 16); put16(hb + IPTS.rtp_ssrc_at + 2, f.ssrc & 0xFFFF);
        hb += IPTS.rtp_min_header;
    }
    for (int k = u / 2; k < hb / 2; ++k) sum += be16(2 * k);
    sum = fold(fold(sum) + fold(paysum));
    unsigned c = ~sum & 0xFFFF;
    if (c == 0) c = 0xFFFF;
    put16(u + IPTS.udp_checksum_at, c);
    *sent = (uint16_t)c;
    return hb;
}

// the row of datagram j of a call
TS_HD inline IpoutRow ipout_row(const IpoutFlow& f, int hb, int j, int npk, unsigned seq, uint32_t tick, bool carried, int first_packet, uint16_t sent) {
    const bool rtp = f.mode == IPOUT_MODE_RTP;
    IpoutRow r = {};
    r.offset = j * (hb + IPOUT_TS * f.packets_per_datagram); r.bytes = hb + IPOUT_TS * npk;
    r.rtp_timestamp = rtp ? f.timestamp_base + tick : 0; r.rtp_seq = rtp ? (uint16_t)seq : (uint16_t)0;
    r.packets = (uint8_t)npk;
    r.flags = (uint8_t)((rtp ? IPOUT_RTP : 0u) | (npk < f.packets_per_datagram ? IPOUT_SHORT : 0u) | (carried ? IPOUT_CARRIED : 0u));
    r.first_packet = first_packet; r.udp_checksum = sent;
    return r;
}

// one stream: four flow slots with their PID lists, the clock, and what the slots hold
struct IpoutHostStream {
    IpoutFlow flow[IPOUT_SLOTS] = {};
    uint32_t map[IPOUT_SLOTS][IPOUT_MAP_WORDS] = {};
    uint64_t tpp = 0;
    struct State {                     // what a call advances; the caller keeps a copy if the call may have to be undone
        IpoutClock clk = {};
        IpoutSlot slot[IPOUT_SLOTS] = {};
        uint8_t held[IPOUT_SLOTS][IPOUT_HELD_BYTES + IPOUT_TS] = {};    // (the packet that completes a datagram lies here for a moment)
    } st;
    // of the last call
    std::vector<IpoutRow> rows[IPOUT_SLOTS];
    std::vector<uint8_t> bytes[IPOUT_SLOTS];
    int32_t passed[IPOUT_SLOTS] = {}, packets = 0, bad_sync = 0;
    int32_t first[IPOUT_SLOTS] = {};   // of the group that a slot is filling: the first packet of this call in it
    bool carried[IPOUT_SLOTS] = {};    // and whether it began with packets of earlier calls

    void clear() { st = State{}; clear_call(); }
    void clear_slot(int k) { st.slot[k] = IpoutSlot{}; }
    void clear_call() {
        for (int k = 0; k < IPOUT_SLOTS; ++k) { rows[k].clear(); bytes[k].clear(); passed[k] = 0; first[k] = -1; carried[k] = st.slot[k].held > 0; }
        packets = bad_sync = 0;
    }
    void emit(int k) {
        const IpoutFlow& f = flow[k];
        IpoutSlot& s = st.slot[k];
        unsigned paysum = 0;
        for (int i = 0; i < IPOUT_TS * s.held; i += 2) paysum += (unsigned)st.held[k][i] << 8 | st.held[k][i + 1];
        uint8_t h[IPOUT_MAX_HEADER];
        uint16_t sent;
        const unsigned seq = (f.seq_base + s.dgrams) & 0xFFFF;
        const bool rtp = f.mode == IPOUT_MODE_RTP;
        const int hb = ipout_headers(h, f, s.held, seq, rtp ? f.timestamp_base + s.held_tick : 0, paysum, &sent);
        rows[k].push_back(ipout_row(f, hb, (int)rows[k].size(), s.held, seq, s.held_tick, carried[k], first[k], sent));
        bytes[k].insert(bytes[k].end(), h, h + hb);
        bytes[k].insert(bytes[k].end(), st.held[k], st.held[k] + IPOUT_TS * s.held);
        ++s.dgrams; s.held = 0; first[k] = -1; carried[k] = false;
    }
    // one call: n packets at ts
    void run(const uint8_t* ts, int n, bool flush) {
        clear_call();
        for (int i = 0; i < n; ++i) {
            const uint8_t* p = ts + (size_t)IPOUT_TS * i;
            const uint32_t tick = st.clk.q;
            st.clk = ipout_advance(st.clk, tpp, 1);
            ++packets;
            if (p[0] != IPTS.ts_sync) { ++bad_sync; continue; }
            const int pid = ipout_pid(p[1], p[2]);
            for (int k = 0; k < IPOUT_SLOTS; ++k) {
                if (!flow[k].family || !ipout_passes(pid, flow[k], map[k])) continue;
                IpoutSlot& s = st.slot[k];
                ++passed[k];
                if (s.held == 0) s.held_tick = tick;
                if (first[k] < 0) first[k] = i;
                memcpy(st.held[k] + IPOUT_TS * s.held, p, IPOUT_TS);
                if (++s.held == flow[k].packets_per_datagram) emit(k);
            }
        }
        for (int k = 0; flush && k < IPOUT_SLOTS; ++k)
            if (flow[k].family && st.slot[k].held > 0) emit(k);
    }
};

}  // namespace s2
