// The rules of the BBFRAME -> TS / GSE bank that the kernels and the native host parsers share, each stated once: BBHEADER parsing,
// the CRC-32/MPEG algebra, the GSE records and reassembly state, and the GSE packet header (gse_parse_packet: the one place that
// reads a GSE header, for the reference's rules and for TS 102 606's).
// Standard headers only: bbts_host.h and the host tests compile this file with a plain C++ compiler.
#pragma once
#include <cstdint>

#ifdef __HIPCC__
#define BBTS_HD __host__ __device__
#define BBTS_INLINE __forceinline__
#else
#define BBTS_HD
#define BBTS_INLINE inline
#endif

namespace s2 {

// check_crc8 (bbframe_ts_parser.cpp:70-83): LSB-first register, polynomial 0xAB (reflected 0xD5), over `nbits` MSB-first bits
BBTS_HD inline unsigned crc8_bits(const uint8_t* in, int nbits) {
    unsigned crc = 0;
    for (int n = 0; n < nbits; ++n) {
        unsigned fb = ((in[n >> 3] >> (7 - (n & 7))) ^ crc) & 1u;
        crc >>= 1;
        if (fb) crc ^= 0xAB;
    }
    return crc;
}
struct HeaderFields { int v[11]; };
BBTS_HD inline HeaderFields parse_bbheader(const uint8_t* b) {
    HeaderFields h;
    h.v[0] = b[0] >> 6; h.v[1] = (b[0] >> 5) & 1; h.v[2] = (b[0] >> 4) & 1; h.v[3] = (b[0] >> 3) & 1; h.v[4] = (b[0] >> 2) & 1;
    h.v[5] = b[0] & 3;
    h.v[6] = h.v[1] == 0 ? b[1] : 0;
    h.v[7] = b[2] << 8 | b[3];
    h.v[8] = b[4] << 8 | b[5];
    h.v[9] = b[6];
    h.v[10] = b[7] << 8 | b[8];
    return h;
}
// header validation of work() (.cpp:119-152): true when the frame is parsed at all
BBTS_HD inline bool header_ok(const uint8_t* frame, int max_dfl, HeaderFields* h) {
    if (crc8_bits(frame, 80) != 0) return false;
    *h = parse_bbheader(frame);
    const int dfl = h->v[8], syncd = h->v[10];
    if ((unsigned)dfl > (unsigned)max_dfl || syncd >= dfl - 8) return false;
    return dfl % 8 == 0;
}

constexpr int TS = 188;

// ------------------------------------------------------------------ CRC-32/MPEG as polynomial arithmetic (GSE, TS 102 606 4.2.2)
// The register after a byte b is (c * x^8 + b * x^32) mod P, P = x^32 + 0x04c11db7, bit k of a word = x^k.  So the CRC of a span
// from a ZERO register is linear in the span, n zero bytes multiply the register by x^(8n), and
//   crc(a ++ b) = crc(a) * x^(8 len b)  ^  crc0(b).
BBTS_HD inline uint32_t crc32m_mulmod(uint32_t a, uint32_t b) {
    uint32_t r = 0;
    for (int i = 31; i >= 0; --i) {
        r = (r << 1) ^ ((r >> 31) ? 0x04c11db7u : 0u);
        if ((b >> i) & 1u) r ^= a;
    }
    return r;
}
struct Crc32mPow { uint32_t v[17]; };                         // v[k] = x^(8 * 2^k) mod P
constexpr Crc32mPow crc32m_make_pow() {
    Crc32mPow t = {};
    uint32_t p = 0x100u;
    for (int k = 0; k < 17; ++k) {
        t.v[k] = p;
        uint32_t r = 0;
        for (int i = 31; i >= 0; --i) {
            r = (r << 1) ^ ((r >> 31) ? 0x04c11db7u : 0u);
            if ((p >> i) & 1u) r ^= p;
        }
        p = r;
    }
    return t;
}
// x^(8 nbytes) mod P, nbytes < 2^17
BBTS_HD inline uint32_t crc32m_xpow(uint32_t nbytes) {
    constexpr Crc32mPow t = crc32m_make_pow();
    uint32_t r = 1;
    for (int k = 0; k < 17; ++k)
        if ((nbytes >> k) & 1u) r = crc32m_mulmod(r, t.v[k]);
    return r;
}
BBTS_HD constexpr uint32_t crc32m_byte(uint32_t c, unsigned byte) {
    c ^= byte << 24;
    for (int b = 0; b < 8; ++b) c = (c << 1) ^ ((c >> 31) ? 0x04c11db7u : 0u);
    return c;
}

// ------------------------------------------------------------------ GSE records and reassembly state
constexpr int GSE_PKT_CAP = 256;                 // packet records per frame on the device; a frame with more goes to the host parser
constexpr int GSE_SLOT_BYTES = 65536;
enum { GSE_COMPLETE = 0, GSE_START = 1, GSE_MIDDLE = 2, GSE_END = 3 };
struct GsePkt {                                   // one GSE packet, 16 bytes
    uint32_t src;                                 // offset of the payload in the call's input
    uint32_t w1;                                  // payload length | frag id << 16 | kind << 24 | label present << 26
    // after the frame pass:   COMPLETE {-, proto}  START {register after the packet, proto}  MIDDLE {crc0, xpow}  END {crc0 ^ received, xpow}
    // after the stream pass:  COMPLETE {offset in out or -1, -}  START / MIDDLE {offset in the PDU, link}  END {row or -1, link}
    // link: the previous fragment of the PDU in this call, or -(1 + slot): what precedes is in that slot's buffer
    uint32_t a, b;
};
struct GseSlot { int busy, frag_id, fill, label; uint32_t proto, crc; };
struct GseCounters {                              // the first nine words of dvbs2gpu_gse_stats
    long long frames, packets, complete_pdus, reassembled_pdus, crc_failures, dropped_no_slot, dropped_overflow, dropped_no_fit, bytes_delivered;
};
struct GseDevState { GseSlot slot[3]; int crc_err, pad; GseCounters cnt; };   // one reassembly context: on the device and, as is, on the host

// ------------------------------------------------------------------ the GSE packet header
// Two rule sets.  GseReference: what dsp::dvbs2::BBFrameTSParser::work does (bbframe_ts_parser.cpp:211-383), with the rules of
// include/dvbs2gpu.h where that is undefined.  GseStrict: TS 102 606, for the mode-adaptation bank.  Every point in which they
// differ is a branch on Rules::reference in gse_parse_packet.
struct GseReference { static constexpr bool reference = true; };
struct GseStrict { static constexpr bool reference = false; };
struct GsePktHdr {
    int kind, id, label, body, plen;              // frag id (0: COMPLETE), label bytes, payload offset and length
    unsigned proto;                               // COMPLETE, START (0 otherwise)
    int span_at, span_len;                        // what the PDU's CRC-32 covers of this packet (nothing of a COMPLETE one)
};
enum { GSE_PADDING = 0, GSE_STOP = -1, GSE_MALFORMED = -2 };
// The packet at offset `at`, rd(i) being byte i.  Returns the bytes it takes, or GSE_PADDING (the walk of the frame ends), GSE_STOP
// (the reference's silent end of the walk) or GSE_MALFORMED (strict).  All offsets count like `at` does.
//   reference: at counts from the start of the stream's input, limit is the end of the CALL's input: a packet may run past its data field;
//   strict:    at counts from the start of the data field (or from wherever the caller's rd does), limit is the end of the DATA FIELD.
template <typename Rules, typename Rd>
BBTS_HD BBTS_INLINE int gse_parse_packet(Rd rd, int at, int limit, GsePktHdr* p) {
    if (Rules::reference && at + 2 > limit) return GSE_STOP;
    const unsigned h1 = rd(at);
    const bool S = h1 & 0x80, E = h1 & 0x40;
    const int lt = h1 >> 4 & 3;
    if (!S && !E && lt == 0) return GSE_PADDING;
    if (at + 2 > limit) return GSE_MALFORMED;
    const int field = (int)((h1 & 0x0f) << 8 | rd(at + 1));
    const int fixed = S && E ? 2 : S ? 5 : 1;       // protocol type | frag id, total length, protocol type | frag id
    // label: the reference tests ((h1 & 0x30) >> 2) against 0 and 2, so only LT = 00 can match; strict: 10 has none, 11 re-uses the
    // label of the packet before and has no bytes
    const int label = !S ? 0 : lt == 0 ? 6 : (!Rules::reference && lt == 1) ? 3 : 0;
    int plen = field - fixed - label;
    if (Rules::reference) plen &= 0xffff;           // the reference's length arithmetic is uint16
    else if (plen < (!S && E ? 4 : 0)) return GSE_MALFORMED;          // an END shorter than its CRC-32 included
    const int body = at + 2 + fixed + label;
    if (body + plen > limit) return Rules::reference ? GSE_STOP : GSE_MALFORMED;
    p->kind = S && E ? GSE_COMPLETE : S ? GSE_START : E ? GSE_END : GSE_MIDDLE;
    p->id = S && E ? 0 : (int)rd(at + 2);
    p->label = label; p->body = body; p->plen = plen;
    p->proto = S && E ? rd(at + 2) << 8 | rd(at + 3) : S ? rd(at + 5) << 8 | rd(at + 6) : 0;
    p->span_at = body; p->span_len = 0;
    if (p->kind == GSE_START) { p->span_at = at + 3; p->span_len = body + plen - (at + 3); }     // total length, protocol type, label, payload
    else if (p->kind == GSE_MIDDLE) p->span_len = plen;
    else if (p->kind == GSE_END) p->span_len = Rules::reference && plen < 4 ? 0 : plen - 4;      // the reference: the received CRC-32 is then read from before the payload
    return body + plen - at;
}

}  // namespace s2
