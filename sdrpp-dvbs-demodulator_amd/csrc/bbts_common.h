// Shared by the BBFRAME -> TS / GSE translation units (bbts.hip: the reference's parser; bbts_ma.hip: the mode-adaptation mode;
// bbts_gse.hip: GSE decapsulation on the device): BBHEADER parsing, the reference-mode state and descriptors, the CRC-32/MPEG
// algebra of the GSE kernels, and the bank's fields the other units need.
#pragma once
#include "ctx.h"

struct dvbs2gpu_bbts;

namespace s2 {

// check_crc8 (bbframe_ts_parser.cpp:70-83): LSB-first register, polynomial 0xAB (reflected 0xD5), over `nbits` MSB-first bits
__host__ __device__ inline unsigned crc8_bits(const uint8_t* in, int nbits) {
    unsigned crc = 0;
    for (int n = 0; n < nbits; ++n) {
        unsigned fb = ((in[n >> 3] >> (7 - (n & 7))) ^ crc) & 1u;
        crc >>= 1;
        if (fb) crc ^= 0xAB;
    }
    return crc;
}
struct HeaderFields { int v[11]; };
__host__ __device__ inline HeaderFields parse_bbheader(const uint8_t* b) {
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
__host__ __device__ inline bool header_ok(const uint8_t* frame, int max_dfl, HeaderFields* h) {
    if (crc8_bits(frame, 80) != 0) return false;
    *h = parse_bbheader(frame);
    const int dfl = h->v[8], syncd = h->v[10];
    if ((unsigned)dfl > (unsigned)max_dfl || syncd >= dfl - 8) return false;
    return dfl % 8 == 0;
}

// ------------------------------------------------------------------ reference-mode state and TS descriptors (bbts.hip, bbts_gse.hip)
constexpr int TS = 188;
constexpr int REASM_STRIDE = 192;

struct BbtsDevState {              // per stream, device resident
    int synched, count;
    int hdr[11];                   // ts_gs, sis_mis, ccm_acm, issyi, npd, ro, isi, upl, dfl, sync, syncd (BBHeader, bbframe_ts_parser.h:37-66)
    int last_cnt, last_proc, pad;
};
struct BbtsFrameDesc {
    int src, npk, pre_len, pre_src, out_off, pad[3];   // pre_src < 0: the carried partial lives in the state buffer
};
struct BbtsStreamPlan {
    int needs_host, out_bytes, fin_len, fin_src;       // fin_src < 0: keep the state buffer's bytes
};
// needs_host: 0 the device finished the stream's call; GSE_SEEN the plan kernel met a GSE frame; the per-stream GSE pass
// turns GSE_SEEN into 0 or into one of the two allowed fallbacks
enum { GSE_SEEN = 1, GSE_FALLBACK_RECORDS = 2, GSE_FALLBACK_CAPACITY = 3 };

#ifdef __HIPCC__
// the packets of one TS frame: 0x47 + 187 bytes each, the first completed from the carried partial (`old` or the input)
__device__ inline void bbts_emit_frame(const uint8_t* __restrict__ bb, const uint8_t* __restrict__ old, const BbtsFrameDesc& e,
                                       uint8_t* __restrict__ o) {
    const uint8_t* pre = e.pre_src < 0 ? old : bb + e.pre_src;
    const uint8_t* src = bb + e.src - e.pre_len;          // virtual stream = partial ++ data field
    auto fetch = [&](int i) -> unsigned {                  // output byte i of this frame's packets
        const int b = i % TS;
        if (b == 0) return 0x47u;                          // TS_SYNC_BYTE in place of the CRC-8 of the previous packet
        const int u = i - 1;                               // packet p is bytes [188 p, 188 p + 187) of the virtual stream; its
        return u < e.pre_len ? pre[u] : src[u];            // 188th byte (the CRC-8 of this packet) is dropped
    };
    const int nbytes = e.npk * TS;
    if ((reinterpret_cast<uintptr_t>(o) & 3) == 0) {
        // 188 = 4 * 47: an output dword never straddles two packets, and its four source bytes are contiguous (one unaligned
        // dword load at src + i - 1; the byte under a packet's sync position is replaced)
        typedef unsigned __attribute__((aligned(1))) unaligned_u32;
        for (int w = threadIdx.x; w < nbytes / 4; w += blockDim.x) {
            const int i = 4 * w;
            unsigned v;
            if (i - 1 >= e.pre_len) {
                v = *reinterpret_cast<const unaligned_u32*>(src + i - 1);
                if (i % TS == 0) v = (v & ~0xffu) | 0x47u;
            } else {
                v = fetch(i) | fetch(i + 1) << 8 | fetch(i + 2) << 16 | fetch(i + 3) << 24;
            }
            reinterpret_cast<unsigned*>(o)[w] = v;
        }
    } else {
        for (int i = threadIdx.x; i < nbytes; i += blockDim.x) o[i] = (uint8_t)fetch(i);
    }
}
#endif

// ------------------------------------------------------------------ CRC-32/MPEG as polynomial arithmetic (GSE, TS 102 606 4.2.2)
// The register after a byte b is (c * x^8 + b * x^32) mod P, P = x^32 + 0x04c11db7, bit k of a word = x^k.  So the CRC of a span
// from a ZERO register is linear in the span, n zero bytes multiply the register by x^(8n), and
//   crc(a ++ b) = crc(a) * x^(8 len b)  ^  crc0(b).
__host__ __device__ inline uint32_t crc32m_mulmod(uint32_t a, uint32_t b) {
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
__host__ __device__ inline uint32_t crc32m_xpow(uint32_t nbytes) {
    constexpr Crc32mPow t = crc32m_make_pow();
    uint32_t r = 1;
    for (int k = 0; k < 17; ++k)
        if ((nbytes >> k) & 1u) r = crc32m_mulmod(r, t.v[k]);
    return r;
}
__host__ __device__ inline uint32_t crc32m_byte(uint32_t c, unsigned byte) {
    c ^= byte << 24;
    for (int b = 0; b < 8; ++b) c = (c << 1) ^ ((c >> 31) ? 0x04c11db7u : 0u);
    return c;
}

// ------------------------------------------------------------------ GSE on the device (bbts_gse.hip)
constexpr int GSE_PKT_CAP = 256;                 // packet records per frame; a frame with more is fallback (a)
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
struct GseFrameRec { int kind, resync, pos, npkt; };   // kind: 0 header rejected, 1 skipped, 2 GSE parsed, 3 TS, 4 GSE with too many packets
struct GseSlot { int busy, frag_id, fill, label; uint32_t proto, crc; };
struct GseCounters {                              // the first nine words of dvbs2gpu_gse_stats
    long long frames, packets, complete_pdus, reassembled_pdus, crc_failures, dropped_no_slot, dropped_overflow, dropped_no_fit, bytes_delivered;
};
struct GseDevState { GseSlot slot[3]; int crc_err, pad; GseCounters cnt; };
struct GseStreamOut { int open_last[3]; int nrows; int ran, pad[3]; };   // ran: the stream pass finished this stream's call

struct BbtsGse;                                 // bbts_gse.hip: the device storage of a bank that has seen a GSE frame
int bbts_gse_create(int nstreams, int max_frames, BbtsGse** out);
void bbts_gse_free(BbtsGse* g);
int bbts_gse_reset(BbtsGse* g);
// enqueues the four GSE launches of one call behind the plan / emit kernels
int bbts_gse_launch(BbtsGse* g, hipStream_t st, const uint8_t* const* d_in, uint8_t* const* d_out, const int* d_nframes, int* d_out_bytes,
                    int fbytes, int max_dfl, int cap, BbtsDevState* d_state, BbtsFrameDesc* d_desc, BbtsStreamPlan* d_plan, uint8_t* d_partial);
GseDevState* bbts_gse_state(BbtsGse* g);
uint8_t* bbts_gse_slot_data(BbtsGse* g, int stream, int slot);
GseStreamOut* bbts_gse_stream_out(BbtsGse* g);
void* bbts_gse_rows(BbtsGse* g, int stream);   // dvbs2gpu_gse_pdu[max_frames * GSE_PKT_CAP]

struct BbtsMa;                                  // bbts_ma.hip
void bbts_ma_free(BbtsMa* m);
struct BbtsBankView {
    dvbs2gpu_ctx* ctx;                          // null: a host-only bank (dvbs2gpu_bbts_create_host)
    int nstreams, kbch, max_frames;
    BbtsMa** ma;
};
BbtsBankView bbts_view(dvbs2gpu_bbts* b);
dvbs2gpu_bbts* bbts_new_host_bank(int kbch_bits, int max_frames);
int bbts_reset_reference_state(dvbs2gpu_bbts* b);   // what a freshly created bank's reference-mode parser starts from

}  // namespace s2
