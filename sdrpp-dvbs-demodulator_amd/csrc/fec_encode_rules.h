// The rules of the DVB-S2 FEC encoder (fec_encode.hip): everything the kernels read that is not a frame, built on the host.
//
//   BCH (ETSI EN 302 307-1 clause 5.3.1)   g(x) = lcm of the minimal polynomials of alpha^1 .. alpha^2t over the field polynomial get_bch uses
//       (capi.hip), degree P = m t; the byte table of the LFSR, v(x) x^P mod g for the 256 bytes v; and, per code, the cut of the kbch / 8 message
//       bytes into BCH_CHUNKS chunks of `chunk_bytes` (the LAST chunk ends with the message, the first ones may lie in front of it and are empty)
//       with the chunk-shift rows x^(i + 8 chunk_bytes (BCH_CHUNKS - 1 - c)) mod g, i < P, that carry chunk c's residue to the end of the message.
//   LDPC (clause 5.3.2)   per layer i the information-bit links (block column r, rotation sp = (360 - s) % 360) of QC_CODES (ldpc_qc_tables.inc),
//       the decoder plans' source: row j of layer i reads information bit 360 r + (j + sp) % 360.
//   Polynomials are bit vectors of BCH_WORDS 32-bit words, the coefficient of x^k in bit k % 32 of word k / 32.
// Standard headers only: the host tests compile this file with a plain C++ compiler.
#pragma once
#include <cstdint>
#include <vector>
#include "s2_params.h"
#include "ldpc_plan.h"      // QC_CODES (ldpc_qc_tables.inc, which has no include guard of its own)

namespace s2 {
namespace fecenc {

constexpr int BCH_WORDS = 6;            // 192 bits: the largest P (m = 16, t = 12)
constexpr int BCH_CHUNKS = 64;          // one chunk per lane of the wave that encodes a frame
constexpr int BCH_FRAMES_PER_WG = 4;    // a workgroup of the BCH encoder: four waves, a frame each
constexpr int LDPC_FRAMES_PER_WG = 1;   // the LDPC encoder: one frame per workgroup at a time
constexpr int MAX_WORKGROUPS = 2048;    // grid bound of every encoder launch; further frames are taken by the same workgroups in turn
constexpr int BER_CHUNK_FRAMES = 4096;  // the channel-error count re-encodes this many frames at a time (its code-word scratch: 33 MB of normal frames)
constexpr int LDPC_EXT_WORDS = 13;      // a 360-bit block followed by its first 56 bits again: any 32 consecutive bits of the rotated block are two adjacent words

// kbch, K and N of all 21 codes are whole bytes, the parity lengths too: the kernels move bytes
constexpr bool sizes_are_whole_bytes() {
    for (int r = 0; r < RATE_COUNT; ++r) {
        if (KBCH_NORMAL[r] % 8 || NBCH_NORMAL[r] % 8 || NBCH_NORMAL[r] % 360) return false;
        if (r != R9_10 && (KBCH_SHORT[r] % 8 || NBCH_SHORT[r] % 8 || NBCH_SHORT[r] % 360)) return false;
    }
    return 64800 % 8 == 0 && 16200 % 8 == 0;
}
static_assert(sizes_are_whole_bytes(), "kbch, K and N are multiples of 8 (and K of 360) for all 21 codes");

struct Poly { uint32_t w[BCH_WORDS] = {0, 0, 0, 0, 0, 0}; };
inline int poly_bit(const Poly& a, int k) { return (int)((a.w[k >> 5] >> (k & 31)) & 1u); }
inline int poly_degree(const Poly& a) {
    for (int k = 32 * BCH_WORDS - 1; k >= 0; --k) if (poly_bit(a, k)) return k;
    return -1;
}
// a(x) x mod g, for a of degree < P; g_low = g - x^P
inline Poly poly_times_x(const Poly& a, const Poly& g_low, int P) {
    const int carry = poly_bit(a, P - 1);
    Poly r;
    for (int w = BCH_WORDS - 1; w > 0; --w) r.w[w] = (a.w[w] << 1) | (a.w[w - 1] >> 31);
    r.w[0] = a.w[0] << 1;
    if (P < 32 * BCH_WORDS) r.w[P >> 5] &= ~(1u << (P & 31));
    if (carry) for (int w = 0; w < BCH_WORDS; ++w) r.w[w] ^= g_low.w[w];
    return r;
}

struct BchRules {
    int m = 0, t = 0, P = 0;
    std::vector<uint8_t> gen;           // [P + 1] coefficients of g, x^0 first
    Poly g_low;                         // g - x^P
    std::vector<uint32_t> byte_tab;     // [256][BCH_WORDS]: v(x) x^P mod g
};

// g(x) from the field alone: the product of the distinct minimal polynomials of alpha^1 .. alpha^2t
inline BchRules build_bch_rules(int m, int t) {
    BchRules B;
    B.m = m; B.t = t; B.P = m * t;
    const int Q = 1 << m, N = Q - 1;
    const uint32_t field = (m == 16) ? 0x1002Du : 0x402Bu;
    std::vector<uint16_t> LOG(Q), EXP(Q);
    uint32_t a = 1;
    for (int i = 0; i < N; ++i) {
        EXP[i] = (uint16_t)a; LOG[a] = (uint16_t)i;
        a <<= 1;
        if (a & (uint32_t)Q) a ^= field;
    }
    auto mul = [&](uint32_t x, uint32_t y) -> uint32_t { return (!x || !y) ? 0u : EXP[(LOG[x] + LOG[y]) % N]; };
    std::vector<uint32_t> g(1, 1u);                     // coefficients in GF(2^m), x^0 first
    std::vector<char> seen(N, 0);
    for (int i = 1; i <= 2 * t; ++i) {
        if (seen[i % N]) continue;                      // a conjugate of an earlier root: same minimal polynomial
        std::vector<uint32_t> mp(1, 1u);
        for (int e = i % N; !seen[e]; e = (int)((2L * e) % N)) {
            seen[e] = 1;                                // mp *= (x + alpha^e)
            std::vector<uint32_t> nx(mp.size() + 1, 0u);
            for (size_t k = 0; k < mp.size(); ++k) { nx[k + 1] ^= mp[k]; nx[k] ^= mul(mp[k], EXP[e]); }
            mp.swap(nx);
        }
        std::vector<uint32_t> nx(g.size() + mp.size() - 1, 0u);
        for (size_t x = 0; x < g.size(); ++x)
            for (size_t y = 0; y < mp.size(); ++y) nx[x + y] ^= mul(g[x], mp[y]);
        g.swap(nx);
    }
    bool binary = (int)g.size() == B.P + 1;
    for (uint32_t c : g) binary = binary && c <= 1u;
    if (!binary) { B.P = 0; return B; }                 // (cannot happen for the four pairs of the standard; the host test looks)
    B.gen.resize(g.size());
    for (size_t k = 0; k < g.size(); ++k) B.gen[k] = (uint8_t)g[k];
    for (int k = 0; k < B.P; ++k) if (B.gen[k]) B.g_low.w[k >> 5] |= 1u << (k & 31);
    B.byte_tab.assign(256 * BCH_WORDS, 0u);
    for (int v = 0; v < 256; ++v) {
        Poly p;
        p.w[0] = (uint32_t)v;
        for (int k = 0; k < B.P; ++k) p = poly_times_x(p, B.g_low, B.P);
        for (int w = 0; w < BCH_WORDS; ++w) B.byte_tab[(size_t)v * BCH_WORDS + w] = p.w[w];
    }
    return B;
}

struct BchChunkPlan {
    int msg_bytes = 0, chunk_bytes = 0;
    std::vector<int> seams;             // frame bit positions where a chunk that holds message bits begins (the first chunk's own beginning, bit 0, left out)
    std::vector<uint32_t> rows;         // [BCH_CHUNKS][P][BCH_WORDS]
};
// the cut alone, without the rows
inline BchChunkPlan bch_chunk_cut(int kbch) {
    BchChunkPlan C;
    C.msg_bytes = kbch / 8;
    C.chunk_bytes = (C.msg_bytes + BCH_CHUNKS - 1) / BCH_CHUNKS;
    for (int c = 1; c < BCH_CHUNKS; ++c) {
        const int begin = C.msg_bytes - (BCH_CHUNKS - c) * C.chunk_bytes;
        if (begin > 0) C.seams.push_back(8 * begin);
    }
    return C;
}
inline BchChunkPlan build_bch_chunk_plan(const BchRules& B, int kbch) {
    BchChunkPlan C = bch_chunk_cut(kbch);
    C.rows.assign((size_t)BCH_CHUNKS * B.P * BCH_WORDS, 0u);
    Poly base;
    base.w[0] = 1u;                     // x^(8 chunk_bytes (BCH_CHUNKS - 1 - c)) mod g
    for (int c = BCH_CHUNKS - 1; c >= 0; --c) {
        Poly p = base;
        for (int i = 0; i < B.P; ++i) {
            for (int w = 0; w < BCH_WORDS; ++w) C.rows[((size_t)c * B.P + i) * BCH_WORDS + w] = p.w[w];
            p = poly_times_x(p, B.g_low, B.P);
        }
        for (int k = 0; k < 8 * C.chunk_bytes; ++k) base = poly_times_x(base, B.g_low, B.P);
    }
    return C;
}

struct LdpcEncodePlan {
    int N = 0, K = 0, q = 0, blocks = 0;
    std::vector<uint32_t> layer_off;    // [q + 1] first link of a layer
    std::vector<uint32_t> ent;          // links: r << 16 | sp
    // the links of the whole parity-check matrix as QC_CODES counts them: 360 rows per link, and the two parity bits of every row but the first
    int edges() const { return 360 * (int)ent.size() + 2 * (N - K) - 1; }
};
inline LdpcEncodePlan build_ldpc_encode_plan(int code_index) {
    const QcCodeDesc& d = QC_CODES[code_index];
    LdpcEncodePlan L;
    L.N = d.N; L.K = d.K; L.q = d.q; L.blocks = d.K / 360;
    for (int i = 0; i <= d.q; ++i) L.layer_off.push_back((uint32_t)d.off[i]);
    for (int e = 0; e < (int)d.off[d.q]; ++e) {
        const uint32_t r = d.ent[e] >> 16, s = d.ent[e] & 0xffffu;
        L.ent.push_back(r << 16 | (360u - s) % 360u);
    }
    return L;
}

// dvbs2gpu_fec_encode_plan_dump: the numbers a caller (and the tests) may want to know about the kernels' cut of a frame
constexpr int PLAN_COUNTS = 16 + BCH_CHUNKS;
inline void plan_counts(const FecParams& f, const BchChunkPlan& C, const LdpcEncodePlan& L, int32_t* counts) {
    for (int k = 0; k < PLAN_COUNTS; ++k) counts[k] = 0;
    counts[0] = f.bch_m * f.bch_t; counts[1] = BCH_CHUNKS; counts[2] = C.chunk_bytes; counts[3] = BCH_FRAMES_PER_WG; counts[4] = LDPC_FRAMES_PER_WG;
    counts[5] = L.q; counts[6] = (int32_t)L.ent.size(); counts[7] = MAX_WORKGROUPS; counts[8] = BER_CHUNK_FRAMES; counts[9] = (int32_t)C.seams.size();
    for (size_t k = 0; k < C.seams.size(); ++k) counts[16 + k] = C.seams[k];
}

}  // namespace fecenc
}  // namespace s2
