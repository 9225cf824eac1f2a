// The rules of the DVB-S2 modulator (s2_tx.hip): everything its kernels and the host agree on, stated once.  Code words -> PLFRAME symbols -> 2-sps IQ -> channel.
//
//   PLS code      pls = modcod << 2 | short << 1 | pilots (ETSI EN 302 307-1 clause 5.5.2).  modcod 0 is the dummy PLFRAME: 36 slots of scrambled (1 + j) / sqrt 2,
//                 3330 symbols, no BBFRAME.  MODCODs 29..31 and short 9/10 are refused (s2::modcod_params).
//   sizes         symbols, BBFRAME bytes and code-word bytes of a PLS list and their prefix sums: host arithmetic, no scan on the device.
//   interleaver   clause 5.3.3, the inverse of the engine's de-interleaver (s2_deinterleave_kernel: out[col[c] + j] = in[bits j + c]): bit c of payload symbol j
//                 is code bit col[c] + j, col[c] = c N / bits (8PSK 3/5: columns 2, 1, 0); QPSK: code bit 2 j + 1 - c (the pair swapped).
//   constellation point v = pts[v] * (1 / amp) * (1 / prescale) * norm, three fp32 products in that order, norm = (float)(1 / sqrt(mean power in double)), pts / amp /
//                 prescale from HostConstel (s2_pl_tables.h); the label v is the complemented interleaved bits, MSB first.
//   framing       SOF and PLSC symbols from build_pl_tables; payload and pilots rotated by Rn[i], i = 0 behind each header, the pilot symbols counted; a pilot
//                 block of 36 symbols behind every 16th slot except the last one.
//   pulse         continuous unit-energy RRC evaluated in double, roll-off 0.35 / 0.25 / 0.20, span +-16 symbols, two polyphase branches of 33 fp32 taps
//                 h_p[k] = (float)rrc((p - timing) / 2 - k); sample 2 m + p = the chain of fmaf over k = -16 .. 16, ascending, of h_p[k] and symbol m + k, re and im
//                 separate chains from 0; symbols outside the block are 0, or wrap around (circular).  The order is part of the rule: shape_pair runs in the
//                 kernel and on the host.
//   channel       per sample n of stream s: rotation by phase0 + cfo n (formed and range-reduced in double, then dvbs2m::sincosf_det), AWGN from a counter-based
//                 generator: splitmix64 finaliser of (seed, stream, n), Box-Muller in fp32 (logf_det, sincosf_det, sqrtf); per-dimension sigma =
//                 sqrt(10^(-esn0 / 10)) (Es = 1 at 2 sps behind a unit-energy matched filter), esn0 >= 100 dB: no noise.  A pure function of (seed, stream, n).
// Standard headers, s2_params.h, s2_pl_tables.h and dvbs2gpu_math.h only: the host tests compile this file with a plain C++ compiler.  Nothing here may be
// contracted: only s2_tx.hip calls the float functions below (capi.hip goes through s2_tx.hip's tx_* functions and uses the integer rules alone), and it is
// built with -ffp-contract=off like the receiver's float stages; the fused operations are written out as fmaf.
#pragma once
#include <cmath>
#include <cstdint>
#include <cstring>
#include <vector>
#include "s2_params.h"
#include "s2_pl_tables.h"

#if defined(__HIPCC__)
#define S2TX_HD __host__ __device__ __forceinline__
#define S2TX_UNROLL _Pragma("unroll")
#else
#define S2TX_HD inline
#define S2TX_UNROLL
#endif

namespace s2 {
namespace s2tx {

constexpr int HEADER = 90, SLOT = 90, PILOT_BLOCK = 36, PILOT_EVERY = 16, DUMMY_SLOTS = 36;
constexpr int PILOT_PERIOD = PILOT_EVERY * SLOT;      // payload symbols between two pilot blocks
constexpr int GROUP = 8;                              // payload symbols a lane of the framing kernel makes: one byte per interleaver column
constexpr int FRAME_LANES = 256;
constexpr int MAX_CODE_BYTES = 8100;                  // a normal code word; the kernel stages it in LDS with CODE_PAD bytes of zeros behind it
constexpr int CODE_PAD = 4;
constexpr int FRAMES_PER_LAUNCH = 16;                 // frame descriptors travel as kernel arguments, this many per launch
constexpr int SPAN = 16, TAPS = 2 * SPAN + 1;         // pulse: +-16 symbols
constexpr int SHAPE_TILE = 256;                       // symbols per workgroup of the shaping kernel (+ 2 SPAN of halo)
constexpr float PILOT_IQ = 0.70710678f;               // both components of an unscrambled pilot / dummy symbol

static_assert(PILOT_PERIOD % GROUP == 0 && HEADER % 2 == 0 && PILOT_BLOCK % 2 == 0, "a group of 8 symbols never straddles a pilot block; 16-byte stores stay aligned");

// ---------------------------------------------------------------------------------------------------------------- PLS code, sizes
struct FrameRule {
    int pls = 0, dummy = 0;
    int constel = 0, rate = 0, bits = 0, N = 0, kbch = 0, modcod = 0;
    int payload = 0;            // payload symbols (slots * 90; the dummy frame's 3240 count here too)
    int pilot_blocks = 0;
    int symbols = 0;            // the whole PLFRAME
    int bb_bytes = 0, code_bytes = 0;
    int qpsk = 0, col[5] = {0, 0, 0, 0, 0};     // interleaver: first code bit of column c
    float g1 = 0.f, g2 = 0.f;
    int constel_key = -1;       // one transmit constellation table per key (the PSK tables do not depend on the MODCOD)
    int fec_rate = 0, shortframe = 0;
};

inline bool frame_rule(int pls, FrameRule* out) {
    if (pls < 0 || pls > 127) return false;
    FrameRule R;
    R.pls = pls;
    if ((pls >> 2) == 0) {
        R.dummy = 1; R.payload = DUMMY_SLOTS * SLOT; R.symbols = HEADER + R.payload;
        *out = R;
        return true;
    }
    ModcodParams mp;
    if (!modcod_params(pls >> 2, (pls >> 1) & 1, pls & 1, &mp)) return false;
    R.constel = mp.constel; R.rate = mp.rate; R.bits = mp.bits; R.N = mp.fec.N; R.kbch = mp.fec.kbch; R.modcod = mp.modcod;
    R.payload = mp.slots * SLOT; R.pilot_blocks = mp.pilot_blocks; R.symbols = mp.plframe;
    R.bb_bytes = mp.fec.kbch / 8; R.code_bytes = mp.fec.N / 8;
    R.qpsk = mp.constel == C_QPSK;
    const int rows = mp.fec.N / mp.bits;
    for (int c = 0; c < mp.bits; ++c) R.col[c] = rows * c;
    if (mp.constel == C_8PSK && mp.rate == R3_5) { R.col[0] = 2 * rows; R.col[1] = rows; R.col[2] = 0; }
    R.g1 = mp.g1; R.g2 = mp.g2;
    R.constel_key = mp.constel >= C_16APSK ? 100 + mp.modcod : mp.constel;
    R.fec_rate = mp.rate; R.shortframe = mp.shortframe;
    *out = R;
    return true;
}

// the sizes of a PLS list and where each frame begins (prefix sums; each vector gets nframes + 1 entries when given).  false: frame *bad has no valid PLS code
struct ListSizes { long long symbols = 0, bb_bytes = 0, code_bytes = 0; };
inline bool list_sizes(const int32_t* pls, int nframes, ListSizes* total, int* bad = nullptr, std::vector<long long>* sym_off = nullptr,
                       std::vector<long long>* bb_off = nullptr, std::vector<long long>* code_off = nullptr) {
    ListSizes S;
    for (int f = 0; f < nframes; ++f) {
        FrameRule R;
        if (!frame_rule(pls[f], &R)) { if (bad) *bad = f; return false; }
        if (sym_off) sym_off->push_back(S.symbols);
        if (bb_off) bb_off->push_back(S.bb_bytes);
        if (code_off) code_off->push_back(S.code_bytes);
        S.symbols += R.symbols; S.bb_bytes += R.bb_bytes; S.code_bytes += R.code_bytes;
    }
    if (sym_off) sym_off->push_back(S.symbols);
    if (bb_off) bb_off->push_back(S.bb_bytes);
    if (code_off) code_off->push_back(S.code_bytes);
    *total = S;
    return true;
}

// ---------------------------------------------------------------------------------------------------------------- interleaver, mapper, PL scrambling
// the code bit that becomes bit c (MSB first) of payload symbol j
S2TX_HD int code_bit_of(int qpsk, const int* col, int j, int c) { return qpsk ? 2 * j + 1 - c : col[c] + j; }

// 8 consecutive code bits from bit `off` on, MSB first; reads the byte behind the last one too (CODE_PAD)
S2TX_HD uint32_t bits8(const uint8_t* code, int off) {
    const uint32_t two = (uint32_t)code[off >> 3] << 8 | (uint32_t)code[(off >> 3) + 1];
    return (two >> (8 - (off & 7))) & 0xffu;
}

// the labels of payload symbols 8 g .. 8 g + 7: one byte per column (QPSK: the two bytes that hold the eight swapped pairs), complemented
S2TX_HD void group_labels(const uint8_t* code, int qpsk, int bits, const int* col, int g, uint32_t v[GROUP]) {
    if (qpsk) {
        const uint32_t w = ~((uint32_t)code[2 * g] << 8 | (uint32_t)code[2 * g + 1]);
S2TX_UNROLL
        for (int k = 0; k < GROUP; ++k) {
            const uint32_t pair = (w >> (14 - 2 * k)) & 3u;     // code bit 2 j, code bit 2 j + 1
            v[k] = (pair & 1u) << 1 | pair >> 1;
        }
        return;
    }
S2TX_UNROLL
    for (int k = 0; k < GROUP; ++k) v[k] = 0;
S2TX_UNROLL
    for (int c = 0; c < 5; ++c) {           // (written out over the five possible columns: col[] and the shifts stay in registers)
        if (c >= bits) break;
        const uint32_t B = ~bits8(code, col[c] + GROUP * g);
S2TX_UNROLL
        for (int k = 0; k < GROUP; ++k) v[k] |= ((B >> (7 - k)) & 1u) << (bits - 1 - c);
    }
}

// PL scrambling: multiplication by j^r, the inverse of the receiver's descrambler
S2TX_HD cf32 pl_rotate(cf32 p, int r) {
    switch (r) {
        case 3: return cf32{p.im, -p.re};
        case 2: return cf32{-p.re, -p.im};
        case 1: return cf32{-p.im, p.re};
        default: return p;
    }
}

// where payload symbol p sits in its PLFRAME; its scrambler index is that position - HEADER
S2TX_HD int payload_pos(int p, int pilot_blocks) { return HEADER + p + (pilot_blocks ? PILOT_BLOCK * (p / PILOT_PERIOD) : 0); }
// ... and symbol k of pilot block b
S2TX_HD int pilot_pos(int b, int k) { return HEADER + (b + 1) * PILOT_PERIOD + b * PILOT_BLOCK + k; }

// the transmit constellation: 32 entries, those behind `states` zero
inline void tx_constellation(int constel, float g1, float g2, cf32 tab[32]) {
    const HostConstel H(constel, g1, g2);
    const float inv_amp = 1.0f / H.amp, inv_pre = 1.0f / H.prescale;
    cf32 m[32];
    double pw = 0;
    for (int v = 0; v < H.states; ++v) {
        m[v] = HostConstel::scale(HostConstel::scale(H.pts[v], inv_amp), inv_pre);
        pw += (double)m[v].re * m[v].re + (double)m[v].im * m[v].im;
    }
    const float norm = (float)(1.0 / std::sqrt(pw / H.states));
    for (int v = 0; v < 32; ++v) tab[v] = v < H.states ? HostConstel::scale(m[v], norm) : cf32{0.f, 0.f};
}

struct HostTables {
    std::vector<cf32> sof, plsc;
    std::vector<uint64_t> codes;
    std::vector<uint8_t> rn;
    HostTables() { build_pl_tables(sof, plsc, codes, rn); }
};

// one PLFRAME on the host, the way the kernel makes it.  code: R.code_bytes bytes (none for a dummy frame); out: R.symbols
inline void host_frame(const FrameRule& R, const HostTables& T, const cf32* tab, const uint8_t* code, cf32* out) {
    for (int i = 0; i < 26; ++i) out[i] = T.sof[i];
    for (int i = 0; i < 64; ++i) out[26 + i] = T.plsc[(size_t)R.pls * 64 + i];
    const cf32 pilot{PILOT_IQ, PILOT_IQ};
    if (R.dummy) {
        for (int i = 0; i < R.payload; ++i) out[HEADER + i] = pl_rotate(pilot, T.rn[i]);
        return;
    }
    std::vector<uint8_t> padded((size_t)R.code_bytes + CODE_PAD, 0);
    memcpy(padded.data(), code, (size_t)R.code_bytes);
    for (int g = 0; g * GROUP < R.payload; ++g) {
        uint32_t v[GROUP];
        group_labels(padded.data(), R.qpsk, R.bits, R.col, g, v);
        for (int k = 0; k < GROUP && g * GROUP + k < R.payload; ++k) {
            const int pos = payload_pos(g * GROUP + k, R.pilot_blocks);
            out[pos] = pl_rotate(tab[v[k]], T.rn[pos - HEADER]);
        }
    }
    for (int b = 0; b < R.pilot_blocks; ++b)
        for (int k = 0; k < PILOT_BLOCK; ++k) {
            const int pos = pilot_pos(b, k);
            out[pos] = pl_rotate(pilot, T.rn[pos - HEADER]);
        }
}

// ---------------------------------------------------------------------------------------------------------------- pulse
inline bool rolloff_ok(double r) { return r == 0.35 || r == 0.25 || r == 0.20; }

// unit-energy root-raised-cosine pulse, t in symbols
inline double rrc(double t, double beta) {
    const double PI = 3.14159265358979323846;
    if (std::fabs(t) < 1e-9) return 1.0 + beta * (4.0 / PI - 1.0);
    if (std::fabs(std::fabs(t) - 1.0 / (4.0 * beta)) < 1e-9)
        return (beta / std::sqrt(2.0)) * ((1.0 + 2.0 / PI) * std::sin(PI / (4.0 * beta)) + (1.0 - 2.0 / PI) * std::cos(PI / (4.0 * beta)));
    const double x = 4.0 * beta * t;
    return (std::sin(PI * t * (1.0 - beta)) + x * std::cos(PI * t * (1.0 + beta))) / (PI * t * (1.0 - x * x));
}

struct Taps { float h[2][TAPS]; };      // h[p][k + SPAN]; a kernel argument
inline Taps make_taps(double rolloff, double timing) {
    Taps H;
    for (int p = 0; p < 2; ++p)
        for (int k = -SPAN; k <= SPAN; ++k) H.h[p][k + SPAN] = (float)rrc(((double)p - timing) / 2.0 - (double)k, rolloff);
    return H;
}

// samples 2 m and 2 m + 1: get(k) is symbol m + k (0, or the wrapped one, outside the block)
template <typename Get>
S2TX_HD void shape_pair(const Taps& H, Get get, float out[4]) {
    float r0 = 0.f, i0 = 0.f, r1 = 0.f, i1 = 0.f;
S2TX_UNROLL
    for (int k = -SPAN; k <= SPAN; ++k) {
        const cf32 s = get(k);
        r0 = __builtin_fmaf(H.h[0][k + SPAN], s.re, r0);
        i0 = __builtin_fmaf(H.h[0][k + SPAN], s.im, i0);
        r1 = __builtin_fmaf(H.h[1][k + SPAN], s.re, r1);
        i1 = __builtin_fmaf(H.h[1][k + SPAN], s.im, i1);
    }
    out[0] = r0; out[1] = i0; out[2] = r1; out[3] = i1;
}

// symbol i of a block of ns as the shaping stage sees it
S2TX_HD long long wrap_index(long long i, long long ns) { return ((i % ns) + ns) % ns; }

inline void host_shape(const cf32* sym, long long ns, const Taps& H, int circular, cf32* iq) {
    for (long long m = 0; m < ns; ++m) {
        float o[4];
        shape_pair(H, [&](int k) -> cf32 {
            long long i = m + k;
            if (circular) i = wrap_index(i, ns);
            else if (i < 0 || i >= ns) return cf32{0.f, 0.f};
            return sym[i];
        }, o);
        iq[2 * m] = cf32{o[0], o[1]};
        iq[2 * m + 1] = cf32{o[2], o[3]};
    }
}

// ---------------------------------------------------------------------------------------------------------------- channel
struct ChanParams {         // one stream's entry of the device table
    double cfo, phase0;
    uint64_t key;           // of (seed, stream)
    float sigma;            // per dimension; 0: no noise
    int rotate;             // 0: cfo and phase0 are both 0, the samples pass unrotated
};

S2TX_HD uint64_t mix64(uint64_t z) {        // the splitmix64 finaliser
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
constexpr uint64_t GOLDEN = 0x9E3779B97F4A7C15ull;

inline ChanParams chan_params(double esn0_db, double cfo, double phase0, uint64_t seed, long long stream) {
    ChanParams P;
    P.cfo = cfo; P.phase0 = phase0;
    P.key = mix64(mix64(seed + GOLDEN) + GOLDEN * ((uint64_t)stream + 1u));
    P.sigma = esn0_db >= 100.0 ? 0.f : (float)std::sqrt(std::pow(10.0, -esn0_db / 10.0));
    P.rotate = cfo != 0.0 || phase0 != 0.0;
    return P;
}

S2TX_HD cf32 chan_sample(const ChanParams& P, long long n, cf32 x) {
    if (P.rotate) {
        double ph = P.phase0 + P.cfo * (double)n;
        ph = ph - 6.283185307179586476925 * __builtin_rint(ph * 0.1591549430918953357689);
        float sn, cs;
        dvbs2m::sincosf_det((float)ph, &sn, &cs);
        const float re = __builtin_fmaf(x.re, cs, -(x.im * sn)), im = __builtin_fmaf(x.re, sn, x.im * cs);
        x = cf32{re, im};
    }
    if (P.sigma > 0.f) {
        const uint64_t a = mix64(P.key + GOLDEN * (2u * (uint64_t)n + 1u)), b = mix64(P.key + GOLDEN * (2u * (uint64_t)n + 2u));
        const float u1 = (float)((uint32_t)(a >> 40) + 1u) * 5.9604644775390625e-8f;       // (0, 1], 24 bits: exact
        const float u2 = (float)(uint32_t)(b >> 40) * 5.9604644775390625e-8f;              // [0, 1)
        const float radius = __builtin_sqrtf(-2.0f * dvbs2m::logf_det(u1));
        float sn, cs;
        dvbs2m::sincosf_det(6.28318530717958647692f * u2, &sn, &cs);
        x = cf32{__builtin_fmaf(P.sigma, radius * cs, x.re), __builtin_fmaf(P.sigma, radius * sn, x.im)};
    }
    return x;
}

inline void host_channel(const ChanParams& P, cf32* iq, long long nsamples) {
    for (long long n = 0; n < nsamples; ++n) iq[n] = chan_sample(P, n, iq[n]);
}

}  // namespace s2tx
}  // namespace s2
