// Host-side builders of the DVB-S2 physical-layer tables, shared by the receiver (s2_demod.hip) and the modulator (s2_tx_rules.h): the
// constellation points with the soft demapper of the reference, and SOF / PLSC / Gold sequence.  (The CPU oracle builds the same tables
// independently in oracle/s2chain.cpp.)  Standard headers and dvbs2gpu_math.h only: the host tests compile this file with a plain C++ compiler.
// Many translation units see this file (s2_rx.h takes cf32 from it), but only s2_demod.hip and s2_tx.hip may CALL its float builders: those two
// are built with -ffp-contract=off (csrc/Makefile), the others are not, and an inline function instantiated in one of them would round
// differently.  A new caller belongs in one of those two files, or gets its own line in that Makefile rule.
#pragma once
#include <cmath>
#include <cstdint>
#include <limits>
#include <vector>
#include "../../include/dvbs2gpu_math.h"
#include "s2_params.h"

namespace s2 {

struct cf32 { float re, im; };

struct HostConstel {
    int constel, bits, states;
    float amp = 1.0f, sca = 50.0f, prescale = 1.0f;
    cf32 pts[32];
    static cf32 polar(float r, int n, float i) {
        float a = i * 2 * M_PI / n, sn, cs;
        dvbs2m::sincosf_det(a, &sn, &cs);
        return cf32{r * cs, r * sn};
    }
    static cf32 scale(cf32 a, float s) { return cf32{a.re * s, a.im * s}; }
    HostConstel(int type, float g1, float g2) : constel(type) {   // constellation.cpp:19-150
        const double SQ2 = 1.41421356237309504880;
        if (type == C_QPSK) {
            states = 4; bits = 2; amp = 3;
            pts[0] = cf32{(float)-SQ2, (float)-SQ2}; pts[1] = cf32{(float)SQ2, (float)-SQ2};
            pts[2] = cf32{(float)-SQ2, (float)SQ2}; pts[3] = cf32{(float)SQ2, (float)SQ2};
        } else if (type == C_8PSK) {
            states = 8; bits = 3;
            float r = 0.70710678118654752440;
            const cf32 p[8] = {{0.0f, -1.0f}, {-r, r}, {r, -r}, {0.0f, 1.0f}, {-r, -r}, {-1.0f, 0.0f}, {1.0f, 0.0f}, {r, r}};
            for (int i = 0; i < 8; ++i) pts[i] = p[i];
        } else if (type == C_16APSK) {
            states = 16; bits = 4; amp = 100; sca = 1; prescale = 0.53;
            float gamma1 = g1 ? g1 : 2.57f;
            float r1 = sqrtf(4 / (1 + 3 * gamma1 * gamma1));
            float r2 = gamma1 * r1;
            r1 *= 0.5; r2 *= 0.5;
            const float inner[4] = {2.5f, 1.5f, 3.5f, 0.5f};
            const float outer[12] = {8.5f, 3.5f, 9.5f, 2.5f, 6.5f, 5.5f, 11.5f, 0.5f, 7.5f, 4.5f, 10.5f, 1.5f};
            for (int i = 0; i < 4; ++i) pts[i] = scale(polar(r1, 4, inner[i]), amp);
            for (int i = 0; i < 12; ++i) pts[4 + i] = scale(polar(r2, 12, outer[i]), amp);
        } else {
            states = 32; bits = 5; amp = 100; sca = 1; prescale = 0.54;
            float gamma1 = g1 ? g1 : 2.53f, gamma2 = g2 ? g2 : 4.30f;
            float r1 = sqrtf(8 / (1 + 3 * gamma1 * gamma1 + 4 * gamma2 * gamma2));
            float r2 = gamma1 * r1, r3 = gamma2 * r1;
            r1 *= 0.5; r2 *= 0.5; r3 *= 0.5;
            struct P { int ring, n; float i; };
            const P tab[32] = {{3, 16, 10}, {3, 16, 8}, {3, 16, 5}, {3, 16, 7}, {3, 16, 13}, {3, 16, 15}, {3, 16, 2}, {3, 16, 0},
                               {1, 4, 2.5f}, {2, 12, 6.5f}, {1, 4, 1.5f}, {2, 12, 5.5f}, {1, 4, 3.5f}, {2, 12, 11.5f}, {1, 4, 0.5f}, {2, 12, 0.5f},
                               {3, 16, 11}, {3, 16, 9}, {3, 16, 4}, {3, 16, 6}, {3, 16, 12}, {3, 16, 14}, {3, 16, 3}, {3, 16, 1},
                               {2, 12, 8.5f}, {2, 12, 7.5f}, {2, 12, 3.5f}, {2, 12, 4.5f}, {2, 12, 9.5f}, {2, 12, 10.5f}, {2, 12, 2.5f}, {2, 12, 1.5f}};
            for (int i = 0; i < 32; ++i) {
                float r = tab[i].ring == 1 ? r1 : (tab[i].ring == 2 ? r2 : r3);
                pts[i] = scale(polar(r, tab[i].n, tab[i].i), amp);
            }
        }
    }
    static int8_t clampv(float x) { return dvbs2m::llr_clamp_det(x); }   // constellation.cpp:263-270
    void soft_calc(cf32 sample, int8_t* bits_out, float* phase_err) const {   // constellation.cpp:205-261
        float tmp[10] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
        if (amp != 1) sample = scale(sample, amp);
        if (prescale != 1) sample = scale(sample, prescale);
        float min_dist = std::numeric_limits<float>::max();
        cf32 closest{0, 0};
        for (int i = 0; i < states; i++) {
            float dre = sample.re - pts[i].re, dim = sample.im - pts[i].im;
            float dist = sqrtf(dre * dre + dim * dim);
            if (dist < min_dist) { min_dist = dist; closest = pts[i]; }
            float d = dvbs2m::expf_det(-dist / 1.0f);
            for (int j = 0; j < bits; j++) {
                if (((i >> j) & 1) == 0) tmp[2 * j + 0] += d;
                else tmp[2 * j + 1] += d;
            }
        }
        for (int i = 0; i < bits; i++) bits_out[bits - 1 - i] = clampv((dvbs2m::logf_det(tmp[2 * i + 1]) - dvbs2m::logf_det(tmp[2 * i + 0])) * sca);
        // sample * conj(closest)
        float pre = sample.re * closest.re - sample.im * (-closest.im), pim = sample.im * closest.re + sample.re * (-closest.im);
        *phase_err = dvbs2m::atan2f_det(pim, pre);
    }
};

// SOF / PLSC / Gold sequence (s2_defs.h:15-80, s2_scrambling.cpp:9-28), on the host: what get_rx_tables uploads and dvbs2gpu_pl_tables_dump hands out
inline void build_pl_tables(std::vector<cf32>& sof, std::vector<cf32>& plsc, std::vector<uint64_t>& codes, std::vector<uint8_t>& rn) {
    sof.assign(26, cf32{0.f, 0.f}); plsc.assign(128 * 64, cf32{0.f, 0.f}); codes.assign(128, 0);
    const uint32_t VALUE = 0x18d2e82;
    for (int s = 0; s < 26; ++s) {
        int bit = (VALUE >> (25 - s)) & 1, angle = bit * 2 + (s & 1);
        dvbs2m::sincosf_det((float)(M_PI / 4 + 2 * M_PI * angle / 4), &sof[s].im, &sof[s].re);
    }
    const uint32_t G[6] = {0x55555555, 0x33333333, 0x0f0f0f0f, 0x00ff00ff, 0x0000ffff, 0xffffffff};
    const uint64_t SCR = 0x719d83c953422dfaull;
    for (int index = 0; index < 128; ++index) {
        uint32_t y = 0;
        for (int row = 0; row < 6; ++row)
            if ((index >> (6 - row)) & 1) y ^= G[row];
        uint64_t code = 0;
        for (int bit = 31; bit >= 0; --bit) {
            int yi = (y >> bit) & 1;
            code = (code << 2) | ((uint64_t)yi << 1) | (uint64_t)((index & 1) ? (yi ^ 1) : yi);
        }
        code ^= SCR;
        codes[index] = code;
        for (int i = 0; i < 64; ++i) {
            int yi = (code >> (63 - i)) & 1, nyi = yi ^ (i & 1);
            plsc[index * 64 + i].re = (1 - 2 * nyi) / sqrtf(2);
            plsc[index * 64 + i].im = (1 - 2 * yi) / sqrtf(2);
        }
    }
    rn.assign(131072, 0);
    auto lfsr_x = [](uint32_t X) { int bit = ((X >> 7) ^ X) & 1; return ((uint32_t)(bit << 18) | X) >> 1; };
    auto lfsr_y = [](uint32_t Y) { int bit = ((Y >> 10) ^ (Y >> 7) ^ (Y >> 5) ^ Y) & 1; return ((uint32_t)(bit << 18) | Y) >> 1; };
    uint32_t stx = 0x00001, sty = 0x3ffff;
    for (int i = 0; i < 131072; ++i) { rn[i] = (uint8_t)((stx ^ sty) & 1); stx = lfsr_x(stx); sty = lfsr_y(sty); }
    for (int i = 0; i < 131072; ++i) { rn[i] |= (uint8_t)(((stx ^ sty) & 1) << 1); stx = lfsr_x(stx); sty = lfsr_y(sty); }
}

}  // namespace s2
