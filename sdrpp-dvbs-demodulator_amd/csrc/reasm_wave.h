// What a wave does with ONE unit of a reassembling bank that decides a row from the unit's leading bytes and takes the CRC-32/MPEG over
// all of them, stated once on top of reasm_pieces (ts_reasm.h): the head gather and the source that the row rules
// read it through (mpe.hip: sections; ule.hip: SNDUs), and the CRC over shares of the pieces (those two and t2mi.hip: T2-MI packets,
// a lane per piece).  Every lane of the wave calls every function.
#pragma once
#include "ts_reasm.h"

namespace s2 {

constexpr int REASM_HEAD = 128;                  // the leading bytes a wave keeps of a unit: two per lane

// a unit's first 128 bytes in a wave, bytes 2 l and 2 l + 1 in lane l: the three-member source of the row rules (mpe_row_fields,
// ule_row_fields, ip_row_fields), a byte read being a shuffle, `any` a ballot and `sum` a wave sum
struct ReasmWaveSrc {
    unsigned h; int lane;
    __device__ unsigned rd(int i) const { return (unsigned)__shfl((int)h, i >> 1) >> (8 * (i & 1)) & 255u; }
    template <typename Fn> __device__ bool any(int n, Fn f) const {
        const bool t = f(lane < n ? lane : 0);
        return __ballot(lane < n && t) != 0;
    }
    template <typename Fn> __device__ unsigned sum(int n, Fn f) const {
        unsigned v = f(lane < n ? lane : 0);
        if (lane >= n) v = 0;
        for (int k = 32; k > 0; k >>= 1) v += (unsigned)__shfl_xor((int)v, k);
        return v;
    }
};

// the head of unit q from the TS payloads where they lie.  The walk is the same in every lane; a piece is read by the lanes it holds
template <typename F>
__device__ inline ReasmWaveSrc reasm_wave_head(const ReasmRec& q, const ReasmView<F>& v, int lane) {
    unsigned h = 0;
    reasm_pieces(q, v, REASM_HEAD, [&](int pos, const uint8_t* src, int len) {
        const int a = 2 * lane - pos;
        if (a >= 0 && a < len) h |= src[a];
        if (a + 1 >= 0 && a + 1 < len) h |= (unsigned)src[a + 1] << 8;
    });
    return {h, lane};
}

// the CRC-32/MPEG register over the `total` bytes of unit q from 0xFFFFFFFF, in every lane: 0 for an intact unit.  Each lane takes the
// CRC of its share of one PIECE (the unit's bytes in one TS payload) from a zero register, shifted to the unit's end, and the wave sums.
// `sub` lanes per piece, 64 / sub pieces a round.  A unit has few pieces (9 at 1416 bytes, 24 at 4096, without adaptation fields): with
// a lane per piece most of the wave would wait for the few lanes that each take 184 bytes, so a piece is cut into `sub` equal shares, as
// many as the pieces expected of `total` leave room for and at most SUB_MAX; units of more pieces (adaptation fields) take further
// rounds.  SUB_MAX 1, a lane per piece, is for units of up to 46 pieces (t2mi.hip)
template <int SUB_MAX = 16, typename F>
__device__ inline uint32_t reasm_wave_crc(const ReasmRec& q, const ReasmView<F>& v, int total, int lane) {
    int sub = SUB_MAX;
    while (sub > 1 && sub * (total / (TSMON_TS - 4) + 2) > 64) sub >>= 1;
    const int per_round = 64 / sub;
    uint32_t x = lane == 0 ? crc32m_mulmod(0xFFFFFFFFu, crc32m_xpow((uint32_t)total)) : 0;
    for (int base = 0;; base += per_round) {
        int idx = 0, ppos = 0, plen = 0;                               // idx: the same in every lane
        const uint8_t* psrc = nullptr;
        const int mine = base + lane / sub;
        reasm_pieces(q, v, total, [&](int pos, const uint8_t* src, int len) {
            if (idx == mine) { ppos = pos; psrc = src; plen = len; }
            ++idx;
        });
        {                                                              // my share of the piece
            const int share = (plen + sub - 1) / sub, a = min((lane % sub) * share, plen), b = min(a + share, plen);
            psrc += a; ppos += a; plen = b - a;
        }
        uint32_t c = 0;
        int i = 0;
        for (; i + 4 <= plen; i += 4) {                                // an unaligned dword inside the piece
            const unsigned d = *reinterpret_cast<const ts_unaligned_u32*>(psrc + i);
            for (int k = 0; k < 4; ++k) c = crc32m_byte(c, d >> (8 * k) & 255);
        }
        for (; i < plen; ++i) c = crc32m_byte(c, psrc[i]);
        if (plen > 0) x ^= crc32m_mulmod(c, crc32m_xpow((uint32_t)(total - ppos - plen)));
        if (idx <= base + per_round) break;
    }
    for (int k = 32; k > 0; k >>= 1) x ^= __shfl_xor(x, k);
    return x;
}

}  // namespace s2
