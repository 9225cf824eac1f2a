// What the IP-TS bank (ipts.hip) and the IP output bank (ipout.hip) share on the device: the ones'-complement byte sums of
// a stretch of memory and its copy, by a group of nl lanes of a wave (64: the whole wave; ipout.hip gives each TS packet of a datagram
// 8 lanes).  16-byte accesses between a byte-wise lead-in up to a 16-byte boundary and a byte-wise tail.
#pragma once
#include "ts_reasm.h"

namespace s2 {

// This lane's share (lane of nl) of the sums of the bytes of [q, q + len): *even += those at even places, *odd += those at odd places; the sum
// of the big-endian words is 256 even + odd.  len < 65536: even <= 32768 * 255, so the total fits 32 bits, and a lane's share of it all
// the more.  The bytes at even and at odd ADDRESSES are summed apart, so that an odd lead-in only swaps them
__device__ inline void ip_lanes_wsum(const uint8_t* q, int len, int lane, int nl, unsigned* even, unsigned* odd) {
    int lead = (int)((16 - (reinterpret_cast<uintptr_t>(q) & 15)) & 15);
    if (lead > len) lead = len;
    const int nvec = (len - lead) / 16, tail = lead + 16 * nvec;
    unsigned a = 0, b = 0;                         // of the 16-byte loads: the bytes at even and at odd ADDRESSES
    const uint4* qv = reinterpret_cast<const uint4*>(q + lead);
    for (int i = lane; i < nvec; i += nl) {
        const uint4 x = qv[i];
        const unsigned d[4] = {x.x, x.y, x.z, x.w};
        for (int k = 0; k < 4; ++k) {
            const unsigned lo = d[k] & 0x00FF00FFu, hi = d[k] >> 8 & 0x00FF00FFu;
            a += (lo & 0xFFFF) + (lo >> 16); b += (hi & 0xFFFF) + (hi >> 16);
        }
    }
    unsigned e = lead & 1 ? b : a, o = lead & 1 ? a : b;
    for (int i = lane; i < lead; i += nl) { if (i & 1) o += q[i]; else e += q[i]; }
    for (int i = tail + lane; i < len; i += nl) { if (i & 1) o += q[i]; else e += q[i]; }
    *even += e; *odd += o;
}

// the lanes' shares over the wave: the sum of the words, not folded
__device__ inline unsigned ip_wave_wsum_reduce(unsigned even, unsigned odd) {
    for (int k = 32; k > 0; k >>= 1) { even += (unsigned)__shfl_xor((int)even, k); odd += (unsigned)__shfl_xor((int)odd, k); }
    return (even << 8) + odd;
}

// n bytes from s to d by nl lanes: where the two agree modulo 16, 16-byte accesses between a byte-wise lead-in and tail; else a dword
// per lane behind d's unaligned head (ts_wave_copy's form)
__device__ inline void ip_lanes_copy(uint8_t* d, const uint8_t* s, int n, int lane, int nl) {
    if ((reinterpret_cast<uintptr_t>(d) ^ reinterpret_cast<uintptr_t>(s)) & 15) {
        int head = (int)((4 - (reinterpret_cast<uintptr_t>(d) & 3)) & 3);
        if (head > n) head = n;
        const int nd = (n - head) / 4, tail = head + 4 * nd;
        for (int i = lane; i < head; i += nl) d[i] = s[i];
        for (int i = lane; i < nd; i += nl) *reinterpret_cast<unsigned*>(d + head + 4 * i) = TsBytes{s}.u32(head + 4 * i);
        for (int i = tail + lane; i < n; i += nl) d[i] = s[i];
        return;
    }
    int lead = (int)((16 - (reinterpret_cast<uintptr_t>(d) & 15)) & 15);
    if (lead > n) lead = n;
    const int nvec = (n - lead) / 16, tail = lead + 16 * nvec;
    for (int i = lane; i < lead; i += nl) d[i] = s[i];
    for (int i = lane; i < nvec; i += nl) reinterpret_cast<uint4*>(d + lead)[i] = reinterpret_cast<const uint4*>(s + lead)[i];
    for (int i = tail + lane; i < n; i += nl) d[i] = s[i];
}

}  // namespace s2
