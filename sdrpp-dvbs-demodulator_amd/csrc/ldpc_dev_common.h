// What the three LDPC decoder kernels share (ldpc_kernel.hip: lane = row; ldpc_split_kernel.hip: two lanes = row; ldpc_wave_kernel.hip: wave = frame), i.e. everything but
// the layout of a sweep over lanes: the launch arguments and how a launch is made, the int8 rules of the reference's SIMD lanes, the bit-vector form of its syndrome check,
// and a frame's way in and out (load, verdict after a check, outputs).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "kernels.h"

namespace s2 {

// Code tables are separate `const T* __restrict__` kernel parameters (not struct members) so that hipcc can
// prove them invariant and fetch the wave-uniform layer/link descriptors with scalar loads (s_load_*).
struct LdpcKernelArgs {
    const int8_t* llr;     // [nframes][N]
    uint8_t* hard;         // [nframes][hard_stride] packed hard decisions of bits [0,K), MSB first
    int8_t* post;          // optional [nframes][N] posteriors (reference layout), may be null
    int32_t* trials;       // [nframes]
    uint32_t* msg_ws;      // [gridDim.x * slots][message records of a slot: LdpcGeometry::rec_bytes]
    int nframes, N, K, R, q;
    int pent_base;         // offset of the pair-format link table inside ents[] (ldpc_plan.h); half-row decoder: message words per workgroup
    int synd_base;         // offset of the syndrome-check table inside ents[] (ldpc_plan.h)
    int max_trials, force;
    int hard_stride;
    int dbg;                    // tests only (context option ldpc_split_fail_attempts): 1 = every attempt of the half-row decoder's layers with shared bits is made to fail (the fall-back path)
    uint32_t* sgn_ws;           // [gridDim.x * slots][SGN_WS_DWORDS]: bit-packed posterior signs for the syndrome check
    unsigned int* work_ctr;     // optional: frames beyond the first gridDim.x * slots are claimed dynamically (workgroups slowed by
                                // co-resident kernels of the pipelined mode then simply take fewer frames)
    unsigned long long* prof;   // development aid (-DLDPC_PROF builds only): per-wave phase cycle sums of workgroup 0
};

// ---- host side of a launch (kernels.h: LdpcJob): the arguments, the dynamic-LDS attribute + launch, the occupancy query
inline hipError_t ldpc_kernel_args(const LdpcDeviceCode& C, const LdpcJob& J, LdpcKernelArgs* A) {
    if (J.work_ctr) {
        hipError_t e = hipMemsetAsync(J.work_ctr, 0, sizeof(unsigned int), J.stream);
        if (e != hipSuccess) return e;
    }
    A->llr = J.llr; A->hard = J.hard; A->post = J.post; A->trials = J.trials; A->msg_ws = J.msg_ws;
    A->nframes = J.nframes; A->N = C.N; A->K = C.K; A->R = C.R; A->q = C.q; A->pent_base = C.pent_base; A->synd_base = C.synd_base;
    A->max_trials = J.max_trials; A->force = J.force; A->hard_stride = J.hard_stride; A->dbg = J.dbg;
    A->sgn_ws = J.sgn_ws; A->work_ctr = J.work_ctr; A->prof = g_ldpc_prof;
    return hipSuccess;
}
template <typename Kern, typename... KArgs>
hipError_t ldpc_launch(Kern kern, int grid, int threads, size_t lds, hipStream_t stream, const KArgs&... args) {
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(kern, dim3(grid), dim3(threads), lds, stream, args...);
    return hipGetLastError();
}
template <typename Kern>
int ldpc_occupancy(Kern kern, int threads, size_t lds) {
    int nb = 0;
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, kern, threads, lds) != hipSuccess) nb = 1;
    return nb < 1 ? 1 : nb;
}

__device__ __forceinline__ int med3i(int a, int lo, int hi) { return min(max(a, lo), hi); }  // folds to v_med3_i32 for lo <= hi
__device__ __forceinline__ int clamp8(int v) { return med3i(v, -128, 127); }

// |max(x,-127)| - 1 clamped at 0  == vqsub(vunsigned(vqabs(x)), 1)   (algorithms.hh:235-238)
__device__ __forceinline__ int mag_of(int in) {
    int a = in < 0 ? -in : in;
    return med3i(a - 1, 0, 126);
}


typedef unsigned short u16x2 __attribute__((ext_vector_type(2)));
// ---- packed int16 helpers: two links per VALU instruction (v_pk_*_i16), the int8 saturation rules emulated in 16 bits
typedef short s16x2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ s16x2 splat2(int v) { return s16x2{(short)v, (short)v}; }
__device__ __forceinline__ s16x2 pmin2(s16x2 a, s16x2 b) { return __builtin_elementwise_min(a, b); }
__device__ __forceinline__ s16x2 pmax2(s16x2 a, s16x2 b) { return __builtin_elementwise_max(a, b); }
__device__ __forceinline__ s16x2 pclamp2(s16x2 v, int lo, int hi) { return pmin2(pmax2(v, splat2(lo)), splat2(hi)); }
__device__ __forceinline__ uint32_t bits2(s16x2 v) { return __builtin_bit_cast(uint32_t, v); }
__device__ __forceinline__ s16x2 from_bits2(uint32_t v) { return __builtin_bit_cast(s16x2, v); }
// The packed row arithmetic works on values scaled by 256 ("Q8": the int8 quantity sits in the HIGH byte of each 16-bit half):
// the 16-bit saturating add/subtract of the hardware (v_pk_add_i16 / v_pk_sub_i16 with clamp) then IS the int8 saturation of the
// reference's SIMD lanes, and message bytes drop into place with one v_perm, no sign extension.  Only the high byte of a half
// is ever consumed (a positive saturation leaves 0xff below it).  Magnitude sentinel ("no link"): 127 (real ones are <= 126).
constexpr int Q8_NONE = 127 << 8;
__device__ __forceinline__ s16x2 q8(int v) { return s16x2{(short)(v << 8), (short)(v << 8)}; }
__device__ __forceinline__ s16x2 sat_sub2(s16x2 a, s16x2 b) { return __builtin_elementwise_sub_sat(a, b); }
__device__ __forceinline__ s16x2 sat_add2(s16x2 a, s16x2 b) { return __builtin_elementwise_add_sat(a, b); }
// message bytes k, k+1 (k even) of a record into the high bytes of the two halves: one v_perm
__device__ __forceinline__ s16x2 rec_pair_dw(uint32_t w, int k) {
    return from_bits2((k & 2) ? __builtin_amdgcn_perm(0u, w, 0x030c020cu) : __builtin_amdgcn_perm(0u, w, 0x010c000cu));
}
template <int REC>
__device__ __forceinline__ s16x2 rec_pair(const uint32_t (&rec)[REC], int k) { return rec_pair_dw(rec[k >> 2], k); }


// LDPCDecoder::bad (layered_decoder.hh:28-45): true if any row is unsatisfied.  A row is bad when the sign product of its links'
// posteriors is negative or when one of them is 0.  Every posterior belongs to at least one row (each parity bit to its own row), so the
// second condition over all rows is "some posterior of the frame is 0": a dword scan shared by the slot's 384 threads.  The first one is
// evaluated on BIT VECTORS: the code is quasi-cyclic, so the 360 sign products of layer i are
//     Y_i = P_i ^ P'_i ^ XOR_k rot(S_{r_k}, sp_k)            (S_r: signs of information group r, P_i: of parity group i)
// -- XORs of cyclic shifts of 360-bit groups: ~15 shifted 64-bit fetches per (layer, 64-row word) instead of 15 byte gathers per row
// (227 k LDS byte reads per check before).  Step 1 (sign_pack): every thread turns 8 posteriors into one sign byte (and scans them for
// zeros); a group is stored as 360 bits followed by a copy of its first 64, so a shifted fetch never wraps; the 10 KB per frame go to a
// per-slot global scratch (L2-resident; LDS has no room for them beside two frames and the co-resident front-end kernels).  Step 2
// (syndromes_bad), after a workgroup barrier: lane t takes (layer, word) = (t / 6, t % 6).
constexpr int SGN_GROUP_DW = 14;                                  // 56 bytes: 360 bits + the first 64 again (424), padded to dwords
constexpr int SGN_WS_DWORDS = 180 * SGN_GROUP_DW + 16;            // per slot (N/360 <= 180 groups)

__device__ __forceinline__ uint32_t sign_pack(const int8_t* __restrict__ post, int N, uint8_t* __restrict__ sg, int j, int tps) {
    const uint2* __restrict__ p8 = reinterpret_cast<const uint2*>(post);
    uint32_t z = 0;
    for (int idx = j; idx < N / 8; idx += tps) {
        const uint2 v = p8[idx];
        z |= ((v.x - 0x01010101u) & ~v.x) | ((v.y - 0x01010101u) & ~v.y);   // bit 7 of a byte set <=> that byte is 0 (or a borrow from a zero byte below: still "a zero")
        // sign bits 7, 15, 23, 31 of a dword -> one nibble, LSB = lowest byte (the multiply adds four shifted copies; no two terms collide)
        const uint32_t lo = ((((v.x >> 7) & 0x01010101u) * 0x01020408u) >> 24);
        const uint32_t hi = ((((v.y >> 7) & 0x01010101u) * 0x01020408u) >> 24);
        const uint32_t sb = lo | (hi << 4);
        const int g = (int)((uint32_t)idx / 45u);
        const int o = idx - 45 * g;
        uint8_t* __restrict__ d = sg + (SGN_GROUP_DW * 4) * g + o;
        d[0] = (uint8_t)sb;
        if (o < 8) d[45] = (uint8_t)sb;                                       // cyclic extension: bits 360..423 = bits 0..63
    }
    return z & 0x80808080u;
}
// the syndromes of 64 rows of one layer per lane: XOR of the 64-bit windows the plan's syndrome table names (ldpc_plan.h), one table
// word and three sign dwords per link, all independent loads (two dependent global round trips per check in total)
template <int MAXDEG>
__device__ __forceinline__ bool syndromes_bad(int q, int synd_base, const uint32_t* __restrict__ ents_all, const uint32_t* __restrict__ S, int j, int tps) {
    const int ntask = q * 6;
    const uint32_t* __restrict__ tab = ents_all + synd_base;
    bool bad = false;
    for (int t = j; t < ntask; t += tps) {
        uint32_t e[MAXDEG + 2];
#pragma unroll
        for (int k = 0; k < MAXDEG + 2; ++k) e[k] = tab[k * ntask + t];
        // all sign windows are fetched before any is used: two dependent global round trips per check, not one per link
        uint32_t d0[MAXDEG + 2], d1[MAXDEG + 2], d2[MAXDEG + 2];
#pragma unroll
        for (int k = 0; k < MAXDEG + 2; ++k) {
            const uint32_t* __restrict__ p = S + (e[k] & 0xffffu);         // (absent links: entry 0 -> a harmless read of the first dwords)
            d0[k] = p[0]; d1[k] = p[1]; d2[k] = p[2];
        }
#pragma unroll
        for (int k = 0; k < MAXDEG + 2; ++k) asm volatile("" : "+v"(d0[k]), "+v"(d1[k]), "+v"(d2[k]));   // (keeps the loads ahead of the arithmetic)
        unsigned long long acc = 0;
#pragma unroll
        for (int k = 0; k < MAXDEG + 2; ++k) {
            const uint32_t sh = (e[k] >> 16) & 31u;
            uint32_t lo = __builtin_amdgcn_alignbit(d1[k], d0[k], sh), hi = __builtin_amdgcn_alignbit(d2[k], d1[k], sh);
            lo &= ~((e[k] >> 30) & 1u);                                      // row 0 of layer 0 has no previous parity bit
            const uint32_t m = (uint32_t)((int)e[k] >> 31);                  // present?
            acc ^= ((unsigned long long)(hi & m) << 32) | (lo & m);
        }
        if (t - 6 * (t / 6) == 5) acc &= (1ull << 40) - 1;                   // rows 320..359
        bad |= acc != 0;
    }
    return bad;
}

// ---- a frame's way in and out.  T = threads of a frame slot (LDPC_TPS, LDPC_SPLIT_T, 64), t = the thread's index within the slot.
// information-bit LLRs: straight copy (K is a multiple of 8); parity LLRs: pty[360*i + jj] = llr[K + q*jj + i]   (layered_decoder.hh:124-126)
template <int T>
__device__ __forceinline__ void ldpc_frame_load(int8_t* __restrict__ post, const int8_t* __restrict__ src, int K, int R, int q, int t) {
    for (int i = t; i < K / 8; i += T) reinterpret_cast<uint2*>(post)[i] = reinterpret_cast<const uint2*>(src)[i];
    for (int c = t; c < R; c += T) {
        const int jj = c / q, i = c - jj * q;
        post[K + 360 * i + jj] = src[K + c];
    }
}
// what a syndrome check decides (`any`: some row is bad): in forced mode the one check after the last sweep, else converged | exhausted | go on
__device__ __forceinline__ bool ldpc_verdict(int force, bool any, int it, int max_trials, int& ret) {
    if (force) { ret = any ? -1 : max_trials; return true; }
    if (!any) { ret = it; return true; }
    if (it == max_trials) { ret = -1; return true; }
    return false;
}
// trials[f]; hard decisions of [0,K): 64 bits per wave step via ballot, MSB-first bytes (module_dvbs2_demod.cpp:357-360); optionally the posteriors, reference layout
template <int T>
__device__ __forceinline__ void ldpc_frame_store(const int8_t* __restrict__ post, int f, int ret, int32_t* trials, uint8_t* hard, int hard_stride, int8_t* post_out,
                                                 int N, int K, int R, int q, int t, int wave) {
    if (t == 0) trials[f] = ret;
    uint8_t* __restrict__ hd = hard + (size_t)f * hard_stride;
    const int lane = t & 63;
    for (int base = wave * 64; base < K; base += T) {
        const int idx = base + lane;
        const int neg = (idx < K) ? (post[idx] < 0) : 0;
        unsigned long long b = __ballot(neg);
        b = __builtin_bswap64(__brevll(b));
        if (lane == 0) {
            const int nbytes = min(8, (K - base) / 8);
            // (K / 8 is odd for some codes, and a caller's stride need not be a multiple of 8: the 8-byte store only where it is aligned)
            if (nbytes == 8 && ((uintptr_t)(hd + base / 8) & 7u) == 0) *reinterpret_cast<uint2*>(hd + base / 8) = make_uint2((uint32_t)b, (uint32_t)(b >> 32));
            else for (int n = 0; n < nbytes; ++n) hd[base / 8 + n] = (uint8_t)(b >> (8 * n));
        }
    }
    if (post_out) {
        int8_t* __restrict__ dst = post_out + (size_t)f * N;
        for (int i = t; i < K / 8; i += T) reinterpret_cast<uint2*>(dst)[i] = reinterpret_cast<const uint2*>(post)[i];
        for (int c = t; c < R; c += T) {
            const int jj = c / q, i = c - jj * q;
            dst[K + c] = post[K + 360 * i + jj];
        }
    }
}

}  // namespace s2
