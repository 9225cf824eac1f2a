// The DVB-S2 FEC encoder on gfx950 -- BB scrambling, BCH encoding, LDPC encoding (ETSI EN 302 307-1 clauses 5.2.2, 5.3.1, 5.3.2), the inverse of the
// stages in bch_kernel.hip and the three LDPC decoder kernels -- and the per-frame channel-error count that is made from it.  Tables: fec_encode_rules.h.
// Frames are packed bits, MSB first, in the order dvbs2gpu_ldpc_decode_batch reads its LLRs in: K information bits, then parity bit p[q j + i] of layer i, row j.
//
// Four kernels, separate launches (the BCH parity must be complete before the LDPC stage reads its last information block, and the two stages want different
// workgroup shapes: a wave per frame against a workgroup per frame):
//   bb_scramble   a byte per lane.
//   bch_encode    a wave per frame, four frames per workgroup.  The message is cut into 64 chunks, the last one ending with the message; lane c pushes its
//                 chunk through the byte-table LFSR (table: 256 x 6 words = 6 KB of LDS per workgroup), which leaves chunk_c(x) x^P mod g.  The map is
//                 GF(2)-linear: the lane then multiplies its residue by x^(8 chunk_bytes (63 - c)) mod g -- for every set bit i the chunk-shift row
//                 x^(i + 8 chunk_bytes (63 - c)) mod g, 64 x P rows of 24 bytes = 295 KB per code at the most, read from L2 -- and the 64 products are XORed
//                 across the wave.  Lanes k < P / 8 write parity byte k.
//   ldpc_encode   a workgroup of 256 lanes per frame.  LDS: every 360-bit information block bit-reversed into 13 words (the block, then its first 56 bits
//                 again) and one 13-word row per layer, (N / 360) x 52 bytes = 9.4 KB for a normal frame.  Lane (i, w) XORs the links of layer i for rows
//                 32 w .. 32 w + 31: a link is block r rotated by s, i.e. the two adjacent words at bit (32 w + 360 - s) % 360 funnel-shifted.  Twelve lanes
//                 turn the raw rows into the running XOR over the layers V_i; the accumulator p[c] ^= p[c - 1] over c = q j + i is V_i[j] ^ T[j] with T the
//                 exclusive prefix XOR of the 360 column sums (V_(q-1)), twelve words scanned in registers.  Output: a lane per parity byte gathers its eight
//                 bits (i, j) -> q j + i from the layer rows (row stride 13 words: odd, so consecutive layers fall into different LDS banks).
//   fec_llr       a lane per bit: +amplitude for 0, -amplitude for 1, the decoder's input.
//   fec_channel_ber   a workgroup per frame, a lane per position: LLRs that are not 0, and those among them whose sign is not the re-encoded bit.
// No inline assembly; every store is a vector store.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "kernels.h"
#include "fec_encode_rules.h"

namespace s2 {

using fecenc::BCH_WORDS;
using fecenc::LDPC_EXT_WORDS;

__global__ __launch_bounds__(256) void bb_scramble_kernel(const uint8_t* __restrict__ bbframes, int kb_bytes, const uint8_t* __restrict__ prbs, int nframes,
                                                          uint8_t* __restrict__ out, size_t out_stride, int out_bytes) {
    for (int f = blockIdx.y; f < nframes; f += gridDim.y)
        for (int b = blockIdx.x * 256 + threadIdx.x; b < out_bytes; b += gridDim.x * 256)
            out[(size_t)f * out_stride + b] = b < kb_bytes ? (uint8_t)(bbframes[(size_t)f * kb_bytes + b] ^ prbs[b]) : (uint8_t)0;
}

// P: the parity bits (128, 160, 168, 192); residues live in NW = ceil(P / 32) registers
template <int P>
__global__ __launch_bounds__(256) void bch_encode_kernel(FecEncDeviceCode C, uint8_t* frames, size_t stride, int nframes) {
    constexpr int NW = (P + 31) / 32, TOP_W = (P - 8) / 32, TOP_S = (P - 8) % 32;
    __shared__ uint32_t s_tab[256 * BCH_WORDS];
    for (int t = threadIdx.x; t < 256 * BCH_WORDS; t += 256) s_tab[t] = C.d_byte_tab[t];
    __syncthreads();
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int kb = C.kbch / 8, L = C.chunk_bytes;
    for (int f = blockIdx.x * fecenc::BCH_FRAMES_PER_WG + wave; f < nframes; f += gridDim.x * fecenc::BCH_FRAMES_PER_WG) {
        uint8_t* fr = frames + (size_t)f * stride;
        // the lane's chunk: bytes [begin, begin + L), what lies in front of the message is empty
        const int begin = kb - (fecenc::BCH_CHUNKS - lane) * L;
        uint32_t r[NW];
#pragma unroll
        for (int w = 0; w < NW; ++w) r[w] = 0;
        for (int b = begin < 0 ? 0 : begin; b < begin + L; ++b) {
            const uint32_t top = ((r[TOP_W] >> TOP_S) & 0xffu) ^ fr[b];
#pragma unroll
            for (int w = NW - 1; w > 0; --w) r[w] = (r[w] << 8) | (r[w - 1] >> 24);
            r[0] <<= 8;
            if (P % 32) r[NW - 1] &= (1u << (P % 32)) - 1u;
#pragma unroll
            for (int w = 0; w < NW; ++w) r[w] ^= s_tab[top * BCH_WORDS + w];
        }
        // residue x x^(8 L (63 - lane)) mod g
        const uint32_t* rows = C.d_rows + (size_t)lane * P * BCH_WORDS;
        uint32_t acc[NW];
#pragma unroll
        for (int w = 0; w < NW; ++w) acc[w] = 0;
#pragma unroll
        for (int w = 0; w < NW; ++w) {
            const uint32_t bits = r[w];
            const int nb = P - 32 * w < 32 ? P - 32 * w : 32;
            for (int b = 0; b < nb; ++b) {
                const uint32_t m = 0u - ((bits >> b) & 1u);
                const uint32_t* row = rows + (size_t)(32 * w + b) * BCH_WORDS;
#pragma unroll
                for (int v = 0; v < NW; ++v) acc[v] ^= row[v] & m;
            }
        }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1)
#pragma unroll
            for (int w = 0; w < NW; ++w) acc[w] ^= __shfl_xor(acc[w], off);
        // parity byte k holds the coefficients of x^(P - 1 - 8 k) .. x^(P - 8 - 8 k)
        if (lane < P / 8) {
            const int bit = P - 8 - 8 * lane;
            uint32_t word = 0;
#pragma unroll
            for (int w = 0; w < NW; ++w) word = (bit >> 5) == w ? acc[w] : word;
            fr[kb + lane] = (uint8_t)(word >> (bit & 31));
        }
    }
}

__global__ __launch_bounds__(256) void ldpc_encode_kernel(FecEncDeviceCode C, const uint8_t* info, size_t info_stride, uint8_t* code, size_t code_stride,
                                                          int nframes) {
    __shared__ uint32_t s_bits[180 * LDPC_EXT_WORDS];       // the information blocks, then the layers' rows: blocks + q = N / 360 <= 180
    __shared__ uint32_t s_sum[12], s_scan[12];
    const int tid = threadIdx.x, nb = C.blocks, q = C.q, kbytes = C.K / 8;
    uint32_t* s_par = s_bits + nb * LDPC_EXT_WORDS;
    for (int f = blockIdx.x; f < nframes; f += gridDim.x) {
        const uint8_t* src = info + (size_t)f * info_stride;
        uint8_t* dst = code + (size_t)f * code_stride;
        // block r as 52 bytes: its 45, then its first 7 again; bit m of the block in bit m % 32 of word m / 32
        for (int t = tid; t < nb * LDPC_EXT_WORDS; t += 256) {
            const int r = t / LDPC_EXT_WORDS, e = t - r * LDPC_EXT_WORDS;
            uint32_t word = 0;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                int b = 4 * e + k;
                if (b >= 45) b -= 45;
                word |= (uint32_t)src[45 * r + b] << (24 - 8 * k);
            }
            s_bits[t] = __brev(word);
        }
        if (dst != src)
            for (int b = tid; b < kbytes; b += 256) dst[b] = src[b];
        __syncthreads();
        // the raw parity rows: layer i, rows 32 w .. 32 w + 31
        for (int t = tid; t < q * 12; t += 256) {
            const int i = t / 12, w = t - i * 12;
            uint32_t acc = 0;
            for (uint32_t e = C.d_layer_off[i]; e < C.d_layer_off[i + 1]; ++e) {
                const uint32_t ent = C.d_ent[e];
                int start = 32 * w + (int)(ent & 0xffffu);
                if (start >= 360) start -= 360;
                const uint32_t* X = s_bits + (ent >> 16) * LDPC_EXT_WORDS + (start >> 5);
                acc ^= __funnelshift_r(X[0], X[1], start & 31);
            }
            s_par[i * LDPC_EXT_WORDS + w] = w == 11 ? acc & 0xffu : acc;
        }
        __syncthreads();
        // V_i = raw_0 ^ .. ^ raw_i, and the column sums
        if (tid < 12) {
            uint32_t acc = 0;
            for (int i = 0; i < q; ++i) {
                acc ^= s_par[i * LDPC_EXT_WORDS + tid];
                s_par[i * LDPC_EXT_WORDS + tid] = acc;
            }
            s_sum[tid] = acc;
        }
        __syncthreads();
        // T[j] = XOR of the column sums of the rows before j
        if (tid < 12) {
            uint32_t x = s_sum[tid];
            x ^= x << 1; x ^= x << 2; x ^= x << 4; x ^= x << 8; x ^= x << 16;
            uint32_t carry = 0;
            for (int k = 0; k < tid; ++k) carry ^= (uint32_t)__popc(s_sum[k]);
            s_scan[tid] = (x << 1) ^ (0u - (carry & 1u));
        }
        __syncthreads();
        // parity byte B: bits c = 8 B .. 8 B + 7, c = q j + i
        for (int B = tid; B < 45 * q; B += 256) {
            int j = (8 * B) / q, i = 8 * B - j * q;
            uint32_t byte = 0;
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                const uint32_t v = s_par[i * LDPC_EXT_WORDS + (j >> 5)] ^ s_scan[j >> 5];
                byte |= ((v >> (j & 31)) & 1u) << (7 - k);
                if (++i == q) { i = 0; ++j; }
            }
            dst[kbytes + B] = (uint8_t)byte;
        }
        __syncthreads();
    }
}

__global__ __launch_bounds__(256) void fec_llr_kernel(const uint8_t* __restrict__ code, int N, int nframes, int amplitude, int8_t* __restrict__ llr) {
    for (int f = blockIdx.y; f < nframes; f += gridDim.y)
        for (int n = blockIdx.x * 256 + threadIdx.x; n < N; n += gridDim.x * 256) {
            const int bit = (code[(size_t)f * (N / 8) + (n >> 3)] >> (7 - (n & 7))) & 1;
            llr[(size_t)f * N + n] = (int8_t)(bit ? -amplitude : amplitude);
        }
}

__global__ __launch_bounds__(256) void fec_channel_ber_kernel(const int8_t* __restrict__ llr, const uint8_t* __restrict__ code, int N,
                                                              const int32_t* __restrict__ corrections, int nframes, int32_t* __restrict__ errors,
                                                              int32_t* __restrict__ counted) {
    __shared__ int s_cnt[2];
    for (int f = blockIdx.x; f < nframes; f += gridDim.x) {
        if (corrections && corrections[f] < 0) {        // the BBFRAME is not the transmitted one: nothing to compare with
            if (threadIdx.x == 0) { errors[f] = -1; counted[f] = 0; }
            continue;
        }
        if (threadIdx.x < 2) s_cnt[threadIdx.x] = 0;
        __syncthreads();
        const int8_t* l = llr + (size_t)f * N;
        const uint8_t* c = code + (size_t)f * (N / 8);
        int ne = 0, nc = 0;
        for (int n = threadIdx.x; n < N; n += 256) {
            const int v = l[n], bit = (c[n >> 3] >> (7 - (n & 7))) & 1;
            nc += v != 0;
            ne += v != 0 && (v < 0) != (bit != 0);
        }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) { ne += __shfl_xor(ne, off); nc += __shfl_xor(nc, off); }
        if ((threadIdx.x & 63) == 0) { atomicAdd(&s_cnt[0], ne); atomicAdd(&s_cnt[1], nc); }
        __syncthreads();
        if (threadIdx.x == 0) { errors[f] = s_cnt[0]; counted[f] = s_cnt[1]; }
        __syncthreads();
    }
}

static int grid_for(int units) { return units < fecenc::MAX_WORKGROUPS ? units : fecenc::MAX_WORKGROUPS; }

hipError_t bb_scramble_launch(const uint8_t* bbframes, int kb_bytes, const uint8_t* prbs, int nframes, uint8_t* out, size_t out_stride, int out_bytes,
                              hipStream_t stream) {
    int gx = (out_bytes + 255) / 256;
    if (gx > 32) gx = 32;
    hipLaunchKernelGGL(bb_scramble_kernel, dim3(gx, grid_for(nframes)), dim3(256), 0, stream, bbframes, kb_bytes, prbs, nframes, out, out_stride, out_bytes);
    return hipGetLastError();
}

hipError_t bch_encode_launch(const FecEncDeviceCode& C, uint8_t* frames, size_t stride, int nframes, hipStream_t stream) {
    const dim3 grid(grid_for((nframes + fecenc::BCH_FRAMES_PER_WG - 1) / fecenc::BCH_FRAMES_PER_WG));
    switch (C.P) {
    case 128: hipLaunchKernelGGL(bch_encode_kernel<128>, grid, dim3(256), 0, stream, C, frames, stride, nframes); break;
    case 160: hipLaunchKernelGGL(bch_encode_kernel<160>, grid, dim3(256), 0, stream, C, frames, stride, nframes); break;
    case 168: hipLaunchKernelGGL(bch_encode_kernel<168>, grid, dim3(256), 0, stream, C, frames, stride, nframes); break;
    case 192: hipLaunchKernelGGL(bch_encode_kernel<192>, grid, dim3(256), 0, stream, C, frames, stride, nframes); break;
    default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

hipError_t ldpc_encode_launch(const FecEncDeviceCode& C, const uint8_t* info, size_t info_stride, uint8_t* code, size_t code_stride, int nframes,
                              hipStream_t stream) {
    if (C.blocks + C.q > 180) return hipErrorInvalidValue;
    hipLaunchKernelGGL(ldpc_encode_kernel, dim3(grid_for(nframes)), dim3(256), 0, stream, C, info, info_stride, code, code_stride, nframes);
    return hipGetLastError();
}

hipError_t fec_llr_launch(const uint8_t* code, int N, int nframes, int amplitude, int8_t* llr, hipStream_t stream) {
    hipLaunchKernelGGL(fec_llr_kernel, dim3(8, grid_for(nframes)), dim3(256), 0, stream, code, N, nframes, amplitude, llr);
    return hipGetLastError();
}

hipError_t fec_channel_ber_launch(const int8_t* llr, const uint8_t* code, int N, const int32_t* corrections, int nframes, int32_t* errors, int32_t* counted,
                                  hipStream_t stream) {
    hipLaunchKernelGGL(fec_channel_ber_kernel, dim3(grid_for(nframes)), dim3(256), 0, stream, llr, code, N, corrections, nframes, errors, counted);
    return hipGetLastError();
}

}  // namespace s2
