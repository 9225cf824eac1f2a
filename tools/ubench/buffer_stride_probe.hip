// Development aid: how a STRIDED buffer resource addresses an array of fixed-size per-thread entries on gfx950 -- (1) with the descriptor's add-thread-id flag
// (word 3 bit 23: address = base + soffset + lane * stride, NO address VGPR) and (2) with an index VGPR (idxen).  Answers, from the hardware:
//   a) what word 3 has to hold beside the flag (are the data-format bits 18:15, which the usual 0x00020000 sets, taken as stride bits 17:14 in that mode?)
//   b) the unit in which num_records bounds a strided descriptor, and whether the scalar offset takes part in the range check
//   c) whether the last entry of the last wave and the first entry behind a layer offset are reached (768 threads x K layers, 16-byte loads, 8-byte stores)
// Every access stays inside its allocation whatever the answers are: a lane reaches at most 63 (add-tid) or 767 (index) entries of at most 2^18 bytes (the widest
// stride the mode could form) + the scalar offset < 32 MiB; the source holds its own word index, so a lane reports WHERE it read.
//   hipcc -O3 --offload-arch=gfx950 -o buffer_stride_probe tools/ubench/buffer_stride_probe.hip
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdint>
#include <vector>
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));
constexpr int T = 768, K = 3, ESRC = 16, EDST = 8;
constexpr size_t BYTES = (size_t)64 << 20;
constexpr uint32_t TAG = 0x40000000u, GUARD = 0xdeadbeefu;

// one wave: where does lane l read with this descriptor?  out[l] = the word found (TAG + word index, or 0 where the range check dropped the load)
__global__ void where_kernel(const uint32_t* src, uint32_t* out, int stride, uint32_t num_records, uint32_t word3, uint32_t soff) {
    const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(const_cast<uint32_t*>(src), (short)stride, (int)num_records, (int)word3);
    const u32x4 v = __builtin_amdgcn_raw_buffer_load_b128(rs, 0, __builtin_amdgcn_readfirstlane((int)soff), 0);
    out[threadIdx.x] = v.x;
}
// the same question for the index form: lane l asks for entry l
__global__ void where_index_kernel(const uint32_t* src, uint32_t* out, int stride, uint32_t num_records, uint32_t soff) {
    const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(const_cast<uint32_t*>(src), (short)stride, (int)num_records, 0x00020000);
    u32x4 v;
    const uint32_t so = (uint32_t)__builtin_amdgcn_readfirstlane((int)soff), l = threadIdx.x;
    asm volatile("buffer_load_dwordx4 %0, %1, %2, %3 idxen\n\ts_waitcnt vmcnt(0)" : "=&v"(v) : "v"(l), "s"(rs), "s"(so) : "memory");
    out[threadIdx.x] = v.x;
}
// the layer loop's pattern: entry (layer, t) -> 16 bytes in, 8 bytes out; wave base + layer offset in the scalar offset
template <bool INDEX>
__global__ void __launch_bounds__(T) sweep_kernel(const uint32_t* src, uint32_t* dst, uint32_t nrec_src, uint32_t nrec_dst, uint32_t word3) {
    const int t = threadIdx.x;
    const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane(t >> 6);
    const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(const_cast<uint32_t*>(src), ESRC, (int)nrec_src, (int)word3);
    const __amdgpu_buffer_rsrc_t rd = __builtin_amdgcn_make_buffer_rsrc(dst, EDST, (int)nrec_dst, (int)word3);
    for (int layer = 0; layer < K; ++layer) {
        u32x4 v;
        u32x2 w;
        if constexpr (INDEX) {
            const uint32_t so_s = (uint32_t)layer * T * ESRC, so_d = (uint32_t)layer * T * EDST;
            asm volatile("buffer_load_dwordx4 %0, %1, %2, %3 idxen\n\ts_waitcnt vmcnt(0)" : "=&v"(v) : "v"(t), "s"(rs), "s"(so_s) : "memory");
            w = u32x2{v.x + v.w, v.y ^ v.z};
            asm volatile("buffer_store_dwordx2 %0, %1, %2, %3 idxen" : : "v"(w), "v"(t), "s"(rd), "s"(so_d) : "memory");
        } else {
            v = __builtin_amdgcn_raw_buffer_load_b128(rs, 0, ((uint32_t)layer * T + wave * 64u) * ESRC, 0);
            w = u32x2{v.x + v.w, v.y ^ v.z};
            __builtin_amdgcn_raw_buffer_store_b64(w, rd, 0, ((uint32_t)layer * T + wave * 64u) * EDST, 0);
        }
    }
}
#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { printf("%s: %s\n", #x, hipGetErrorString(e_)); return 2; } } while (0)

int main() {
    uint32_t *src, *dst, *out;
    CK(hipMalloc(&src, BYTES)); CK(hipMalloc(&dst, BYTES)); CK(hipMalloc(&out, 64 * 4));
    std::vector<uint32_t> h(BYTES / 4), hd(BYTES / 4);
    for (size_t i = 0; i < h.size(); ++i) h[i] = TAG + (uint32_t)i;
    CK(hipMemcpy(src, h.data(), BYTES, hipMemcpyHostToDevice));
    uint32_t o[64];
    auto where = [&](int stride, uint32_t nrec, uint32_t w3, uint32_t soff, bool index = false) -> int {
        if (index) hipLaunchKernelGGL(where_index_kernel, dim3(1), dim3(64), 0, 0, src, out, stride, nrec, soff);
        else hipLaunchKernelGGL(where_kernel, dim3(1), dim3(64), 0, 0, src, out, stride, nrec, w3, soff);
        return hipMemcpy(o, out, sizeof o, hipMemcpyDeviceToHost) == hipSuccess ? 0 : 2;
    };
    // a) word 3
    const uint32_t w3s[] = {0x00800000u, 0x00820000u, 0x00020000u};
    for (uint32_t w3 : w3s) {
        if (where(ESRC, 1u << 20, w3, 0)) return 2;
        printf("word3 %08x stride 16: lane 0 reads byte %u, lane 1 byte %u, lane 63 byte %u -> effective stride %u\n", w3, o[0] ? (o[0] - TAG) * 4 : ~0u, o[1] ? (o[1] - TAG) * 4 : ~0u,
               o[63] ? (o[63] - TAG) * 4 : ~0u, o[1] && o[0] ? (o[1] - o[0]) * 4 : 0u);
    }
    // b) num_records, both forms: how many lanes of a wave get through, without and with a scalar offset far behind num_records of either unit
    const uint32_t nrs[] = {0, 1, 16, 40, 63, 64, 40 * 16, 63 * 16, 64 * 16};
    for (int index = 0; index < 2; ++index)
    for (uint32_t soff : {0u, (uint32_t)(2 * T + 11 * 64) * ESRC})
        for (uint32_t nr : nrs) {
            if (where(ESRC, nr, 0x00800000u, soff, index != 0)) return 2;
            int ok = 0, wrong = 0;
            for (int l = 0; l < 64; ++l) { if (o[l]) { ++ok; wrong += o[l] != TAG + (soff + (uint32_t)l * ESRC) / 4; } }
            printf("%s, soffset %6u, num_records %5u: %2d lanes read (%d from a wrong place), %2d got zero\n", index ? "index  " : "add-tid", soff, nr, ok, wrong, 64 - ok);
        }
    // c) the layer loop's pattern, both forms; num_records = the whole array in entries (the add-tid form is not bounded by it, see b)
    int rc = 0;
    for (int form = 0; form < 2; ++form) {
        CK(hipMemset(dst, 0, BYTES));
        for (size_t i = 0; i < hd.size(); ++i) hd[i] = GUARD;
        CK(hipMemcpy(dst, hd.data(), BYTES, hipMemcpyHostToDevice));
        if (form == 0) hipLaunchKernelGGL(sweep_kernel<false>, dim3(1), dim3(T), 0, 0, src, dst, (uint32_t)T * K, (uint32_t)T * K, 0x00800000u);
        else hipLaunchKernelGGL(sweep_kernel<true>, dim3(1), dim3(T), 0, 0, src, dst, (uint32_t)T * K, (uint32_t)T * K, 0x00020000u);
        CK(hipDeviceSynchronize());
        CK(hipMemcpy(hd.data(), dst, BYTES, hipMemcpyDeviceToHost));
        size_t bad = 0, first_bad = 0, stray = 0;
        for (size_t e = 0; e < (size_t)T * K; ++e) {
            const uint32_t* s = &h[e * 4];
            const bool good = hd[2 * e] == s[0] + s[3] && hd[2 * e + 1] == (s[1] ^ s[2]);
            if (!good && !bad++) first_bad = e;
        }
        for (size_t i = (size_t)T * K * 2; i < hd.size(); ++i) stray += hd[i] != GUARD;
        const size_t last = (size_t)T * K - 1, firstl = T;
        printf("%s form: %zu of %d entries wrong (first: %zu), %zu words written outside the array; entry %zu (first behind a layer offset) %s, entry %zu (last lane of the last wave) %s\n",
               form ? "index  " : "add-tid", bad, T * K, first_bad, stray, firstl, hd[2 * firstl] == h[4 * firstl] + h[4 * firstl + 3] ? "ok" : "WRONG", last,
               hd[2 * last] == h[4 * last] + h[4 * last + 3] ? "ok" : "WRONG");
        rc |= (bad || stray) ? 1 : 0;
    }
    return rc;
}
