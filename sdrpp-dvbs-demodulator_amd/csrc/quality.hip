// Signal-quality estimates: per DVB-S2 frame, a data-aided Es/N0 from the known symbols of its PLL output and the MER of its
// payload; per DVB-S stream and call, a blind M2M4 Es/N0 and the QPSK-decision MER of the Costas output.  One workgroup per frame / stream, sums
// in a fixed order (per lane, then wave butterflies, then the four waves in order): the same input gives the same bits.
#include "kernels.h"
#include "s2_rx.h"
#include "s2_params.h"

namespace s2 {

namespace {

constexpr int QB = 256;            // lanes per workgroup (four waves)
constexpr int Q_KPL = 4;           // known symbols per lane: K <= 90 + 22 * 36 = 882 (QPSK normal frames with pilots) <= Q_KPL * QB
constexpr int Q_PRIO = 2;          // wave priority of the post stages beside the decoder where the host asks for it (= POST_PRIO, s2_rx_kernels.hip)

__device__ __forceinline__ int q_pilot_start(int b) { return 90 + (b + 1) * 1440 + b * 36; }   // (pilot_start, s2_rx_kernels.hip)

// every lane of the workgroup ends with the same sums; `lds` holds 4 * N floats
template <int N, typename T>
__device__ __forceinline__ void block_sum(T (&v)[N], T* lds) {
#pragma unroll
    for (int k = 0; k < N; ++k)
        for (int o = 32; o >= 1; o >>= 1) v[k] += __shfl_xor(v[k], o, 64);
    const int w = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0)
#pragma unroll
        for (int k = 0; k < N; ++k) lds[w * N + k] = v[k];
    __syncthreads();
#pragma unroll
    for (int k = 0; k < N; ++k) v[k] = ((lds[k] + lds[N + k]) + lds[2 * N + k]) + lds[3 * N + k];
    __syncthreads();
}

// known symbol q of a frame (q < 90: header, transformed in the PLL output -- each transform is its own inverse; then the pilot blocks)
__device__ __forceinline__ void known_symbol(const cf32* __restrict__ fr, const cf32* __restrict__ sof, const cf32* __restrict__ plsc, int q,
                                             cf32* y, cf32* a) {
    if (q < 90) {
        const cf32 o = fr[q];
        *y = (q & 1) ? cf32{-o.re, o.im} : cf32{o.im, o.re};
        *a = q < 26 ? sof[q] : plsc[q - 26];
    } else {
        const int b = (q - 90) / 36;
        *y = fr[q_pilot_start(b) + (q - 90 - 36 * b)];
        *a = cf32{0.70710678118654752f, 0.70710678118654752f};
    }
}

__global__ __launch_bounds__(QB) void s2_quality_kernel(const S2QualityDesc* __restrict__ desc, const S2VcmMod* __restrict__ mods,
                                                        const S2ConstelDev* __restrict__ cons, const cf32* __restrict__ sof, const cf32* __restrict__ plsc_all,
                                                        S2FrameQuality* __restrict__ out, int prio) {
    if (prio) __builtin_amdgcn_s_setprio(Q_PRIO);
    __shared__ float red[4 * 4];
    __shared__ cf32 pts[32];
    const int f = blockIdx.x, t = threadIdx.x;
    const S2QualityDesc D = desc[f];
    const S2VcmMod& M = mods[D.pls];
    const float qnan = __builtin_nanf("");
    if (M.valid != 1 || !D.pll) {        // dummy PLFRAME: no PLL output, no payload
        if (t == 0) out[f] = S2FrameQuality{qnan, qnan, qnan, qnan, 0, 0};
        return;
    }
    const cf32* __restrict__ fr = D.pll;
    const cf32* __restrict__ plsc = plsc_all + D.pls * 64;
    const int P = M.pilots ? 36 * M.pilot_blocks : 0, K = 90 + P, S = M.slots * 90;
    // the constellation, rescaled to unit mean energy once (APSK decisions search it; PSK decisions are made directly)
    const S2ConstelDev& C = cons[M.con];
    const int states = C.states;
    const bool psk = C.constel <= C_8PSK;
    if (!psk && t < states) pts[t] = C.pts[t];
    // ---- channel gain of each run of known symbols, h = sum y conj(a) / count: the header's (its symbols in the PLL output come from the header
    // demodulator's own phase loop) and the pilots' (the payload's phase reference).  The lane's known symbols stay in registers for the noise sum.
    cf32 ky[Q_KPL], ka[Q_KPL];
    float v[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int r = 0; r < Q_KPL; ++r) {
        const int q = t + r * QB;
        ky[r] = cf32{0.f, 0.f}; ka[r] = cf32{0.f, 0.f};
        if (q < K) known_symbol(fr, sof, plsc, q, &ky[r], &ka[r]);
        const int o = q < 90 ? 0 : 2;
        v[o] += ky[r].re * ka[r].re + ky[r].im * ka[r].im;
        v[o + 1] += ky[r].im * ka[r].re - ky[r].re * ka[r].im;
    }
    block_sum(v, red);
    const float hh_re = v[0] / 90.f, hh_im = v[1] / 90.f;
    const float hp_re = P ? v[2] / (float)P : 0.f, hp_im = P ? v[3] / (float)P : 0.f;
    // ---- noise: sum |y - h a|^2 over both runs / (K - runs)
    float e[1] = {0.f};
#pragma unroll
    for (int r = 0; r < Q_KPL; ++r) {
        const int q = t + r * QB;
        if (q >= K) continue;
        const float hre = q < 90 ? hh_re : hp_re, him = q < 90 ? hh_im : hp_im;
        const float dre = ky[r].re - (hre * ka[r].re - him * ka[r].im), dim = ky[r].im - (hre * ka[r].im + him * ka[r].re);
        e[0] += dre * dre + dim * dim;
    }
    block_sum(e, red);     // (its barriers also publish pts[])
    const float hh2 = hh_re * hh_re + hh_im * hh_im, hp2 = hp_re * hp_re + hp_im * hp_im;
    const float g2 = (90.f * hh2 + (float)P * hp2) / (float)K, sigma2 = e[0] / (float)(K - (P ? 2 : 1));
    // the payload's reference: the pilots' gain, or (no pilots) the header's magnitude at the PLL's own phase
    const float hre = P ? hp_re : sqrtf(hh2), him = P ? hp_im : 0.f, h2 = hre * hre + him * him;
    // ---- MER over the payload: z = y conj(h) / |h|^2 against the nearest point of the unit-energy constellation
    if (!psk) {
        float en = 0.f;
        for (int k = 0; k < states; ++k) en += pts[k].re * pts[k].re + pts[k].im * pts[k].im;
        const float scale = 1.0f / sqrtf(en / (float)states);
        __syncthreads();
        if (t < states) pts[t] = cf32{pts[t].re * scale, pts[t].im * scale};
        __syncthreads();
    }
    const float gre = hre / h2, gim = -him / h2;
    constexpr float R2 = 0.70710678118654752f, T8 = 0.41421356237309505f;     // 1/sqrt2, tan(pi/8)
    float m[2] = {0.f, 0.f};
    for (int j = t; j < S; j += QB) {
        const cf32 y = fr[90 + j + (M.pilots ? 36 * (j / 1440) : 0)];
        const float zre = y.re * gre - y.im * gim, zim = y.re * gim + y.im * gre;
        float dre, dim;
        if (psk) {
            // the point of largest Re(z conj(p)): QPSK (+-1 +-j)/sqrt2; 8PSK the nearest multiple of 45 degrees
            const float sr = zre < 0.f ? -1.f : 1.f, si = zim < 0.f ? -1.f : 1.f, ar = fabsf(zre), ai = fabsf(zim);
            if (states == 4 || (ai >= T8 * ar && ar >= T8 * ai)) { dre = sr * R2; dim = si * R2; }
            else if (ai < T8 * ar) { dre = sr; dim = 0.f; }
            else { dre = 0.f; dim = si; }
        } else {
            int best = 0;
            float bm = 3.0e38f;
            for (int k = 0; k < states; ++k) {
                const float pr = zre - pts[k].re, pi = zim - pts[k].im, dd = pr * pr + pi * pi;
                if (dd < bm) { bm = dd; best = k; }
            }
            dre = pts[best].re; dim = pts[best].im;
        }
        m[0] += dre * dre + dim * dim;
        m[1] += (zre - dre) * (zre - dre) + (zim - dim) * (zim - dim);
    }
    block_sum(m, red);
    if (t == 0)
        out[f] = S2FrameQuality{10.0f * log10f(g2 / sigma2), 10.0f * log10f(m[0] / m[1]), sqrtf(g2), atan2f(him, hre), K, S};
}

// DVB-S: M2M4 Es/N0 and the QPSK-decision MER of the symbols a stream's Costas loop produced in the call (double sums: a call holds up to a few
// hundred thousand symbols, and the M2M4 signal power is a difference of two nearly equal moments)
__global__ __launch_bounds__(QB) void dvbs_quality_kernel(const DvbsStreamWork* __restrict__ work, DvbsQuality* __restrict__ out) {
    __shared__ double red[4 * 3];
    const int s = blockIdx.x, t = threadIdx.x;
    const cf32* __restrict__ y = work[s].sym;
    const int n = work[s].st->n_sym;
    const float qnan = __builtin_nanf("");
    if (n <= 0) {
        if (t == 0) out[s] = DvbsQuality{qnan, qnan, qnan, 0};
        return;
    }
    double v[3] = {0.0, 0.0, 0.0};      // sum |y|^2, sum |y|^4, sum (|Re y| + |Im y|)
    for (int i = t; i < n; i += QB) {
        const double re = y[i].re, im = y[i].im, p = re * re + im * im;
        v[0] += p; v[1] += p * p; v[2] += fabs(re) + fabs(im);
    }
    block_sum(v, red);
    const double m2 = v[0] / n, m4 = v[1] / n, A = v[2] / n / 2.0;
    double w[3] = {0.0, 0.0, 0.0};
    for (int i = t; i < n; i += QB) {
        const double re = y[i].re, im = y[i].im;
        const double dre = A * (double)((re > 0.0) - (re < 0.0)), dim = A * (double)((im > 0.0) - (im < 0.0));
        w[0] += dre * dre + dim * dim;
        w[1] += (re - dre) * (re - dre) + (im - dim) * (im - dim);
    }
    block_sum(w, red);
    if (t == 0) {
        const double r = 2.0 * m2 * m2 - m4;
        const double S = r >= 0.0 ? sqrt(r) : -1.0, N = m2 - S;
        const float esn0 = (S > 0.0 && N > 0.0) ? (float)(10.0 * log10(S / N)) : qnan;
        out[s] = DvbsQuality{esn0, (float)(10.0 * log10(w[0] / w[1])), (float)A, n};
    }
}

}  // namespace

hipError_t s2_quality_launch(const S2QualityDesc* d_desc, int nframes, const S2VcmMod* d_mods, const S2ConstelDev* d_cons, const cf32* d_sof,
                             const cf32* d_plsc, S2FrameQuality* d_out, hipStream_t st, int prio) {
    hipLaunchKernelGGL(s2_quality_kernel, dim3(nframes), dim3(QB), 0, st, d_desc, d_mods, d_cons, d_sof, d_plsc, d_out, prio);
    return hipGetLastError();
}

hipError_t dvbs_quality_launch(const DvbsStreamWork* d_work, int nstreams, DvbsQuality* d_out, hipStream_t st) {
    hipLaunchKernelGGL(dvbs_quality_kernel, dim3(nstreams), dim3(QB), 0, st, d_work, d_out);
    return hipGetLastError();
}

}  // namespace s2
