// The DVB-S2 modulator on gfx950: code words -> PLFRAME symbols -> 2-sps IQ -> channel (ETSI EN 302 307-1 clauses 5.3.3, 5.4, 5.5, 5.6), the inverse of the
// receive chain in s2_rx_kernels.hip.  Rules: s2_tx_rules.h; the same inline functions run here and in tx_host below.
//
// Three kernels:
//   s2_pl_frame      a workgroup per (stream, frame), the frames' descriptors in the kernel's arguments.  The packed code word is staged in LDS (aligned dwords
//                    from global memory, funnel-shifted by the code word's byte offset: N / 8 is odd for short frames), 8.1 KB at the most.  A lane makes 8
//                    consecutive payload symbols: a byte per interleaver column, read across a byte boundary where the column's first bit is no multiple of 8
//                    (16APSK short: 4050), through the 32-entry table (LDS), rotated by Rn (two dwords of the Gold sequence), written as four 16-byte stores --
//                    the lane's 64 contiguous bytes, a wave's four stores fill one contiguous 4 KB run.  Lanes 0..89 write the header, the pilot blocks and the
//                    dummy frame's slots are written a symbol per lane.
//   s2_pulse_shape   a workgroup per tile of 256 symbols of a stream: the tile and 16 symbols of halo either side in LDS (2.3 KB), the 66 taps in the kernel's
//                    arguments (scalar registers); a lane makes the two samples of its symbol and writes them as one 16-byte store.
//   s2_channel       element-wise in place, a stream's parameters from a device table of 32-byte entries.
// No inline assembly; every store is a vector store; no scratch.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "ctx.h"
#include "s2_tx.h"

namespace s2 {

using namespace s2tx;

constexpr int CODE_WORDS = (MAX_CODE_BYTES + CODE_PAD + 3) / 4;

__global__ __launch_bounds__(FRAME_LANES) void s2_pl_frame_kernel(TxFrameArgs A, const uint8_t* __restrict__ code, cf32* __restrict__ sym, long long sym_stride,
                                                                  const cf32* __restrict__ sof, const cf32* __restrict__ plsc, const uint8_t* __restrict__ rn) {
    __shared__ uint32_t s_code[CODE_WORDS];
    __shared__ cf32 s_tab[32];
    const TxFrameDev& F = A.f[blockIdx.y];
    const int tid = threadIdx.x;
    cf32* out = sym + (size_t)blockIdx.x * sym_stride + F.sym_off;
    if (tid < HEADER) out[tid] = tid < 26 ? sof[tid] : plsc[F.pls * 64 + tid - 26];
    const cf32 pilot{PILOT_IQ, PILOT_IQ};
    if (F.dummy) {
        for (int i = tid; i < F.payload; i += FRAME_LANES) out[HEADER + i] = pl_rotate(pilot, rn[i]);
        return;
    }
    // the code word, bytes [0, code_bytes), then zeros
    const uint8_t* src = code + F.code_off + (long long)blockIdx.x * F.code_stride;
    const int sh = (int)((uintptr_t)src & 3u);
    const uint32_t* words = (const uint32_t*)(src - sh);
    const int nwords = (F.code_bytes + CODE_PAD + 3) / 4;
    for (int t = tid; t < nwords; t += FRAME_LANES) {
        uint32_t w = 0;
        if (4 * t < F.code_bytes) {
            const uint32_t lo = words[t];
            const uint32_t hi = 4 * t + 4 - sh < F.code_bytes ? words[t + 1] : 0u;      // (the dword behind one that already holds the last byte is never touched)
            w = __funnelshift_r(lo, hi, 8 * sh);
            const int left = F.code_bytes - 4 * t;
            if (left < 4) w &= (1u << (8 * left)) - 1u;
        }
        s_code[t] = w;
    }
    if (tid < 32) s_tab[tid] = F.tab[tid];
    __syncthreads();
    const uint8_t* cw = (const uint8_t*)s_code;
    const int col[5] = {F.col[0], F.col[1], F.col[2], F.col[3], F.col[4]};
    const uint32_t* rn32 = (const uint32_t*)rn;
    const int groups = (F.payload + GROUP - 1) / GROUP;
    for (int g = tid; g < groups; g += FRAME_LANES) {
        uint32_t v[GROUP];
        group_labels(cw, F.qpsk, F.bits, col, g, v);
        const int pos = payload_pos(GROUP * g, F.pilot_blocks);
        const uint32_t r0 = rn32[(pos - HEADER) >> 2], r1 = rn32[((pos - HEADER) >> 2) + 1];
        cf32 s[GROUP];
#pragma unroll
        for (int k = 0; k < GROUP; ++k) s[k] = pl_rotate(s_tab[v[k]], (int)(((k < 4 ? r0 : r1) >> (8 * (k & 3))) & 3u));
        if (GROUP * g + GROUP <= F.payload) {
            float4* o4 = (float4*)(out + pos);
#pragma unroll
            for (int k = 0; k < GROUP; k += 2) o4[k >> 1] = make_float4(s[k].re, s[k].im, s[k + 1].re, s[k + 1].im);
        } else {
#pragma unroll
            for (int k = 0; k < GROUP; ++k) if (GROUP * g + k < F.payload) out[pos + k] = s[k];
        }
    }
    for (int t = tid; t < F.pilot_blocks * PILOT_BLOCK; t += FRAME_LANES) {
        const int pos = pilot_pos(t / PILOT_BLOCK, t % PILOT_BLOCK);
        out[pos] = pl_rotate(pilot, rn[pos - HEADER]);
    }
}

__global__ __launch_bounds__(SHAPE_TILE) void s2_pulse_shape_kernel(Taps H, const cf32* __restrict__ sym, long long ns, int circular, int nstreams,
                                                                    cf32* __restrict__ iq) {
    __shared__ cf32 s_sym[SHAPE_TILE + 2 * SPAN];
    const int tid = threadIdx.x;
    const long long first = (long long)blockIdx.x * SHAPE_TILE;
    for (int s = blockIdx.y; s < nstreams; s += gridDim.y) {
        const cf32* in = sym + (size_t)s * ns;
        for (int t = tid; t < SHAPE_TILE + 2 * SPAN; t += SHAPE_TILE) {
            long long i = first - SPAN + t;
            if ((i < 0 || i >= ns) && circular) i = wrap_index(i, ns);
            s_sym[t] = i >= 0 && i < ns ? in[i] : cf32{0.f, 0.f};
        }
        __syncthreads();
        const long long m = first + tid;
        if (m < ns) {
            float o[4];
            shape_pair(H, [&](int k) -> cf32 { return s_sym[tid + SPAN + k]; }, o);
            *(float4*)(iq + ((size_t)s * ns + m) * 2) = make_float4(o[0], o[1], o[2], o[3]);
        }
        __syncthreads();
    }
}

__global__ __launch_bounds__(256) void s2_channel_kernel(const ChanParams* __restrict__ tab, cf32* iq, long long nsamples, int nstreams) {
    for (int s = blockIdx.y; s < nstreams; s += gridDim.y) {
        const ChanParams P = tab[s];
        cf32* x = iq + (size_t)s * nsamples;
        for (long long n = (long long)blockIdx.x * 256 + threadIdx.x; n < nsamples; n += (long long)gridDim.x * 256) x[n] = chan_sample(P, n, x[n]);
    }
}

// ---------------------------------------------------------------------------------------------------------------- host side
int tx_buffers_enter(dvbs2gpu_ctx* ctx, hipStream_t st) {
    TxState& T = ctx->tx;
    if (!T.ev) HIP_TRY(hipEventCreateWithFlags(&T.ev, hipEventDisableTiming));
    if (T.ev_recorded) HIP_TRY(hipStreamWaitEvent(st, T.ev, 0));
    return 0;
}
int tx_buffers_leave(dvbs2gpu_ctx* ctx, hipStream_t st) {
    HIP_TRY(hipEventRecord(ctx->tx.ev, st));
    ctx->tx.ev_recorded = true;
    return 0;
}

static int tx_constel(dvbs2gpu_ctx* ctx, const FrameRule& R, const cf32** out) {
    std::lock_guard<std::mutex> l(ctx->mtx);
    auto it = ctx->tx.constel.find(R.constel_key);
    if (it == ctx->tx.constel.end()) {
        std::vector<cf32> tab(32);
        tx_constellation(R.constel, R.g1, R.g2, tab.data());
        DevBuf<cf32> d;
        RC_TRY(upload(tab, d));
        it = ctx->tx.constel.emplace(R.constel_key, std::move(d)).first;
    }
    *out = it->second.get();
    return 0;
}

int tx_pl_frame(dvbs2gpu_ctx* ctx, const int32_t* pls, int nframes, const uint8_t* d_code, const long long* code_off, const long long* code_stride, int nstreams,
                cf32* d_symbols, hipStream_t st) {
    RC_TRY(get_rx_tables(ctx));
    ListSizes total;
    std::vector<long long> sym_off;
    if (!list_sizes(pls, nframes, &total, nullptr, &sym_off)) return DVBS2GPU_ERR_ARG;
    std::vector<TxFrameDev> frames((size_t)nframes);
    for (int f = 0; f < nframes; ++f) {
        FrameRule R;
        frame_rule(pls[f], &R);
        TxFrameDev& D = frames[f];
        D.code_off = R.dummy ? 0 : code_off[f]; D.code_stride = R.dummy ? 0 : code_stride[f]; D.sym_off = sym_off[f];
        D.tab = nullptr;
        if (!R.dummy) RC_TRY(tx_constel(ctx, R, &D.tab));
        D.pls = R.pls; D.dummy = R.dummy; D.qpsk = R.qpsk; D.bits = R.bits; D.payload = R.payload; D.pilot_blocks = R.pilot_blocks; D.code_bytes = R.code_bytes;
        for (int c = 0; c < 5; ++c) D.col[c] = R.col[c];
    }
    for (int a = 0; a < nframes; a += FRAMES_PER_LAUNCH) {
        const int n = std::min(FRAMES_PER_LAUNCH, nframes - a);
        TxFrameArgs A{};
        for (int k = 0; k < n; ++k) A.f[k] = frames[a + k];
        hipLaunchKernelGGL(s2_pl_frame_kernel, dim3(nstreams, n), dim3(FRAME_LANES), 0, st, A, d_code, d_symbols, total.symbols, ctx->pl.sof, ctx->pl.plsc,
                           ctx->pl.rn);
        HIP_TRY(hipGetLastError());
    }
    return 0;
}

int tx_pulse_shape(dvbs2gpu_ctx* ctx, const cf32* d_symbols, int nstreams, long long symbols, double rolloff, double timing, int circular, cf32* d_iq,
                   hipStream_t st) {
    (void)ctx;
    const Taps H = make_taps(rolloff, timing);
    const long long tiles = (symbols + SHAPE_TILE - 1) / SHAPE_TILE;
    hipLaunchKernelGGL(s2_pulse_shape_kernel, dim3((unsigned)tiles, (unsigned)std::min(nstreams, 32768)), dim3(SHAPE_TILE), 0, st, H, d_symbols, symbols,
                       circular ? 1 : 0, nstreams, d_iq);
    HIP_TRY(hipGetLastError());
    return 0;
}

int tx_channel(dvbs2gpu_ctx* ctx, cf32* d_iq, int nstreams, long long nsamples, const double* esn0_db, const double* cfo, const double* phase0,
               const uint64_t* seed, hipStream_t st) {
    // the table goes through a pinned staging buffer of the context, so the copy is asynchronous and the call does not wait for the stream; the host waits
    // only where the PREVIOUS call's copy out of that buffer has not happened yet
    TxState& T = ctx->tx;
    const size_t bytes = (size_t)nstreams * sizeof(ChanParams);
    if (!T.ev_stage) HIP_TRY(hipEventCreateWithFlags(&T.ev_stage, hipEventDisableTiming));
    if (T.stage_recorded) HIP_TRY(hipEventSynchronize(T.ev_stage));
    if (bytes > T.stage_bytes) {
        if (T.stage) (void)hipHostFree(T.stage);
        T.stage = nullptr; T.stage_bytes = 0;
        HIP_TRY(hipHostMalloc(&T.stage, bytes + bytes / 4, hipHostMallocDefault));
        T.stage_bytes = bytes + bytes / 4;
    }
    ChanParams* tab = (ChanParams*)T.stage;
    for (int s = 0; s < nstreams; ++s) tab[s] = chan_params(esn0_db[s], cfo[s], phase0[s], seed[s], s);
    RC_TRY(T.chan.ensure(bytes));
    HIP_TRY(hipMemcpyAsync(T.chan.p, tab, bytes, hipMemcpyHostToDevice, st));
    HIP_TRY(hipEventRecord(T.ev_stage, st));
    T.stage_recorded = true;
    const long long blocks = std::min<long long>((nsamples + 255) / 256, 1024);
    hipLaunchKernelGGL(s2_channel_kernel, dim3((unsigned)blocks, (unsigned)std::min(nstreams, 32768)), dim3(256), 0, st, (const ChanParams*)ctx->tx.chan.p, d_iq,
                       nsamples, nstreams);
    HIP_TRY(hipGetLastError());
    return 0;
}

void tx_host(const int32_t* pls, int nframes, const uint8_t* code, double rolloff, double timing, int circular, const double* esn0_db, const double* cfo,
             const double* phase0, const uint64_t* seed, long long stream, cf32* symbols, cf32* iq) {
    static const HostTables T;
    ListSizes total;
    std::vector<long long> sym_off, code_off;
    if (!list_sizes(pls, nframes, &total, nullptr, &sym_off, nullptr, &code_off)) return;
    std::vector<cf32> own;
    if (!symbols) { own.resize((size_t)total.symbols); symbols = own.data(); }
    for (int f = 0; f < nframes; ++f) {
        FrameRule R;
        frame_rule(pls[f], &R);
        cf32 tab[32] = {};
        if (!R.dummy) tx_constellation(R.constel, R.g1, R.g2, tab);
        host_frame(R, T, tab, code + code_off[f], symbols + sym_off[f]);
    }
    if (!iq) return;
    tx_shape_host(symbols, total.symbols, rolloff, timing, circular, iq);
    if (esn0_db) tx_channel_host(iq, 2 * total.symbols, *esn0_db, *cfo, *phase0, *seed, stream);
}

void tx_shape_host(const cf32* symbols, long long nsymbols, double rolloff, double timing, int circular, cf32* iq) {
    host_shape(symbols, nsymbols, make_taps(rolloff, timing), circular, iq);
}

void tx_channel_host(cf32* iq, long long nsamples, double esn0_db, double cfo, double phase0, uint64_t seed, long long stream) {
    host_channel(chan_params(esn0_db, cfo, phase0, seed, stream), iq, nsamples);
}

}  // namespace s2
