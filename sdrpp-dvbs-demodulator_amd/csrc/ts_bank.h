// Shared by the banks that work on transport streams in HBM (tsmon.hip: the TS monitor; psi.hip: the PSI sections; pcr.hip: the PCRs; pes.hip: the PES packets;
// es.hip: the elementary streams; t2mi.hip, mpe.hip, ule.hip: T2-MI packets, MPE sections, ULE SNDUs):
// what a "packet bank" does around its rules.  On the device: the one header read, the one workgroup prefix sum and the contiguous
// run of items a thread takes ("flags in a mask, scan, scatter").  On the host: the argument table of a call, the count checks,
// the staging of the single-stream host-buffer entry point and the table getters.  The rules stay in tsmon_rules.h / psi_rules.h / pcr_rules.h / pes_rules.h /
// t2mi_rules.h / mpe_rules.h / ule_rules.h; what the four reassembling banks (PSI, T2-MI, MPE, ULE) share beyond this is ts_reasm.h, what
// the three watched-PID banks (PCR, PES, ES) share is watch_bank.h (the host half) and, PES and ES, ts_watch.h (device phases A-C); the
// three datagram banks (T2-MI, MPE, ULE) are dgram_bank.h.
#pragma once
#include "bbts_common.h"
#include "tsmon_rules.h"

namespace s2 {

#ifdef __HIPCC__
typedef unsigned __attribute__((aligned(1))) ts_unaligned_u32;
// the header of packet k of a stream, read as two dwords (they lie inside the packet: 188 >= 8).  *b4: byte 4 (adaptation field length)
__device__ inline TsmonHdr ts_load_header(const uint8_t* __restrict__ ts, int k, unsigned* b4 = nullptr) {
    const uint8_t* p = ts + (size_t)k * TSMON_TS;
    const unsigned a = *reinterpret_cast<const ts_unaligned_u32*>(p), b = *reinterpret_cast<const ts_unaligned_u32*>(p + 4);
    const uint8_t h[8] = {(uint8_t)a, (uint8_t)(a >> 8), (uint8_t)(a >> 16), (uint8_t)(a >> 24), (uint8_t)b, (uint8_t)(b >> 8), 0, 0};
    if (b4) *b4 = b & 255;
    return tsmon_parse(h);
}

// header dword d of packet k, bytes 4 d .. 4 d + 3: d 1 holds the adaptation field's length and flags, d 2 (bytes 8..11, still inside
// the packet) what a bank reads of the field's first entry, the PCR
__device__ inline unsigned ts_load_header_dword(const uint8_t* __restrict__ ts, int k, int d) {
    return *reinterpret_cast<const ts_unaligned_u32*>(ts + (size_t)k * TSMON_TS + 4 * d);
}

// exclusive prefix sum of one int per thread over the WG threads of the workgroup; *total: the sum.  wsum: WG / 64 ints of LDS
template <int WG>
__device__ inline int ts_block_scan(int v, int* wsum, int* total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int inc = v;
    for (int k = 1; k < 64; k <<= 1) { const int t = __shfl_up(inc, k); if (lane >= k) inc += t; }
    if (lane == 63) wsum[wave] = inc;
    __syncthreads();
    int base = 0, sum = 0;
    for (int w = 0; w < WG / 64; ++w) { if (w < wave) base += wsum[w]; sum += wsum[w]; }
    __syncthreads();                               // wsum may be written again
    *total = sum;
    return base + inc - v;
}

// exclusive maximum over the threads before this one (-1: none).  wsum: one int of LDS per wave
__device__ inline int ts_block_scan_max(int v, int* wsum) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int inc = v;
    for (int k = 1; k < 64; k <<= 1) { const int t = __shfl_up(inc, k); if (lane >= k && t > inc) inc = t; }
    if (lane == 63) wsum[wave] = inc;
    __syncthreads();
    int base = -1;
    for (int w = 0; w < wave; ++w) if (wsum[w] > base) base = wsum[w];
    __syncthreads();
    const int prev = __shfl_up(inc, 1);
    return lane && prev > base ? prev : base;
}

// the contiguous run [*k0, *k1) of n items that this thread of a workgroup of wg takes: ceil(n / wg) items, the last runs shorter or
// empty.  One flag per item in a 32-bit mask needs n <= 32 wg: at most 32 items per thread at 8192 packets, 16 at 4096 (asserted by the banks)
__device__ inline void ts_thread_run(int n, int wg, int* k0, int* k1) {
    const int chunk = (n + wg - 1) / wg;
    *k0 = (int)threadIdx.x * chunk;
    *k1 = *k0 + chunk < n ? *k0 + chunk : n;
}
#endif

// the argument table of a call for n streams: input pointers | output pointers, SLOTS per stream (the datagram banks: 4) | byte counts
template <int SLOTS>
struct TsBankArgsN {
    ScratchLayout L;
    ScratchPart<const uint8_t*> in; ScratchPart<uint8_t*> out; ScratchPart<int> nbytes;
    explicit TsBankArgsN(size_t n) : in(L.add<const uint8_t*>(n)), out(L.add<uint8_t*>(n * SLOTS)), nbytes(L.add<int>(n)) {}
    void fill(void* h_args, int n, const uint8_t* const* d_ts, uint8_t* const* d_out, const int* nb) const {
        const uint8_t** pi = in(h_args); uint8_t** po = out(h_args); int* pn = nbytes(h_args);
        for (int i = 0; i < n; ++i) { pi[i] = d_ts[i]; po[i] = d_out ? d_out[i] : nullptr; pn[i] = nb[i]; }
        if constexpr (SLOTS > 1) for (int g = n; g < n * SLOTS; ++g) po[g] = d_out ? d_out[g] : nullptr;
    }
};
typedef TsBankArgsN<1> TsBankArgs;

// n byte counts of a call: whole packets, at most max_packets of them.  false: last_error() has the text, behind the bank's prefix.
// The banks call it per stream inside their loops over thousands of streams: the two compares are inlined there, the text is built out of line
__attribute__((noinline, cold)) inline bool ts_bank_count_error(const char* prefix, const char* text) { last_error() = std::string(prefix) + text; return false; }
__attribute__((always_inline)) inline bool ts_bank_check_counts(const char* prefix, const int* nbytes, int n, int max_packets) {
    for (int i = 0; i < n; ++i) {
        if (nbytes[i] < 0 || nbytes[i] % TSMON_TS) return ts_bank_count_error(prefix, "a byte count is a whole number of 188-byte packets");
        if (nbytes[i] / TSMON_TS > max_packets) return ts_bank_count_error(prefix, "packet count exceeds max_packets");
    }
    return true;
}

// The device copies of one stream's host buffers (the single-stream entry points).  Workspace::ensure grows with a quarter of
// slack: harmless here, the input never grows after the first call and the output follows the largest cap seen.
struct TsHostStage { Workspace in, out; };
// The device path of a single-stream call with host buffers: h_ts staged, room for cap + 4 output bytes, per-stream vectors in which the other
// streams bring nothing (out_all: they have the output pointer all the same), the bank's batch(in, nbytes, out or null, out_bytes), copy back.
// With SLOTS outputs per stream the output vectors hold that many per stream and the call is for `slot` of `stream`
template <int SLOTS = 1, typename Batch>
inline int ts_bank_work(TsHostStage& sg, int nstreams, int stream, const uint8_t* h_ts, int nbytes, int max_packets, uint8_t* h_out, int cap, bool out_all, Batch batch,
                        int slot = 0) {
    if (const int e = sg.in.ensure((size_t)max_packets * TSMON_TS)) return e;
    if (nbytes > 0) HIP_TRY(hipMemcpy(sg.in.p, h_ts, nbytes, hipMemcpyHostToDevice));
    if (const int e = h_out ? sg.out.ensure((size_t)cap + 4) : 0) return e;
    std::vector<const uint8_t*> in(nstreams, nullptr);
    const int g = SLOTS > 1 ? stream * SLOTS + slot : stream;
    std::vector<uint8_t*> out(nstreams * SLOTS, out_all ? static_cast<uint8_t*>(sg.out.p) : nullptr);
    std::vector<int> nb(nstreams, 0), ob(nstreams * SLOTS, 0);
    in[stream] = static_cast<const uint8_t*>(sg.in.p); out[g] = static_cast<uint8_t*>(sg.out.p); nb[stream] = nbytes;
    const int rc = batch(in.data(), nb.data(), h_out ? out.data() : nullptr, ob.data());
    if (rc < 0) return rc;
    if (h_out && ob[g] > 0) HIP_TRY(hipMemcpy(h_out, sg.out.p, ob[g], hipMemcpyDeviceToHost));
    return ob[g];
}

// The table getters of a bank `b` (null: an argument error) with ctx, nstreams, nrows[], the device table d_rows of b->*stride rows per
// stream and, in a host bank (ctx null), host[stream].rows.  The rows of the stream's last call into h_rows, at most cap; *n: how many there are.
// A bank with a table per (stream, slot) has SLOTS of each per stream
template <int SLOTS = 1, typename Bank, typename Pub>
inline int ts_bank_rows(Bank* b, int Bank::*stride, int stream, Pub* h_rows, int cap, int* n, int slot = 0) {
    if (!b || stream < 0 || stream >= b->nstreams || (SLOTS > 1 && (slot < 0 || slot >= SLOTS)) || !n || cap < 0 || (cap > 0 && !h_rows)) return DVBS2GPU_ERR_ARG;
    static_assert(sizeof(Pub) == sizeof(*b->d_rows), "row layout");
    const int g = SLOTS > 1 ? stream * SLOTS + slot : stream, k = (*n = b->nrows[g]) < cap ? *n : cap;
    if (k <= 0) return 0;
    if (!b->ctx) { memcpy(h_rows, b->host[g].rows.data(), k * sizeof(Pub)); return 0; }
    HIP_TRY(hipSetDevice(b->ctx->device));
    HIP_TRY(hipMemcpy(h_rows, b->d_rows + (size_t)g * (b->*stride), k * sizeof(Pub), hipMemcpyDeviceToHost));
    return 0;
}
// the same table where it lies in HBM (device banks only)
template <int SLOTS = 1, typename Bank, typename Pub>
inline int ts_bank_rows_device(Bank* b, int Bank::*stride, int stream, const Pub** d_rows, int* n, int slot = 0) {
    if (!b || !b->ctx || stream < 0 || stream >= b->nstreams || (SLOTS > 1 && (slot < 0 || slot >= SLOTS)) || !n || !d_rows) return DVBS2GPU_ERR_ARG;
    const int g = SLOTS > 1 ? stream * SLOTS + slot : stream;
    *n = b->nrows[g]; *d_rows = *n ? reinterpret_cast<const Pub*>(b->d_rows + (size_t)g * (b->*stride)) : nullptr;
    return 0;
}

}  // namespace s2
