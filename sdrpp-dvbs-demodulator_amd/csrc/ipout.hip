// IP output bank (own extension; include/dvbs2gpu.h): the packets of up to four flow slots per stream among the
// transport streams that the packetisers or another bank left in HBM, grouped into UDP or RTP/MP2T datagrams with complete IPv4 / IPv6,
// UDP and RTP headers and checksums, laid back to back per slot in a device buffer with one table row each -- a view that the IP-TS bank
// (ipts.hip) reads back.  Every rule is in ipout_rules.h, whose IpoutHostStream is the sequential definition, the host bank and the
// kernels' yardstick.
//
//   ipout_scan_kernel    one workgroup per stream, 256 packets a round: a lane per packet reads the packet's first dword, tests the sync
//     byte and the four PID bitmaps; a ballot per slot and the waves' counts in LDS give every passing packet its rank, and its index
//     goes to the slot's list in scratch.  From what the slot holds, what passed and P: the slot's bytes (ipout_plan).  The call record
//     (sizes, passing packets, packets, bad sync bytes) goes to the host in one copy.  It stores no state.
//   ipout_commit_kernel  (once the host has seen that every slot's bytes fit) one workgroup per stream, a wave per datagram in turn.
//     Eight lanes per TS packet copy it -- from the slot's held packets or through the index list -- and sum its bytes at even and at
//     odd places (ip_wave.h; every packet starts at an even place of the UDP bytes); the wave reduces; lane 0 writes the headers with
//     the checksums into LDS (ipout_headers, the host's function) and the row, the wave copies the headers out.  A barrier; then a wave
//     per slot stores the slot's new held packets, held tick and datagram count, and one thread the stream's clock.  The barrier is what
//     keeps the held packets single: a call's first datagram reads them, the call's end writes them.  Where a call completes no
//     datagram the held packets stay where they are and the new ones are appended.
// Two launches per call and one device-to-host copy.  The kernels read nothing behind nbytes[i] of a stream and write nothing at or
// behind cap of a slot.  Static LDS: 0.3 KB (scan), 0.5 KB (commit).
#include "ip_wave.h"
#include "ipout_rules.h"

#include <memory>

using namespace s2;

static_assert(sizeof(IpoutRow) == sizeof(dvbs2gpu_ipout_row) && sizeof(IpoutRow) == 24 && IPOUT.row_bytes == 24, "row layout");
static_assert(offsetof(IpoutRow, offset) == offsetof(dvbs2gpu_ipout_row, offset) && offsetof(IpoutRow, bytes) == offsetof(dvbs2gpu_ipout_row, bytes) &&
              offsetof(IpoutRow, first_packet) == offsetof(dvbs2gpu_ipout_row, first_packet) && offsetof(IpoutRow, udp_checksum) == offsetof(dvbs2gpu_ipout_row, udp_checksum), "row layout");
static_assert(sizeof(IpoutFlow) == sizeof(dvbs2gpu_ipout_flow) && sizeof(IpoutFlow) == 56 && IPOUT.flow_bytes == 56, "flow layout");
static_assert(offsetof(IpoutFlow, src_port) == offsetof(dvbs2gpu_ipout_flow, src_port) && offsetof(IpoutFlow, ssrc) == offsetof(dvbs2gpu_ipout_flow, ssrc) &&
              offsetof(IpoutFlow, seq_base) == offsetof(dvbs2gpu_ipout_flow, seq_base) && offsetof(IpoutFlow, drop_null) == offsetof(dvbs2gpu_ipout_flow, drop_null), "flow layout");
static_assert(sizeof(IpoutLayout) == sizeof(dvbs2gpu_ipout_layout), "layout layout");
static_assert(IPOUT_MODE_RTP == DVBS2GPU_IPOUT_MODE_RTP && IPOUT_RTP == DVBS2GPU_IPOUT_RTP && IPOUT_SHORT == DVBS2GPU_IPOUT_SHORT && IPOUT_CARRIED == DVBS2GPU_IPOUT_CARRIED, "constants");
static_assert(IPOUT_SLOTS == IPTS_SLOTS && IPOUT_TS == TSMON_TS && IPOUT_MAP_WORDS == TSMON_MAP_WORDS, "constants");

namespace {

constexpr int IPOUT_WG = 256, IPOUT_WAVES = IPOUT_WG / 64, IPOUT_PKT_LANES = 8;
static_assert(IPOUT_WAVES == IPOUT_SLOTS, "a wave per slot stores the held packets");
static_assert(IPOUT_PKT_LANES * IPOUT.max_packets_per_datagram <= 64, "eight lanes per packet of a datagram");

// of one stream and call
struct IpoutCall { int32_t needed[IPOUT_SLOTS], passed[IPOUT_SLOTS], packets, bad_sync; };
// the counters of a stream on the host, in the order of dvbs2gpu_ipout_stats: 2 of the stream, 6 per slot
constexpr int IPOUT_NSTREAM_CNT = 2, IPOUT_NSLOT_CNT = 6, IPOUT_NCNT = IPOUT_NSTREAM_CNT + IPOUT_SLOTS * IPOUT_NSLOT_CNT;
enum { OC_PASSED = 0, OC_DGRAMS, OC_SHORT, OC_TS_PACKETS, OC_BYTES, OC_HELD };
static_assert(sizeof(dvbs2gpu_ipout_stats) == (IPOUT_NSTREAM_CNT + IPOUT_NSLOT_CNT) * sizeof(int64_t), "stats order");

__global__ void __launch_bounds__(IPOUT_WG) ipout_scan_kernel(const uint8_t* const* __restrict__ in, const int* __restrict__ nbytes, int max_packets,
                                                              const IpoutFlow* __restrict__ flows, const uint32_t* __restrict__ maps,
                                                              const IpoutSlot* __restrict__ state, uint16_t* __restrict__ idx_g, IpoutCall* __restrict__ call,
                                                              int flush, int flush_only) {
    __shared__ int wcnt[IPOUT_SLOTS + 1][IPOUT_WAVES];       // of a round: the passing packets per slot and wave; [4]: the bad sync bytes
    __shared__ IpoutFlow fl[IPOUT_SLOTS];
    const int s = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int n = nbytes[s] / IPOUT_TS;
    if (n > max_packets) n = max_packets;                    // (the host has refused such a call: the lists hold max_packets)
    if (tid < IPOUT_SLOTS) fl[tid] = flows[s * IPOUT_SLOTS + tid];
    __syncthreads();
    const uint8_t* ts = in[s];
    int base[IPOUT_SLOTS + 1] = {0, 0, 0, 0, 0};
    for (int k0 = 0; k0 < n; k0 += IPOUT_WG) {
        const int k = k0 + tid;
        const unsigned a = k < n ? ts_load_header_dword(ts, k, 0) : 0u;
        const bool good = (a & 255u) == (unsigned)IPTS.ts_sync;     // (a packet beyond n: not good, and not bad either)
        const int pid = ipout_pid(a >> 8 & 255u, a >> 16 & 255u);
        bool pass[IPOUT_SLOTS + 1];
        int rank[IPOUT_SLOTS];
        for (int q = 0; q < IPOUT_SLOTS; ++q) pass[q] = good && fl[q].family && ipout_passes(pid, fl[q], maps + ((size_t)s * IPOUT_SLOTS + q) * IPOUT_MAP_WORDS);
        pass[IPOUT_SLOTS] = k < n && !good;
        for (int q = 0; q <= IPOUT_SLOTS; ++q) {
            const unsigned long long b = __ballot(pass[q]);
            if (q < IPOUT_SLOTS) rank[q] = __popcll(b & ((1ull << lane) - 1ull));
            if (lane == 0) wcnt[q][wave] = __popcll(b);
        }
        __syncthreads();
        for (int q = 0; q <= IPOUT_SLOTS; ++q) {
            int before = 0, total = 0;
            for (int w = 0; w < IPOUT_WAVES; ++w) { const int c = wcnt[q][w]; before += w < wave ? c : 0; total += c; }
            if (q < IPOUT_SLOTS && pass[q]) idx_g[((size_t)s * IPOUT_SLOTS + q) * max_packets + base[q] + before + rank[q]] = (uint16_t)k;
            base[q] += total;
        }
        __syncthreads();                                     // wcnt is written again
    }
    const bool fl_now = flush && (flush_only < 0 || flush_only == s);
    if (tid < IPOUT_SLOTS) {
        int passed = 0;
        for (int q = 0; q < IPOUT_SLOTS; ++q) passed = q == tid ? base[q] : passed;
        call[s].passed[tid] = passed;
        call[s].needed[tid] = fl[tid].family ? ipout_plan(fl[tid], state[s * IPOUT_SLOTS + tid].held, passed, fl_now).bytes : 0;
    }
    if (tid == 0) { call[s].packets = n; call[s].bad_sync = base[IPOUT_SLOTS]; }
}

__global__ void __launch_bounds__(IPOUT_WG) ipout_commit_kernel(const uint8_t* const* __restrict__ in, const int* __restrict__ nbytes, uint8_t* const* __restrict__ out,
                                                                int max_packets, int cap, const IpoutFlow* __restrict__ flows, const uint64_t* __restrict__ rates,
                                                                IpoutClock* __restrict__ clock, IpoutSlot* __restrict__ state, uint8_t* __restrict__ held_g,
                                                                const uint16_t* __restrict__ idx_g, const IpoutCall* __restrict__ call, IpoutRow* __restrict__ rows_g,
                                                                int flush, int flush_only) {
    __shared__ __attribute__((aligned(16))) uint8_t hdr[IPOUT_WAVES][64];
    __shared__ IpoutFlow fl[IPOUT_SLOTS];
    const int s = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int n = nbytes[s] / IPOUT_TS;
    if (n > max_packets) n = max_packets;
    if (tid < IPOUT_SLOTS) fl[tid] = flows[s * IPOUT_SLOTS + tid];
    __syncthreads();
    const uint8_t* ts = in[s];
    const IpoutClock clk = clock[s];
    const uint64_t tpp = rates[s];
    const bool fl_now = flush && (flush_only < 0 || flush_only == s);
    for (int q = 0; q < IPOUT_SLOTS; ++q) {
        const IpoutFlow& f = fl[q];
        const int g = s * IPOUT_SLOTS + q;
        uint8_t* o = out[g];
        if (!f.family || !o) continue;
        const IpoutSlot st = state[g];
        int passed = call[s].passed[q];
        if (passed > n) passed = n;
        const IpoutPlan pl = ipout_plan(f, st.held, passed, fl_now);
        const uint8_t* hp = held_g + (size_t)g * IPOUT_HELD_BYTES;
        const uint16_t* idx = idx_g + (size_t)g * max_packets;
        const int P = f.packets_per_datagram, hb = ipout_header_bytes(f);
        for (int j = wave; j < pl.nd && j < max_packets; j += IPOUT_WAVES) {
            const int cnt = j < pl.nfull ? P : pl.last, t0 = j * P, off = j * (hb + IPOUT_TS * P);
            if (off + hb + IPOUT_TS * cnt > cap) continue;   // (the host launches this kernel only when every slot fits)
            // the packets: sequence index t of held ++ passing
            const int pi = lane / IPOUT_PKT_LANES, sl = lane % IPOUT_PKT_LANES;
            unsigned even = 0, odd = 0;
            if (pi < cnt) {
                const int t = t0 + pi;
                const uint8_t* src = t < st.held ? hp + IPOUT_TS * t : ts + (size_t)IPOUT_TS * idx[t - st.held];
                ip_lanes_copy(o + off + hb + IPOUT_TS * pi, src, IPOUT_TS, sl, IPOUT_PKT_LANES);
                ip_lanes_wsum(src, IPOUT_TS, sl, IPOUT_PKT_LANES, &even, &odd);
            }
            const unsigned paysum = ip_wave_wsum_reduce(even, odd);
            if (lane == 0) {
                const int tf = t0 > st.held ? t0 : st.held;  // the first packet of this call in the datagram
                const uint32_t tick = t0 < st.held ? st.held_tick : ipout_tick(clk, tpp, idx[t0 - st.held]);
                const unsigned seq = (f.seq_base + st.dgrams + (unsigned)j) & 0xFFFFu;
                uint16_t sent;
                ipout_headers(hdr[wave], f, cnt, seq, f.mode == IPOUT_MODE_RTP ? f.timestamp_base + tick : 0u, paysum, &sent);
                rows_g[(size_t)g * max_packets + j] = ipout_row(f, hb, j, cnt, seq, tick, j == 0 && st.held > 0, tf < t0 + cnt ? (int)idx[tf - st.held] : -1, sent);
            }
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
            if (lane < hb) o[off + lane] = hdr[wave][lane];
            __builtin_amdgcn_wave_barrier();                 // (lane 0 writes hdr again in the wave's next round)
        }
    }
    __syncthreads();                                         // the first datagrams have read the held packets
    {
        const int q = wave, g = s * IPOUT_SLOTS + q;
        const IpoutFlow& f = fl[q];
        if (f.family && out[g]) {
            const IpoutSlot st = state[g];
            int passed = call[s].passed[q];
            if (passed > n) passed = n;
            const IpoutPlan pl = ipout_plan(f, st.held, passed, fl_now);
            const uint16_t* idx = idx_g + (size_t)g * max_packets;
            uint8_t* hp = held_g + (size_t)g * IPOUT_HELD_BYTES;
            // no datagram: the held packets stay and the passing ones follow them; else the call's last packets, from the list's entry i0
            const int keep = pl.nd ? 0 : st.held, i0 = pl.nd ? pl.nd * f.packets_per_datagram - st.held : 0;
            for (int i = keep; i < pl.held && i < IPOUT.held_packets; ++i)
                ip_lanes_copy(hp + IPOUT_TS * i, ts + (size_t)IPOUT_TS * idx[i0 + i - keep], IPOUT_TS, lane, 64);
            if (lane == 0) {
                const uint32_t tick = keep || pl.held == 0 ? st.held_tick : ipout_tick(clk, tpp, idx[i0]);
                state[g] = IpoutSlot{st.dgrams + (unsigned)pl.nd, tick, pl.held, 0};
            }
        }
    }
    if (tid == 0) clock[s] = ipout_advance(clk, tpp, n);
}

constexpr const char* BANK = "IP output bank: ";
int fail_arg(const char* text) { last_error() = std::string(BANK) + text; return DVBS2GPU_ERR_ARG; }

}  // namespace

struct dvbs2gpu_ipout {
    dvbs2gpu_ctx* ctx = nullptr;                   // null: a host-only bank (dvbs2gpu_ipout_create_host)
    int nstreams = 0, max_packets = 0;
    std::vector<IpoutFlow> flow;                   // nstreams x 4
    std::vector<int64_t> stats;                    // nstreams x IPOUT_NCNT, since reset (a slot's since its last set_flow)
    std::vector<int> held;                         // nstreams x 4: what every slot holds (device banks: as the kernels' plan says)
    std::vector<int> nrows, need_bytes;            // of the last call, per (stream, slot)
    std::vector<IpoutCall> h_call;
    std::vector<char> h_args;                      // TsBankArgsN<4>
    // device banks
    DevBuf<IpoutFlow> d_flow;
    DevBuf<uint32_t> d_map;                        // nstreams x 4 x 256 words
    DevBuf<uint64_t> d_rate;
    DevBuf<IpoutClock> d_clock;
    DevBuf<IpoutSlot> d_state;
    DevBuf<uint8_t> d_held;                        // nstreams x 4 x 6 x 188
    DevBuf<uint16_t> d_idx;                        // nstreams x 4 x max_packets
    DevBuf<IpoutRow> d_rows;                       // nstreams x 4 x max_packets
    DevBuf<IpoutCall> d_call;
    DevBuf<char> d_args;
    Workspace st_in, st_out;                       // of the host-buffer entry point
    // host-only banks
    std::vector<IpoutHostStream> host;

    // what a call that succeeded adds: from the plan of every slot
    void account_call(int s, const IpoutCall& c, bool flush) {
        int64_t* a = stats.data() + (size_t)s * IPOUT_NCNT;
        a[0] += c.packets; a[1] += c.bad_sync;
        for (int k = 0; k < IPOUT_SLOTS; ++k) {
            const size_t g = (size_t)s * IPOUT_SLOTS + k;
            nrows[g] = 0;
            if (!flow[g].family) continue;
            const IpoutPlan pl = ipout_plan(flow[g], held[g], c.passed[k], flush);
            int64_t* q = a + IPOUT_NSTREAM_CNT + k * IPOUT_NSLOT_CNT;
            q[OC_PASSED] += c.passed[k]; q[OC_DGRAMS] += pl.nd; q[OC_SHORT] += pl.last ? 1 : 0;
            q[OC_TS_PACKETS] += (int64_t)pl.nfull * flow[g].packets_per_datagram + pl.last; q[OC_BYTES] += pl.bytes;
            q[OC_HELD] = held[g] = pl.held;
            nrows[g] = pl.nd;
        }
    }
};

namespace {

typedef TsBankArgsN<IPOUT_SLOTS> IpoutArgs;

// the device call: d_ts, nbytes, d_out (4 pointers per stream) are host arrays.  flush_only >= 0: the flush flag is that stream's alone
int ipout_batch(dvbs2gpu_ipout* b, const uint8_t* const* d_ts, const int* nbytes, uint8_t* const* d_out, int cap, int* out_bytes, int* out_rows, int flush,
                int flush_only, hipStream_t st) {
    const int n = b->nstreams, ns = n * IPOUT_SLOTS;
    HIP_TRY(hipSetDevice(b->ctx->device));
    const IpoutArgs a((size_t)n);
    a.fill(b->h_args.data(), n, d_ts, d_out, nbytes);
    HIP_TRY(hipMemcpyAsync(b->d_args, b->h_args.data(), b->h_args.size(), hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(ipout_scan_kernel, dim3(n), dim3(IPOUT_WG), 0, st, a.in(b->d_args.get()), a.nbytes(b->d_args.get()), b->max_packets, b->d_flow, b->d_map, b->d_state,
                       b->d_idx, b->d_call, flush, flush_only);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(b->h_call.data(), b->d_call, sizeof(IpoutCall) * (size_t)n, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    bool fits = true;
    for (int g = 0; g < ns; ++g) {
        const int need = b->h_call[g / IPOUT_SLOTS].needed[g % IPOUT_SLOTS];
        fits &= need <= cap;
        b->need_bytes[g] = need;
        if (out_bytes) out_bytes[g] = need;
    }
    if (!fits) {                                       // nothing has been stored: the same call may come again with more room
        std::fill(b->nrows.begin(), b->nrows.end(), 0);
        for (int g = 0; out_rows && g < ns; ++g) out_rows[g] = 0;
        last_error() = std::string(BANK) + "the datagrams of a slot do not fit cap (out_bytes holds the sizes)";
        return DVBS2GPU_ERR_CAPACITY;
    }
    hipLaunchKernelGGL(ipout_commit_kernel, dim3(n), dim3(IPOUT_WG), 0, st, a.in(b->d_args.get()), a.nbytes(b->d_args.get()), a.out(b->d_args.get()), b->max_packets, cap,
                       b->d_flow, b->d_rate, b->d_clock, b->d_state, b->d_held, b->d_idx, b->d_call, b->d_rows, flush, flush_only);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(st));
    for (int i = 0; i < n; ++i) b->account_call(i, b->h_call[i], flush && (flush_only < 0 || flush_only == i));
    for (int g = 0; out_rows && g < ns; ++g) out_rows[g] = b->nrows[g];
    return 0;
}

int ipout_create(dvbs2gpu_ctx* ctx, int nstreams, int max_packets, dvbs2gpu_ipout** out) {
    if (!out || nstreams <= 0 || max_packets <= 0) return DVBS2GPU_ERR_ARG;
    if (max_packets > IPOUT_MAX_PACKETS) return fail_arg("max_packets is at most 8192 per stream and call");
    if (ctx) HIP_TRY(hipSetDevice(ctx->device));
    std::unique_ptr<dvbs2gpu_ipout> b(new dvbs2gpu_ipout());
    const size_t n = (size_t)nstreams, ns = n * IPOUT_SLOTS;
    b->ctx = ctx; b->nstreams = nstreams; b->max_packets = max_packets;
    b->flow.assign(ns, IpoutFlow{});
    b->stats.assign(n * IPOUT_NCNT, 0);
    b->held.assign(ns, 0); b->nrows.assign(ns, 0); b->need_bytes.assign(ns, 0);
    b->h_call.resize(n);
    if (!ctx) {
        b->host.resize(n);
        *out = b.release();
        return 0;
    }
    const char* what = "hipMalloc(ipout)";             // (zero-filled: flows, lists, rates and state; the kernels write the rest before it is read)
    RC_TRY(b->d_flow.alloc(ns, true, what));
    RC_TRY(b->d_map.alloc(ns * IPOUT_MAP_WORDS, true, what));
    RC_TRY(b->d_rate.alloc(n, true, what));
    RC_TRY(b->d_clock.alloc(n, true, what));
    RC_TRY(b->d_state.alloc(ns, true, what));
    RC_TRY(b->d_held.alloc(ns * IPOUT_HELD_BYTES, true, what));
    RC_TRY(b->d_idx.alloc(ns * max_packets, false, what));
    RC_TRY(b->d_rows.alloc(ns * max_packets, false, what));
    RC_TRY(b->d_call.alloc(n, false, what));
    b->h_args.resize(IpoutArgs(n).L.bytes());
    RC_TRY(b->d_args.alloc(b->h_args.size(), false, what));
    *out = b.release();
    return 0;
}

// the arguments of a call for stream i: whole packets, its buffers
bool ipout_stream_ok(const dvbs2gpu_ipout* b, int i, const uint8_t* ts, int nbytes, uint8_t* const* out4) {
    if (!ts_bank_check_counts(BANK, &nbytes, 1, b->max_packets)) return false;
    if (nbytes > 0 && !ts) { fail_arg("null input buffer"); return false; }
    for (int k = 0; k < IPOUT_SLOTS; ++k) {
        if (!b->flow[(size_t)i * IPOUT_SLOTS + k].family) continue;
        if (!out4 || !out4[k] || out4[k] == ts) { fail_arg("a slot with a flow needs an output buffer, and not its stream's input"); return false; }
    }
    return true;
}

}  // namespace

extern "C" {

void dvbs2gpu_ipout_destroy(dvbs2gpu_ipout* b) { delete b; }
int dvbs2gpu_ipout_create(dvbs2gpu_ctx* ctx, int nstreams, int max_packets, dvbs2gpu_ipout** out) { return ctx ? ipout_create(ctx, nstreams, max_packets, out) : DVBS2GPU_ERR_ARG; }
int dvbs2gpu_ipout_create_host(int nstreams, int max_packets, dvbs2gpu_ipout** out) { return ipout_create(nullptr, nstreams, max_packets, out); }

int dvbs2gpu_ipout_reset(dvbs2gpu_ipout* b) {
    if (!b) return DVBS2GPU_ERR_ARG;
    if (b->ctx) {
        HIP_TRY(hipSetDevice(b->ctx->device));
        HIP_TRY(hipMemset(b->d_clock, 0, (size_t)b->nstreams * sizeof(IpoutClock)));
        HIP_TRY(hipMemset(b->d_state, 0, (size_t)b->nstreams * IPOUT_SLOTS * sizeof(IpoutSlot)));
    }
    for (IpoutHostStream& h : b->host) h.clear();
    std::fill(b->stats.begin(), b->stats.end(), 0);
    std::fill(b->held.begin(), b->held.end(), 0);
    std::fill(b->nrows.begin(), b->nrows.end(), 0);
    return 0;
}

int dvbs2gpu_ipout_get_layout(dvbs2gpu_ipout_layout* h_out) {
    if (!h_out) return DVBS2GPU_ERR_ARG;
    memcpy(h_out, &IPOUT, sizeof(IPOUT));
    return 0;
}

int dvbs2gpu_ipout_set_flow(dvbs2gpu_ipout* b, int stream, int slot, const dvbs2gpu_ipout_flow* flow, const uint16_t* pids, int npids) {
    if (!b || stream < 0 || stream >= b->nstreams || slot < 0 || slot >= IPOUT_SLOTS || npids < 0 || (npids > 0 && !pids)) return DVBS2GPU_ERR_ARG;
    IpoutFlow f = {};
    uint32_t map[IPOUT_MAP_WORDS] = {};
    if (flow && flow->family) {
        if (flow->family != 4 && flow->family != 6) return fail_arg("a flow's family is 4, 6 or 0 (the slot is empty)");
        if (flow->packets_per_datagram < 1 || flow->packets_per_datagram > IPOUT.max_packets_per_datagram) return fail_arg("packets_per_datagram is 1..7");
        if (flow->dscp > 63 || flow->mode > IPOUT_MODE_RTP || flow->pid_mode > 2) return fail_arg("dscp is 0..63, mode RAW or RTP, pid_mode 0, 1 or 2");
        for (int k = 0; k < npids; ++k) if (pids[k] >= TSMON_PIDS) return fail_arg("a PID is at most 0x1FFF");
        memcpy(&f, flow, sizeof(f));
        f.drop_null = f.drop_null != 0;
        if (f.family == 4) { memset(f.src_addr + 4, 0, 12); memset(f.dst_addr + 4, 0, 12); }
        for (int k = 0; k < npids; ++k) map[pids[k] >> 5] |= 1u << (pids[k] & 31);
    }
    const size_t at = (size_t)stream * IPOUT_SLOTS + slot;
    b->flow[at] = f;
    b->held[at] = 0;
    std::fill_n(b->stats.begin() + (size_t)stream * IPOUT_NCNT + IPOUT_NSTREAM_CNT + (size_t)slot * IPOUT_NSLOT_CNT, IPOUT_NSLOT_CNT, 0);
    if (b->ctx) {
        HIP_TRY(hipSetDevice(b->ctx->device));
        HIP_TRY(hipMemcpy(b->d_flow + at, &f, sizeof(f), hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(b->d_map + at * IPOUT_MAP_WORDS, map, sizeof(map), hipMemcpyHostToDevice));
        HIP_TRY(hipMemset(b->d_state + at, 0, sizeof(IpoutSlot)));
    } else {
        IpoutHostStream& h = b->host[stream];
        h.flow[slot] = f;
        memcpy(h.map[slot], map, sizeof(map));
        h.clear_slot(slot);
    }
    return 0;
}

int dvbs2gpu_ipout_set_rate(dvbs2gpu_ipout* b, int stream, uint64_t ticks_per_packet_q24) {
    if (!b || stream < 0 || stream >= b->nstreams) return DVBS2GPU_ERR_ARG;
    if (ticks_per_packet_q24 >> 48) return fail_arg("ticks_per_packet_q24 is below 2^48");
    if (b->ctx) {
        HIP_TRY(hipSetDevice(b->ctx->device));
        HIP_TRY(hipMemcpy(b->d_rate + stream, &ticks_per_packet_q24, sizeof(uint64_t), hipMemcpyHostToDevice));
    } else {
        b->host[stream].tpp = ticks_per_packet_q24;
    }
    return 0;
}

int dvbs2gpu_ipout_process_batch(dvbs2gpu_ipout* b, const uint8_t* const* d_ts, const int* nbytes, uint8_t* const* d_out, int cap, int* out_bytes, int* out_rows,
                                 int flush, void* stream) {
    if (!b || !d_ts || !nbytes || !d_out || !out_bytes || cap < 0) return DVBS2GPU_ERR_ARG;
    if (!b->ctx) return fail_arg("a host bank takes host buffers (dvbs2gpu_ipout_work)");
    for (int i = 0; i < b->nstreams; ++i)
        if (!ipout_stream_ok(b, i, d_ts[i], nbytes[i], d_out + (size_t)i * IPOUT_SLOTS)) return DVBS2GPU_ERR_ARG;
    return ipout_batch(b, d_ts, nbytes, d_out, cap, out_bytes, out_rows, flush != 0, -1, (hipStream_t)stream);
}

int dvbs2gpu_ipout_work(dvbs2gpu_ipout* b, int stream, const uint8_t* h_ts, int nbytes, uint8_t* const* h_out, int cap, int* out_bytes, int flush) {
    if (!b || stream < 0 || stream >= b->nstreams || cap < 0) return DVBS2GPU_ERR_ARG;
    if (!ipout_stream_ok(b, stream, h_ts, nbytes, h_out)) return DVBS2GPU_ERR_ARG;
    int* need = b->need_bytes.data() + (size_t)stream * IPOUT_SLOTS;
    if (!b->ctx) {
        IpoutHostStream& h = b->host[stream];
        std::fill(b->nrows.begin(), b->nrows.end(), 0);        // the tables are of the LAST call, which brought the other streams nothing
        std::fill(b->need_bytes.begin(), b->need_bytes.end(), 0);
        const std::unique_ptr<IpoutHostStream::State> before(new IpoutHostStream::State(h.st));     // what a capacity failure has to put back
        h.run(h_ts, nbytes / IPOUT_TS, flush != 0);
        bool fits = true;
        for (int k = 0; k < IPOUT_SLOTS; ++k) {
            need[k] = (int)h.bytes[k].size();
            if (out_bytes) out_bytes[k] = need[k];
            fits &= need[k] <= cap;
        }
        if (!fits) {
            h.st = *before;
            h.clear_call();
            last_error() = std::string(BANK) + "the datagrams of a slot do not fit cap (dvbs2gpu_ipout_get_needed holds the sizes)";
            return DVBS2GPU_ERR_CAPACITY;
        }
        IpoutCall c = {};
        c.packets = h.packets; c.bad_sync = h.bad_sync;
        memcpy(c.passed, h.passed, sizeof(c.passed));
        b->account_call(stream, c, flush != 0);
        for (int k = 0; k < IPOUT_SLOTS; ++k)
            if (!h.bytes[k].empty()) memcpy(h_out[k], h.bytes[k].data(), h.bytes[k].size());
        return 0;
    }
    // a device bank: the packets staged, room for every slot; the other streams bring nothing and keep what they hold
    HIP_TRY(hipSetDevice(b->ctx->device));
    const size_t slot_room = ((size_t)cap + 31) & ~(size_t)15;
    RC_TRY(b->st_in.ensure((size_t)b->max_packets * IPOUT_TS));
    RC_TRY(b->st_out.ensure(slot_room * IPOUT_SLOTS));
    if (nbytes > 0) HIP_TRY(hipMemcpy(b->st_in.p, h_ts, nbytes, hipMemcpyHostToDevice));
    std::vector<const uint8_t*> in(b->nstreams, nullptr);
    std::vector<int> nb(b->nstreams, 0);
    // (every slot of every stream has a pointer: a flow of another stream needs one though nothing is written through it)
    std::vector<uint8_t*> out((size_t)b->nstreams * IPOUT_SLOTS, nullptr);
    for (size_t g = 0; g < out.size(); ++g) out[g] = static_cast<uint8_t*>(b->st_out.p) + slot_room * (g % IPOUT_SLOTS);
    in[stream] = static_cast<const uint8_t*>(b->st_in.p); nb[stream] = nbytes;
    std::vector<int> ob(out.size(), 0);
    const int rc = ipout_batch(b, in.data(), nb.data(), out.data(), cap, ob.data(), nullptr, flush != 0, stream, nullptr);
    for (int k = 0; out_bytes && k < IPOUT_SLOTS; ++k) out_bytes[k] = need[k];
    if (rc < 0) return rc;
    for (int k = 0; k < IPOUT_SLOTS; ++k)
        if (need[k] > 0) HIP_TRY(hipMemcpy(h_out[k], out[(size_t)stream * IPOUT_SLOTS + k], need[k], hipMemcpyDeviceToHost));
    return 0;
}

int dvbs2gpu_ipout_get_needed(dvbs2gpu_ipout* b, int stream, int slot, int* bytes) {
    if (!b || stream < 0 || stream >= b->nstreams || slot < 0 || slot >= IPOUT_SLOTS || !bytes) return DVBS2GPU_ERR_ARG;
    *bytes = b->need_bytes[(size_t)stream * IPOUT_SLOTS + slot];
    return 0;
}

int dvbs2gpu_ipout_get_stats(dvbs2gpu_ipout* b, int stream, int slot, dvbs2gpu_ipout_stats* h_out) {
    if (!b || stream < 0 || stream >= b->nstreams || slot < -1 || slot >= IPOUT_SLOTS || !h_out) return DVBS2GPU_ERR_ARG;
    *h_out = dvbs2gpu_ipout_stats{};
    int64_t* d = reinterpret_cast<int64_t*>(h_out);
    const int64_t* a = b->stats.data() + (size_t)stream * IPOUT_NCNT;
    for (int k = 0; slot < 0 && k < IPOUT_NSTREAM_CNT; ++k) d[k] = a[k];
    for (int s = slot < 0 ? 0 : slot; s < (slot < 0 ? IPOUT_SLOTS : slot + 1); ++s)
        for (int k = 0; k < IPOUT_NSLOT_CNT; ++k) d[IPOUT_NSTREAM_CNT + k] += a[IPOUT_NSTREAM_CNT + s * IPOUT_NSLOT_CNT + k];
    return 0;
}

int dvbs2gpu_ipout_get_row_table(dvbs2gpu_ipout* b, int stream, int slot, dvbs2gpu_ipout_row* h_rows, int cap, int* n) {
    if (!b || stream < 0 || stream >= b->nstreams || slot < 0 || slot >= IPOUT_SLOTS || !n || cap < 0 || (cap > 0 && !h_rows)) return DVBS2GPU_ERR_ARG;
    const size_t g = (size_t)stream * IPOUT_SLOTS + slot;
    const int k = (*n = b->nrows[g]) < cap ? *n : cap;
    if (k <= 0) return 0;
    if (!b->ctx) { memcpy(h_rows, b->host[stream].rows[slot].data(), k * sizeof(IpoutRow)); return 0; }
    HIP_TRY(hipSetDevice(b->ctx->device));
    HIP_TRY(hipMemcpy(h_rows, b->d_rows + g * b->max_packets, k * sizeof(IpoutRow), hipMemcpyDeviceToHost));
    return 0;
}
int dvbs2gpu_ipout_get_row_table_device(dvbs2gpu_ipout* b, int stream, int slot, const dvbs2gpu_ipout_row** d_rows, int* n) {
    if (!b || !b->ctx || stream < 0 || stream >= b->nstreams || slot < 0 || slot >= IPOUT_SLOTS || !n || !d_rows) return DVBS2GPU_ERR_ARG;
    const size_t g = (size_t)stream * IPOUT_SLOTS + slot;
    *n = b->nrows[g];
    *d_rows = *n ? reinterpret_cast<const dvbs2gpu_ipout_row*>(b->d_rows + g * b->max_packets) : nullptr;
    return 0;
}

}  // extern "C"
