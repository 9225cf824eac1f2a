// The watched-PID bank: what the banks that judge up to 16 watched PIDs per stream and write one row table per stream (pcr.hip: the
// PCRs; pes.hip: the PES packets; es.hip: the video elementary streams; aud.hip: the audio frames) are on the host
// around their kernels and rules, stated once: the handle's members and the bodies of the C functions.  The kernels stay in the .hip
// files (the device phases that PES, ES and audio share are ts_watch.h; what ES and audio share beyond them, on the device and in
// their descriptions here, is es_stream.h), the rules and the sequential host streams in *_rules.h.  A bank supplies a description D:
//   SLOTS, MAX_PACKETS                watched PIDs per stream; packets per stream and call (4096: the text of create)
//   State, Row, Call, HostStream      the slot's carried state, the row, the call record (head + cnt[SLOTS]), the sequential stream
//   Stats, StreamStats, SUMS          the public statistics; the first SUMS 64-bit words of Stats add up over slots, the rest are maxima
//   NO_STREAM_STATS                   a stream's statistics before any packet
//   Config, CONFIGS, NO_CONFIG        what a bank is told beyond the watch list, CONFIGS of them per stream (a rate per stream, a codec
//                                     per slot): the mirror cfg and its device copy d_cfg, written by the bank's own set_rate / set_watch
//   BANK, CNAME, ALLOC                "PES bank: ", "dvbs2gpu_pes", "hipMalloc(pes)": the bank in error texts, its C prefix, its allocations
//   account(b, i, npackets, head, cnt)   one stream's call into stats[], sstats[i], nrows[i] and total[i]
//   launch(b, args, stream)           the kernel launch, with the bank's LDS size
//   fix_stream_stats(StreamStats*)    what get_stream_stats turns on read (a position into "packets since")
// and a handle `struct dvbs2gpu_x : WatchBank<D> {}`; the C functions pass the handle and forward.
#pragma once
#include "ts_bank.h"

#include <memory>

namespace s2 {

template <typename D>
struct WatchBank {
    typedef D Desc;
    dvbs2gpu_ctx* ctx = nullptr;                   // null: a host-only bank (create_host)
    int nstreams = 0, max_packets = 0, max_rows = 0;
    std::vector<int32_t> watch;                    // nstreams x SLOTS
    std::vector<typename D::Config> cfg;           // nstreams x CONFIGS
    std::vector<typename D::Stats> stats;          // nstreams x SLOTS, since reset; the kernel reports each call's share (Call)
    std::vector<typename D::StreamStats> sstats;
    std::vector<int> nrows, total;                 // of the last call per stream: rows in the table, rows in all
    std::vector<typename D::Call> h_call;
    std::vector<char> h_args;
    // device banks
    DevBuf<int32_t> d_watch;
    DevBuf<typename D::Config> d_cfg;
    DevBuf<typename D::State> d_state;
    DevBuf<int64_t> d_pos;
    DevBuf<typename D::Row> d_rows;                // nstreams x max_rows
    DevBuf<typename D::Call> d_call;
    DevBuf<uint8_t> d_args;                        // TsBankArgs(nstreams)
    TsHostStage stage;                             // of the host-buffer entry point
    // host-only banks
    std::vector<typename D::HostStream> host;
};

// ------------------------------------------------------------------------------------------------- the bodies of the C functions
// H: the handle, a WatchBank<D>
template <typename D>
__attribute__((noinline, cold)) int watch_error(const char* a, const char* cname = "", const char* b = "") {
    last_error() = std::string(D::BANK) + a + cname + b;
    return DVBS2GPU_ERR_ARG;
}

// device: a bank on ctx's device; else a host-only bank, ctx null
template <typename H>
int watch_create(bool device, dvbs2gpu_ctx* ctx, int nstreams, int max_packets, int max_rows, H** out) {
    typedef typename H::Desc D;
    static_assert(D::MAX_PACKETS == 4096, "the text below");
    if ((device && !ctx) || !out || nstreams <= 0 || max_packets <= 0 || max_rows <= 0) return DVBS2GPU_ERR_ARG;
    if (max_packets > D::MAX_PACKETS) return watch_error<D>("max_packets is at most 4096 per stream and call");
    if (ctx) HIP_TRY(hipSetDevice(ctx->device));
    std::unique_ptr<H> b(new H());
    const size_t n = (size_t)nstreams, ns = n * D::SLOTS, nc = n * D::CONFIGS;
    b->ctx = ctx; b->nstreams = nstreams; b->max_packets = max_packets; b->max_rows = max_rows;
    b->watch.assign(ns, -1);
    b->cfg.assign(nc, D::NO_CONFIG);
    b->stats.assign(ns, typename D::Stats{});
    b->sstats.assign(n, D::NO_STREAM_STATS);
    b->nrows.assign(n, 0); b->total.assign(n, 0);
    b->h_call.resize(n);
    if (!ctx) {
        b->host.resize(n);
        *out = b.release();
        return 0;
    }
    const char* what = D::ALLOC;                       // (zero-filled: the slots' states and the positions; the kernel writes rows and call records before they are read)
    RC_TRY(b->d_watch.alloc(ns, false, what));
    HIP_TRY(hipMemcpy(b->d_watch, b->watch.data(), ns * sizeof(int32_t), hipMemcpyHostToDevice));
    RC_TRY(b->d_cfg.alloc(nc, false, what));
    HIP_TRY(hipMemcpy(b->d_cfg, b->cfg.data(), nc * sizeof(typename D::Config), hipMemcpyHostToDevice));
    RC_TRY(b->d_state.alloc(ns, true, what));
    RC_TRY(b->d_pos.alloc(n, true, what));
    RC_TRY(b->d_rows.alloc(n * max_rows, false, what));
    RC_TRY(b->d_call.alloc(n, false, what));
    RC_TRY(b->d_args.alloc(TsBankArgs(n).L.bytes(), false, what));
    b->h_args.resize(TsBankArgs(n).L.bytes());
    *out = b.release();
    return 0;
}

template <typename H>
int watch_reset(H* b) {
    typedef typename H::Desc D;
    if (!b) return DVBS2GPU_ERR_ARG;
    if (b->ctx) {
        HIP_TRY(hipSetDevice(b->ctx->device));
        HIP_TRY(hipMemset(b->d_state, 0, (size_t)b->nstreams * D::SLOTS * sizeof(typename D::State)));
        HIP_TRY(hipMemset(b->d_pos, 0, (size_t)b->nstreams * sizeof(int64_t)));
    }
    for (auto& h : b->host) h.reset();
    std::fill(b->stats.begin(), b->stats.end(), typename D::Stats{});
    std::fill(b->sstats.begin(), b->sstats.end(), D::NO_STREAM_STATS);
    std::fill(b->nrows.begin(), b->nrows.end(), 0);
    std::fill(b->total.begin(), b->total.end(), 0);
    return 0;
}

// set_watch in two steps, so that a bank can put a check of its own between them.  First the arguments:
template <typename H>
bool watch_slot_ok(const H* b, int stream, int slot, int pid) {
    if (!b || stream < 0 || stream >= b->nstreams || slot < 0 || slot >= H::Desc::SLOTS) return false;
    if (pid < -1 || pid >= TSMON_NULL_PID) { watch_error<typename H::Desc>("a watched PID is 0..0x1FFE (-1 clears the slot)"); return false; }
    return true;
}
// then the slot takes the PID (-1: none) with cleared statistics and state
template <typename H>
int watch_set_watch(H* b, int stream, int slot, int pid) {
    typedef typename H::Desc D;
    int32_t* w = b->watch.data() + (size_t)stream * D::SLOTS;
    for (int s = 0; s < D::SLOTS; ++s)
        if (pid >= 0 && s != slot && w[s] == pid) return watch_error<D>("the PID is watched in another slot of the stream");
    const size_t at = (size_t)stream * D::SLOTS + slot;
    w[slot] = pid;
    b->stats[at] = typename D::Stats{};
    if (b->ctx) {
        HIP_TRY(hipSetDevice(b->ctx->device));
        HIP_TRY(hipMemcpy(b->d_watch + at, &w[slot], sizeof(int32_t), hipMemcpyHostToDevice));
        HIP_TRY(hipMemset(b->d_state + at, 0, sizeof(typename D::State)));
    } else {
        b->host[stream].watch[slot] = pid;
        b->host[stream].clear_slot(slot);
    }
    return 0;
}

// entry `at` of the mirror cfg to the device (device banks)
template <typename H>
int watch_upload_config(H* b, size_t at) {
    HIP_TRY(hipSetDevice(b->ctx->device));
    HIP_TRY(hipMemcpy(b->d_cfg + at, &b->cfg[at], sizeof(typename H::Desc::Config), hipMemcpyHostToDevice));
    return 0;
}

template <typename H>
int watch_process_batch(H* b, const uint8_t* const* d_ts, const int* nbytes, int* out_rows, void* stream) {
    typedef typename H::Desc D;
    if (!b || !d_ts || !nbytes) return DVBS2GPU_ERR_ARG;
    if (!b->ctx) return watch_error<D>("a host bank takes host buffers (", D::CNAME, "_work)");
    const int n = b->nstreams;
    for (int i = 0; i < n; ++i) {
        if (!ts_bank_check_counts(D::BANK, nbytes + i, 1, b->max_packets)) return DVBS2GPU_ERR_ARG;
        if (nbytes[i] > 0 && !d_ts[i]) return watch_error<D>("null buffer");
    }
    HIP_TRY(hipSetDevice(b->ctx->device));
    hipStream_t st = (hipStream_t)stream;
    const TsBankArgs a(n);
    a.fill(b->h_args.data(), n, d_ts, nullptr, nbytes);
    HIP_TRY(hipMemcpyAsync(b->d_args, b->h_args.data(), b->h_args.size(), hipMemcpyHostToDevice, st));
    D::launch(*b, a, st);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(b->h_call.data(), b->d_call, sizeof(typename D::Call) * n, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    for (int i = 0; i < n; ++i) {
        D::account(*b, i, nbytes[i] / TSMON_TS, b->h_call[i].head, b->h_call[i].cnt);
        if (out_rows) out_rows[i] = b->total[i];
    }
    return 0;
}

template <typename H>
int watch_work(H* b, int stream, const uint8_t* h_ts, int nbytes) {
    typedef typename H::Desc D;
    if (!b || stream < 0 || stream >= b->nstreams || nbytes < 0 || (nbytes > 0 && !h_ts)) return DVBS2GPU_ERR_ARG;
    if (!ts_bank_check_counts(D::BANK, &nbytes, 1, b->max_packets)) return DVBS2GPU_ERR_ARG;
    if (!b->ctx) {
        for (int i = 0; i < b->nstreams; ++i) {        // the other streams receive an empty call
            typename D::HostStream& h = b->host[i];
            const int np = i == stream ? nbytes / TSMON_TS : 0;
            h.run(h_ts, np, b->max_rows);
            D::account(*b, i, np, h.head, h.cnt);
        }
        return b->total[stream];
    }
    HIP_TRY(hipSetDevice(b->ctx->device));
    const int rc = ts_bank_work(b->stage, b->nstreams, stream, h_ts, nbytes, b->max_packets, nullptr, 0, false, [&](const uint8_t* const* in, const int* nb, uint8_t* const*, int*) {
        return watch_process_batch(b, in, nb, nullptr, nullptr);
    });
    return rc < 0 ? rc : b->total[stream];
}

// slot -1: the stream's slots together, the sums added and the maxima as maxima
template <typename H>
int watch_get_stats(H* b, int stream, int slot, typename H::Desc::Stats* h_out) {
    typedef typename H::Desc D;
    constexpr int WORDS = sizeof(typename D::Stats) / sizeof(int64_t);
    static_assert(sizeof(typename D::Stats) == WORDS * sizeof(int64_t) && D::SUMS <= WORDS, "stats order");
    if (!b || stream < 0 || stream >= b->nstreams || slot < -1 || slot >= D::SLOTS || !h_out) return DVBS2GPU_ERR_ARG;
    *h_out = typename D::Stats{};
    int64_t* d = reinterpret_cast<int64_t*>(h_out);
    for (int s = slot < 0 ? 0 : slot; s < (slot < 0 ? D::SLOTS : slot + 1); ++s) {
        const int64_t* a = reinterpret_cast<const int64_t*>(&b->stats[(size_t)stream * D::SLOTS + s]);
        for (int k = 0; k < D::SUMS; ++k) d[k] += a[k];
        for (int k = D::SUMS; k < WORDS; ++k) if (a[k] > d[k]) d[k] = a[k];
    }
    return 0;
}

template <typename H>
int watch_get_stream_stats(H* b, int stream, typename H::Desc::StreamStats* h_out) {
    if (!b || stream < 0 || stream >= b->nstreams || !h_out) return DVBS2GPU_ERR_ARG;
    *h_out = b->sstats[stream];
    H::Desc::fix_stream_stats(h_out);
    return 0;
}

template <typename H, typename Pub>
int watch_get_row_table(H* b, int stream, Pub* h_rows, int cap, int* n) {
    return ts_bank_rows(static_cast<WatchBank<typename H::Desc>*>(b), &WatchBank<typename H::Desc>::max_rows, stream, h_rows, cap, n);
}
template <typename H, typename Pub>
int watch_get_row_table_device(H* b, int stream, const Pub** d_rows, int* n) {
    return ts_bank_rows_device(static_cast<WatchBank<typename H::Desc>*>(b), &WatchBank<typename H::Desc>::max_rows, stream, d_rows, n);
}

}  // namespace s2
