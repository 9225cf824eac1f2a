// ULE bank (own extension; include/dvbs2gpu.h): the SNDUs (Unidirectional Lightweight Encapsulation, RFC 4326) of a
// PID of each of `nstreams` transport streams in HBM, reassembled, checked (CRC-32, NPA filter, extension headers, bridged frames, IP
// header) and their IP datagrams laid back to back per slot.  Every rule is in ule_rules.h, whose UleHostStream is the sequential
// definition, the host bank and the kernels' yardstick.  How a call's packets are cut into independent pieces is ts_reasm.h with the
// one-slot format UleFmt below (the MPE bank's arrangement); what a wave does with one unit -- head gather, CRC over shares of the
// pieces -- is reasm_wave.h, shared with mpe.hip; this file holds what is the bank's own.
//
//   ule_scan_kernel     one workgroup per (stream, slot); an empty slot returns at once.
//     A-C  ts_reasm.h: the slot's packets into LDS, one lane for the continuity walk, one lane per PUSI packet and one for the SNDU
//        carried in, one record per row.
//     D  one wave per row.  The wave gathers the SNDU's first 128 bytes, two per lane, from the TS payloads where they lie (all 128 can
//        decide a row: base header, NPA, 40 bytes of optional headers, a bridged MAC header, an IPv4 header with options, the ports),
//        takes the CRC-32 (always: there is no unchecked SNDU) with 2 to 16 lanes to a piece, and every lane evaluates ule_row_fields,
//        a byte read being a shuffle, the NPA compare a ballot over six lanes and the header checksum a wave sum.  The extension-header
//        walk is data dependent, but every lane walks the same chain from the same shuffled bytes: no divergence.  Lane 0 writes the row.
//     E  the rows do not depend on each other: one prefix sum over the delivered rows' bytes gives their offsets.
//   ule_commit_kernel   (once the host has seen that every slot's bytes and rows fit) one workgroup per (stream, slot): a wave per
//     delivered row copies the datagram -- the SNDU's bytes from ule_ip_at(row) on, without the stuffing -- piece by piece to its
//     offset; then the open SNDU goes to the slot's 4096-byte buffer and the state is stored.
// Two launches per call and one device-to-host copy, of the call record per (stream, slot).
#include "reasm_wave.h"
#include "ule_rules.h"

#include <memory>

using namespace s2;
#define g_err last_error()

namespace s2 {

constexpr int ULE_MAX_PACKETS = 4096;            // per stream and call: 10 bytes of LDS per packet
constexpr int ULE_WG = 256, ULE_WAVES = ULE_WG / 64, ULE_HEAD = REASM_HEAD;
static_assert(sizeof(UleRow) == sizeof(dvbs2gpu_ule_row) && sizeof(UleRow) == 48, "row layout");
static_assert(sizeof(UleLayout) == sizeof(dvbs2gpu_ule_layout), "layout layout");
static_assert(ULE_MAX_PACKETS <= 32 * ULE_WG, "reasm_collect keeps a thread's match flags in one 32-bit mask (ts_thread_run)");
static_assert(sizeof(UleCnt) == ULE_NCNT * sizeof(int32_t), "counter order");
static_assert(sizeof(dvbs2gpu_ule_stats) == ULE_NCNT * sizeof(int64_t), "stats order");
static_assert(sizeof(UleWatch) == 20, "watch layout");
static_assert(ULE.max_sndu_bytes <= ULE_BUF && ULE.max_sndu_bytes < (1 << 17), "crc32m_xpow takes 17 bits of length");
static_assert(ULE.head_bytes == ULE_HEAD && ULE_HEAD == 2 * 64, "the head gather, two bytes per lane, holds exactly what a row reads");

struct UleDevSlot { int32_t fill; uint8_t cont, pad[3]; };
// the SNDU format of ts_reasm.h with one slot per workgroup: the length is known from the first two bytes (D and the 15-bit Length), a
// Length beyond 4092 is bad, 0xFF in an SNDU's first place is stuffing (End Indicator and padding alike), every finished SNDU a row
struct UleFmt {
    typedef UleDevSlot State;
    static constexpr int WG = ULE_WG, SLOTS = 1, BUF = ULE_BUF, HEADER = ULE.length_bytes, LEN_A = 0, LEN_B = 1, STUFFING = 0xFF;
    static constexpr int NCNT = ULE_NCNT, C_DROPPED = ULC_DROPPED, C_BAD_UNIT = ULC_MALSNDU, C_SLACK = ULC_SLACK;
    __device__ static int total(unsigned b0, unsigned b1) { return ule_total(b0, b1); }
    __device__ static bool is_row(unsigned, int) { return true; }
};
typedef ReasmRec UleRec;
typedef ReasmView<UleFmt> UleView;
struct UleCall { int32_t needed, nrows, watched, ndelivered; UleCnt cnt; };

// dynamic LDS: wa[max_packets] (dwords), rc[max_packets] (dwords), wb[max_packets] (16 bits each).  only >= 0: the one (stream, slot)
// that receives its stream's packets (the single-slot entry point); the others take an empty call
__global__ void __launch_bounds__(ULE_WG) ule_scan_kernel(const uint8_t* const* __restrict__ in, const int* __restrict__ nbytes, int max_packets, int max_rows, int only,
                                                          const UleWatch* __restrict__ watch, const UleDevSlot* __restrict__ state, UleDevSlot* __restrict__ newst,
                                                          const uint8_t* __restrict__ bufs, unsigned* __restrict__ wa_g, uint16_t* __restrict__ wb_g,
                                                          UleRec* __restrict__ recs, UleRec* __restrict__ opens, UleRow* __restrict__ rows_g, UleCall* __restrict__ call,
                                                          int have_out) {
    extern __shared__ __attribute__((aligned(16))) unsigned ule_lds[];
    __shared__ int cnt[ULE_NCNT], wsum[ULE_WAVES];
    __shared__ UleDevSlot nss;
    const int g = blockIdx.x, s = g / ULE_SLOTS, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const UleWatch& w = watch[g];
    const int pid = w.pid;
    if (pid < 0) {                                   // an empty slot: nothing carried, nothing to do
        if (tid == 0) {
            UleCall c = {};
            call[g] = c;
            const UleRec none = {-2, 0, 0, 0, 0};
            opens[g] = none;
            newst[g] = state[g];
        }
        return;
    }
    unsigned* wa = ule_lds;
    int* rc = reinterpret_cast<int*>(ule_lds + max_packets);
    uint16_t* wb = reinterpret_cast<uint16_t*>(ule_lds + 2 * (size_t)max_packets);
    int n = (only >= 0 && only != g) ? 0 : nbytes[s] / TSMON_TS;
    if (n > max_packets) n = max_packets;            // (the host has refused such a call)
    const UleDevSlot ss = state[g];
    if (tid == 0) {
        nss = ss;
        const UleRec none = {-2, 0, 0, 0, 0};
        opens[g] = none;
    }
    if (tid < ULE_NCNT) cnt[tid] = 0;
    __syncthreads();
    const uint8_t* ts = in[s];
    const int W = n > 0 ? reasm_collect<ULE_WG>(ts, n, [&](const TsmonHdr& h) { return h.cls == TSMON_DATA && h.pid == pid ? 0 : -1; }, wa, wb, wsum) : 0;
    // B: the continuity walk, one lane
    if (tid == 0) {
        uint8_t st = ss.cont;
        const ReasmWalk c = reasm_classify<UleFmt>(wa, wb, W, 0, &st);
        nss.cont = st;
        nss.fill = 0;
        cnt[ULC_PACKETS] = c.packets; cnt[ULC_SCR] = c.scrambled; cnt[ULC_MALPKT] = c.malformed;
    }
    for (int j = tid; j < W; j += ULE_WG) rc[j] = 0;
    __syncthreads();
    // C: SNDUs
    const UleView v = {ts, wa, wb, W, bufs + (size_t)g * ULE_BUF, state + g};
    UleRec* rec = recs + (size_t)g * max_rows;
    const ReasmOut<UleFmt> o = {rc, rec, opens + g, &nss, &cnt, max_rows};
    reasm_jobs<false>(v, o);
    __syncthreads();
    const int nrows = reasm_number_rows<ULE_WG>(rc, W, wsum);
    const bool fits = nrows <= max_rows;
    UleRow* rows = rows_g + (size_t)g * max_rows;
    int needed = fits ? 0 : -1, ndelivered = 0;
    if (fits) {
        reasm_jobs<true>(v, o);
        __syncthreads();
        // D: a wave per row
        for (int r = wave; r < nrows; r += ULE_WAVES) {
            const UleRec q = rec[r];
            const int total = q.total;
            // the head (lane l keeps bytes 2 l and 2 l + 1 of the SNDU) and the CRC, which the rules always take: reasm_wave.h
            const ReasmWaveSrc hd = reasm_wave_head(q, v, lane);
            const uint32_t x = reasm_wave_crc(q, v, total, lane);
            const UleRow row = ule_row_fields(hd, total, x == 0, w, q.j0 < 0 ? -1 : wa_k(wa[q.j0]), wa_k(wa[q.j1]));
            if (lane == 0) {
                rows[r] = row;
                ule_account(row.flags, [&](int c) { atomicAdd(&cnt[c], 1); });
            }
        }
        __syncthreads();
        // E: the offsets of the delivered rows
        {
            int r0, r1; ts_thread_run(nrows, ULE_WG, &r0, &r1);
            auto bytes_of = [&](int r) { return have_out && (rows[r].flags & ULE_DATAGRAM) ? rows[r].bytes : 0; };
            int mine = 0, mine_n = 0;
            for (int r = r0; r < r1; ++r) { const int b = bytes_of(r); mine += b; mine_n += b > 0; }
            int at = ts_block_scan<ULE_WG>(mine, wsum, &needed);
            ts_block_scan<ULE_WG>(mine_n, wsum, &ndelivered);
            for (int r = r0; r < r1; ++r) {
                const int b = bytes_of(r);
                if (b) rows[r].offset = at;
                at += b;
            }
        }
        __syncthreads();
        if (tid == 0) { cnt[ULC_DELIVERED] = ndelivered; cnt[ULC_BYTES] = needed; }
    }
    for (int j = tid; j < W; j += ULE_WG) { wa_g[(size_t)g * max_packets + j] = wa[j]; wb_g[(size_t)g * max_packets + j] = wb[j]; }
    __syncthreads();
    if (tid == 0) {
        newst[g] = nss;
        UleCall c;
        c.needed = needed; c.nrows = nrows; c.watched = W; c.ndelivered = ndelivered;
        int32_t* dst = reinterpret_cast<int32_t*>(&c.cnt);
        for (int k = 0; k < ULE_NCNT; ++k) dst[k] = cnt[k];
        call[g] = c;
    }
}

__global__ void __launch_bounds__(ULE_WG) ule_commit_kernel(const uint8_t* const* __restrict__ in, uint8_t* const* __restrict__ out, int max_packets, int max_rows, int cap,
                                                            UleDevSlot* __restrict__ state, const UleDevSlot* __restrict__ newst, uint8_t* __restrict__ bufs,
                                                            const unsigned* __restrict__ wa_g, const uint16_t* __restrict__ wb_g, const UleRec* __restrict__ recs,
                                                            const UleRec* __restrict__ opens, const UleRow* __restrict__ rows_g, const UleCall* __restrict__ call) {
    const int g = blockIdx.x, s = g / ULE_SLOTS, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int W = call[g].watched, nrows = call[g].nrows;
    if (W > max_packets) W = max_packets;
    if (nrows > max_rows) nrows = max_rows;
    const UleRec q = opens[g];
    if (nrows == 0 && q.j0 == -2 && W == 0) return;  // (an empty slot, or an empty call with nothing open: the state is what it was)
    uint8_t* sbuf = bufs + (size_t)g * ULE_BUF;
    const UleView v = {in[s], wa_g + (size_t)g * max_packets, wb_g + (size_t)g * max_packets, W, sbuf, state + g};
    const UleRec* rec = recs + (size_t)g * max_rows;
    const UleRow* rows = rows_g + (size_t)g * max_rows;
    uint8_t* o = out ? out[g] : nullptr;
    for (int r = wave; o && r < nrows; r += ULE_WAVES) {
        const int off = rows[r].offset, nb = rows[r].bytes;
        if (off < 0 || nb <= 0 || off + nb > cap) continue;
        const int skip = ule_ip_at(rows[r]);         // the datagram is the SNDU's bytes [skip, skip + nb)
        reasm_pieces(rec[r], v, skip + nb, [&](int pos, const uint8_t* src, int len) {
            const int a = pos > skip ? pos : skip, b = pos + len;
            if (b > a) ts_wave_copy(o + off + (a - skip), TsBytes{src + (a - pos)}, b - a, lane);
        });
    }
    __syncthreads();                                 // the carried rows have read the buffer
    if (wave == 0 && q.j0 > -2)                      // the open SNDU: what the buffer holds already (an SNDU carried in and on) stays where it is
        reasm_pieces(q, v, ULE_BUF, [&](int pos, const uint8_t* src, int len) {
            if (src != sbuf) for (int i = lane; i < len; i += 64) sbuf[pos + i] = src[i];
        });
    if (tid == 0) state[g] = newst[g];
}

}  // namespace s2

struct dvbs2gpu_ule {
    dvbs2gpu_ctx* ctx = nullptr;                   // null: a host-only bank (dvbs2gpu_ule_create_host)
    int nstreams = 0, max_packets = 0, max_rows = 0;
    std::vector<UleWatch> watch;                   // nstreams x 4
    std::vector<dvbs2gpu_ule_stats> stats;         // nstreams x 4, since reset; the kernels report each call's share (UleCall)
    std::vector<int> nrows, need_bytes, need_rows; // of the last call per (stream, slot)
    std::vector<UleCall> h_call;
    std::vector<char> h_args;
    // device banks
    DevBuf<UleWatch> d_watch;
    DevBuf<UleDevSlot> d_state, d_newst;
    DevBuf<uint8_t> d_bufs;                        // nstreams x 4 x 4096
    DevBuf<unsigned> d_wa;                         // nstreams x 4 x max_packets: the slots' packets of the last call
    DevBuf<uint16_t> d_wb;
    DevBuf<UleRec> d_recs, d_opens;
    DevBuf<UleRow> d_rows;                         // nstreams x 4 x max_rows
    DevBuf<UleCall> d_call;
    DevBuf<uint8_t> d_args;                        // TsBankArgsN<4>(nstreams)
    TsHostStage stage;                             // of the host-buffer entry point
    // host-only banks
    std::vector<UleHostStream> host;               // nstreams x 4
};

namespace s2 {
constexpr UleWatch ULE_NO_WATCH = {-1, {0, 0, 0, 0, 0, 0}, {0, 0, 0, 0, 0, 0}, 0};
static void ule_account_call(dvbs2gpu_ule* b, int g, const UleCnt& c) {
    int64_t* d = reinterpret_cast<int64_t*>(&b->stats[g]);
    const int32_t* a = reinterpret_cast<const int32_t*>(&c);
    for (int k = 0; k < ULE_NCNT; ++k) d[k] += a[k];
}
static bool ule_create_args_ok(int nstreams, int max_packets, int max_rows, dvbs2gpu_ule** out) {
    if (!out || nstreams <= 0 || max_packets <= 0 || max_rows <= 0) return false;
    if (max_packets > ULE_MAX_PACKETS) { g_err = "ULE bank: max_packets is at most 4096 per stream and call"; return false; }
    return true;
}
static std::unique_ptr<dvbs2gpu_ule> ule_new(dvbs2gpu_ctx* ctx, int nstreams, int max_packets, int max_rows) {
    std::unique_ptr<dvbs2gpu_ule> b(new dvbs2gpu_ule());
    const size_t ns = (size_t)nstreams * ULE_SLOTS;
    b->ctx = ctx; b->nstreams = nstreams; b->max_packets = max_packets; b->max_rows = max_rows;
    b->watch.assign(ns, ULE_NO_WATCH);
    b->stats.assign(ns, dvbs2gpu_ule_stats{});
    b->nrows.assign(ns, 0); b->need_bytes.assign(ns, 0); b->need_rows.assign(ns, 0);
    b->h_call.resize(ns);
    return b;
}
static bool ule_slot_ok(const dvbs2gpu_ule* b, int stream, int slot) { return b && stream >= 0 && stream < b->nstreams && slot >= 0 && slot < ULE_SLOTS; }

// the device call: d_out 4 pointers per stream or null; only: the one (stream, slot) index that is served, -1: all
static int ule_batch(dvbs2gpu_ule* b, const uint8_t* const* d_ts, const int* nbytes, uint8_t* const* d_out, int cap, int* out_bytes, int* out_rows, int only,
                     hipStream_t st) {
    const int n = b->nstreams, ns = n * ULE_SLOTS;
    HIP_TRY(hipSetDevice(b->ctx->device));
    const TsBankArgsN<ULE_SLOTS> a(n);
    a.fill(b->h_args.data(), n, d_ts, d_out, nbytes);
    HIP_TRY(hipMemcpyAsync(b->d_args, b->h_args.data(), b->h_args.size(), hipMemcpyHostToDevice, st));
    const size_t lds = (size_t)b->max_packets * 10 + 16;               // <= 40 KiB
    hipLaunchKernelGGL(ule_scan_kernel, dim3(ns), dim3(ULE_WG), lds, st, a.in(b->d_args), a.nbytes(b->d_args), b->max_packets, b->max_rows, only, b->d_watch, b->d_state,
                       b->d_newst, b->d_bufs, b->d_wa, b->d_wb, b->d_recs, b->d_opens, b->d_rows, b->d_call, d_out ? 1 : 0);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(b->h_call.data(), b->d_call, sizeof(UleCall) * ns, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    bool fits = true;
    for (int g = 0; g < ns; ++g) {
        const UleCall& c = b->h_call[g];
        fits &= c.nrows <= b->max_rows && (!d_out || c.needed <= cap);
        b->need_bytes[g] = c.needed; b->need_rows[g] = c.nrows;
        if (out_bytes) out_bytes[g] = c.needed;
        if (out_rows) out_rows[g] = c.nrows;
    }
    if (!fits) {                                       // nothing has been stored: the same call may come again with more room
        std::fill(b->nrows.begin(), b->nrows.end(), 0);
        g_err = "ULE bank: the datagrams of a slot do not fit cap, or its rows max_rows (out_bytes / out_rows hold the sizes)";
        return DVBS2GPU_ERR_CAPACITY;
    }
    hipLaunchKernelGGL(ule_commit_kernel, dim3(ns), dim3(ULE_WG), 0, st, a.in(b->d_args), d_out ? a.out(b->d_args) : nullptr, b->max_packets, b->max_rows, cap, b->d_state,
                       b->d_newst, b->d_bufs, b->d_wa, b->d_wb, b->d_recs, b->d_opens, b->d_rows, b->d_call);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(st));
    for (int g = 0; g < ns; ++g) { ule_account_call(b, g, b->h_call[g].cnt); b->nrows[g] = b->h_call[g].nrows; }
    return 0;
}
}  // namespace s2

extern "C" {

void dvbs2gpu_ule_destroy(dvbs2gpu_ule* b) { delete b; }

int dvbs2gpu_ule_create(dvbs2gpu_ctx* ctx, int nstreams, int max_packets, int max_rows, dvbs2gpu_ule** out) {
    if (!ctx || !ule_create_args_ok(nstreams, max_packets, max_rows, out)) return DVBS2GPU_ERR_ARG;
    HIP_TRY(hipSetDevice(ctx->device));
    auto b = ule_new(ctx, nstreams, max_packets, max_rows);
    const size_t n = (size_t)nstreams, ns = n * ULE_SLOTS;
    const char* what = "hipMalloc(ule)";               // (zero-filled: the slots' states; the kernels write the rest before it is read)
    RC_TRY(b->d_watch.alloc(ns, false, what));
    HIP_TRY(hipMemcpy(b->d_watch, b->watch.data(), ns * sizeof(UleWatch), hipMemcpyHostToDevice));
    RC_TRY(b->d_state.alloc(ns, true, what));
    RC_TRY(b->d_newst.alloc(ns, false, what));
    RC_TRY(b->d_bufs.alloc(ns * ULE_BUF, false, what));
    RC_TRY(b->d_wa.alloc(ns * max_packets, false, what));
    RC_TRY(b->d_wb.alloc(ns * max_packets, false, what));
    RC_TRY(b->d_recs.alloc(ns * max_rows, false, what));
    RC_TRY(b->d_opens.alloc(ns, false, what));
    RC_TRY(b->d_rows.alloc(ns * max_rows, false, what));
    RC_TRY(b->d_call.alloc(ns, false, what));
    RC_TRY(b->d_args.alloc(TsBankArgsN<ULE_SLOTS>(n).L.bytes(), false, what));
    b->h_args.resize(TsBankArgsN<ULE_SLOTS>(n).L.bytes());
    *out = b.release();
    return 0;
}

int dvbs2gpu_ule_create_host(int nstreams, int max_packets, int max_rows, dvbs2gpu_ule** out) {
    if (!ule_create_args_ok(nstreams, max_packets, max_rows, out)) return DVBS2GPU_ERR_ARG;
    auto b = ule_new(nullptr, nstreams, max_packets, max_rows);
    b->host.resize((size_t)nstreams * ULE_SLOTS);
    *out = b.release();
    return 0;
}

int dvbs2gpu_ule_reset(dvbs2gpu_ule* b) {
    if (!b) return DVBS2GPU_ERR_ARG;
    if (b->ctx) {
        HIP_TRY(hipSetDevice(b->ctx->device));
        HIP_TRY(hipMemset(b->d_state, 0, (size_t)b->nstreams * ULE_SLOTS * sizeof(UleDevSlot)));
    }
    for (auto& h : b->host) h.clear();
    std::fill(b->stats.begin(), b->stats.end(), dvbs2gpu_ule_stats{});
    std::fill(b->nrows.begin(), b->nrows.end(), 0);
    return 0;
}

int dvbs2gpu_ule_get_layout(dvbs2gpu_ule_layout* h_out) {
    if (!h_out) return DVBS2GPU_ERR_ARG;
    memcpy(h_out, &ULE, sizeof(ULE));
    return 0;
}

int dvbs2gpu_ule_set_watch(dvbs2gpu_ule* b, int stream, int slot, int pid, const uint8_t npa_value[6], const uint8_t npa_mask[6], int accept_unaddressed) {
    if (!ule_slot_ok(b, stream, slot)) return DVBS2GPU_ERR_ARG;
    if (pid < -1 || pid >= TSMON_NULL_PID) {
        g_err = "ULE bank: a slot's PID is 0..0x1FFE (-1 empties the slot)";
        return DVBS2GPU_ERR_ARG;
    }
    const size_t at = (size_t)stream * ULE_SLOTS + slot;
    UleWatch w = ULE_NO_WATCH;
    w.pid = pid;
    if (pid >= 0 && npa_value) memcpy(w.npa_value, npa_value, 6);
    if (pid >= 0 && npa_mask) memcpy(w.npa_mask, npa_mask, 6);
    if (pid >= 0) w.accept_unaddressed = accept_unaddressed != 0;
    b->watch[at] = w;
    b->stats[at] = dvbs2gpu_ule_stats{};
    b->nrows[at] = 0;
    if (b->ctx) {
        HIP_TRY(hipSetDevice(b->ctx->device));
        HIP_TRY(hipMemcpy(b->d_watch + at, &b->watch[at], sizeof(UleWatch), hipMemcpyHostToDevice));
        HIP_TRY(hipMemset(b->d_state + at, 0, sizeof(UleDevSlot)));
    } else {
        b->host[at].clear();
        b->host[at].watch = b->watch[at];
    }
    return 0;
}

int dvbs2gpu_ule_process_batch(dvbs2gpu_ule* b, const uint8_t* const* d_ts, const int* nbytes, uint8_t* const* d_out, int cap, int* out_bytes, int* out_rows,
                               void* stream) {
    if (!b || !d_ts || !nbytes || cap < 0 || (d_out && !out_bytes)) return DVBS2GPU_ERR_ARG;
    if (!b->ctx) { g_err = "ULE bank: a host bank takes host buffers (dvbs2gpu_ule_work)"; return DVBS2GPU_ERR_ARG; }
    for (int i = 0; i < b->nstreams; ++i) {
        if (!ts_bank_check_counts("ULE bank: ", nbytes + i, 1, b->max_packets)) return DVBS2GPU_ERR_ARG;
        bool bad = nbytes[i] > 0 && !d_ts[i];
        // once d_out is given every watching slot needs its output pointer, one of an empty stream too
        for (int k = 0; d_out && k < ULE_SLOTS; ++k) {
            uint8_t* o = d_out[i * ULE_SLOTS + k];
            bad |= (b->watch[(size_t)i * ULE_SLOTS + k].pid >= 0 && !o) || (o && o == d_ts[i]);
        }
        if (bad) { g_err = "ULE bank: null buffer, or an output buffer that is its stream's input"; return DVBS2GPU_ERR_ARG; }
    }
    return ule_batch(b, d_ts, nbytes, d_out, cap, out_bytes, out_rows, -1, (hipStream_t)stream);
}

int dvbs2gpu_ule_work(dvbs2gpu_ule* b, int stream, int slot, const uint8_t* h_ts, int nbytes, uint8_t* h_out, int cap) {
    if (!ule_slot_ok(b, stream, slot) || nbytes < 0 || cap < 0 || (nbytes > 0 && !h_ts)) return DVBS2GPU_ERR_ARG;
    if (!ts_bank_check_counts("ULE bank: ", &nbytes, 1, b->max_packets)) return DVBS2GPU_ERR_ARG;
    if (h_out && h_out == h_ts) { g_err = "ULE bank: the output buffer is the input"; return DVBS2GPU_ERR_ARG; }
    const int g = stream * ULE_SLOTS + slot;
    if (!b->ctx) {
        UleHostStream& h = b->host[g];
        // The tables are of the LAST call, which brought the others nothing.  An empty call changes no state (run() with no packet
        // is the identity), so the other slots are not run: their tables are emptied by count alone.
        std::fill(b->nrows.begin(), b->nrows.end(), 0);
        const std::unique_ptr<UleState> before(new UleState(h.st));    // what a capacity failure has to put back
        h.run(h_ts, nbytes / TSMON_TS, h_out != nullptr);
        const bool rows_fit = (int)h.rows.size() <= b->max_rows;
        b->need_rows[g] = (int)h.rows.size();
        b->need_bytes[g] = rows_fit ? (int)h.bytes.size() : -1;
        if (!rows_fit || (h_out && (int)h.bytes.size() > cap)) {
            h.st = *before;
            h.rows.clear(); h.bytes.clear();
            g_err = "ULE bank: the datagrams do not fit cap, or the rows max_rows (dvbs2gpu_ule_get_needed holds the sizes)";
            return DVBS2GPU_ERR_CAPACITY;
        }
        ule_account_call(b, g, h.cnt);
        b->nrows[g] = (int)h.rows.size();
        if (h_out && !h.bytes.empty()) memcpy(h_out, h.bytes.data(), h.bytes.size());
        return (int)h.bytes.size();
    }
    HIP_TRY(hipSetDevice(b->ctx->device));
    return ts_bank_work<ULE_SLOTS>(b->stage, b->nstreams, stream, h_ts, nbytes, b->max_packets, h_out, cap, false, [&](const uint8_t* const* in, const int* nb, uint8_t* const* out, int* ob) {
        return ule_batch(b, in, nb, out, cap, ob, nullptr, g, nullptr);
    }, slot);
}

/* the byte and row sizes the slot's last call needed, whether it succeeded or failed for capacity (bytes -1: the rows did not fit) */
int dvbs2gpu_ule_get_needed(dvbs2gpu_ule* b, int stream, int slot, int* bytes, int* rows) {
    if (!ule_slot_ok(b, stream, slot) || !bytes || !rows) return DVBS2GPU_ERR_ARG;
    *bytes = b->need_bytes[stream * ULE_SLOTS + slot]; *rows = b->need_rows[stream * ULE_SLOTS + slot];
    return 0;
}

int dvbs2gpu_ule_get_stats(dvbs2gpu_ule* b, int stream, int slot, dvbs2gpu_ule_stats* h_out) {
    if (!b || stream < 0 || stream >= b->nstreams || slot < -1 || slot >= ULE_SLOTS || !h_out) return DVBS2GPU_ERR_ARG;
    *h_out = dvbs2gpu_ule_stats{};
    int64_t* d = reinterpret_cast<int64_t*>(h_out);
    for (int s = slot < 0 ? 0 : slot; s < (slot < 0 ? ULE_SLOTS : slot + 1); ++s) {
        const int64_t* a = reinterpret_cast<const int64_t*>(&b->stats[(size_t)stream * ULE_SLOTS + s]);
        for (int k = 0; k < ULE_NCNT; ++k) d[k] += a[k];
    }
    return 0;
}

int dvbs2gpu_ule_get_row_table(dvbs2gpu_ule* b, int stream, int slot, dvbs2gpu_ule_row* h_rows, int cap, int* n) {
    return ts_bank_rows<ULE_SLOTS>(b, &dvbs2gpu_ule::max_rows, stream, h_rows, cap, n, slot);
}

int dvbs2gpu_ule_get_row_table_device(dvbs2gpu_ule* b, int stream, int slot, const dvbs2gpu_ule_row** d_rows, int* n) {
    return ts_bank_rows_device<ULE_SLOTS>(b, &dvbs2gpu_ule::max_rows, stream, d_rows, n, slot);
}

}  // extern "C"
