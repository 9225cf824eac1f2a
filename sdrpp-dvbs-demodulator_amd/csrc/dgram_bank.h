// The datagram bank: what the banks that deliver the payloads of length-prefixed units of a TS PID -- IP datagrams (mpe.hip: MPE
// sections; ule.hip: ULE SNDUs) or BBFRAMEs (t2mi.hip: T2-MI packets) -- are around their rules, stated once.  How a
// call's packets are cut into independent pieces is ts_reasm.h with the one-slot format DgramFmt below; what a wave does with one unit
// in phase D -- the head gather, the source the row rules read it through, the CRC over shares of the pieces -- is reasm_wave.h; this
// file holds the two kernels, the call record, the handle and the bodies of the C functions.  A bank supplies a description D: its
// rules (MpeRules, UleRules, T2miRules: dgram_rules.h lists the members) and
//   Stats                             the public statistics, NCNT 64-bit counters in the order of Cnt
//   BANK, CNAME, ALLOC, NOUN          "MPE bank: ", "dvbs2gpu_mpe", "hipMalloc(mpe)", "datagrams": the bank in error texts, its C prefix,
//                                     its allocations, what it delivers
//   OWN_ROWS, SIZE_LIST               the bank brings phases D and D' below as wave_row(q, v, lane, row) and sequence_pass(rows, nrows,
//                                     ss, nss, cnt, wsum); it keeps the list of the delivered sizes.  DgramIpBank: neither (MPE, ULE)
// and a handle `struct dvbs2gpu_x : DgramBank<D> {}`; the C functions pass the handle and forward.
//
//   dgram_scan_kernel<D>    one workgroup per (stream, slot); an empty slot returns at once.
//     A-C  ts_reasm.h: the slot's packets into LDS, one lane for the continuity walk, one lane per PUSI packet and one for the unit
//        carried in, one record per row.
//     D  one wave per row.  Without D::OWN_ROWS the wave gathers the unit's first 128 bytes, two per lane, from the TS payloads
//        where they lie (behind adaptation fields they may lie a byte per TS packet), and every lane evaluates D::row_fields on them, a
//        byte read being a shuffle, the address compare a ballot and the header checksum a wave sum; lane 0 writes the row and steps its
//        counters.  Where D::takes_crc says so each lane takes the CRC-32 of its share of one PIECE from a zero register, shifted to the
//        unit's end and summed, with 2 to 16 lanes to a piece: a unit has 24 pieces at most where a T2-MI packet has 46, and a lane per
//        piece left most of the wave waiting (DESIGN).  With it, D::wave_row: t2mi.hip.
//     D' D::sequence_pass: what the finished rows, in order, do to the bytes the bank carries from unit to unit (DgramDevSlot::own) and
//        they to the rows.  Only T2-MI has one (COUNT_ERROR).
//     E  the rows do not depend on each other any more: one prefix sum over the delivered rows' bytes gives their offsets, and where
//        D::SIZE_LIST a second one their places in the list of delivered sizes.
//   dgram_commit_kernel<D>  (once the host has seen that every slot's bytes and rows fit) one workgroup per (stream, slot): a wave per
//     delivered row copies the payload -- the unit's bytes from D::ip_at(row) on, without the stuffing -- piece by piece to its
//     offset; then the open unit goes to the slot's buffer and the state is stored.
// Two launches per call and one device-to-host copy, of the call record per (stream, slot).
#pragma once
#include "reasm_wave.h"
#include "dgram_rules.h"

#include <memory>

namespace s2 {

constexpr int DGRAM_MAX_PACKETS = 4096;          // per stream and call: 10 bytes of LDS per packet
constexpr int DGRAM_WG = 256, DGRAM_WAVES = DGRAM_WG / 64;
static_assert(DGRAM_MAX_PACKETS <= 32 * DGRAM_WG, "reasm_collect keeps a thread's match flags in one 32-bit mask (ts_thread_run)");

struct DgramDevSlot { int32_t fill; uint8_t cont, own[DGRAM_OWN]; };      // own: DgramState::own
static_assert(sizeof(DgramDevSlot) == 8, "reset and set_watch clear a slot's eight bytes");
// the format of ts_reasm.h with one slot per workgroup: the bank's header, length rule and stuffing byte, every finished unit a row
template <typename D>
struct DgramFmt {
    typedef DgramDevSlot State;
    static constexpr int WG = DGRAM_WG, SLOTS = 1, BUF = D::BUF, HEADER = D::HEADER, LEN_A = D::LEN_A, LEN_B = D::LEN_B, STUFFING = D::STUFFING;
    static constexpr int NCNT = D::NCNT, C_DROPPED = D::C_DROPPED, C_BAD_UNIT = D::C_BAD_UNIT, C_SLACK = D::C_SLACK;
    __device__ static int total(unsigned a, unsigned b) { return D::total(a, b); }
    __device__ static bool is_row(unsigned, int) { return true; }
};
template <typename D> struct DgramCall { int32_t needed, nrows, watched, ndelivered; typename D::Cnt cnt; };

// what a description says that decides a row from the unit's head, carries nothing from unit to unit and keeps no size list (MPE, ULE)
struct DgramIpBank {
    static constexpr const char* NOUN = "datagrams";
    static constexpr bool OWN_ROWS = false, SIZE_LIST = false;
};

// Where D::SIZE_LIST, the sizes of slot g's delivered payloads in order: max_rows ints per slot, behind the rows of all `ns` slots in the
// rows' buffer (the list has no kernel argument of its own, so that the kernels of the banks without one are what they were)
template <typename Row>
__host__ __device__ inline int* dgram_size_list(Row* rows_g, size_t ns, int max_rows, size_t g) {
    return reinterpret_cast<int*>(rows_g + ns * max_rows) + g * max_rows;
}
template <typename D> inline size_t dgram_row_slots(size_t ns, int max_rows) {          // the rows' buffer in rows
    return ns * max_rows + (D::SIZE_LIST ? (ns * max_rows * sizeof(int) + sizeof(typename D::Row) - 1) / sizeof(typename D::Row) : 0);
}

// dynamic LDS: wa[max_packets] (dwords), rc[max_packets] (dwords), wb[max_packets] (16 bits each).  only >= 0: the one (stream, slot)
// that receives its stream's packets (the single-slot entry point); the others take an empty call
template <typename D>
__global__ void __launch_bounds__(DGRAM_WG) dgram_scan_kernel(const uint8_t* const* __restrict__ in, const int* __restrict__ nbytes, int max_packets, int max_rows, int only,
                                                              const typename D::Watch* __restrict__ watch, const DgramDevSlot* __restrict__ state,
                                                              DgramDevSlot* __restrict__ newst, const uint8_t* __restrict__ bufs, unsigned* __restrict__ wa_g,
                                                              uint16_t* __restrict__ wb_g, ReasmRec* __restrict__ recs, ReasmRec* __restrict__ opens,
                                                              typename D::Row* __restrict__ rows_g, DgramCall<D>* __restrict__ call, int have_out) {
    typedef DgramFmt<D> Fmt;
    extern __shared__ __attribute__((aligned(16))) unsigned dgram_lds[];
    __shared__ int cnt[D::NCNT], wsum[DGRAM_WAVES];
    __shared__ DgramDevSlot nss;
    const int g = blockIdx.x, s = g / D::SLOTS, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const typename D::Watch& w = watch[g];
    const int pid = w.pid;
    if (pid < 0) {                                   // an empty slot: nothing carried, nothing to do
        if (tid == 0) {
            DgramCall<D> c = {};
            call[g] = c;
            const ReasmRec none = {-2, 0, 0, 0, 0};
            opens[g] = none;
            newst[g] = state[g];
        }
        return;
    }
    unsigned* wa = dgram_lds;
    int* rc = reinterpret_cast<int*>(dgram_lds + max_packets);
    uint16_t* wb = reinterpret_cast<uint16_t*>(dgram_lds + 2 * (size_t)max_packets);
    int n = (only >= 0 && only != g) ? 0 : nbytes[s] / TSMON_TS;
    if (n > max_packets) n = max_packets;            // (the host has refused such a call)
    const DgramDevSlot ss = state[g];
    if (tid == 0) {
        nss = ss;
        const ReasmRec none = {-2, 0, 0, 0, 0};
        opens[g] = none;
    }
    if (tid < D::NCNT) cnt[tid] = 0;
    __syncthreads();
    const uint8_t* ts = in[s];
    const int W = n > 0 ? reasm_collect<DGRAM_WG>(ts, n, [&](const TsmonHdr& h) { return h.cls == TSMON_DATA && h.pid == pid ? 0 : -1; }, wa, wb, wsum) : 0;
    // B: the continuity walk, one lane
    if (tid == 0) {
        uint8_t st = ss.cont;
        const ReasmWalk c = reasm_classify<Fmt>(wa, wb, W, 0, &st);
        nss.cont = st;
        nss.fill = 0;
        cnt[D::C_PACKETS] = c.packets; cnt[D::C_SCR] = c.scrambled; cnt[D::C_MALPKT] = c.malformed;
    }
    for (int j = tid; j < W; j += DGRAM_WG) rc[j] = 0;
    __syncthreads();
    // C: units
    const ReasmView<Fmt> v = {ts, wa, wb, W, bufs + (size_t)g * D::BUF, state + g};
    ReasmRec* rec = recs + (size_t)g * max_rows;
    const ReasmOut<Fmt> o = {rc, rec, opens + g, &nss, &cnt, max_rows};
    reasm_jobs<false>(v, o);
    __syncthreads();
    const int nrows = reasm_number_rows<DGRAM_WG>(rc, W, wsum);
    const bool fits = nrows <= max_rows;
    typename D::Row* rows = rows_g + (size_t)g * max_rows;
    int needed = fits ? 0 : -1, ndelivered = 0;
    if (fits) {
        reasm_jobs<true>(v, o);
        __syncthreads();
        // D: a wave per row
        for (int r = wave; r < nrows; r += DGRAM_WAVES) {
            const ReasmRec q = rec[r];
            if constexpr (D::OWN_ROWS) D::wave_row(q, v, lane, &rows[r]);
            else {
                const int total = q.total;
                // the head (lane l keeps bytes 2 l and 2 l + 1 of the unit) and, where the rules take it, the CRC: reasm_wave.h
                const ReasmWaveSrc hd = reasm_wave_head(q, v, lane);
                uint32_t x = 0;
                if (D::takes_crc(hd.rd(0), hd.rd(1), total)) x = reasm_wave_crc(q, v, total, lane);   // (the same in every lane; a unit has two bytes at least)
                const typename D::Row row = D::template row_fields<ReasmWaveSrc>(hd, total, x == 0, w, q.j0 < 0 ? -1 : wa_k(wa[q.j0]), wa_k(wa[q.j1]));
                if (lane == 0) {
                    rows[r] = row;
                    D::account(row.flags, [&](int c) { atomicAdd(&cnt[c], 1); });
                }
            }
        }
        __syncthreads();
        // D': the rows in order and the bytes the bank carries from unit to unit
        if constexpr (D::OWN_ROWS) D::sequence_pass(rows, nrows, ss, &nss, cnt, wsum);
        // E: the offsets of the delivered rows
        {
            int r0, r1; ts_thread_run(nrows, DGRAM_WG, &r0, &r1);
            // (the watch as an argument: a lambda that captures it costs the MPE kernel its instruction stream)
            auto bytes_of = [&](int r, const typename D::Watch& of) { return have_out && D::delivers(rows[r], of) ? D::bytes_of(rows[r]) : 0; };
            int mine = 0, mine_n = 0;
            for (int r = r0; r < r1; ++r) { const int b = bytes_of(r, w); mine += b; mine_n += b > 0; }
            int at = ts_block_scan<DGRAM_WG>(mine, wsum, &needed);
            int idx = ts_block_scan<DGRAM_WG>(mine_n, wsum, &ndelivered);
            int* sizes = D::SIZE_LIST ? dgram_size_list(rows_g, gridDim.x, max_rows, g) : nullptr;
            for (int r = r0; r < r1; ++r) {
                const int b = bytes_of(r, w);
                if (b) rows[r].offset = at;
                if (D::SIZE_LIST && b) sizes[idx++] = b;
                at += b;
            }
        }
        __syncthreads();
        if (tid == 0) { cnt[D::C_DELIVERED] = ndelivered; cnt[D::C_BYTES] = needed; }
    }
    for (int j = tid; j < W; j += DGRAM_WG) { wa_g[(size_t)g * max_packets + j] = wa[j]; wb_g[(size_t)g * max_packets + j] = wb[j]; }
    __syncthreads();
    if (tid == 0) {
        newst[g] = nss;
        DgramCall<D> c;
        c.needed = needed; c.nrows = nrows; c.watched = W; c.ndelivered = ndelivered;
        int32_t* dst = reinterpret_cast<int32_t*>(&c.cnt);
        for (int k = 0; k < D::NCNT; ++k) dst[k] = cnt[k];
        call[g] = c;
    }
}

template <typename D>
__global__ void __launch_bounds__(DGRAM_WG) dgram_commit_kernel(const uint8_t* const* __restrict__ in, uint8_t* const* __restrict__ out, int max_packets, int max_rows, int cap,
                                                                DgramDevSlot* __restrict__ state, const DgramDevSlot* __restrict__ newst, uint8_t* __restrict__ bufs,
                                                                const unsigned* __restrict__ wa_g, const uint16_t* __restrict__ wb_g, const ReasmRec* __restrict__ recs,
                                                                const ReasmRec* __restrict__ opens, const typename D::Row* __restrict__ rows_g,
                                                                const DgramCall<D>* __restrict__ call) {
    const int g = blockIdx.x, s = g / D::SLOTS, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int W = call[g].watched, nrows = call[g].nrows;
    if (W > max_packets) W = max_packets;
    if (nrows > max_rows) nrows = max_rows;
    const ReasmRec q = opens[g];
    if (nrows == 0 && q.j0 == -2 && W == 0) return;  // (an empty slot, or an empty call with nothing open: the state is what it was)
    uint8_t* sbuf = bufs + (size_t)g * D::BUF;
    const ReasmView<DgramFmt<D>> v = {in[s], wa_g + (size_t)g * max_packets, wb_g + (size_t)g * max_packets, W, sbuf, state + g};
    const ReasmRec* rec = recs + (size_t)g * max_rows;
    const typename D::Row* rows = rows_g + (size_t)g * max_rows;
    uint8_t* o = out ? out[g] : nullptr;
    for (int r = wave; o && r < nrows; r += DGRAM_WAVES) {
        const int off = rows[r].offset, nb = D::bytes_of(rows[r]);
        if (off < 0 || nb <= 0 || off + nb > cap) continue;
        const int skip = D::ip_at(rows[r]);          // the payload is the unit's bytes [skip, skip + nb)
        reasm_pieces(rec[r], v, skip + nb, [&](int pos, const uint8_t* src, int len) {
            const int a = pos > skip ? pos : skip, b = pos + len;
            if (b > a) ts_wave_copy(o + off + (a - skip), TsBytes{src + (a - pos)}, b - a, lane);
        });
    }
    __syncthreads();                                 // the carried rows have read the buffer
    if (wave == 0 && q.j0 > -2)                      // the open unit: what the buffer holds already (a unit carried in and on) stays where it is
        reasm_pieces(q, v, D::BUF, [&](int pos, const uint8_t* src, int len) {
            if (src != sbuf) for (int i = lane; i < len; i += 64) sbuf[pos + i] = src[i];
        });
    if (tid == 0) state[g] = newst[g];
}

// the members of a bank's handle
template <typename D_>
struct DgramBank {
    typedef D_ D;
    typedef DgramHostStream<D> HostStream;
    dvbs2gpu_ctx* ctx = nullptr;                   // null: a host-only bank (dvbs2gpu_x_create_host)
    int nstreams = 0, max_packets = 0, max_rows = 0;
    std::vector<typename D::Watch> watch;          // nstreams x 4
    std::vector<typename D::Stats> stats;          // nstreams x 4, since reset; the kernels report each call's share (DgramCall)
    std::vector<int> nrows, need_bytes, need_rows; // of the last call per (stream, slot)
    std::vector<int> ndelivered;                   // where D::SIZE_LIST (else empty): the entries of its size list
    std::vector<DgramCall<D>> h_call;
    std::vector<char> h_args;
    // device banks
    DevBuf<typename D::Watch> d_watch;
    DevBuf<DgramDevSlot> d_state, d_newst;
    DevBuf<uint8_t> d_bufs;                        // nstreams x 4 x 4096
    DevBuf<unsigned> d_wa;                         // nstreams x 4 x max_packets: the slots' packets of the last call
    DevBuf<uint16_t> d_wb;
    DevBuf<ReasmRec> d_recs, d_opens;
    DevBuf<typename D::Row> d_rows;                // nstreams x 4 x max_rows, and where D::SIZE_LIST the size lists (dgram_size_list)
    DevBuf<DgramCall<D>> d_call;
    DevBuf<uint8_t> d_args;                        // TsBankArgsN<4>(nstreams)
    TsHostStage stage;                             // of the host-buffer entry point
    // host-only banks
    std::vector<HostStream> host;                  // nstreams x 4

    bool slot_ok(int stream, int slot) const { return stream >= 0 && stream < nstreams && slot >= 0 && slot < D::SLOTS; }
    void account_call(int g, const typename D::Cnt& c) {
        int64_t* d = reinterpret_cast<int64_t*>(&stats[g]);
        const int32_t* a = reinterpret_cast<const int32_t*>(&c);
        for (int k = 0; k < D::NCNT; ++k) d[k] += a[k];
    }
    // a slot's watch record: the slot starts afresh
    int set_watch(size_t at, const typename D::Watch& w) {
        watch[at] = w;
        stats[at] = typename D::Stats{};
        nrows[at] = 0;
        if (D::SIZE_LIST) ndelivered[at] = 0;
        if (ctx) {
            HIP_TRY(hipSetDevice(ctx->device));
            HIP_TRY(hipMemcpy(d_watch + at, &watch[at], sizeof(w), hipMemcpyHostToDevice));
            HIP_TRY(hipMemset(d_state + at, 0, sizeof(DgramDevSlot)));
        } else {
            host[at].clear();
            host[at].watch = watch[at];
        }
        return 0;
    }
};

// ------------------------------------------------------------------------------------------------- the bodies of the C functions
// H: the handle, a DgramBank<D>
template <typename... T> inline std::string dgram_text(T... parts) { std::string s; ((s += parts), ...); return s; }

// the device call: d_out 4 pointers per stream or null; only: the one (stream, slot) index that is served, -1: all
template <typename H>
int dgram_batch(H* b, const uint8_t* const* d_ts, const int* nbytes, uint8_t* const* d_out, int cap, int* out_bytes, int* out_rows, int only, hipStream_t st) {
    typedef typename H::D D;
    const int n = b->nstreams, ns = n * D::SLOTS;
    HIP_TRY(hipSetDevice(b->ctx->device));
    const TsBankArgsN<D::SLOTS> a(n);
    a.fill(b->h_args.data(), n, d_ts, d_out, nbytes);
    HIP_TRY(hipMemcpyAsync(b->d_args, b->h_args.data(), b->h_args.size(), hipMemcpyHostToDevice, st));
    const size_t lds = (size_t)b->max_packets * 10 + 16;               // <= 40 KiB
    hipLaunchKernelGGL(dgram_scan_kernel<D>, dim3(ns), dim3(DGRAM_WG), lds, st, a.in(b->d_args), a.nbytes(b->d_args), b->max_packets, b->max_rows, only, b->d_watch, b->d_state,
                       b->d_newst, b->d_bufs, b->d_wa, b->d_wb, b->d_recs, b->d_opens, b->d_rows, b->d_call, d_out ? 1 : 0);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(b->h_call.data(), b->d_call, sizeof(DgramCall<D>) * ns, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    bool fits = true;
    for (int g = 0; g < ns; ++g) {
        const DgramCall<D>& c = b->h_call[g];
        fits &= c.nrows <= b->max_rows && (!d_out || c.needed <= cap);
        b->need_bytes[g] = c.needed; b->need_rows[g] = c.nrows;
        if (out_bytes) out_bytes[g] = c.needed;
        if (out_rows) out_rows[g] = c.nrows;
    }
    if (!fits) {                                       // nothing has been stored: the same call may come again with more room
        std::fill(b->nrows.begin(), b->nrows.end(), 0);
        std::fill(b->ndelivered.begin(), b->ndelivered.end(), 0);
        last_error() = dgram_text(D::BANK, "the ", D::NOUN, " of a slot do not fit cap, or its rows max_rows (out_bytes / out_rows hold the sizes)");
        return DVBS2GPU_ERR_CAPACITY;
    }
    hipLaunchKernelGGL(dgram_commit_kernel<D>, dim3(ns), dim3(DGRAM_WG), 0, st, a.in(b->d_args), d_out ? a.out(b->d_args) : nullptr, b->max_packets, b->max_rows, cap,
                       b->d_state, b->d_newst, b->d_bufs, b->d_wa, b->d_wb, b->d_recs, b->d_opens, b->d_rows, b->d_call);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(st));
    for (int g = 0; g < ns; ++g) {
        b->account_call(g, b->h_call[g].cnt);
        b->nrows[g] = b->h_call[g].nrows;
        if (D::SIZE_LIST) b->ndelivered[g] = b->h_call[g].ndelivered;
    }
    return 0;
}

// device: a bank on ctx's device; else a host-only bank, ctx null
template <typename H>
int dgram_create(bool device, dvbs2gpu_ctx* ctx, int nstreams, int max_packets, int max_rows, H** out) {
    typedef typename H::D D;
    if ((device && !ctx) || !out || nstreams <= 0 || max_packets <= 0 || max_rows <= 0) return DVBS2GPU_ERR_ARG;
    if (max_packets > DGRAM_MAX_PACKETS) { last_error() = dgram_text(D::BANK, "max_packets is at most 4096 per stream and call"); return DVBS2GPU_ERR_ARG; }
    if (ctx) HIP_TRY(hipSetDevice(ctx->device));
    std::unique_ptr<H> b(new H());
    const size_t n = (size_t)nstreams, ns = n * D::SLOTS;
    b->ctx = ctx; b->nstreams = nstreams; b->max_packets = max_packets; b->max_rows = max_rows;
    b->watch.assign(ns, D::NO_WATCH);
    b->stats.assign(ns, typename D::Stats{});
    b->nrows.assign(ns, 0); b->need_bytes.assign(ns, 0); b->need_rows.assign(ns, 0); b->ndelivered.assign(D::SIZE_LIST ? ns : 0, 0);
    b->h_call.resize(ns);
    if (!ctx) {
        b->host.resize(ns);
        *out = b.release();
        return 0;
    }
    const char* what = D::ALLOC;                       // (zero-filled: the slots' states; the kernels write the rest before it is read)
    RC_TRY(b->d_watch.alloc(ns, false, what));
    HIP_TRY(hipMemcpy(b->d_watch, b->watch.data(), ns * sizeof(typename D::Watch), hipMemcpyHostToDevice));
    RC_TRY(b->d_state.alloc(ns, true, what));
    RC_TRY(b->d_newst.alloc(ns, false, what));
    RC_TRY(b->d_bufs.alloc(ns * D::BUF, false, what));
    RC_TRY(b->d_wa.alloc(ns * max_packets, false, what));
    RC_TRY(b->d_wb.alloc(ns * max_packets, false, what));
    RC_TRY(b->d_recs.alloc(ns * max_rows, false, what));
    RC_TRY(b->d_opens.alloc(ns, false, what));
    RC_TRY(b->d_rows.alloc(dgram_row_slots<D>(ns, max_rows), false, what));
    RC_TRY(b->d_call.alloc(ns, false, what));
    RC_TRY(b->d_args.alloc(TsBankArgsN<D::SLOTS>(n).L.bytes(), false, what));
    b->h_args.resize(TsBankArgsN<D::SLOTS>(n).L.bytes());
    *out = b.release();
    return 0;
}

template <typename H>
int dgram_reset(H* b) {
    if (!b) return DVBS2GPU_ERR_ARG;
    if (b->ctx) {
        HIP_TRY(hipSetDevice(b->ctx->device));
        HIP_TRY(hipMemset(b->d_state, 0, (size_t)b->nstreams * H::D::SLOTS * sizeof(DgramDevSlot)));
    }
    for (auto& h : b->host) h.clear();
    std::fill(b->stats.begin(), b->stats.end(), typename H::D::Stats{});
    std::fill(b->nrows.begin(), b->nrows.end(), 0);
    std::fill(b->ndelivered.begin(), b->ndelivered.end(), 0);
    return 0;
}

// the checks of set_watch that the banks share; true: `at` is the slot's index
template <typename H>
bool dgram_watch_args_ok(const H* b, int stream, int slot, int pid, size_t* at) {
    if (!b || !b->slot_ok(stream, slot)) return false;
    if (pid < -1 || pid >= TSMON_NULL_PID) { last_error() = dgram_text(H::D::BANK, "a slot's PID is 0..0x1FFE (-1 empties the slot)"); return false; }
    *at = (size_t)stream * H::D::SLOTS + slot;
    return true;
}

template <typename H>
int dgram_process_batch(H* b, const uint8_t* const* d_ts, const int* nbytes, uint8_t* const* d_out, int cap, int* out_bytes, int* out_rows, void* stream) {
    typedef typename H::D D;
    if (!b || !d_ts || !nbytes || cap < 0 || (d_out && !out_bytes)) return DVBS2GPU_ERR_ARG;
    if (!b->ctx) { last_error() = dgram_text(D::BANK, "a host bank takes host buffers (", D::CNAME, "_work)"); return DVBS2GPU_ERR_ARG; }
    for (int i = 0; i < b->nstreams; ++i) {
        if (!ts_bank_check_counts(D::BANK, nbytes + i, 1, b->max_packets)) return DVBS2GPU_ERR_ARG;
        bool bad = nbytes[i] > 0 && !d_ts[i];
        // once d_out is given every watching slot needs its output pointer, one of an empty stream too
        for (int k = 0; d_out && k < D::SLOTS; ++k) {
            uint8_t* o = d_out[i * D::SLOTS + k];
            bad |= (b->watch[(size_t)i * D::SLOTS + k].pid >= 0 && !o) || (o && o == d_ts[i]);
        }
        if (bad) { last_error() = dgram_text(D::BANK, "null buffer, or an output buffer that is its stream's input"); return DVBS2GPU_ERR_ARG; }
    }
    return dgram_batch(b, d_ts, nbytes, d_out, cap, out_bytes, out_rows, -1, (hipStream_t)stream);
}

template <typename H>
int dgram_work(H* b, int stream, int slot, const uint8_t* h_ts, int nbytes, uint8_t* h_out, int cap) {
    typedef typename H::D D;
    if (!b || !b->slot_ok(stream, slot) || nbytes < 0 || cap < 0 || (nbytes > 0 && !h_ts)) return DVBS2GPU_ERR_ARG;
    if (!ts_bank_check_counts(D::BANK, &nbytes, 1, b->max_packets)) return DVBS2GPU_ERR_ARG;
    if (h_out && h_out == h_ts) { last_error() = dgram_text(D::BANK, "the output buffer is the input"); return DVBS2GPU_ERR_ARG; }
    const int g = stream * D::SLOTS + slot;
    if (!b->ctx) {
        typename H::HostStream& h = b->host[g];
        // The tables are of the LAST call, which brought the others nothing.  An empty call changes no state (run() with no packet
        // is the identity), so the other slots are not run: their tables are emptied by count alone.  host[].rows and .bytes of those
        // slots keep what their own last call left; every getter reads them through nrows / ndelivered, which are 0.
        std::fill(b->nrows.begin(), b->nrows.end(), 0);
        std::fill(b->ndelivered.begin(), b->ndelivered.end(), 0);
        const std::unique_ptr<typename H::HostStream::State> before(new typename H::HostStream::State(h.st));    // what a capacity failure has to put back
        h.run(h_ts, nbytes / TSMON_TS, h_out != nullptr);
        const bool rows_fit = (int)h.rows.size() <= b->max_rows;
        b->need_rows[g] = (int)h.rows.size();
        b->need_bytes[g] = rows_fit ? (int)h.bytes.size() : -1;
        if (!rows_fit || (h_out && (int)h.bytes.size() > cap)) {
            h.st = *before;
            h.rows.clear(); h.bytes.clear();
            last_error() = dgram_text(D::BANK, "the ", D::NOUN, " do not fit cap, or the rows max_rows (", D::CNAME, "_get_needed holds the sizes)");
            return DVBS2GPU_ERR_CAPACITY;
        }
        b->account_call(g, h.cnt);
        b->nrows[g] = (int)h.rows.size();
        if (D::SIZE_LIST) b->ndelivered[g] = h.counter(D::C_DELIVERED);
        if (h_out && !h.bytes.empty()) memcpy(h_out, h.bytes.data(), h.bytes.size());
        return (int)h.bytes.size();
    }
    HIP_TRY(hipSetDevice(b->ctx->device));
    return ts_bank_work<D::SLOTS>(b->stage, b->nstreams, stream, h_ts, nbytes, b->max_packets, h_out, cap, false, [&](const uint8_t* const* in, const int* nb, uint8_t* const* out, int* ob) {
        return dgram_batch(b, in, nb, out, cap, ob, nullptr, g, nullptr);
    }, slot);
}

// the byte and row sizes the slot's last call needed, whether it succeeded or failed for capacity (bytes -1: the rows did not fit)
template <typename H>
int dgram_get_needed(H* b, int stream, int slot, int* bytes, int* rows) {
    if (!b || !b->slot_ok(stream, slot) || !bytes || !rows) return DVBS2GPU_ERR_ARG;
    *bytes = b->need_bytes[stream * H::D::SLOTS + slot]; *rows = b->need_rows[stream * H::D::SLOTS + slot];
    return 0;
}

// slot -1: the sum over the stream's slots
template <typename H>
int dgram_get_stats(H* b, int stream, int slot, typename H::D::Stats* h_out) {
    typedef typename H::D D;
    if (!b || stream < 0 || stream >= b->nstreams || slot < -1 || slot >= D::SLOTS || !h_out) return DVBS2GPU_ERR_ARG;
    *h_out = typename D::Stats{};
    int64_t* d = reinterpret_cast<int64_t*>(h_out);
    for (int s = slot < 0 ? 0 : slot; s < (slot < 0 ? D::SLOTS : slot + 1); ++s) {
        const int64_t* a = reinterpret_cast<const int64_t*>(&b->stats[(size_t)stream * D::SLOTS + s]);
        for (int k = 0; k < D::NCNT; ++k) d[k] += a[k];
    }
    return 0;
}

template <typename H, typename Pub>
int dgram_get_row_table(H* b, int stream, int slot, Pub* h_rows, int cap, int* n) {
    return ts_bank_rows<H::D::SLOTS>(static_cast<DgramBank<typename H::D>*>(b), &DgramBank<typename H::D>::max_rows, stream, h_rows, cap, n, slot);
}
template <typename H, typename Pub>
int dgram_get_row_table_device(H* b, int stream, int slot, const Pub** d_rows, int* n) {
    return ts_bank_rows_device<H::D::SLOTS>(static_cast<DgramBank<typename H::D>*>(b), &DgramBank<typename H::D>::max_rows, stream, d_rows, n, slot);
}

}  // namespace s2
