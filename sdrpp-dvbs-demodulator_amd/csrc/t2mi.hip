// T2-MI bank (own extension; include/dvbs2gpu.h): the T2-MI packets of a PID of each of `nstreams` transport streams
// in HBM, reassembled, checked (CRC-32, packet count) and the BBFRAMEs of the chosen PLP laid back to back for the mode-adaptation
// packetiser.  Every rule is in t2mi_rules.h, whose T2miHostStream is the sequential definition, the host bank and the kernels'
// yardstick.  How a call's packets are cut into independent pieces -- why that is possible, the packet list, the walkers and the row
// numbering -- is ts_reasm.h with the format T2Fmt below (the section bank, psi.hip, is its other user); this file holds what is the
// bank's own.
//
//   t2mi_scan_kernel    one workgroup per (stream, slot): the slots are independent reassemblers, an empty one returns at once, and
//                       a slot sees one PID, so there is no sort by slot.
//     A-C  ts_reasm.h: the slot's packets into LDS, one lane for the continuity walk, one lane per PUSI packet and one for the packet
//        carried in (a header split after 1 to 5 bytes too), one record per row.
//     D  one wave per row: each lane takes the CRC of one PIECE of the packet (its bytes in one TS payload, at most 184; 46 pieces at
//        8202 bytes, 64 a round) from a zero register, reading the bytes from the TS payloads where they lie (a gathered copy of
//        4 x 8202 bytes beside the packet list would not leave two workgroups per CU their LDS), the registers are shifted to the
//        packet's end (crc32m_mulmod, crc32m_xpow) and summed; lane 0 reads the nine bytes the row needs.
//     E  COUNT_ERROR: "the last valid row before mine" is an exclusive maximum scan over the rows; two prefix sums over the delivered
//        rows give their offsets and their places in the frame-size list.
//   t2mi_commit_kernel  (once the host has seen that every slot's bytes and rows fit) one workgroup per (stream, slot): a wave per
//     delivered row copies the BBFRAME's pieces to its offset, a dword per lane behind the unaligned head; then the open packet goes
//     to the slot's 8208-byte buffer and the state is stored.
// Two launches per call and one device-to-host copy, of the call record per (stream, slot).
#include "ts_reasm.h"
#include "t2mi_rules.h"

#include <memory>

using namespace s2;
#define g_err last_error()

namespace s2 {

constexpr int T2_MAX_PACKETS = 4096;             // per stream and call: 10 bytes of LDS per packet
constexpr int T2_WG = 256, T2_WAVES = T2_WG / 64;
static_assert(sizeof(T2miRow) == sizeof(dvbs2gpu_t2mi_row) && sizeof(T2miRow) == 32, "row layout");
static_assert(sizeof(T2miLayout) == sizeof(dvbs2gpu_t2mi_layout), "layout layout");
static_assert(T2_MAX_PACKETS <= 32 * T2_WG, "reasm_collect keeps a thread's match flags in one 32-bit mask (ts_thread_run)");
static_assert(sizeof(T2miCnt) == T2MI_NCNT * sizeof(int32_t), "counter order");
static_assert(sizeof(dvbs2gpu_t2mi_stats) == T2MI_NCNT * sizeof(int64_t), "stats order");
static_assert(T2MI.max_packet_bytes <= T2MI_BUF && T2MI.max_packet_bytes < (1 << 17), "crc32m_xpow takes 17 bits of length");

enum { T2C_PACKETS = 0, T2C_T2MI, T2C_CRC, T2C_COUNT, T2C_BB, T2C_BADPAY, T2C_DELIVERED, T2C_BYTES, T2C_DROPPED, T2C_MALPKT, T2C_SCR, T2C_SLACK };

struct T2DevSlot { int32_t fill; uint8_t cont, has_count, last_count, pad; };
// the T2-MI packet format of ts_reasm.h: one slot per workgroup, a 6-byte header with payload_bits in bytes 4 and 5, no stuffing, no
// bad length, every packet a row; what a PUSI packet's pointer bytes hold beyond the open packet's end is counted
struct T2Fmt {
    typedef T2DevSlot State;
    static constexpr int WG = T2_WG, SLOTS = 1, BUF = T2MI_BUF, HEADER = T2MI.header_bytes, LEN_A = 4, LEN_B = 5, STUFFING = -1;
    static constexpr int NCNT = T2MI_NCNT, C_DROPPED = T2C_DROPPED, C_BAD_UNIT = -1, C_SLACK = T2C_SLACK;
    __device__ static int total(unsigned b4, unsigned b5) { return t2mi_total(b4, b5); }
    __device__ static bool is_row(unsigned, int) { return true; }
};
typedef ReasmRec T2Rec;
typedef ReasmView<T2Fmt> T2View;
struct T2Call { int32_t needed, nrows, watched, ndelivered; T2miCnt cnt; };

// dynamic LDS: wa[max_packets] (dwords), rc[max_packets] (dwords), wb[max_packets] (16 bits each).  only >= 0: the one (stream, slot)
// that receives its stream's packets (the single-slot entry point); the others take an empty call
__global__ void __launch_bounds__(T2_WG) t2mi_scan_kernel(const uint8_t* const* __restrict__ in, const int* __restrict__ nbytes, int max_packets, int max_rows,
                                                          int only, const T2miWatch* __restrict__ watch, const T2DevSlot* __restrict__ state,
                                                          T2DevSlot* __restrict__ newst, const uint8_t* __restrict__ bufs, unsigned* __restrict__ wa_g,
                                                          uint16_t* __restrict__ wb_g, T2Rec* __restrict__ recs, T2Rec* __restrict__ opens,
                                                          T2miRow* __restrict__ rows_g, int* __restrict__ fb_g, T2Call* __restrict__ call, int have_out) {
    extern __shared__ __attribute__((aligned(16))) unsigned t2_lds[];
    __shared__ int cnt[T2MI_NCNT], wsum[T2_WAVES], last_valid;
    __shared__ T2DevSlot nss;
    const int g = blockIdx.x, s = g / T2MI_SLOTS, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const T2miWatch w = watch[g];
    if (w.pid < 0) {                                 // an empty slot: nothing carried, nothing to do
        if (tid == 0) {
            T2Call c = {};
            call[g] = c;
            const T2Rec none = {-2, 0, 0, 0, 0};
            opens[g] = none;
            newst[g] = state[g];
        }
        return;
    }
    unsigned* wa = t2_lds;
    int* rc = reinterpret_cast<int*>(t2_lds + max_packets);
    uint16_t* wb = reinterpret_cast<uint16_t*>(t2_lds + 2 * (size_t)max_packets);
    int n = (only >= 0 && only != g) ? 0 : nbytes[s] / TSMON_TS;
    if (n > max_packets) n = max_packets;            // (the host has refused such a call)
    const T2DevSlot ss = state[g];
    if (tid == 0) {
        nss = ss;
        last_valid = -1;
        const T2Rec none = {-2, 0, 0, 0, 0};
        opens[g] = none;
    }
    if (tid < T2MI_NCNT) cnt[tid] = 0;
    __syncthreads();
    const uint8_t* ts = in[s];
    const int W = n > 0 ? reasm_collect<T2_WG>(ts, n, [&](const TsmonHdr& h) { return h.cls == TSMON_DATA && h.pid == w.pid ? 0 : -1; }, wa, wb, wsum) : 0;
    // B: the continuity walk, one lane
    if (tid == 0) {
        uint8_t st = ss.cont;
        const ReasmWalk c = reasm_classify<T2Fmt>(wa, wb, W, 0, &st);
        nss.cont = st;
        nss.fill = 0;
        cnt[T2C_PACKETS] = c.packets; cnt[T2C_SCR] = c.scrambled; cnt[T2C_MALPKT] = c.malformed;
    }
    for (int j = tid; j < W; j += T2_WG) rc[j] = 0;
    __syncthreads();
    // C: T2-MI packets
    const T2View v = {ts, wa, wb, W, bufs + (size_t)g * T2MI_BUF, state + g};
    T2Rec* rec = recs + (size_t)g * max_rows;
    const ReasmOut<T2Fmt> o = {rc, rec, opens + g, &nss, &cnt, max_rows};
    reasm_jobs<false>(v, o);
    __syncthreads();
    const int nrows = reasm_number_rows<T2_WG>(rc, W, wsum);
    const bool fits = nrows <= max_rows;
    T2miRow* rows = rows_g + (size_t)g * max_rows;
    int needed = fits ? 0 : -1, ndelivered = 0;
    if (fits) {
        reasm_jobs<true>(v, o);
        __syncthreads();
        // D: a wave per row
        for (int r = wave; r < nrows; r += T2_WAVES) {
            const T2Rec q = rec[r];
            // A lane per PIECE (the packet's bytes in one TS payload, at most 184), 64 pieces a round: the walk only notes the lane's
            // piece, and the CRC loops of all lanes then run side by side.  (A lane per 64th of the packet, taken inside the walk,
            // has two or three lanes at work in each of the packet's pieces: 26 ms per call of tools/t2mi_bench.py)
            const int total = q.total;
            uint32_t x = lane == 0 ? crc32m_mulmod(0xFFFFFFFFu, crc32m_xpow((uint32_t)total)) : 0;
            for (int base = 0;; base += 64) {
                int idx = 0, ppos = 0, plen = 0;                                   // idx: the same in every lane
                const uint8_t* psrc = nullptr;
                reasm_pieces(q, v, total, [&](int pos, const uint8_t* src, int len) {
                    if (idx == base + lane) { ppos = pos; psrc = src; plen = len; }
                    ++idx;
                });
                uint32_t c = 0;
                int i = 0;
                for (; i + 4 <= plen; i += 4) {                                    // an unaligned dword inside the piece
                    const unsigned d = *reinterpret_cast<const ts_unaligned_u32*>(psrc + i);
                    for (int k = 0; k < 4; ++k) c = crc32m_byte(c, d >> (8 * k) & 255);
                }
                for (; i < plen; ++i) c = crc32m_byte(c, psrc[i]);
                if (plen > 0) x ^= crc32m_mulmod(c, crc32m_xpow((uint32_t)(total - ppos - plen)));
                if (idx <= base + 64) break;
            }
            for (int k = 32; k > 0; k >>= 1) x ^= __shfl_xor(x, k);
            if (lane == 0) {
                unsigned long long h8 = 0;
                unsigned h9 = 0;
                reasm_pieces(q, v, 9, [&](int pos, const uint8_t* src, int len) {
                    for (int i = 0; i < len; ++i) {
                        const int at = pos + i;
                        if (at < 8) h8 |= (unsigned long long)src[i] << (8 * at); else h9 = src[i];
                    }
                });
                auto rd = [&](int i) { return i < 8 ? (unsigned)(h8 >> (8 * i) & 255) : h9; };
                rows[r] = t2mi_row_fields(rd, total, x == 0, q.j0 < 0 ? -1 : wa_k(wa[q.j0]), wa_k(wa[q.j1]));
            }
        }
        __syncthreads();
        // E: COUNT_ERROR from the last valid row before each, then the offsets of the delivered rows
        int r0, r1; ts_thread_run(nrows, T2_WG, &r0, &r1);
        {
            int lastv = -1;
            for (int r = r0; r < r1; ++r) if (!(rows[r].flags & T2MI_CRC_ERROR)) lastv = r;
            const int prev = ts_block_scan_max(lastv, wsum);
            int has = prev >= 0 ? 1 : ss.has_count, last = prev >= 0 ? rows[prev].packet_count : ss.last_count;
            int c_crc = 0, c_cnt = 0, c_bb = 0, c_bad = 0;
            for (int r = r0; r < r1; ++r) {
                const T2miRow row = rows[r];
                if (row.flags & T2MI_CRC_ERROR) { ++c_crc; continue; }
                if (has && row.packet_count != ((last + 1) & 255)) { rows[r].flags = row.flags | T2MI_COUNT_ERROR; ++c_cnt; }
                has = 1; last = row.packet_count;
                c_bb += (row.flags & T2MI_BBFRAME) != 0; c_bad += (row.flags & T2MI_BAD_PAYLOAD) != 0;
            }
            if (c_crc) atomicAdd(&cnt[T2C_CRC], c_crc);
            if (c_cnt) atomicAdd(&cnt[T2C_COUNT], c_cnt);
            if (c_bb) atomicAdd(&cnt[T2C_BB], c_bb);
            if (c_bad) atomicAdd(&cnt[T2C_BADPAY], c_bad);
            if (lastv >= 0) atomicMax(&last_valid, lastv);
        }
        {
            auto bytes_of = [&](int r) { return have_out && t2mi_delivers(rows[r], w.plp) ? rows[r].bbframe_bytes : 0; };
            int mine = 0, mine_n = 0;
            for (int r = r0; r < r1; ++r) { const int b = bytes_of(r); mine += b; mine_n += b > 0; }
            int at = ts_block_scan<T2_WG>(mine, wsum, &needed);
            int idx = ts_block_scan<T2_WG>(mine_n, wsum, &ndelivered);
            int* fb = fb_g + (size_t)g * max_rows;
            for (int r = r0; r < r1; ++r) {
                const int b = bytes_of(r);
                rows[r].offset = b ? at : -1;
                if (b) fb[idx++] = b;
                at += b;
            }
        }
        __syncthreads();
        if (tid == 0) {
            cnt[T2C_T2MI] = nrows; cnt[T2C_DELIVERED] = ndelivered; cnt[T2C_BYTES] = needed;
            if (last_valid >= 0) { nss.has_count = 1; nss.last_count = rows[last_valid].packet_count; }
        }
    }
    for (int j = tid; j < W; j += T2_WG) { wa_g[(size_t)g * max_packets + j] = wa[j]; wb_g[(size_t)g * max_packets + j] = wb[j]; }
    __syncthreads();
    if (tid == 0) {
        newst[g] = nss;
        T2Call c;
        c.needed = needed; c.nrows = nrows; c.watched = W; c.ndelivered = ndelivered;
        int32_t* dst = reinterpret_cast<int32_t*>(&c.cnt);
        for (int k = 0; k < T2MI_NCNT; ++k) dst[k] = cnt[k];
        call[g] = c;
    }
}

__global__ void __launch_bounds__(T2_WG) t2mi_commit_kernel(const uint8_t* const* __restrict__ in, uint8_t* const* __restrict__ out, int max_packets, int max_rows,
                                                            int cap, T2DevSlot* __restrict__ state, const T2DevSlot* __restrict__ newst,
                                                            uint8_t* __restrict__ bufs, const unsigned* __restrict__ wa_g, const uint16_t* __restrict__ wb_g,
                                                            const T2Rec* __restrict__ recs, const T2Rec* __restrict__ opens, const T2miRow* __restrict__ rows_g,
                                                            const T2Call* __restrict__ call) {
    const int g = blockIdx.x, s = g / T2MI_SLOTS, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int W = call[g].watched, nrows = call[g].nrows;
    if (W > max_packets) W = max_packets;
    if (nrows > max_rows) nrows = max_rows;
    const T2Rec q = opens[g];
    if (nrows == 0 && q.j0 == -2 && W == 0) return;  // (an empty slot, or an empty call with nothing open: the state is what it was)
    uint8_t* sbuf = bufs + (size_t)g * T2MI_BUF;
    const T2View v = {in[s], wa_g + (size_t)g * max_packets, wb_g + (size_t)g * max_packets, W, sbuf, state + g};
    const T2Rec* rec = recs + (size_t)g * max_rows;
    const T2miRow* rows = rows_g + (size_t)g * max_rows;
    uint8_t* o = out ? out[g] : nullptr;
    const int skip = T2MI.header_bytes + T2MI.bbframe_prefix_bytes;
    for (int r = wave; o && r < nrows; r += T2_WAVES) {
        const int off = rows[r].offset, bb = rows[r].bbframe_bytes;
        if (off < 0 || bb <= 0 || off + bb > cap) continue;
        reasm_pieces(rec[r], v, skip + bb, [&](int pos, const uint8_t* src, int len) {
            const int a = pos > skip ? pos : skip, b = pos + len;
            if (b > a) ts_wave_copy(o + off + (a - skip), TsBytes{src + (a - pos)}, b - a, lane);
        });
    }
    __syncthreads();                                 // the carried rows have read the buffer
    if (wave == 0 && q.j0 > -2)                      // the open packet: what the buffer holds already (a packet carried in and on) stays where it is
        reasm_pieces(q, v, T2MI_BUF, [&](int pos, const uint8_t* src, int len) {
            if (src != sbuf) for (int i = lane; i < len; i += 64) sbuf[pos + i] = src[i];
        });
    if (tid == 0) state[g] = newst[g];
}

}  // namespace s2

struct dvbs2gpu_t2mi {
    dvbs2gpu_ctx* ctx = nullptr;                   // null: a host-only bank (dvbs2gpu_t2mi_create_host)
    int nstreams = 0, max_packets = 0, max_rows = 0;
    std::vector<T2miWatch> watch;                  // nstreams x 4
    std::vector<dvbs2gpu_t2mi_stats> stats;        // nstreams x 4, since reset; the kernels report each call's share (T2Call)
    std::vector<int> nrows, need_bytes, need_rows, ndelivered;   // of the last call per (stream, slot)
    std::vector<T2Call> h_call;
    std::vector<char> h_args;
    // device banks
    DevBuf<T2miWatch> d_watch;
    DevBuf<T2DevSlot> d_state, d_newst;
    DevBuf<uint8_t> d_bufs;                        // nstreams x 4 x 8208
    DevBuf<unsigned> d_wa;                         // nstreams x 4 x max_packets: the slots' packets of the last call
    DevBuf<uint16_t> d_wb;
    DevBuf<T2Rec> d_recs, d_opens;
    DevBuf<T2miRow> d_rows;                        // nstreams x 4 x max_rows
    DevBuf<int> d_fb;                              // the sizes of the delivered BBFRAMEs, nstreams x 4 x max_rows
    DevBuf<T2Call> d_call;
    DevBuf<uint8_t> d_args;                        // TsBankArgsN<4>(nstreams)
    TsHostStage stage;                             // of the host-buffer entry point
    // host-only banks
    std::vector<T2miHostStream> host;              // nstreams x 4
};

namespace s2 {
static void t2_account(dvbs2gpu_t2mi* b, int g, const T2miCnt& c) {
    int64_t* d = reinterpret_cast<int64_t*>(&b->stats[g]);
    const int32_t* a = reinterpret_cast<const int32_t*>(&c);
    for (int k = 0; k < T2MI_NCNT; ++k) d[k] += a[k];
}
static bool t2_create_args_ok(int nstreams, int max_packets, int max_rows, dvbs2gpu_t2mi** out) {
    if (!out || nstreams <= 0 || max_packets <= 0 || max_rows <= 0) return false;
    if (max_packets > T2_MAX_PACKETS) { g_err = "T2-MI bank: max_packets is at most 4096 per stream and call"; return false; }
    return true;
}
static std::unique_ptr<dvbs2gpu_t2mi> t2_new(dvbs2gpu_ctx* ctx, int nstreams, int max_packets, int max_rows) {
    std::unique_ptr<dvbs2gpu_t2mi> b(new dvbs2gpu_t2mi());
    const size_t ns = (size_t)nstreams * T2MI_SLOTS;
    b->ctx = ctx; b->nstreams = nstreams; b->max_packets = max_packets; b->max_rows = max_rows;
    b->watch.assign(ns, T2miWatch{-1, -1});
    b->stats.assign(ns, dvbs2gpu_t2mi_stats{});
    b->nrows.assign(ns, 0); b->need_bytes.assign(ns, 0); b->need_rows.assign(ns, 0); b->ndelivered.assign(ns, 0);
    b->h_call.resize(ns);
    return b;
}
static bool t2_slot_ok(const dvbs2gpu_t2mi* b, int stream, int slot) { return b && stream >= 0 && stream < b->nstreams && slot >= 0 && slot < T2MI_SLOTS; }

// the device call: d_out 4 pointers per stream or null; only: the one (stream, slot) index that is served, -1: all
static int t2_batch(dvbs2gpu_t2mi* b, const uint8_t* const* d_ts, const int* nbytes, uint8_t* const* d_out, int cap, int* out_bytes, int* out_rows, int only,
                    hipStream_t st) {
    const int n = b->nstreams, ns = n * T2MI_SLOTS;
    HIP_TRY(hipSetDevice(b->ctx->device));
    const TsBankArgsN<T2MI_SLOTS> a(n);
    a.fill(b->h_args.data(), n, d_ts, d_out, nbytes);
    HIP_TRY(hipMemcpyAsync(b->d_args, b->h_args.data(), b->h_args.size(), hipMemcpyHostToDevice, st));
    const size_t lds = (size_t)b->max_packets * 10 + 16;               // <= 40 KiB
    hipLaunchKernelGGL(t2mi_scan_kernel, dim3(ns), dim3(T2_WG), lds, st, a.in(b->d_args), a.nbytes(b->d_args), b->max_packets, b->max_rows, only, b->d_watch, b->d_state,
                       b->d_newst, b->d_bufs, b->d_wa, b->d_wb, b->d_recs, b->d_opens, b->d_rows, b->d_fb, b->d_call, d_out ? 1 : 0);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(b->h_call.data(), b->d_call, sizeof(T2Call) * ns, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    bool fits = true;
    for (int g = 0; g < ns; ++g) {
        const T2Call& c = b->h_call[g];
        fits &= c.nrows <= b->max_rows && (!d_out || c.needed <= cap);
        b->need_bytes[g] = c.needed; b->need_rows[g] = c.nrows;
        if (out_bytes) out_bytes[g] = c.needed;
        if (out_rows) out_rows[g] = c.nrows;
    }
    if (!fits) {                                       // nothing has been stored: the same call may come again with more room
        std::fill(b->nrows.begin(), b->nrows.end(), 0);
        std::fill(b->ndelivered.begin(), b->ndelivered.end(), 0);
        g_err = "T2-MI bank: the BBFRAMEs of a slot do not fit cap, or its rows max_rows (out_bytes / out_rows hold the sizes)";
        return DVBS2GPU_ERR_CAPACITY;
    }
    hipLaunchKernelGGL(t2mi_commit_kernel, dim3(ns), dim3(T2_WG), 0, st, a.in(b->d_args), d_out ? a.out(b->d_args) : nullptr, b->max_packets, b->max_rows, cap, b->d_state,
                       b->d_newst, b->d_bufs, b->d_wa, b->d_wb, b->d_recs, b->d_opens, b->d_rows, b->d_call);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(st));
    for (int g = 0; g < ns; ++g) { t2_account(b, g, b->h_call[g].cnt); b->nrows[g] = b->h_call[g].nrows; b->ndelivered[g] = b->h_call[g].ndelivered; }
    return 0;
}
}  // namespace s2

extern "C" {

void dvbs2gpu_t2mi_destroy(dvbs2gpu_t2mi* b) { delete b; }

int dvbs2gpu_t2mi_create(dvbs2gpu_ctx* ctx, int nstreams, int max_packets, int max_rows, dvbs2gpu_t2mi** out) {
    if (!ctx || !t2_create_args_ok(nstreams, max_packets, max_rows, out)) return DVBS2GPU_ERR_ARG;
    HIP_TRY(hipSetDevice(ctx->device));
    auto b = t2_new(ctx, nstreams, max_packets, max_rows);
    const size_t n = (size_t)nstreams, ns = n * T2MI_SLOTS;
    const char* what = "hipMalloc(t2mi)";              // (zero-filled: the slots' states; the kernels write the rest before it is read)
    RC_TRY(b->d_watch.alloc(ns, false, what));
    HIP_TRY(hipMemcpy(b->d_watch, b->watch.data(), ns * sizeof(T2miWatch), hipMemcpyHostToDevice));
    RC_TRY(b->d_state.alloc(ns, true, what));
    RC_TRY(b->d_newst.alloc(ns, false, what));
    RC_TRY(b->d_bufs.alloc(ns * T2MI_BUF, false, what));
    RC_TRY(b->d_wa.alloc(ns * max_packets, false, what));
    RC_TRY(b->d_wb.alloc(ns * max_packets, false, what));
    RC_TRY(b->d_recs.alloc(ns * max_rows, false, what));
    RC_TRY(b->d_opens.alloc(ns, false, what));
    RC_TRY(b->d_rows.alloc(ns * max_rows, false, what));
    RC_TRY(b->d_fb.alloc(ns * max_rows, false, what));
    RC_TRY(b->d_call.alloc(ns, false, what));
    RC_TRY(b->d_args.alloc(TsBankArgsN<T2MI_SLOTS>(n).L.bytes(), false, what));
    b->h_args.resize(TsBankArgsN<T2MI_SLOTS>(n).L.bytes());
    *out = b.release();
    return 0;
}

int dvbs2gpu_t2mi_create_host(int nstreams, int max_packets, int max_rows, dvbs2gpu_t2mi** out) {
    if (!t2_create_args_ok(nstreams, max_packets, max_rows, out)) return DVBS2GPU_ERR_ARG;
    auto b = t2_new(nullptr, nstreams, max_packets, max_rows);
    b->host.resize((size_t)nstreams * T2MI_SLOTS);
    *out = b.release();
    return 0;
}

int dvbs2gpu_t2mi_reset(dvbs2gpu_t2mi* b) {
    if (!b) return DVBS2GPU_ERR_ARG;
    if (b->ctx) {
        HIP_TRY(hipSetDevice(b->ctx->device));
        HIP_TRY(hipMemset(b->d_state, 0, (size_t)b->nstreams * T2MI_SLOTS * sizeof(T2DevSlot)));
    }
    for (auto& h : b->host) h.clear();
    std::fill(b->stats.begin(), b->stats.end(), dvbs2gpu_t2mi_stats{});
    std::fill(b->nrows.begin(), b->nrows.end(), 0);
    std::fill(b->ndelivered.begin(), b->ndelivered.end(), 0);
    return 0;
}

int dvbs2gpu_t2mi_get_layout(dvbs2gpu_t2mi_layout* h_out) {
    if (!h_out) return DVBS2GPU_ERR_ARG;
    memcpy(h_out, &T2MI, sizeof(T2MI));
    return 0;
}

int dvbs2gpu_t2mi_set_watch(dvbs2gpu_t2mi* b, int stream, int slot, int pid, int plp) {
    if (!t2_slot_ok(b, stream, slot)) return DVBS2GPU_ERR_ARG;
    if (pid < -1 || pid >= TSMON_NULL_PID || plp < -1 || plp > 255) {
        g_err = "T2-MI bank: a slot's PID is 0..0x1FFE (-1 empties the slot), its PLP 0..255 or -1 for every PLP";
        return DVBS2GPU_ERR_ARG;
    }
    const size_t at = (size_t)stream * T2MI_SLOTS + slot;
    b->watch[at] = {pid, pid < 0 ? -1 : plp};
    b->stats[at] = dvbs2gpu_t2mi_stats{};
    b->nrows[at] = 0; b->ndelivered[at] = 0;
    if (b->ctx) {
        HIP_TRY(hipSetDevice(b->ctx->device));
        HIP_TRY(hipMemcpy(b->d_watch + at, &b->watch[at], sizeof(T2miWatch), hipMemcpyHostToDevice));
        HIP_TRY(hipMemset(b->d_state + at, 0, sizeof(T2DevSlot)));
    } else {
        b->host[at].clear();
        b->host[at].watch = b->watch[at];
    }
    return 0;
}

int dvbs2gpu_t2mi_process_batch(dvbs2gpu_t2mi* b, const uint8_t* const* d_ts, const int* nbytes, uint8_t* const* d_out, int cap, int* out_bytes, int* out_rows,
                                void* stream) {
    if (!b || !d_ts || !nbytes || cap < 0 || (d_out && !out_bytes)) return DVBS2GPU_ERR_ARG;
    if (!b->ctx) { g_err = "T2-MI bank: a host bank takes host buffers (dvbs2gpu_t2mi_work)"; return DVBS2GPU_ERR_ARG; }
    for (int i = 0; i < b->nstreams; ++i) {
        if (!ts_bank_check_counts("T2-MI bank: ", nbytes + i, 1, b->max_packets)) return DVBS2GPU_ERR_ARG;
        bool bad = nbytes[i] > 0 && !d_ts[i];
        // once d_out is given every watching slot needs its output pointer, one of an empty stream too
        for (int k = 0; d_out && k < T2MI_SLOTS; ++k) {
            uint8_t* o = d_out[i * T2MI_SLOTS + k];
            bad |= (b->watch[(size_t)i * T2MI_SLOTS + k].pid >= 0 && !o) || (o && o == d_ts[i]);
        }
        if (bad) { g_err = "T2-MI bank: null buffer, or an output buffer that is its stream's input"; return DVBS2GPU_ERR_ARG; }
    }
    return t2_batch(b, d_ts, nbytes, d_out, cap, out_bytes, out_rows, -1, (hipStream_t)stream);
}

int dvbs2gpu_t2mi_work(dvbs2gpu_t2mi* b, int stream, int slot, const uint8_t* h_ts, int nbytes, uint8_t* h_out, int cap) {
    if (!t2_slot_ok(b, stream, slot) || nbytes < 0 || cap < 0 || (nbytes > 0 && !h_ts)) return DVBS2GPU_ERR_ARG;
    if (!ts_bank_check_counts("T2-MI bank: ", &nbytes, 1, b->max_packets)) return DVBS2GPU_ERR_ARG;
    if (h_out && h_out == h_ts) { g_err = "T2-MI bank: the output buffer is the input"; return DVBS2GPU_ERR_ARG; }
    const int g = stream * T2MI_SLOTS + slot;
    if (!b->ctx) {
        T2miHostStream& h = b->host[g];
        // The tables are of the LAST call, which brought the others nothing.  An empty call changes no state (run() with no packet
        // is the identity), so the other slots are not run: their tables are emptied by count alone.  host[].rows and .bytes of those
        // slots keep what their own last call left; every getter reads them through nrows / ndelivered, which are 0.
        std::fill(b->nrows.begin(), b->nrows.end(), 0);
        std::fill(b->ndelivered.begin(), b->ndelivered.end(), 0);
        const std::unique_ptr<T2miState> before(new T2miState(h.st));  // what a capacity failure has to put back
        h.run(h_ts, nbytes / TSMON_TS, h_out != nullptr);
        const bool rows_fit = (int)h.rows.size() <= b->max_rows;
        b->need_rows[g] = (int)h.rows.size();
        b->need_bytes[g] = rows_fit ? (int)h.bytes.size() : -1;
        if (!rows_fit || (h_out && (int)h.bytes.size() > cap)) {
            h.st = *before;
            h.rows.clear(); h.bytes.clear();
            g_err = "T2-MI bank: the BBFRAMEs do not fit cap, or the rows max_rows (dvbs2gpu_t2mi_get_needed holds the sizes)";
            return DVBS2GPU_ERR_CAPACITY;
        }
        t2_account(b, g, h.cnt);
        b->nrows[g] = (int)h.rows.size();
        b->ndelivered[g] = h.cnt.bbframes_delivered;
        if (h_out && !h.bytes.empty()) memcpy(h_out, h.bytes.data(), h.bytes.size());
        return (int)h.bytes.size();
    }
    HIP_TRY(hipSetDevice(b->ctx->device));
    return ts_bank_work<T2MI_SLOTS>(b->stage, b->nstreams, stream, h_ts, nbytes, b->max_packets, h_out, cap, false, [&](const uint8_t* const* in, const int* nb, uint8_t* const* out, int* ob) {
        return t2_batch(b, in, nb, out, cap, ob, nullptr, g, nullptr);
    }, slot);
}

/* the byte and row sizes the slot's last call needed, whether it succeeded or failed for capacity (bytes -1: the rows did not fit) */
int dvbs2gpu_t2mi_get_needed(dvbs2gpu_t2mi* b, int stream, int slot, int* bytes, int* rows) {
    if (!t2_slot_ok(b, stream, slot) || !bytes || !rows) return DVBS2GPU_ERR_ARG;
    *bytes = b->need_bytes[stream * T2MI_SLOTS + slot]; *rows = b->need_rows[stream * T2MI_SLOTS + slot];
    return 0;
}

int dvbs2gpu_t2mi_get_stats(dvbs2gpu_t2mi* b, int stream, int slot, dvbs2gpu_t2mi_stats* h_out) {
    if (!b || stream < 0 || stream >= b->nstreams || slot < -1 || slot >= T2MI_SLOTS || !h_out) return DVBS2GPU_ERR_ARG;
    *h_out = dvbs2gpu_t2mi_stats{};
    int64_t* d = reinterpret_cast<int64_t*>(h_out);
    for (int s = slot < 0 ? 0 : slot; s < (slot < 0 ? T2MI_SLOTS : slot + 1); ++s) {
        const int64_t* a = reinterpret_cast<const int64_t*>(&b->stats[(size_t)stream * T2MI_SLOTS + s]);
        for (int k = 0; k < T2MI_NCNT; ++k) d[k] += a[k];
    }
    return 0;
}

int dvbs2gpu_t2mi_get_row_table(dvbs2gpu_t2mi* b, int stream, int slot, dvbs2gpu_t2mi_row* h_rows, int cap, int* n) {
    return ts_bank_rows<T2MI_SLOTS>(b, &dvbs2gpu_t2mi::max_rows, stream, h_rows, cap, n, slot);
}

int dvbs2gpu_t2mi_get_row_table_device(dvbs2gpu_t2mi* b, int stream, int slot, const dvbs2gpu_t2mi_row** d_rows, int* n) {
    return ts_bank_rows_device<T2MI_SLOTS>(b, &dvbs2gpu_t2mi::max_rows, stream, d_rows, n, slot);
}

int dvbs2gpu_t2mi_get_frame_bytes(dvbs2gpu_t2mi* b, int stream, int slot, int* h_sizes, int cap, int* n) {
    if (!t2_slot_ok(b, stream, slot) || !n || cap < 0 || (cap > 0 && !h_sizes)) return DVBS2GPU_ERR_ARG;
    const int g = stream * T2MI_SLOTS + slot;
    const int k = (*n = b->ndelivered[g]) < cap ? *n : cap;
    if (k <= 0) return 0;
    if (!b->ctx) {
        int i = 0;
        for (const T2miRow& r : b->host[g].rows)
            if (r.offset >= 0 && i < k) h_sizes[i++] = r.bbframe_bytes;
        return 0;
    }
    HIP_TRY(hipSetDevice(b->ctx->device));
    HIP_TRY(hipMemcpy(h_sizes, b->d_fb + (size_t)g * b->max_rows, k * sizeof(int), hipMemcpyDeviceToHost));
    return 0;
}

}  // extern "C"
