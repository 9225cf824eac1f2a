// PSI section bank (own extension; include/dvbs2gpu.h): PAT / PMT / SI section reassembly with CRC-32 on up to 16
// watched PIDs of each of `nstreams` transport streams in HBM.  Every rule is in psi_rules.h, whose PsiHostStream is the sequential
// definition, the host bank and the kernels' yardstick.  How a call's packets are cut into independent pieces -- why that is possible,
// the packet list, the section walkers and the row numbering -- is ts_reasm.h with the format PsiFmt below (the datagram banks, dgram_bank.h,
// are its other users); this file holds what is the bank's own.
//
//   psi_scan_kernel    one workgroup per stream.
//     A-C  ts_reasm.h: the packets of the 16 watched PIDs into LDS, one lane per slot for the continuity walk, one lane per PUSI packet
//        and per carried-in section for the sections, one record (first packet, offset, last packet, bytes) per row.
//     D  one wave per row gathers the section's pieces into LDS, each lane takes the CRC of 64 bytes from a zero register
//        (crc32m_byte), the lanes' registers are shifted to the section's end (crc32m_mulmod, crc32m_xpow) and summed; the row's
//        fields come from the gathered bytes.
//     E  one lane per slot walks the slot's rows in order for CHANGED (the one sequential dependency between sections); a prefix sum
//        over the rows gives the output offsets; the changed PAT / PMT sections are gathered once more into the view staging.
//   psi_commit_kernel  (once the host has seen that every stream's bytes and rows fit) one workgroup per stream: a wave per delivered
//     row gathers the section and stores it at its offset, a dword per lane where the destination allows; then the open section
//     goes to the slot's 4 KiB buffer and the slots' new states are stored.
// Two launches per call, one device-to-host copy of the per-stream call record (PsiCall), and one small copy per changed PAT / PMT.
#include "ts_reasm.h"
#include "psi_rules.h"

#include <memory>

using namespace s2;
#define g_err last_error()

namespace s2 {

constexpr int PSI_MAX_PACKETS = 4096;            // per stream and call: 10 bytes of LDS per packet (scan; 6 in commit) beside 17 KiB of gathered sections
constexpr int PSI_WG = 256, PSI_WAVES = PSI_WG / 64;
constexpr int PSI_SEC_LDS = PSI_BUF + PSI_BUF / 64 * 4;    // a gathered section, 4 bytes of padding behind every 64: lane L's chunk starts in bank 17 L
static_assert(sizeof(PsiRow) == sizeof(dvbs2gpu_psi_section) && sizeof(PsiRow) == 24, "row layout");
static_assert(sizeof(PsiLayout) == sizeof(dvbs2gpu_psi_layout), "layout layout");
static_assert(PSI_MAX_PACKETS <= 32 * PSI_WG, "reasm_collect keeps a thread's match flags in one 32-bit mask (ts_thread_run)");
static_assert(sizeof(PsiProgram) == sizeof(dvbs2gpu_psi_program) && sizeof(PsiEs) == sizeof(dvbs2gpu_psi_es), "view rows");
static_assert(sizeof(PsiPatHeader) == sizeof(dvbs2gpu_psi_pat) && sizeof(PsiPmtHeader) == sizeof(dvbs2gpu_psi_pmt), "view headers");

enum { C_PACKETS = 0, C_SECTIONS, C_VALID, C_CHANGED, C_CRC, C_DROPPED, C_MALSEC, C_MALPKT, C_SCR, C_UNEXP, C_BYTES };
static_assert(sizeof(PsiCnt) == PSI_NCNT * sizeof(int32_t) && C_BYTES == PSI_NCNT - 1, "counter order");

struct PsiDevSlot { uint32_t last4; uint16_t fill; uint8_t cont, has_last; };
// the section format of ts_reasm.h: 16 slots per workgroup, a 3-byte header with the length in bytes 1 and 2, stuffing 0xFF; a bad
// length and a long-syntax section too short for its header and CRC are malformed sections
struct PsiFmt {
    typedef PsiDevSlot State;
    static constexpr int WG = PSI_WG, SLOTS = PSI_SLOTS, BUF = PSI_BUF, HEADER = PSI.header_bytes, LEN_A = 1, LEN_B = 2, STUFFING = 0xFF;
    static constexpr int NCNT = PSI_NCNT, C_DROPPED = s2::C_DROPPED, C_BAD_UNIT = C_MALSEC, C_SLACK = -1;
    __device__ static int total(unsigned b1, unsigned b2) { const int n = psi_section_length(b1, b2); return n > PSI.max_section_length ? -1 : PSI.header_bytes + n; }
    __device__ static bool is_row(unsigned b1, int total) { return !((b1 >> 7) && total < PSI.min_long_section); }
};
typedef ReasmRec PsiRec;
typedef ReasmView<PsiFmt> PsiView;
struct PsiCall { int32_t needed, nrows, watched, pad; uint16_t view_len[PSI_SLOTS]; PsiCnt cnt[PSI_SLOTS]; };

__device__ inline int psi_sx(int i) { return i + (i >> 6) * 4; }

__device__ inline int psi_match(const TsmonHdr& h, const PsiWatch* w) {
    if (h.cls != TSMON_DATA) return -1;
    for (int s = 0; s < PSI_SLOTS; ++s) if (w[s].pid == h.pid) return s;
    return -1;
}

// the pieces of section r, in order, into dst (indexed through psi_sx): all 64 lanes of a wave
__device__ inline void psi_copy_in(uint8_t* dst, int pos, const uint8_t* src, int len, int lane) {
    for (int i = lane; i < len; i += 64) dst[psi_sx(pos + i)] = src[i];
}
__device__ void psi_gather(uint8_t* dst, const PsiRec& r, const PsiView& v, int lane) {
    reasm_pieces(r, v, PSI_BUF, [&](int pos, const uint8_t* src, int len) { psi_copy_in(dst, pos, src, len, lane); });
}
// a gathered section as the source of ts_wave_copy
struct PsiLdsBytes {
    const uint8_t* sb;
    __device__ unsigned u8(int i) const { return sb[psi_sx(i)]; }
    __device__ unsigned u32(int i) const { return u8(i) | u8(i + 1) << 8 | u8(i + 2) << 16 | u8(i + 3) << 24; }
};

// dynamic LDS: wa[max_packets] (dwords), rc[max_packets] (dwords), wb[max_packets] (16 bits each)
__global__ void __launch_bounds__(PSI_WG) psi_scan_kernel(const uint8_t* const* __restrict__ in, const int* __restrict__ nbytes, int max_packets,
                                                          int max_sections, const PsiWatch* __restrict__ watch, const int* __restrict__ deliver,
                                                          const PsiDevSlot* __restrict__ state, PsiDevSlot* __restrict__ newst,
                                                          const uint8_t* __restrict__ bufs, uint8_t* __restrict__ views, unsigned* __restrict__ wa_g,
                                                          uint16_t* __restrict__ wb_g, PsiRec* __restrict__ recs, PsiRec* __restrict__ opens,
                                                          PsiRow* __restrict__ rows_g, PsiCall* __restrict__ call, int have_out) {
    extern __shared__ __attribute__((aligned(16))) unsigned psi_lds[];
    __shared__ __attribute__((aligned(16))) uint8_t sec[PSI_WAVES][PSI_SEC_LDS];
    __shared__ int cnt[PSI_SLOTS][PSI_NCNT], wsum[PSI_WAVES], view_row[PSI_SLOTS];
    __shared__ PsiWatch w[PSI_SLOTS];
    __shared__ PsiDevSlot ss[PSI_SLOTS], nss[PSI_SLOTS];
    unsigned* wa = psi_lds;
    int* rc = reinterpret_cast<int*>(psi_lds + max_packets);
    uint16_t* wb = reinterpret_cast<uint16_t*>(psi_lds + 2 * (size_t)max_packets);
    const int s = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int n = nbytes[s] / TSMON_TS;
    if (n > max_packets) n = max_packets;            // (the host has refused such a call)
    if (tid < PSI_SLOTS) {
        w[tid] = watch[(size_t)s * PSI_SLOTS + tid];
        ss[tid] = state[(size_t)s * PSI_SLOTS + tid];
        nss[tid] = ss[tid];
        view_row[tid] = -1;
        for (int c = 0; c < PSI_NCNT; ++c) cnt[tid][c] = 0;
        const PsiRec none = {-2, 0, 0, (uint16_t)tid, 0};
        opens[(size_t)s * PSI_SLOTS + tid] = none;
    }
    __syncthreads();
    const uint8_t* ts = in[s];
    const int W = n > 0 ? reasm_collect<PSI_WG>(ts, n, [&](const TsmonHdr& h) { return psi_match(h, w); }, wa, wb, wsum) : 0;
    // B: the continuity walk, one lane per slot
    if (tid < PSI_SLOTS && w[tid].pid >= 0) {
        uint8_t st = ss[tid].cont;
        const ReasmWalk c = reasm_classify<PsiFmt>(wa, wb, W, tid, &st);
        nss[tid].cont = st;
        nss[tid].fill = 0;
        cnt[tid][C_PACKETS] = c.packets; cnt[tid][C_SCR] = c.scrambled; cnt[tid][C_MALPKT] = c.malformed;
    }
    for (int j = tid; j < W; j += PSI_WG) rc[j] = 0;
    __syncthreads();
    // C: sections
    const PsiView v = {ts, wa, wb, W, bufs + (size_t)s * PSI_SLOTS * PSI_BUF, ss};
    PsiRec* rec = recs + (size_t)s * max_sections;
    const ReasmOut<PsiFmt> o = {rc, rec, opens + (size_t)s * PSI_SLOTS, nss, cnt, max_sections};
    reasm_jobs<false>(v, o);
    __syncthreads();
    const int nrows = reasm_number_rows<PSI_WG>(rc, W, wsum);
    const bool fits = nrows <= max_sections;
    PsiRow* rows = rows_g + (size_t)s * max_sections;
    int needed = fits ? 0 : -1;
    if (fits) {
        reasm_jobs<true>(v, o);
        __syncthreads();
        // D: a wave per row
        for (int r0 = 0; r0 < nrows; r0 += PSI_WAVES) {
            const int r = r0 + wave;
            PsiRec q = {0, 0, 0, 0, 0};
            if (r < nrows) { q = rec[r]; psi_gather(sec[wave], q, v, lane); }
            __syncthreads();
            if (r < nrows) {
                const uint8_t* sb = sec[wave];
                const int total = q.total < PSI_BUF ? q.total : PSI_BUF, start = 64 * lane;
                const int len = total - start < 0 ? 0 : (total - start < 64 ? total - start : 64);
                uint32_t c = 0;
                for (int i = 0; i < len; i += 4) {
                    const unsigned d = *reinterpret_cast<const unsigned*>(sb + 68 * lane + i);
                    for (int b = 0; b < 4; ++b) if (i + b < len) c = crc32m_byte(c, d >> (8 * b) & 255);
                }
                uint32_t x = len > 0 ? crc32m_mulmod(c, crc32m_xpow((uint32_t)(total - start - len))) : 0;
                if (lane == 0) x ^= crc32m_mulmod(0xFFFFFFFFu, crc32m_xpow((uint32_t)total));
                for (int k = 32; k > 0; k >>= 1) x ^= __shfl_xor(x, k);
                if (lane == 0) {
                    auto rd = [&](int i) { return (unsigned)sb[psi_sx(i)]; };
                    const bool valid = !(rd(1) >> 7) || x == 0;
                    PsiRow row = psi_row_fields(rd, total, w[q.slot].pid, valid, q.j0 < 0 ? -1 : wa_k(wa[q.j0]));
                    uint32_t l4 = 0;
                    for (int i = total < 4 ? 0 : total - 4; i < total; ++i) l4 = l4 << 8 | rd(i);
                    row.offset = (int32_t)l4;                   // until phase E has used it
                    rows[r] = row;
                }
            }
            __syncthreads();
        }
        // E: CHANGED, one lane per slot over its rows in order
        if (tid < PSI_SLOTS && w[tid].pid >= 0) {
            uint32_t last = ss[tid].last4;
            int has = ss[tid].has_last, c_sec = 0, c_valid = 0, c_chg = 0, c_crc = 0, c_unexp = 0;
            for (int r = 0; r < nrows; ++r) {
                if (rec[r].slot != tid) continue;
                PsiRow row = rows[r];
                ++c_sec;
                c_unexp += w[tid].expect >= 0 && row.table_id != w[tid].expect;
                if (row.flags & PSI_CRC_ERROR) ++c_crc;
                else {
                    ++c_valid;
                    if (!has || (uint32_t)row.offset != last) { row.flags |= PSI_CHANGED; ++c_chg; rows[r].flags = row.flags; }
                    has = 1; last = (uint32_t)row.offset;
                    if (psi_is_view(row)) view_row[tid] = r;
                }
            }
            nss[tid].last4 = last; nss[tid].has_last = (uint8_t)has;
            cnt[tid][C_SECTIONS] = c_sec; cnt[tid][C_VALID] = c_valid; cnt[tid][C_CHANGED] = c_chg; cnt[tid][C_CRC] = c_crc; cnt[tid][C_UNEXP] = c_unexp;
        }
        __syncthreads();
        {   // the output offsets: an exact prefix sum in row order
            const int mode = deliver[s];
            int r0, r1; ts_thread_run(nrows, PSI_WG, &r0, &r1);
            auto bytes_of = [&](int r) { return have_out && (mode == 0 || (rows[r].flags & PSI_CHANGED)) ? rows[r].length : 0; };
            int mine = 0;
            for (int r = r0; r < r1; ++r) mine += bytes_of(r);
            int at = ts_block_scan<PSI_WG>(mine, wsum, &needed);
            for (int r = r0; r < r1; ++r) {
                const int b = bytes_of(r);
                rows[r].offset = b ? at : -1;
                if (b) atomicAdd(&cnt[rec[r].slot][C_BYTES], b);
                at += b;
            }
        }
        // the changed PAT / PMT sections, once more, for the host's decoded views
        for (int s0 = 0; s0 < PSI_SLOTS; s0 += PSI_WAVES) {
            const int sl = s0 + wave, r = view_row[sl];
            PsiRec q = {0, 0, 0, 0, 0};
            if (r >= 0) { q = rec[r]; psi_gather(sec[wave], q, v, lane); }
            __syncthreads();
            if (r >= 0) {
                uint8_t* dst = views + ((size_t)s * PSI_SLOTS + sl) * PSI_BUF;
                for (int i = lane; i < q.total && i < PSI_BUF; i += 64) dst[i] = sec[wave][psi_sx(i)];
            }
            __syncthreads();
        }
    }
    for (int j = tid; j < W; j += PSI_WG) { wa_g[(size_t)s * max_packets + j] = wa[j]; wb_g[(size_t)s * max_packets + j] = wb[j]; }
    if (tid < PSI_SLOTS) {
        newst[(size_t)s * PSI_SLOTS + tid] = nss[tid];
        PsiCall* c = call + s;
        if (tid == 0) { c->needed = needed; c->nrows = nrows; c->watched = W; c->pad = 0; }
        c->view_len[tid] = (uint16_t)(fits && view_row[tid] >= 0 ? rec[view_row[tid]].total : 0);
        int32_t* dst = reinterpret_cast<int32_t*>(&c->cnt[tid]);
        for (int k = 0; k < PSI_NCNT; ++k) dst[k] = cnt[tid][k];
    }
}

// dynamic LDS: wa[max_packets] (dwords), wb[max_packets] (16 bits each)
__global__ void __launch_bounds__(PSI_WG) psi_commit_kernel(const uint8_t* const* __restrict__ in, uint8_t* const* __restrict__ out, int max_packets,
                                                            int max_sections, int cap, PsiDevSlot* __restrict__ state,
                                                            const PsiDevSlot* __restrict__ newst, uint8_t* __restrict__ bufs,
                                                            const unsigned* __restrict__ wa_g, const uint16_t* __restrict__ wb_g,
                                                            const PsiRec* __restrict__ recs, const PsiRec* __restrict__ opens,
                                                            const PsiRow* __restrict__ rows_g, const PsiCall* __restrict__ call) {
    extern __shared__ __attribute__((aligned(16))) unsigned psi_lds[];
    __shared__ __attribute__((aligned(16))) uint8_t sec[PSI_WAVES][PSI_SEC_LDS];
    __shared__ PsiDevSlot ss[PSI_SLOTS];
    unsigned* wa = psi_lds;
    uint16_t* wb = reinterpret_cast<uint16_t*>(psi_lds + max_packets);
    const int s = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int W = call[s].watched, nrows = call[s].nrows;
    if (W > max_packets) W = max_packets;
    if (nrows > max_sections) nrows = max_sections;
    for (int j = tid; j < W; j += PSI_WG) { wa[j] = wa_g[(size_t)s * max_packets + j]; wb[j] = wb_g[(size_t)s * max_packets + j]; }
    if (tid < PSI_SLOTS) ss[tid] = state[(size_t)s * PSI_SLOTS + tid];
    __syncthreads();
    uint8_t* sbuf = bufs + (size_t)s * PSI_SLOTS * PSI_BUF;
    const PsiView v = {in[s], wa, wb, W, sbuf, ss};
    const PsiRec* rec = recs + (size_t)s * max_sections;
    const PsiRow* rows = rows_g + (size_t)s * max_sections;
    uint8_t* o = out ? out[s] : nullptr;
    for (int r0 = 0; o && r0 < nrows; r0 += PSI_WAVES) {
        const int r = r0 + wave;
        int off = -1, total = 0;
        if (r < nrows) { off = rows[r].offset; total = rows[r].length < PSI_BUF ? rows[r].length : PSI_BUF; }
        if (off < 0 || off + total > cap) off = -1;
        if (off >= 0) psi_gather(sec[wave], rec[r], v, lane);
        __syncthreads();
        if (off >= 0) ts_wave_copy(o + off, PsiLdsBytes{sec[wave]}, total, lane);
        __syncthreads();
    }
    // the open sections into the slots' buffers (what they read of the buffers is in LDS before the barrier), then the states
    for (int s0 = 0; s0 < PSI_SLOTS; s0 += PSI_WAVES) {
        const int sl = s0 + wave;
        const PsiRec q = opens[(size_t)s * PSI_SLOTS + sl];
        if (q.j0 > -2) psi_gather(sec[wave], q, v, lane);
        __syncthreads();
        if (q.j0 > -2) for (int i = lane; i < q.total && i < PSI_BUF; i += 64) sbuf[(size_t)sl * PSI_BUF + i] = sec[wave][psi_sx(i)];
        __syncthreads();
    }
    if (tid < PSI_SLOTS) state[(size_t)s * PSI_SLOTS + tid] = newst[(size_t)s * PSI_SLOTS + tid];
}

}  // namespace s2

struct dvbs2gpu_psi {
    dvbs2gpu_ctx* ctx = nullptr;                   // null: a host-only bank (dvbs2gpu_psi_create_host)
    int nstreams = 0, max_packets = 0, max_sections = 0;
    std::vector<PsiWatch> watch;                   // nstreams x 16
    std::vector<int> deliver;
    std::vector<dvbs2gpu_psi_stats> stats;         // nstreams x 16, since reset; the kernels report each call's share (PsiCall)
    std::vector<int> nrows, need_bytes, need_rows; // of the last call per stream
    std::vector<std::vector<uint8_t>> view;        // nstreams x 16: the decoded views' sections (device banks)
    std::vector<PsiCall> h_call;
    std::vector<char> h_args;
    // device banks
    DevBuf<PsiWatch> d_watch;
    DevBuf<int> d_deliver;
    DevBuf<PsiDevSlot> d_state, d_newst;
    DevBuf<uint8_t> d_bufs, d_views;               // nstreams x 16 x 4096 each
    DevBuf<unsigned> d_wa;                         // nstreams x max_packets: the watched packets of the last call
    DevBuf<uint16_t> d_wb;
    DevBuf<PsiRec> d_recs, d_opens;
    DevBuf<PsiRow> d_rows;                         // nstreams x max_sections
    DevBuf<PsiCall> d_call;
    DevBuf<uint8_t> d_args;                        // TsBankArgs(nstreams)
    TsHostStage stage;                             // of the host-buffer entry point
    // host-only banks
    std::vector<PsiHostStream> host;
};

namespace s2 {
static void psi_account(dvbs2gpu_psi* b, int i, const PsiCnt* c) {
    for (int s = 0; s < PSI_SLOTS; ++s) {
        int64_t* d = reinterpret_cast<int64_t*>(&b->stats[(size_t)i * PSI_SLOTS + s]);
        const int32_t* a = reinterpret_cast<const int32_t*>(&c[s]);
        for (int k = 0; k < PSI_NCNT; ++k) d[k] += a[k];
    }
}
static_assert(sizeof(dvbs2gpu_psi_stats) == PSI_NCNT * sizeof(int64_t), "stats order");
static bool psi_create_args_ok(int nstreams, int max_packets, int max_sections, dvbs2gpu_psi** out) {
    if (!out || nstreams <= 0 || max_packets <= 0 || max_sections <= 0) return false;
    if (max_packets > PSI_MAX_PACKETS) { g_err = "PSI bank: max_packets is at most 4096 per stream and call"; return false; }
    return true;
}
static std::unique_ptr<dvbs2gpu_psi> psi_new(dvbs2gpu_ctx* ctx, int nstreams, int max_packets, int max_sections) {
    std::unique_ptr<dvbs2gpu_psi> b(new dvbs2gpu_psi());
    b->ctx = ctx; b->nstreams = nstreams; b->max_packets = max_packets; b->max_sections = max_sections;
    b->watch.assign((size_t)nstreams * PSI_SLOTS, PsiWatch{-1, -1});
    for (int i = 0; i < nstreams; ++i) b->watch[(size_t)i * PSI_SLOTS] = {0, 0};
    b->deliver.assign(nstreams, 0);
    b->stats.assign((size_t)nstreams * PSI_SLOTS, dvbs2gpu_psi_stats{});
    b->nrows.assign(nstreams, 0); b->need_bytes.assign(nstreams, 0); b->need_rows.assign(nstreams, 0);
    b->h_call.resize(nstreams);
    return b;
}
static const std::vector<uint8_t>& psi_view_of(dvbs2gpu_psi* b, int stream, int slot) {
    return b->ctx ? b->view[(size_t)stream * PSI_SLOTS + slot] : b->host[stream].view[slot];
}
}  // namespace s2

extern "C" {

void dvbs2gpu_psi_destroy(dvbs2gpu_psi* b) { delete b; }

int dvbs2gpu_psi_create(dvbs2gpu_ctx* ctx, int nstreams, int max_packets, int max_sections, dvbs2gpu_psi** out) {
    if (!ctx || !psi_create_args_ok(nstreams, max_packets, max_sections, out)) return DVBS2GPU_ERR_ARG;
    HIP_TRY(hipSetDevice(ctx->device));
    auto b = psi_new(ctx, nstreams, max_packets, max_sections);
    b->view.resize((size_t)nstreams * PSI_SLOTS);
    const size_t n = (size_t)nstreams, ns = n * PSI_SLOTS;
    const char* what = "hipMalloc(psi)";               // (zero-filled: the delivery modes and the slots' states; the kernels write the rest before it is read)
    RC_TRY(b->d_watch.alloc(ns, false, what));
    HIP_TRY(hipMemcpy(b->d_watch, b->watch.data(), ns * sizeof(PsiWatch), hipMemcpyHostToDevice));
    RC_TRY(b->d_deliver.alloc(n, true, what));
    RC_TRY(b->d_state.alloc(ns, true, what));
    RC_TRY(b->d_newst.alloc(ns, false, what));
    RC_TRY(b->d_bufs.alloc(ns * PSI_BUF, false, what));
    RC_TRY(b->d_views.alloc(ns * PSI_BUF, false, what));
    RC_TRY(b->d_wa.alloc(n * max_packets, false, what));
    RC_TRY(b->d_wb.alloc(n * max_packets, false, what));
    RC_TRY(b->d_recs.alloc(n * max_sections, false, what));
    RC_TRY(b->d_opens.alloc(ns, false, what));
    RC_TRY(b->d_rows.alloc(n * max_sections, false, what));
    RC_TRY(b->d_call.alloc(n, false, what));
    RC_TRY(b->d_args.alloc(TsBankArgs(n).L.bytes(), false, what));
    b->h_args.resize(TsBankArgs(n).L.bytes());
    *out = b.release();
    return 0;
}

int dvbs2gpu_psi_create_host(int nstreams, int max_packets, int max_sections, dvbs2gpu_psi** out) {
    if (!psi_create_args_ok(nstreams, max_packets, max_sections, out)) return DVBS2GPU_ERR_ARG;
    auto b = psi_new(nullptr, nstreams, max_packets, max_sections);
    b->host.resize(nstreams);
    *out = b.release();
    return 0;
}

int dvbs2gpu_psi_reset(dvbs2gpu_psi* b) {
    if (!b) return DVBS2GPU_ERR_ARG;
    if (b->ctx) {
        HIP_TRY(hipSetDevice(b->ctx->device));
        HIP_TRY(hipMemset(b->d_state, 0, (size_t)b->nstreams * PSI_SLOTS * sizeof(PsiDevSlot)));
    }
    for (auto& h : b->host) { for (int s = 0; s < PSI_SLOTS; ++s) h.clear_slot(s); h.rows.clear(); h.bytes.clear(); }
    for (auto& v : b->view) v.clear();
    std::fill(b->stats.begin(), b->stats.end(), dvbs2gpu_psi_stats{});
    std::fill(b->nrows.begin(), b->nrows.end(), 0);
    return 0;
}

int dvbs2gpu_psi_get_layout(dvbs2gpu_psi_layout* h_out) {
    if (!h_out) return DVBS2GPU_ERR_ARG;
    memcpy(h_out, &PSI, sizeof(PSI));
    return 0;
}

int dvbs2gpu_psi_set_watch(dvbs2gpu_psi* b, int stream, int slot, int pid, int expect_table_id) {
    if (!b || stream < 0 || stream >= b->nstreams || slot < 0 || slot >= PSI_SLOTS) return DVBS2GPU_ERR_ARG;
    if (pid < -1 || pid >= TSMON_NULL_PID || expect_table_id < -1 || expect_table_id > 255) {
        g_err = "PSI bank: a watched PID is 0..0x1FFE (-1 clears the slot), an expected table_id 0..255 or -1";
        return DVBS2GPU_ERR_ARG;
    }
    PsiWatch* w = b->watch.data() + (size_t)stream * PSI_SLOTS;
    for (int s = 0; s < PSI_SLOTS; ++s)
        if (pid >= 0 && s != slot && w[s].pid == pid) { g_err = "PSI bank: the PID is watched in another slot of the stream"; return DVBS2GPU_ERR_ARG; }
    const size_t at = (size_t)stream * PSI_SLOTS + slot;
    w[slot] = {pid, pid < 0 ? -1 : expect_table_id};
    b->stats[at] = dvbs2gpu_psi_stats{};
    if (b->ctx) {
        HIP_TRY(hipSetDevice(b->ctx->device));
        HIP_TRY(hipMemcpy(b->d_watch + at, &w[slot], sizeof(PsiWatch), hipMemcpyHostToDevice));
        HIP_TRY(hipMemset(b->d_state + at, 0, sizeof(PsiDevSlot)));
        b->view[at].clear();
    } else {
        b->host[stream].watch[slot] = w[slot];
        b->host[stream].clear_slot(slot);
    }
    return 0;
}

int dvbs2gpu_psi_set_deliver(dvbs2gpu_psi* b, int stream, int mode) {
    if (!b || stream < 0 || stream >= b->nstreams) return DVBS2GPU_ERR_ARG;
    if (mode < 0 || mode > 1) { g_err = "PSI bank: deliver mode is 0 (every section) or 1 (valid changed sections)"; return DVBS2GPU_ERR_ARG; }
    b->deliver[stream] = mode;
    if (b->ctx) {
        HIP_TRY(hipSetDevice(b->ctx->device));
        HIP_TRY(hipMemcpy(b->d_deliver + stream, &mode, sizeof(int), hipMemcpyHostToDevice));
    } else b->host[stream].deliver = mode;
    return 0;
}

int dvbs2gpu_psi_process_batch(dvbs2gpu_psi* b, const uint8_t* const* d_ts, const int* nbytes, uint8_t* const* d_out, int cap, int* out_bytes,
                               int* out_rows, void* stream) {
    if (!b || !d_ts || !nbytes || cap < 0 || (d_out && !out_bytes)) return DVBS2GPU_ERR_ARG;
    if (!b->ctx) { g_err = "PSI bank: a host bank takes host buffers (dvbs2gpu_psi_work)"; return DVBS2GPU_ERR_ARG; }
    const int n = b->nstreams;
    for (int i = 0; i < n; ++i) {
        if (!ts_bank_check_counts("PSI bank: ", nbytes + i, 1, b->max_packets)) return DVBS2GPU_ERR_ARG;
        // once d_out is given every stream needs its output pointer, an empty one too (the TS monitor asks only streams that bring packets)
        if ((nbytes[i] > 0 && !d_ts[i]) || (d_out && (!d_out[i] || d_out[i] == d_ts[i]))) {
            g_err = "PSI bank: null buffer, or an output buffer that is its stream's input";
            return DVBS2GPU_ERR_ARG;
        }
    }
    HIP_TRY(hipSetDevice(b->ctx->device));
    hipStream_t st = (hipStream_t)stream;
    const TsBankArgs a(n);
    a.fill(b->h_args.data(), n, d_ts, d_out, nbytes);
    HIP_TRY(hipMemcpyAsync(b->d_args, b->h_args.data(), b->h_args.size(), hipMemcpyHostToDevice, st));
    const size_t lds_scan = (size_t)b->max_packets * 10 + 16, lds_commit = (size_t)b->max_packets * 6 + 16;   // <= 40 KiB beside 18 KiB static
    hipLaunchKernelGGL(psi_scan_kernel, dim3(n), dim3(PSI_WG), lds_scan, st, a.in(b->d_args), a.nbytes(b->d_args), b->max_packets, b->max_sections, b->d_watch, b->d_deliver,
                       b->d_state, b->d_newst, b->d_bufs, b->d_views, b->d_wa, b->d_wb, b->d_recs, b->d_opens, b->d_rows, b->d_call, d_out ? 1 : 0);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(b->h_call.data(), b->d_call, sizeof(PsiCall) * n, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    bool fits = true;
    for (int i = 0; i < n; ++i) {
        const PsiCall& c = b->h_call[i];
        fits &= c.nrows <= b->max_sections && (!d_out || c.needed <= cap);
        b->need_bytes[i] = c.needed; b->need_rows[i] = c.nrows;
        if (out_bytes) out_bytes[i] = c.needed;
        if (out_rows) out_rows[i] = c.nrows;
    }
    if (!fits) {                                       // nothing has been stored: the same call may come again with more room
        std::fill(b->nrows.begin(), b->nrows.end(), 0);
        g_err = "PSI bank: the sections of a stream do not fit cap, or its rows max_sections (out_bytes / out_rows hold the sizes)";
        return DVBS2GPU_ERR_CAPACITY;
    }
    hipLaunchKernelGGL(psi_commit_kernel, dim3(n), dim3(PSI_WG), lds_commit, st, a.in(b->d_args), d_out ? a.out(b->d_args) : nullptr, b->max_packets, b->max_sections, cap,
                       b->d_state, b->d_newst, b->d_bufs, b->d_wa, b->d_wb, b->d_recs, b->d_opens, b->d_rows, b->d_call);
    HIP_TRY(hipGetLastError());
    for (int i = 0; i < n; ++i)                        // the changed PAT / PMT sections, and only those
        for (int s = 0; s < PSI_SLOTS; ++s) {
            const int len = b->h_call[i].view_len[s];
            if (!len) continue;
            std::vector<uint8_t>& v = b->view[(size_t)i * PSI_SLOTS + s];
            v.resize(len);
            HIP_TRY(hipMemcpyAsync(v.data(), b->d_views + ((size_t)i * PSI_SLOTS + s) * PSI_BUF, len, hipMemcpyDeviceToHost, st));
        }
    HIP_TRY(hipStreamSynchronize(st));
    for (int i = 0; i < n; ++i) { psi_account(b, i, b->h_call[i].cnt); b->nrows[i] = b->h_call[i].nrows; }
    return 0;
}

int dvbs2gpu_psi_work(dvbs2gpu_psi* b, int stream, const uint8_t* h_ts, int nbytes, uint8_t* h_out, int cap) {
    if (!b || stream < 0 || stream >= b->nstreams || nbytes < 0 || cap < 0 || (nbytes > 0 && !h_ts)) return DVBS2GPU_ERR_ARG;
    if (!ts_bank_check_counts("PSI bank: ", &nbytes, 1, b->max_packets)) return DVBS2GPU_ERR_ARG;
    if (h_out && h_out == h_ts) { g_err = "PSI bank: the output buffer is the input"; return DVBS2GPU_ERR_ARG; }
    if (!b->ctx) {
        PsiHostStream& h = b->host[stream];
        std::fill(b->nrows.begin(), b->nrows.end(), 0);    // the table is of the LAST call, which brought the others nothing
        std::vector<std::pair<int, PsiSlot>> before;       // what a capacity failure has to put back: the watched slots and their views
        std::vector<uint8_t> views[PSI_SLOTS];
        for (int s = 0; s < PSI_SLOTS; ++s)
            if (h.watch[s].pid >= 0) { before.emplace_back(s, h.slot[s]); views[s] = h.view[s]; }
        h.run(h_ts, nbytes / TSMON_TS, h_out != nullptr);
        const bool rows_fit = (int)h.rows.size() <= b->max_sections;
        b->need_rows[stream] = (int)h.rows.size();
        b->need_bytes[stream] = rows_fit ? (int)h.bytes.size() : -1;
        if (!rows_fit || (h_out && (int)h.bytes.size() > cap)) {
            for (const auto& kv : before) { h.slot[kv.first] = kv.second; h.view[kv.first] = views[kv.first]; }
            h.rows.clear(); h.bytes.clear();
            g_err = "PSI bank: the sections do not fit cap, or the rows max_sections (dvbs2gpu_psi_get_needed holds the sizes)";
            return DVBS2GPU_ERR_CAPACITY;
        }
        psi_account(b, stream, h.cnt);
        b->nrows[stream] = (int)h.rows.size();
        if (h_out && !h.bytes.empty()) memcpy(h_out, h.bytes.data(), h.bytes.size());
        return (int)h.bytes.size();
    }
    HIP_TRY(hipSetDevice(b->ctx->device));
    return ts_bank_work(b->stage, b->nstreams, stream, h_ts, nbytes, b->max_packets, h_out, cap, true, [&](const uint8_t* const* in, const int* nb, uint8_t* const* out, int* ob) {
        return dvbs2gpu_psi_process_batch(b, in, nb, out, cap, ob, nullptr, nullptr);
    });
}

/* the byte and row sizes the stream's last call needed, whether it succeeded or failed for capacity (bytes -1: the rows did not fit) */
int dvbs2gpu_psi_get_needed(dvbs2gpu_psi* b, int stream, int* bytes, int* rows) {
    if (!b || stream < 0 || stream >= b->nstreams || !bytes || !rows) return DVBS2GPU_ERR_ARG;
    *bytes = b->need_bytes[stream]; *rows = b->need_rows[stream];
    return 0;
}

int dvbs2gpu_psi_get_stats(dvbs2gpu_psi* b, int stream, int slot, dvbs2gpu_psi_stats* h_out) {
    if (!b || stream < 0 || stream >= b->nstreams || slot < -1 || slot >= PSI_SLOTS || !h_out) return DVBS2GPU_ERR_ARG;
    *h_out = dvbs2gpu_psi_stats{};
    int64_t* d = reinterpret_cast<int64_t*>(h_out);
    for (int s = slot < 0 ? 0 : slot; s < (slot < 0 ? PSI_SLOTS : slot + 1); ++s) {
        const int64_t* a = reinterpret_cast<const int64_t*>(&b->stats[(size_t)stream * PSI_SLOTS + s]);
        for (int k = 0; k < PSI_NCNT; ++k) d[k] += a[k];
    }
    return 0;
}

int dvbs2gpu_psi_get_section_table(dvbs2gpu_psi* b, int stream, dvbs2gpu_psi_section* h_rows, int cap, int* n) {
    return ts_bank_rows(b, &dvbs2gpu_psi::max_sections, stream, h_rows, cap, n);
}

int dvbs2gpu_psi_get_section_table_device(dvbs2gpu_psi* b, int stream, const dvbs2gpu_psi_section** d_rows, int* n) {
    return ts_bank_rows_device(b, &dvbs2gpu_psi::max_sections, stream, d_rows, n);
}

int dvbs2gpu_psi_get_programs(dvbs2gpu_psi* b, int stream, dvbs2gpu_psi_pat* hdr, dvbs2gpu_psi_program* h_rows, int cap, int* n) {
    if (!b || stream < 0 || stream >= b->nstreams || !hdr || !n || cap < 0 || (cap > 0 && !h_rows)) return DVBS2GPU_ERR_ARG;
    *n = 0;
    *hdr = {-1, -1, 0};
    for (int s = 0; s < PSI_SLOTS; ++s) {
        const std::vector<uint8_t>& v = psi_view_of(b, stream, s);
        if (v.empty() || v[0] != 0) continue;
        std::vector<PsiProgram> out;
        const PsiPatHeader h = psi_parse_pat(v.data(), (int)v.size(), &out);
        memcpy(hdr, &h, sizeof(h));
        *n = (int)out.size();
        if (cap > 0 && !out.empty()) memcpy(h_rows, out.data(), (size_t)(*n < cap ? *n : cap) * sizeof(PsiProgram));
        break;
    }
    return 0;
}

int dvbs2gpu_psi_get_program_map(dvbs2gpu_psi* b, int stream, int slot, dvbs2gpu_psi_pmt* hdr, dvbs2gpu_psi_es* h_rows, int cap, int* n) {
    if (!b || stream < 0 || stream >= b->nstreams || slot < 0 || slot >= PSI_SLOTS || !hdr || !n || cap < 0 || (cap > 0 && !h_rows)) return DVBS2GPU_ERR_ARG;
    *n = 0;
    *hdr = {-1, -1, -1, 0};
    const std::vector<uint8_t>& v = psi_view_of(b, stream, slot);
    if (v.empty() || v[0] != 2) return 0;
    std::vector<PsiEs> out;
    const PsiPmtHeader h = psi_parse_pmt(v.data(), (int)v.size(), &out);
    memcpy(hdr, &h, sizeof(h));
    *n = (int)out.size();
    if (cap > 0 && !out.empty()) memcpy(h_rows, out.data(), (size_t)(*n < cap ? *n : cap) * sizeof(PsiEs));
    return 0;
}

}  // extern "C"
