// Mode-adaptation mode of the BBFRAME -> TS bank: ISI demultiplexing, ISSY / DNP slots, null-packet reinsertion
// and the per-packet CRC-8 for multiple-input-stream and ACM/VCM carriers, whose BBFRAMEs differ in size from frame to frame.
// Not part of the reference (its parser cuts every data field each 188 bytes of one stream); off unless asked for.
//
// A slot is [CRC-8 of the previous UP][187 UP bytes][ISSY 0/2/3][DNP 0/1] (MaLayout below: the one place that says so).  The first
// slot that starts in a frame starts SYNCD/8 bytes into the data field, so every frame is parsed on its own:
//   bbts_ma_frame_kernel  one wave per frame: header, lane (selected ISI) lookup, ISSY length, slot geometry; one lane per whole slot
//                         for its CRC-8 (four table look-ups per dword), DNP and ISCR; wave reductions -> one record per frame;
//   bbts_ma_lane_kernel   one wave per (stream, selected ISI): walks the stream's records in order, joins the tail of a frame with the
//                         head of the next one of its ISI (the spanning slot's CRC-8 by the wave, one byte per lane), sums the
//                         output offsets and writes the lane's new state to the shadow copy;
//   bbts_ma_emit_kernel   one workgroup per frame: DNP prefix sum, null packets, 0x47 + 187 bytes per slot in dwords, TEI.
// The host commits the shadow state and launches the third kernel only when every lane's output fits.
// MaHostStream below applies the same rules to host buffers, byte by byte (host-only banks; the GPU path's second implementation).
//
// DVB-T2 high-efficiency mode (dvbs2gpu_bbts_ma_set_t2_hem; rules in include/dvbs2gpu.h): a header whose CRC-8 carries the MODE value
// announces a slot of [187 UP bytes][DNP 0/1] (MaHemLayout below) with neither sync byte nor CRC-8 and the ISSY field in the header.
// The three kernels are the same; a HEM frame's wave (a wave is a frame, so the branch is uniform) skips the CRC and ISSY-length
// loops, a slot leaves with its own last byte, and the mode is one more bit of MaFrameRec::cfl / MaLaneState::cfl that a join compares.
//
// GSE in this mode (dvbs2gpu_bbts_ma_set_gse; rules in include/dvbs2gpu.h): one reassembly context per (stream, selected ISI) lane.
// Nothing of GSE is stated here: the packet header is gse_parse_packet<GseStrict> (bbts_rules.h), the device's chain walk and
// reassembly are gse_walk_frame and gse_apply_packet (bbts_gse_dev.h), the host's are GseHostCtx (bbts_host.h), and a context moves
// between the two with gse_ctx_to_host / gse_ctx_to_device (bbts_common.h).  This file says which frames, which lane, which order.
//   bbts_ma_frame_kernel      marks the GSE frames of selected ISIs in their records;
//   bbts_ma_gse_scan_kernel   one workgroup per (frame, stream): the data field staged in LDS, one lane follows the packet chain, a wave
//                             per fragment computes the CRC-32 of its span (bbts_gse_dev.h); 16 bytes per packet;
//   bbts_ma_lane_kernel<true> the lane pass above, which now also applies the packet records of its lane's GSE frames to the lane's
//                             three slots where the frame stands in the sequence: the GRE bytes enter the SAME running output offset
//                             as the TS packets, so both interleave in frame order and the call still synchronises twice;
//   bbts_ma_gse_move_kernel   behind the emit kernel: complete PDUs and PDUs that END in a frame, gathered into the lane's buffer;
//   bbts_ma_gse_append_kernel fragments of PDUs still open go to the lane's slot buffers (only read by move, only written here).
#include "bbts_common.h"
#include "bbts_gse_dev.h"

#include <climits>

#include <memory>

using namespace s2;
#define g_err last_error()

namespace s2 {

// ------------------------------------------------------------------------------------------------- the slot layout
struct MaLayout { int crc_off, up_off, up_len, issy_off; };      // the DNP byte follows the ISSY field and ends the slot
constexpr MaLayout kMa = {0, 1, 187, 188};
static_assert(kMa.up_len == 187 && kMa.up_off >= 1 && kMa.issy_off >= kMa.up_off + kMa.up_len, "a TS packet is 0x47 + 187 UP bytes");
constexpr int MA_TS = 188, MA_LANES = 8, MA_CARRY = 192, MA_NO_START = 65535, MA_MAX_FRAME = 58192 / 8;
__host__ __device__ inline int ma_slot_len(int issy, int npd) { return kMa.issy_off + issy + npd; }
// DVB-T2 high-efficiency mode: [187 UP bytes][DNP 0/1]; `mode` is XORed into the header's CRC-8 (0 would be normal mode)
struct MaHemLayout { int up_off, up_len, dnp_off, mode; };       // dnp_off: also the slot length without NPD
constexpr MaHemLayout kHem = {0, 187, 187, 1};
static_assert(kHem.up_len == kMa.up_len && kHem.dnp_off == kHem.up_off + kHem.up_len && kHem.mode > 0 && kHem.mode < 256, "0x47 + the same 187 UP bytes");
constexpr int MA_CFL_HEM = 8;                                    // the mode bit of cfl, above issy | npd << 2
__host__ __device__ inline int ma_hem_slot_len(int npd) { return kHem.dnp_off + npd; }
static_assert(kHem.dnp_off + 1 <= MA_CARRY, "a HEM slot fits the carry buffers");
__host__ __device__ inline int ma_crc_end(int span, int L) { return span ? L : kMa.up_off + kMa.up_len; }   // CRC-8 over [up_off, end)

struct MaHdr { int ts_gs, isi, issyi, npd, df, s0, nostart, upl, hem; };
// a frame of `size` bytes: CRC-8 of the BBHEADER, DFL whole bytes that fit the frame, SYNCD inside the data field or 65535 (no slot
// starts here).  The reference's `syncd >= dfl - 8` rejection is not applied: a slot may start in the last byte of a data field.
// hem_on: byte 9 = c ^ kHem.mode, c the CRC-8 of the nine bytes before it, announces a high-efficiency-mode frame (upl is then not a
// UPL).  The CRC is linear: over all ten bytes it leaves 0 for byte 9 = c and, for c ^ mode, what the byte `mode` alone leaves.
__host__ __device__ inline bool ma_header(const uint8_t* fr, int size, int hem_on, MaHdr* h) {
    if (size < 10) return false;
    h->hem = 0;
    if (const unsigned q = crc8_bits(fr, 80)) {
        const uint8_t mode = (uint8_t)kHem.mode;
        if (!hem_on || q != crc8_bits(&mode, 8)) return false;
        h->hem = 1;
    }
    const HeaderFields p = parse_bbheader(fr);
    const int dfl = p.v[8], syncd = p.v[10];
    if (dfl % 8 || dfl > (size - 10) * 8 || !(syncd == MA_NO_START || syncd < dfl)) return false;
    h->ts_gs = p.v[0]; h->isi = p.v[6]; h->issyi = p.v[3]; h->npd = p.v[4]; h->df = dfl / 8;
    h->nostart = syncd == MA_NO_START; h->upl = p.v[7];
    h->s0 = h->nostart ? h->df : syncd / 8;
    return true;
}
// what a frame says about the ISSY length: the first ISSY field that starts in it (0: nothing)
__host__ __device__ inline int ma_issy_cand(const uint8_t* fr, const MaHdr& h) {
    if (!h.issyi || h.nostart || h.s0 + kMa.issy_off >= h.df) return 0;
    const unsigned top = fr[10 + h.s0 + kMa.issy_off];
    return top < 0x80 ? 2 : top < 0xC0 ? 3 : 0;
}
__host__ __device__ inline bool ma_iscr(const uint8_t* f, int issy, unsigned* v) {
    if (issy < 2) return false;
    if (f[0] < 0x80) { *v = f[0] << 8 | f[1]; return true; }
    if (f[0] < 0xC0 && issy == 3) { *v = (f[0] & 0x3fu) << 16 | f[1] << 8 | f[2]; return true; }
    return false;
}

struct MaCfg { int issy_bytes, crc_span, reinsert_nulls, check_crc, gse, hem; };
struct MaSel { uint8_t isi[MA_LANES]; int n; };
struct MaLaneState {
    int c, Lc, cfl, issy;                      // carried bytes, their slot length, issy | npd << 2 | MA_CFL_HEM of that slot, ISSY length in use
    int iscr_valid; unsigned iscr;
    int frames, broken, undecided, hem;        // hem: high-efficiency-mode frames among `frames`
    long long packets, nulls, ts_errs;
};
struct MaStreamState { unsigned seen[8]; int rejected, skipped; };
struct MaFrameRec {
    int lane, isi, L, cfl;                     // lane: 0..7, -1 skipped (not TS / ISI not selected), -2 header rejected; L 0: ISSY length unknown
    int s0, nslots, tail, df, data_off, nostart;
    int nnull, issy_dec, first_byte, iscr_valid;
    unsigned iscr;
    int gse;                                   // a GSE frame of lane `lane` that is walked (df, data_off set; the TS fields are not)
    unsigned long long errmask;
};
struct MaFrameDesc { const uint8_t* carry; int out_off, joined, c, dnp, tei, pad; };
struct MaFin { const uint8_t* src; int len, pad; };

// ------------------------------------------------------------------------------------------------- GSE per lane
__host__ __device__ inline bool ma_gse_frame(const MaHdr& h) { return h.ts_gs == 1 && h.upl == 0 && !h.issyi && !h.npd && !h.hem; }
struct MaGseLane { GseDevState g; long long malformed; };          // three slots, the counters, the last END's verdict
struct MaGseFrame { int npkt, malformed, over, pad; };              // over: more than GSE_PKT_CAP packets (the one host fallback)
enum { MA_GSE_DONE = 0, MA_GSE_RECORDS = 1, MA_GSE_STORAGE = 2 };
struct MaGseOut { int open_last[3]; int nrows, flag, rowbase, pad[2]; };   // per lane and call; rowbase: its rows in the stream's table
struct MaGseDev {                                                   // what the lane pass needs for GSE (all null while the switch is off)
    const MaGseFrame* gfr; GsePkt* pkts; dvbs2gpu_gse_pdu* rows;
    const MaGseLane* lanes_old; MaGseLane* lanes_new; MaGseOut* out; int* info;
};

// CRC-8 tables: T[k][x] = CRC of byte x followed by k zero bytes (k < 4); ADV[k][b] = register bit b after k zero bytes (k <= 192)
constexpr int MA_TAB_BYTES = 1024 + (MA_CARRY + 1) * 8;
static void ma_build_tables(uint8_t* t) {
    for (int x = 0; x < 256; ++x) {
        unsigned c = x;
        for (int i = 0; i < 8; ++i) c = (c & 0x80) ? ((c << 1) ^ 0xD5) & 0xff : (c << 1) & 0xff;   // the BBHEADER's polynomial, MSB first
        t[x] = (uint8_t)c;
    }
    for (int k = 1; k < 4; ++k) for (int x = 0; x < 256; ++x) t[k * 256 + x] = t[t[(k - 1) * 256 + x]];
    uint8_t* adv = t + 1024;
    for (int b = 0; b < 8; ++b) adv[b] = (uint8_t)(1u << b);
    for (int k = 1; k <= MA_CARRY; ++k) for (int b = 0; b < 8; ++b) adv[k * 8 + b] = t[adv[(k - 1) * 8 + b]];
}

typedef unsigned __attribute__((aligned(1))) unaligned_u32;

__device__ inline int ma_frame_off(const int* foff, int s, int f, int max_frames, int fbytes) {
    return foff ? foff[s * (max_frames + 1) + f] : f * fbytes;
}

__global__ void __launch_bounds__(256) bbts_ma_frame_kernel(const uint8_t* const* __restrict__ in, const int* __restrict__ foff, int fbytes,
                                                            const int* __restrict__ nframes, int nstreams, int max_frames, MaCfg cfg,
                                                            const MaSel* __restrict__ sel, const MaLaneState* __restrict__ lanes,
                                                            const uint8_t* __restrict__ tabs, MaFrameRec* __restrict__ recs) {
    __shared__ uint8_t T[4][256];
    for (int i = threadIdx.x; i < 1024; i += 256) (&T[0][0])[i] = tabs[i];
    __syncthreads();
    const int lane = threadIdx.x & 63, w = blockIdx.x * 4 + (threadIdx.x >> 6);
    const int s = w / max_frames, f = w % max_frames;
    if (s >= nstreams || f >= nframes[s]) return;
    const uint8_t* bb = in[s];
    const int off = ma_frame_off(foff, s, f, max_frames, fbytes), size = ma_frame_off(foff, s, f + 1, max_frames, fbytes) - off;
    MaFrameRec r = {};
    MaFrameRec* out = recs + (size_t)s * max_frames + f;
    MaHdr h;
    if (!ma_header(bb + off, size, cfg.hem, &h)) { r.lane = -2; if (lane == 0) *out = r; return; }
    r.isi = h.isi; r.lane = -1;
    const MaSel se = sel[s];
    for (int k = se.n - 1; k >= 0; --k) if (se.isi[k] == h.isi) r.lane = k;
    if (cfg.gse && r.lane >= 0 && ma_gse_frame(h)) {
        r.gse = 1; r.df = h.df; r.data_off = off + 10;
        if (lane == 0) *out = r;
        return;
    }
    if (h.ts_gs != 3 || r.lane < 0) { r.lane = -1; if (lane == 0) *out = r; return; }
    if (h.hem) {                                   // no sync byte, CRC-8 or ISSY field in the slot: geometry, DNP sum, the header's ISCR
        const int L = ma_hem_slot_len(h.npd);
        r.L = L; r.cfl = h.npd << 2 | MA_CFL_HEM; r.s0 = h.s0; r.df = h.df; r.data_off = off + 10; r.nostart = h.nostart;
        if (h.nostart) { if (lane == 0) *out = r; return; }
        int n = (h.df - h.s0) / L;                 // a slot leaves with its own last byte
        n = n < 64 ? n : 64;
        r.nslots = n; r.tail = h.df - h.s0 - n * L;
        int sum = lane < n && h.npd && cfg.reinsert_nulls ? bb[off + 10 + h.s0 + lane * L + L - 1] : 0;
        for (int d = 32; d; d >>= 1) sum += __shfl_xor(sum, d);
        r.nnull = sum;
        if (h.issyi) {                             // of the first UP that starts here: bytes 2, 3 and 6 of the header
            const uint8_t fld[3] = {bb[off + 2], bb[off + 3], bb[off + 6]};
            r.iscr_valid = ma_iscr(fld, 3, &r.iscr);
        }
        if (lane == 0) *out = r;
        return;
    }
    int issy = 0;
    if (h.issyi) {
        issy = cfg.issy_bytes ? cfg.issy_bytes : lanes[s * MA_LANES + r.lane].issy;
        // not known yet: the first frame of this ISI in the call, up to this one, that shows an ISCR decides (64 frames at a time)
        for (int g0 = 0; g0 <= f && !issy; g0 += 64) {
            const int g = g0 + lane;
            int cand = 0;
            if (g <= f) {
                const int o = ma_frame_off(foff, s, g, max_frames, fbytes);
                MaHdr hg;
                if (ma_header(bb + o, ma_frame_off(foff, s, g + 1, max_frames, fbytes) - o, cfg.hem, &hg) && !hg.hem && hg.ts_gs == 3 && hg.isi == h.isi)
                    cand = ma_issy_cand(bb + o, hg);
            }
            const unsigned long long m = __ballot(cand != 0);
            if (m) issy = __shfl(cand, __ffsll((long long)m) - 1);
        }
        r.issy_dec = issy;
        if (!issy) { if (lane == 0) *out = r; return; }          // L = 0
    }
    const int L = ma_slot_len(issy, h.npd);
    r.L = L; r.cfl = issy | h.npd << 2; r.s0 = h.s0; r.df = h.df; r.data_off = off + 10; r.nostart = h.nostart;
    if (h.nostart) { if (lane == 0) *out = r; return; }
    const uint8_t* data = bb + off + 10;
    int n = (h.df - h.s0 - 1) / L;
    n = n < 64 ? n : 64;
    r.nslots = n; r.tail = h.df - h.s0 - n * L; r.first_byte = data[h.s0];
    const bool act = lane < n;
    int dnp = 0, err = 0, has_iscr = 0;
    unsigned iscr = 0;
    if (act) {
        const uint8_t* p = data + h.s0 + lane * L;
        const int e = ma_crc_end(cfg.crc_span, L);
        unsigned crc = 0;
        int i = kMa.up_off;
        while (i < e) {
            if ((i & 3) == 0 && i + 4 <= e) {
                const unsigned v = *reinterpret_cast<const unaligned_u32*>(p + i);
                crc = T[3][(v & 0xff) ^ crc] ^ T[2][(v >> 8) & 0xff] ^ T[1][(v >> 16) & 0xff] ^ T[0][v >> 24];
                i += 4;
            } else {
                crc = T[0][crc ^ p[i]];
                ++i;
            }
        }
        err = cfg.check_crc && crc != p[L];
        if (h.npd && cfg.reinsert_nulls) dnp = p[L - 1];
        if (issy) has_iscr = ma_iscr(p + kMa.issy_off, issy, &iscr);
    }
    r.errmask = __ballot(err);
    int sum = dnp;
    for (int d = 32; d; d >>= 1) sum += __shfl_xor(sum, d);
    r.nnull = sum;
    const unsigned long long vm = __ballot(has_iscr);
    if (vm) { r.iscr_valid = 1; r.iscr = __shfl(iscr, 63 - __clzll((long long)vm)); }
    if (lane == 0) *out = r;
}

// CRC-8 of the slot `carry[0..c) ++ data[0..)` over [up_off, e), by one wave: every byte's contribution advanced to the end, XORed
__device__ inline unsigned ma_wave_crc(const uint8_t* carry, int c, const uint8_t* data, int e, const uint8_t* adv, int lane) {
    unsigned x = 0;
    for (int i = kMa.up_off + lane; i < e; i += 64) {
        const unsigned v = i < c ? carry[i] : data[i - c];
        const uint8_t* a = adv + (e - i) * 8;
        for (int b = 0; b < 8; ++b) if (v >> b & 1) x ^= a[b];
    }
    for (int d = 32; d; d >>= 1) x ^= __shfl_xor(x, d);
    return x;
}

template <bool GSE>
__global__ void __launch_bounds__(256) bbts_ma_lane_kernel(const uint8_t* const* __restrict__ in, const int* __restrict__ nframes, int nstreams,
                                                           int max_frames, MaCfg cfg, const MaSel* __restrict__ sel,
                                                           const MaFrameRec* __restrict__ recs, const uint8_t* __restrict__ tabs,
                                                           const MaLaneState* __restrict__ lanes_old, MaLaneState* __restrict__ lanes_new,
                                                           const MaStreamState* __restrict__ strm_old, MaStreamState* __restrict__ strm_new,
                                                           const uint8_t* __restrict__ carry_old, uint8_t* __restrict__ joinbuf,
                                                           MaFrameDesc* __restrict__ desc, MaFin* __restrict__ fins, int* __restrict__ needed,
                                                           MaGseDev gd) {
    const int lane = threadIdx.x & 63, w = blockIdx.x * 4 + (threadIdx.x >> 6);
    const int s = w / MA_LANES, slot = w % MA_LANES;
    if (s >= nstreams) return;
    const int nf = nframes[s];
    const uint8_t* bb = in[s];
    const uint8_t* adv = tabs + 1024;
    const MaFrameRec* rs = recs + (size_t)s * max_frames;
    MaLaneState st = lanes_old[w];
    const uint8_t* carry = carry_old + (size_t)w * MA_CARRY;
    if (slot == 0) {                               // the stream's own counters travel with its first lane
        MaStreamState ss = strm_old[s];
        for (int f = 0; f < nf; ++f) {
            const int l = rs[f].lane, isi = rs[f].isi;
            if (l == -2) { ++ss.rejected; continue; }
            for (int k = 0; k < 8; ++k) if (k == isi >> 5) ss.seen[k] |= 1u << (isi & 31);   // (a variable index would put the array into LDS)
            if (l == -1) ++ss.skipped;
        }
        if (lane == 0) strm_new[s] = ss;
    }
    int out_off = 0;
    // GSE: the lane's context and what this call does to it; every lane of the wave computes the same, lane 0 stores
    MaGseLane gs = {};
    GseStreamOut so = {{-1, -1, -1}, 0, 0, {0, 0, 0}};
    int gflag = MA_GSE_DONE, rowbase = 0;
    if (GSE) gs = gd.lanes_old[w];
    if (slot < sel[s].n) {
        if (GSE)                                   // the lane's rows follow those of the lower lanes' GSE frames in the stream's table
            for (int f = 0; f < nf; ++f) if (rs[f].gse && rs[f].lane < slot) rowbase += GSE_PKT_CAP;
        for (int f = 0; f < nf; ++f) {
            const MaFrameRec r = rs[f];
            if (r.lane != slot) continue;
            ++st.frames;
            if (GSE && r.gse) {
                if (gflag) continue;
                if (!gd.pkts) { gflag = MA_GSE_STORAGE; continue; }
                const MaGseFrame gf = gd.gfr[(size_t)s * max_frames + f];
                if (gf.over) { gflag = MA_GSE_RECORDS; continue; }
                ++gs.g.cnt.frames; gs.malformed += gf.malformed;
                GsePkt* pk = gd.pkts + (size_t)s * max_frames * GSE_PKT_CAP;
                dvbs2gpu_gse_pdu* row = gd.rows + (size_t)s * max_frames * GSE_PKT_CAP + rowbase;
                for (int k = 0; k < gf.npkt; ++k) gse_apply_packet(gs.g, so, out_off, INT_MAX, pk, f * GSE_PKT_CAP + k, row, lane == 0);
                continue;
            }
            if (r.issy_dec) st.issy = r.issy_dec;
            if (r.L == 0) { ++st.undecided; st.c = 0; continue; }
            const uint8_t* data = bb + r.data_off;
            const int issy = r.cfl & 3, npd = r.cfl >> 2 & 1, hem = r.cfl & MA_CFL_HEM;
            if (hem) ++st.hem;
            const bool same = st.Lc == r.L && (st.cfl & MA_CFL_HEM) == hem;       // the carried bytes are of this frame's slot shape
            if (r.nostart) {                       // the whole data field continues the carried slot: collect both in this frame's join buffer
                if (st.c > 0) {
                    if (same && st.c + r.df <= r.L) {
                        uint8_t* jb = joinbuf + ((size_t)s * max_frames + f) * MA_CARRY;
                        for (int i = lane; i < st.c + r.df; i += 64) jb[i] = i < st.c ? carry[i] : data[i - st.c];
                        __threadfence();
                        carry = jb; st.c += r.df;
                    } else {
                        ++st.broken; st.c = 0;
                    }
                }
                continue;
            }
            MaFrameDesc d = {carry, out_off, 0, st.c, 0, 0, 0};
            if (st.c > 0) {
                if (same && st.c + r.s0 == r.L) {
                    d.joined = 1;
                    if (npd && cfg.reinsert_nulls) d.dnp = r.s0 > 0 ? data[r.s0 - 1] : carry[st.c - 1];
                    if (cfg.check_crc && !hem) d.tei = ma_wave_crc(carry, st.c, data, ma_crc_end(cfg.crc_span, r.L), adv, lane) != (unsigned)r.first_byte;
                    if (issy) {
                        uint8_t fld[3];
                        for (int k = 0; k < 3; ++k) { const int i = kMa.issy_off + k; fld[k] = k < issy ? (i < st.c ? carry[i] : data[i - st.c]) : 0; }
                        unsigned v;
                        if (ma_iscr(fld, issy, &v)) { st.iscr = v; st.iscr_valid = 1; }
                    }
                    ++st.packets; st.nulls += d.dnp; st.ts_errs += d.tei;
                    out_off += (1 + d.dnp) * MA_TS;
                } else {
                    ++st.broken;
                }
            }
            if (lane == 0) desc[(size_t)s * max_frames + f] = d;
            out_off += (r.nslots + r.nnull) * MA_TS;
            st.packets += r.nslots; st.nulls += r.nnull; st.ts_errs += __popcll(r.errmask);
            if (r.iscr_valid) { st.iscr = r.iscr; st.iscr_valid = 1; }
            st.c = r.tail; st.Lc = r.L; st.cfl = r.cfl;
            carry = data + r.s0 + r.nslots * r.L;
        }
    }
    if (lane == 0) {
        lanes_new[w] = st;
        MaFin fn = {carry, st.c, 0};
        fins[w] = fn;
        needed[w] = out_off;
        if (GSE) {
            MaGseOut o = {{-1, -1, -1}, so.nrows, gflag, rowbase, {0, 0}};
            if (gs.g.slot[0].busy) o.open_last[0] = so.open_last[0];
            if (gs.g.slot[1].busy) o.open_last[1] = so.open_last[1];
            if (gs.g.slot[2].busy) o.open_last[2] = so.open_last[2];
            gd.lanes_new[w] = gs;
            gd.out[w] = o;
            gd.info[w] = gflag | so.nrows << 2;
        }
    }
}

// ------------------------------------------------------------------------------------------------- GSE: frame pass, byte movement
__global__ void __launch_bounds__(256) bbts_ma_gse_scan_kernel(const uint8_t* const* __restrict__ in, const int* __restrict__ nframes, int max_frames,
                                                               const MaFrameRec* __restrict__ recs, MaGseFrame* __restrict__ gfr,
                                                               GsePkt* __restrict__ pkts) {
    const int s = blockIdx.y, f = blockIdx.x, tid = threadIdx.x;
    if (f >= nframes[s]) return;
    const MaFrameRec r = recs[(size_t)s * max_frames + f];
    if (!r.gse) return;
    __shared__ __attribute__((aligned(16))) uint8_t stage[MA_MAX_FRAME - 10];
    __shared__ GsePkt rec[GSE_PKT_CAP];
    __shared__ int span_at[GSE_PKT_CAP], span_len[GSE_PKT_CAP];
    __shared__ MaGseFrame fr;
    // r.df <= frame size - 10 <= sizeof(stage) by ma_header and the size check of the call
    gse_walk_frame<GseStrict>(in[s], r.data_off, r.df, stage, rec, span_at, span_len,
                              [&]() -> GseWalkRange { return {r.data_off, r.data_off + r.df, r.data_off + r.df}; },
                              [&](int n, int why) { fr = {why == GSE_OVER ? 0 : n, why == GSE_MALFORMED, why == GSE_OVER, 0}; }, &fr.npkt,
                              pkts + ((size_t)s * max_frames + f) * GSE_PKT_CAP, tid);
    if (tid == 0) gfr[(size_t)s * max_frames + f] = fr;
}

// nframes: 0 for a stream whose call the host parser runs
__global__ void __launch_bounds__(256) bbts_ma_gse_move_kernel(const uint8_t* const* __restrict__ in, uint8_t* const* __restrict__ out,
                                                               const int* __restrict__ nframes, int max_frames, const MaFrameRec* __restrict__ recs,
                                                               const MaGseFrame* __restrict__ gfr, const GsePkt* __restrict__ pkts,
                                                               const dvbs2gpu_gse_pdu* __restrict__ rows, const MaGseOut* __restrict__ gout,
                                                               const int* __restrict__ slotmap, const uint8_t* __restrict__ slots) {
    const int s = blockIdx.y, f = blockIdx.x;
    if (f >= nframes[s]) return;
    const MaFrameRec r = recs[(size_t)s * max_frames + f];
    if (!r.gse) return;
    const int w = s * MA_LANES + r.lane, sm = slotmap[w];
    if (sm < 0) return;
    const size_t sb = (size_t)s * max_frames * GSE_PKT_CAP;
    gse_move_packets(in[s], out[w], pkts + sb, rows + sb + gout[w].rowbase, f, gfr[(size_t)s * max_frames + f].npkt,
                     slots + (size_t)sm * 3 * GSE_SLOT_BYTES);
}

__global__ void __launch_bounds__(256) bbts_ma_gse_append_kernel(const uint8_t* const* __restrict__ in, const int* __restrict__ nframes,
                                                                 int max_frames, const GsePkt* __restrict__ pkts, const MaGseOut* __restrict__ gout,
                                                                 const int* __restrict__ slotmap, const int* __restrict__ placed,
                                                                 uint8_t* __restrict__ slots) {
    const int w = placed[blockIdx.y], r = blockIdx.x;      // the lanes that have a place in the pool: the selected ones
    if (w < 0) return;
    const int s = w / MA_LANES;
    if (nframes[s] == 0) return;
    const int at = gout[w].open_last[r], sm = slotmap[w];
    if (at < 0 || sm < 0) return;
    gse_append_chain(in[s], pkts + (size_t)s * max_frames * GSE_PKT_CAP, at, slots + ((size_t)sm * 3 + r) * GSE_SLOT_BYTES);
}

__device__ inline void ma_store4(uint8_t* o, unsigned v, bool aligned) {
    if (aligned) {
        *reinterpret_cast<unsigned*>(o) = v;
    } else {
        o[0] = (uint8_t)v; o[1] = (uint8_t)(v >> 8); o[2] = (uint8_t)(v >> 16); o[3] = (uint8_t)(v >> 24);
    }
}
// `dnp` null packets, then 0x47 + the 187 UP bytes of one slot, by one wave; 188 = 4 * 47: a dword never straddles two packets
// UP: where the UP starts in the slot (kMa.up_off or kHem.up_off); the byte before it, if there is one, gives way to 0x47
template <int UP>
__device__ inline void ma_put_slot(uint8_t* o, int dnp, const uint8_t* carry, int c, const uint8_t* data, int tei, bool aligned, int lane) {
    for (int w = lane; w < dnp * 47; w += 64) ma_store4(o + 4 * w, w % 47 == 0 ? 0x10ff1f47u : 0xffffffffu, aligned);
    o += (size_t)dnp * MA_TS;
    if (lane < 47) {
        const int i = UP - 1 + 4 * lane;                         // slot bytes [i, i + 4); data[] starts at slot byte c
        unsigned v;
        if (i >= c && i >= 0) {
            v = *reinterpret_cast<const unaligned_u32*>(data + i - c);
        } else {                                                 // (slot byte -1 of a HEM slot is not read)
            v = 0;
            for (int k = 0; k < 4; ++k) if (i + k >= 0) v |= (unsigned)(i + k < c ? carry[i + k] : data[i + k - c]) << (8 * k);
        }
        if (lane == 0) v = ((v & ~0xffu) | 0x47u) | (tei ? 0x8000u : 0u);
        ma_store4(o + 4 * lane, v, aligned);
    }
}

// the joined slot by the last wave, the whole slots of the frame by all four
template <int UP>
__device__ inline void ma_put_frame(uint8_t* o, const MaFrameRec& r, const MaFrameDesc& d, const uint8_t* data, const int* idx, const int* dnps,
                                    int wave, int lane) {
    const bool aligned = (reinterpret_cast<uintptr_t>(o) & 3) == 0;
    if (d.joined) {
        if (wave == 3) ma_put_slot<UP>(o, d.dnp, d.carry, d.c, data, d.tei, aligned, lane);
        o += (size_t)(1 + d.dnp) * MA_TS;
    }
    for (int k = wave; k < r.nslots; k += 4)
        ma_put_slot<UP>(o + (size_t)idx[k] * MA_TS, dnps[k], nullptr, 0, data + r.s0 + k * r.L, (int)(r.errmask >> k & 1), aligned, lane);
}

__global__ void __launch_bounds__(256) bbts_ma_emit_kernel(const uint8_t* const* __restrict__ in, uint8_t* const* __restrict__ out,
                                                           const int* __restrict__ nframes, int max_frames, MaCfg cfg,
                                                           const MaFrameRec* __restrict__ recs, const MaFrameDesc* __restrict__ desc,
                                                           const MaFin* __restrict__ fins, uint8_t* __restrict__ carry_new) {
    __shared__ int idx[64], dnps[64];
    const int s = blockIdx.y, f = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (f == max_frames) {                         // what every lane of this stream carries into the next call
        for (int l = 0; l < MA_LANES; ++l) {
            const MaFin fn = fins[s * MA_LANES + l];
            uint8_t* nw = carry_new + (size_t)(s * MA_LANES + l) * MA_CARRY;
            for (int i = threadIdx.x; i < fn.len; i += blockDim.x) nw[i] = fn.src[i];
        }
        return;
    }
    if (f >= nframes[s]) return;
    const MaFrameRec r = recs[(size_t)s * max_frames + f];
    if (r.lane < 0 || r.L == 0 || r.nostart) return;
    const MaFrameDesc d = desc[(size_t)s * max_frames + f];
    const uint8_t* data = in[s] + r.data_off;
    const int npd = r.cfl >> 2 & 1;
    if (wave == 0) {                               // packet index of every whole slot inside the frame: prefix sum of 1 + DNP
        int dn = 0;
        if (lane < r.nslots && npd && cfg.reinsert_nulls) dn = data[r.s0 + (lane + 1) * r.L - 1];
        int inc = 1 + dn;
        for (int k = 1; k < 64; k <<= 1) { const int t = __shfl_up(inc, k); if (lane >= k) inc += t; }
        idx[lane] = inc - 1 - dn; dnps[lane] = dn;
    }
    __syncthreads();
    uint8_t* o = out[s * MA_LANES + r.lane] + d.out_off;
    if (r.cfl & MA_CFL_HEM) ma_put_frame<kHem.up_off>(o, r, d, data, idx, dnps, wave, lane);
    else ma_put_frame<kMa.up_off>(o, r, d, data, idx, dnps, wave, lane);
}

// ------------------------------------------------------------------------------------------------- host parser
// The same rules, one byte at a time, for one stream in host memory.
struct MaHostStream {
    MaLaneState st[MA_LANES] = {};
    uint8_t carry[MA_LANES][MA_CARRY] = {};
    MaStreamState ss = {};
    uint8_t tab[256];
    // GSE: per lane the context (bbts_host.h: state, the bytes of its open reassemblies, the rows of the last call)
    GseHostCtx gse[MA_LANES];
    long long malformed[MA_LANES] = {};

    MaHostStream() {
        uint8_t t[MA_TAB_BYTES];
        ma_build_tables(t);
        memcpy(tab, t, 256);
    }
    void gse_reset() {
        for (int k = 0; k < MA_LANES; ++k) { gse[k] = GseHostCtx(); malformed[k] = 0; }
    }
    void clear_rows() { for (auto& c : gse) c.rows.clear(); }
    unsigned crc(const uint8_t* p, int a, int e) const {
        unsigned c = 0;
        for (int i = a; i < e; ++i) c = tab[c ^ p[i]];
        return c;
    }
    // one slot (L bytes at p) -> out; chk < 0: no CRC-8 to compare with; up: where its UP starts (a HEM slot: kHem.up_off, issy 0, chk < 0)
    void emit(MaLaneState& l, const uint8_t* p, int L, int issy, int npd, int chk, const MaCfg& cfg, std::vector<uint8_t>& out, int up = kMa.up_off) const {
        const int dnp = npd && cfg.reinsert_nulls ? p[L - 1] : 0;
        for (int k = 0; k < dnp; ++k) {
            const size_t at = out.size();
            out.resize(at + MA_TS, 0xff);
            out[at] = 0x47; out[at + 1] = 0x1f; out[at + 3] = 0x10;
        }
        l.nulls += dnp;
        const size_t at = out.size();
        out.push_back(0x47);
        out.insert(out.end(), p + up, p + up + kMa.up_len);
        if (cfg.check_crc && chk >= 0 && crc(p, kMa.up_off, ma_crc_end(cfg.crc_span, L)) != (unsigned)chk) { out[at + 1] |= 0x80; ++l.ts_errs; }
        ++l.packets;
        unsigned v;
        if (issy && ma_iscr(p + kMa.issy_off, issy, &v)) { l.iscr = v; l.iscr_valid = 1; }
    }
    void frame(const uint8_t* fr, int size, const MaCfg& cfg, const MaSel& sel, std::vector<uint8_t>* outs) {
        MaHdr h;
        if (!ma_header(fr, size, cfg.hem, &h)) { ++ss.rejected; return; }
        ss.seen[h.isi >> 5] |= 1u << (h.isi & 31);
        int slot = -1;
        for (int k = sel.n - 1; k >= 0; --k) if (sel.isi[k] == h.isi) slot = k;
        if (cfg.gse && slot >= 0 && ma_gse_frame(h)) {     // strict rules, offsets from the start of the data field
            ++st[slot].frames;
            GseGrowingOut sink = {outs[slot]};
            if (gse[slot].frame<GseStrict>(fr + 10, 0, h.df, h.df, sink) == GSE_MALFORMED) ++malformed[slot];
            return;
        }
        if (h.ts_gs != 3 || slot < 0) { ++ss.skipped; return; }
        MaLaneState& l = st[slot];
        uint8_t* cy = carry[slot];
        ++l.frames;
        if (h.hem) { hem_frame(l, cy, fr, h, cfg, outs[slot]); return; }
        int issy = 0;
        if (h.issyi) {
            if (!l.issy) l.issy = ma_issy_cand(fr, h);
            if (!l.issy) { ++l.undecided; l.c = 0; return; }
            issy = l.issy;
        }
        const int L = ma_slot_len(issy, h.npd);
        const uint8_t* data = fr + 10;
        if (h.nostart) {
            if (l.c > 0) {
                if (l.Lc == L && !(l.cfl & MA_CFL_HEM) && l.c + h.df <= L) { memcpy(cy + l.c, data, h.df); l.c += h.df; }
                else { ++l.broken; l.c = 0; }
            }
            return;
        }
        if (l.c > 0) {
            if (l.Lc == L && !(l.cfl & MA_CFL_HEM) && l.c + h.s0 == L) {
                memcpy(cy + l.c, data, h.s0);
                emit(l, cy, L, issy, h.npd, data[h.s0], cfg, outs[slot]);
            } else {
                ++l.broken;
            }
        }
        const int n = (h.df - h.s0 - 1) / L;
        for (int k = 0; k < n; ++k) emit(l, data + h.s0 + k * L, L, issy, h.npd, data[h.s0 + (k + 1) * L], cfg, outs[slot]);
        l.c = h.df - h.s0 - n * L; l.Lc = L; l.cfl = issy | h.npd << 2;
        memcpy(cy, data + h.s0 + n * L, l.c);
    }
    // a high-efficiency-mode frame of lane l: the framing above without the byte after a slot, the ISCR from the header
    void hem_frame(MaLaneState& l, uint8_t* cy, const uint8_t* fr, const MaHdr& h, const MaCfg& cfg, std::vector<uint8_t>& out) const {
        ++l.hem;
        const int L = ma_hem_slot_len(h.npd);
        const uint8_t* data = fr + 10;
        const bool same = l.Lc == L && (l.cfl & MA_CFL_HEM);
        if (h.nostart) {
            if (l.c > 0) {
                if (same && l.c + h.df <= L) { memcpy(cy + l.c, data, h.df); l.c += h.df; }
                else { ++l.broken; l.c = 0; }
            }
            return;
        }
        if (l.c > 0) {
            if (same && l.c + h.s0 == L) {
                memcpy(cy + l.c, data, h.s0);
                emit(l, cy, L, 0, h.npd, -1, cfg, out, kHem.up_off);
            } else {
                ++l.broken;
            }
        }
        const int n = (h.df - h.s0) / L;
        for (int k = 0; k < n; ++k) emit(l, data + h.s0 + k * L, L, 0, h.npd, -1, cfg, out, kHem.up_off);
        const uint8_t fld[3] = {fr[2], fr[3], fr[6]};
        unsigned v;
        if (h.issyi && ma_iscr(fld, 3, &v)) { l.iscr = v; l.iscr_valid = 1; }
        l.c = h.df - h.s0 - n * L; l.Lc = L; l.cfl = h.npd << 2 | MA_CFL_HEM;
        memcpy(cy, data + h.s0 + n * L, l.c);
    }
};

// a whole slot held back for its CRC-8 leaves unchecked.  A HEM slot waits for nothing, so a HEM carry is a partial slot and is only
// cleared; the one whole one, completed by a SYNCD = 65535 frame with no frame behind it yet, leaves like any other
static void ma_flush_lane(MaHostStream& tool, MaLaneState& l, const uint8_t* cy, const MaCfg& cfg, std::vector<uint8_t>& out) {
    if (l.c > 0 && l.c == l.Lc) {
        tool.emit(l, cy, l.Lc, l.cfl & 3, l.cfl >> 2 & 1, -1, cfg, out, l.cfl & MA_CFL_HEM ? kHem.up_off : kMa.up_off);
        l.c = 0;
    } else if (l.cfl & MA_CFL_HEM) {
        l.c = 0;
    }
}

struct MaArgs {                                // the layout of d_args for n streams of up to mf frames
    ScratchLayout L;
    ScratchPart<const uint8_t*> in; ScratchPart<uint8_t*> out; ScratchPart<int> nf, need, foff, ginfo, nf2;
    MaArgs(size_t n, size_t mf) : in(L.add<const uint8_t*>(n)), out(L.add<uint8_t*>(n * MA_LANES)), nf(L.add<int>(n)), need(L.add<int>(n * MA_LANES)), foff(L.add<int>(n * (mf + 1))),
                                  ginfo(L.add<int>(n * MA_LANES)), nf2(L.add<int>(n)) {}   // GSE: flag | rows << 2 per lane; frame counts without the host parser's streams
};
struct BbtsMa {
    MaCfg cfg;
    std::vector<MaSel> sel;
    // device banks
    DevBuf<MaLaneState> d_lane[2];
    DevBuf<MaStreamState> d_strm[2];
    DevBuf<uint8_t> d_carry[2];
    int cur = 0;
    DevBuf<MaSel> d_sel;
    DevBuf<uint8_t> d_tabs, d_join;
    DevBuf<MaFrameRec> d_recs;
    DevBuf<MaFrameDesc> d_desc;
    DevBuf<MaFin> d_fins;
    DevBuf<uint8_t> d_args;                    // MaArgs: [in ptrs][8 out ptrs per stream][nframes][needed per lane][frame offsets]
    std::vector<int> h_foff;
    Workspace in1, out1;                       // staging of the single-stream host-buffer entry point
    // GSE (dvbs2gpu_bbts_ma_set_gse): contexts and per-call results from the first switch-on; records, rows and slot buffers from the
    // first GSE frame.  The slot pool has 3 x 64 KiB per SELECTED lane: slotmap[stream * 8 + k] is the lane's place in it or -1.
    DevBuf<MaGseLane> d_glane[2];
    DevBuf<MaGseOut> d_gout;
    DevBuf<int> d_slotmap;
    DevBuf<MaGseFrame> d_gfr;
    DevBuf<GsePkt> d_pkt;
    DevBuf<dvbs2gpu_gse_pdu> d_rows;
    DevBuf<uint8_t> d_slots;
    size_t slot_cap = 0;                       // lanes the pool holds
    std::vector<int> slotmap, slot_free, ginfo;
    std::vector<long long> fb_calls;           // per stream: calls the host parser ran
    std::vector<std::vector<dvbs2gpu_gse_pdu>> fb_rows;   // per lane: the rows of such a call
    std::vector<char> rows_host;
    // host-only banks
    std::unique_ptr<MaHostStream> host;
    MaHostStream tool;                         // flush of a device bank
};

void bbts_ma_free(BbtsMa* m) { delete m; }

static int ma_upload_sel(const BbtsBankView& v, BbtsMa* m) {
    if (!v.ctx) return 0;
    HIP_TRY(hipMemcpy(m->d_sel, m->sel.data(), m->sel.size() * sizeof(MaSel), hipMemcpyHostToDevice));
    return 0;
}

// frame offsets of one stream from its size list (null: all kbch/8); false when a size cannot be a BBFRAME
static bool ma_offsets(const int* sizes, int n, int fbytes, int* off) {
    off[0] = 0;
    for (int f = 0; f < n; ++f) {
        const int b = sizes ? sizes[f] : fbytes;
        if (b < 10 || b > MA_MAX_FRAME) return false;
        off[f + 1] = off[f] + b;
    }
    return true;
}

// ---- GSE storage of a device bank
// d_slotmap: lane -> place [nstreams * 8], then place -> lane [nstreams * 8, of which slot_cap are used] for the append launch
static int ma_gse_upload_map(BbtsMa* m) {
    const size_t nl = m->slotmap.size();
    std::vector<int> both(2 * nl, -1);
    for (size_t w = 0; w < nl; ++w) {
        both[w] = m->slotmap[w];
        if (m->slotmap[w] >= 0) both[nl + m->slotmap[w]] = (int)w;
    }
    HIP_TRY(hipMemcpy(m->d_slotmap, both.data(), both.size() * sizeof(int), hipMemcpyHostToDevice));
    return 0;
}
// the pool grows to `lanes` places; what the lanes in it hold is kept
static int ma_gse_grow_pool(BbtsMa* m, size_t lanes) {
    if (lanes <= m->slot_cap) return 0;
    DevBuf<uint8_t> nw;
    RC_TRY(nw.alloc(lanes * 3 * GSE_SLOT_BYTES, false, "hipMalloc(bbts gse slots)"));
    if (m->d_slots) {
        hipError_t e = hipMemcpy(nw, m->d_slots, m->slot_cap * 3 * GSE_SLOT_BYTES, hipMemcpyDeviceToDevice);
        if (e != hipSuccess) return fail_hip(e, "hipMemcpy(bbts gse slots)");
    }
    for (size_t k = lanes; k-- > m->slot_cap;) m->slot_free.push_back((int)k);
    m->d_slots = std::move(nw); m->slot_cap = lanes;
    return 0;
}
// every selected lane of `stream` gets a place in the pool (its old ones go back first: a new selection starts afresh)
static int ma_gse_place_stream(BbtsMa* m, int stream) {
    int* map = m->slotmap.data() + (size_t)stream * MA_LANES;
    for (int k = 0; k < MA_LANES; ++k) if (map[k] >= 0) { m->slot_free.push_back(map[k]); map[k] = -1; }
    const int want = m->sel[stream].n;
    if ((int)m->slot_free.size() < want) {
        // at least the missing places, and at least half as many again as there are: re-selecting stream after stream
        // reallocates and copies the pool a logarithmic number of times, not once per call
        const size_t miss = want - m->slot_free.size(), half = m->slot_cap / 2;
        size_t to = m->slot_cap + (miss > half ? miss : half);
        if (to > m->slotmap.size()) to = m->slotmap.size();      // every lane of the bank placed: never more (and then enough)
        const int rc = ma_gse_grow_pool(m, to);
        if (rc) return rc;
    }
    for (int k = 0; k < want; ++k) { map[k] = m->slot_free.back(); m->slot_free.pop_back(); }
    return 0;
}
// records, rows and the slot pool: when a bank with the switch on first meets a GSE frame
static int ma_gse_storage(const BbtsBankView& v, BbtsMa* m) {
    if (m->d_pkt) return 0;                        // the last of the allocations below: set when all of them stand
    const size_t nfr = (size_t)v.nstreams * v.max_frames;
    size_t lanes = 0;
    for (const MaSel& s : m->sel) lanes += s.n;
    // a call that failed half way (the pool is the large one) left what it had got: taken up here, not allocated again
    const char* what = "hipMalloc(bbts mode adaptation gse)";
    if (!m->d_gfr) RC_TRY(m->d_gfr.alloc(nfr, false, what));
    if (!m->d_rows) RC_TRY(m->d_rows.alloc(nfr * GSE_PKT_CAP, false, what));
    int rc = ma_gse_grow_pool(m, lanes > 0 ? lanes : 1);
    for (int i = 0; i < v.nstreams && !rc; ++i) rc = ma_gse_place_stream(m, i);
    if (rc || (rc = ma_gse_upload_map(m))) return rc;
    return m->d_pkt.alloc(nfr * GSE_PKT_CAP, false, what);
}

// the three slot buffers of lane w, or null while it has no place in the pool
static uint8_t* ma_lane_slots(BbtsMa* m, size_t w) { return m->slotmap[w] < 0 ? nullptr : m->d_slots + (size_t)m->slotmap[w] * 3 * GSE_SLOT_BYTES; }
// One stream of a device bank as a host parser, from state bank `bank`, and back: TS lanes, carried bytes, counters, GSE contexts and
// the bytes of their open reassemblies.  This is how the host parser runs a stream's call in place of the kernels.
static int ma_stream_to_host(BbtsMa* m, int i, int bank, MaHostStream& hs) {
    const size_t w0 = (size_t)i * MA_LANES;
    HIP_TRY(hipMemcpy(hs.st, m->d_lane[bank] + w0, sizeof(hs.st), hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(hs.carry, m->d_carry[bank] + w0 * MA_CARRY, sizeof(hs.carry), hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(&hs.ss, m->d_strm[bank] + i, sizeof(hs.ss), hipMemcpyDeviceToHost));
    for (int k = 0; k < MA_LANES; ++k) {
        const MaGseLane* gl = m->d_glane[bank] + w0 + k;
        const int rc = gse_ctx_to_host(hs.gse[k], &gl->g, ma_lane_slots(m, w0 + k));
        if (rc) return rc;
        HIP_TRY(hipMemcpy(&hs.malformed[k], &gl->malformed, sizeof(gl->malformed), hipMemcpyDeviceToHost));
    }
    return 0;
}
static int ma_stream_to_device(BbtsMa* m, int i, int bank, const MaHostStream& hs) {
    const size_t w0 = (size_t)i * MA_LANES;
    HIP_TRY(hipMemcpy(m->d_lane[bank] + w0, hs.st, sizeof(hs.st), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(m->d_carry[bank] + w0 * MA_CARRY, hs.carry, sizeof(hs.carry), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(m->d_strm[bank] + i, &hs.ss, sizeof(hs.ss), hipMemcpyHostToDevice));
    for (int k = 0; k < MA_LANES; ++k) {
        MaGseLane* gl = m->d_glane[bank] + w0 + k;
        const int rc = gse_ctx_to_device(hs.gse[k], &gl->g, ma_lane_slots(m, w0 + k));
        if (rc) return rc;
        HIP_TRY(hipMemcpy(&gl->malformed, &hs.malformed[k], sizeof(gl->malformed), hipMemcpyHostToDevice));
    }
    return 0;
}

}  // namespace s2

extern "C" {

void dvbs2gpu_bbts_ma_default_cfg(dvbs2gpu_bbts_ma_cfg* cfg) {
    if (!cfg) return;
    cfg->issy_bytes = 0; cfg->crc_span = 0; cfg->reinsert_nulls = 1; cfg->check_crc = 1;
}

int dvbs2gpu_bbts_ma_get_layout(int32_t* out4) {
    if (!out4) return DVBS2GPU_ERR_ARG;
    out4[0] = kMa.crc_off; out4[1] = kMa.up_off; out4[2] = kMa.up_len; out4[3] = kMa.issy_off;
    return 0;
}

int dvbs2gpu_bbts_ma_get_hem_layout(int32_t* out4) {
    if (!out4) return DVBS2GPU_ERR_ARG;
    out4[0] = kHem.up_off; out4[1] = kHem.up_len; out4[2] = kHem.dnp_off; out4[3] = kHem.mode;
    return 0;
}

int dvbs2gpu_bbts_create_host(int kbch_bits, int max_frames, dvbs2gpu_bbts** out) {
    if (!out || max_frames <= 0 || kbch_bits < 88 || kbch_bits % 8 || kbch_bits > 65536) return DVBS2GPU_ERR_ARG;
    *out = bbts_new_host_bank(kbch_bits, max_frames);
    return 0;
}

int dvbs2gpu_bbts_set_mode_adaptation(dvbs2gpu_bbts* b, const dvbs2gpu_bbts_ma_cfg* cfg) {
    if (!b) return DVBS2GPU_ERR_ARG;
    const BbtsBankView v = bbts_view(b);
    if (!cfg) {
        if (!*v.ma) return 0;
        if (v.ctx) HIP_TRY(hipSetDevice(v.ctx->device));
        bbts_ma_free(*v.ma);
        *v.ma = nullptr;
        return bbts_reset_reference_state(b);          // the reference-mode parser starts afresh
    }
    if ((cfg->issy_bytes != 0 && cfg->issy_bytes != 2 && cfg->issy_bytes != 3) || (cfg->crc_span != 0 && cfg->crc_span != 1)) {
        g_err = "mode adaptation: issy_bytes is 0 (auto), 2 or 3 and crc_span 0 or 1";
        return DVBS2GPU_ERR_ARG;
    }
    if (v.ctx) HIP_TRY(hipSetDevice(v.ctx->device));
    bbts_ma_free(*v.ma);
    *v.ma = nullptr;
    std::unique_ptr<BbtsMa> m(new BbtsMa());
    m->cfg = {cfg->issy_bytes, cfg->crc_span, cfg->reinsert_nulls != 0, cfg->check_crc != 0};
    MaSel s0 = {};
    s0.n = 1;                                      // ISI 0: a single-input-stream carrier works without a selection
    m->sel.assign(v.nstreams, s0);
    const size_t n = v.nstreams, nl = n * MA_LANES, nfr = n * v.max_frames;
    if (v.ctx) {
        const char* what = "hipMalloc(bbts mode adaptation)";
        for (int k = 0; k < 2; ++k) {
            RC_TRY(m->d_lane[k].alloc(nl, true, what));
            RC_TRY(m->d_strm[k].alloc(n, true, what));
            RC_TRY(m->d_carry[k].alloc(nl * MA_CARRY, true, what));
        }
        RC_TRY(m->d_sel.alloc(n, true, what));
        RC_TRY(m->d_tabs.alloc(MA_TAB_BYTES, true, what));
        RC_TRY(m->d_join.alloc(nfr * MA_CARRY, true, what));
        RC_TRY(m->d_recs.alloc(nfr, true, what));
        RC_TRY(m->d_desc.alloc(nfr, true, what));
        RC_TRY(m->d_fins.alloc(nl, true, what));
        RC_TRY(m->d_args.alloc(MaArgs(n, v.max_frames).L.bytes(), true, what));
        uint8_t t[MA_TAB_BYTES];
        ma_build_tables(t);
        HIP_TRY(hipMemcpy(m->d_tabs, t, sizeof(t), hipMemcpyHostToDevice));
        if (cfg->issy_bytes) {                         // a configured ISSY length is the lanes' from the start
            std::vector<MaLaneState> ls(nl);
            for (auto& l : ls) l.issy = cfg->issy_bytes;
            HIP_TRY(hipMemcpy(m->d_lane[0], ls.data(), nl * sizeof(MaLaneState), hipMemcpyHostToDevice));
        }
        m->h_foff.resize(n * (v.max_frames + 1));
        const int rc = ma_upload_sel(v, m.get());
        if (rc) return rc;
    } else {
        m->host.reset(new MaHostStream());
        for (auto& l : m->host->st) l.issy = cfg->issy_bytes;
    }
    *v.ma = m.release();
    return 0;
}

int dvbs2gpu_bbts_select_isi(dvbs2gpu_bbts* b, int stream, const uint8_t* isi, int n) {
    if (!b) return DVBS2GPU_ERR_ARG;
    const BbtsBankView v = bbts_view(b);
    BbtsMa* m = *v.ma;
    if (!m) { g_err = "select_isi: the mode-adaptation mode is off"; return DVBS2GPU_ERR_ARG; }
    if (stream < 0 || stream >= v.nstreams || n < 0 || n > MA_LANES || (n > 0 && !isi)) return DVBS2GPU_ERR_ARG;
    MaSel s = {};
    s.n = n;
    for (int k = 0; k < n; ++k) s.isi[k] = isi[k];
    m->sel[stream] = s;
    // the stream's lanes start afresh: state, counters and the carried bytes belong to the old selection
    std::vector<MaLaneState> z(MA_LANES);
    for (auto& l : z) l.issy = m->cfg.issy_bytes;
    if (v.ctx) {
        HIP_TRY(hipSetDevice(v.ctx->device));
        HIP_TRY(hipMemcpy(m->d_lane[m->cur] + (size_t)stream * MA_LANES, z.data(), MA_LANES * sizeof(MaLaneState), hipMemcpyHostToDevice));
        if (m->d_glane[0]) {                           // and so do their GSE contexts and, once there is a pool, their places in it
            HIP_TRY(hipMemset(m->d_glane[m->cur] + (size_t)stream * MA_LANES, 0, MA_LANES * sizeof(MaGseLane)));
            for (int k = 0; k < MA_LANES; ++k) { m->ginfo[stream * MA_LANES + k] = 0; m->rows_host[stream * MA_LANES + k] = 0; }
            if (m->d_pkt) {
                int rc = ma_gse_place_stream(m, stream);
                if (rc || (rc = ma_gse_upload_map(m))) return rc;
            }
        }
        return ma_upload_sel(v, m);
    }
    memcpy(m->host->st, z.data(), sizeof(m->host->st));
    m->host->gse_reset();
    return 0;
}

int dvbs2gpu_bbts_process_ma_batch(dvbs2gpu_bbts* b, const uint8_t* const* d_bb, const int* const* frame_bytes, const int* nframes,
                                   uint8_t* const* d_out, int cap, int* out_bytes, int* needed, void* stream) {
    if (!b || !d_bb || !nframes || !d_out || !out_bytes || cap < 0) return DVBS2GPU_ERR_ARG;
    const BbtsBankView v = bbts_view(b);
    BbtsMa* m = *v.ma;
    if (!v.ctx || !m) { g_err = "process_ma_batch: needs a device bank with the mode-adaptation mode on"; return DVBS2GPU_ERR_ARG; }
    HIP_TRY(hipSetDevice(v.ctx->device));
    hipStream_t st = (hipStream_t)stream;
    const int n = v.nstreams, nl = n * MA_LANES, mf = v.max_frames;
    for (int i = 0; i < n; ++i) {
        if (nframes[i] < 0 || nframes[i] > mf) { g_err = "frame count exceeds max_frames"; return DVBS2GPU_ERR_ARG; }
        if (nframes[i] > 0 && !d_bb[i]) return DVBS2GPU_ERR_ARG;
        for (int k = 0; k < m->sel[i].n; ++k) if (nframes[i] > 0 && !d_out[i * MA_LANES + k]) return DVBS2GPU_ERR_ARG;
        if (frame_bytes && !ma_offsets(frame_bytes[i], nframes[i], v.kbch / 8, m->h_foff.data() + (size_t)i * (mf + 1))) {
            g_err = "a BBFRAME is 10 to 7274 bytes";
            return DVBS2GPU_ERR_ARG;
        }
    }
    if (!frame_bytes && v.kbch / 8 > MA_MAX_FRAME) { g_err = "a BBFRAME is 10 to 7274 bytes"; return DVBS2GPU_ERR_ARG; }
    const MaArgs a(n, mf);
    const uint8_t** a_in = a.in(m->d_args); uint8_t** a_out = a.out(m->d_args);
    int *a_nf = a.nf(m->d_args), *a_need = a.need(m->d_args), *a_foff = a.foff(m->d_args);
    HIP_TRY(hipMemcpyAsync(a_in, d_bb, sizeof(void*) * n, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(a_out, d_out, sizeof(void*) * nl, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(a_nf, nframes, sizeof(int) * n, hipMemcpyHostToDevice, st));
    if (frame_bytes) HIP_TRY(hipMemcpyAsync(a_foff, m->h_foff.data(), sizeof(int) * n * (mf + 1), hipMemcpyHostToDevice, st));
    const int* foff = frame_bytes ? a_foff : nullptr;
    const int cur = m->cur;
    const bool gse = m->cfg.gse != 0;
    int *a_ginfo = a.ginfo(m->d_args), *a_nf2 = a.nf2(m->d_args);
    hipLaunchKernelGGL(bbts_ma_frame_kernel, dim3((n * mf + 3) / 4), dim3(256), 0, st, a_in, foff, v.kbch / 8, a_nf, n, mf, m->cfg, m->d_sel,
                       m->d_lane[cur], m->d_tabs, m->d_recs);
    std::vector<int> need(nl);
    // GSE on: the scan pass once the bank has its records, then the lane pass with the lanes' contexts.  A bank that meets its first GSE
    // frame learns so from the lanes' flags, gets its storage and runs the two again (that one call synchronises three times).
    auto lane_pass = [&]() -> int {
        if (gse) {
            if (m->d_pkt) hipLaunchKernelGGL(bbts_ma_gse_scan_kernel, dim3(mf, n), dim3(256), 0, st, a_in, a_nf, mf, m->d_recs, m->d_gfr, m->d_pkt);
            const MaGseDev gd = {m->d_gfr, m->d_pkt, m->d_rows, m->d_glane[cur], m->d_glane[cur ^ 1], m->d_gout, a_ginfo};
            hipLaunchKernelGGL(bbts_ma_lane_kernel<true>, dim3((nl + 3) / 4), dim3(256), 0, st, a_in, a_nf, n, mf, m->cfg, m->d_sel, m->d_recs, m->d_tabs,
                               m->d_lane[cur], m->d_lane[cur ^ 1], m->d_strm[cur], m->d_strm[cur ^ 1], m->d_carry[cur], m->d_join, m->d_desc,
                               m->d_fins, a_need, gd);
        } else {
            hipLaunchKernelGGL(bbts_ma_lane_kernel<false>, dim3((nl + 3) / 4), dim3(256), 0, st, a_in, a_nf, n, mf, m->cfg, m->d_sel, m->d_recs, m->d_tabs,
                               m->d_lane[cur], m->d_lane[cur ^ 1], m->d_strm[cur], m->d_strm[cur ^ 1], m->d_carry[cur], m->d_join, m->d_desc,
                               m->d_fins, a_need, MaGseDev{});
        }
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(need.data(), a_need, sizeof(int) * nl, hipMemcpyDeviceToHost, st));
        if (gse) HIP_TRY(hipMemcpyAsync(m->ginfo.data(), a_ginfo, sizeof(int) * nl, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        return 0;
    };
    { const int rc = lane_pass(); if (rc) return rc; }
    // the one host fallback: a frame with more than GSE_PKT_CAP packets.  The host parser runs that stream's call from the same state;
    // first only for the sizes, so that the capacity rule holds for it as for every other stream
    struct Fallback { int stream; MaHostStream hs; std::vector<uint8_t> outs[MA_LANES]; };
    std::vector<std::unique_ptr<Fallback>> fbs;
    bool moved = false;
    if (gse) {
        bool storage = false;
        for (int i = 0; i < nl; ++i) storage |= (m->ginfo[i] & 3) == MA_GSE_STORAGE;
        if (storage) {
            int rc = ma_gse_storage(v, m);
            if (rc || (rc = lane_pass())) return rc;
        }
        std::vector<uint8_t> h_in;
        for (int i = 0; i < n; ++i) {
            bool over = false;
            for (int k = 0; k < MA_LANES; ++k) over |= (m->ginfo[i * MA_LANES + k] & 3) == MA_GSE_RECORDS;
            if (!over) continue;
            std::unique_ptr<Fallback> fb(new Fallback());
            fb->stream = i;
            const int rc = ma_stream_to_host(m, i, cur, fb->hs);
            if (rc) return rc;
            std::vector<int> own(nframes[i] + 1);
            const int* off = frame_bytes ? m->h_foff.data() + (size_t)i * (mf + 1) : own.data();
            if (!frame_bytes) for (int f = 0; f <= nframes[i]; ++f) own[f] = f * (v.kbch / 8);
            h_in.resize(off[nframes[i]]);
            HIP_TRY(hipMemcpy(h_in.data(), d_bb[i], h_in.size(), hipMemcpyDeviceToHost));
            fb->hs.clear_rows();
            for (int f = 0; f < nframes[i]; ++f) fb->hs.frame(h_in.data() + off[f], off[f + 1] - off[f], m->cfg, m->sel[i], fb->outs);
            for (int k = 0; k < MA_LANES; ++k) need[i * MA_LANES + k] = (int)fb->outs[k].size();
            fbs.push_back(std::move(fb));
        }
        moved = m->d_pkt != nullptr;
    }
    bool fits = true;
    for (int i = 0; i < nl; ++i) {
        if (needed) needed[i] = need[i];
        fits = fits && need[i] <= cap;
    }
    if (!fits) {                                   // nothing committed: the shadow state is simply not taken
        for (int i = 0; i < nl; ++i) out_bytes[i] = 0;
        if (gse) { std::fill(m->ginfo.begin(), m->ginfo.end(), 0); std::fill(m->rows_host.begin(), m->rows_host.end(), 0); }
        g_err = "mode adaptation: an output does not fit into cap (needed[] has the sizes)";
        return DVBS2GPU_ERR_CAPACITY;
    }
    const int* e_nf = a_nf;
    if (!fbs.empty()) {                            // the kernels leave the host parser's streams alone
        std::vector<int> nf2(nframes, nframes + n);
        for (auto& fb : fbs) nf2[fb->stream] = 0;
        HIP_TRY(hipMemcpyAsync(a_nf2, nf2.data(), sizeof(int) * n, hipMemcpyHostToDevice, st));
        HIP_TRY(hipStreamSynchronize(st));         // nf2 leaves this scope
        e_nf = a_nf2;
    }
    hipLaunchKernelGGL(bbts_ma_emit_kernel, dim3(mf + 1, n), dim3(256), 0, st, a_in, a_out, e_nf, mf, m->cfg, m->d_recs, m->d_desc, m->d_fins,
                       m->d_carry[cur ^ 1]);
    if (moved) {
        hipLaunchKernelGGL(bbts_ma_gse_move_kernel, dim3(mf, n), dim3(256), 0, st, a_in, a_out, e_nf, mf, m->d_recs, m->d_gfr, m->d_pkt, m->d_rows,
                           m->d_gout, m->d_slotmap, m->d_slots);
        hipLaunchKernelGGL(bbts_ma_gse_append_kernel, dim3(3, (unsigned)m->slot_cap), dim3(256), 0, st, a_in, e_nf, mf, m->d_pkt, m->d_gout, m->d_slotmap,
                           m->d_slotmap + nl, m->d_slots);
    }
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(st));
    if (gse) std::fill(m->rows_host.begin(), m->rows_host.end(), 0);
    for (auto& fb : fbs) {                         // their output and their state, into the half the call makes current
        const int i = fb->stream;
        ++m->fb_calls[i];
        for (int k = 0; k < MA_LANES; ++k) {
            if (!fb->outs[k].empty()) HIP_TRY(hipMemcpy(d_out[i * MA_LANES + k], fb->outs[k].data(), fb->outs[k].size(), hipMemcpyHostToDevice));
            m->fb_rows[i * MA_LANES + k] = fb->hs.gse[k].rows;
            m->rows_host[i * MA_LANES + k] = 1;
        }
        const int rc = ma_stream_to_device(m, i, cur ^ 1, fb->hs);
        if (rc) return rc;
    }
    m->cur = cur ^ 1;
    for (int i = 0; i < nl; ++i) out_bytes[i] = need[i];
    return 0;
}

int dvbs2gpu_bbts_ma_work(dvbs2gpu_bbts* b, const uint8_t* h_bb, const int* frame_bytes, int cnt, uint8_t* const* h_out, int cap,
                          int* out_bytes, int* needed) {
    if (!b || !h_out || !out_bytes || cnt < 0 || cap < 0 || (cnt > 0 && !h_bb)) return DVBS2GPU_ERR_ARG;
    const BbtsBankView v = bbts_view(b);
    BbtsMa* m = *v.ma;
    if (!m || v.nstreams != 1) { g_err = "ma_work: needs a bank of one stream with the mode-adaptation mode on"; return DVBS2GPU_ERR_ARG; }
    if (cnt > v.max_frames) { g_err = "frame count exceeds max_frames"; return DVBS2GPU_ERR_ARG; }
    std::vector<int> off(cnt + 1);
    if (!ma_offsets(frame_bytes, cnt, v.kbch / 8, off.data())) { g_err = "a BBFRAME is 10 to 7274 bytes"; return DVBS2GPU_ERR_ARG; }
    const MaSel& sel = m->sel[0];
    for (int k = 0; k < sel.n; ++k) if (cnt > 0 && !h_out[k]) return DVBS2GPU_ERR_ARG;
    if (!v.ctx) {
        MaHostStream trial = *m->host;             // the state advances only when every output fits
        trial.clear_rows();
        std::vector<uint8_t> outs[MA_LANES];
        for (int f = 0; f < cnt; ++f) trial.frame(h_bb + off[f], off[f + 1] - off[f], m->cfg, sel, outs);
        bool fits = true;
        for (int k = 0; k < MA_LANES; ++k) {
            if (needed) needed[k] = (int)outs[k].size();
            fits = fits && (long)outs[k].size() <= cap;
            out_bytes[k] = 0;
        }
        if (!fits) {                               // nothing advanced; the failed call has no rows
            m->host->clear_rows();
            g_err = "mode adaptation: an output does not fit into cap (needed[] has the sizes)";
            return DVBS2GPU_ERR_CAPACITY;
        }
        *m->host = trial;
        for (int k = 0; k < MA_LANES; ++k) {
            out_bytes[k] = (int)outs[k].size();
            if (!outs[k].empty()) memcpy(h_out[k], outs[k].data(), outs[k].size());
        }
        return 0;
    }
    HIP_TRY(hipSetDevice(v.ctx->device));
    if (const int e = m->in1.ensure((size_t)v.max_frames * MA_MAX_FRAME + 64)) return e;
    if (cnt > 0) HIP_TRY(hipMemcpy(m->in1.p, h_bb, off[cnt], hipMemcpyHostToDevice));
    const size_t per = ((size_t)cap + 67) & ~(size_t)3;
    if (const int e = m->out1.ensure(per * MA_LANES)) return e;
    uint8_t* d_out[MA_LANES];
    for (int k = 0; k < MA_LANES; ++k) d_out[k] = static_cast<uint8_t*>(m->out1.p) + per * k;
    const uint8_t* in_p = static_cast<const uint8_t*>(m->in1.p);
    const int rc = dvbs2gpu_bbts_process_ma_batch(b, &in_p, frame_bytes ? &frame_bytes : nullptr, &cnt, d_out, cap, out_bytes, needed, nullptr);
    if (rc) return rc;
    for (int k = 0; k < sel.n; ++k) if (out_bytes[k] > 0) HIP_TRY(hipMemcpy(h_out[k], d_out[k], out_bytes[k], hipMemcpyDeviceToHost));
    return 0;
}

static int ma_flush(dvbs2gpu_bbts* b, uint8_t* const* out, int cap, int* out_bytes, bool host_out) {
    if (!b || !out || !out_bytes || cap < 0) return DVBS2GPU_ERR_ARG;
    const BbtsBankView v = bbts_view(b);
    BbtsMa* m = *v.ma;
    if (!m) { g_err = "ma_flush: the mode-adaptation mode is off"; return DVBS2GPU_ERR_ARG; }
    const int nl = v.nstreams * MA_LANES;
    std::vector<MaLaneState> ls(nl);
    std::vector<uint8_t> cy((size_t)nl * MA_CARRY);
    if (v.ctx) {
        HIP_TRY(hipSetDevice(v.ctx->device));
        HIP_TRY(hipMemcpy(ls.data(), m->d_lane[m->cur], nl * sizeof(MaLaneState), hipMemcpyDeviceToHost));
        HIP_TRY(hipMemcpy(cy.data(), m->d_carry[m->cur], cy.size(), hipMemcpyDeviceToHost));
    } else {
        memcpy(ls.data(), m->host->st, sizeof(m->host->st));
        memcpy(cy.data(), m->host->carry, sizeof(m->host->carry));
    }
    std::vector<std::vector<uint8_t>> outs(nl);
    for (int i = 0; i < nl; ++i) {
        out_bytes[i] = 0;
        if (i % MA_LANES >= m->sel[i / MA_LANES].n) continue;
        ma_flush_lane(m->tool, ls[i], cy.data() + (size_t)i * MA_CARRY, m->cfg, outs[i]);
        if ((long)outs[i].size() > cap) { g_err = "ma_flush: cap is smaller than a held packet and its null packets"; return DVBS2GPU_ERR_CAPACITY; }
        if (!outs[i].empty() && !out[i]) return DVBS2GPU_ERR_ARG;
    }
    for (int i = 0; i < nl; ++i) {
        if (outs[i].empty()) continue;
        if (v.ctx && !host_out) HIP_TRY(hipMemcpy(out[i], outs[i].data(), outs[i].size(), hipMemcpyHostToDevice));
        else memcpy(out[i], outs[i].data(), outs[i].size());
        out_bytes[i] = (int)outs[i].size();
    }
    if (v.ctx) HIP_TRY(hipMemcpy(m->d_lane[m->cur], ls.data(), nl * sizeof(MaLaneState), hipMemcpyHostToDevice));
    else memcpy(m->host->st, ls.data(), sizeof(m->host->st));
    return 0;
}

int dvbs2gpu_bbts_ma_flush(dvbs2gpu_bbts* b, uint8_t* const* out, int cap, int* out_bytes) { return ma_flush(b, out, cap, out_bytes, false); }
int dvbs2gpu_bbts_ma_flush_host(dvbs2gpu_bbts* b, uint8_t* const* h_out, int cap, int* out_bytes) { return ma_flush(b, h_out, cap, out_bytes, true); }

int dvbs2gpu_bbts_ma_get_stats(dvbs2gpu_bbts* b, int stream, int slot, dvbs2gpu_bbts_ma_stats* h_out) {
    if (!b || !h_out || slot < 0 || slot >= MA_LANES) return DVBS2GPU_ERR_ARG;
    const BbtsBankView v = bbts_view(b);
    BbtsMa* m = *v.ma;
    if (!m || stream < 0 || stream >= v.nstreams) return DVBS2GPU_ERR_ARG;
    MaLaneState l;
    MaStreamState ss;
    if (v.ctx) {
        HIP_TRY(hipSetDevice(v.ctx->device));
        HIP_TRY(hipMemcpy(&l, m->d_lane[m->cur] + (size_t)stream * MA_LANES + slot, sizeof(l), hipMemcpyDeviceToHost));
        HIP_TRY(hipMemcpy(&ss, m->d_strm[m->cur] + stream, sizeof(ss), hipMemcpyDeviceToHost));
    } else {
        l = m->host->st[slot]; ss = m->host->ss;
    }
    const MaSel& sel = m->sel[stream];
    dvbs2gpu_bbts_ma_stats o = {};
    o.packets = l.packets; o.nulls = l.nulls; o.ts_errs = l.ts_errs;
    o.broken_joins = l.broken; o.undecided = l.undecided; o.frames = l.frames;
    o.skipped_frames = ss.skipped; o.rejected_frames = ss.rejected;
    o.issy_bytes = l.issy; o.iscr_valid = l.iscr_valid; o.last_iscr = l.iscr; o.carried = l.c;
    o.selected = slot < sel.n; o.isi = o.selected ? sel.isi[slot] : -1;
    o.hem_frames = l.hem;
    *h_out = o;
    return 0;
}

int dvbs2gpu_bbts_ma_set_gse(dvbs2gpu_bbts* b, int on) {
    if (!b) return DVBS2GPU_ERR_ARG;
    const BbtsBankView v = bbts_view(b);
    BbtsMa* m = *v.ma;
    if (!m) { g_err = "ma_set_gse: the mode-adaptation mode is off"; return DVBS2GPU_ERR_ARG; }
    if (!v.ctx) {
        if (!on) m->host->gse_reset();
        m->cfg.gse = on != 0;
        return 0;
    }
    HIP_TRY(hipSetDevice(v.ctx->device));
    const size_t nl = (size_t)v.nstreams * MA_LANES;
    if (on && !m->d_glane[0]) {
        const char* what = "hipMalloc(bbts mode adaptation gse)";
        for (auto& gl : m->d_glane) RC_TRY(gl.alloc(nl, true, what));
        RC_TRY(m->d_gout.alloc(nl, false, what));
        RC_TRY(m->d_slotmap.alloc(2 * nl, false, what));
        m->slotmap.assign(nl, -1); m->ginfo.assign(nl, 0); m->rows_host.assign(nl, 0);
        m->fb_rows.resize(nl); m->fb_calls.assign(v.nstreams, 0);
    }
    if (!on && m->d_glane[0]) {                        // the lanes' GSE state is dropped; the storage stays with the bank
        HIP_TRY(hipMemset(m->d_glane[m->cur], 0, nl * sizeof(MaGseLane)));
        std::fill(m->ginfo.begin(), m->ginfo.end(), 0);
        std::fill(m->rows_host.begin(), m->rows_host.end(), 0);
        std::fill(m->fb_calls.begin(), m->fb_calls.end(), 0);
    }
    m->cfg.gse = on != 0;
    return 0;
}

int dvbs2gpu_bbts_ma_set_t2_hem(dvbs2gpu_bbts* b, int on) {
    if (!b) return DVBS2GPU_ERR_ARG;
    const BbtsBankView v = bbts_view(b);
    BbtsMa* m = *v.ma;
    if (!m) { g_err = "ma_set_t2_hem: the mode-adaptation mode is off"; return DVBS2GPU_ERR_ARG; }
    // every lane starts afresh, as after dvbs2gpu_bbts_select_isi: what is carried was cut by the other rules
    std::vector<MaLaneState> z((size_t)v.nstreams * MA_LANES);
    for (auto& l : z) l.issy = m->cfg.issy_bytes;
    if (v.ctx) {
        HIP_TRY(hipSetDevice(v.ctx->device));
        HIP_TRY(hipMemcpy(m->d_lane[m->cur], z.data(), z.size() * sizeof(MaLaneState), hipMemcpyHostToDevice));
    } else {
        memcpy(m->host->st, z.data(), sizeof(m->host->st));
    }
    m->cfg.hem = on != 0;
    return 0;
}

int dvbs2gpu_bbts_ma_get_gse_stats(dvbs2gpu_bbts* b, int stream, int slot, dvbs2gpu_bbts_ma_gse_stats* h_out) {
    if (!b || !h_out || slot < 0 || slot >= MA_LANES) return DVBS2GPU_ERR_ARG;
    const BbtsBankView v = bbts_view(b);
    BbtsMa* m = *v.ma;
    if (!m || stream < 0 || stream >= v.nstreams) return DVBS2GPU_ERR_ARG;
    MaGseLane gl = {};
    if (!v.ctx) {
        gl = {m->host->gse[slot].g, m->host->malformed[slot]};
    } else if (m->d_glane[0]) {
        HIP_TRY(hipSetDevice(v.ctx->device));
        HIP_TRY(hipMemcpy(&gl, m->d_glane[m->cur] + (size_t)stream * MA_LANES + slot, sizeof(gl), hipMemcpyDeviceToHost));
    }
    static_assert(sizeof(GseCounters) == 9 * sizeof(int64_t) && sizeof(dvbs2gpu_bbts_ma_gse_stats) == 12 * sizeof(int64_t), "layout");
    dvbs2gpu_bbts_ma_gse_stats o = {};
    memcpy(&o.frames, &gl.g.cnt, sizeof(GseCounters));
    o.malformed_frames = gl.malformed;
    o.host_fallback_calls = v.ctx && !m->fb_calls.empty() ? m->fb_calls[stream] : 0;
    o.open_slots = gl.g.slot[0].busy + gl.g.slot[1].busy + gl.g.slot[2].busy;
    o.last_crc_err = gl.g.crc_err;
    *h_out = o;
    return 0;
}

// the rows of lane (stream, slot) of the last call: where they are and how many
static int ma_rows(const BbtsBankView& v, BbtsMa* m, int stream, int slot, const dvbs2gpu_gse_pdu** host, const dvbs2gpu_gse_pdu** dev, int* n) {
    *host = nullptr; *dev = nullptr; *n = 0;
    const int w = stream * MA_LANES + slot;
    if (!v.ctx) { *host = m->host->gse[slot].rows.data(); *n = (int)m->host->gse[slot].rows.size(); return 0; }
    if (!m->d_glane[0]) return 0;
    if (m->rows_host[w]) { *host = m->fb_rows[w].data(); *n = (int)m->fb_rows[w].size(); return 0; }
    *n = m->ginfo[w] >> 2;
    if (*n == 0) return 0;
    MaGseOut o;
    HIP_TRY(hipMemcpy(&o, m->d_gout + w, sizeof(o), hipMemcpyDeviceToHost));
    *dev = m->d_rows + (size_t)stream * v.max_frames * GSE_PKT_CAP + o.rowbase;
    return 0;
}

int dvbs2gpu_bbts_ma_get_pdu_table(dvbs2gpu_bbts* b, int stream, int slot, dvbs2gpu_gse_pdu* h_rows, int cap, int* n) {
    if (!b || !n || cap < 0 || (cap > 0 && !h_rows) || slot < 0 || slot >= MA_LANES) return DVBS2GPU_ERR_ARG;
    const BbtsBankView v = bbts_view(b);
    BbtsMa* m = *v.ma;
    if (!m || stream < 0 || stream >= v.nstreams) return DVBS2GPU_ERR_ARG;
    if (v.ctx) HIP_TRY(hipSetDevice(v.ctx->device));
    const dvbs2gpu_gse_pdu *host, *dev;
    const int rc = ma_rows(v, m, stream, slot, &host, &dev, n);
    if (rc) return rc;
    const int k = *n < cap ? *n : cap;
    if (k <= 0) return 0;
    if (host) memcpy(h_rows, host, k * sizeof(dvbs2gpu_gse_pdu));
    else HIP_TRY(hipMemcpy(h_rows, dev, k * sizeof(dvbs2gpu_gse_pdu), hipMemcpyDeviceToHost));
    return 0;
}

int dvbs2gpu_bbts_ma_get_pdu_table_device(dvbs2gpu_bbts* b, int stream, int slot, const dvbs2gpu_gse_pdu** d_rows, int* n) {
    if (!b || !n || !d_rows || slot < 0 || slot >= MA_LANES) return DVBS2GPU_ERR_ARG;
    const BbtsBankView v = bbts_view(b);
    BbtsMa* m = *v.ma;
    if (!m || stream < 0 || stream >= v.nstreams) return DVBS2GPU_ERR_ARG;
    if (!v.ctx) { g_err = "ma_get_pdu_table_device: a host bank has no device table"; return DVBS2GPU_ERR_ARG; }
    HIP_TRY(hipSetDevice(v.ctx->device));
    const dvbs2gpu_gse_pdu *host, *dev;
    const int rc = ma_rows(v, m, stream, slot, &host, &dev, n);
    if (rc) return rc;
    *d_rows = dev;
    if (!host || *n == 0) return 0;
    // a call the host parser ran: its rows go to where the kernels put theirs, lane after lane, if the stream's table holds them
    size_t at = 0;
    for (int k = 0; k < slot; ++k) at += m->fb_rows[stream * MA_LANES + k].size();
    if (at + *n > (size_t)v.max_frames * GSE_PKT_CAP) { g_err = "more rows than the device table holds"; return DVBS2GPU_ERR_CAPACITY; }
    dvbs2gpu_gse_pdu* d = m->d_rows + (size_t)stream * v.max_frames * GSE_PKT_CAP + at;
    HIP_TRY(hipMemcpy(d, host, *n * sizeof(dvbs2gpu_gse_pdu), hipMemcpyHostToDevice));
    *d_rows = d;
    return 0;
}

int dvbs2gpu_bbts_get_isi_seen(dvbs2gpu_bbts* b, int stream, uint32_t* mask8) {
    if (!b || !mask8) return DVBS2GPU_ERR_ARG;
    const BbtsBankView v = bbts_view(b);
    BbtsMa* m = *v.ma;
    if (!m || stream < 0 || stream >= v.nstreams) return DVBS2GPU_ERR_ARG;
    MaStreamState ss;
    if (v.ctx) {
        HIP_TRY(hipSetDevice(v.ctx->device));
        HIP_TRY(hipMemcpy(&ss, m->d_strm[m->cur] + stream, sizeof(ss), hipMemcpyDeviceToHost));
    } else {
        ss = m->host->ss;
    }
    for (int k = 0; k < 8; ++k) mask8[k] = ss.seen[k];
    return 0;
}

}  // extern "C"
