// Shared by the BBFRAME -> TS / GSE translation units (bbts.hip: the reference's parser; bbts_ma.hip: the mode-adaptation mode;
// bbts_gse.hip: GSE decapsulation on the device): the reference-mode state and descriptors, the movement of a reassembly context
// between HBM and the host, and the bank's fields the other units need.  The rules themselves are in bbts_rules.h (HIP-free).
#pragma once
#include "ctx.h"
#include "bbts_host.h"

struct dvbs2gpu_bbts;

namespace s2 {

// ------------------------------------------------------------------ reference-mode state and TS descriptors (bbts.hip, bbts_gse.hip)
constexpr int REASM_STRIDE = 192;

struct BbtsDevState {              // per stream, device resident
    int synched, count;
    int hdr[11];                   // ts_gs, sis_mis, ccm_acm, issyi, npd, ro, isi, upl, dfl, sync, syncd (BBHeader, bbframe_ts_parser.h:37-66)
    int last_cnt, last_proc, pad;
};
struct BbtsFrameDesc {
    int src, npk, pre_len, pre_src, out_off, pad[3];   // pre_src < 0: the carried partial lives in the state buffer
};
struct BbtsStreamPlan {
    int needs_host, out_bytes, fin_len, fin_src;       // fin_src < 0: keep the state buffer's bytes
};
// needs_host: 0 the device finished the stream's call; GSE_SEEN the plan kernel met a GSE frame; the per-stream GSE pass
// turns GSE_SEEN into 0 or into one of the two allowed fallbacks
enum { GSE_SEEN = 1, GSE_FALLBACK_RECORDS = 2, GSE_FALLBACK_CAPACITY = 3 };

#ifdef __HIPCC__
// the packets of one TS frame: 0x47 + 187 bytes each, the first completed from the carried partial (`old` or the input)
__device__ inline void bbts_emit_frame(const uint8_t* __restrict__ bb, const uint8_t* __restrict__ old, const BbtsFrameDesc& e,
                                       uint8_t* __restrict__ o) {
    const uint8_t* pre = e.pre_src < 0 ? old : bb + e.pre_src;
    const uint8_t* src = bb + e.src - e.pre_len;          // virtual stream = partial ++ data field
    auto fetch = [&](int i) -> unsigned {                  // output byte i of this frame's packets
        const int b = i % TS;
        if (b == 0) return 0x47u;                          // TS_SYNC_BYTE in place of the CRC-8 of the previous packet
        const int u = i - 1;                               // packet p is bytes [188 p, 188 p + 187) of the virtual stream; its
        return u < e.pre_len ? pre[u] : src[u];            // 188th byte (the CRC-8 of this packet) is dropped
    };
    const int nbytes = e.npk * TS;
    if ((reinterpret_cast<uintptr_t>(o) & 3) == 0) {
        // 188 = 4 * 47: an output dword never straddles two packets, and its four source bytes are contiguous (one unaligned
        // dword load at src + i - 1; the byte under a packet's sync position is replaced)
        typedef unsigned __attribute__((aligned(1))) unaligned_u32;
        for (int w = threadIdx.x; w < nbytes / 4; w += blockDim.x) {
            const int i = 4 * w;
            unsigned v;
            if (i - 1 >= e.pre_len) {
                v = *reinterpret_cast<const unaligned_u32*>(src + i - 1);
                if (i % TS == 0) v = (v & ~0xffu) | 0x47u;
            } else {
                v = fetch(i) | fetch(i + 1) << 8 | fetch(i + 2) << 16 | fetch(i + 3) << 24;
            }
            reinterpret_cast<unsigned*>(o)[w] = v;
        }
    } else {
        for (int i = threadIdx.x; i < nbytes; i += blockDim.x) o[i] = (uint8_t)fetch(i);
    }
}
#endif

// ------------------------------------------------------------------ GSE on the device (bbts_gse.hip)
struct GseFrameRec { int kind, resync, pos, npkt; };   // kind: 0 header rejected, 1 skipped, 2 GSE parsed, 3 TS, 4 GSE with too many packets
struct GseStreamOut { int open_last[3]; int nrows; int ran, pad[3]; };   // ran: the stream pass finished this stream's call

struct BbtsGse;                                 // bbts_gse.hip: the device storage of a bank that has seen a GSE frame
int bbts_gse_create(int nstreams, int max_frames, BbtsGse** out);
void bbts_gse_free(BbtsGse* g);
int bbts_gse_reset(BbtsGse* g);
// enqueues the four GSE launches of one call behind the plan / emit kernels
int bbts_gse_launch(BbtsGse* g, hipStream_t st, const uint8_t* const* d_in, uint8_t* const* d_out, const int* d_nframes, int* d_out_bytes,
                    int fbytes, int max_dfl, int cap, BbtsDevState* d_state, BbtsFrameDesc* d_desc, BbtsStreamPlan* d_plan, uint8_t* d_partial);
GseDevState* bbts_gse_state(BbtsGse* g);
uint8_t* bbts_gse_slot_data(BbtsGse* g, int stream, int slot);
GseStreamOut* bbts_gse_stream_out(BbtsGse* g);
void* bbts_gse_rows(BbtsGse* g, int stream);   // dvbs2gpu_gse_pdu[max_frames * GSE_PKT_CAP]

// One reassembly context between HBM and the host: its GseDevState and the first `fill` bytes of each busy slot.  d_slots: the context's
// three buffers (null: it has none yet, so nothing is open).  This is how a host parser runs a call in place of the kernels.
inline int gse_ctx_to_host(GseHostCtx& c, const GseDevState* d_state, const uint8_t* d_slots) {
    HIP_TRY(hipMemcpy(&c.g, d_state, sizeof(c.g), hipMemcpyDeviceToHost));
    for (int q = 0; q < 3; ++q) {
        const GseSlot& sl = c.g.slot[q];
        c.data[q].assign(sl.busy && sl.fill > 0 ? sl.fill : 0, 0);
        if (!c.data[q].empty() && d_slots) HIP_TRY(hipMemcpy(c.data[q].data(), d_slots + (size_t)q * GSE_SLOT_BYTES, sl.fill, hipMemcpyDeviceToHost));
    }
    return 0;
}
inline int gse_ctx_to_device(const GseHostCtx& c, GseDevState* d_state, uint8_t* d_slots) {
    for (int q = 0; q < 3; ++q) {
        const std::vector<uint8_t>& d = c.data[q];
        if (c.g.slot[q].busy && !d.empty() && d_slots) HIP_TRY(hipMemcpy(d_slots + (size_t)q * GSE_SLOT_BYTES, d.data(), d.size(), hipMemcpyHostToDevice));
    }
    HIP_TRY(hipMemcpy(d_state, &c.g, sizeof(c.g), hipMemcpyHostToDevice));
    return 0;
}
struct BbtsMa;                                  // bbts_ma.hip
void bbts_ma_free(BbtsMa* m);
struct BbtsBankView {
    dvbs2gpu_ctx* ctx;                          // null: a host-only bank (dvbs2gpu_bbts_create_host)
    int nstreams, kbch, max_frames;
    BbtsMa** ma;
};
BbtsBankView bbts_view(dvbs2gpu_bbts* b);
dvbs2gpu_bbts* bbts_new_host_bank(int kbch_bits, int max_frames);
int bbts_reset_reference_state(dvbs2gpu_bbts* b);   // what a freshly created bank's reference-mode parser starts from

}  // namespace s2
