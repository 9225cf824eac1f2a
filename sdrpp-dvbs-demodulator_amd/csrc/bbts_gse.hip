// GSE decapsulation on the device for the BBFRAME -> TS / GSE parser bank: the rules of BbtsHostParser (bbts_host.h;
// dsp::dvbs2::BBFrameTSParser::work, dvbs2/bbframe_ts_parser.cpp:104-390) split into four kernels.  The packet header is read by
// gse_parse_packet<GseReference> (bbts_rules.h), the chain walked by gse_walk_frame and the reassembly rule stated by gse_apply_packet
// (bbts_gse_dev.h); this file has the frame selection, synchronisation, TS descriptors and capacity rules of the reference mode.
//   gse_scan_kernel     one workgroup per (frame, stream): header check, the frame staged in LDS, one lane follows the packet chain
//                       and writes one 16-byte record per packet; the waves then compute, per fragment, the CRC-32 of its span
//                       from a zero register and x^(8 len) mod P, 64-byte chunks per lane;
//   gse_stream_kernel   one lane per stream, over the frame and packet records only: synchronisation, TS descriptors, slot choice and
//                       fill, the running CRC as crc' = crc * xpow ^ crc0, the END verdict, every output offset, the PDU table rows,
//                       the capacity rules.  State is kept in registers and stored only when the call needs no fallback;
//   gse_move_kernel     one workgroup per (frame, stream): TS packets, complete PDUs, and PDUs that END in this frame, gathered
//                       from their fragments in the input and, for what earlier calls brought, from the slot buffer;
//   gse_append_kernel   one workgroup per (slot, stream): fragments of PDUs still open go to the slot buffers; one more
//                       workgroup per stream stores the carried TS partial.
// The slot buffers are only READ by gse_move_kernel and only WRITTEN by gse_append_kernel, a later launch on the same stream:
// a slot restarted within the call is written at offset 0 after the PDU that ended in it has been gathered.
#include "ctx.h"
#include "bbts_common.h"
#include "bbts_gse_dev.h"

using namespace s2;

namespace s2 {

struct BbtsGse {
    int nstreams = 0, max_frames = 0;
    DevBuf<GseDevState> d_state;
    DevBuf<GseFrameRec> d_frec;             // [stream][max_frames]
    DevBuf<GsePkt> d_pkt;                   // [stream][max_frames][GSE_PKT_CAP]
    DevBuf<dvbs2gpu_gse_pdu> d_rows;        // [stream][max_frames * GSE_PKT_CAP]
    DevBuf<GseStreamOut> d_sout;
    DevBuf<uint8_t> d_slots;                // [stream][3][GSE_SLOT_BYTES]
};

// ---------------------------------------------------------------------------------------------------------------- frame pass
__global__ void __launch_bounds__(256) gse_scan_kernel(const uint8_t* const* __restrict__ in, const int* __restrict__ nframes, int fbytes, int max_dfl,
                                                       int max_frames, const BbtsDevState* __restrict__ state,
                                                       const BbtsStreamPlan* __restrict__ plan, GseFrameRec* __restrict__ frec,
                                                       GsePkt* __restrict__ pkts) {
    const int s = blockIdx.y, f = blockIdx.x, tid = threadIdx.x;
    if (plan[s].needs_host != GSE_SEEN || f >= nframes[s]) return;
    __shared__ __attribute__((aligned(16))) uint8_t stage[8192];
    __shared__ GsePkt rec[GSE_PKT_CAP];
    __shared__ int span_at[GSE_PKT_CAP], span_len[GSE_PKT_CAP];
    __shared__ GseFrameRec fr;
    const uint8_t* bb = in[s];
    const int base = f * fbytes, in_end = nframes[s] * fbytes;
    auto prologue = [&]() -> GseWalkRange {       // header check and resynchronisation; a GSE frame is walked from fr.pos for DFL/8 bytes
        fr = {0, 0, 0, 0};
        HeaderFields h, hp;
        if (!header_ok(stage, max_dfl, &h)) return {0, 0, 0};
        const bool synched = f == 0 ? state[s].synched != 0 : header_ok(bb + base - fbytes, max_dfl, &hp);
        const int pos = base + 10 + (synched ? 0 : h.v[10] / 8 + 1);
        fr.resync = !synched; fr.pos = pos;
        fr.kind = h.v[0] == 3 ? 3 : 1;
        if (h.v[0] != 1 || h.v[3] || h.v[4] || h.v[7] != 0) return {0, 0, 0};
        fr.kind = 2;
        return {pos, pos + h.v[8] / 8, in_end};
    };
    gse_walk_frame<GseReference>(bb, base, fbytes, stage, rec, span_at, span_len, prologue,
                                 [&](int n, int why) { fr.npkt = n; if (why == GSE_OVER) fr.kind = 4; }, &fr.npkt,
                                 pkts + ((size_t)s * max_frames + f) * GSE_PKT_CAP, tid);
    if (tid == 0) frec[(size_t)s * max_frames + f] = fr;
}

// --------------------------------------------------------------------------------------------------------------- stream pass
__global__ void __launch_bounds__(64) gse_stream_kernel(const uint8_t* const* __restrict__ in, const int* __restrict__ nframes, int nstreams, int fbytes,
                                                        int max_frames, int cap, BbtsDevState* __restrict__ state, GseDevState* __restrict__ gstate,
                                                        const GseFrameRec* __restrict__ frec, GsePkt* __restrict__ pkts,
                                                        BbtsFrameDesc* __restrict__ desc, BbtsStreamPlan* __restrict__ plan,
                                                        dvbs2gpu_gse_pdu* __restrict__ rows, GseStreamOut* __restrict__ sout,
                                                        int* __restrict__ out_bytes) {
    const int s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= nstreams) return;
    GseStreamOut so = {{-1, -1, -1}, 0, 0, {0, 0, 0}};
    if (plan[s].needs_host != GSE_SEEN) { sout[s] = so; return; }
    BbtsDevState st = state[s];
    GseDevState gs = gstate[s];
    const uint8_t* bb = in[s];
    const int nf = nframes[s];
    BbtsFrameDesc* d = desc + (size_t)s * max_frames;
    GsePkt* pk = pkts + (size_t)s * max_frames * GSE_PKT_CAP;
    dvbs2gpu_gse_pdu* row = rows + (size_t)s * max_frames * GSE_PKT_CAP;
    int synched = st.synched, pre_len = st.count, pre_src = -1, w = 0, proc = 0, last_good = -1, fallback = 0;
    for (int f = 0; f < nf && !fallback; ++f) {
        BbtsFrameDesc e = {0, 0, 0, -1, 0, {0, 0, 0}};
        const GseFrameRec fr = frec[(size_t)s * max_frames + f];
        if (fr.kind == 0) { synched = 0; d[f] = e; continue; }
        if (fr.resync) pre_len = 0;
        synched = 1;
        last_good = f;
        ++proc;
        if (fr.kind == 4) { fallback = GSE_FALLBACK_RECORDS; break; }
        if (fr.kind == 3) {
            const int pos = fr.pos;
            const int df = (bb[f * fbytes + 4] << 8 | bb[f * fbytes + 5]) / 8 - (pos - (f * fbytes + 10));
            if (df >= TS) {
                const int d1 = pre_len > 0 ? df - (TS - pre_len) : df;
                const int n = (pre_len > 0 ? 1 : 0) + d1 / TS, rem = d1 % TS;
                e.src = pos; e.npk = n; e.pre_len = pre_len; e.pre_src = pre_src; e.out_off = w;
                w += n * TS;
                pre_len = rem; pre_src = pos + df - rem;
            } else if (df > 0) {
                pre_len = df; pre_src = pos;
            }
            // the host parser's loop wants more than 188 bytes free before every packet and stops the call when no more than
            // 188 are left after a TS frame (.cpp:178,206): both are seen from the sizes
            if (cap - w <= TS) { fallback = GSE_FALLBACK_CAPACITY; break; }
        } else if (fr.kind == 2) {
            ++gs.cnt.frames;
            for (int k = 0; k < fr.npkt && !fallback; ++k) {
                const int idx = f * GSE_PKT_CAP + k;
                if (!gse_apply_packet(gs, so, w, cap, pk, idx, row, true)) fallback = GSE_FALLBACK_CAPACITY;
            }
        }
        d[f] = e;
    }
    BbtsStreamPlan p;
    if (fallback) {
        // nothing of this call is kept: the host parser runs it again from the state as it was
        for (int f = 0; f < nf; ++f) d[f].npk = 0;
        so = {{-1, -1, -1}, 0, 0, {0, 0, 0}};
        p.needs_host = fallback; p.out_bytes = 0; p.fin_len = 0; p.fin_src = -1;
    } else {
        if (last_good >= 0) {
            const HeaderFields h = parse_bbheader(bb + last_good * fbytes);
            for (int k = 0; k < 11; ++k) st.hdr[k] = h.v[k];
        }
        st.synched = synched; st.count = pre_len; st.last_cnt = nf; st.last_proc = proc;
        state[s] = st;
#pragma unroll
        for (int q = 0; q < 3; ++q) if (!gs.slot[q].busy) so.open_last[q] = -1;
        gstate[s] = gs;
        so.ran = 1;
        p.needs_host = 0; p.out_bytes = w; p.fin_len = pre_src < 0 ? 0 : pre_len; p.fin_src = pre_src;
    }
    plan[s] = p;
    sout[s] = so;
    out_bytes[s] = p.out_bytes;
}

// ------------------------------------------------------------------------------------------------------------- byte movement
__global__ void __launch_bounds__(256) gse_move_kernel(const uint8_t* const* __restrict__ in, uint8_t* const* __restrict__ out,
                                                       const int* __restrict__ nframes, int max_frames, const BbtsFrameDesc* __restrict__ desc,
                                                       const BbtsStreamPlan* __restrict__ plan, const GseFrameRec* __restrict__ frec,
                                                       const GsePkt* __restrict__ pkts, const dvbs2gpu_gse_pdu* __restrict__ rows,
                                                       const GseStreamOut* __restrict__ sout, const uint8_t* __restrict__ partial,
                                                       const uint8_t* __restrict__ slots) {
    const int s = blockIdx.y, f = blockIdx.x;
    // streams the stream pass did not finish have no rows and no TS descriptors; streams without GSE were emitted before
    if (f >= nframes[s] || !sout[s].ran) return;
    const GseFrameRec fr = frec[(size_t)s * max_frames + f];
    const uint8_t* bb = in[s];
    if (fr.kind == 3) {
        const BbtsFrameDesc e = desc[(size_t)s * max_frames + f];
        if (e.npk > 0) bbts_emit_frame(bb, partial + (size_t)s * REASM_STRIDE, e, out[s] + e.out_off);
        return;
    }
    if (fr.kind != 2) return;
    const GsePkt* pk = pkts + (size_t)s * max_frames * GSE_PKT_CAP;
    const dvbs2gpu_gse_pdu* row = rows + (size_t)s * max_frames * GSE_PKT_CAP;
    gse_move_packets(bb, out[s], pk, row, f, fr.npkt, slots + (size_t)s * 3 * GSE_SLOT_BYTES);
}

__global__ void __launch_bounds__(256) gse_append_kernel(const uint8_t* const* __restrict__ in, const BbtsStreamPlan* __restrict__ plan,
                                                         const GsePkt* __restrict__ pkts, int max_frames, const GseStreamOut* __restrict__ sout,
                                                         uint8_t* __restrict__ partial, uint8_t* __restrict__ slots) {
    const int s = blockIdx.y, r = blockIdx.x;
    const BbtsStreamPlan p = plan[s];
    if (!sout[s].ran) return;
    const uint8_t* bb = in[s];
    if (r == 3) {                                 // the TS partial carried into the next call (streams without GSE: fin_len 0 here)
        if (p.fin_src >= 0) gse_copy(partial + (size_t)s * REASM_STRIDE, bb + p.fin_src, p.fin_len, threadIdx.x, 256);
        return;
    }
    int at = sout[s].open_last[r];
    if (at < 0) return;
    const GsePkt* pk = pkts + (size_t)s * max_frames * GSE_PKT_CAP;
    gse_append_chain(bb, pk, at, slots + ((size_t)s * 3 + r) * GSE_SLOT_BYTES);
}

// -------------------------------------------------------------------------------------------------------------------- host
void bbts_gse_free(BbtsGse* g) { delete g; }

int bbts_gse_create(int nstreams, int max_frames, BbtsGse** out) {
    std::unique_ptr<BbtsGse> g(new BbtsGse());
    g->nstreams = nstreams; g->max_frames = max_frames;
    const size_t n = (size_t)nstreams, np = n * max_frames * GSE_PKT_CAP;
    const char* what = "hipMalloc(bbts gse)";
    RC_TRY(g->d_state.alloc(n, true, what));
    RC_TRY(g->d_frec.alloc(n * max_frames, true, what));
    RC_TRY(g->d_pkt.alloc(np, false, what));
    RC_TRY(g->d_rows.alloc(np, false, what));
    RC_TRY(g->d_sout.alloc(n, true, what));
    RC_TRY(g->d_slots.alloc(n * 3 * GSE_SLOT_BYTES, false, what));
    *out = g.release();
    return 0;
}

int bbts_gse_reset(BbtsGse* g) {
    if (!g) return 0;
    HIP_TRY(hipMemset(g->d_state, 0, (size_t)g->nstreams * sizeof(GseDevState)));
    HIP_TRY(hipMemset(g->d_sout, 0, (size_t)g->nstreams * sizeof(GseStreamOut)));
    return 0;
}

GseDevState* bbts_gse_state(BbtsGse* g) { return g->d_state; }
uint8_t* bbts_gse_slot_data(BbtsGse* g, int stream, int slot) { return g->d_slots + ((size_t)stream * 3 + slot) * GSE_SLOT_BYTES; }
GseStreamOut* bbts_gse_stream_out(BbtsGse* g) { return g->d_sout; }
void* bbts_gse_rows(BbtsGse* g, int stream) { return g->d_rows + (size_t)stream * g->max_frames * GSE_PKT_CAP; }

int bbts_gse_launch(BbtsGse* g, hipStream_t st, const uint8_t* const* d_in, uint8_t* const* d_out, const int* d_nframes, int* d_out_bytes,
                    int fbytes, int max_dfl, int cap, BbtsDevState* d_state, BbtsFrameDesc* d_desc, BbtsStreamPlan* d_plan, uint8_t* d_partial) {
    const int n = g->nstreams, mf = g->max_frames;
    hipLaunchKernelGGL(gse_scan_kernel, dim3(mf, n), dim3(256), 0, st, d_in, d_nframes, fbytes, max_dfl, mf, d_state, d_plan, g->d_frec, g->d_pkt);
    hipLaunchKernelGGL(gse_stream_kernel, dim3((n + 63) / 64), dim3(64), 0, st, d_in, d_nframes, n, fbytes, mf, cap, d_state, g->d_state, g->d_frec,
                       g->d_pkt, d_desc, d_plan, g->d_rows, g->d_sout, d_out_bytes);
    hipLaunchKernelGGL(gse_move_kernel, dim3(mf, n), dim3(256), 0, st, d_in, d_out, d_nframes, mf, d_desc, d_plan, g->d_frec, g->d_pkt, g->d_rows,
                       g->d_sout, d_partial, g->d_slots);
    hipLaunchKernelGGL(gse_append_kernel, dim3(4, n), dim3(256), 0, st, d_in, d_plan, g->d_pkt, mf, g->d_sout, d_partial, g->d_slots);
    HIP_TRY(hipGetLastError());
    return 0;
}

}  // namespace s2
