// Device routines of GSE decapsulation that the reference-mode kernels (bbts_gse.hip) and the mode-adaptation ones (bbts_ma.hip)
// share: the walk of one frame's packet chain (gse_walk_frame, over gse_parse_packet of bbts_rules.h), the CRC-32 of a fragment's
// span, what one packet record does to a reassembly context (gse_apply_packet: the device's statement of the reassembly rule;
// GseHostCtx::apply of bbts_host.h is the host's), and the byte movement of the move / append launches.  What differs -- which
// frames are walked and under which rule set, capacity -- stays with each mode.
#pragma once
#include "bbts_common.h"

#ifdef __HIPCC__
namespace s2 {

// CRC-32 of every fragment's span from a zero register: a wave per packet, 64-byte chunks counted from the END of the
// span per lane, each moved to the end of the span by x^(8 * 64 m), XOR-reduced over the wave.  rd(i): byte i of the stream's input.
// 256 threads; rec / span_at / span_len are the workgroup's LDS tables of the frame's n packets.
template <typename Rd>
__device__ inline void gse_span_crcs(GsePkt* rec, const int* span_at, const int* span_len, int n, Rd rd, int tid) {
    const int wave = tid >> 6, lane = tid & 63;
    for (int k = wave; k < n; k += 4) {
        const int kind = (rec[k].w1 >> 24) & 3;
        if (kind == GSE_COMPLETE) continue;
        const int sa = span_at[k], sl = span_len[k];
        uint32_t acc = 0;
        for (int m = lane; m * 64 < sl; m += 64) {
            const int hi = sl - 64 * m, lo = hi > 64 ? hi - 64 : 0;
            uint32_t c = 0;
            for (int i = lo; i < hi; ++i) c = crc32m_byte(c, rd(sa + i));
            acc ^= crc32m_mulmod(c, crc32m_xpow(64u * m));
        }
        for (int d = 32; d > 0; d >>= 1) acc ^= __shfl_xor(acc, d, 64);
        if (lane == 0) {
            const uint32_t xp = crc32m_xpow((uint32_t)sl);
            if (kind == GSE_START) {
                rec[k].a = crc32m_mulmod(0xffffffffu, xp) ^ acc;
            } else if (kind == GSE_MIDDLE) {
                rec[k].a = acc; rec[k].b = xp;
            } else {
                const int e = (int)rec[k].src + (int)(rec[k].w1 & 0xffff);
                const uint32_t rx = rd(e - 4) << 24 | rd(e - 3) << 16 | rd(e - 2) << 8 | rd(e - 1);
                rec[k].a = acc ^ rx; rec[k].b = xp;
            }
        }
    }
}

// One frame's packets, by a workgroup of 256 threads.  Bytes [lo, lo + len) of the stream's input `bb` are staged in `stage`; lane 0
// asks the kernel's prologue `where()` what to walk, follows the chain (next = at + what gse_parse_packet returns: the only serial
// dependency) and fills one record and one CRC span per packet; `done(n, why)` puts the kernel's own frame record into LDS, *npkt
// included (why: what ended the walk; GSE_OVER: more than GSE_PKT_CAP packets); the waves compute the spans' CRCs and the n records
// go to `out`.  Offsets count from the start of the stream's input.  Only a reference packet can leave the staged bytes.
enum { GSE_OVER = -3 };
struct GseWalkRange { int at, end, limit; };      // at >= end: nothing to walk
template <typename Rules, typename Where, typename Done>
__device__ __forceinline__ void gse_walk_frame(const uint8_t* __restrict__ bb, int lo, int len, uint8_t* stage, GsePkt* rec, int* span_at,
                                               int* span_len, Where where, Done done, const int* npkt, GsePkt* __restrict__ out, int tid) {
    const uint8_t* src = bb + lo;
    if ((reinterpret_cast<uintptr_t>(src) & 3) == 0) {
        for (int i = tid; i < len / 4; i += 256) reinterpret_cast<uint32_t*>(stage)[i] = reinterpret_cast<const uint32_t*>(src)[i];
        for (int i = (len & ~3) + tid; i < len; i += 256) stage[i] = src[i];
    } else {
        for (int i = tid; i < len; i += 256) stage[i] = src[i];
    }
    __syncthreads();
    auto rd = [&](int i) -> unsigned {
        const bool staged = !Rules::reference || (i >= lo && i < lo + len);
        unsigned v = stage[staged ? i - lo : 0];
        if (!staged) v = bb[i];
        return v;
    };
    if (tid == 0) {
        const GseWalkRange w = where();
        int at = w.at, n = 0, why = GSE_PADDING;
        while (at < w.end) {
            GsePktHdr p;
            const int took = gse_parse_packet<Rules>(rd, at, w.limit, &p);
            if (took <= 0) { why = took; break; }
            if (n == GSE_PKT_CAP) { why = GSE_OVER; break; }
            rec[n] = {(uint32_t)p.body, (uint32_t)p.plen | (uint32_t)p.id << 16 | (uint32_t)p.kind << 24 | (uint32_t)(p.label ? 1 : 0) << 26, 0, p.proto};
            span_at[n] = p.span_at; span_len[n] = p.span_len;
            ++n;
            at += took;
        }
        done(n, why);
    }
    __syncthreads();
    const int n = *npkt;
    gse_span_crcs(rec, span_at, span_len, n, rd, tid);
    __syncthreads();
    for (int k = tid; k < n; k += 256) out[k] = rec[k];
}

// One packet record (pk[idx], as the frame pass left it) applied to a reassembly context: slot choice (three slots, first fit; a
// START takes a free slot or the one that holds its frag id), fill, the running CRC as crc' = crc * xpow ^ crc0, the END verdict, the
// PDU's output offset and table row, the counters.  The record is rewritten for the move / append launches (bbts_common.h, GsePkt).
// `w` is the write position in the context's output.  Returns false, with nothing changed, when a PDU does not fit into cap.
// store: this lane writes records and rows (every lane of a wave may run the routine on the same context).
__device__ __forceinline__ bool gse_apply_packet(GseDevState& gs, GseStreamOut& so, int& w, int cap, GsePkt* __restrict__ pk, int idx,
                                                 dvbs2gpu_gse_pdu* __restrict__ row, bool store) {
    const GsePkt p = pk[idx];
    const int plen = p.w1 & 0xffff, id = (p.w1 >> 16) & 0xff, kind = (p.w1 >> 24) & 3, label = (p.w1 >> 26) & 1;
    auto rec = [&](uint32_t a, uint32_t b, bool with_b) { if (store) { pk[idx].a = a; if (with_b) pk[idx].b = b; } };
    auto add_row = [&](int total, unsigned proto, int flags) {
        if (store) row[so.nrows] = {(uint32_t)w, (uint32_t)total, (uint16_t)proto, (uint16_t)flags, 0};
        ++so.nrows;
    };
    if (kind == GSE_COMPLETE) {
        const unsigned proto = p.b;
        const int total = 2 + ((proto == 0x0800 || proto == 0x86DD) ? 2 : 0) + plen;
        if (w + total > cap) return false;
        ++gs.cnt.packets;
        add_row(total, proto, label ? 2 : 0);
        rec((uint32_t)w, 0, false);
        w += total;
        ++gs.cnt.complete_pdus; gs.cnt.bytes_delivered += total;
        return true;
    }
    int r = -1;
#pragma unroll
    for (int q = 2; q >= 0; --q) {
        const GseSlot& sq = gs.slot[q];
        if (kind == GSE_START ? (!sq.busy || sq.frag_id == id) : (sq.busy && sq.frag_id == id)) r = q;
    }
    if (r < 0) {
        ++gs.cnt.packets;
        if (kind == GSE_START) ++gs.cnt.dropped_no_slot;
        rec(0xffffffffu, 0, false);
        return true;
    }
    // the slot and its chain end in registers (selected, not indexed: indexing would put the state into scratch)
    GseSlot sl = r == 0 ? gs.slot[0] : r == 1 ? gs.slot[1] : gs.slot[2];
    int ol = r == 0 ? so.open_last[0] : r == 1 ? so.open_last[1] : so.open_last[2];
    auto put = [&]() {
        if (r == 0) { gs.slot[0] = sl; so.open_last[0] = ol; }
        else if (r == 1) { gs.slot[1] = sl; so.open_last[1] = ol; }
        else { gs.slot[2] = sl; so.open_last[2] = ol; }
    };
    const int link = ol >= 0 ? ol : -(1 + r);
    if (kind == GSE_START) {
        sl.busy = 1; sl.frag_id = id; sl.proto = p.b; sl.fill = plen; sl.crc = p.a; sl.label = label;
        rec(0, (uint32_t)(-(1 + r)), true);
        ol = idx;
    } else if (sl.fill + plen > GSE_SLOT_BYTES) {
        sl.busy = 0; ol = -1;
        ++gs.cnt.dropped_overflow;
        rec(0xffffffffu, 0, false);
    } else if (kind == GSE_MIDDLE) {
        sl.crc = crc32m_mulmod(sl.crc, p.b) ^ p.a;
        rec((uint32_t)sl.fill, (uint32_t)link, true);
        sl.fill += plen;
        ol = idx;
    } else {
        const int len = sl.fill + plen - 4;
        const int crc_err = crc32m_mulmod(sl.crc, p.b) != p.a;
        const int total = 2 + ((sl.proto == 0x0800 || sl.proto == 0x86DD) ? 2 : 0) + len;
        if (!crc_err && len >= 0 && w + total > cap) return false;
        sl.busy = 0; ol = -1;
        gs.crc_err = crc_err;
        if (crc_err) {
            ++gs.cnt.crc_failures;
            rec(0xffffffffu, 0, false);
        } else if (len < 0) {
            ++gs.cnt.dropped_no_fit;
            rec(0xffffffffu, 0, false);
        } else {
            rec((uint32_t)so.nrows, (uint32_t)link, true);
            add_row(total, sl.proto, 1 | (sl.label ? 2 : 0));
            w += total;
            ++gs.cnt.reassembled_pdus; gs.cnt.bytes_delivered += total;
        }
    }
    ++gs.cnt.packets;
    put();
    return true;
}

// ------------------------------------------------------------------------------------------------------------- byte movement
// dword stores where the destination allows, the source read unaligned
// (t of nt threads take part)
__device__ inline void gse_copy(uint8_t* __restrict__ dst, const uint8_t* __restrict__ src, int n, int t, int nt) {
    typedef unsigned __attribute__((aligned(1))) unaligned_u32;
    if (n <= 0) return;
    int head = (int)((4 - (reinterpret_cast<uintptr_t>(dst) & 3)) & 3);
    if (head > n) head = n;
    const int words = (n - head) / 4;
    for (int i = t; i < head; i += nt) dst[i] = src[i];
    for (int i = t; i < words; i += nt)
        reinterpret_cast<unsigned*>(dst + head)[i] = *reinterpret_cast<const unaligned_u32*>(src + head + 4 * i);
    for (int i = head + 4 * words + t; i < n; i += nt) dst[i] = src[i];
}

__device__ inline int gse_gre_header(uint8_t* o, unsigned proto, int t) {
    const bool known = proto == 0x0800 || proto == 0x86DD;
    if (t == 0) {
        o[0] = 0; o[1] = 0;                    // GRE: no checksum, no key, no sequence number, version 0
        if (known) { o[2] = (uint8_t)(proto >> 8); o[3] = (uint8_t)proto; }
    }
    return known ? 4 : 2;
}

// The GRE packets of frame f of one context, a wave per packet (256 threads): complete PDUs, and PDUs that END in the frame, gathered
// from their fragments in the input by walking the links backwards and, for what earlier calls brought, from the slot buffers.
// pk: the records of the context's stream ([frame][GSE_PKT_CAP]); row: the context's table; slots: its three buffers.
__device__ inline void gse_move_packets(const uint8_t* __restrict__ bb, uint8_t* __restrict__ out, const GsePkt* __restrict__ pk,
                                        const dvbs2gpu_gse_pdu* __restrict__ row, int f, int npkt, const uint8_t* __restrict__ slots) {
    const int lane = threadIdx.x & 63;
    for (int k = threadIdx.x >> 6; k < npkt; k += 4) {
        const GsePkt p = pk[f * GSE_PKT_CAP + k];
        if (p.a == 0xffffffffu) continue;
        const int plen = p.w1 & 0xffff, kind = (p.w1 >> 24) & 3;
        if (kind == GSE_COMPLETE) {
            uint8_t* o = out + p.a;
            const int hl = gse_gre_header(o, p.b, lane);
            gse_copy(o + hl, bb + p.src, plen, lane, 64);
        } else if (kind == GSE_END) {
            const dvbs2gpu_gse_pdu r = row[p.a];
            uint8_t* o = out + r.offset;
            const int hl = gse_gre_header(o, r.protocol, lane);
            const int len = (int)r.bytes - hl;
            o += hl;
            GsePkt q = p;
            int off = len - (plen - 4);           // where this fragment starts in the PDU; the PDU is the first `len` bytes
            for (;;) {
                const int n = (int)(q.w1 & 0xffff);
                gse_copy(o + off, bb + q.src, (off + n > len ? len - off : n), lane, 64);
                const int link = (int)q.b;
                if (link < 0) {
                    gse_copy(o, slots + (size_t)(-1 - link) * GSE_SLOT_BYTES, off < len ? off : len, lane, 64);
                    break;
                }
                q = pk[link];
                off = (int)q.a;
            }
        }
    }
}

// the fragments of a PDU still open, from the last one (`at`) backwards, into its slot buffer (256 threads)
__device__ inline void gse_append_chain(const uint8_t* __restrict__ bb, const GsePkt* __restrict__ pk, int at, uint8_t* __restrict__ buf) {
    while (at >= 0) {
        const GsePkt q = pk[at];
        gse_copy(buf + q.a, bb + q.src, (int)(q.w1 & 0xffff), threadIdx.x, 256);      // fill + length <= 64 KiB by the overflow rule
        at = (int)q.b;
    }
}

}  // namespace s2
#endif
