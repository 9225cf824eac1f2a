// The native host side of the BBFRAME -> TS / GSE bank: GseHostCtx, the one host reassembler (the host twin of gse_apply_packet,
// bbts_gse_dev.h; both modes' host parsers hold contexts of this type), and BbtsHostParser, the reference-mode parser of one stream.
// No HIP: tests/cpp/bbts_host_parser.cpp drives BbtsHostParser on a machine without a GPU.
#pragma once
#include "bbts_rules.h"
#include "../../include/dvbs2gpu.h"

#include <cstring>
#include <vector>

namespace s2 {

struct Crc32mTable { uint32_t v[256]; };
constexpr Crc32mTable crc32m_make_table() {
    Crc32mTable t = {};
    for (unsigned i = 0; i < 256; ++i) t.v[i] = crc32m_byte(0, i);
    return t;
}
inline uint32_t crc32m_span(uint32_t c, const uint8_t* p, int n) {
    static constexpr Crc32mTable t = crc32m_make_table();
    for (int i = 0; i < n; ++i) c = (c << 8) ^ t.v[(c >> 24) ^ p[i]];
    return c;
}

// Where a context's GRE packets go.  room(total, &off): `total` bytes at offset `off` of the output, or null when they do not fit.
struct GseBoundedOut {                            // reference mode: the caller's buffer; what does not fit is dropped
    uint8_t* out; int cap, w;
    uint8_t* room(int total, uint32_t* off) {
        if (w + total > cap) return nullptr;
        *off = (uint32_t)w; w += total;
        return out + *off;
    }
};
struct GseGrowingOut {                            // mode adaptation: sizes first, the caller compares them with its capacity afterwards
    std::vector<uint8_t>& out;
    uint8_t* room(int total, uint32_t* off) {
        *off = (uint32_t)out.size(); out.resize(out.size() + total);
        return out.data() + *off;
    }
};

// One reassembly context on the host: the device's own state (three slots, the last END's verdict, the counters), the bytes of the
// open reassemblies (data[q].size() == slot[q].fill while slot q is busy) and the table rows of the last call.
struct GseHostCtx {
    GseDevState g = {};
    std::vector<uint8_t> data[3];
    std::vector<dvbs2gpu_gse_pdu> rows;

    // a PDU of n bytes as a GRE packet; one that does not fit, or has a negative length, is dropped and counted
    template <typename Sink>
    void deliver(unsigned proto, const uint8_t* p, int n, int flags, Sink& sink) {
        const bool known = proto == 0x0800 || proto == 0x86DD;
        const int total = 2 + (known ? 2 : 0) + n;
        uint32_t off = 0;
        uint8_t* o = n < 0 ? nullptr : sink.room(total, &off);
        if (!o) { ++g.cnt.dropped_no_fit; return; }
        ++((flags & 1) ? g.cnt.reassembled_pdus : g.cnt.complete_pdus);
        g.cnt.bytes_delivered += total;
        rows.push_back({off, (uint32_t)total, (uint16_t)proto, (uint16_t)flags, 0});
        *o++ = 0; *o++ = 0;                    // GRE: no checksum, no key, no sequence number, version 0
        if (known) { *o++ = (uint8_t)(proto >> 8); *o++ = (uint8_t)proto; }
        if (n > 0) memcpy(o, p, n);
    }
    // what one packet does to the context; the packet's offsets count from `in`
    template <typename Sink>
    void apply(const GsePktHdr& p, const uint8_t* in, Sink& sink) {
        const uint8_t* body = in + p.body;
        ++g.cnt.packets;
        if (p.kind == GSE_COMPLETE) { deliver(p.proto, body, p.plen, p.label ? 2 : 0, sink); return; }
        int r = -1;                             // three slots, first fit; a START takes a free slot or the one that holds its frag id
        for (int q = 2; q >= 0; --q) {
            const GseSlot& sq = g.slot[q];
            if (p.kind == GSE_START ? (!sq.busy || sq.frag_id == p.id) : (sq.busy && sq.frag_id == p.id)) r = q;
        }
        if (r < 0) { if (p.kind == GSE_START) ++g.cnt.dropped_no_slot; return; }
        GseSlot& sl = g.slot[r];
        std::vector<uint8_t>& buf = data[r];
        if (p.kind == GSE_START) {
            sl = {1, p.id, p.plen, p.label ? 1 : 0, p.proto, crc32m_span(0xffffffffu, in + p.span_at, p.span_len)};
            buf.assign(body, body + p.plen);
        } else if (sl.fill + p.plen > GSE_SLOT_BYTES) {
            sl.busy = 0; buf.clear();
            ++g.cnt.dropped_overflow;
        } else if (p.kind == GSE_MIDDLE) {
            buf.insert(buf.end(), body, body + p.plen);
            sl.fill += p.plen; sl.crc = crc32m_span(sl.crc, body, p.plen);
        } else {
            const uint8_t* e = body + p.plen;   // the PDU is the first fill + plen - 4 bytes of what the slot holds with this payload
            if (p.plen > 4) buf.insert(buf.end(), body, e - 4);
            const uint32_t rx = (uint32_t)e[-4] << 24 | (uint32_t)e[-3] << 16 | (uint32_t)e[-2] << 8 | e[-1];
            sl.busy = 0;
            g.crc_err = crc32m_span(sl.crc, in + p.span_at, p.span_len) != rx;
            if (g.crc_err) ++g.cnt.crc_failures;
            else deliver(sl.proto, buf.data(), sl.fill + p.plen - 4, 1 | (sl.label ? 2 : 0), sink);
            buf.clear();
        }
    }
    // the packets of one GSE frame from offset `at` up to `end`, with no limit on their number; returns how the walk ended
    // (GSE_PADDING: also at `end`)
    template <typename Rules, typename Sink>
    int frame(const uint8_t* in, int at, int end, int limit, Sink& sink) {
        ++g.cnt.frames;
        while (at < end) {
            GsePktHdr p;
            const int len = gse_parse_packet<Rules>([&](int i) -> unsigned { return in[i]; }, at, limit, &p);
            if (len <= 0) return len;
            apply(p, in, sink);
            at += len;
        }
        return GSE_PADDING;
    }
};

// Full BBFrameTSParser::work semantics for one stream (dsp::dvbs2::BBFrameTSParser::work, dvbs2/bbframe_ts_parser.cpp:104-390).
// Where the reference's behaviour is undefined (reads past the input buffer, writes past the output or the 64 KiB reassembly
// buffers, negative copy lengths) the rules stated in include/dvbs2gpu.h apply.
class BbtsHostParser {
public:
    int synched = 0, count = 0;
    uint8_t partial[TS] = {0};
    int hdr[11] = {0};
    int last_cnt = 0, last_proc = 0;
    GseHostCtx gse;                             // its counters are what dvbs2gpu_bbts_get_gse_stats reports; its rows those of the last run()

    // returns bytes produced or DVBS2GPU_ERR_CAPACITY
    int run(const uint8_t* bb, int cnt, int fbytes, int max_dfl, uint8_t* out, int cap) {
        in_ = bb;
        out_ = {out, cap, 0};
        gse.rows.clear();
        int proc = 0;
        bool stop = false;
        for (int f = 0; f < cnt && !stop; ++f) {
            const int base = fbytes * f;
            HeaderFields h;
            if (!header_ok(bb + base, max_dfl, &h)) { synched = 0; continue; }
            int pos = base + 10;
            int df = h.v[8] / 8;
            if (!synched) {
                const int skip = h.v[10] / 8 + 1;
                pos += skip; df -= skip; count = 0; synched = 1;
            }
            memcpy(hdr, h.v, sizeof(hdr));
            ++proc;
            switch (h.v[0]) {
            case 3: {
                const int rc = ts_frame(pos, df);
                if (rc < 0) { synched = 0; return DVBS2GPU_ERR_CAPACITY; }
                stop = rc > 0;
                break;
            }
            case 1:                             // a resynchronising frame is walked for DFL/8 bytes from its late start
                if (!h.v[3] && !h.v[4] && h.v[7] == 0) gse.frame<GseReference>(bb, pos, pos + h.v[8] / 8, fbytes * cnt, out_);
                break;
            default: break;
            }
        }
        last_cnt = cnt; last_proc = proc;
        return out_.w;
    }

private:
    const uint8_t* in_ = nullptr;
    GseBoundedOut out_ = {nullptr, 0, 0};

    // 1: the output is nearly full, stop after this frame (.cpp:206-209); -1: undefined in the reference; 0 otherwise
    int ts_frame(int pos, int df) {
        int& w = out_.w;
        while (df >= TS && out_.cap - w > TS) {
            uint8_t* o = out_.out + w;
            o[0] = 0x47;
            if (count > 0) {
                const int need = TS - count;
                memcpy(partial + count, in_ + pos, need);
                memcpy(o + 1, partial, TS - 1);
                pos += need; df -= need; count = 0;
            } else {
                memcpy(o + 1, in_ + pos, TS - 1);
                pos += TS; df -= TS;
            }
            w += TS;
        }
        if (df >= TS) return -1;
        if (df > 0) { memcpy(partial, in_ + pos, df); count = df; }
        return out_.cap - w <= TS ? 1 : 0;
    }
};

}  // namespace s2
