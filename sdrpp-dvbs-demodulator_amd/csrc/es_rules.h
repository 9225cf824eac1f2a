// The rules of the ES bank (own extension; include/dvbs2gpu.h), each stated once and shared by the kernel (es.hip),
// the native host bank (EsHostStream below, behind dvbs2gpu_es_create_host) and a plain C++ test program: which bytes of a watched
// video PID are elementary-stream bytes (es_packet_plan: the packet's reset, its PES start and its segment), the start-code scanner
// over them (es_scan_byte: a code is a pure function of the last 8 ES bytes), what a code means in MPEG-2, H.264 and H.265 video
// (es_classify) and what a row adds to its slot's counters.  The PES start itself is pes_start() of pes_rules.h, not restated here.
//
// The sequential form -- EsHostStream::run, packet by packet and byte by byte -- IS the definition; every other form must give its
// rows, counters and state for every cut of a stream into calls.  Its packet walk (EsHostWalk) and the twelve counters in front of
// the bank's own (EsStreamCnt) are stated here for the audio bank too (aud_rules.h).  Start-code and header syntax as remembered from
// ISO/IEC 13818-1, 13818-2, 14496-10 and 23008-2; pinned to no vector of theirs.
// Standard headers only: the host tests compile this file with a plain C++ compiler.
#pragma once
#include "pes_rules.h"

#define ES_HD PES_HD

namespace s2 {

constexpr int ES_SLOTS = PES_SLOTS;
enum EsCodec { ES_NONE = 0, ES_MPEG2 = 1, ES_H264 = 2, ES_H265 = 3 };
// a row's unit; behind them what a code without a row is counted as
enum EsUnit { ES_PES = 0, ES_PICTURE = 1, ES_SEQUENCE = 2, ES_GOP = 3, ES_PARAM = 4, ES_AUD = 5, ES_END = 6, ES_UNITS = 7, ES_SLICE = 7, ES_OTHER = 8, ES_BAD = 9 };
enum EsPicture { ES_PIC_NONE = 0, ES_PIC_I = 1, ES_PIC_P = 2, ES_PIC_B = 3 };
// row flags (DVBS2GPU_ES_*)
constexpr int ES_KEY = 1, ES_RESYNC = 2, ES_UNSYNCED = 4, ES_SPLIT_HEADER = 8;
constexpr int ES_WINDOW = 8;                                // ES bytes that decide a code: 00 00 01, the code byte, four head bytes
constexpr uint64_t ES_TAIL_MASK = (1ull << 56) - 1;

#pragma pack(push, 4)
struct EsRow {                                              // the layout of dvbs2gpu_es_row: 48 bytes, es_offset at 16
    uint16_t pid; uint8_t slot, unit, code, detail; uint16_t flags;
    int32_t packet; uint32_t head;
    uint64_t es_offset, pts, dts, reserved;
};
#pragma pack(pop)

// what a code means: unit (ES_PICTURE .. ES_END: a row; ES_SLICE, ES_OTHER, ES_BAD: counted only), the picture type and KEY
struct EsCode { uint32_t unit, detail, key; };

// slice_type of an H.264 slice header whose first_mb_in_slice is 0: the ue(v) in the 7 bits x behind the first bit
ES_HD inline uint32_t es_h264_slice_picture(uint32_t x) {
    int z = 0;
    while (z < 4 && !(x >> (6 - z) & 1)) ++z;
    if (z > 3) return ES_PIC_NONE;
    const uint32_t v = (x >> (6 - 2 * z)) - 1;
    if (v > 9) return ES_PIC_NONE;
    const uint32_t m = v % 5;
    return m == 0 ? ES_PIC_P : m == 1 ? ES_PIC_B : m == 2 ? ES_PIC_I : ES_PIC_NONE;
}

ES_HD inline EsCode es_classify(int codec, uint32_t code, uint32_t head) {
    EsCode c = {ES_OTHER, ES_PIC_NONE, 0};
    if (codec == ES_MPEG2) {
        if (code == 0x00) {
            const uint32_t t = head >> 19 & 7;
            c.unit = ES_PICTURE; c.detail = t >= 1 && t <= 3 ? t : 0u; c.key = t == 1;     // (ES_PIC_I, _P, _B are the standard's 1, 2, 3)
        } else if (code == 0xB3) c.unit = ES_SEQUENCE;
        else if (code == 0xB8) c.unit = ES_GOP;
        else if (code == 0xB7) c.unit = ES_END;
        else if (code <= 0xAF) c.unit = ES_SLICE;
    } else if (codec == ES_H264) {
        const uint32_t t = code & 31;
        if (code & 0x80) c.unit = ES_BAD;
        else if (t == 1 || t == 5) {
            if (head >> 31) { c.unit = ES_PICTURE; c.key = t == 5; c.detail = es_h264_slice_picture(head >> 24 & 127); }
            else c.unit = ES_SLICE;
        } else if (t == 7) c.unit = ES_SEQUENCE;
        else if (t == 8) c.unit = ES_PARAM;
        else if (t == 9) c.unit = ES_AUD;
        else if (t == 10 || t == 11) c.unit = ES_END;
    } else if (codec == ES_H265) {
        const uint32_t t = code >> 1 & 63;
        if ((code & 0x80) || (head >> 24 & 7) == 0) c.unit = ES_BAD;
        else if (t <= 9 || (t >= 16 && t <= 21)) {
            if (head >> 23 & 1) { c.unit = ES_PICTURE; c.key = t >= 16; c.detail = t >= 16 ? ES_PIC_I : ES_PIC_NONE; }
            else c.unit = ES_SLICE;
        } else if (t == 33) c.unit = ES_SEQUENCE;
        else if (t == 32 || t == 34) c.unit = ES_PARAM;
        else if (t == 35) c.unit = ES_AUD;
        else if (t == 36 || t == 37) c.unit = ES_END;
    }
    return c;
}

// The scanner: `win` holds the last 8 accepted bytes (the newest in the low byte), `since` the bytes accepted since the last reset.
// One byte in; true: it completes a code (code byte and head in *code, *head), whose first byte lies 7 bytes back
ES_HD inline bool es_scan_byte(uint64_t* win, uint32_t* since, uint32_t byte, uint32_t* code, uint32_t* head) {
    *win = *win << 8 | byte;
    ++*since;
    if (*since < ES_WINDOW || *win >> 40 != 1) return false;
    *code = (uint32_t)(*win >> 32) & 255; *head = (uint32_t)*win;
    return true;
}

// The state of one slot.  tail: the last `have` accepted bytes, the newest in the low byte, the rest 0.  cc: the TS monitor's byte
struct EsState { uint64_t es_count, tail; uint8_t cc, have, synced, lost; uint8_t pad[4]; };

// What a packet with L >= 1 payload bytes does, given only its own bytes and whether its slot is synced in front of it.
// `cont` is "the continuity step said CC_ERROR or DISC".  reset: the scanner is reset in front of the packet's row and segment.
// start: a PES row (hd, row_flags but RESYNC); after it the slot is synced == valid, and an invalid start resets once more.
// seg_off / seg_len: the ES bytes are payload[seg_off .. seg_off + seg_len)
struct EsPlan { bool reset, start, valid; int seg_off, seg_len, unsynced_bytes; uint32_t row_flags; PesHead hd; };
// w: the first min(L, 19) payload bytes as pes_start takes them (not read for a scrambled packet or one without PUSI)
ES_HD inline EsPlan es_packet_plan(const uint32_t* w, int L, int tsc, int pusi, bool cont, bool synced) {
    EsPlan p = {cont || tsc != 0, pusi != 0, false, 0, 0, 0, 0, {PES_SCRAMBLED, 0, 0, 0, PES_NO_TS, PES_NO_TS}};
    if (pusi) {
        p.hd = pes_start(w, L, tsc);
        const int hdl = (int)(w[2] & 255);                  // PES_header_data_length, payload[8]: a HEADER has it
        if (p.hd.kind == PES_HEADER && 9 + hdl <= L) { p.valid = true; p.seg_off = 9 + hdl; p.seg_len = L - 9 - hdl; }
        else p.row_flags = ES_UNSYNCED | (p.hd.kind == PES_HEADER ? ES_SPLIT_HEADER : 0);
    } else if (!tsc) {
        if (synced) p.seg_len = L; else p.unsynced_bytes = L;
    }
    return p;
}

// what one call adds to a slot's statistics.  The twelve counters that every bank over an elementary stream begins with (the ES bank
// here, the audio bank in aud_rules.h), in the order of dvbs2gpu_es_stats and dvbs2gpu_aud_stats
struct EsStreamCnt {
    int32_t packets, payload_bytes, es_bytes, bytes_unsynced, duplicates, cc_errors, scrambled_packets, malformed_packets, resets, pes_starts, pes_invalid,
            split_headers;
};
// behind them the ES bank's own, in the order of dvbs2gpu_es_stats
struct EsCnt : EsStreamCnt {
    int32_t codes, pictures, pictures_i, pictures_p, pictures_b, key_pictures, sequences, gops, params, auds, ends, slices, other_codes, bad_codes;
};
constexpr int ES_STREAM_COUNTERS = 12, ES_COUNTERS = 26;
static_assert(sizeof(EsStreamCnt) == ES_STREAM_COUNTERS * sizeof(int32_t) && sizeof(EsCnt) == ES_COUNTERS * sizeof(int32_t), "counter order");
ES_HD inline EsCnt es_cnt_zero() { return EsCnt{}; }
// a code into its slot's counters (no run-time index: the kernel keeps *c in registers)
ES_HD inline void es_cnt_code(EsCnt* c, const EsCode& e) {
    ++c->codes;
    c->pictures += e.unit == ES_PICTURE; c->sequences += e.unit == ES_SEQUENCE; c->gops += e.unit == ES_GOP; c->params += e.unit == ES_PARAM;
    c->auds += e.unit == ES_AUD; c->ends += e.unit == ES_END; c->slices += e.unit == ES_SLICE; c->other_codes += e.unit == ES_OTHER; c->bad_codes += e.unit == ES_BAD;
    c->pictures_i += e.unit == ES_PICTURE && e.detail == ES_PIC_I; c->pictures_p += e.unit == ES_PICTURE && e.detail == ES_PIC_P;
    c->pictures_b += e.unit == ES_PICTURE && e.detail == ES_PIC_B; c->key_pictures += e.key;
}
// a start into its slot's counters
ES_HD inline void es_cnt_start(EsStreamCnt* c, const EsPlan& p) {
    ++c->pes_starts; c->pes_invalid += !p.valid; c->split_headers += (p.row_flags & ES_SPLIT_HEADER) != 0;
}
ES_HD inline EsRow es_pes_row(int pid, int slot, int k, const EsPlan& p, uint64_t es_count, bool lost) {
    return EsRow{(uint16_t)pid, (uint8_t)slot, ES_PES, (uint8_t)p.hd.stream_id, (uint8_t)p.hd.kind, (uint16_t)(p.row_flags | (lost ? ES_RESYNC : 0)), k, p.hd.declared,
                 es_count, p.hd.pts, p.hd.dts, 0};
}
ES_HD inline EsRow es_code_row(int pid, int slot, int k, const EsCode& e, uint32_t code, uint32_t head, uint64_t es_offset, bool lost) {
    return EsRow{(uint16_t)pid, (uint8_t)slot, (uint8_t)e.unit, (uint8_t)code, (uint8_t)e.detail, (uint16_t)((e.key ? ES_KEY : 0) | (lost ? ES_RESYNC : 0)), k, head,
                 es_offset, PES_NO_TS, PES_NO_TS, 0};
}
// the header of a stream's call record; the slots' counters follow it (EsStreamCall in es_stream.h)
struct EsCallHead { int32_t rows, pad[3]; };

// ------------------------------------------------------------------------------------------------- the sequential definition
// The packet walk of a bank over the elementary streams of watched PIDs, stated once for EsHostStream below and AudHostStream
// (aud_rules.h): everything around what the bank does with a reset, a start and the bytes of a segment.  State has es_count, tail,
// have and cc; Cnt begins with EsStreamCnt.  Self supplies
//   static bool synced(const State&)                 the slot's synced bit in front of the packet
//   static void stream_reset(State&)                 a reset: the window is forgotten, the slot is lost (and what the bank forgets with it)
//   void start(k, s, pl, max_rows)                   a start: its PES row, the synced bit, what a valid start does to the bank's own state
//                                                    (an invalid one is followed by a reset)
//   void segment(k, s, pl, pay, &win, &since, max_rows)   the segment pay[pl.seg_off ..], byte by byte into the window (win, since)
template <typename Self, typename State, typename Cnt, typename Row>
struct EsHostWalk {
    int32_t watch[ES_SLOTS];                                // -1: the slot watches nothing
    int32_t codec[ES_SLOTS];
    State slot[ES_SLOTS];
    int64_t packets = 0;                                    // the position of the next call's first packet
    // of the last call
    std::vector<Row> rows;                                  // the first max_rows
    Cnt cnt[ES_SLOTS];
    EsCallHead head = {0, {0, 0, 0}};

    EsHostWalk() {
        for (int s = 0; s < ES_SLOTS; ++s) { watch[s] = -1; codec[s] = 0; clear_slot(s); cnt[s] = Cnt{}; }
    }
    void clear_slot(int s) { slot[s] = State{}; }
    void reset() {
        for (int s = 0; s < ES_SLOTS; ++s) clear_slot(s);
        packets = 0; rows.clear(); head = {0, {0, 0, 0}};
    }
    void emit(const Row& r, int max_rows) { if (head.rows++ < max_rows) rows.push_back(r); }
    // one call: n packets
    void run(const uint8_t* ts, int n, int max_rows) {
        Self& self = static_cast<Self&>(*this);
        rows.clear();
        head = {0, {0, 0, 0}};
        for (int s = 0; s < ES_SLOTS; ++s) cnt[s] = Cnt{};
        for (int k = 0; k < n; ++k) {
            const uint8_t* p = ts + (size_t)k * TSMON_TS;
            const TsmonHdr h = tsmon_parse(p);
            if (h.cls != TSMON_DATA) continue;
            int s = 0;
            while (s < ES_SLOTS && watch[s] != h.pid) ++s;
            if (s == ES_SLOTS) continue;
            State& st = slot[s];
            Cnt& c = cnt[s];
            ++c.packets;
            const int v = tsmon_step(&st.cc, h.afc, h.cc, h.di);
            if (v == TSMON_DUPLICATE) { ++c.duplicates; continue; }
            c.cc_errors += v == TSMON_CC_ERROR;
            const bool cont = v == TSMON_CC_ERROR || v == TSMON_DISC;
            const int L = pes_payload_len(h.afc, h.afc == 3 ? p[4] : 0);
            if (L <= 0) {
                const bool malformed = L == 0;
                c.malformed_packets += malformed;
                if (cont || malformed) { ++c.resets; Self::stream_reset(st); }
                continue;
            }
            c.payload_bytes += L;
            c.scrambled_packets += h.tsc != 0;
            uint32_t w[5] = {0, 0, 0, 0, 0};
            const uint8_t* pay = p + TSMON_TS - L;
            if (h.pusi && !h.tsc) for (int i = 0; i < L && i < PES_HEAD_BYTES; ++i) w[i >> 2] |= (uint32_t)pay[i] << (8 * (i & 3));
            const EsPlan pl = es_packet_plan(w, L, h.tsc, h.pusi, cont, Self::synced(st));
            if (pl.reset) Self::stream_reset(st);
            if (pl.start) {
                self.start(k, s, pl, max_rows);
                es_cnt_start(&c, pl);
                if (!pl.valid) Self::stream_reset(st);
            }
            c.resets += pl.reset || (pl.start && !pl.valid);
            c.bytes_unsynced += pl.unsynced_bytes;
            c.es_bytes += pl.seg_len;
            uint64_t win = st.tail;
            uint32_t since = st.have;
            self.segment(k, s, pl, pay, &win, &since, max_rows);
            st.es_count += pl.seg_len;
            st.have = (uint8_t)(since < 7 ? since : 7);
            st.tail = st.have == 7 ? win & ES_TAIL_MASK : win & ((1ull << (8 * st.have)) - 1);
        }
        packets += n;
    }
};

struct EsHostStream : EsHostWalk<EsHostStream, EsState, EsCnt, EsRow> {
    static bool synced(const EsState& st) { return st.synced != 0; }
    static void stream_reset(EsState& st) { st.have = 0; st.tail = 0; st.lost = 1; }
    void start(int k, int s, const EsPlan& pl, int max_rows) {
        EsState& st = slot[s];
        emit(es_pes_row(watch[s], s, k, pl, st.es_count, st.lost != 0), max_rows);
        st.lost = 0;
        st.synced = pl.valid;
    }
    void segment(int k, int s, const EsPlan& pl, const uint8_t* pay, uint64_t* win, uint32_t* since, int max_rows) {
        EsState& st = slot[s];
        for (int i = 0; i < pl.seg_len; ++i) {
            uint32_t code, hd;
            if (es_scan_byte(win, since, pay[pl.seg_off + i], &code, &hd)) {
                const EsCode e = es_classify(codec[s], code, hd);
                es_cnt_code(&cnt[s], e);
                if (e.unit < ES_UNITS) { emit(es_code_row(watch[s], s, k, e, code, hd, st.es_count + i - 7, st.lost != 0), max_rows); st.lost = 0; }
            }
        }
    }
};

}  // namespace s2
