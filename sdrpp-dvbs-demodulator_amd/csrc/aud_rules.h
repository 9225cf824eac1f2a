// The rules of the audio bank (own extension; include/dvbs2gpu.h), each stated once and shared by the kernel
// (aud.hip), the native host bank (AudHostStream below, behind dvbs2gpu_aud_create_host) and a plain C++ test program: what the first 8
// bytes of an MPEG audio, ADTS or AC-3 / E-AC-3 frame say (aud_parse: a pure function of 8 bytes), the framer's check of one header
// (aud_check) and what a row adds to its slot's counters.  Which bytes of a watched PID are elementary-stream bytes is the ES bank's
// rule (es_packet_plan of es_rules.h: the packet's reset, its PES start and its segment), not restated here.
//
// The sequential form -- AudHostStream::run, packet by packet and byte by byte -- IS the definition; every other form must give its
// rows, counters and state for every cut of a stream into calls.  Header syntax as remembered from ISO/IEC 11172-3, 13818-3, 13818-7
// and ETSI TS 102 366; pinned to no vector of theirs.
// Standard headers only: the host tests compile this file with a plain C++ compiler.
#pragma once
#include "es_rules.h"

#define AUD_HD PES_HD

namespace s2 {

constexpr int AUD_SLOTS = ES_SLOTS;
enum AudCodec { AUD_NONE = 0, AUD_MPA = 1, AUD_ADTS = 2, AUD_AC3 = 3 };
enum AudUnit { AUD_PES = 0, AUD_FRAME = 1, AUD_LOSS = 2 };
// row flags (DVBS2GPU_AUD_*); RESYNC, UNSYNCED and SPLIT_HEADER are the ES bank's
constexpr int AUD_ACQUIRED = 1, AUD_RESYNC = ES_RESYNC, AUD_UNSYNCED = ES_UNSYNCED, AUD_SPLIT_HEADER = ES_SPLIT_HEADER, AUD_CHANGE = 16;
constexpr int AUD_WINDOW = 8;                               // ES bytes that decide a frame
constexpr int AUD_MIN_FRAME = 7;                            // no valid header says less
constexpr int AUD_MAX_FRAME = 8191;                         // nor more (ADTS: 13 bits)
constexpr int AUD_PACKET_ROWS = (TSMON_TS - 4 + AUD_MIN_FRAME - 1) / AUD_MIN_FRAME + 1;   // 27 frame / LOSS rows and the PES row

#pragma pack(push, 4)
struct AudRow {                                             // the layout of dvbs2gpu_aud_row: 48 bytes, es_offset at 16
    uint16_t pid; uint8_t slot, unit, code, detail; uint16_t flags;
    uint16_t packet, kbps; uint32_t head;
    uint64_t es_offset, pts, dts;
    uint32_t sample_rate; uint16_t frame_bytes, samples;
};
#pragma pack(pop)

// what 8 bytes say: frame_bytes 0: no valid header.  params: everything of the header but padding and length, never 0
struct AudParse { uint32_t frame_bytes, sample_rate, samples, kbps, code, detail, params; };

// eight bitrates in kbit/s, all multiples of 8, as one word: the first in the low byte
AUD_HD constexpr uint64_t aud_kbps8(uint64_t a, uint64_t b, uint64_t c, uint64_t d, uint64_t e, uint64_t f, uint64_t g, uint64_t h) {
    return a / 8 | b / 8 << 8 | c / 8 << 16 | d / 8 << 24 | e / 8 << 32 | f / 8 << 40 | g / 8 << 48 | h / 8 << 56;
}

// MPEG-1/2/2.5 audio, layers I-III.  code: version << 2 | layer (the header's bits), detail: mode
AUD_HD inline AudParse aud_parse_mpa(uint32_t h) {
    AudParse p = {0, 0, 0, 0, 0, 0, 0};
    const uint32_t ver = h >> 19 & 3, layer = h >> 17 & 3, bri = h >> 12 & 15, sri = h >> 10 & 3, pad = h >> 9 & 1;
    if (h >> 21 != 0x7FF || ver == 1 || layer == 0 || bri == 0 || bri == 15 || sri == 3) return p;
    // the five bitrate tables, index 1..14 (no array: the kernel keeps them in registers): V1 L1, V1 L2, V1 L3, V2 L1, V2 L2 and L3
    const uint32_t row = ver == 3 ? 3 - layer : layer == 3 ? 3 : 4;
    const uint64_t lo = row == 1 ? aud_kbps8(32, 48, 56, 64, 80, 96, 112, 128) : row == 2 ? aud_kbps8(32, 40, 48, 56, 64, 80, 96, 112)
                      : row == 3 ? aud_kbps8(32, 48, 56, 64, 80, 96, 112, 128) : aud_kbps8(8, 16, 24, 32, 40, 48, 56, 64);
    const uint64_t hi = row == 1 ? aud_kbps8(160, 192, 224, 256, 320, 384, 0, 0) : row == 2 ? aud_kbps8(128, 160, 192, 224, 256, 320, 0, 0)
                      : row == 3 ? aud_kbps8(144, 160, 176, 192, 224, 256, 0, 0) : aud_kbps8(80, 96, 112, 128, 144, 160, 0, 0);
    const uint32_t kbps = row == 0 ? 32 * bri : 8 * (uint32_t)((bri <= 8 ? lo >> (8 * (bri - 1)) : hi >> (8 * (bri - 9))) & 255);
    const uint32_t base = sri == 0 ? 44100 : sri == 1 ? 48000 : 32000, fs = ver == 3 ? base : ver == 2 ? base / 2 : base / 4;
    p.sample_rate = fs; p.kbps = kbps;
    if (layer == 3) { p.frame_bytes = (12 * kbps * 1000 / fs + pad) * 4; p.samples = 384; }
    else if (layer == 2 || ver == 3) { p.frame_bytes = 144 * kbps * 1000 / fs + pad; p.samples = 1152; }
    else { p.frame_bytes = 72 * kbps * 1000 / fs + pad; p.samples = 576; }
    p.code = ver << 2 | layer; p.detail = h >> 6 & 3;
    p.params = (uint32_t)AUD_MPA << 30 | (h & 0x001FFCC0u);         // version, layer, protection, bitrate, rate, mode
    return p;
}

// bits per second as the frame's own size gives them, in kbit/s (the codecs whose header names no bitrate)
AUD_HD inline uint32_t aud_kbps_of(uint32_t frame_bytes, uint32_t fs, uint32_t samples) { return (uint32_t)((uint64_t)frame_bytes * 8 * fs / ((uint64_t)samples * 1000)); }

// AAC in ADTS.  code: ID << 2 | profile, detail: channel_configuration
AUD_HD inline AudParse aud_parse_adts(const uint8_t* w) {
    AudParse p = {0, 0, 0, 0, 0, 0, 0};
    const uint32_t sfi = w[2] >> 2 & 15, len = (uint32_t)(w[3] & 3) << 11 | (uint32_t)w[4] << 3 | w[5] >> 5, absent = w[1] & 1, blocks = w[6] & 3;
    if (w[0] != 0xFF || w[1] >> 4 != 0xF || (w[1] >> 1 & 3) != 0 || sfi > 12 || len < (absent ? 7u : 9u)) return p;
    const uint32_t k = sfi % 3, oct = sfi / 3;                   // 96000 88200 64000 and their halves; 7350 alone
    p.sample_rate = sfi == 12 ? 7350 : (k == 0 ? 96000u : k == 1 ? 88200u : 64000u) >> oct;
    p.frame_bytes = len; p.samples = 1024 * (blocks + 1);
    p.kbps = aud_kbps_of(len, p.sample_rate, p.samples);
    p.code = (w[1] >> 3 & 1) << 2 | w[2] >> 6; p.detail = (w[2] & 1) << 2 | w[3] >> 6;
    p.params = (uint32_t)AUD_ADTS << 30 | (uint32_t)(w[1] & 15) << 16 | (uint32_t)(w[2] & 0xFD) << 8 | (w[3] & 0xC0) | blocks;
    return p;
}

// AC-3 (bsid <= 10) and E-AC-3 (bsid 11..16).  code: bsid, detail: acmod (E-AC-3: | lfeon << 3)
AUD_HD inline AudParse aud_parse_ac3(const uint8_t* w) {
    AudParse p = {0, 0, 0, 0, 0, 0, 0};
    if (w[0] != 0x0B || w[1] != 0x77) return p;
    const uint32_t bsid = w[5] >> 3, fscod = w[4] >> 6;
    if (bsid <= 10) {
        const uint32_t fsc = w[4] & 63;
        if (fscod == 3 || fsc > 37) return p;
        const uint32_t i = fsc >> 1;                              // 32 40 48 56 64 80 96 112 128 160 192 224 256 320 384 448 512 576 640
        const uint32_t br = i < 4 ? 32 + 8 * i : i < 8 ? 64 + 16 * (i - 4) : i < 12 ? 128 + 32 * (i - 8) : i < 18 ? 256 + 64 * (i - 12) : 640;
        const uint32_t words = fscod == 0 ? 2 * br : fscod == 2 ? 3 * br : 320 * br / 147 + (fsc & 1);
        p.frame_bytes = 2 * words; p.sample_rate = fscod == 0 ? 48000 : fscod == 1 ? 44100 : 32000; p.samples = 1536; p.kbps = br;
        p.code = bsid; p.detail = w[6] >> 5;
        p.params = (uint32_t)AUD_AC3 << 30 | fscod << 22 | i << 16 | (uint32_t)w[5] << 8 | w[6] >> 5;
    } else if (bsid <= 16) {
        const uint32_t frmsiz = (uint32_t)(w[2] & 7) << 8 | w[3], c2 = w[4] >> 4 & 3;
        if ((fscod == 3 && c2 == 3) || 2 * (frmsiz + 1) < (uint32_t)AUD_MIN_FRAME) return p;
        const uint32_t blocks = fscod == 3 ? 6 : c2 == 3 ? 6 : c2 + 1, sel = fscod == 3 ? c2 : fscod;
        p.sample_rate = (sel == 0 ? 48000u : sel == 1 ? 44100u : 32000u) >> (fscod == 3);
        p.frame_bytes = 2 * (frmsiz + 1); p.samples = 256 * blocks;
        p.kbps = aud_kbps_of(p.frame_bytes, p.sample_rate, p.samples);
        p.code = bsid; p.detail = (w[4] >> 1 & 7) | (w[4] & 1) << 3;
        p.params = (uint32_t)AUD_AC3 << 30 | 1u << 29 | (uint32_t)(w[2] >> 3) << 16 | (uint32_t)w[4] << 8 | w[5] >> 3;
    }
    return p;
}

// the window w0..w7 as one word, w0 in the high byte
AUD_HD inline AudParse aud_parse(int codec, uint64_t win) {
    const uint8_t w[8] = {(uint8_t)(win >> 56), (uint8_t)(win >> 48), (uint8_t)(win >> 40), (uint8_t)(win >> 32),
                          (uint8_t)(win >> 24), (uint8_t)(win >> 16), (uint8_t)(win >> 8), (uint8_t)win};
    if (codec == AUD_MPA) return aud_parse_mpa((uint32_t)(win >> 32));
    if (codec == AUD_ADTS) return aud_parse_adts(w);
    if (codec == AUD_AC3) return aud_parse_ac3(w);
    return AudParse{0, 0, 0, 0, 0, 0, 0};
}

// The state of one slot: the ES bank's (es_count, the last `have` accepted bytes, cc) and the framer's: next, the ES position of the
// next header while LOCKED (any distance ahead), and params, the parameter word of the frame before it (0: none since the
// acquisition, the coming row is marked ACQUIRED)
constexpr int AUD_SYNCED = 1, AUD_LOST = 2, AUD_LOCKED = 4;
struct AudState { uint64_t es_count, tail, next; uint32_t params; uint8_t cc, have, bits, pad; };

// what one call adds to a slot's statistics, in the order of dvbs2gpu_aud_stats: the ES bank's twelve (EsStreamCnt, with es_cnt_start
// for a start) and the framer's
struct AudCnt : EsStreamCnt {
    int32_t frames, frame_bytes_total, samples_total, acquisitions, sync_losses, param_changes, unaligned_starts, bytes_unlocked;
};
constexpr int AUD_COUNTERS = 20;
static_assert(sizeof(AudCnt) == AUD_COUNTERS * sizeof(int32_t), "counter order");
AUD_HD inline AudCnt aud_cnt_zero() { return AudCnt{}; }

// The framer's check of the header at `next`: the window w0..w7 against the frame before it (params; 0: the first since the
// acquisition).  A valid header: a FRAME row, params and the next header's place follow it, true.  Else a LOSS row, false: the lock is lost
struct AudLock { uint64_t next; uint32_t params; };
AUD_HD inline bool aud_check(int codec, uint64_t win, AudLock* lk, AudCnt* c, AudRow* r) {
    const AudParse p = aud_parse(codec, win);
    const uint32_t acq = lk->params == 0 ? AUD_ACQUIRED : 0;
    r->head = (uint32_t)(win >> 32); r->es_offset = lk->next; r->pts = PES_NO_TS; r->dts = PES_NO_TS;
    if (!p.frame_bytes) {
        r->unit = AUD_LOSS; r->code = 0; r->detail = 0; r->flags = (uint16_t)acq; r->kbps = 0; r->sample_rate = 0; r->frame_bytes = 0; r->samples = 0;
        ++c->sync_losses;
        return false;
    }
    const bool change = !acq && p.params != lk->params;
    r->unit = AUD_FRAME; r->code = (uint8_t)p.code; r->detail = (uint8_t)p.detail; r->flags = (uint16_t)(acq | (change ? AUD_CHANGE : 0));
    r->kbps = (uint16_t)p.kbps; r->sample_rate = p.sample_rate; r->frame_bytes = (uint16_t)p.frame_bytes; r->samples = (uint16_t)p.samples;
    ++c->frames; c->frame_bytes_total += (int32_t)p.frame_bytes; c->samples_total += (int32_t)p.samples; c->param_changes += change;
    lk->next += p.frame_bytes; lk->params = p.params;
    return true;
}
AUD_HD inline AudRow aud_pes_row(int pid, int slot, int k, const EsPlan& p, uint64_t es_count, bool lost) {
    return AudRow{(uint16_t)pid, (uint8_t)slot, AUD_PES, (uint8_t)p.hd.stream_id, (uint8_t)p.hd.kind, (uint16_t)(p.row_flags | (lost ? AUD_RESYNC : 0)), (uint16_t)k, 0,
                  p.hd.declared, es_count, p.hd.pts, p.hd.dts, 0, 0, 0};
}
// ------------------------------------------------------------------------------------------------- the sequential definition
// the packet walk is the ES bank's (EsHostWalk, es_rules.h); here what the framer does with a reset, a start and a segment's bytes
struct AudHostStream : EsHostWalk<AudHostStream, AudState, AudCnt, AudRow> {
    void emit(AudRow r, AudState& st, int max_rows) {
        if (st.bits & AUD_LOST) r.flags |= AUD_RESYNC;
        st.bits &= (uint8_t)~AUD_LOST;
        EsHostWalk::emit(r, max_rows);
    }
    static bool synced(const AudState& st) { return (st.bits & AUD_SYNCED) != 0; }
    // a reset: the window is forgotten, the lock is lost without a row
    static void stream_reset(AudState& st) { st.have = 0; st.tail = 0; st.bits = (uint8_t)((st.bits | AUD_LOST) & ~AUD_LOCKED); }
    void start(int k, int s, const EsPlan& pl, int max_rows) {
        AudState& st = slot[s];
        emit(aud_pes_row(watch[s], s, k, pl, st.es_count, false), st, max_rows);
        st.bits = (uint8_t)(pl.valid ? st.bits | AUD_SYNCED : st.bits & ~AUD_SYNCED);
        if (!pl.valid) return;
        if (!(st.bits & AUD_LOCKED)) { st.bits |= AUD_LOCKED; st.next = st.es_count; st.params = 0; ++cnt[s].acquisitions; }
        else if (st.next != st.es_count) ++cnt[s].unaligned_starts;
    }
    void segment(int k, int s, const EsPlan& pl, const uint8_t* pay, uint64_t* win, uint32_t* since, int max_rows) {
        AudState& st = slot[s];
        AudCnt& c = cnt[s];
        for (int i = 0; i < pl.seg_len; ++i) {
            c.bytes_unlocked += !(st.bits & AUD_LOCKED);        // (the byte that completes a failing window was accepted while locked)
            *win = *win << 8 | pay[pl.seg_off + i];
            ++*since;
            if (*since < (uint32_t)AUD_WINDOW || !(st.bits & AUD_LOCKED) || st.es_count + i - 7 != st.next) continue;
            AudLock lk = {st.next, st.params};
            AudRow r = {(uint16_t)watch[s], (uint8_t)s, 0, 0, 0, 0, (uint16_t)k, 0, 0, 0, 0, 0, 0, 0, 0};
            if (!aud_check(codec[s], *win, &lk, &c, &r)) st.bits &= (uint8_t)~AUD_LOCKED;
            st.next = lk.next; st.params = lk.params;
            emit(r, st, max_rows);
        }
    }
};

}  // namespace s2
