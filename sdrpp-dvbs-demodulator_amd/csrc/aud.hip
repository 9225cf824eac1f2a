// Audio bank (own extension; include/dvbs2gpu.h): frame index of up to 16 watched audio PIDs (MPEG audio, ADTS,
// AC-3 / E-AC-3) of each of `nstreams` transport streams in HBM.  Every rule is in aud_rules.h, whose AudHostStream is the sequential
// definition, the host bank and the kernel's yardstick; this file says how a call's packets and their frames are taken in parallel.
//
// What is different from the ES bank: a frame boundary is no function of the bytes around it.  Sync words occur inside payloads; a
// header counts only where the chain header -> length -> next header arrives, and the chain runs through the whole call and across
// calls.  What makes a parallel form possible all the same: lock is taken at valid PES starts only, so the chain that a start begins
// is known from the start alone, and for PES-aligned audio the chain before a start ends exactly where the start's own begins.
//
//   aud_kernel  one workgroup per stream, one launch per call.
//     A-E  es_stream.h, shared with the ES bank: the trusted packets of watched PIDs sorted by slot with their verdicts, the starts'
//        plans, every packet's segment of ES bytes and its ES position by one prefix sum (exs), the last reset mark before a packet.
//        This bank's hook adds the events: an EVENT is a packet that is a start or carries a reset mark; link[] chains a slot's events,
//        and the packets from an event up to the next one are its TERRITORY.  Only an event changes the lock from outside; inside a
//        territory the chain alone does.
//     S  speculate: the lane of every valid start walks the chain through its territory as if the start acquired: hop by hop, a binary
//        search over exs maps the header's last byte to its packet, the 8 bytes are read (two dwords where they lie in one packet).
//        It writes every packet of the territory its ENTRY, 16 bits: the framer's state in front of the packet -- UNLOCKED, CARRY (the
//        state the call began with), PREV d (locked, the last frame began d bytes in front of the packet: its header gives next and
//        params) or ACQ v (locked since the start v packets back, no frame yet) -- and the territory's exit (locked and next, 16
//        bits, relative to the territory's end).  The lane of a slot's first packet walks the packets in front of the first event
//        from the carried state: that walk is no speculation.
//     J  join: one lane per slot goes from event to event with (locked, next) alone, reading no packet: a reset unlocks; a valid start
//        that finds the slot unlocked acquires, and its speculation holds; one that finds it locked with next at its own first byte
//        continues the chain, its speculation holds but for the first frame's flags (the start is marked CONT, and the lane of that
//        frame's packet looks back for the parameters); any other start is UNALIGNED: the lane takes the true state in front of it
//        and walks its territory frame by frame, writing the entries anew.  Only then does one lane's work grow with the frames.
//     F  every lane takes its packets' entries and checks the headers whose last byte lies in the packet (at most 27): the frames and
//        losses are counted, rows counted per packet.
//     G  es_stream.h: a prefix sum over the rows per packet in INPUT order, the PES rows, a second walk of each row-bearing packet
//        that writes its rows; the lane of the slot's last packet writes the slot's new state: here the tail and the framer's lock.
// Every loop is bounded by a size: positions strictly increase along a chain, a territory of B bytes has at most B / 7 + 2 hops.
// Vector stores and plain C++ only.
#include "es_stream.h"
#include "aud_rules.h"

using namespace s2;

namespace s2 {

constexpr int AUD_MAX_PACKETS = ES_MAX_PACKETS;
constexpr int AUD_WG = ES_WG;
static_assert(sizeof(AudRow) == sizeof(dvbs2gpu_aud_row) && sizeof(AudRow) == 48, "row layout");
static_assert(sizeof(AudCnt) * 2 == sizeof(dvbs2gpu_aud_stats), "stats order");
static_assert(sizeof(AudState) == 32, "state layout");
static_assert(AUD_SLOTS == ES_SLOTS && AUD_NONE == 0, "es_stream.h");
static_assert(AUD_MPA == DVBS2GPU_AUD_MPA && AUD_ADTS == DVBS2GPU_AUD_ADTS && AUD_AC3 == DVBS2GPU_AUD_AC3, "public values");
static_assert(AUD_PES == DVBS2GPU_AUD_UNIT_PES && AUD_FRAME == DVBS2GPU_AUD_UNIT_FRAME && AUD_LOSS == DVBS2GPU_AUD_UNIT_LOSS, "public values");
static_assert(AUD_ACQUIRED == DVBS2GPU_AUD_ACQUIRED && AUD_RESYNC == DVBS2GPU_AUD_RESYNC && AUD_UNSYNCED == DVBS2GPU_AUD_UNSYNCED &&
              AUD_SPLIT_HEADER == DVBS2GPU_AUD_SPLIT_HEADER && AUD_CHANGE == DVBS2GPU_AUD_CHANGE, "public values");
static_assert(AUD_PACKET_ROWS == 28 && AUD_MAX_FRAME + AUD_WINDOW < (1 << 14), "rows per packet in a byte; a distance inside a frame in an entry");

// bits 18 and 19 of a word are the bank's (ts_watch.h): VALID is es_stream.h's; behind phase J bit 19 says that a start continues a chain
constexpr uint32_t AW_CONT = 1u << 19;
__device__ inline bool aud_event(uint32_t e) { return pw_start(e) || es_reset_mark(e); }
constexpr uint16_t AUD_NO_LINK = 0xFFFF;
// an entry: the kind in bits 14-15, d or v below
constexpr int AE_UNLOCKED = 0, AE_CARRY = 1, AE_PREV = 2, AE_ACQ = 3;

// the framer's state along a walk.  next: relative to the slot's es_count before the call.  kind / ref: where it comes from -- CARRY;
// PREV, the last frame's position; ACQ, the start's sorted place
struct AudSt { bool locked; int64_t next; uint32_t params; int kind, ref; };

// what the kernel keeps in LDS beside the packets: es_stream.h's (place[]: behind the sort link[], an event's next event in sorted
// order) and the framer's
struct alignas(16) AudShared : EsStreamShared<AudCnt, AudState> {
    int64_t x0_next[AUD_SLOTS];                  // the exit of the walk in front of a slot's first event
    int32_t first_ev[AUD_SLOTS];                 // a slot's first event, -1: none
    int32_t x0_locked[AUD_SLOTS];
};
// what the bank is to es_stream.h
struct AudT {
    typedef AudState State; typedef AudCnt Cnt; typedef AudRow Row; typedef AudShared Shared;
    __device__ static void flush(AudCnt* d, const AudCnt& a) {
#define AUD_ADD(f) if (a.f) atomicAdd(&d->f, a.f)
        AUD_ADD(es_bytes); AUD_ADD(bytes_unsynced); AUD_ADD(resets); AUD_ADD(pes_starts); AUD_ADD(pes_invalid); AUD_ADD(split_headers);
        AUD_ADD(frames); AUD_ADD(frame_bytes_total); AUD_ADD(samples_total); AUD_ADD(acquisitions); AUD_ADD(sync_losses); AUD_ADD(param_changes);
        AUD_ADD(unaligned_starts); AUD_ADD(bytes_unlocked);
#undef AUD_ADD
    }
    __device__ static bool synced(const AudState& st) { return (st.bits & AUD_SYNCED) != 0; }
    __device__ static bool lost(const AudState& st) { return (st.bits & AUD_LOST) != 0; }
    // (LOCKED is the kernel's to set behind it)
    __device__ static void set_synced_lost(AudState& st, bool synced, bool lost) { st.bits = (uint8_t)((synced ? AUD_SYNCED : 0) | (lost ? AUD_LOST : 0)); }
    __device__ static AudRow pes_row(int pid, int slot, int k, const EsPlan& pl, uint64_t es_pos, bool lost) { return aud_pes_row(pid, slot, k, pl, es_pos, lost); }
};
typedef EsStreamCall<AudCnt> AudCall;
static_assert(sizeof(AudShared) % 16 == 0 && sizeof(AudShared::place) == AUD_MAX_PACKETS * sizeof(uint16_t), "the packets behind it; an index per packet");
// dynamic LDS: AudShared, srt[max_packets], exs[max_packets + 2] (32 bits each), ent[], xit[] (16 bits per packet), rc[] (8 bits)
constexpr size_t aud_even(int max_packets) { return ((size_t)max_packets + 1) & ~(size_t)1; }
constexpr size_t aud_lds_bytes(int max_packets) {
    return sizeof(AudShared) + ((size_t)max_packets * 2 + 2) * sizeof(uint32_t) + 2 * aud_even(max_packets) * sizeof(uint16_t) + (((size_t)max_packets + 15) & ~(size_t)15);
}
static_assert(aud_lds_bytes(AUD_MAX_PACKETS) < 64 * 1024, "dynamic LDS of a workgroup");        // 63.3 KiB

// the front's hook: the entries cleared, and the events chained: link[] and the slots' first events
struct AudEvents {
    AudShared& sh; uint16_t *ent, *xit, *link; int le;
    __device__ __forceinline__ void placed(int j) { ent[j] = 0; xit[j] = 0; link[j] = AUD_NO_LINK; }
    __device__ __forceinline__ void first(int j, uint32_t e, int) { if (aud_event(e)) le = j; }
    __device__ __forceinline__ void between(int* wsum) { le = ts_block_scan_max(le, wsum); }                 // the last event before the thread's run
    __device__ __forceinline__ void second(int j, uint32_t e, int) {
        if (!aud_event(e)) return;
        if (le >= sh.start[pw_slot(e)]) link[le] = (uint16_t)j; else sh.first_ev[pw_slot(e)] = j;
        le = j;
    }
};

// One slot's packets of the call as the walks see them: the sorted run [head, end), their words and prefix values, and the ES bytes at
// positions relative to the slot's es_count before the call (negative: the carried tail)
struct AudRun {
    const uint8_t* __restrict__ ts;
    const uint32_t* srt;
    const uint32_t* exs;
    uint64_t tail;
    int head, end;

    __device__ int pos(int j) const { return (int)(exs[j] - exs[head]); }                 // of the first byte of sorted packet j (j = end: the call's bytes)
    // the packet that holds position r, 0 <= r < pos(end), searched from sorted place lo on (pos(lo) <= r)
    __device__ __forceinline__ int find(int r, int lo) const {
        int hi = end - 1;
        for (int it = 0; it < 13 && lo < hi; ++it) {
            const int mid = (lo + hi + 1) >> 1;
            if (pos(mid) <= r) lo = mid; else hi = mid - 1;
        }
        return lo;
    }
    // n <= 8 bytes from position q >= -7 on, the first in the highest of the n low bytes.  q + n <= pos(end)
    __device__ __forceinline__ uint64_t bytes(int q, int n) const {
        uint64_t v = 0;
        int j = -1, a = 0, b = 0;
        if (q >= 0) {
            j = find(q, head); a = pos(j); b = pos(j + 1);
            if (n == 8 && q + 8 <= b) {                                                   // inside one packet: two dwords
                const uint8_t* p = ts + (size_t)pw_k(srt[j]) * TSMON_TS + TSMON_TS - (b - a) + (q - a);
                const uint32_t lo = *reinterpret_cast<const ts_unaligned_u32*>(p), hi = *reinterpret_cast<const ts_unaligned_u32*>(p + 4);
                return (uint64_t)__builtin_bswap32(lo) << 32 | __builtin_bswap32(hi);
            }
        }
        for (int i = 0; i < n; ++i) {
            const int r = q + i;
            uint32_t byte = 0;
            if (r < 0) byte = (uint32_t)(tail >> (8 * (-r - 1))) & 255;
            else {
                if (j < 0 || r >= b) { j = find(r, j < 0 ? head : j); a = pos(j); b = pos(j + 1); }
                if (r < b) byte = ts[(size_t)pw_k(srt[j]) * TSMON_TS + TSMON_TS - (b - a) + (r - a)];
            }
            v = v << 8 | byte;
        }
        return v;
    }
};

__global__ void __launch_bounds__(AUD_WG) aud_kernel(const uint8_t* const* __restrict__ in, const int* __restrict__ nbytes, int max_packets, int max_rows,
                                                     const int32_t* __restrict__ watch, const int32_t* __restrict__ codec, AudState* __restrict__ state,
                                                     int64_t* __restrict__ pos, AudRow* __restrict__ rows_g, AudCall* __restrict__ call) {
    extern __shared__ __attribute__((aligned(16))) unsigned char aud_lds[];
    EsStream<AudT> f(aud_lds, in, nbytes, max_packets, max_rows);
    AudShared& sh = f.sh;
    uint32_t* srt = f.srt;
    const uint32_t* exs = f.exs;
    const uint8_t* ts = f.ts;
    uint16_t* ent = reinterpret_cast<uint16_t*>(f.exs + max_packets + 2);   // the entries, per sorted packet
    uint16_t* xit = ent + aud_even(max_packets);                            // a valid start's exit: 0 unlocked, else 8 + next - the territory's end
    uint8_t* rc = reinterpret_cast<uint8_t*>(xit + aud_even(max_packets));  // rows per INPUT packet
    uint16_t* link = &sh.place[0][0];
    const int tid = f.tid;
    if (tid < AUD_SLOTS) {
        sh.first_ev[tid] = -1;
        sh.x0_locked[tid] = 0; sh.x0_next[tid] = 0;
    }
    for (int k = tid; k < f.n; k += AUD_WG) rc[k] = 0;
    EsStreamAcc<AudT> acc(sh.cnt);
    AudEvents hook = {sh, ent, xit, link, -1};
    int nrows = 0;
    // A-E: es_stream.h
    if (f.front(watch, codec, state, pos, acc, hook)) {
        const int j0 = f.j0, j1 = f.j1;
        auto run_of = [&](int slot) { return AudRun{ts, srt, exs, sh.ss[slot].tail, sh.start[slot], sh.start[slot + 1]}; };
        auto carried = [&](int slot) {
            const AudState& c = sh.ss[slot];
            return AudSt{(c.bits & AUD_LOCKED) != 0, (int64_t)(c.next - c.es_count), c.params, AE_CARRY, 0};
        };
        auto encode = [&](const AudRun& r, const AudSt& st, int j) {
            if (!st.locked) return (uint16_t)0;
            if (st.kind == AE_CARRY) return (uint16_t)(AE_CARRY << 14);
            return (uint16_t)(st.kind << 14 | (st.kind == AE_PREV ? r.pos(j) - st.ref : j - st.ref));
        };
        // the header at st.next, whose 8 bytes lie in the call or its carried tail: checked as the rules say
        auto check = [&](const AudRun& r, int slot, AudSt& st, AudCnt* c, AudRow* row) {
            const int q = (int)st.next;
            AudLock lk = {sh.ss[slot].es_count + (uint64_t)(int64_t)q, st.params};
            if (aud_check(sh.codec[slot], r.bytes(q, 8), &lk, c, row)) { st.next = (int64_t)(lk.next - sh.ss[slot].es_count); st.params = lk.params; st.kind = AE_PREV; st.ref = q; }
            else st.locked = false;
        };
        // The headers whose last byte lies in sorted packet j, from the state in front of it (at most 27).  rows: written at
        // rows[rank ..] below max_rows, the first with RESYNC if `lost`.  *loss_at: the place in the segment of a LOSS's last byte -> the checks
        auto walk_packet = [&](const AudRun& r, int slot, int j, AudSt& st, AudCnt* c, AudRow* rows, int rank, int max_r, bool lost, int* loss_at) {
            const int a = r.pos(j), b = r.pos(j + 1);
            int checks = 0;
            for (int it = 0; it < AUD_PACKET_ROWS && st.locked; ++it) {
                if (st.next + 7 >= b || st.next + 7 < a) break;
                const int t = (int)st.next + 7 - a;
                AudRow row;
                check(r, slot, st, c, &row);
                if (!st.locked && loss_at) *loss_at = t;
                if (rows) {
                    row.pid = (uint16_t)sh.w[slot]; row.slot = (uint8_t)slot; row.packet = (uint16_t)pw_k(srt[j]);
                    if (lost) row.flags |= AUD_RESYNC;
                    lost = false;
                    if (rank + checks < max_r) rows[rank + checks] = row;
                }
                ++checks;
            }
            return checks;
        };
        // the parameters of the frame in front of the start js that continues a chain (0: none since the acquisition): those behind the
        // packet before it, looked up through the entries; a packet without a header whose own start continues a chain leads further back
        auto prev_params = [&](const AudRun& r, int slot, int js) {
            AudCnt none = aud_cnt_zero();
            for (int it = r.head; it < r.end; ++it) {
                if (js <= r.head) return sh.ss[slot].params;
                const int jp = js - 1, kind = ent[jp] >> 14, v = ent[jp] & 0x3FFF;
                AudSt st = {kind != AE_UNLOCKED, 0, 0, kind, 0};
                if (kind == AE_CARRY) st = carried(slot);
                else if (kind == AE_PREV) {
                    st.ref = r.pos(jp) - v;
                    const AudParse p = aud_parse(sh.codec[slot], r.bytes(st.ref, 8));
                    st.next = st.ref + (int64_t)p.frame_bytes; st.params = p.params;
                } else if (kind == AE_ACQ) { st.ref = jp - v; st.next = r.pos(st.ref); }
                const int checks = walk_packet(r, slot, jp, st, &none, nullptr, 0, 0, false, nullptr);
                if (!st.locked) return 0u;
                if (kind != AE_ACQ || checks > 0) return st.params;
                js = jp - v;
                if (!(srt[js] & AW_CONT)) return 0u;
            }
            return 0u;
        };
        // the framer's state in front of sorted packet j, from its entry
        auto state_in = [&](const AudRun& r, int slot, int j) {
            const int kind = ent[j] >> 14, v = ent[j] & 0x3FFF;
            AudSt st = {kind != AE_UNLOCKED, 0, 0, kind, 0};
            if (kind == AE_CARRY) st = carried(slot);
            else if (kind == AE_PREV) {
                st.ref = r.pos(j) - v;
                const AudParse p = aud_parse(sh.codec[slot], r.bytes(st.ref, 8));
                st.next = st.ref + (int64_t)p.frame_bytes; st.params = p.params;
            } else if (kind == AE_ACQ) {
                st.ref = j - v; st.next = r.pos(st.ref);
                if (srt[st.ref] & AW_CONT) st.params = prev_params(r, slot, st.ref);
            }
            return st;
        };
        // the chain through the territory [ja, jb) from the state in front of ja: every packet's entry, and the state behind it
        auto walk_territory = [&](const AudRun& r, int slot, int ja, int jb, AudSt st) {
            const int T = r.pos(jb), hops = (T - r.pos(ja)) / AUD_MIN_FRAME + 2;
            AudCnt none = aud_cnt_zero();
            AudRow row;
            int j = ja;
            for (int hop = 0; hop < hops && st.locked; ++hop) {
                if (st.next + 7 >= T) break;
                const int jw = r.find((int)st.next + 7, j > ja ? j - 1 : ja);
                for (; j <= jw; ++j) ent[j] = encode(r, st, j);
                check(r, slot, st, &none, &row);
            }
            for (; j < jb; ++j) ent[j] = encode(r, st, j);
            return st;
        };
        // S: the walks of the valid starts, and of the packets in front of a slot's first event
        for (int j = j0; j < j1; ++j) {
            const uint32_t e = srt[j];
            const int slot = pw_slot(e);
            const AudRun r = run_of(slot);
            if (j == r.head && sh.first_ev[slot] != j && (sh.ss[slot].bits & AUD_LOCKED)) {
                const int fe = sh.first_ev[slot];
                const AudSt st = walk_territory(r, slot, j, fe >= 0 ? fe : r.end, carried(slot));
                sh.x0_locked[slot] = st.locked; sh.x0_next[slot] = st.next;
            }
            if (pw_start(e) && (e & PW_VALID)) {
                const int jb = link[j] != AUD_NO_LINK && link[j] < r.end ? link[j] : r.end;
                const AudSt st = walk_territory(r, slot, j, jb, AudSt{true, r.pos(j), 0, AE_ACQ, j});
                xit[j] = st.locked ? (uint16_t)(8 + st.next - r.pos(jb)) : (uint16_t)0;
            }
        }
        __syncthreads();
        // J: the join, one lane per slot
        if (tid < AUD_SLOTS && sh.start[tid] < sh.start[tid + 1]) {
            const int slot = tid;
            const AudRun r = run_of(slot);
            int ev = sh.first_ev[slot], acquisitions = 0, unaligned = 0;
            AudSt st = ev == r.head ? carried(slot) : AudSt{sh.x0_locked[slot] != 0, sh.x0_next[slot], 0, AE_CARRY, 0};
            bool full = ev == r.head;                            // st has params, kind and ref, beyond (locked, next)
            for (int it = r.head; it < r.end && ev >= 0; ++it) {
                const uint32_t e = srt[ev];
                const int jb = link[ev] != AUD_NO_LINK && link[ev] < r.end ? link[ev] : r.end;
                if (es_reset_mark(e)) st.locked = false;                                 // (a reset in front of a valid start: it acquires)
                if (pw_start(e) && (e & PW_VALID)) {
                    if (!st.locked || st.next == r.pos(ev)) {                             // the speculation holds
                        if (!st.locked) ++acquisitions; else srt[ev] = e | AW_CONT;
                        st.locked = xit[ev] != 0; st.next = r.pos(jb) + (int)xit[ev] - 8;
                        full = false;
                    } else {
                        ++unaligned;
                        if (!full) {                                                      // the state behind the packet in front of the start
                            AudCnt none = aud_cnt_zero();
                            st = state_in(r, slot, ev - 1);
                            walk_packet(r, slot, ev - 1, st, &none, nullptr, 0, 0, false, nullptr);
                        }
                        st = walk_territory(r, slot, ev, jb, st);
                        full = true;
                    }
                }
                ev = jb < r.end ? jb : -1;
            }
            if (acquisitions) atomicAdd(&sh.cnt[slot].acquisitions, acquisitions);
            if (unaligned) atomicAdd(&sh.cnt[slot].unaligned_starts, unaligned);
        }
        __syncthreads();
        // F: the frames, counted; the rows per packet
        int last_row = -1;
        for (int j = j0; j < j1; ++j) {
            const uint32_t e = srt[j];
            const int slot = pw_slot(e), len = (int)(exs[j + 1] - exs[j]);
            acc.at(slot);
            int nr = pw_start(e);
            if (len > 0) {
                const AudRun r = run_of(slot);
                AudSt st = state_in(r, slot, j);
                if (!st.locked) acc.c.bytes_unlocked += len;
                else {
                    int loss_at = len - 1;
                    nr += walk_packet(r, slot, j, st, &acc.c, nullptr, 0, 0, false, &loss_at);
                    acc.c.bytes_unlocked += len - 1 - loss_at;
                }
            }
            if (nr) { rc[pw_k(e)] = (uint8_t)nr; last_row = j; }
        }
        acc.done();
        __syncthreads();
        // G: es_stream.h; a second walk of each row-bearing packet writes its rows
        AudRow* rows = rows_g + (size_t)f.s * max_rows;
        nrows = f.rows(rc, last_row, rows_g, state,
            [&](int j, uint32_t e, uint64_t, int, int rank, bool lost) {
                const int slot = pw_slot(e);
                const AudRun r = run_of(slot);
                AudSt st = state_in(r, slot, j);
                AudCnt none = aud_cnt_zero();
                walk_packet(r, slot, j, st, &none, rows, rank, max_rows, lost, nullptr);
            },
            [&](AudState& nx, int slot, int j, int lr) {
                const AudRun r = run_of(slot);
                AudSt st = state_in(r, slot, j);
                AudCnt none = aud_cnt_zero();
                walk_packet(r, slot, j, st, &none, nullptr, 0, 0, false, nullptr);
                const int total = r.pos(r.end);
                const uint32_t sn = lr >= r.head ? (uint32_t)(total - r.pos(lr)) : (uint32_t)nx.have + (uint32_t)total;
                const int have = sn < 7 ? (int)sn : 7;
                nx.tail = r.bytes(total - have, have); nx.have = (uint8_t)have;
                if (st.locked) { nx.bits |= AUD_LOCKED; nx.next = sh.ss[slot].es_count + (uint64_t)st.next; nx.params = st.params; }
            });
    }
    f.finish(call, pos, nrows);
}

}  // namespace s2

// the host half is the watched-PID bank's (watch_bank.h) with what es_stream.h adds for a bank with a codec per slot; here what is the bank's own
struct AudBankD : EsStreamBankD<AudBankD, AudT, aud_kernel, aud_lds_bytes, AUD_COUNTERS> {
    typedef AudHostStream HostStream; typedef dvbs2gpu_aud_stats Stats; typedef dvbs2gpu_aud_stream_stats StreamStats;
    static constexpr StreamStats NO_STREAM_STATS = {};
    static constexpr const char *BANK = "audio bank: ", *CNAME = "dvbs2gpu_aud", *ALLOC = "hipMalloc(aud)";
};
struct dvbs2gpu_aud : WatchBank<AudBankD> {};

extern "C" {

void dvbs2gpu_aud_destroy(dvbs2gpu_aud* b) { delete b; }
int dvbs2gpu_aud_create(dvbs2gpu_ctx* ctx, int nstreams, int max_packets, int max_rows, dvbs2gpu_aud** out) { return watch_create(true, ctx, nstreams, max_packets, max_rows, out); }
int dvbs2gpu_aud_create_host(int nstreams, int max_packets, int max_rows, dvbs2gpu_aud** out) { return watch_create(false, nullptr, nstreams, max_packets, max_rows, out); }
int dvbs2gpu_aud_reset(dvbs2gpu_aud* b) { return watch_reset(b); }

int dvbs2gpu_aud_set_watch(dvbs2gpu_aud* b, int stream, int slot, int pid, int codec) {
    return es_stream_set_watch(b, stream, slot, pid, codec, AUD_AC3, "audio bank: the codec is DVBS2GPU_AUD_MPA, _ADTS or _AC3");
}

int dvbs2gpu_aud_process_batch(dvbs2gpu_aud* b, const uint8_t* const* d_ts, const int* nbytes, int* out_rows, void* stream) {
    return watch_process_batch(b, d_ts, nbytes, out_rows, stream);
}
int dvbs2gpu_aud_work(dvbs2gpu_aud* b, int stream, const uint8_t* h_ts, int nbytes) { return watch_work(b, stream, h_ts, nbytes); }
int dvbs2gpu_aud_get_stats(dvbs2gpu_aud* b, int stream, int slot, dvbs2gpu_aud_stats* h_out) { return watch_get_stats(b, stream, slot, h_out); }
int dvbs2gpu_aud_get_stream_stats(dvbs2gpu_aud* b, int stream, dvbs2gpu_aud_stream_stats* h_out) { return watch_get_stream_stats(b, stream, h_out); }
int dvbs2gpu_aud_get_row_table(dvbs2gpu_aud* b, int stream, dvbs2gpu_aud_row* h_rows, int cap, int* n) { return watch_get_row_table(b, stream, h_rows, cap, n); }
int dvbs2gpu_aud_get_row_table_device(dvbs2gpu_aud* b, int stream, const dvbs2gpu_aud_row** d_rows, int* n) { return watch_get_row_table_device(b, stream, d_rows, n); }

}  // extern "C"
