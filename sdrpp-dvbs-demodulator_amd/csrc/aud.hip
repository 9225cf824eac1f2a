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
//     A-E  as in the ES bank (ts_watch.h; es.hip): the trusted packets of watched PIDs sorted by slot with their verdicts, the starts'
//        plans, every packet's segment of ES bytes and its ES position by one prefix sum (exs), the last reset mark before a packet.
//        An EVENT is a packet that is a start or carries a reset mark; link[] chains a slot's events, and the packets from an event up
//        to the next one are its TERRITORY.  Only an event changes the lock from outside; inside a territory the chain alone does.
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
//     G  the ES bank's: a prefix sum over the rows per packet in INPUT order, the PES rows, a second walk of each row-bearing packet
//        that writes its rows; the lane of the slot's last packet writes the slot's new state.
// Every loop is bounded by a size: positions strictly increase along a chain, a territory of B bytes has at most B / 7 + 2 hops.
// Vector stores and plain C++ only.
#include "ts_watch.h"
#include "watch_bank.h"
#include "aud_rules.h"

using namespace s2;
#define g_err last_error()

namespace s2 {

constexpr int AUD_MAX_PACKETS = PW_MAX_PACKETS;
constexpr int AUD_WG = 256;
static_assert(sizeof(AudRow) == sizeof(dvbs2gpu_aud_row) && sizeof(AudRow) == 48, "row layout");
static_assert(sizeof(AudCnt) * 2 == sizeof(dvbs2gpu_aud_stats), "stats order");
static_assert(sizeof(AudState) == 32, "state layout");
static_assert(AUD_MAX_PACKETS <= 16 * AUD_WG, "a thread's verdicts are 16 bits of a mask, its slot counts 16-bit words (ts_thread_run)");
static_assert(AUD_MAX_PACKETS * (TSMON_TS - 4) < (1 << 20), "the prefix sum of segment bytes in an int");
static_assert(AUD_MPA == DVBS2GPU_AUD_MPA && AUD_ADTS == DVBS2GPU_AUD_ADTS && AUD_AC3 == DVBS2GPU_AUD_AC3, "public values");
static_assert(AUD_PES == DVBS2GPU_AUD_UNIT_PES && AUD_FRAME == DVBS2GPU_AUD_UNIT_FRAME && AUD_LOSS == DVBS2GPU_AUD_UNIT_LOSS, "public values");
static_assert(AUD_ACQUIRED == DVBS2GPU_AUD_ACQUIRED && AUD_RESYNC == DVBS2GPU_AUD_RESYNC && AUD_UNSYNCED == DVBS2GPU_AUD_UNSYNCED &&
              AUD_SPLIT_HEADER == DVBS2GPU_AUD_SPLIT_HEADER && AUD_CHANGE == DVBS2GPU_AUD_CHANGE, "public values");
static_assert(AUD_PACKET_ROWS == 28 && AUD_MAX_FRAME + AUD_WINDOW < (1 << 14), "rows per packet in a byte; a distance inside a frame in an entry");

struct AudCall { AudCallHead head; AudCnt cnt[AUD_SLOTS]; };

// behind phase D bit 18 of a start's word says that the start is valid; behind phase J bit 19 that it continues a chain
constexpr uint32_t AW_VALID = 1u << 18, AW_CONT = 1u << 19;
__device__ inline bool aud_invalid_start(uint32_t e) { return pw_start(e) && !(e & AW_VALID); }
__device__ inline bool aud_reset_front(uint32_t e) { return (e & PW_GAP) || (pw_counts(e) && pw_scr(e)); }
__device__ inline bool aud_reset_mark(uint32_t e) { return aud_reset_front(e) || aud_invalid_start(e); }
__device__ inline bool aud_event(uint32_t e) { return pw_start(e) || aud_reset_mark(e); }
constexpr uint16_t AUD_NO_LINK = 0xFFFF;
// an entry: the kind in bits 14-15, d or v below
constexpr int AE_UNLOCKED = 0, AE_CARRY = 1, AE_PREV = 2, AE_ACQ = 3;

// the framer's state along a walk.  next: relative to the slot's es_count before the call.  kind / ref: where it comes from -- CARRY;
// PREV, the last frame's position; ACQ, the start's sorted place
struct AudSt { bool locked; int64_t next; uint32_t params; int kind, ref; };

// what the kernel keeps in LDS beside the packets; a multiple of 16 bytes in front of them
struct alignas(16) AudShared {
    AudCnt cnt[AUD_SLOTS];
    AudState ss[AUD_SLOTS];                      // the slots' states before the call
    uint16_t place[AUD_SLOTS][AUD_WG];           // the counting sort's counts, then places; behind the sort link[]: an event's next event in sorted order
    int32_t tbase[AUD_WG];                       // the rows in front of a thread's run of input packets
    int64_t x0_next[AUD_SLOTS];                  // the exit of the walk in front of a slot's first event
    int32_t w[AUD_SLOTS], codec[AUD_SLOTS];
    int32_t start[AUD_SLOTS + 1];                // the slots' runs in sorted order
    int32_t first_ev[AUD_SLOTS];                 // a slot's first event, -1: none
    int32_t x0_locked[AUD_SLOTS];
    int32_t wsum[AUD_WG / 64];
    uint8_t ncc[AUD_SLOTS];                      // the slots' continuity bytes behind the call
    int64_t pos0;
};
static_assert(sizeof(AudShared) % 16 == 0 && sizeof(AudShared::place) == AUD_MAX_PACKETS * sizeof(uint16_t), "the packets behind it; an index per packet");
// dynamic LDS: AudShared, srt[max_packets], exs[max_packets + 2] (32 bits each), ent[], xit[] (16 bits per packet), rc[] (8 bits)
constexpr size_t aud_even(int max_packets) { return ((size_t)max_packets + 1) & ~(size_t)1; }
constexpr size_t aud_lds_bytes(int max_packets) {
    return sizeof(AudShared) + ((size_t)max_packets * 2 + 2) * sizeof(uint32_t) + 2 * aud_even(max_packets) * sizeof(uint16_t) + (((size_t)max_packets + 15) & ~(size_t)15);
}
static_assert(aud_lds_bytes(AUD_MAX_PACKETS) < 64 * 1024, "dynamic LDS of a workgroup");

__device__ inline void aud_flush(AudCnt* d, const AudCnt& a) {
#define AUD_ADD(f) if (a.f) atomicAdd(&d->f, a.f)
    AUD_ADD(es_bytes); AUD_ADD(bytes_unsynced); AUD_ADD(resets); AUD_ADD(pes_starts); AUD_ADD(pes_invalid); AUD_ADD(split_headers);
    AUD_ADD(frames); AUD_ADD(frame_bytes_total); AUD_ADD(samples_total); AUD_ADD(acquisitions); AUD_ADD(sync_losses); AUD_ADD(param_changes);
    AUD_ADD(unaligned_starts); AUD_ADD(bytes_unlocked);
#undef AUD_ADD
}
// the packet counters of phase C, per thread and slot run
__device__ inline void aud_flush_pk(AudCnt* d, const PwPk& a) {
    atomicAdd(&d->packets, a.packets);
    if (a.payload_bytes) atomicAdd(&d->payload_bytes, a.payload_bytes);
    if (a.duplicates) atomicAdd(&d->duplicates, a.duplicates);
    if (a.cc_errors) atomicAdd(&d->cc_errors, a.cc_errors);
    if (a.scrambled) atomicAdd(&d->scrambled_packets, a.scrambled);
    if (a.malformed) atomicAdd(&d->malformed_packets, a.malformed);
}
// counters summed per thread and slot run
struct AudAcc {
    AudCnt c; int slot; AudCnt* dst;
    __device__ AudAcc(AudCnt* d) : c(aud_cnt_zero()), slot(-1), dst(d) {}
    __device__ __forceinline__ void at(int s) { if (s != slot) { done(); c = aud_cnt_zero(); slot = s; } }
    __device__ __forceinline__ void done() { if (slot >= 0) aud_flush(&dst[slot], c); slot = -1; }
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
    AudShared& sh = *reinterpret_cast<AudShared*>(aud_lds);
    uint32_t* srt = reinterpret_cast<uint32_t*>(aud_lds + sizeof(AudShared));
    uint32_t* exs = srt + max_packets;               // a segment's length, then the exclusive prefix: the ES bytes of the call in front of it
    uint16_t* ent = reinterpret_cast<uint16_t*>(exs + max_packets + 2);     // the entries, per sorted packet
    uint16_t* xit = ent + aud_even(max_packets);                            // a valid start's exit: 0 unlocked, else 8 + next - the territory's end
    uint8_t* rc = reinterpret_cast<uint8_t*>(xit + aud_even(max_packets));  // rows per INPUT packet
    uint32_t* rec = exs;
    uint16_t* link = &sh.place[0][0];
    const int s = blockIdx.x, tid = threadIdx.x;
    int n = nbytes[s] / TSMON_TS;
    if (n > max_packets) n = max_packets;            // (the host has refused such a call)
    if (tid < AUD_SLOTS) {
        sh.w[tid] = watch[(size_t)s * AUD_SLOTS + tid];
        sh.codec[tid] = codec[(size_t)s * AUD_SLOTS + tid];
        sh.ss[tid] = state[(size_t)s * AUD_SLOTS + tid];
        sh.cnt[tid] = aud_cnt_zero();
        sh.first_ev[tid] = -1;
        sh.x0_locked[tid] = 0; sh.x0_next[tid] = 0;
    }
    for (int k = tid; k < n; k += AUD_WG) rc[k] = 0;
    if (tid == 0) sh.pos0 = pos[s];
    __syncthreads();
    const uint8_t* ts = in[s];
    // A: the watched packets, compacted in input order
    const int W = pw_compact<AUD_WG>(ts, n, sh.w, sh.wsum, rec);
    int nrows = 0;
    if (W > 0) {
        // B: the stable counting sort by slot
        int j0, j1;
        pw_sort<AUD_WG>(rec, srt, W, sh.place, sh.start, sh.wsum, &j0, &j1);
        // C: the continuity verdicts
        unsigned dupm, gapm;
        pw_verdicts(srt, j0, j1, sh.start, [&](int slot) { return sh.ss[slot].cc; }, sh.wsum, sh.ncc,
                    [&](int slot, const PwPk& pk) { aud_flush_pk(&sh.cnt[slot], pk); }, &dupm, &gapm);
        __syncthreads();                                         // every counter has been read: the verdicts take their bits
        AudAcc acc(sh.cnt);
        // D: the starts: valid or not, and their segments
        int last_start = -1;
        for (int j = j0; j < j1; ++j) {
            uint32_t e = pw_with_verdict(srt[j], dupm >> (j - j0) & 1, gapm >> (j - j0) & 1);
            if (pw_start(e)) {
                uint32_t w5[5];
                pw_load_start(ts, e, w5);
                const EsPlan pl = es_packet_plan(w5, pw_len(e), pw_scr(e), 1, false, false);
                if (pl.valid) e |= AW_VALID;
                exs[j] = (uint32_t)pl.seg_len;
                acc.at(pw_slot(e));
                aud_cnt_start(&acc.c, pl);
                last_start = j;
            }
            srt[j] = e;
            ent[j] = 0; xit[j] = 0; link[j] = AUD_NO_LINK;
        }
        __syncthreads();
        const int ls0 = ts_block_scan_max(last_start, sh.wsum);   // the last sorted start before the thread's run
        // the slot's synced bit behind its start ls (or none in this call)
        auto synced_at = [&](int slot, int ls) { return ls >= sh.start[slot] ? (srt[ls] & AW_VALID) != 0 : (sh.ss[slot].bits & AUD_SYNCED) != 0; };
        // E: the segment lengths, the reset marks, the events
        int lr0 = -1;
        {
            int ls = ls0, sum = 0, lr = -1, le = -1;
            for (int j = j0; j < j1; ++j) {
                const uint32_t e = srt[j];
                const int slot = pw_slot(e);
                acc.at(slot);
                int len = 0;
                if (pw_start(e)) { len = (int)exs[j]; ls = j; }
                else if (pw_counts(e) && !pw_scr(e)) {
                    if (synced_at(slot, ls)) len = pw_len(e); else acc.c.bytes_unsynced += pw_len(e);
                }
                exs[j] = (uint32_t)len;
                sum += len;
                acc.c.es_bytes += len;
                if (aud_reset_mark(e)) { lr = j; ++acc.c.resets; }
                if (aud_event(e)) le = j;
            }
            int total;
            int at = ts_block_scan<AUD_WG>(sum, sh.wsum, &total);
            lr0 = ts_block_scan_max(lr, sh.wsum);                // the last sorted packet with a reset mark before the run,
            le = ts_block_scan_max(le, sh.wsum);                 // and the last event
            for (int j = j0; j < j1; ++j) {
                const int len = (int)exs[j];
                exs[j] = (uint32_t)at; at += len;
                const uint32_t e = srt[j];
                if (aud_event(e)) {
                    if (le >= sh.start[pw_slot(e)]) link[le] = (uint16_t)j; else sh.first_ev[pw_slot(e)] = j;
                    le = j;
                }
            }
            if (tid == 0) exs[W] = (uint32_t)total;
        }
        __syncthreads();
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
            if (pw_start(e) && (e & AW_VALID)) {
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
                if (aud_reset_mark(e)) st.locked = false;                                 // (a reset in front of a valid start: it acquires)
                if (pw_start(e) && (e & AW_VALID)) {
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
        // G: the rows' places in input order, the slot's last row-bearing packet, the rows and the new states
        const int chunk = (n + AUD_WG - 1) / AUD_WG;
        {
            int k0, k1; ts_thread_run(n, AUD_WG, &k0, &k1);
            int sum = 0;
            for (int k = k0; k < k1; ++k) sum += rc[k];
            sh.tbase[tid] = ts_block_scan<AUD_WG>(sum, sh.wsum, &nrows);
        }
        int lp = ts_block_scan_max(last_row, sh.wsum);
        __syncthreads();
        AudRow* rows = rows_g + (size_t)s * max_rows;
        int lr = lr0, ls = ls0;
        // the slot's lost bit where its last row-bearing packet is p and its last reset mark r (both before the place, -1 or another slot's: none)
        auto lost_behind = [&](int slot, int p, int r) {
            const int head = sh.start[slot];
            if (p >= head) return r > p || (r == p && aud_invalid_start(srt[p]));
            return (sh.ss[slot].bits & AUD_LOST) != 0 || r >= head;
        };
        for (int j = j0; j < j1; ++j) {
            const uint32_t e = srt[j];
            const int slot = pw_slot(e), k = pw_k(e), head = sh.start[slot];
            const AudRun r = run_of(slot);
            const int nr = rc[k];
            if (nr) {
                bool lost = aud_reset_front(e) || lost_behind(slot, lp, lr);
                int rank = sh.tbase[k / chunk];
                for (int q = (k / chunk) * chunk; q < k; ++q) rank += rc[q];
                if (pw_start(e)) {
                    uint32_t w5[5];
                    pw_load_start(ts, e, w5);
                    const EsPlan pl = es_packet_plan(w5, pw_len(e), pw_scr(e), 1, false, false);
                    if (rank < max_rows) rows[rank] = aud_pes_row(sh.w[slot], slot, k, pl, sh.ss[slot].es_count + (uint64_t)r.pos(j), lost);
                    lost = false;
                    ++rank;
                }
                if (nr > pw_start(e)) {
                    AudSt st = state_in(r, slot, j);
                    AudCnt none = aud_cnt_zero();
                    walk_packet(r, slot, j, st, &none, rows, rank, max_rows, lost, nullptr);
                }
                lp = j;
            }
            if (aud_reset_mark(e)) lr = j;
            if (pw_start(e)) ls = j;
            if (j == r.end - 1) {
                AudState nx = sh.ss[slot];
                AudSt st = state_in(r, slot, j);
                AudCnt none = aud_cnt_zero();
                walk_packet(r, slot, j, st, &none, nullptr, 0, 0, false, nullptr);
                const int total = r.pos(r.end);
                const uint32_t sn = lr >= head ? (uint32_t)(total - r.pos(lr)) : (uint32_t)nx.have + (uint32_t)total;
                const int have = sn < 7 ? (int)sn : 7;
                nx.tail = r.bytes(total - have, have); nx.have = (uint8_t)have;
                nx.es_count += (uint64_t)total;
                nx.cc = sh.ncc[slot];
                nx.bits = (uint8_t)((synced_at(slot, ls) ? AUD_SYNCED : 0) | (lost_behind(slot, lp, lr) ? AUD_LOST : 0) | (st.locked ? AUD_LOCKED : 0));
                if (st.locked) { nx.next = sh.ss[slot].es_count + (uint64_t)st.next; nx.params = st.params; }
                state[(size_t)s * AUD_SLOTS + slot] = nx;
            }
        }
        __syncthreads();
    }
    if (tid < AUD_SLOTS) call[s].cnt[tid] = sh.cnt[tid];
    if (tid == 0) {
        call[s].head = AudCallHead{nrows, {0, 0, 0}};
        pos[s] = sh.pos0 + n;
    }
}

}  // namespace s2

// the host half is the watched-PID bank's (watch_bank.h); here what is the bank's own
struct AudBankD {
    static constexpr int SLOTS = AUD_SLOTS, MAX_PACKETS = AUD_MAX_PACKETS;
    typedef AudState State; typedef AudRow Row; typedef AudCall Call; typedef AudHostStream HostStream;
    typedef dvbs2gpu_aud_stats Stats; typedef dvbs2gpu_aud_stream_stats StreamStats;
    static constexpr int SUMS = AUD_COUNTERS;          // every word of dvbs2gpu_aud_stats is a counter
    static constexpr StreamStats NO_STREAM_STATS = {};
    typedef int32_t Config;                            // the codec, per slot
    static constexpr int CONFIGS = AUD_SLOTS;
    static constexpr Config NO_CONFIG = AUD_NONE;
    static constexpr const char *BANK = "audio bank: ", *CNAME = "dvbs2gpu_aud", *ALLOC = "hipMalloc(aud)";

    // one stream's call into its statistics; `n` packets came
    static void account(WatchBank<AudBankD>& b, int i, int n, const AudCallHead& head, const AudCnt* c) {
        dvbs2gpu_aud_stream_stats& ss = b.sstats[i];
        for (int s = 0; s < AUD_SLOTS; ++s) {
            if (!c[s].packets) continue;                   // (no packet of the slot's PID came: every counter is 0)
            const int32_t* a = reinterpret_cast<const int32_t*>(&c[s]);
            int64_t* d = reinterpret_cast<int64_t*>(&b.stats[(size_t)i * AUD_SLOTS + s]);
            for (int k = 0; k < AUD_COUNTERS; ++k) d[k] += a[k];
        }
        ss.packets += n;
        if (head.rows > b.max_rows) ss.rows_dropped += head.rows - b.max_rows;
        b.total[i] = head.rows;
        b.nrows[i] = head.rows < b.max_rows ? head.rows : b.max_rows;
    }
    static void launch(WatchBank<AudBankD>& b, const TsBankArgs& a, hipStream_t st) {
        const size_t lds = aud_lds_bytes(b.max_packets);       // <= 63.3 KiB
        hipLaunchKernelGGL(aud_kernel, dim3(b.nstreams), dim3(AUD_WG), lds, st, a.in(b.d_args), a.nbytes(b.d_args), b.max_packets, b.max_rows, b.d_watch, b.d_cfg, b.d_state,
                           b.d_pos, b.d_rows, b.d_call);
    }
    static void fix_stream_stats(StreamStats*) {}
};
struct dvbs2gpu_aud : WatchBank<AudBankD> {};

extern "C" {

void dvbs2gpu_aud_destroy(dvbs2gpu_aud* b) { delete b; }
int dvbs2gpu_aud_create(dvbs2gpu_ctx* ctx, int nstreams, int max_packets, int max_rows, dvbs2gpu_aud** out) { return watch_create(true, ctx, nstreams, max_packets, max_rows, out); }
int dvbs2gpu_aud_create_host(int nstreams, int max_packets, int max_rows, dvbs2gpu_aud** out) { return watch_create(false, nullptr, nstreams, max_packets, max_rows, out); }
int dvbs2gpu_aud_reset(dvbs2gpu_aud* b) { return watch_reset(b); }

int dvbs2gpu_aud_set_watch(dvbs2gpu_aud* b, int stream, int slot, int pid, int codec) {
    if (!watch_slot_ok(b, stream, slot, pid)) return DVBS2GPU_ERR_ARG;
    if (pid >= 0 && (codec < AUD_MPA || codec > AUD_AC3)) { g_err = "audio bank: the codec is DVBS2GPU_AUD_MPA, _ADTS or _AC3"; return DVBS2GPU_ERR_ARG; }
    if (const int e = watch_set_watch(b, stream, slot, pid)) return e;
    const size_t at = (size_t)stream * AUD_SLOTS + slot;
    b->cfg[at] = pid >= 0 ? codec : AUD_NONE;
    if (b->ctx) return watch_upload_config(b, at);
    b->host[stream].codec[slot] = b->cfg[at];
    return 0;
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
