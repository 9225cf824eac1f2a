// The sequential form that the banks share which deliver the payloads of length-prefixed units of one PID -- IP datagrams (mpe_rules.h:
// MPE sections; ule_rules.h: ULE SNDUs) or BBFRAMEs (t2mi_rules.h: T2-MI packets) -- stated once: a unit's bytes as
// the source of the row rules, and one slot of one stream as a complete reassembler on top of ts_reasm_run.  DgramHostStream<R>::run IS
// each bank's definition, the host bank and the kernels' yardstick.  R is the bank's rules (MpeRules, UleRules, T2miRules), and names
// only what differs between the banks:
//   Row, Watch, Cnt, NO_WATCH         the row, a slot's watch record and the empty one, the counters of one call (32-bit, in C_* order)
//   BUF                               the bytes a slot buffers: the longest unit
//   HEADER, LEN_A, LEN_B              a unit's length is known once HEADER bytes are in, from bytes LEN_A and LEN_B: total(a, b), -1: bad
//   STUFFING                          the byte in a unit's first place that ends a packet's chain (0xFF), -1: the bank has none
//   C_DROPPED, C_BAD_UNIT, C_SLACK    the counters of a dropped unit, a bad length and slack (-1: the bank does not count it)
//   C_DELIVERED, C_BYTES              the counters of the delivered payloads and their bytes
//   takes_crc(b0, b1, total)          is the CRC-32 of an emitted unit taken
//   row_fields<Src>(src, total, crc_ok, watch, first_packet, last_packet), account(flags, add)
//   sequence(row, own)                what a row does to the bytes the bank carries from unit to unit (DgramState::own) and they to it,
//                                     between row_fields and account; MPE and ULE carry nothing
//   delivers(row, watch), bytes_of(row), ip_at(row)   is the row's payload delivered; its bytes; where it starts in the unit
// Standard headers and ts_reasm_rules.h only: the host tests compile this file with a plain C++ compiler.
#pragma once
#include "ts_reasm_rules.h"

#include <cstring>
#include <vector>

namespace s2 {

// a unit's bytes in memory, the reductions as loops
struct DgramHostSrc {
    const uint8_t* b;
    unsigned rd(int i) const { return b[i]; }
    template <typename Fn> bool any(int n, Fn f) const { for (int k = 0; k < n; ++k) if (f(k)) return true; return false; }
    template <typename Fn> unsigned sum(int n, Fn f) const { unsigned v = 0; for (int k = 0; k < n; ++k) v += f(k); return v; }
};

constexpr int DGRAM_OWN = 3;                               // (the device slot's spare bytes: DgramDevSlot, dgram_bank.h)
template <int BUF>
struct DgramState {
    uint8_t cont = 0, own[DGRAM_OWN] = {};                 // tsmon_step's byte; what the bank carries from unit to unit (R::sequence)
    int fill = 0;                                          // bytes buffered; 0: no unit is open
    uint8_t buf[BUF];
};

// one slot of one stream: a complete reassembler
template <typename R>
struct DgramHostStream {
    typedef DgramState<R::BUF> State;
    typedef typename R::Cnt Cnt;
    typename R::Watch watch = R::NO_WATCH;
    State st;
    int first_packet = -1;                                 // of the open unit, in this call
    // of the last call
    std::vector<typename R::Row> rows;
    std::vector<uint8_t> bytes;
    Cnt cnt = {};

    void clear() { st = State(); rows.clear(); bytes.clear(); }
    int32_t& counter(int c) { return reinterpret_cast<int32_t*>(&cnt)[c]; }
    int unit_total() const { return R::total(st.buf[R::LEN_A], st.buf[R::LEN_B]); }    // (once HEADER bytes are in)

    void drop() {
        if (st.fill > 0) ++counter(R::C_DROPPED);
        st.fill = 0;
    }
    void emit(int k, bool want_bytes) {
        const uint8_t* b = st.buf;
        const int total = st.fill;
        const bool crc_ok = !R::takes_crc(b[0], b[1], total) || ts_crc32(b, total) == 0;
        typename R::Row r = R::template row_fields<DgramHostSrc>(DgramHostSrc{b}, total, crc_ok, watch, first_packet, k);
        R::sequence(r, st.own);
        R::account(r.flags, [&](int c) { ++counter(c); });
        if (want_bytes && R::delivers(r, watch)) {
            const uint8_t* d = b + R::ip_at(r);
            r.offset = (int32_t)bytes.size();
            bytes.insert(bytes.end(), d, d + R::bytes_of(r));
            ++counter(R::C_DELIVERED); counter(R::C_BYTES) += R::bytes_of(r);
        }
        rows.push_back(r);
    }
    // n bytes for the slot's unit (open, or starting with them): stops behind the unit's last byte.  true: it was emitted; a bad length
    // forgets the header and is false too
    bool feed(const uint8_t* b, int n, int* used, int k, bool want_bytes) {
        int i = 0;
        bool done = false;
        while (i < n) {
            if (st.fill < R::HEADER) {
                st.buf[st.fill++] = b[i++];
                if (st.fill < R::HEADER) continue;
                if (R::C_BAD_UNIT >= 0 && unit_total() < 0) { ++counter(R::C_BAD_UNIT); st.fill = 0; break; }
            } else {
                const int left = unit_total() - st.fill, take = n - i < left ? n - i : left;
                memcpy(st.buf + st.fill, b + i, (size_t)take);
                st.fill += take; i += take;
            }
            if (st.fill == unit_total()) { emit(k, want_bytes); st.fill = 0; done = true; break; }
        }
        *used = i;
        return done;
    }
    // what the shared packet loop asks of a format (ts_reasm_rules.h): one slot; 0xFF in a unit's first place -- the section banks'
    // stuffing byte, ULE's End Indicator 0xFFFF and its 0xFF padding alike -- ends the packet's chain; T2-MI has no stuffing
    struct Format {
        DgramHostStream& h;
        int slot_of(int pid) const { return pid == h.watch.pid ? 0 : -1; }
        State& state(int) { return h.st; }
        Cnt& cnt(int) { return h.cnt; }
        void drop(int) { h.drop(); }
        bool feed(int, const uint8_t* b, int n, int* used, int k, bool want_bytes) { return h.feed(b, n, used, k, want_bytes); }
        void begin(int, int k) { h.first_packet = k; }
        void slack(int) { if (R::C_SLACK >= 0) ++h.counter(R::C_SLACK); }
        bool stuffing(uint8_t b) const { return R::STUFFING >= 0 && b == R::STUFFING; }
    };
    // one call: n packets.  The caller keeps a copy of `st` if the call may have to be undone.
    void run(const uint8_t* ts, int n, bool want_bytes) {
        rows.clear(); bytes.clear();
        cnt = Cnt{};
        first_packet = -1;
        if (watch.pid >= 0) ts_reasm_run(Format{*this}, ts, n, want_bytes);
    }
};

}  // namespace s2
