// T2-MI bank (own extension; include/dvbs2gpu.h): the T2-MI packets of a PID of each of `nstreams` transport streams
// in HBM, reassembled, checked (CRC-32, packet count) and the BBFRAMEs of the chosen PLP laid back to back for the mode-adaptation
// packetiser.  Every rule is in t2mi_rules.h, whose T2miHostStream is the sequential definition, the host bank and the kernels'
// yardstick.  The kernels, the handle and the call are the datagram bank's (dgram_bank.h, shared with mpe.hip and ule.hip), here
// instantiated with T2miRules: a 6-byte header with payload_bits in bytes 4 and 5, no stuffing, no bad length, the pointer slack
// counted; the BBFRAME is the packet's bytes from 9 on.  This file holds what is the bank's own: the layout checks, the description
// with its phases D and D', the watch and the list of the delivered BBFRAMEs' sizes.
//     D  one wave per row: each lane takes the CRC of one PIECE of the packet (its bytes in one TS payload, at most 184; 46 pieces at
//        8202 bytes, 64 a round) from a zero register, reading the bytes from the TS payloads where they lie (a gathered copy of
//        4 x 8202 bytes beside the packet list would not leave two workgroups per CU their LDS), the registers are shifted to the
//        packet's end and summed (reasm_wave_crc with one lane to a piece); lane 0 reads the nine bytes the row needs.
//     D' COUNT_ERROR: "the last valid row before mine" is an exclusive maximum scan over the rows.
#include "dgram_bank.h"
#include "t2mi_rules.h"

using namespace s2;

static_assert(sizeof(T2miRow) == sizeof(dvbs2gpu_t2mi_row) && sizeof(T2miRow) == 32, "row layout");
static_assert(sizeof(T2miLayout) == sizeof(dvbs2gpu_t2mi_layout), "layout layout");
static_assert(sizeof(T2miCnt) == T2MI_NCNT * sizeof(int32_t), "counter order");
static_assert(sizeof(dvbs2gpu_t2mi_stats) == T2MI_NCNT * sizeof(int64_t), "stats order");
static_assert(T2MI.max_packet_bytes <= T2MI_BUF && T2MI.max_packet_bytes < (1 << 17), "crc32m_xpow takes 17 bits of length");
static_assert(T2S_LAST_COUNT < DGRAM_OWN, "the packet-count pair lies in the slot's own bytes");

struct T2miBankDesc : T2miRules {
    typedef dvbs2gpu_t2mi_stats Stats;
    static constexpr const char *BANK = "T2-MI bank: ", *CNAME = "dvbs2gpu_t2mi", *ALLOC = "hipMalloc(t2mi)", *NOUN = "BBFRAMEs";
    static constexpr bool OWN_ROWS = true, SIZE_LIST = true;         // phases D and D' below; dvbs2gpu_t2mi_get_frame_bytes
    template <typename F>
    __device__ static void wave_row(const ReasmRec& q, const ReasmView<F>& v, int lane, T2miRow* out) {
        // A lane per PIECE (the packet's bytes in one TS payload, at most 184), 64 pieces a round: the walk only notes the lane's
        // piece, and the CRC loops of all lanes then run side by side.  (A lane per 64th of the packet, taken inside the walk,
        // has two or three lanes at work in each of the packet's pieces: 26 ms per call of tools/t2mi_bench.py)
        const int total = q.total;
        const uint32_t x = reasm_wave_crc<1>(q, v, total, lane);
        if (lane == 0) {
            unsigned long long h8 = 0;
            unsigned h9 = 0;
            reasm_pieces(q, v, 9, [&](int pos, const uint8_t* src, int len) {
                for (int i = 0; i < len; ++i) {
                    const int at = pos + i;
                    if (at < 8) h8 |= (unsigned long long)src[i] << (8 * at); else h9 = src[i];
                }
            });
            auto rd = [&](int i) { return i < 8 ? (unsigned)(h8 >> (8 * i) & 255) : h9; };
            *out = t2mi_row_fields(rd, total, x == 0, q.j0 < 0 ? -1 : wa_k(v.wa[q.j0]), wa_k(v.wa[q.j1]));
        }
    }
    // Whole workgroup.  t2mi_sequence over the rows in order, each thread from the last valid row before its run; the counters a row
    // steps (t2mi_account) as one sum per thread; the thread of the last run knows the last valid row of the call
    __device__ static void sequence_pass(T2miRow* rows, int nrows, const DgramDevSlot& ss, DgramDevSlot* nss, int* cnt, int* wsum) {
        int r0, r1; ts_thread_run(nrows, DGRAM_WG, &r0, &r1);
        int lastv = -1;
        for (int r = r0; r < r1; ++r) if (!(rows[r].flags & T2MI_CRC_ERROR)) lastv = r;
        const int prev = ts_block_scan_max(lastv, wsum);
        int has = prev >= 0 ? 1 : ss.own[T2S_HAS_COUNT], last = prev >= 0 ? rows[prev].packet_count : ss.own[T2S_LAST_COUNT];
        int c_crc = 0, c_cnt = 0, c_bb = 0, c_bad = 0;
        for (int r = r0; r < r1; ++r) {
            const T2miRow row = rows[r];
            if (row.flags & T2MI_CRC_ERROR) { ++c_crc; continue; }
            if (has && row.packet_count != ((last + 1) & 255)) { rows[r].flags = row.flags | T2MI_COUNT_ERROR; ++c_cnt; }
            has = 1; last = row.packet_count;
            c_bb += (row.flags & T2MI_BBFRAME) != 0; c_bad += (row.flags & T2MI_BAD_PAYLOAD) != 0;
        }
        if (c_crc) atomicAdd(&cnt[T2C_CRC], c_crc);
        if (c_cnt) atomicAdd(&cnt[T2C_COUNT], c_cnt);
        if (c_bb) atomicAdd(&cnt[T2C_BB], c_bb);
        if (c_bad) atomicAdd(&cnt[T2C_BADPAY], c_bad);
        if (threadIdx.x == 0) cnt[T2C_T2MI] = nrows;
        if (threadIdx.x == DGRAM_WG - 1 && (lastv >= 0 || prev >= 0)) {
            nss->own[T2S_HAS_COUNT] = 1; nss->own[T2S_LAST_COUNT] = rows[lastv >= 0 ? lastv : prev].packet_count;
        }
    }
};
struct dvbs2gpu_t2mi : DgramBank<T2miBankDesc> {};

extern "C" {

void dvbs2gpu_t2mi_destroy(dvbs2gpu_t2mi* b) { delete b; }
int dvbs2gpu_t2mi_create(dvbs2gpu_ctx* ctx, int nstreams, int max_packets, int max_rows, dvbs2gpu_t2mi** out) { return dgram_create(true, ctx, nstreams, max_packets, max_rows, out); }
int dvbs2gpu_t2mi_create_host(int nstreams, int max_packets, int max_rows, dvbs2gpu_t2mi** out) { return dgram_create(false, nullptr, nstreams, max_packets, max_rows, out); }
int dvbs2gpu_t2mi_reset(dvbs2gpu_t2mi* b) { return dgram_reset(b); }

int dvbs2gpu_t2mi_get_layout(dvbs2gpu_t2mi_layout* h_out) {
    if (!h_out) return DVBS2GPU_ERR_ARG;
    memcpy(h_out, &T2MI, sizeof(T2MI));
    return 0;
}

int dvbs2gpu_t2mi_set_watch(dvbs2gpu_t2mi* b, int stream, int slot, int pid, int plp) {
    if (!b || !b->slot_ok(stream, slot)) return DVBS2GPU_ERR_ARG;
    size_t at;
    if (plp < -1 || plp > 255 || !dgram_watch_args_ok(b, stream, slot, pid, &at)) {
        last_error() = "T2-MI bank: a slot's PID is 0..0x1FFE (-1 empties the slot), its PLP 0..255 or -1 for every PLP";
        return DVBS2GPU_ERR_ARG;
    }
    return b->set_watch(at, T2miWatch{pid, pid < 0 ? -1 : plp});
}

int dvbs2gpu_t2mi_process_batch(dvbs2gpu_t2mi* b, const uint8_t* const* d_ts, const int* nbytes, uint8_t* const* d_out, int cap, int* out_bytes, int* out_rows,
                                void* stream) {
    return dgram_process_batch(b, d_ts, nbytes, d_out, cap, out_bytes, out_rows, stream);
}
int dvbs2gpu_t2mi_work(dvbs2gpu_t2mi* b, int stream, int slot, const uint8_t* h_ts, int nbytes, uint8_t* h_out, int cap) {
    return dgram_work(b, stream, slot, h_ts, nbytes, h_out, cap);
}
int dvbs2gpu_t2mi_get_needed(dvbs2gpu_t2mi* b, int stream, int slot, int* bytes, int* rows) { return dgram_get_needed(b, stream, slot, bytes, rows); }
int dvbs2gpu_t2mi_get_stats(dvbs2gpu_t2mi* b, int stream, int slot, dvbs2gpu_t2mi_stats* h_out) { return dgram_get_stats(b, stream, slot, h_out); }
int dvbs2gpu_t2mi_get_row_table(dvbs2gpu_t2mi* b, int stream, int slot, dvbs2gpu_t2mi_row* h_rows, int cap, int* n) {
    return dgram_get_row_table(b, stream, slot, h_rows, cap, n);
}
int dvbs2gpu_t2mi_get_row_table_device(dvbs2gpu_t2mi* b, int stream, int slot, const dvbs2gpu_t2mi_row** d_rows, int* n) {
    return dgram_get_row_table_device(b, stream, slot, d_rows, n);
}

int dvbs2gpu_t2mi_get_frame_bytes(dvbs2gpu_t2mi* b, int stream, int slot, int* h_sizes, int cap, int* n) {
    if (!b || !b->slot_ok(stream, slot) || !n || cap < 0 || (cap > 0 && !h_sizes)) return DVBS2GPU_ERR_ARG;
    const int g = stream * T2MI_SLOTS + slot;
    const int k = (*n = b->ndelivered[g]) < cap ? *n : cap;
    if (k <= 0) return 0;
    if (!b->ctx) {
        int i = 0;
        for (const T2miRow& r : b->host[g].rows)
            if (r.offset >= 0 && i < k) h_sizes[i++] = r.bbframe_bytes;
        return 0;
    }
    HIP_TRY(hipSetDevice(b->ctx->device));
    HIP_TRY(hipMemcpy(h_sizes, dgram_size_list<T2miRow>(b->d_rows, (size_t)b->nstreams * T2MI_SLOTS, b->max_rows, g), k * sizeof(int), hipMemcpyDeviceToHost));
    return 0;
}

}  // extern "C"
