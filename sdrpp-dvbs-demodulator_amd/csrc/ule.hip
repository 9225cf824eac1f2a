// ULE bank (own extension; include/dvbs2gpu.h): the SNDUs (Unidirectional Lightweight Encapsulation, RFC 4326) of a
// PID of each of `nstreams` transport streams in HBM, reassembled, checked (CRC-32, NPA filter, extension headers, bridged frames, IP
// header) and their IP datagrams laid back to back per slot.  Every rule is in ule_rules.h, whose UleHostStream is the sequential
// definition, the host bank and the kernels' yardstick.  The kernels, the handle and the call are the datagram bank's (dgram_bank.h,
// shared with mpe.hip and t2mi.hip), here instantiated with UleRules: the length is known from the first two bytes, and in phase D all
// 128 leading bytes can decide a row (base header, NPA, 40 bytes of optional headers, a bridged MAC header, an IPv4 header with options, the ports)
// and the CRC-32 is always taken: there is no unchecked SNDU.  The extension-header walk of ule_row_fields is data dependent, but every
// lane walks the same chain from the same shuffled bytes: no divergence.  The datagram is the SNDU's bytes from ule_ip_at(row) on.
// This file holds what is the bank's own: the layout checks, the description and the watch.
#include "dgram_bank.h"
#include "ule_rules.h"

using namespace s2;

static_assert(sizeof(UleRow) == sizeof(dvbs2gpu_ule_row) && sizeof(UleRow) == 48, "row layout");
static_assert(sizeof(UleLayout) == sizeof(dvbs2gpu_ule_layout), "layout layout");
static_assert(sizeof(UleCnt) == ULE_NCNT * sizeof(int32_t), "counter order");
static_assert(sizeof(dvbs2gpu_ule_stats) == ULE_NCNT * sizeof(int64_t), "stats order");
static_assert(sizeof(UleWatch) == 20, "watch layout");
static_assert(ULE.max_sndu_bytes <= ULE_BUF && ULE.max_sndu_bytes < (1 << 17), "crc32m_xpow takes 17 bits of length");
static_assert(ULE.head_bytes == REASM_HEAD && REASM_HEAD == 2 * 64, "the head gather, two bytes per lane, holds exactly what a row reads");

struct UleBankDesc : UleRules, DgramIpBank {
    typedef dvbs2gpu_ule_stats Stats;
    static constexpr const char *BANK = "ULE bank: ", *CNAME = "dvbs2gpu_ule", *ALLOC = "hipMalloc(ule)";
};
struct dvbs2gpu_ule : DgramBank<UleBankDesc> {};

extern "C" {

void dvbs2gpu_ule_destroy(dvbs2gpu_ule* b) { delete b; }
int dvbs2gpu_ule_create(dvbs2gpu_ctx* ctx, int nstreams, int max_packets, int max_rows, dvbs2gpu_ule** out) { return dgram_create(true, ctx, nstreams, max_packets, max_rows, out); }
int dvbs2gpu_ule_create_host(int nstreams, int max_packets, int max_rows, dvbs2gpu_ule** out) { return dgram_create(false, nullptr, nstreams, max_packets, max_rows, out); }
int dvbs2gpu_ule_reset(dvbs2gpu_ule* b) { return dgram_reset(b); }

int dvbs2gpu_ule_get_layout(dvbs2gpu_ule_layout* h_out) {
    if (!h_out) return DVBS2GPU_ERR_ARG;
    memcpy(h_out, &ULE, sizeof(ULE));
    return 0;
}

int dvbs2gpu_ule_set_watch(dvbs2gpu_ule* b, int stream, int slot, int pid, const uint8_t npa_value[6], const uint8_t npa_mask[6], int accept_unaddressed) {
    size_t at;
    if (!dgram_watch_args_ok(b, stream, slot, pid, &at)) return DVBS2GPU_ERR_ARG;
    UleWatch w = UleRules::NO_WATCH;
    w.pid = pid;
    if (pid >= 0 && npa_value) memcpy(w.npa_value, npa_value, 6);
    if (pid >= 0 && npa_mask) memcpy(w.npa_mask, npa_mask, 6);
    if (pid >= 0) w.accept_unaddressed = accept_unaddressed != 0;
    return b->set_watch(at, w);
}

int dvbs2gpu_ule_process_batch(dvbs2gpu_ule* b, const uint8_t* const* d_ts, const int* nbytes, uint8_t* const* d_out, int cap, int* out_bytes, int* out_rows,
                               void* stream) {
    return dgram_process_batch(b, d_ts, nbytes, d_out, cap, out_bytes, out_rows, stream);
}
int dvbs2gpu_ule_work(dvbs2gpu_ule* b, int stream, int slot, const uint8_t* h_ts, int nbytes, uint8_t* h_out, int cap) {
    return dgram_work(b, stream, slot, h_ts, nbytes, h_out, cap);
}
int dvbs2gpu_ule_get_needed(dvbs2gpu_ule* b, int stream, int slot, int* bytes, int* rows) { return dgram_get_needed(b, stream, slot, bytes, rows); }
int dvbs2gpu_ule_get_stats(dvbs2gpu_ule* b, int stream, int slot, dvbs2gpu_ule_stats* h_out) { return dgram_get_stats(b, stream, slot, h_out); }
int dvbs2gpu_ule_get_row_table(dvbs2gpu_ule* b, int stream, int slot, dvbs2gpu_ule_row* h_rows, int cap, int* n) {
    return dgram_get_row_table(b, stream, slot, h_rows, cap, n);
}
int dvbs2gpu_ule_get_row_table_device(dvbs2gpu_ule* b, int stream, int slot, const dvbs2gpu_ule_row** d_rows, int* n) {
    return dgram_get_row_table_device(b, stream, slot, d_rows, n);
}

}  // extern "C"
