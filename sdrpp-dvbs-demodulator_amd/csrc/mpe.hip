// MPE bank (own extension; include/dvbs2gpu.h): the DSM-CC datagram_sections (Multi-Protocol Encapsulation, EN 301 192)
// of a PID of each of `nstreams` transport streams in HBM, reassembled, checked (CRC-32, MAC filter, LLC/SNAP, IP header) and their IP
// datagrams laid back to back per slot.  Every rule is in mpe_rules.h, whose MpeHostStream is the sequential definition, the host bank
// and the kernels' yardstick.  The kernels, the handle and the call are the datagram bank's (dgram_bank.h, shared with ule.hip and
// t2mi.hip), here instantiated with MpeRules: a 3-byte header with section_length in bytes 1 and 2, and in phase D up to 84 bytes
// decide a row (MPE header, LLC/SNAP, an IPv4 header with options, the ports) and the CRC-32 is taken only where mpe_takes_crc says
// so; the datagram is the section's bytes from 12 or 20 on.  This file holds what is the bank's own: the layout checks, the description
// and the watch.
#include "dgram_bank.h"
#include "mpe_rules.h"

using namespace s2;

static_assert(sizeof(MpeRow) == sizeof(dvbs2gpu_mpe_row) && sizeof(MpeRow) == 48, "row layout");
static_assert(sizeof(MpeLayout) == sizeof(dvbs2gpu_mpe_layout), "layout layout");
static_assert(sizeof(MpeCnt) == MPE_NCNT * sizeof(int32_t), "counter order");
static_assert(sizeof(dvbs2gpu_mpe_stats) == MPE_NCNT * sizeof(int64_t), "stats order");
static_assert(sizeof(MpeWatch) == 16, "watch layout");
static_assert(MPE.max_section_bytes <= MPE_BUF && MPE.max_section_bytes < (1 << 17), "crc32m_xpow takes 17 bits of length");
static_assert(MPE.head_bytes <= REASM_HEAD && MPE.head_bytes == MPE.mpe_header_bytes + MPE.llc_snap_bytes + 60 + 4, "the head gather holds what a row reads");

struct MpeBankDesc : MpeRules, DgramIpBank {
    typedef dvbs2gpu_mpe_stats Stats;
    static constexpr const char *BANK = "MPE bank: ", *CNAME = "dvbs2gpu_mpe", *ALLOC = "hipMalloc(mpe)";
};
struct dvbs2gpu_mpe : DgramBank<MpeBankDesc> {};

extern "C" {

void dvbs2gpu_mpe_destroy(dvbs2gpu_mpe* b) { delete b; }
int dvbs2gpu_mpe_create(dvbs2gpu_ctx* ctx, int nstreams, int max_packets, int max_rows, dvbs2gpu_mpe** out) { return dgram_create(true, ctx, nstreams, max_packets, max_rows, out); }
int dvbs2gpu_mpe_create_host(int nstreams, int max_packets, int max_rows, dvbs2gpu_mpe** out) { return dgram_create(false, nullptr, nstreams, max_packets, max_rows, out); }
int dvbs2gpu_mpe_reset(dvbs2gpu_mpe* b) { return dgram_reset(b); }

int dvbs2gpu_mpe_get_layout(dvbs2gpu_mpe_layout* h_out) {
    if (!h_out) return DVBS2GPU_ERR_ARG;
    memcpy(h_out, &MPE, sizeof(MPE));
    return 0;
}

int dvbs2gpu_mpe_set_watch(dvbs2gpu_mpe* b, int stream, int slot, int pid, const uint8_t mac_value[6], const uint8_t mac_mask[6]) {
    size_t at;
    if (!dgram_watch_args_ok(b, stream, slot, pid, &at)) return DVBS2GPU_ERR_ARG;
    MpeWatch w = MpeRules::NO_WATCH;
    w.pid = pid;
    if (pid >= 0 && mac_value) memcpy(w.mac_value, mac_value, 6);
    if (pid >= 0 && mac_mask) memcpy(w.mac_mask, mac_mask, 6);
    return b->set_watch(at, w);
}

int dvbs2gpu_mpe_process_batch(dvbs2gpu_mpe* b, const uint8_t* const* d_ts, const int* nbytes, uint8_t* const* d_out, int cap, int* out_bytes, int* out_rows,
                               void* stream) {
    return dgram_process_batch(b, d_ts, nbytes, d_out, cap, out_bytes, out_rows, stream);
}
int dvbs2gpu_mpe_work(dvbs2gpu_mpe* b, int stream, int slot, const uint8_t* h_ts, int nbytes, uint8_t* h_out, int cap) {
    return dgram_work(b, stream, slot, h_ts, nbytes, h_out, cap);
}
int dvbs2gpu_mpe_get_needed(dvbs2gpu_mpe* b, int stream, int slot, int* bytes, int* rows) { return dgram_get_needed(b, stream, slot, bytes, rows); }
int dvbs2gpu_mpe_get_stats(dvbs2gpu_mpe* b, int stream, int slot, dvbs2gpu_mpe_stats* h_out) { return dgram_get_stats(b, stream, slot, h_out); }
int dvbs2gpu_mpe_get_row_table(dvbs2gpu_mpe* b, int stream, int slot, dvbs2gpu_mpe_row* h_rows, int cap, int* n) {
    return dgram_get_row_table(b, stream, slot, h_rows, cap, n);
}
int dvbs2gpu_mpe_get_row_table_device(dvbs2gpu_mpe* b, int stream, int slot, const dvbs2gpu_mpe_row** d_rows, int* n) {
    return dgram_get_row_table_device(b, stream, slot, d_rows, n);
}

}  // extern "C"
