// Shared by the two BBFRAME -> TS translation units (bbts.hip: the reference's parser; bbts_ma.hip: the mode-adaptation mode):
// BBHEADER parsing and the bank's fields the second one needs.
#pragma once
#include "ctx.h"

struct dvbs2gpu_bbts;

namespace s2 {

// check_crc8 (bbframe_ts_parser.cpp:70-83): LSB-first register, polynomial 0xAB (reflected 0xD5), over `nbits` MSB-first bits
__host__ __device__ inline unsigned crc8_bits(const uint8_t* in, int nbits) {
    unsigned crc = 0;
    for (int n = 0; n < nbits; ++n) {
        unsigned fb = ((in[n >> 3] >> (7 - (n & 7))) ^ crc) & 1u;
        crc >>= 1;
        if (fb) crc ^= 0xAB;
    }
    return crc;
}
struct HeaderFields { int v[11]; };
__host__ __device__ inline HeaderFields parse_bbheader(const uint8_t* b) {
    HeaderFields h;
    h.v[0] = b[0] >> 6; h.v[1] = (b[0] >> 5) & 1; h.v[2] = (b[0] >> 4) & 1; h.v[3] = (b[0] >> 3) & 1; h.v[4] = (b[0] >> 2) & 1;
    h.v[5] = b[0] & 3;
    h.v[6] = h.v[1] == 0 ? b[1] : 0;
    h.v[7] = b[2] << 8 | b[3];
    h.v[8] = b[4] << 8 | b[5];
    h.v[9] = b[6];
    h.v[10] = b[7] << 8 | b[8];
    return h;
}
// header validation of work() (.cpp:119-152): true when the frame is parsed at all
__host__ __device__ inline bool header_ok(const uint8_t* frame, int max_dfl, HeaderFields* h) {
    if (crc8_bits(frame, 80) != 0) return false;
    *h = parse_bbheader(frame);
    const int dfl = h->v[8], syncd = h->v[10];
    if ((unsigned)dfl > (unsigned)max_dfl || syncd >= dfl - 8) return false;
    return dfl % 8 == 0;
}

struct BbtsMa;                                  // bbts_ma.hip
void bbts_ma_free(BbtsMa* m);
struct BbtsBankView {
    dvbs2gpu_ctx* ctx;                          // null: a host-only bank (dvbs2gpu_bbts_create_host)
    int nstreams, kbch, max_frames;
    BbtsMa** ma;
};
BbtsBankView bbts_view(dvbs2gpu_bbts* b);
dvbs2gpu_bbts* bbts_new_host_bank(int kbch_bits, int max_frames);
int bbts_reset_reference_state(dvbs2gpu_bbts* b);   // what a freshly created bank's reference-mode parser starts from

}  // namespace s2
