// csrc/bbts_host.h on its own, no GPU and no HIP header: BbtsHostParser::run, call by call, the way the bank drives it for a stream.
//   bbts_host_parser <in.bin> <out.bin>
// in.bin: int32 kbch bits, cap, ncalls, ncalls frame counts; then the frames.  out.bin gets every call's output bytes; stdout one
// "call" line per call (bytes or the error code, the 15 header / stat words of dvbs2gpu_bbts_get_stats, synched, count), one "row"
// line per PDU table row of that call, and the nine GSE counters at the end.
#include "bbts_host.h"

#include <cstdio>
#include <fstream>
#include <iterator>

int main(int argc, char** argv) {
    if (argc < 3) { fprintf(stderr, "usage: bbts_host_parser in.bin out.bin\n"); return 2; }
    std::ifstream fi(argv[1], std::ios::binary);
    const std::vector<char> raw((std::istreambuf_iterator<char>(fi)), std::istreambuf_iterator<char>());
    if (raw.size() < 12) return 2;
    const int32_t* w = reinterpret_cast<const int32_t*>(raw.data());
    const int kbch = w[0], cap = w[1], ncalls = w[2], fb = kbch / 8;
    const uint8_t* frames = reinterpret_cast<const uint8_t*>(raw.data()) + 4 * (3 + (size_t)ncalls);
    s2::BbtsHostParser p;
    std::vector<uint8_t> buf(cap > 0 ? cap : 1), all;
    size_t at = 0;
    for (int c = 0; c < ncalls; ++c) {
        const int cnt = w[3 + c];
        if (4 * (3 + (size_t)ncalls) + at + (size_t)cnt * fb > raw.size()) return 2;
        const int n = p.run(frames + at, cnt, fb, kbch - 80, buf.data(), cap);
        at += (size_t)cnt * fb;
        printf("call %d", n);
        for (int k = 0; k < 11; ++k) printf(" %d", p.hdr[k]);
        printf(" %d %d %d 0 %d %d\n", p.gse.g.crc_err, p.last_cnt, p.last_proc, p.synched, p.count);
        for (const dvbs2gpu_gse_pdu& r : p.gse.rows) printf("row %u %u %u %u\n", r.offset, r.bytes, (unsigned)r.protocol, (unsigned)r.flags);
        if (n > 0) all.insert(all.end(), buf.begin(), buf.begin() + n);
    }
    std::ofstream(argv[2], std::ios::binary).write(reinterpret_cast<const char*>(all.data()), (std::streamsize)all.size());
    const s2::GseCounters& g = p.gse.g.cnt;
    printf("gse %lld %lld %lld %lld %lld %lld %lld %lld %lld\n", g.frames, g.packets, g.complete_pdus, g.reassembled_pdus, g.crc_failures,
           g.dropped_no_slot, g.dropped_overflow, g.dropped_no_fit, g.bytes_delivered);
    return 0;
}
