// dvbs2gpu_host::dvbs2::BBFrameTSParser (include/dvbs2gpu_host.hpp) on GSE frames, driven the way the plugin's sink handler would:
//   gse_host <frames.bin> <kbch bits> <frames per call> <out.bin> <gse path 0|1>
// Writes every call's output to out.bin, prints one "row" line per PDU table row (offsets counted over the whole run) and one
// "stats" line at the end.
#include <dvbs2gpu_host.hpp>

#include <cstdio>
#include <cstdlib>
#include <fstream>

int main(int argc, char** argv) {
    if (argc < 6) { fprintf(stderr, "usage: gse_host frames kbch per_call out path\n"); return 2; }
    std::ifstream fi(argv[1], std::ios::binary);
    std::vector<uint8_t> bb((std::istreambuf_iterator<char>(fi)), std::istreambuf_iterator<char>());
    const int kbch = atoi(argv[2]), per_call = atoi(argv[3]), fb = kbch / 8;
    try {
        dvbs2gpu_host::dvbs2::BBFrameTSParser p;
        p.max_frames = per_call;
        p.setFrameSize(kbch);
        p.set_gse_path(atoi(argv[5]));
        const int cap = per_call * fb + 376 + 3 * 65536;
        std::vector<uint8_t> buf(cap), all;
        const int total = (int)(bb.size() / fb);
        for (int f = 0; f < total; f += per_call) {
            const int cnt = std::min(per_call, total - f);
            const int n = p.work(bb.data() + (size_t)f * fb, cnt, buf.data(), cap);
            for (const dvbs2gpu_gse_pdu& r : p.pdu_table())
                printf("row offset=%zu bytes=%u protocol=%u flags=%u\n", all.size() + r.offset, r.bytes, (unsigned)r.protocol, (unsigned)r.flags);
            all.insert(all.end(), buf.begin(), buf.begin() + n);
        }
        std::ofstream(argv[4], std::ios::binary).write((const char*)all.data(), all.size());
        const dvbs2gpu_gse_stats s = p.gse_stats();
        printf("stats frames=%lld packets=%lld complete=%lld reassembled=%lld crc_failures=%lld bytes=%lld fallbacks=%lld\n", (long long)s.frames,
               (long long)s.packets, (long long)s.complete_pdus, (long long)s.reassembled_pdus, (long long)s.crc_failures,
               (long long)s.bytes_delivered, (long long)s.host_fallback_calls);
    } catch (const std::exception& e) {
        fprintf(stderr, "%s\n", e.what());
        return 3;
    }
    return 0;
}
