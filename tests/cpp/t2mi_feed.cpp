// dvbs2gpu_host::T2miBank::feed (include/dvbs2gpu_host.hpp) with a DEVICE bank in front of a dvbs2::BBFrameTSParser in mode-adaptation
// mode, driven the way a sink handler would:
//   t2mi_feed <ts.bin> <packets per call> <pid> <plp> <max_rows> <inner.bin>
// Slot 0 takes the PLP.  Every call's BBFRAMEs go through feed(); the first feed() of a call that brought frames is given an output
// buffer of 187 bytes, less than one TS packet, so that it must say false and name the size, and is repeated.  Prints one line per
// call and the parser's counters; the inner transport stream goes to <inner.bin>.
#include <dvbs2gpu_host.hpp>

#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iterator>

int main(int argc, char** argv) {
    if (argc < 7) { fprintf(stderr, "usage: t2mi_feed ts per_call pid plp max_rows inner\n"); return 2; }
    std::ifstream fi(argv[1], std::ios::binary);
    const std::vector<uint8_t> ts((std::istreambuf_iterator<char>(fi)), std::istreambuf_iterator<char>());
    const int per_call = atoi(argv[2]), pid = atoi(argv[3]), plp = atoi(argv[4]), max_rows = atoi(argv[5]);
    std::ofstream fo(argv[6], std::ios::binary);
    try {
        dvbs2gpu_host::T2miBank t2;
        t2.init(per_call, max_rows);
        t2.setWatch(0, pid, plp);
        dvbs2gpu_host::dvbs2::BBFrameTSParser parser;
        parser.setFrameSize(58192);
        dvbs2gpu_bbts_ma_cfg cfg;
        dvbs2gpu_bbts_ma_default_cfg(&cfg);
        parser.setModeAdaptation(&cfg);
        std::vector<uint8_t> bb((size_t)per_call * 188 + 8), inner(1 << 20);
        uint8_t* outs[8] = {inner.data(), nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
        int calls = 0;
        for (size_t at = 0; at < ts.size(); at += (size_t)per_call * 188, ++calls) {
            const int nbytes = (int)std::min<size_t>((size_t)per_call * 188, ts.size() - at);
            const int got = t2.work(0, ts.data() + at, nbytes, bb.data(), (int)bb.size());
            if (t2.status() != 0) { fprintf(stderr, "%s\n", t2.error().c_str()); return 5; }
            int out_bytes[8] = {0}, needed[8] = {0}, refused = 0;
            if (got > 0) {
                if (t2.feed(0, parser, bb.data(), outs, 187, out_bytes, needed)) { fprintf(stderr, "feed() into 187 bytes must say false\n"); return 4; }
                refused = needed[0];
            }
            if (!t2.feed(0, parser, bb.data(), outs, (int)inner.size(), out_bytes, needed)) { fprintf(stderr, "feed() needs %d bytes\n", needed[0]); return 4; }
            printf("call %d bytes %d frames %zu refused %d inner %d\n", calls, got, t2.frameBytes(0).size(), refused, out_bytes[0]);
            fo.write(reinterpret_cast<const char*>(inner.data()), out_bytes[0]);
        }
        const dvbs2gpu_bbts_ma_stats s = parser.modeAdaptationStats(0);
        printf("parser packets %lld rejected %d skipped %d\n", (long long)s.packets, s.rejected_frames, s.skipped_frames);
    } catch (const std::exception& e) {
        fprintf(stderr, "%s\n", e.what());
        return 3;
    }
    return 0;
}
