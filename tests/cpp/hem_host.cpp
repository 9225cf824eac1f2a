// dvbs2gpu_host::dvbs2::BBFrameTSParser (include/dvbs2gpu_host.hpp) on DVB-T2 high-efficiency-mode BBFRAMEs: setModeAdaptation, selectISI and
// setModeAdaptationT2HEM, then work() with a frame-size list and flush():
//   hem_host <frames.bin> <sizes.txt> <out prefix> <frames per call> <switch 0|1> <isi> [<isi> ...]
// frames.bin: BBFRAMEs back to back, sizes.txt: one size per line.  Writes <out prefix><k>.ts per selected ISI and prints one status
// line per output.
#include <dvbs2gpu_host.hpp>

#include <cstdio>
#include <cstdlib>
#include <fstream>

int main(int argc, char** argv) {
    if (argc < 7) { fprintf(stderr, "usage: hem_host frames sizes prefix per_call switch isi...\n"); return 2; }
    std::ifstream fi(argv[1], std::ios::binary);
    std::vector<uint8_t> bb((std::istreambuf_iterator<char>(fi)), std::istreambuf_iterator<char>());
    std::vector<int> sizes;
    { std::ifstream fs(argv[2]); int v; while (fs >> v) sizes.push_back(v); }
    const std::string prefix = argv[3];
    const int per_call = atoi(argv[4]), cap = 1 << 20;
    std::vector<uint8_t> isi;
    for (int k = 6; k < argc; ++k) isi.push_back((uint8_t)atoi(argv[k]));
    try {
        dvbs2gpu_host::dvbs2::BBFrameTSParser p;
        p.max_frames = per_call;
        p.setFrameSize(58192);
        dvbs2gpu_bbts_ma_cfg cfg;
        dvbs2gpu_bbts_ma_default_cfg(&cfg);
        p.setModeAdaptation(&cfg);
        p.selectISI(isi.data(), (int)isi.size());
        if (atoi(argv[5])) p.setModeAdaptationT2HEM(true);
        std::vector<std::vector<uint8_t>> ts(8), buf(8, std::vector<uint8_t>(cap));
        uint8_t* outs[8];
        for (int k = 0; k < 8; ++k) outs[k] = buf[k].data();
        int nb[8];
        size_t at = 0;
        auto deliver = [&]() { for (int k = 0; k < 8; ++k) ts[k].insert(ts[k].end(), buf[k].begin(), buf[k].begin() + nb[k]); };
        for (size_t f = 0; f < sizes.size(); f += per_call) {
            const int cnt = (int)std::min<size_t>(per_call, sizes.size() - f);
            if (!p.work(bb.data() + at, sizes.data() + f, cnt, outs, cap, nb)) { fprintf(stderr, "an output does not fit\n"); return 4; }
            deliver();
            for (int k = 0; k < cnt; ++k) at += sizes[f + k];
        }
        p.flush(outs, cap, nb);
        deliver();
        for (size_t k = 0; k < isi.size(); ++k) {
            std::ofstream(prefix + std::to_string(k) + ".ts", std::ios::binary).write((const char*)ts[k].data(), ts[k].size());
            const dvbs2gpu_bbts_ma_stats s = p.modeAdaptationStats((int)k);
            printf("out isi=%d bytes=%zu packets=%lld nulls=%lld frames=%d hem_frames=%d broken_joins=%d rejected=%d skipped=%d\n", s.isi, ts[k].size(),
                   (long long)s.packets, (long long)s.nulls, s.frames, s.hem_frames, s.broken_joins, s.rejected_frames, s.skipped_frames);
        }
    } catch (const std::exception& e) {
        fprintf(stderr, "%s\n", e.what());
        return 3;
    }
    return 0;
}
