// dvbs2gpu_host::dvbs2::BBFrameTSParser (include/dvbs2gpu_host.hpp) in its mode-adaptation mode, driven the way the plugin's sink handler would:
//   ma_host <frames.bin> <sizes.txt> <out prefix> <frames per call> <cap> <issy_bytes> <crc_span> <isi> [<isi> ...]
// frames.bin: BBFRAMEs back to back, sizes.txt: one size per line.  Writes <out prefix><k>.ts per selected ISI and prints one
// status line per output.  A call whose output does not fit is repeated with the sizes the parser asks for.
#include <dvbs2gpu_host.hpp>

#include <cstdio>
#include <cstdlib>
#include <fstream>

int main(int argc, char** argv) {
    if (argc < 9) { fprintf(stderr, "usage: ma_host frames sizes prefix per_call cap issy span isi...\n"); return 2; }
    std::ifstream fi(argv[1], std::ios::binary);
    std::vector<uint8_t> bb((std::istreambuf_iterator<char>(fi)), std::istreambuf_iterator<char>());
    std::vector<int> sizes;
    { std::ifstream fs(argv[2]); int v; while (fs >> v) sizes.push_back(v); }
    const std::string prefix = argv[3];
    const int per_call = atoi(argv[4]);
    int cap = atoi(argv[5]);
    std::vector<uint8_t> isi;
    for (int k = 8; k < argc; ++k) isi.push_back((uint8_t)atoi(argv[k]));
    try {
        dvbs2gpu_host::dvbs2::BBFrameTSParser p;
        p.max_frames = per_call;
        p.setFrameSize(58192);
        dvbs2gpu_bbts_ma_cfg cfg;
        dvbs2gpu_bbts_ma_default_cfg(&cfg);
        cfg.issy_bytes = atoi(argv[6]); cfg.crc_span = atoi(argv[7]);
        p.setModeAdaptation(&cfg);
        p.selectISI(isi.data(), (int)isi.size());
        std::vector<std::vector<uint8_t>> ts(8), buf(8);
        int retries = 0;
        size_t at = 0;
        auto deliver = [&](const int* n) { for (int k = 0; k < 8; ++k) ts[k].insert(ts[k].end(), buf[k].begin(), buf[k].begin() + n[k]); };
        for (size_t f = 0; f < sizes.size(); f += per_call) {
            const int cnt = (int)std::min<size_t>(per_call, sizes.size() - f);
            int nb[8], need[8];
            for (;;) {
                uint8_t* outs[8];
                for (int k = 0; k < 8; ++k) { buf[k].resize(cap > 0 ? cap : 1); outs[k] = buf[k].data(); }
                if (p.work(bb.data() + at, sizes.data() + f, cnt, outs, cap, nb, need)) break;
                for (int k = 0; k < 8; ++k) cap = std::max(cap, need[k]);
                ++retries;
            }
            deliver(nb);
            for (int k = 0; k < cnt; ++k) at += sizes[f + k];
        }
        int nb[8];
        uint8_t* outs[8];
        cap = std::max(cap, 256 * 188);
        for (int k = 0; k < 8; ++k) { buf[k].resize(cap); outs[k] = buf[k].data(); }
        p.flush(outs, cap, nb);
        deliver(nb);
        for (size_t k = 0; k < isi.size(); ++k) {
            std::ofstream(prefix + std::to_string(k) + ".ts", std::ios::binary).write((const char*)ts[k].data(), ts[k].size());
            const dvbs2gpu_bbts_ma_stats s = p.modeAdaptationStats((int)k);
            printf("out isi=%d bytes=%zu packets=%lld nulls=%lld ts_errs=%lld broken_joins=%d rejected=%d skipped=%d issy=%d retries=%d\n", s.isi, ts[k].size(),
                   (long long)s.packets, (long long)s.nulls, (long long)s.ts_errs, s.broken_joins, s.rejected_frames, s.skipped_frames, s.issy_bytes, retries);
        }
    } catch (const std::exception& e) {
        fprintf(stderr, "%s\n", e.what());
        return 3;
    }
    return 0;
}
