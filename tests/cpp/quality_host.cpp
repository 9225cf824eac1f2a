// Reads a file of complex64 samples (2 per symbol) and runs it through the C++ host classes with quality estimation on, call by call; prints the
// figures the plugin would poll after the last call:
//   quality_host s2 <iq.cf32> <modcod> <short> <pilots> <chunk>     dvbs2::DVBS2Demod: frames, quality records, esn0_db, mer_db
//   quality_host dvbs <iq.cf32> <chunk>                             dvbs::DVBSDemod: calls with a figure, stats_esn0_db, stats_mer_db
// Exit codes: 0 ok, 2 bad arguments, 3 exception (e.g. no device: the engine has no CPU fallback).
#include <dvbs2gpu_host.hpp>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iterator>
#include <string>
#include <vector>

using namespace dvbs2gpu_host;

int main(int argc, char** argv) {
    if (argc < 4) { fprintf(stderr, "usage: quality_host s2 <iq.cf32> <modcod> <short> <pilots> <chunk> | dvbs <iq.cf32> <chunk>\n"); return 2; }
    const std::string mode = argv[1];
    if (!((mode == "s2" && argc == 7) || (mode == "dvbs" && argc == 4))) return 2;
    std::ifstream f(argv[2], std::ios::binary);
    if (!f) return 2;
    std::vector<char> raw((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
    const int chunk = atoi(argv[argc - 1]);
    if (chunk <= 0 || chunk > STREAM_BUFFER_SIZE) return 2;
    const complex_t* iq = reinterpret_cast<const complex_t*>(raw.data());
    const long n = (long)(raw.size() / sizeof(complex_t));
    const double bw = 0.00628, damp = 0.707, den = 1.0 + 2.0 * damp * bw + bw * bw;     // (main.cpp's timing-loop gains)
    const double omega_gain = 4.0 * bw * bw / den, mu_gain = 4.0 * damp * bw / den;
    std::vector<uint8_t> out(8 * 1024 * 1024);
    try {
        if (mode == "s2") {
            const int modcod = atoi(argv[3]), shortframes = atoi(argv[4]), pilots = atoi(argv[5]);
            dvbs2::DVBS2Demod d;
            d.setQualityEstimation(true);      // (before init: applied to the handle init creates)
            d.init(2e6, 4e6, 0.0001f, 0.35f, 65, 0.00628f, 0.006f, omega_gain, mu_gain, nullptr, nullptr, modcod, shortframes != 0, pilots != 0, 0.6f, 16, 0.02);
            d.setSymbolrate(2e6);              // (a rebuilt handle keeps the setting)
            long frames = 0, records = 0;
            for (long a = 0; a < n; a += chunk) {
                const int cnt = (int)(n - a < chunk ? n - a : chunk);
                const int bytes = d.process(cnt, iq + a, out.data());
                records += (long)d.frameQuality().size();
                if (bytes > 0) frames += bytes / (d.getKBCH() / 8);
            }
            printf("s2 frames=%ld records=%ld esn0_db=%.3f mer_db=%.3f\n", frames, records, d.esn0_db, d.mer_db);
        } else {
            dvbs::DVBSDemod d;
            d.setQualityEstimation(true);
            d.init(2e6, 4e6, 0.0001f, 0.35f, 65, 0.00628f, 0.006f, omega_gain, mu_gain, nullptr, nullptr, 0.02);
            long figures = 0;
            for (long a = 0; a < n; a += chunk) {
                const int cnt = (int)(n - a < chunk ? n - a : chunk);
                d.process(cnt, iq + a, out.data());
                if (std::isfinite(d.stats_esn0_db)) ++figures;
            }
            printf("dvbs calls_with_figure=%ld esn0_db=%.3f mer_db=%.3f\n", figures, d.stats_esn0_db, d.stats_mer_db);
        }
    } catch (const std::exception& e) {
        fprintf(stderr, "%s\n", e.what());
        return 3;
    }
    return 0;
}
