// dvbs2gpu_host::AudBank (include/dvbs2gpu_host.hpp) over a host bank, driven the way a sink handler would, beside a PsiBank that
// reads the same packets:
//   aud_host <ts.bin> <packets per call> <max_rows>
// The PSI bank follows the PAT after the first call; the audio bank takes its watches from the decoded PMTs after the second.  Prints
// every call's rows, then the counters and the stream counters.
#include <dvbs2gpu_host.hpp>

#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iterator>

int main(int argc, char** argv) {
    if (argc < 4) { fprintf(stderr, "usage: aud_host ts per_call max_rows\n"); return 2; }
    std::ifstream fi(argv[1], std::ios::binary);
    const std::vector<uint8_t> ts((std::istreambuf_iterator<char>(fi)), std::istreambuf_iterator<char>());
    const int per_call = atoi(argv[2]), max_rows = atoi(argv[3]);
    try {
        dvbs2gpu_host::PsiBank psi;
        dvbs2gpu_host::AudBank aud;
        if (aud.work(ts.data(), 0) != 0 || aud.status() != DVBS2GPU_ERR_ARG) { fprintf(stderr, "work() before init() must fail quietly\n"); return 4; }
        aud.clearStatus();
        psi.initHost(per_call, 64);
        aud.initHost(per_call, max_rows);
        int calls = 0;
        for (size_t at = 0; at < ts.size(); at += (size_t)per_call * 188, ++calls) {
            const int nbytes = (int)std::min<size_t>((size_t)per_call * 188, ts.size() - at);
            psi.work(ts.data() + at, nbytes, nullptr, 0);
            const int rows = aud.work(ts.data() + at, nbytes);
            if (psi.status() != 0 || aud.status() != 0) { fprintf(stderr, "%s%s\n", psi.error().c_str(), aud.error().c_str()); return 5; }
            printf("call %d rows %d\n", calls, rows);
            for (const dvbs2gpu_aud_row& r : aud.rows())
                printf("row %d %u %u %u %u %u %u %u %u %u %llu %llu %llu %u %u %u\n", calls, r.pid, r.slot, r.unit, r.code, r.detail, r.flags, r.packet, r.kbps, r.head,
                       (unsigned long long)r.es_offset, (unsigned long long)r.pts, (unsigned long long)r.dts, r.sample_rate, r.frame_bytes, r.samples);
            if (calls == 0) psi.followPat();
            if (calls == 1)
                for (int pid : aud.followPmts(psi)) printf("left %d\n", pid);
        }
        const dvbs2gpu_aud_stats s = aud.stats();
        const int64_t* v = &s.packets;
        printf("stats");
        for (size_t i = 0; i < sizeof(s) / sizeof(int64_t); ++i) printf(" %lld", (long long)v[i]);
        const dvbs2gpu_aud_stream_stats t = aud.streamStats();
        printf("\nstream %lld %lld\n", (long long)t.packets, (long long)t.rows_dropped);
    } catch (const std::exception& e) {
        fprintf(stderr, "%s\n", e.what());
        return 3;
    }
    return 0;
}
