// dvbs2gpu_host::PcrBank (include/dvbs2gpu_host.hpp) over a host bank, driven the way a sink handler would, beside a PsiBank that
// reads the same packets:
//   pcr_host <ts.bin> <packets per call> <max_rows>
// The PSI bank follows the PAT after the first call; the PCR bank takes its watches from the decoded PMTs after the second.  Prints
// every call's rows, then the counters, the stream counters and the rate.
#include <dvbs2gpu_host.hpp>

#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iterator>

int main(int argc, char** argv) {
    if (argc < 4) { fprintf(stderr, "usage: pcr_host ts per_call max_rows\n"); return 2; }
    std::ifstream fi(argv[1], std::ios::binary);
    const std::vector<uint8_t> ts((std::istreambuf_iterator<char>(fi)), std::istreambuf_iterator<char>());
    const int per_call = atoi(argv[2]), max_rows = atoi(argv[3]);
    try {
        dvbs2gpu_host::PsiBank psi;
        dvbs2gpu_host::PcrBank pcr;
        if (pcr.work(ts.data(), 0) != 0 || pcr.status() != DVBS2GPU_ERR_ARG) { fprintf(stderr, "work() before init() must fail quietly\n"); return 4; }
        pcr.clearStatus();
        psi.initHost(per_call, 64);
        pcr.initHost(per_call, max_rows);
        pcr.setRate((uint64_t)1000 << 24);
        int calls = 0;
        for (size_t at = 0; at < ts.size(); at += (size_t)per_call * 188, ++calls) {
            const int nbytes = (int)std::min<size_t>((size_t)per_call * 188, ts.size() - at);
            psi.work(ts.data() + at, nbytes, nullptr, 0);
            const int records = pcr.work(ts.data() + at, nbytes);
            if (psi.status() != 0 || pcr.status() != 0) { fprintf(stderr, "%s%s\n", psi.error().c_str(), pcr.error().c_str()); return 5; }
            printf("call %d records %d\n", calls, records);
            for (const dvbs2gpu_pcr_row& r : pcr.rowTable())
                printf("row %d %u %u %u %u %d %llu %u %u %d\n", calls, r.pid, r.slot, r.kind, r.flags, r.packet, (unsigned long long)r.pcr, r.delta_ticks, r.delta_packets,
                       r.accuracy);
            if (calls == 0) psi.followPat();
            if (calls == 1)
                for (int pid : pcr.followPmts(psi)) printf("left %d\n", pid);
        }
        const dvbs2gpu_pcr_stats s = pcr.stats();
        printf("stats %lld %lld %lld %lld %lld %lld %lld %lld %lld %lld %lld %lld %lld %lld\n", (long long)s.pcr_packets, (long long)s.first, (long long)s.announced,
               (long long)s.repeated, (long long)s.jumps, (long long)s.late, (long long)s.ok, (long long)s.malformed, (long long)s.accuracy_measured,
               (long long)s.accuracy_errors, (long long)s.sum_ticks, (long long)s.sum_packets, (long long)s.max_delta_ticks, (long long)s.max_abs_accuracy);
        const dvbs2gpu_pcr_stream_stats t = pcr.streamStats();
        printf("stream %lld %lld %lld %d since %lld %lld\n", (long long)t.packets, (long long)t.unwatched_pcr_packets, (long long)t.rows_dropped, t.first_unwatched_pid,
               (long long)t.packets_since_pcr[0], (long long)t.packets_since_pcr[1]);
        printf("rate %.3f\n", pcr.rate(0));
    } catch (const std::exception& e) {
        fprintf(stderr, "%s\n", e.what());
        return 3;
    }
    return 0;
}
