// dvbs2gpu_host::TSMonitor (include/dvbs2gpu_host.hpp) driven the way a sink handler would:
//   tsmon_host <ts.bin> <out.bin> <packets per call> <cap> <mode> [<pid> ...]
// Writes the passing packets to out.bin and prints the counters and the PID table of the last call.  work() never throws: a call
// whose packets do not fit leaves DVBS2GPU_ERR_CAPACITY in status() and is repeated with a buffer that holds the whole call.
#include <dvbs2gpu_host.hpp>

#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iterator>

int main(int argc, char** argv) {
    if (argc < 6) { fprintf(stderr, "usage: tsmon_host ts out per_call cap mode pid...\n"); return 2; }
    std::ifstream fi(argv[1], std::ios::binary);
    const std::vector<uint8_t> ts((std::istreambuf_iterator<char>(fi)), std::istreambuf_iterator<char>());
    const int per_call = atoi(argv[3]);
    int cap = atoi(argv[4]);
    std::vector<uint16_t> pids;
    for (int k = 6; k < argc; ++k) pids.push_back((uint16_t)atoi(argv[k]));
    try {
        dvbs2gpu_host::TSMonitor mon;
        if (mon.work(ts.data(), 0, nullptr, 0) != 0 || mon.status() != DVBS2GPU_ERR_ARG) { fprintf(stderr, "work() before init() must fail quietly\n"); return 4; }
        mon.clearStatus();
        mon.init(per_call);
        mon.setFilter(atoi(argv[5]), pids);
        std::vector<uint8_t> out, buf;
        int retries = 0;
        for (size_t at = 0; at < ts.size(); at += (size_t)per_call * 188) {
            const int nbytes = (int)std::min<size_t>((size_t)per_call * 188, ts.size() - at);
            buf.resize(cap > 0 ? cap : 1);
            int n = mon.work(ts.data() + at, nbytes, buf.data(), cap);
            if (mon.status() == DVBS2GPU_ERR_CAPACITY) {
                mon.clearStatus();
                cap = nbytes; ++retries;
                buf.resize(cap);
                n = mon.work(ts.data() + at, nbytes, buf.data(), cap);
            }
            if (mon.status() != 0) { fprintf(stderr, "%s (%d)\n", mon.error().c_str(), mon.status()); return 5; }
            out.insert(out.end(), buf.begin(), buf.begin() + n);
        }
        std::ofstream(argv[2], std::ios::binary).write((const char*)out.data(), (std::streamsize)out.size());
        const dvbs2gpu_tsmon_stats s = mon.stats();
        printf("stats %lld %lld %lld %lld %lld %lld %lld %lld %lld %lld retries=%d\n", (long long)s.packets, (long long)s.null_packets, (long long)s.tei_packets,
               (long long)s.sync_byte_errors, (long long)s.cc_errors, (long long)s.duplicates, (long long)s.discontinuities, (long long)s.scrambled_packets,
               (long long)s.passed_packets, (long long)s.pids_seen, retries);
        for (const dvbs2gpu_tsmon_pid& r : mon.pidTable()) printf("row %u %u %u %u %u %u %u\n", r.pid, r.flags, r.packets, r.cc_errors, r.duplicates, r.scrambled, r.pusi);
    } catch (const std::exception& e) {
        fprintf(stderr, "%s\n", e.what());
        return 3;
    }
    return 0;
}
