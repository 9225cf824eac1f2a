// dvbs2gpu_host::PsiBank (include/dvbs2gpu_host.hpp) over a host bank, driven the way a sink handler would:
//   psi_host <ts.bin> <packets per call> <cap>
// Follows the PAT after the first call, prints every call's rows, the counters and the decoded views.  work() never throws: a call
// whose sections do not fit leaves DVBS2GPU_ERR_CAPACITY in status() and is repeated with the size needed() reports.
#include <dvbs2gpu_host.hpp>

#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iterator>

int main(int argc, char** argv) {
    if (argc < 4) { fprintf(stderr, "usage: psi_host ts per_call cap\n"); return 2; }
    std::ifstream fi(argv[1], std::ios::binary);
    const std::vector<uint8_t> ts((std::istreambuf_iterator<char>(fi)), std::istreambuf_iterator<char>());
    const int per_call = atoi(argv[2]);
    int cap = atoi(argv[3]);
    try {
        dvbs2gpu_host::PsiBank psi;
        if (psi.work(ts.data(), 0, nullptr, 0) != 0 || psi.status() != DVBS2GPU_ERR_ARG) { fprintf(stderr, "work() before init() must fail quietly\n"); return 4; }
        psi.clearStatus();
        psi.initHost(per_call, 64);
        std::vector<uint8_t> buf;
        int retries = 0, calls = 0;
        long long bytes = 0;
        for (size_t at = 0; at < ts.size(); at += (size_t)per_call * 188, ++calls) {
            const int nbytes = (int)std::min<size_t>((size_t)per_call * 188, ts.size() - at);
            buf.resize(cap > 0 ? cap : 1);
            int n = psi.work(ts.data() + at, nbytes, buf.data(), cap);
            if (psi.status() == DVBS2GPU_ERR_CAPACITY) {
                int rows;
                psi.clearStatus();
                psi.needed(&cap, &rows);
                ++retries;
                buf.resize(cap);
                n = psi.work(ts.data() + at, nbytes, buf.data(), cap);
            }
            if (psi.status() != 0) { fprintf(stderr, "%s (%d)\n", psi.error().c_str(), psi.status()); return 5; }
            bytes += n;
            for (const dvbs2gpu_psi_section& r : psi.sectionTable())
                printf("row %d %u %u %u %u %u %u %u %u %u %d %d %d\n", calls, r.pid, r.flags, r.table_id, r.ssi, r.version, r.current_next, r.section_number,
                       r.last_section_number, r.table_id_ext, r.length, r.offset, r.first_packet);
            if (calls == 0)
                for (const dvbs2gpu_psi_program& p : psi.followPat()) printf("left %u %u\n", p.program_number, p.pid);
        }
        const dvbs2gpu_psi_stats s = psi.stats();
        printf("stats %lld %lld %lld %lld %lld %lld %lld %lld %lld %lld %lld bytes=%lld retries=%d\n", (long long)s.packets, (long long)s.sections, (long long)s.valid,
               (long long)s.changed, (long long)s.crc_errors, (long long)s.dropped_sections, (long long)s.malformed_sections, (long long)s.malformed_packets,
               (long long)s.scrambled_packets, (long long)s.unexpected_table_id, (long long)s.bytes_delivered, bytes, retries);
        dvbs2gpu_psi_pat pat;
        for (const dvbs2gpu_psi_program& p : psi.programs(&pat)) printf("program %u %u\n", p.program_number, p.pid);
        printf("pat %d %d %d\n", pat.transport_stream_id, pat.version, pat.malformed);
        for (int slot = 1; slot < 4; ++slot) {
            dvbs2gpu_psi_pmt pmt;
            const std::vector<dvbs2gpu_psi_es> es = psi.programMap(slot, &pmt);
            printf("pmt %d %d %d %d %d", slot, pmt.program_number, pmt.version, pmt.pcr_pid, pmt.malformed);
            for (const dvbs2gpu_psi_es& e : es) printf(" %u:%u", e.stream_type, e.elementary_pid);
            printf("\n");
        }
    } catch (const std::exception& e) {
        fprintf(stderr, "%s\n", e.what());
        return 3;
    }
    return 0;
}
