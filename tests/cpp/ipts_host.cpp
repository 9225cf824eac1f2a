// dvbs2gpu_host::IpTsBank (include/dvbs2gpu_host.hpp) over host banks, driven the way a sink handler would, behind an MpeBank:
//   ipts_host <ts.bin> <packets per call> <pid> <IPv4 group hex8> <port> <cap> <inner.bin>
// The MPE bank's slot 0 takes every MAC address; the IP-TS bank's slot 1 takes (group, port).  Prints every call's rows, then the
// counters; the TS packets of slot 1 go to <inner.bin>, back to back.
#include <dvbs2gpu_host.hpp>

#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iterator>
#include <string>

int main(int argc, char** argv) {
    if (argc < 8 || std::string(argv[4]).size() != 8) { fprintf(stderr, "usage: ipts_host ts per_call pid group port cap out\n"); return 2; }
    std::ifstream fi(argv[1], std::ios::binary);
    const std::vector<uint8_t> ts((std::istreambuf_iterator<char>(fi)), std::istreambuf_iterator<char>());
    const int per_call = atoi(argv[2]), pid = atoi(argv[3]), port = atoi(argv[5]);
    int cap = atoi(argv[6]);
    uint8_t group[16] = {};
    for (int i = 0; i < 4; ++i) group[i] = (uint8_t)strtol(std::string(argv[4] + 2 * i, 2).c_str(), nullptr, 16);
    std::ofstream fo(argv[7], std::ios::binary);
    try {
        dvbs2gpu_host::MpeBank mpe;
        dvbs2gpu_host::IpTsBank bank;
        std::vector<uint8_t> ip((size_t)per_call * 188 + 4096), inner(ip.size());
        int bytes[4] = {};
        uint8_t* outs[4] = {nullptr, inner.data(), nullptr, nullptr};
        if (bank.work(dvbs2gpu_ipts_view{}, outs, cap, bytes) || bank.status() != DVBS2GPU_ERR_ARG) { fprintf(stderr, "work() before init() must fail quietly\n"); return 4; }
        bank.clearStatus();
        mpe.initHost(per_call, 64);
        mpe.setWatch(0, pid);
        bank.initHost(64);
        bank.setFlow(1, 4, group, port);
        int calls = 0;
        for (size_t at = 0; at < ts.size(); at += (size_t)per_call * 188, ++calls) {
            const int nbytes = (int)std::min<size_t>((size_t)per_call * 188, ts.size() - at);
            mpe.work(0, ts.data() + at, nbytes, ip.data(), (int)ip.size());
            if (mpe.status() != 0) { fprintf(stderr, "%s\n", mpe.error().c_str()); return 5; }
            const std::vector<dvbs2gpu_mpe_row> rows = mpe.rowTable(0);
            const dvbs2gpu_ipts_view v = dvbs2gpu_host::IpTsBank::view(ip.data(), rows);
            if (!bank.work(v, outs, cap, bytes) && bank.status() == DVBS2GPU_ERR_CAPACITY) {      // nothing was consumed: say what was needed and come again with room
                printf("call %d capacity %d\n", calls, bank.needed(1));
                cap = bank.needed(1);
                bank.clearStatus();
                if (!bank.work(v, outs, cap, bytes)) { fprintf(stderr, "%s\n", bank.error().c_str()); return 5; }
            }
            if (bank.status() != 0) { fprintf(stderr, "%s\n", bank.error().c_str()); return 5; }
            printf("call %d bytes %d %d %d %d\n", calls, bytes[0], bytes[1], bytes[2], bytes[3]);
            for (const dvbs2gpu_ipts_row& r : bank.rowTable())
                printf("row %d %u %d %u %u %u %u %u %u %u %u %d %d %d %d\n", calls, r.flags, r.slot, r.family, r.payload_type, r.src_port, r.dst_port, r.rtp_seq, r.ts_at,
                       r.rtp_timestamp, r.rtp_ssrc, r.packets, r.lost, r.offset, r.bytes);
            fo.write(reinterpret_cast<const char*>(inner.data()), bytes[1]);
        }
        for (int slot = -1; slot < 2; ++slot) {
            const dvbs2gpu_ipts_stats s = bank.stats(slot);
            const int64_t* v = &s.rows;
            printf("stats %d", slot);
            for (size_t i = 0; i < sizeof(s) / sizeof(int64_t); ++i) printf(" %lld", (long long)v[i]);
            printf("\n");
        }
    } catch (const std::exception& e) {
        fprintf(stderr, "%s\n", e.what());
        return 3;
    }
    return 0;
}
