// dvbs2gpu_host::UleBank (include/dvbs2gpu_host.hpp) over a host bank, driven the way a sink handler would:
//   ule_host <ts.bin> <packets per call> <pid> <npa_value hex12> <npa_mask hex12> <max_rows> <datagrams.bin>
// Slot 0 takes the NPA filter and no SNDU without an address, slot 1 every address and those too (rows and counters only).  Prints every call's rows, then the counters; the
// datagrams of slot 0 go to <datagrams.bin>, back to back.
#include <dvbs2gpu_host.hpp>

#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iterator>
#include <string>

static void hex6(const char* s, uint8_t* out) {
    for (int i = 0; i < 6; ++i) out[i] = (uint8_t)strtol(std::string(s + 2 * i, 2).c_str(), nullptr, 16);
}

int main(int argc, char** argv) {
    if (argc < 8 || std::string(argv[4]).size() != 12 || std::string(argv[5]).size() != 12) { fprintf(stderr, "usage: ule_host ts per_call pid npa mask max_rows out\n"); return 2; }
    std::ifstream fi(argv[1], std::ios::binary);
    const std::vector<uint8_t> ts((std::istreambuf_iterator<char>(fi)), std::istreambuf_iterator<char>());
    const int per_call = atoi(argv[2]), pid = atoi(argv[3]), max_rows = atoi(argv[6]);
    uint8_t npa[6], mask[6];
    hex6(argv[4], npa), hex6(argv[5], mask);
    std::ofstream fo(argv[7], std::ios::binary);
    try {
        dvbs2gpu_host::UleBank ule;
        std::vector<uint8_t> out((size_t)per_call * 188 + 4096);
        if (ule.work(0, ts.data(), 0, out.data(), (int)out.size()) != 0 || ule.status() != DVBS2GPU_ERR_ARG) { fprintf(stderr, "work() before init() must fail quietly\n"); return 4; }
        ule.clearStatus();
        auto init = [&](int rows) {
            ule.initHost(per_call, rows);
            ule.setWatch(0, pid, npa, mask);
            ule.setWatch(1, pid, nullptr, nullptr, true);
        };
        init(max_rows);
        int calls = 0;
        for (size_t at = 0; at < ts.size(); at += (size_t)per_call * 188, ++calls) {
            const int nbytes = (int)std::min<size_t>((size_t)per_call * 188, ts.size() - at);
            const int got = ule.work(0, ts.data() + at, nbytes, out.data(), (int)out.size());
            if (ule.status() == DVBS2GPU_ERR_CAPACITY) {         // nothing was consumed: say what was needed and come again with room
                printf("call %d capacity %d %d\n", calls, ule.needed(0).first, ule.needed(0).second);
                ule.clearStatus();
                init(ule.needed(0).second);                      // (a fresh bank: this happens in the first call only)
                at -= (size_t)per_call * 188; --calls;
                continue;
            }
            if (ule.status() != 0) { fprintf(stderr, "%s\n", ule.error().c_str()); return 5; }
            printf("call %d bytes %d\n", calls, got);
            for (const dvbs2gpu_ule_row& r : ule.rowTable(0))
                printf("row %d %u %u %u %02x%02x%02x%02x%02x%02x %u %u %u %u %u %u %d %d %d %d %d %u %u\n", calls, r.flags, r.family, r.protocol, r.mac[0], r.mac[1],
                       r.mac[2], r.mac[3], r.mac[4], r.mac[5], r.ip_at, r.extension_bytes, r.src_port, r.dst_port, r.src4, r.dst4, r.length, r.offset,
                       r.bytes, r.first_packet, r.last_packet, r.ethertype, r.stuffing);
            fo.write(reinterpret_cast<const char*>(out.data()), got);
            ule.work(1, ts.data() + at, nbytes, nullptr, 0);
        }
        for (int slot = 0; slot < 2; ++slot) {
            const dvbs2gpu_ule_stats s = ule.stats(slot);
            const int64_t* v = &s.packets;
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
