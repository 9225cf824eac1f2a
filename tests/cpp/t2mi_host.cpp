// dvbs2gpu_host::T2miBank (include/dvbs2gpu_host.hpp) over a host bank, driven the way a sink handler would, in front of a host
// mode-adaptation bank (dvbs2gpu_bbts_create_host) that takes its BBFRAMEs:
//   t2mi_host <ts.bin> <packets per call> <pid> <plp> <max_rows> <inner.bin>
// Slot 0 takes the PLP, slot 1 every PLP (rows and counters only).  Prints every call's rows and frame sizes, then the counters; the
// inner transport stream goes to <inner.bin>.  T2miBank::feed() takes a dvbs2::BBFrameTSParser, which has no host form, so it is not
// called here: tests/cpp/t2mi_feed.cpp calls it on the device.
#include <dvbs2gpu_host.hpp>

#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iterator>

int main(int argc, char** argv) {
    if (argc < 7) { fprintf(stderr, "usage: t2mi_host ts per_call pid plp max_rows inner\n"); return 2; }
    std::ifstream fi(argv[1], std::ios::binary);
    const std::vector<uint8_t> ts((std::istreambuf_iterator<char>(fi)), std::istreambuf_iterator<char>());
    const int per_call = atoi(argv[2]), pid = atoi(argv[3]), plp = atoi(argv[4]), max_rows = atoi(argv[5]);
    std::ofstream fo(argv[6], std::ios::binary);
    dvbs2gpu_bbts* ma = nullptr;
    try {
        dvbs2gpu_host::T2miBank t2;
        std::vector<uint8_t> bb((size_t)per_call * 188 + 8), inner(1 << 20);
        if (t2.work(0, ts.data(), 0, bb.data(), (int)bb.size()) != 0 || t2.status() != DVBS2GPU_ERR_ARG) { fprintf(stderr, "work() before init() must fail quietly\n"); return 4; }
        t2.clearStatus();
        t2.initHost(per_call, max_rows);
        t2.setWatch(0, pid, plp);
        t2.setWatch(1, pid);
        dvbs2gpu_host::check(dvbs2gpu_bbts_create_host(58192, 64, &ma));
        dvbs2gpu_bbts_ma_cfg cfg;
        dvbs2gpu_bbts_ma_default_cfg(&cfg);
        dvbs2gpu_host::check(dvbs2gpu_bbts_set_mode_adaptation(ma, &cfg));
        int calls = 0;
        for (size_t at = 0; at < ts.size(); at += (size_t)per_call * 188, ++calls) {
            const int nbytes = (int)std::min<size_t>((size_t)per_call * 188, ts.size() - at);
            int got = t2.work(0, ts.data() + at, nbytes, bb.data(), (int)bb.size());
            if (t2.status() == DVBS2GPU_ERR_CAPACITY) {          // nothing was consumed: say what was needed and come again with room
                printf("call %d capacity %d %d\n", calls, t2.needed(0).first, t2.needed(0).second);
                t2.clearStatus();
                t2.initHost(per_call, t2.needed(0).second);
                t2.setWatch(0, pid, plp);
                t2.setWatch(1, pid);
                at -= (size_t)per_call * 188; --calls;
                continue;
            }
            if (t2.status() != 0) { fprintf(stderr, "%s\n", t2.error().c_str()); return 5; }
            const std::vector<int> sizes = t2.frameBytes(0);
            printf("call %d bytes %d frames", calls, got);
            for (int s : sizes) printf(" %d", s);
            printf("\n");
            for (const dvbs2gpu_t2mi_row& r : t2.rowTable(0))
                printf("row %d %u %u %u %u %u %u %u %u %d %d %d %d %d\n", calls, r.packet_type, r.packet_count, r.superframe_idx, r.stream_id, r.flags, r.plp_id,
                       r.frame_idx, r.payload_bits, r.length, r.offset, r.bbframe_bytes, r.first_packet, r.last_packet);
            uint8_t* outs[8] = {inner.data(), nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
            int out_bytes[8] = {0};
            dvbs2gpu_host::check(dvbs2gpu_bbts_ma_work(ma, bb.data(), sizes.data(), (int)sizes.size(), outs, (int)inner.size(), out_bytes, nullptr));
            fo.write(reinterpret_cast<const char*>(inner.data()), out_bytes[0]);
            t2.work(1, ts.data() + at, nbytes, nullptr, 0);
        }
        for (int slot = 0; slot < 2; ++slot) {
            const dvbs2gpu_t2mi_stats s = t2.stats(slot);
            const int64_t* v = &s.packets;
            printf("stats %d", slot);
            for (size_t i = 0; i < sizeof(s) / sizeof(int64_t); ++i) printf(" %lld", (long long)v[i]);
            printf("\n");
        }
    } catch (const std::exception& e) {
        fprintf(stderr, "%s\n", e.what());
        return 3;
    }
    if (ma) dvbs2gpu_bbts_destroy(ma);
    return 0;
}
