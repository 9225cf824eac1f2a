// dvbs2gpu_host::IpOutBank (include/dvbs2gpu_host.hpp) over host banks, driven the way a sink handler would, in front of an IpTsBank:
//   ipout_host <ts.bin> <packets per call> <P> <mode> <pid> <cap> <inner.bin>
// The output bank's slot 2 sends the packets of <pid> and of PID 0x1FFF but the null packets -- pid_mode 1, drop_null -- as RAW (mode 0)
// or RTP (1) datagrams of P packets over IPv4 to 239.9.9.9:5500; the last call flushes.  The IP-TS bank's slot 0 watches that flow
// and reads every call's datagrams back.  Prints every call's datagram rows and the IP-TS rows' flags, then both banks' counters; the
// TS that the IP-TS bank delivers goes to <inner.bin>.
#include <dvbs2gpu_host.hpp>

#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iterator>
#include <string>

int main(int argc, char** argv) {
    if (argc < 8) { fprintf(stderr, "usage: ipout_host ts per_call P mode pid cap out\n"); return 2; }
    std::ifstream fi(argv[1], std::ios::binary);
    const std::vector<uint8_t> ts((std::istreambuf_iterator<char>(fi)), std::istreambuf_iterator<char>());
    const int per_call = atoi(argv[2]), P = atoi(argv[3]), mode = atoi(argv[4]), pid = atoi(argv[5]);
    int cap = atoi(argv[6]);
    std::ofstream fo(argv[7], std::ios::binary);
    try {
        dvbs2gpu_host::IpOutBank out;
        dvbs2gpu_host::IpTsBank back;
        std::vector<uint8_t> ip((size_t)(per_call + 7) * 256), inner((size_t)(per_call + 7) * 188);
        int bytes[4] = {}, got[4] = {};
        uint8_t* outs[4] = {nullptr, nullptr, ip.data(), nullptr};
        uint8_t* inners[4] = {inner.data(), nullptr, nullptr, nullptr};
        if (out.work(ts.data(), 0, outs, cap, bytes) || out.status() != DVBS2GPU_ERR_ARG) { fprintf(stderr, "work() before init() must fail quietly\n"); return 4; }
        out.clearStatus();
        dvbs2gpu_ipout_flow f = {};
        f.family = 4;
        const uint8_t src[4] = {10, 0, 0, 1}, dst[4] = {239, 9, 9, 9};
        for (int i = 0; i < 4; ++i) { f.src_addr[i] = src[i]; f.dst_addr[i] = dst[i]; }
        f.src_port = 4000; f.dst_port = 5500; f.ttl = 5; f.dscp = 34; f.mode = (uint8_t)mode; f.packets_per_datagram = (uint8_t)P;
        f.ssrc = 0xA1B2C3D4u; f.timestamp_base = 90000; f.seq_base = 65534; f.pid_mode = 1; f.drop_null = 1;
        out.initHost(per_call);
        out.setFlow(2, f, {(uint16_t)pid, 0x1FFF});
        out.setRate(1000ull << 24);
        back.initHost(per_call + 1);
        back.setFlow(0, 4, f.dst_addr, f.dst_port);
        int calls = 0;
        for (size_t at = 0; at < ts.size(); at += (size_t)per_call * 188, ++calls) {
            const int nbytes = (int)std::min<size_t>((size_t)per_call * 188, ts.size() - at);
            const bool flush = at + (size_t)nbytes == ts.size();
            if (!out.work(ts.data() + at, nbytes, outs, cap, bytes, flush) && out.status() == DVBS2GPU_ERR_CAPACITY) {   // nothing was consumed: come again with room
                printf("call %d capacity %d\n", calls, out.needed(2));
                cap = out.needed(2);
                out.clearStatus();
                if (!out.work(ts.data() + at, nbytes, outs, cap, bytes, flush)) { fprintf(stderr, "%s\n", out.error().c_str()); return 5; }
            }
            if (out.status() != 0) { fprintf(stderr, "%s\n", out.error().c_str()); return 5; }
            printf("call %d bytes %d %d %d %d\n", calls, bytes[0], bytes[1], bytes[2], bytes[3]);
            const std::vector<dvbs2gpu_ipout_row> rows = out.rowTable(2);
            for (const dvbs2gpu_ipout_row& r : rows)
                printf("row %d %d %d %u %u %u %u %d %u\n", calls, r.offset, r.bytes, r.rtp_timestamp, r.rtp_seq, r.packets, r.flags, r.first_packet, r.udp_checksum);
            if (!back.work(dvbs2gpu_host::IpTsBank::view(ip.data(), rows), inners, (int)inner.size(), got)) { fprintf(stderr, "%s\n", back.error().c_str()); return 5; }
            for (const dvbs2gpu_ipts_row& r : back.rowTable()) printf("back %d %u %d %u\n", calls, r.flags, r.packets, r.rtp_seq);
            fo.write(reinterpret_cast<const char*>(inner.data()), got[0]);
        }
        const dvbs2gpu_ipout_stats s = out.stats(2), all = out.stats(-1);
        printf("stats %lld %lld %lld %lld %lld %lld %lld %lld\n", (long long)all.packets, (long long)all.bad_sync, (long long)s.passed, (long long)s.datagrams,
               (long long)s.short_datagrams, (long long)s.ts_packets, (long long)s.bytes_delivered, (long long)s.held);
        const dvbs2gpu_ipts_stats b = back.stats(0);
        printf("back stats %lld %lld %lld %lld %lld\n", (long long)b.matched, (long long)b.ts, (long long)b.ts_packets, (long long)(b.lost + b.late), (long long)b.bad_checksum);
    } catch (const std::exception& e) {
        fprintf(stderr, "%s\n", e.what());
        return 3;
    }
    return 0;
}
