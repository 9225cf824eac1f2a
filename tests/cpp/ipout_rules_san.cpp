// The IP output bank's rules (csrc/ipout_rules.h) alone, under the sanitizers: the host stream (IpoutHostStream, one stream).
//   ipout_rules_san <ts.bin> <script.txt>
// The script, one command per line:
//   flow <slot> <family> <src hex> <dst hex> <src port> <dst port> <ttl> <dscp> <mode> <P> <ssrc> <timestamp base> <seq base> <pid mode> <drop null> <n> <pid> ...
//   rate <ticks_per_packet_q24>
//   call <first packet in ts.bin> <packets> <flush>
// Every call's packets are copied into a heap block of their exact size, so a read past the last packet is a report.  Prints every
// call's rows, then the counters and a hash of each slot's bytes.
#include "../../sdrpp-dvbs-demodulator_amd/csrc/ipout_rules.h"

#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iterator>
#include <memory>
#include <sstream>
#include <string>

using namespace s2;

int main(int argc, char** argv) {
    if (argc < 3) { fprintf(stderr, "usage: ipout_rules_san ts script\n"); return 2; }
    std::ifstream fi(argv[1], std::ios::binary);
    const std::vector<uint8_t> ts((std::istreambuf_iterator<char>(fi)), std::istreambuf_iterator<char>());
    std::ifstream script(argv[2]);
    std::unique_ptr<IpoutHostStream> h(new IpoutHostStream());
    long long packets = 0, bad_sync = 0, cnt[IPOUT_SLOTS][5] = {}, bytes[IPOUT_SLOTS] = {};
    std::string line;
    int c = 0;
    while (std::getline(script, line)) {
        std::istringstream in(line);
        std::string cmd;
        in >> cmd;
        if (cmd == "flow") {
            int slot, family, n;
            std::string src, dst;
            unsigned long long a[11];
            in >> slot >> family >> src >> dst;
            for (unsigned long long& x : a) in >> x;
            in >> n;
            if (!in || slot < 0 || slot >= IPOUT_SLOTS || src.size() != dst.size() || src.size() > 32) { fprintf(stderr, "a bad flow\n"); return 2; }
            IpoutFlow f = {};
            f.family = family;
            for (size_t i = 0; i < src.size() / 2; ++i) {
                f.src_addr[i] = (uint8_t)strtol(src.substr(2 * i, 2).c_str(), nullptr, 16);
                f.dst_addr[i] = (uint8_t)strtol(dst.substr(2 * i, 2).c_str(), nullptr, 16);
            }
            f.src_port = (uint16_t)a[0]; f.dst_port = (uint16_t)a[1]; f.ttl = (uint8_t)a[2]; f.dscp = (uint8_t)a[3]; f.mode = (uint8_t)a[4];
            f.packets_per_datagram = (uint8_t)a[5]; f.ssrc = (uint32_t)a[6]; f.timestamp_base = (uint32_t)a[7]; f.seq_base = (uint16_t)a[8];
            f.pid_mode = (uint8_t)a[9]; f.drop_null = (uint8_t)a[10];
            h->flow[slot] = f;
            memset(h->map[slot], 0, sizeof(h->map[slot]));
            for (int i = 0; i < n; ++i) {
                int pid;
                in >> pid;
                if (!in || pid < 0 || pid >= TSMON_PIDS) { fprintf(stderr, "a bad PID\n"); return 2; }
                h->map[slot][pid >> 5] |= 1u << (pid & 31);
            }
            h->clear_slot(slot);
            for (long long& x : cnt[slot]) x = 0;
        } else if (cmd == "rate") {
            unsigned long long r;
            in >> r;
            h->tpp = r;
        } else if (cmd == "call") {
            long long first, n;
            int flush;
            in >> first >> n >> flush;
            if (!in || first < 0 || n < 0 || (size_t)(first + n) * IPOUT_TS > ts.size()) { fprintf(stderr, "a call outside the stream\n"); return 2; }
            std::unique_ptr<uint8_t[]> exact(n ? new uint8_t[(size_t)n * IPOUT_TS] : nullptr);
            if (n) memcpy(exact.get(), ts.data() + (size_t)first * IPOUT_TS, (size_t)n * IPOUT_TS);
            h->run(exact.get(), (int)n, flush != 0);
            packets += h->packets; bad_sync += h->bad_sync;
            for (int k = 0; k < IPOUT_SLOTS; ++k) {
                cnt[k][0] += h->passed[k]; cnt[k][1] += (long long)h->rows[k].size(); cnt[k][4] += (long long)h->bytes[k].size();
                for (const IpoutRow& r : h->rows[k]) {
                    cnt[k][2] += (r.flags & IPOUT_SHORT) != 0; cnt[k][3] += r.packets;
                    printf("row %d %d %d %d %u %u %u %u %d %u\n", c, k, r.offset, r.bytes, r.rtp_timestamp, r.rtp_seq, r.packets, r.flags, r.first_packet, r.udp_checksum);
                }
                for (uint8_t b : h->bytes[k]) bytes[k] = (bytes[k] * 131 + b) % 1000000007LL;
            }
            ++c;
        } else if (!cmd.empty()) {
            fprintf(stderr, "an unknown command\n");
            return 2;
        }
    }
    printf("stats %lld %lld", packets, bad_sync);
    for (int k = 0; k < IPOUT_SLOTS; ++k) printf(" %lld %lld %lld %lld %lld %d", cnt[k][0], cnt[k][1], cnt[k][2], cnt[k][3], cnt[k][4], h->st.slot[k].held);
    printf("\nbytes %lld %lld %lld %lld\n", bytes[0], bytes[1], bytes[2], bytes[3]);      // a hash of each slot's bytes
    printf("ipout rules run ok\n");
    return 0;
}
