// The MPE bank's rules (csrc/mpe_rules.h) alone, under the sanitizers: the host stream (MpeHostStream, one slot).
//   mpe_rules_san <ts.bin> <per_call> <pid> <mac_value hex12> <mac_mask hex12>
// The file in calls of <per_call> packets (0: one call); prints rows and counters.  Every call's packets are copied into a heap block
// of exactly their size, so a read past a packet's end is a report.
#include "../../sdrpp-dvbs-demodulator_amd/csrc/mpe_rules.h"

#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iterator>
#include <memory>
#include <string>

using namespace s2;

static bool hex6(const char* s, uint8_t* out) {
    if (std::string(s).size() != 12) return false;
    for (int i = 0; i < 6; ++i) out[i] = (uint8_t)strtol(std::string(s + 2 * i, 2).c_str(), nullptr, 16);
    return true;
}

int main(int argc, char** argv) {
    if (argc < 6) { fprintf(stderr, "usage: mpe_rules_san ts per_call pid mac_value mac_mask\n"); return 2; }
    std::unique_ptr<MpeHostStream> h(new MpeHostStream());
    std::ifstream fi(argv[1], std::ios::binary);
    const std::vector<uint8_t> all((std::istreambuf_iterator<char>(fi)), std::istreambuf_iterator<char>());
    h->watch.pid = atoi(argv[3]);
    if (all.size() % TSMON_TS || !hex6(argv[4], h->watch.mac_value) || !hex6(argv[5], h->watch.mac_mask)) { fprintf(stderr, "not whole packets, or a bad MAC\n"); return 2; }
    const int total = (int)(all.size() / TSMON_TS);
    int per_call = atoi(argv[2]);
    if (per_call <= 0) per_call = total > 0 ? total : 1;
    long long tot[MPE_NCNT] = {}, bytes = 0;
    for (int a = 0, c = 0; a < total; a += per_call, ++c) {
        const int n = total - a < per_call ? total - a : per_call;
        std::unique_ptr<uint8_t[]> call(new uint8_t[(size_t)n * TSMON_TS]);
        memcpy(call.get(), all.data() + (size_t)a * TSMON_TS, (size_t)n * TSMON_TS);
        h->run(call.get(), n, true);
        const int32_t* k = reinterpret_cast<const int32_t*>(&h->cnt);
        for (int i = 0; i < MPE_NCNT; ++i) tot[i] += k[i];
        for (uint8_t b : h->bytes) bytes = (bytes * 131 + b) % 1000000007LL;
        for (const MpeRow& r : h->rows)
            printf("row %d %u %u %u %02x%02x%02x%02x%02x%02x %u %u %u %u %u %u %d %d %d %d %d %u %u\n", c, r.flags, r.family, r.protocol, r.mac[0], r.mac[1], r.mac[2],
                   r.mac[3], r.mac[4], r.mac[5], r.section_number, r.last_section_number, r.src_port, r.dst_port, r.src4, r.dst4, r.length, r.offset, r.bytes,
                   r.first_packet, r.last_packet, r.ethertype, r.stuffing);
    }
    printf("stats");
    for (int i = 0; i < MPE_NCNT; ++i) printf(" %lld", tot[i]);
    printf("\nbytes %lld %d\n", bytes, h->st.fill);      // a hash of the delivered bytes; the bytes left open
    printf("mpe rules run ok\n");
    return 0;
}
