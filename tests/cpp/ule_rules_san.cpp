// The ULE bank's rules (csrc/ule_rules.h) alone, under the sanitizers: the host stream (UleHostStream, one slot).
//   ule_rules_san <ts.bin> <per_call> <pid> <npa_value hex12> <npa_mask hex12> <accept_unaddressed>
// The file in calls of <per_call> packets (0: one call); prints rows and counters.  Every call's packets are copied into a heap block
// of exactly their size, so a read past a packet's end is a report.
#include "../../sdrpp-dvbs-demodulator_amd/csrc/ule_rules.h"

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
    if (argc < 7) { fprintf(stderr, "usage: ule_rules_san ts per_call pid npa_value npa_mask accept_unaddressed\n"); return 2; }
    std::unique_ptr<UleHostStream> h(new UleHostStream());
    std::ifstream fi(argv[1], std::ios::binary);
    const std::vector<uint8_t> all((std::istreambuf_iterator<char>(fi)), std::istreambuf_iterator<char>());
    h->watch.pid = atoi(argv[3]);
    h->watch.accept_unaddressed = atoi(argv[6]);
    if (all.size() % TSMON_TS || !hex6(argv[4], h->watch.npa_value) || !hex6(argv[5], h->watch.npa_mask)) { fprintf(stderr, "not whole packets, or a bad NPA\n"); return 2; }
    const int total = (int)(all.size() / TSMON_TS);
    int per_call = atoi(argv[2]);
    if (per_call <= 0) per_call = total > 0 ? total : 1;
    long long tot[ULE_NCNT] = {}, bytes = 0;
    for (int a = 0, c = 0; a < total; a += per_call, ++c) {
        const int n = total - a < per_call ? total - a : per_call;
        std::unique_ptr<uint8_t[]> call(new uint8_t[(size_t)n * TSMON_TS]);
        memcpy(call.get(), all.data() + (size_t)a * TSMON_TS, (size_t)n * TSMON_TS);
        h->run(call.get(), n, true);
        const int32_t* k = reinterpret_cast<const int32_t*>(&h->cnt);
        for (int i = 0; i < ULE_NCNT; ++i) tot[i] += k[i];
        for (uint8_t b : h->bytes) bytes = (bytes * 131 + b) % 1000000007LL;
        for (const UleRow& r : h->rows)
            printf("row %d %u %u %u %02x%02x%02x%02x%02x%02x %u %u %u %u %u %u %d %d %d %d %d %u %u\n", c, r.flags, r.family, r.protocol, r.mac[0], r.mac[1], r.mac[2],
                   r.mac[3], r.mac[4], r.mac[5], r.ip_at, r.extension_bytes, r.src_port, r.dst_port, r.src4, r.dst4, r.length, r.offset, r.bytes,
                   r.first_packet, r.last_packet, r.ethertype, r.stuffing);
    }
    printf("stats");
    for (int i = 0; i < ULE_NCNT; ++i) printf(" %lld", tot[i]);
    printf("\nbytes %lld %d\n", bytes, h->st.fill);      // a hash of the delivered bytes; the bytes left open
    printf("ule rules run ok\n");
    return 0;
}
