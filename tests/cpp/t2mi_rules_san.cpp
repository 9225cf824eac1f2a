// The T2-MI bank's rules (csrc/t2mi_rules.h) alone, under the sanitizers: the host stream (T2miHostStream, one slot).
//   t2mi_rules_san <ts.bin> <per_call> <pid> <plp>     the file in calls of <per_call> packets (0: one call); prints rows and counters
//   t2mi_rules_san random <seed> <packets>             seeded random packets on two PIDs, one of them watched: random headers,
//                                                      adaptation lengths 0..255, pointers of any size and payload bytes biased
//                                                      towards short T2-MI headers, so that packets complete, split and drop
// Every call's packets are copied into a heap block of exactly their size, so a read past a packet's end is a report.
#include "../../sdrpp-dvbs-demodulator_amd/csrc/t2mi_rules.h"

#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iterator>
#include <memory>
#include <random>
#include <string>

using namespace s2;

static void run_calls(T2miHostStream& h, const std::vector<uint8_t>& all, int per_call, long long* tot, long long* bytes, bool print_rows) {
    const int total = (int)(all.size() / TSMON_TS);
    if (per_call <= 0) per_call = total > 0 ? total : 1;
    for (int a = 0, c = 0; a < total; a += per_call, ++c) {
        const int n = total - a < per_call ? total - a : per_call;
        std::unique_ptr<uint8_t[]> call(new uint8_t[(size_t)n * TSMON_TS]);
        memcpy(call.get(), all.data() + (size_t)a * TSMON_TS, (size_t)n * TSMON_TS);
        h.run(call.get(), n, true);
        const int32_t* k = reinterpret_cast<const int32_t*>(&h.cnt);
        for (int i = 0; i < T2MI_NCNT; ++i) tot[i] += k[i];
        for (uint8_t b : h.bytes) *bytes = (*bytes * 131 + b) % 1000000007LL;
        if (print_rows)
            for (const T2miRow& r : h.rows)
                printf("row %d %u %u %u %u %u %u %u %u %d %d %d %d %d\n", c, r.packet_type, r.packet_count, r.superframe_idx, r.stream_id, r.flags, r.plp_id,
                       r.frame_idx, r.payload_bits, r.length, r.offset, r.bbframe_bytes, r.first_packet, r.last_packet);
    }
}

int main(int argc, char** argv) {
    if (argc < 4) { fprintf(stderr, "usage: t2mi_rules_san ts per_call pid plp | random seed packets\n"); return 2; }
    std::unique_ptr<T2miHostStream> h(new T2miHostStream());
    long long tot[T2MI_NCNT] = {}, bytes = 0;
    std::vector<uint8_t> all;
    const bool random = std::string(argv[1]) == "random";
    int per_call = 0;
    if (random) {
        std::mt19937_64 rng((unsigned)atoi(argv[2]));
        const int n = atoi(argv[3]);
        h->watch = {0x40, (int)(rng() % 3) - 1};
        all.resize((size_t)n * TSMON_TS);
        int cc[2] = {0, 0};
        for (int k = 0; k < n; ++k) {
            uint8_t* p = all.data() + (size_t)k * TSMON_TS;
            for (int i = 0; i < TSMON_TS; ++i) p[i] = (uint8_t)(rng() % 4 ? 0 : rng());       // mostly zero: payload_bits stay small, packets complete
            const int which = rng() % 5 == 0;
            const bool wild = rng() % 10 == 0;
            const int afc = wild ? (int)(rng() & 3) : (rng() % 4 ? 1 : 3);
            if (rng() % 15) cc[which] = (cc[which] + (afc & 1)) & 15;                         // mostly continuous; else an equal counter
            if (rng() % 50 == 0) cc[which] = (int)(rng() & 15);
            p[0] = (uint8_t)(rng() % 60 ? 0x47 : 0x46);
            p[1] = (uint8_t)((rng() % 60 ? 0 : 0x80) | (rng() % 3 ? 0 : 0x40));
            p[2] = (uint8_t)(0x40 + which);
            p[3] = (uint8_t)((rng() % 40 ? 0 : 0x80) | afc << 4 | cc[which]);
            p[4] = (uint8_t)(wild ? rng() : rng() % 184);
            p[5] = (uint8_t)(rng() % 30 ? 0 : 0x80);
            const int ps = t2mi_payload_start(afc, p[4]);
            if (ps < TSMON_TS && (p[1] & 0x40)) p[ps] = (uint8_t)(rng() % 6 ? rng() % (TSMON_TS - ps) : rng());   // a pointer that mostly fits
            if (ps + 12 < TSMON_TS && rng() % 3 == 0) { p[ps + 5] = 0; p[ps + 6] = (uint8_t)(rng() % 200); }      // (near the first header's length)
        }
        per_call = 5 + (int)(rng() % 60);
    } else {
        std::ifstream fi(argv[1], std::ios::binary);
        all.assign((std::istreambuf_iterator<char>(fi)), std::istreambuf_iterator<char>());
        if (all.size() % TSMON_TS || argc < 5) { fprintf(stderr, "not a whole number of packets, or no watch\n"); return 2; }
        per_call = atoi(argv[2]);
        h->watch = {atoi(argv[3]), atoi(argv[4])};
    }
    run_calls(*h, all, per_call, tot, &bytes, !random);
    printf("stats");
    for (int i = 0; i < T2MI_NCNT; ++i) printf(" %lld", tot[i]);
    printf("\nbytes %lld %d\n", bytes, h->st.fill);      // a hash of the delivered bytes; the bytes left open
    printf("t2mi rules run ok\n");
    return 0;
}
