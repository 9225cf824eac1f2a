// The PCR bank's rules (csrc/pcr_rules.h) alone, under the sanitizers: the host stream (PcrHostStream).
//   pcr_rules_san <ts.bin> <per_call> <pid of slot 0> <tpp q24>    the file in calls of <per_call> packets (0: one call); prints rows and counters
//   pcr_rules_san random <seed> <packets>                          seeded random packets on three PIDs, two of them watched: random
//                                                                  adaptation lengths, flags and PCR bytes, steps of every size and sign
// Every call's packets are copied into a heap block of exactly their size, so a read past a packet's end is a report.
#include "../../sdrpp-dvbs-demodulator_amd/csrc/pcr_rules.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iterator>
#include <memory>
#include <random>
#include <string>

using namespace s2;

struct Totals { PcrCnt cnt; long long packets, unwatched, dropped, records; int first_unwatched; };

static void run_calls(PcrHostStream& h, const std::vector<uint8_t>& all, int per_call, int max_rows, Totals* t, bool print_rows) {
    const int total = (int)(all.size() / TSMON_TS);
    if (per_call <= 0) per_call = total > 0 ? total : 1;
    for (int a = 0, c = 0; a < total; a += per_call, ++c) {
        const int n = total - a < per_call ? total - a : per_call;
        std::unique_ptr<uint8_t[]> call(new uint8_t[(size_t)n * TSMON_TS]);
        memcpy(call.get(), all.data() + (size_t)a * TSMON_TS, (size_t)n * TSMON_TS);
        h.run(call.get(), n, max_rows);
        for (int s = 0; s < PCR_SLOTS; ++s) {
            const PcrCnt& k = h.cnt[s];
            for (int i = 0; i < PCR_KINDS; ++i) t->cnt.kind[i] += k.kind[i];
            t->cnt.malformed += k.malformed; t->cnt.accuracy_measured += k.accuracy_measured; t->cnt.accuracy_errors += k.accuracy_errors;
            t->cnt.sum_ticks += k.sum_ticks; t->cnt.sum_packets += k.sum_packets;
            if (k.max_delta_ticks > t->cnt.max_delta_ticks) t->cnt.max_delta_ticks = k.max_delta_ticks;
            if (k.max_abs_accuracy > t->cnt.max_abs_accuracy) t->cnt.max_abs_accuracy = k.max_abs_accuracy;
        }
        t->unwatched += h.head.unwatched; t->records += h.head.records; t->first_unwatched = h.head.first_unwatched_pid;
        if (h.head.records > max_rows) t->dropped += h.head.records - max_rows;
        if (print_rows)
            for (const PcrRow& r : h.rows)
                printf("row %d %u %u %u %u %d %llu %u %u %d\n", c, r.pid, r.slot, r.kind, r.flags, r.packet, (unsigned long long)r.pcr, r.delta_ticks, r.delta_packets,
                       r.accuracy);
    }
    t->packets = h.packets;
}

int main(int argc, char** argv) {
    if (argc < 4) { fprintf(stderr, "usage: pcr_rules_san ts per_call pid tpp | random seed packets\n"); return 2; }
    PcrHostStream h;
    Totals t = {pcr_cnt_zero(), 0, 0, 0, 0, -1};
    std::vector<uint8_t> all;
    const bool random = std::string(argv[1]) == "random";
    int per_call = 0, max_rows = 1 << 20;
    if (random) {
        std::mt19937_64 rng((unsigned)atoi(argv[2]));
        const int n = atoi(argv[3]);
        h.watch[2] = 0x30; h.watch[9] = 0x31;
        h.rate = {rng() % PCR_MAX_TPP, (int32_t)(rng() % 4000), 0};
        all.resize((size_t)n * TSMON_TS);
        uint64_t clock[3] = {0, PCR_MOD - 5000000, 123456789};
        for (int k = 0; k < n; ++k) {
            uint8_t* p = all.data() + (size_t)k * TSMON_TS;
            for (int i = 0; i < TSMON_TS; ++i) p[i] = (uint8_t)rng();
            const int which = (int)(rng() % 3);
            const bool wild = rng() % 8 == 0;
            p[0] = (uint8_t)(rng() % 50 ? 0x47 : 0x46); p[1] = (uint8_t)(rng() % 50 ? 0 : 0x80); p[2] = (uint8_t)(0x30 + which);
            p[3] = (uint8_t)((wild ? rng() & 3 : 3) << 4 | (rng() & 0xCF));
            p[4] = (uint8_t)(wild ? rng() : 7 + rng() % 100);
            p[5] = (uint8_t)(wild ? rng() : 0x10 | (rng() % 40 ? 0 : 0x80));
            if (!wild || rng() % 2) {                                  // a clock that steps forward by anything up to seconds, sometimes back, sometimes not at all
                const uint64_t step = rng() % 5 == 0 ? 0 : (rng() % 7 == 0 ? rng() % PCR_MOD : rng() % (rng() % 3 ? 60000 : 4000000));
                clock[which] = (clock[which] + step) % PCR_MOD;
                const uint64_t base = clock[which] / 300, ext = clock[which] % 300;
                p[6] = (uint8_t)(base >> 25); p[7] = (uint8_t)(base >> 17); p[8] = (uint8_t)(base >> 9); p[9] = (uint8_t)(base >> 1);
                p[10] = (uint8_t)((base & 1) << 7 | 0x7E | ext >> 8); p[11] = (uint8_t)ext;
            }
        }
        per_call = 10 + (int)(rng() % 40);
        max_rows = 2;                                              // every call drops rows
    } else {
        std::ifstream fi(argv[1], std::ios::binary);
        all.assign((std::istreambuf_iterator<char>(fi)), std::istreambuf_iterator<char>());
        if (all.size() % TSMON_TS || argc < 5) { fprintf(stderr, "not a whole number of packets, or no rate\n"); return 2; }
        per_call = atoi(argv[2]);
        h.watch[0] = atoi(argv[3]);
        h.rate.tpp = strtoull(argv[4], nullptr, 10);
    }
    run_calls(h, all, per_call, max_rows, &t, !random);
    const PcrCnt& c = t.cnt;
    printf("stats %lld %d %d %d %d %d %d %d %d %d %llu %llu %u %u\n", t.records, c.kind[PCR_FIRST], c.kind[PCR_ANNOUNCED], c.kind[PCR_REPEATED], c.kind[PCR_JUMP],
           c.kind[PCR_LATE], c.kind[PCR_OK], c.malformed, c.accuracy_measured, c.accuracy_errors, (unsigned long long)c.sum_ticks, (unsigned long long)c.sum_packets,
           c.max_delta_ticks, c.max_abs_accuracy);
    printf("stream %lld %lld %lld %d\n", t.packets, t.unwatched, t.dropped, t.first_unwatched);
    printf("pcr rules run ok\n");
    return 0;
}
