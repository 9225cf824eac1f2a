// The PES bank's rules (csrc/pes_rules.h) alone, under the sanitizers: the host stream (PesHostStream).
//   pes_rules_san <ts.bin> <per_call> <pid of slot 0> <tpp q24>    the file in calls of <per_call> packets (0: one call); prints rows and counters
//   pes_rules_san random <seed> <packets>                          seeded random packets on three PIDs, two of them watched: random
//                                                                  headers, adaptation lengths 0..255 and payload bytes biased towards
//                                                                  PES syntax, timestamps that step by anything
// Every call's packets are copied into a heap block of exactly their size, so a read past a packet's end is a report.
#include "../../sdrpp-dvbs-demodulator_amd/csrc/pes_rules.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iterator>
#include <memory>
#include <random>
#include <string>

using namespace s2;

struct Totals { long long v[24]; long long packets, dropped, starts; };

static void run_calls(PesHostStream& h, const std::vector<uint8_t>& all, int per_call, int max_rows, Totals* t, bool print_rows) {
    const int total = (int)(all.size() / TSMON_TS);
    if (per_call <= 0) per_call = total > 0 ? total : 1;
    for (int a = 0, c = 0; a < total; a += per_call, ++c) {
        const int n = total - a < per_call ? total - a : per_call;
        std::unique_ptr<uint8_t[]> call(new uint8_t[(size_t)n * TSMON_TS]);
        memcpy(call.get(), all.data() + (size_t)a * TSMON_TS, (size_t)n * TSMON_TS);
        h.run(call.get(), n, max_rows);
        for (int s = 0; s < PES_SLOTS; ++s) {
            const PesCnt& k = h.cnt[s];
            const long long add[23] = {k.packets, k.payload_bytes, k.duplicates, k.cc_errors, k.scrambled_packets, k.malformed_packets,
                                       k.kind[0] + k.kind[1] + k.kind[2] + k.kind[3] + k.kind[4] + k.kind[5], k.kind[PES_SCRAMBLED], k.kind[PES_SHORT],
                                       k.kind[PES_BAD_START], k.kind[PES_PLAIN], k.kind[PES_MALFORMED], k.kind[PES_HEADER], k.with_pts, k.with_dts, k.closed_ok,
                                       k.closed_mismatch, k.closed_gap, k.closed_unchecked, k.ts_backward, k.ts_gap, k.pts_late, k.dts_after_pts};
            for (int i = 0; i < 23; ++i) t->v[i] += add[i];
            if ((long long)k.max_delta_packets > t->v[23]) t->v[23] = k.max_delta_packets;
        }
        t->starts += h.head.starts;
        if (h.head.starts > max_rows) t->dropped += h.head.starts - max_rows;
        if (print_rows)
            for (const PesRow& r : h.rows)
                printf("row %d %u %u %u %u %u %d %u %llu %llu %u %u %u %d\n", c, r.pid, r.slot, r.kind, r.flags, r.stream_id, r.packet, r.declared,
                       (unsigned long long)r.pts, (unsigned long long)r.dts, r.closed_bytes, r.closed_packets, r.delta_packets, r.delta_ts);
    }
    t->packets = h.packets;
}

int main(int argc, char** argv) {
    if (argc < 4) { fprintf(stderr, "usage: pes_rules_san ts per_call pid tpp | random seed packets\n"); return 2; }
    PesHostStream h;
    Totals t = {};
    std::vector<uint8_t> all;
    const bool random = std::string(argv[1]) == "random";
    int per_call = 0, max_rows = 1 << 20;
    if (random) {
        std::mt19937_64 rng((unsigned)atoi(argv[2]));
        const int n = atoi(argv[3]);
        h.watch[2] = 0x30; h.watch[9] = 0x31;
        h.rate = pes_rate(rng() % PES_MAX_TPP);
        all.resize((size_t)n * TSMON_TS);
        uint64_t clock[3] = {0, PES_TS_MOD - 50000, 123456789};
        int cc[3] = {0, 0, 0};
        for (int k = 0; k < n; ++k) {
            uint8_t* p = all.data() + (size_t)k * TSMON_TS;
            for (int i = 0; i < TSMON_TS; ++i) p[i] = (uint8_t)rng();
            const int which = (int)(rng() % 3);
            const bool wild = rng() % 8 == 0;
            const int afc = wild ? (int)(rng() & 3) : (rng() % 3 ? 1 : 3);
            if (rng() % 12) cc[which] = (cc[which] + (afc & 1)) & 15;          // mostly continuous; else an equal counter
            if (rng() % 40 == 0) cc[which] = (int)(rng() & 15);
            p[0] = (uint8_t)(rng() % 50 ? 0x47 : 0x46);
            p[1] = (uint8_t)((rng() % 50 ? 0 : 0x80) | (rng() % 3 ? 0 : 0x40));
            p[2] = (uint8_t)(0x30 + which);
            p[3] = (uint8_t)((rng() % 20 ? 0 : 0x80) | afc << 4 | cc[which]);
            p[4] = (uint8_t)(wild ? rng() : (rng() % 4 ? 183 - (1 + rng() % 30) : rng() % 184));      // with AFC 3: mostly short payloads
            p[5] = (uint8_t)(rng() % 30 ? 0 : 0x80);
            const int L = pes_payload_len(afc, p[4]);
            if (L > 0 && (p[1] & 0x40) && rng() % 6) {                         // something like a PES header where the payload starts
                uint8_t hd[19] = {0, 0, 1, 0xE0, 0, 0, 0x80, 0, 10};
                const int fl = (int)(rng() % 8 ? 2 + rng() % 2 : rng() % 4);
                const uint64_t step = rng() % 5 == 0 ? rng() % PES_TS_MOD : rng() % 100000;
                clock[which] = (clock[which] + step) % PES_TS_MOD;
                const uint64_t v[2] = {clock[which], (clock[which] + PES_TS_MOD - rng() % 4000 + 400) % PES_TS_MOD};
                const uint8_t sids[6] = {0xE0, 0xC0, 0xBD, 0xBE, 0xFF, 0xF3};
                hd[3] = sids[rng() % 6]; hd[4] = (uint8_t)(rng() % 3 ? 0 : rng()); hd[5] = (uint8_t)rng();
                hd[7] = (uint8_t)(fl << 6);
                hd[8] = (uint8_t)(rng() % 10 ? 10 : rng() % 12);
                for (int j = 0; j < 2; ++j) {
                    uint8_t* b = hd + 9 + 5 * j;
                    const unsigned prefix = j ? 1 : (unsigned)fl;
                    b[0] = (uint8_t)(prefix << 4 | (v[j] >> 30 & 7) << 1 | 1); b[1] = (uint8_t)(v[j] >> 22); b[2] = (uint8_t)((v[j] >> 15 & 127) << 1 | 1);
                    b[3] = (uint8_t)(v[j] >> 7); b[4] = (uint8_t)((v[j] & 127) << 1 | 1);
                }
                if (rng() % 10 == 0) hd[rng() % 19] ^= (uint8_t)(1u << (rng() % 8));                      // one flipped bit: markers, prefixes, the start code
                memcpy(p + TSMON_TS - L, hd, L < 19 ? L : 19);
            }
        }
        per_call = 10 + (int)(rng() % 40);
        max_rows = 2;                                              // most calls drop rows
    } else {
        std::ifstream fi(argv[1], std::ios::binary);
        all.assign((std::istreambuf_iterator<char>(fi)), std::istreambuf_iterator<char>());
        if (all.size() % TSMON_TS || argc < 5) { fprintf(stderr, "not a whole number of packets, or no rate\n"); return 2; }
        per_call = atoi(argv[2]);
        h.watch[0] = atoi(argv[3]);
        h.rate = pes_rate(strtoull(argv[4], nullptr, 10));
    }
    run_calls(h, all, per_call, max_rows, &t, !random);
    printf("stats");
    for (int i = 0; i < 24; ++i) printf(" %lld", t.v[i]);
    printf("\nstream %lld %lld %lld\n", t.packets, t.dropped, t.starts);
    printf("pes rules run ok\n");
    return 0;
}
