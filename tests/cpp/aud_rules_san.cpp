// The audio bank's rules (csrc/aud_rules.h) alone, under the sanitizers: the host stream (AudHostStream).
//   aud_rules_san <ts.bin> <per_call> <pid,codec> [<pid,codec> ...]  the file in calls of <per_call> packets (0: one call), the pairs watched
//                                                                    in slots 0, 1, ...; prints rows and counters
//   aud_rules_san random <seed> <packets>                            seeded random packets on three PIDs of the three codecs: random
//                                                                    headers, adaptation lengths 0..255, payload bytes biased towards
//                                                                    sync words, short frame headers and PES headers
// Every call's packets are copied into a heap block of exactly their size, so a read past a packet's end is a report.
#include "../../sdrpp-dvbs-demodulator_amd/csrc/aud_rules.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iterator>
#include <memory>
#include <random>
#include <string>

using namespace s2;

struct Totals { long long v[AUD_COUNTERS]; long long packets, dropped, rows; };

static void run_calls(AudHostStream& h, const std::vector<uint8_t>& all, int per_call, int max_rows, Totals* t, bool print_rows) {
    const int total = (int)(all.size() / TSMON_TS);
    if (per_call <= 0) per_call = total > 0 ? total : 1;
    for (int a = 0, c = 0; a < total; a += per_call, ++c) {
        const int n = total - a < per_call ? total - a : per_call;
        std::unique_ptr<uint8_t[]> call(new uint8_t[(size_t)n * TSMON_TS]);
        memcpy(call.get(), all.data() + (size_t)a * TSMON_TS, (size_t)n * TSMON_TS);
        h.run(call.get(), n, max_rows);
        for (int s = 0; s < AUD_SLOTS; ++s) {
            const int32_t* k = &h.cnt[s].packets;
            for (int i = 0; i < AUD_COUNTERS; ++i) t->v[i] += k[i];
        }
        t->rows += h.head.rows;
        if (h.head.rows > max_rows) t->dropped += h.head.rows - max_rows;
        if (print_rows)
            for (const AudRow& r : h.rows)
                printf("row %d %u %u %u %u %u %u %u %u %u %llu %llu %llu %u %u %u\n", c, r.pid, r.slot, r.unit, r.code, r.detail, r.flags, r.packet, r.kbps, r.head,
                       (unsigned long long)r.es_offset, (unsigned long long)r.pts, (unsigned long long)r.dts, r.sample_rate, r.frame_bytes, r.samples);
    }
    t->packets = h.packets;
}

int main(int argc, char** argv) {
    if (argc < 4) { fprintf(stderr, "usage: aud_rules_san ts per_call pid,codec ... | random seed packets\n"); return 2; }
    AudHostStream h;
    Totals t = {};
    std::vector<uint8_t> all;
    const bool random = std::string(argv[1]) == "random";
    int per_call = 0, max_rows = 1 << 20;
    if (random) {
        std::mt19937_64 rng((unsigned)atoi(argv[2]));
        const int n = atoi(argv[3]);
        h.watch[2] = 0x30; h.codec[2] = AUD_MPA; h.watch[9] = 0x31; h.codec[9] = AUD_ADTS; h.watch[15] = 0x32; h.codec[15] = AUD_AC3;
        all.resize((size_t)n * TSMON_TS);
        int cc[3] = {0, 0, 0};
        for (int k = 0; k < n; ++k) {
            uint8_t* p = all.data() + (size_t)k * TSMON_TS;
            const int which = (int)(rng() % 3);
            // short frames of the PID's codec back to back from the payload's likely start on, and noise between: the chain often holds
            // for a few frames, breaks, and is taken up again at a start
            static const uint8_t frame[3][8] = {{0xFF, 0xF3, 0x14, 0xC4, 0, 0, 0, 0}, {0xFF, 0xF1, 0x4C, 0x80, 0x01, 0x3F, 0xFC, 0}, {0x0B, 0x77, 0x00, 0x07, 0x30, 0x80, 0x40, 0}};
            for (int i = 0; i < TSMON_TS; ++i) {
                const unsigned r = (unsigned)rng();
                p[i] = (uint8_t)(r % 16 < 5 ? 0xFF : r % 16 < 7 ? 0x0B : r % 16 < 9 ? 0x77 : r >> 8);
            }
            const int step = which == 0 ? 24 : which == 1 ? 9 : 16;            // the lengths the three headers above say
            if (rng() % 4) for (int i = 18 + (int)(rng() % 3 ? 0 : rng() % 8); i + 8 <= TSMON_TS; i += step) memcpy(p + i, frame[which], 8);
            const bool wild = rng() % 8 == 0;
            const int afc = wild ? (int)(rng() & 3) : (rng() % 3 ? 1 : 3);
            if (rng() % 12) cc[which] = (cc[which] + (afc & 1)) & 15;          // mostly continuous; else an equal counter
            if (rng() % 40 == 0) cc[which] = (int)(rng() & 15);
            p[0] = (uint8_t)(rng() % 50 ? 0x47 : 0x46);
            p[1] = (uint8_t)((rng() % 50 ? 0 : 0x80) | (rng() % 4 ? 0 : 0x40));
            p[2] = (uint8_t)(0x30 + which);
            p[3] = (uint8_t)((rng() % 20 ? 0 : 0x80) | afc << 4 | cc[which]);
            p[4] = (uint8_t)(wild ? rng() : (rng() % 4 ? rng() % 184 : 183 - (1 + rng() % 12)));    // with AFC 3: any length, often a few bytes
            p[5] = (uint8_t)(rng() % 30 ? 0 : 0x80);
            const int L = pes_payload_len(afc, p[4]);
            if (L > 0 && (p[1] & 0x40) && rng() % 6) {                         // something like a PES header where the payload starts
                uint8_t hd[19] = {0, 0, 1, 0xC0, 0, 0, 0x80, 0x80, 5, 0x21, 0, 1, 0, 1, 0xFF, 0xFF, 0xFF, 0xFF, 0xFF};
                hd[8] = (uint8_t)(rng() % 4 ? 5 + rng() % 6 : rng());           // PES_header_data_length: mostly inside the packet, sometimes beyond
                if (rng() % 10 == 0) hd[rng() % 19] ^= (uint8_t)(1u << (rng() % 8));
                memcpy(p + TSMON_TS - L, hd, L < 19 ? L : 19);
                if (L >= 14 + 8 && hd[8] == 5) memcpy(p + TSMON_TS - L + 14, frame[which], 8);      // and a frame where its segment starts
            }
        }
        per_call = 1 + (int)(rng() % 40);
        max_rows = 3;                                              // most calls drop rows
    } else {
        std::ifstream fi(argv[1], std::ios::binary);
        all.assign((std::istreambuf_iterator<char>(fi)), std::istreambuf_iterator<char>());
        if (all.size() % TSMON_TS || argc - 3 > AUD_SLOTS) { fprintf(stderr, "not a whole number of packets, or too many watches\n"); return 2; }
        per_call = atoi(argv[2]);
        for (int s = 0; s + 3 < argc; ++s) {
            int pid = 0, codec = 0;
            if (sscanf(argv[s + 3], "%d,%d", &pid, &codec) != 2) { fprintf(stderr, "a watch is pid,codec\n"); return 2; }
            h.watch[s] = pid; h.codec[s] = codec;
        }
    }
    run_calls(h, all, per_call, max_rows, &t, !random);
    printf("stats");
    for (int i = 0; i < AUD_COUNTERS; ++i) printf(" %lld", t.v[i]);
    printf("\nstream %lld %lld %lld\n", t.packets, t.dropped, t.rows);
    printf("aud rules run ok\n");
    return 0;
}
