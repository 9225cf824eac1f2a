// The PSI section bank's rules (csrc/psi_rules.h) alone, under the sanitizers: the host assembler (PsiHostStream) and the PAT / PMT
// parsers.
//   psi_rules_san <ts.bin> <per_call> <pid of slot 1>    the file in calls of <per_call> packets (0: one call); prints counters and rows
//   psi_rules_san random <seed> <packets>                seeded random packets on a watched PID: random pointer fields, section
//                                                        lengths and adaptation lengths, a tenth of them with random header bits
// Every call's packets are copied into a heap block of exactly their size, so a read past a packet's end is a report; every valid
// changed PAT / PMT goes through its parser from a heap block of exactly the section's size.
#include "../../sdrpp-dvbs-demodulator_amd/csrc/psi_rules.h"

#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iterator>
#include <memory>
#include <random>
#include <string>

using namespace s2;

static long long g_parsed = 0;
static void parse_views(PsiHostStream& h) {
    for (int s = 0; s < PSI_SLOTS; ++s) {
        if (!h.view_new[s]) continue;
        const size_t n = h.view[s].size();
        std::unique_ptr<uint8_t[]> sec(new uint8_t[n]);
        memcpy(sec.get(), h.view[s].data(), n);
        std::vector<PsiProgram> pr;
        std::vector<PsiEs> es;
        if (sec[0] == 0) g_parsed += psi_parse_pat(sec.get(), (int)n, &pr).malformed + (long long)pr.size();
        else g_parsed += psi_parse_pmt(sec.get(), (int)n, &es).malformed + (long long)es.size();
    }
}
static void run_calls(PsiHostStream& h, const std::vector<uint8_t>& all, int per_call, long long* cnt, bool print_rows) {
    const int total = (int)(all.size() / TSMON_TS);
    if (per_call <= 0) per_call = total > 0 ? total : 1;
    for (int a = 0, c = 0; a < total; a += per_call, ++c) {
        const int n = total - a < per_call ? total - a : per_call;
        std::unique_ptr<uint8_t[]> call(new uint8_t[(size_t)n * TSMON_TS]);
        memcpy(call.get(), all.data() + (size_t)a * TSMON_TS, (size_t)n * TSMON_TS);
        h.run(call.get(), n, true);
        parse_views(h);
        for (int s = 0; s < PSI_SLOTS; ++s)
            for (int k = 0; k < PSI_NCNT; ++k) cnt[k] += reinterpret_cast<const int32_t*>(&h.cnt[s])[k];
        if (print_rows)
            for (const PsiRow& r : h.rows)
                printf("row %d %u %u %u %u %u %u %u %u %u %d %d %d\n", c, r.pid, r.flags, r.table_id, r.ssi, r.version, r.current_next, r.section_number,
                       r.last_section_number, r.table_id_ext, r.length, r.offset, r.first_packet);
    }
}

int main(int argc, char** argv) {
    if (argc < 4) { fprintf(stderr, "usage: psi_rules_san ts per_call pid | random seed packets\n"); return 2; }
    PsiHostStream h;
    long long cnt[PSI_NCNT] = {};
    std::vector<uint8_t> all;
    const bool random = std::string(argv[1]) == "random";
    int per_call = 0;
    if (random) {
        std::mt19937 rng((unsigned)atoi(argv[2]));
        const int n = atoi(argv[3]);
        h.watch[1] = {0x30, 2};
        all.resize((size_t)n * TSMON_TS);
        int cc = 0;
        for (int k = 0; k < n; ++k) {
            uint8_t* p = all.data() + (size_t)k * TSMON_TS;
            for (int i = 0; i < TSMON_TS; ++i) p[i] = (uint8_t)(rng() % 7 == 0 ? 0xFF : rng());
            const bool wild = rng() % 10 == 0;
            const int afc = wild ? rng() & 3 : (rng() % 4 == 0 ? 3 : 1);
            p[0] = 0x47; p[1] = (uint8_t)((rng() % 3 == 0) << 6); p[2] = 0x30;
            cc = wild ? (int)(rng() & 15) : (cc + 1) & 15;
            p[3] = (uint8_t)(afc << 4 | cc | (wild && rng() % 4 == 0 ? 0x80 : 0));
            if (afc & 2) p[4] = (uint8_t)(wild ? rng() : rng() % 184);
            const int ps = psi_payload_start(afc, p[4]);
            if ((p[1] & 0x40) && ps < TSMON_TS) {                       // a pointer, then section headers with lengths of every size
                p[ps] = (uint8_t)(wild ? rng() : rng() % (TSMON_TS - ps));
                for (int at = ps + 1 + p[ps]; at + 3 <= TSMON_TS; at += 3 + (int)(rng() % 40)) {
                    p[at] = (uint8_t)(rng() % 2 ? 0 : 2); p[at + 1] = (uint8_t)((rng() & 0x80) | 0x30 | (rng() % 8 == 0 ? rng() & 15 : 0)); p[at + 2] = (uint8_t)rng();
                }
            }
        }
        per_call = 1 + (int)(rng() % 50);
    } else {
        std::ifstream fi(argv[1], std::ios::binary);
        all.assign((std::istreambuf_iterator<char>(fi)), std::istreambuf_iterator<char>());
        if (all.size() % TSMON_TS) { fprintf(stderr, "not a whole number of packets\n"); return 2; }
        per_call = atoi(argv[2]);
        h.watch[1] = {atoi(argv[3]), -1};
    }
    run_calls(h, all, per_call, cnt, !random);
    printf("stats");
    for (long long c : cnt) printf(" %lld", c);
    printf("\nparsed %lld\n", g_parsed);
    // the parsers on cut and damaged sections: every prefix of a PMT-shaped block, from a heap block of exactly its size
    std::mt19937 rng(99);
    for (int n = 0; n <= 64; ++n)
        for (int rep = 0; rep < 20; ++rep) {
            std::unique_ptr<uint8_t[]> sec(new uint8_t[n ? n : 1]);
            for (int i = 0; i < n; ++i) sec[i] = (uint8_t)(rng() % 3 ? rng() & 0x0F : rng());
            std::vector<PsiProgram> pr;
            std::vector<PsiEs> es;
            g_parsed += psi_parse_pat(sec.get(), n, &pr).malformed + psi_parse_pmt(sec.get(), n, &es).malformed;
        }
    printf("psi rules run ok\n");
    return 0;
}
