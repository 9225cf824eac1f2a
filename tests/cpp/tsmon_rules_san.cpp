// The TS monitor's rules (csrc/tsmon_rules.h) alone, under the sanitizers: a plain sequential monitor built from tsmon_parse,
// tsmon_row_add and tsmon_passes, run over a file of packets in calls of <per_call> packets.
//   tsmon_rules_san <ts.bin> <out.bin> <per_call> <mode> <drop_null> <drop_tei> <drop_bad_sync> [<pid> ...]
// Every call's packets are copied into a heap block of exactly their size, so a read past a packet's end is a report.  Writes the
// passing packets to out.bin and prints the counters and the PID table of the last call.
#include "../../sdrpp-dvbs-demodulator_amd/csrc/tsmon_rules.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iterator>
#include <map>
#include <memory>
#include <vector>

using namespace s2;

int main(int argc, char** argv) {
    if (argc < 8) { fprintf(stderr, "usage: tsmon_rules_san ts out per_call mode drop_null drop_tei drop_bad_sync pid...\n"); return 2; }
    std::ifstream fi(argv[1], std::ios::binary);
    const std::vector<uint8_t> all((std::istreambuf_iterator<char>(fi)), std::istreambuf_iterator<char>());
    if (all.size() % TSMON_TS) { fprintf(stderr, "not a whole number of packets\n"); return 2; }
    const int total = (int)(all.size() / TSMON_TS), per_call = atoi(argv[3]) > 0 ? atoi(argv[3]) : (total > 0 ? total : 1);
    const TsmonFilter f = {atoi(argv[4]), atoi(argv[5]), atoi(argv[6]), atoi(argv[7])};
    std::vector<uint32_t> map(TSMON_MAP_WORDS, 0);
    for (int k = 8; k < argc; ++k) { const int p = atoi(argv[k]) & (TSMON_PIDS - 1); map[p >> 5] |= 1u << (p & 31); }
    std::vector<uint8_t> state(TSMON_PIDS, 0), out;
    long long cnt[10] = {};          // packets, null, tei, sync, cc, dup, disc, scrambled, passed, pids_seen
    std::map<int, TsmonRow> tab;
    for (int a = 0; a < total || a == 0; a += per_call) {
        const int n = total - a < per_call ? total - a : per_call;
        std::unique_ptr<uint8_t[]> call(new uint8_t[(size_t)n * TSMON_TS]);
        if (n > 0) memcpy(call.get(), all.data() + (size_t)a * TSMON_TS, (size_t)n * TSMON_TS);
        tab.clear();
        for (int k = 0; k < n; ++k) {
            const uint8_t* p = call.get() + (size_t)k * TSMON_TS;
            const TsmonHdr h = tsmon_parse(p);
            ++cnt[0];
            cnt[1] += h.cls == TSMON_NULL; cnt[2] += h.cls == TSMON_TEI; cnt[3] += h.cls == TSMON_SYNC_ERROR;
            if (tsmon_passes(h, f, map.data())) { ++cnt[8]; out.insert(out.end(), p, p + TSMON_TS); }
            if (h.cls < TSMON_NULL) continue;
            TsmonRow& r = tab.emplace(h.pid, TsmonRow{(uint16_t)h.pid, 0, 0, 0, 0, 0, 0}).first->second;
            const TsmonRow before = r;
            const int v = tsmon_row_add(&r, &state[h.pid], h);
            cnt[4] += r.cc_errors - before.cc_errors; cnt[5] += r.duplicates - before.duplicates; cnt[7] += r.scrambled - before.scrambled;
            cnt[6] += v == TSMON_DISC; cnt[9] += v == TSMON_FIRST;
        }
        if (total == 0) break;
    }
    std::ofstream(argv[2], std::ios::binary).write((const char*)out.data(), (std::streamsize)out.size());
    printf("stats");
    for (long long c : cnt) printf(" %lld", c);
    printf("\n");
    for (const auto& kv : tab) {
        const TsmonRow& r = kv.second;
        printf("row %u %u %u %u %u %u %u\n", r.pid, r.flags, r.packets, r.cc_errors, r.duplicates, r.scrambled, r.pusi);
    }
    printf("tsmon rules run ok\n");
    return 0;
}
