// The IP-TS bank's rules (csrc/ipts_rules.h) alone, under the sanitizers: the host stream (IptsHostStream, one stream).
//   ipts_rules_san <data.bin> <table.bin> <per_call> <kind> <flow> <flow> <flow> <flow>      flow: family:address hex (8 or 32 digits):port, or -
// table.bin: (int32 offset, int32 bytes) per row.  The table in calls of <per_call> rows (0: one call); prints rows and counters.
// Every call's datagrams are copied into a heap block in which the bytes behind each datagram are poisoned, so a read past a
// datagram's end is a report.
#include "../../sdrpp-dvbs-demodulator_amd/csrc/ipts_rules.h"

#ifdef __SANITIZE_ADDRESS__
#include <sanitizer/asan_interface.h>
#else
#define ASAN_POISON_MEMORY_REGION(a, n) ((void)(a), (void)(n))
#define ASAN_UNPOISON_MEMORY_REGION(a, n) ((void)(a), (void)(n))
#endif

#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iterator>
#include <memory>
#include <string>

using namespace s2;

static std::vector<uint8_t> slurp(const char* path) {
    std::ifstream fi(path, std::ios::binary);
    return std::vector<uint8_t>((std::istreambuf_iterator<char>(fi)), std::istreambuf_iterator<char>());
}

static bool parse_flow(const std::string& s, IptsFlow* f) {
    *f = IptsFlow{};
    if (s == "-") return true;
    const size_t a = s.find(':'), b = s.rfind(':');
    if (a == std::string::npos || b == a) return false;
    f->family = atoi(s.substr(0, a).c_str());
    const std::string hex = s.substr(a + 1, b - a - 1);
    if ((f->family != 4 && f->family != 6) || hex.size() != (f->family == 4 ? 8u : 32u)) return false;
    for (size_t i = 0; i < hex.size() / 2; ++i) f->addr[i] = (uint8_t)strtol(hex.substr(2 * i, 2).c_str(), nullptr, 16);
    f->port = atoi(s.substr(b + 1).c_str());
    return true;
}

int main(int argc, char** argv) {
    if (argc < 9) { fprintf(stderr, "usage: ipts_rules_san data table per_call kind flow flow flow flow\n"); return 2; }
    std::unique_ptr<IptsHostStream> h(new IptsHostStream());
    const std::vector<uint8_t> data = slurp(argv[1]), tab = slurp(argv[2]);
    for (int k = 0; k < IPTS_SLOTS; ++k)
        if (!parse_flow(argv[5 + k], &h->flow[k])) { fprintf(stderr, "a bad flow\n"); return 2; }
    if (tab.size() % 8) { fprintf(stderr, "not whole rows\n"); return 2; }
    const int total = (int)(tab.size() / 8), kind = atoi(argv[4]);
    int per_call = atoi(argv[3]);
    if (per_call <= 0) per_call = total > 0 ? total : 1;
    long long tot[IPTS_NSTREAM_CNT + IPTS_SLOTS * IPTS_NSLOT_CNT] = {}, bytes[IPTS_SLOTS] = {};
    for (int a = 0, c = 0; a < total || c == 0; a += per_call, ++c) {
        const int n = total - a < per_call ? total - a : per_call;
        // the call's datagrams in one heap block, each at a multiple of 8 with the 32 to 39 bytes behind it poisoned
        std::vector<int32_t> rows(2 * (size_t)n + 2);
        size_t size = 8;
        for (int r = 0; r < n; ++r) {
            int32_t off, nb;
            memcpy(&off, tab.data() + 8 * (size_t)(a + r), 4); memcpy(&nb, tab.data() + 8 * (size_t)(a + r) + 4, 4);
            rows[2 * r] = off; rows[2 * r + 1] = nb;
            if (off < 0) continue;
            if (nb < 0 || (size_t)off + nb > data.size()) { fprintf(stderr, "a row outside the data\n"); return 2; }
            rows[2 * r] = (int32_t)size;
            size += (((size_t)nb + 7) & ~(size_t)7) + 32;
        }
        std::unique_ptr<uint8_t[]> block(new uint8_t[size]);
        uint8_t* base = block.get();
        for (int r = 0; r < n; ++r) {
            if (rows[2 * r] < 0) continue;
            int32_t off;
            memcpy(&off, tab.data() + 8 * (size_t)(a + r), 4);
            const size_t pos = (size_t)rows[2 * r], nb = (size_t)rows[2 * r + 1], room = ((nb + 7) & ~(size_t)7) + 32;
            memcpy(base + pos, data.data() + off, nb);
            ASAN_POISON_MEMORY_REGION(base + pos + nb, room - nb);
        }
        const IptsView v = {base, reinterpret_cast<const uint8_t*>(rows.data()), 8, 0, 4, kind, n, 0};
        h->run(v, true);
        ASAN_UNPOISON_MEMORY_REGION(base, size);
        const int32_t* k = reinterpret_cast<const int32_t*>(&h->scnt);
        for (int i = 0; i < IPTS_NSTREAM_CNT; ++i) tot[i] += k[i];
        for (int s = 0; s < IPTS_SLOTS; ++s) {
            const int32_t* q = reinterpret_cast<const int32_t*>(&h->cnt[s]);
            for (int i = 0; i < IPTS_NSLOT_CNT; ++i) tot[IPTS_NSTREAM_CNT + s * IPTS_NSLOT_CNT + i] += q[i];
            for (uint8_t b : h->bytes[s]) bytes[s] = (bytes[s] * 131 + b) % 1000000007LL;
        }
        for (const IptsRow& r : h->rows)
            printf("row %d %u %d %u %u %u %u %u %u %u %u %d %d %d %d\n", c, r.flags, r.slot, r.family, r.payload_type, r.src_port, r.dst_port, r.rtp_seq, r.ts_at,
                   r.rtp_timestamp, r.rtp_ssrc, r.packets, r.lost, r.offset, r.bytes);
    }
    printf("stats");
    for (long long v : tot) printf(" %lld", v);
    printf("\nbytes %lld %lld %lld %lld\n", bytes[0], bytes[1], bytes[2], bytes[3]);      // a hash of each slot's delivered bytes
    printf("state");
    for (const IptsSeq& q : h->seq) printf(" %d %u %u", q.has, q.last_seq, q.ssrc);
    printf("\nipts rules run ok\n");
    return 0;
}
