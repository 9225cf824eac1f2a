// csrc/fec_encode_rules.h on its own, no GPU: the encoder's tables for all 21 codes.  Built with -fsanitize=address,undefined by tests/test_host_cpp_fec_encode_rules.py.
//   BCH   g has degree m t, g(0) = 1 and every alpha^1 .. alpha^2t as a root (evaluated in the field, built here a second time); the byte table and the
//         chunk-shift rows are reduced (degree < P) and are what shift-and-reduce gives: table[v] = v(x) x^P mod g by Horner over the bits of v, row (c, i) =
//         x * row (c, i - 1), the last chunk's rows the unit vectors; the chunks tile the message up to its last byte and the seams are where they begin;
//         a model of the kernel -- byte-table LFSR per chunk, rows, XOR -- gives the parity of the bit-serial LFSR on a random message.
//   LDPC  links per layer as QC_CODES has them, r inside the information blocks, rotation < 360, edges() == QC_CODES[..].edges; the funnel-shift reading of a
//         rotated block (13-word extended block, two adjacent words) equals the bit-by-bit rotation; blocks + layers fit the kernel's LDS rows.
//   sizes kbch, K, N whole bytes (the header's static_assert, looked at again at run time), parity lengths whole bytes.
// Exit status 0: all checks passed; otherwise the failed checks are on stderr.
#include "fec_encode_rules.h"

#include <cstdio>
#include <cstdlib>
#include <vector>

using namespace s2;
using namespace s2::fecenc;

static int failures = 0;
#define CHECK(cond, ...)                                                          \
    do {                                                                          \
        if (!(cond)) { ++failures; fprintf(stderr, "FAILED %s: ", #cond); fprintf(stderr, __VA_ARGS__); fputc('\n', stderr); } \
    } while (0)

static uint32_t rnd_state = 12345u;
static uint32_t rnd() { rnd_state = rnd_state * 1664525u + 1013904223u; return rnd_state >> 8; }

static Poly row_of(const std::vector<uint32_t>& v, size_t idx) {
    Poly p;
    for (int w = 0; w < BCH_WORDS; ++w) p.w[w] = v[idx * BCH_WORDS + w];
    return p;
}
static bool same(const Poly& a, const Poly& b) {
    for (int w = 0; w < BCH_WORDS; ++w) if (a.w[w] != b.w[w]) return false;
    return true;
}

// g(alpha^i) in GF(2^m), the field built independently of the header
static uint32_t eval_at_root(const std::vector<uint8_t>& gen, int m, int i) {
    const uint32_t field = m == 16 ? 0x1002Du : 0x402Bu, Q = 1u << m;
    auto mul = [&](uint32_t a, uint32_t b) {
        uint32_t r = 0;
        for (; b; b >>= 1) { if (b & 1u) r ^= a; a <<= 1; if (a & Q) a ^= field; }
        return r;
    };
    uint32_t root = 1;
    for (int k = 0; k < i; ++k) root = mul(root, 2u);
    uint32_t acc = 0;
    for (int k = (int)gen.size() - 1; k >= 0; --k) acc = mul(acc, root) ^ gen[k];
    return acc;
}

static void check_bch(int rate, int shortframes, const FecParams& f) {
    const BchRules B = build_bch_rules(f.bch_m, f.bch_t);
    const int P = f.bch_m * f.bch_t;
    CHECK(B.P == P && P == f.K - f.kbch && P % 8 == 0 && P <= 32 * BCH_WORDS, "rate %d short %d: P %d", rate, shortframes, B.P);
    if (B.P != P) return;
    CHECK((int)B.gen.size() == P + 1 && B.gen[0] == 1 && B.gen[P] == 1, "generator ends");
    for (int i = 1; i <= 2 * f.bch_t; ++i) CHECK(eval_at_root(B.gen, f.bch_m, i) == 0, "alpha^%d is no root (m %d t %d)", i, f.bch_m, f.bch_t);
    CHECK(poly_degree(B.g_low) < P, "g_low degree");
    // byte table
    for (int v = 0; v < 256; ++v) {
        Poly p;         // Horner over the bits of v, then P more shifts
        for (int b = 7; b >= 0; --b) { p = poly_times_x(p, B.g_low, P); if ((v >> b) & 1) p.w[0] ^= 1u; }
        for (int k = 0; k < P; ++k) p = poly_times_x(p, B.g_low, P);
        const Poly t = row_of(B.byte_tab, (size_t)v);
        CHECK(poly_degree(t) < P && same(t, p), "byte table entry %d", v);
    }
    const BchChunkPlan C = build_bch_chunk_plan(B, f.kbch);
    CHECK(C.msg_bytes == f.kbch / 8 && C.chunk_bytes >= 1 && BCH_CHUNKS * C.chunk_bytes >= C.msg_bytes && BCH_CHUNKS * (C.chunk_bytes - 1) < C.msg_bytes,
          "chunk cut %d x %d for %d bytes", BCH_CHUNKS, C.chunk_bytes, C.msg_bytes);
    CHECK(C.rows.size() == (size_t)BCH_CHUNKS * P * BCH_WORDS, "row table size");
    if (C.rows.size() != (size_t)BCH_CHUNKS * P * BCH_WORDS) return;
    size_t nseam = 0;
    for (int c = 0; c < BCH_CHUNKS; ++c) {
        const int begin = C.msg_bytes - (BCH_CHUNKS - c) * C.chunk_bytes;
        if (c > 0 && begin > 0) { CHECK(nseam < C.seams.size() && C.seams[nseam] == 8 * begin, "seam of chunk %d", c); ++nseam; }
        for (int i = 0; i < P; ++i) {
            const Poly r = row_of(C.rows, (size_t)c * P + i);
            CHECK(poly_degree(r) < P && poly_degree(r) >= 0, "row (%d, %d) not reduced", c, i);
            if (i > 0) CHECK(same(r, poly_times_x(row_of(C.rows, (size_t)c * P + i - 1), B.g_low, P)), "row (%d, %d) is not x times the one before", c, i);
            if (c == BCH_CHUNKS - 1) CHECK(poly_degree(r) == i && r.w[i >> 5] == 1u << (i & 31), "last chunk's row %d is not x^%d", i, i);
        }
        if (c + 1 < BCH_CHUNKS) {       // row (c, 0) = row (c + 1, 0) x^(8 chunk_bytes)
            Poly p = row_of(C.rows, (size_t)(c + 1) * P);
            for (int k = 0; k < 8 * C.chunk_bytes; ++k) p = poly_times_x(p, B.g_low, P);
            CHECK(same(p, row_of(C.rows, (size_t)c * P)), "chunk %d starts at the wrong power", c);
        }
    }
    CHECK(nseam == C.seams.size(), "seam count");
    // the kernel's arithmetic against the bit-serial LFSR on one random message
    std::vector<uint8_t> msg(C.msg_bytes);
    for (uint8_t& b : msg) b = (uint8_t)rnd();
    Poly serial;
    for (int j = 0; j < f.kbch; ++j) {
        const int fb = ((msg[j / 8] >> (7 - j % 8)) & 1) ^ poly_bit(serial, P - 1);
        Poly nx = serial;
        if (poly_bit(serial, P - 1)) nx.w[(P - 1) >> 5] ^= 1u << ((P - 1) & 31);
        for (int w = BCH_WORDS - 1; w > 0; --w) nx.w[w] = (nx.w[w] << 1) | (nx.w[w - 1] >> 31);
        nx.w[0] <<= 1;
        if (fb) for (int w = 0; w < BCH_WORDS; ++w) nx.w[w] ^= B.g_low.w[w];
        serial = nx;
    }
    Poly total;
    const int TW = (P - 8) / 32, TS = (P - 8) % 32, NW = (P + 31) / 32;
    for (int c = 0; c < BCH_CHUNKS; ++c) {
        const int begin = C.msg_bytes - (BCH_CHUNKS - c) * C.chunk_bytes;
        Poly r;
        for (int b = begin < 0 ? 0 : begin; b < begin + C.chunk_bytes; ++b) {
            const uint32_t top = ((r.w[TW] >> TS) & 0xffu) ^ msg[b];
            for (int w = NW - 1; w > 0; --w) r.w[w] = (r.w[w] << 8) | (r.w[w - 1] >> 24);
            r.w[0] <<= 8;
            if (P % 32) r.w[NW - 1] &= (1u << (P % 32)) - 1u;
            for (int w = 0; w < NW; ++w) r.w[w] ^= B.byte_tab[(size_t)top * BCH_WORDS + w];
        }
        for (int i = 0; i < P; ++i)
            if (poly_bit(r, i)) for (int w = 0; w < BCH_WORDS; ++w) total.w[w] ^= C.rows[((size_t)c * P + i) * BCH_WORDS + w];
    }
    CHECK(same(total, serial), "rate %d short %d: chunked parity differs from the serial LFSR", rate, shortframes);
}

static void check_ldpc(int rate, int shortframes, const FecParams& f) {
    const QcCodeDesc& d = QC_CODES[f.code_index];
    const LdpcEncodePlan L = build_ldpc_encode_plan(f.code_index);
    CHECK(L.N == f.N && L.K == f.K && L.blocks * 360 == f.K && L.q * 360 == f.N - f.K, "rate %d short %d: sizes", rate, shortframes);
    CHECK(L.blocks + L.q <= 180, "LDS rows: %d blocks + %d layers", L.blocks, L.q);
    CHECK((int)L.layer_off.size() == L.q + 1 && L.layer_off[0] == 0 && L.layer_off[L.q] == L.ent.size(), "layer offsets");
    CHECK(L.edges() == d.edges, "rate %d short %d: %d links against %d", rate, shortframes, L.edges(), d.edges);
    for (int i = 0; i < L.q; ++i) {
        CHECK(L.layer_off[i] < L.layer_off[i + 1] && L.layer_off[i + 1] - L.layer_off[i] <= (uint32_t)d.max_deg, "layer %d degree", i);
        for (uint32_t e = L.layer_off[i]; e < L.layer_off[i + 1]; ++e) {
            const int r = (int)(L.ent[e] >> 16), sp = (int)(L.ent[e] & 0xffffu);
            CHECK(r < L.blocks && sp < 360 && (sp + (int)(d.ent[e] & 0xffffu)) % 360 == 0, "layer %d link %u: r %d sp %d", i, e, r, sp);
        }
    }
}

// the kernel's reading of a rotated block: word w of (block rotated by s) from the 13-word extended block
static void check_funnel() {
    uint8_t bit[360];
    for (int m = 0; m < 360; ++m) bit[m] = (uint8_t)(rnd() & 1u);
    uint32_t ext[LDPC_EXT_WORDS] = {};
    for (int m = 0; m < 32 * LDPC_EXT_WORDS; ++m) if (bit[m % 360]) ext[m >> 5] |= 1u << (m & 31);
    for (int s = 0; s < 360; ++s) {
        const int sp = (360 - s) % 360;
        for (int w = 0; w < 12; ++w) {
            int start = 32 * w + sp;
            if (start >= 360) start -= 360;
            CHECK((start >> 5) + 1 < LDPC_EXT_WORDS, "rotation %d word %d reads past the extended block", s, w);
            const uint64_t two = (uint64_t)ext[start >> 5] | ((uint64_t)ext[(start >> 5) + 1] << 32);
            uint32_t got = (uint32_t)(two >> (start & 31));
            if (w == 11) got &= 0xffu;
            uint32_t want = 0;
            for (int b = 0; b < 32 && 32 * w + b < 360; ++b) if (bit[(32 * w + b - s + 360) % 360]) want |= 1u << b;
            CHECK(got == want, "rotation %d word %d", s, w);
        }
    }
}

int main() {
    int codes = 0;
    for (int shortframes = 0; shortframes < 2; ++shortframes)
        for (int rate = 0; rate < RATE_COUNT; ++rate) {
            FecParams f;
            if (!fec_params(rate, shortframes, &f)) continue;
            ++codes;
            CHECK(f.kbch % 8 == 0 && f.K % 8 == 0 && f.N % 8 == 0 && f.K % 360 == 0 && (f.N - f.K) % 8 == 0, "rate %d short %d: sizes in whole bytes", rate, shortframes);
            check_bch(rate, shortframes, f);
            check_ldpc(rate, shortframes, f);
            int32_t counts[PLAN_COUNTS];
            const BchChunkPlan cut = bch_chunk_cut(f.kbch);
            plan_counts(f, cut, build_ldpc_encode_plan(f.code_index), counts);
            CHECK(counts[0] == f.K - f.kbch && counts[9] == (int32_t)cut.seams.size() && counts[9] <= BCH_CHUNKS - 1, "plan counts");
        }
    CHECK(codes == 21, "%d codes", codes);
    CHECK(sizes_are_whole_bytes(), "sizes_are_whole_bytes");
    check_funnel();
    if (failures) fprintf(stderr, "%d checks failed\n", failures);
    return failures ? 1 : 0;
}
