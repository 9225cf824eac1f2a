// csrc/s2_tx_rules.h on its own, no GPU: the modulator's rules over every PLS code.  Built with -fsanitize=address,undefined by tests/test_host_cpp_s2_tx_rules.py.
//   PLS codes   108 of the 128 name a frame; the others (MODCODs 29..31, short 9/10) and codes outside 0..127 are refused; sizes against s2::modcod_params and
//               the list's prefix sums against the sum.
//   framing     host_frame -- the kernel's group reader, byte-crossing columns and all -- against a bit-by-bit restatement that de-interleaves with the
//               receiver's rule (out[col[c] + j] = in[bits j + c]) and walks slots and pilot blocks the way the standard lists them (the constellation table
//               and the PL tables are the header's own in both: what this program checks is the indexing; tests/test_s2_tx_cpu.py ties the values to the oracle
//               transmitter); every symbol of the frame
//               written exactly once, nothing outside it (guard symbols either side); code words in exactly sized heap blocks, so a read past the end is seen.
//   pulse       taps are the two polyphase branches of rrc; host_shape's block ends: zero outside against wrap-around, a block shorter than the span.
//   channel     esn0 >= 100 with no offsets is the identity; the generator's uniforms stay inside (0, 1] and [0, 1): finite samples for 2^16 indices; samples of two
//               streams and of two seeds differ.
// Exit status 0: all checks passed; otherwise the failed checks are on stderr.
#include "s2_tx_rules.h"

#include <cstdio>
#include <cstdlib>
#include <memory>
#include <vector>

using namespace s2;
using namespace s2::s2tx;

static int failures = 0;
#define CHECK(cond, ...)                                                          \
    do {                                                                          \
        if (!(cond)) { ++failures; fprintf(stderr, "FAILED %s: ", #cond); fprintf(stderr, __VA_ARGS__); fputc('\n', stderr); } \
    } while (0)

static uint32_t rnd_state = 2468u;
static uint32_t rnd() { rnd_state = rnd_state * 1664525u + 1013904223u; return rnd_state >> 8; }
static bool same(cf32 a, cf32 b) { return memcmp(&a, &b, sizeof(cf32)) == 0; }

static void check_frame(int pls, const HostTables& T) {
    FrameRule R;
    if (!frame_rule(pls, &R)) { CHECK(false, "pls %d refused", pls); return; }
    ModcodParams mp{};
    const bool dummy = (pls >> 2) == 0;
    if (!dummy) {
        CHECK(modcod_params(pls >> 2, (pls >> 1) & 1, pls & 1, &mp), "pls %d", pls);
        CHECK(R.symbols == mp.plframe && R.bb_bytes == mp.fec.kbch / 8 && R.code_bytes == mp.fec.N / 8 && R.payload * mp.bits == mp.fec.N && R.code_bytes <= MAX_CODE_BYTES,
              "pls %d: sizes", pls);
    } else {
        CHECK(R.symbols == 3330 && R.bb_bytes == 0 && R.code_bytes == 0 && R.payload == 3240, "dummy frame sizes");
    }
    CHECK(R.symbols % 2 == 0, "pls %d: an odd PLFRAME would misalign the 16-byte stores", pls);
    // a code word in a block of exactly its size
    std::unique_ptr<uint8_t[]> code(new uint8_t[R.code_bytes ? R.code_bytes : 1]);
    for (int b = 0; b < R.code_bytes; ++b) code[b] = (uint8_t)rnd();
    cf32 tab[32] = {};
    if (!dummy) tx_constellation(R.constel, R.g1, R.g2, tab);
    const int GUARD = 8;
    const cf32 mark{12345.f, -54321.f};
    std::vector<cf32> out((size_t)R.symbols + 2 * GUARD, mark);
    host_frame(R, T, tab, code.get(), out.data() + GUARD);
    for (int g = 0; g < GUARD; ++g) CHECK(same(out[g], mark) && same(out[GUARD + R.symbols + g], mark), "pls %d: a symbol written outside the frame", pls);
    // bit by bit
    std::vector<cf32> want((size_t)R.symbols, mark);
    for (int i = 0; i < 26; ++i) want[i] = T.sof[i];
    for (int i = 0; i < 64; ++i) want[26 + i] = T.plsc[(size_t)pls * 64 + i];
    const cf32 pilot{PILOT_IQ, PILOT_IQ};
    int pos = HEADER, scr = 0;
    if (dummy) {
        for (int k = 0; k < 36 * 90; ++k) want[pos++] = pl_rotate(pilot, T.rn[scr++]);
    } else {
        std::vector<uint8_t> inter((size_t)mp.fec.N);           // the receiver's de-interleaver, inverted
        const int rows = mp.fec.N / mp.bits;
        for (int j = 0; j < rows; ++j)
            for (int c = 0; c < mp.bits; ++c) {
                int src;
                if (mp.constel == C_QPSK) src = 2 * j + (1 - c);
                else if (mp.constel == C_8PSK && mp.rate == R3_5) src = rows * (2 - c) + j;
                else src = rows * c + j;
                CHECK(src == code_bit_of(R.qpsk, R.col, j, c), "pls %d: code_bit_of(%d, %d)", pls, j, c);
                inter[(size_t)mp.bits * j + c] = (uint8_t)((code[src >> 3] >> (7 - (src & 7))) & 1);
            }
        int sidx = 0;
        for (int slot = 0; slot < mp.slots; ++slot) {
            for (int k = 0; k < 90; ++k, ++sidx) {
                int v = 0;
                for (int b = 0; b < mp.bits; ++b) v = v << 1 | (inter[(size_t)sidx * mp.bits + b] ^ 1);
                want[pos++] = pl_rotate(tab[v], T.rn[scr++]);
            }
            if (mp.pilots && (slot + 1) % 16 == 0 && slot + 1 < mp.slots)
                for (int k = 0; k < 36; ++k) want[pos++] = pl_rotate(pilot, T.rn[scr++]);
        }
    }
    CHECK(pos == R.symbols, "pls %d: %d symbols walked, %d in the rule", pls, pos, R.symbols);
    int bad = 0;
    for (int i = 0; i < R.symbols; ++i) bad += !same(want[i], out[GUARD + i]);
    CHECK(bad == 0, "pls %d: %d symbols differ from the bit-by-bit frame", pls, bad);
    if (!dummy) {       // unit mean power
        double pw = 0;
        for (int v = 0; v < (1 << mp.bits); ++v) pw += (double)tab[v].re * tab[v].re + (double)tab[v].im * tab[v].im;
        CHECK(std::fabs(pw / (1 << mp.bits) - 1.0) < 1e-6, "pls %d: mean power %f", pls, pw / (1 << mp.bits));
        for (int v = 1 << mp.bits; v < 32; ++v) CHECK(tab[v].re == 0.f && tab[v].im == 0.f, "table entries behind the constellation");
    }
}

static void check_sizes() {
    std::vector<int32_t> list;
    for (int pls = -2; pls < 130; ++pls) {
        FrameRule R;
        ModcodParams mp;
        const bool valid = pls >= 0 && pls < 128 && ((pls >> 2) == 0 || modcod_params(pls >> 2, (pls >> 1) & 1, pls & 1, &mp));
        CHECK(frame_rule(pls, &R) == valid, "pls %d", pls);
        if (valid) list.push_back(pls);
    }
    CHECK(list.size() == 108, "%zu valid PLS codes", list.size());
    ListSizes total;
    std::vector<long long> so, bo, co;
    CHECK(list_sizes(list.data(), (int)list.size(), &total, nullptr, &so, &bo, &co), "the list of all valid codes");
    CHECK(so.size() == list.size() + 1 && so.back() == total.symbols && bo.back() == total.bb_bytes && co.back() == total.code_bytes && so[0] == 0, "prefix sums");
    long long s = 0;
    for (size_t f = 0; f < list.size(); ++f) {
        FrameRule R;
        frame_rule(list[f], &R);
        CHECK(so[f] == s, "frame %zu begins at %lld", f, so[f]);
        s += R.symbols;
    }
    int bad = -1;
    list[5] = 29 << 2;
    CHECK(!list_sizes(list.data(), (int)list.size(), &total, &bad) && bad == 5, "a reserved MODCOD in a list");
    CHECK(list_sizes(nullptr, 0, &total) && total.symbols == 0, "the empty list");
}

static void check_pulse() {
    const double rolls[3] = {0.35, 0.25, 0.20};
    for (double beta : rolls) {
        CHECK(rolloff_ok(beta), "roll-off %f", beta);
        for (double timing : {0.0, 0.3, -0.7}) {
            const Taps H = make_taps(beta, timing);
            double energy = 0;
            for (int p = 0; p < 2; ++p)
                for (int k = -SPAN; k <= SPAN; ++k) {
                    CHECK(H.h[p][k + SPAN] == (float)rrc((p - timing) / 2.0 - k, beta), "tap (%d, %d)", p, k);
                    energy += (double)H.h[p][k + SPAN] * H.h[p][k + SPAN];
                }
            CHECK(std::fabs(energy / 2.0 - 1.0) < 2e-3, "roll-off %.2f timing %.1f: pulse energy %f per symbol", beta, timing, energy / 2.0);
        }
        CHECK(std::isfinite(rrc(1.0 / (4.0 * beta), beta)) && std::isfinite(rrc(-1.0 / (4.0 * beta), beta)) && rrc(0.0, beta) > 1.0, "the pulse's removable singularities");
    }
    CHECK(!rolloff_ok(0.3) && !rolloff_ok(0.0) && !rolloff_ok(0.35f), "roll-offs outside the three");
    // a lone symbol reads the taps back, backwards in k; block ends; a block shorter than the span
    const Taps H = make_taps(0.35, 0.3);
    for (long long ns : {1LL, 20LL, 33LL, 300LL}) {
        std::unique_ptr<cf32[]> sym(new cf32[ns]), a(new cf32[2 * ns]), b(new cf32[2 * ns]);
        for (long long i = 0; i < ns; ++i) sym[i] = cf32{(float)(rnd() % 200) / 100.f - 1.f, (float)(rnd() % 200) / 100.f - 1.f};
        host_shape(sym.get(), ns, H, 0, a.get());
        host_shape(sym.get(), ns, H, 1, b.get());
        for (long long m = 0; m < ns; ++m)
            for (int p = 0; p < 2; ++p) {
                float re0 = 0.f, re1 = 0.f, im0 = 0.f, im1 = 0.f;
                for (int k = -SPAN; k <= SPAN; ++k) {
                    const long long i = m + k, w = ((i % ns) + ns) % ns;
                    const bool in = i >= 0 && i < ns;
                    re0 = fmaf(H.h[p][k + SPAN], in ? sym[i].re : 0.f, re0);
                    im0 = fmaf(H.h[p][k + SPAN], in ? sym[i].im : 0.f, im0);
                    re1 = fmaf(H.h[p][k + SPAN], sym[w].re, re1);
                    im1 = fmaf(H.h[p][k + SPAN], sym[w].im, im1);
                }
                CHECK(a[2 * m + p].re == re0 && a[2 * m + p].im == im0 && b[2 * m + p].re == re1 && b[2 * m + p].im == im1, "block of %lld: sample %lld", ns, 2 * m + p);
            }
    }
}

static void check_channel() {
    const ChanParams I = chan_params(200.0, 0.0, 0.0, 5, 0);
    CHECK(I.sigma == 0.f && I.rotate == 0, "no channel");
    const cf32 x{0.25f, -0.0f};
    CHECK(same(chan_sample(I, 12345, x), x), "the identity keeps a -0.0");
    const ChanParams A = chan_params(0.0, 1e-3, 0.5, 5, 0), B = chan_params(0.0, 1e-3, 0.5, 5, 1), C = chan_params(0.0, 1e-3, 0.5, 6, 0);
    CHECK(A.sigma == 1.0f && A.key != B.key && A.key != C.key && B.key != C.key, "keys of (seed, stream)");
    int differ = 0;
    for (long long n = 0; n < (1 << 16); ++n) {
        const cf32 a = chan_sample(A, n, x), b = chan_sample(B, n, x);
        CHECK(std::isfinite(a.re) && std::isfinite(a.im) && std::fabs(a.re) < 8.f && std::fabs(a.im) < 8.f, "sample %lld", n);
        differ += !same(a, b);
        CHECK(same(a, chan_sample(A, n, x)), "sample %lld is not a function of its index", n);
    }
    CHECK(differ > 65000, "streams 0 and 1 share %d of 65536 samples", 65536 - differ);
    // far out: the phase is reduced in double
    const ChanParams F = chan_params(200.0, 0.5, 0.0, 0, 0);
    const cf32 far = chan_sample(F, 1LL << 31, cf32{1.f, 0.f});
    const double ph = std::fmod(0.5 * (double)(1LL << 31), 6.283185307179586476925);
    CHECK(std::fabs(far.re - std::cos(ph)) < 1e-6 && std::fabs(far.im - std::sin(ph)) < 1e-6, "rotation at sample 2^31");
}

int main() {
    const HostTables T;
    CHECK(T.sof.size() == 26 && T.plsc.size() == 128 * 64 && T.rn.size() == 131072, "PL tables");
    check_sizes();
    for (int pls = 0; pls < 128; ++pls) {
        FrameRule R;
        if (frame_rule(pls, &R)) check_frame(pls, T);
    }
    check_pulse();
    check_channel();
    if (failures) fprintf(stderr, "%d checks failed\n", failures);
    return failures ? 1 : 0;
}
