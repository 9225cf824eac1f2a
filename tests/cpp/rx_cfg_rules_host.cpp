// csrc/rx_cfg_rules.h on its own, no GPU: what a receiver configuration may be, and the key of the RRC tap cache.
//   * every bound of the DVB-S2 and DVB-S rules from both sides (the last accepted float / double and the first refused one), the plugin's configuration;
//   * what the bounds promise, on a model of the kernels' loops: the timing recurrence in float with the error held at the clamp that makes it emit most
//     (and freq at its lower limit), cut into the periods of both DVB-S2 forms and the tiles of the DVB-S kernel with their list, budget and stage bounds
//     -- at the edge of the rule no bound is ever reached, no step leaves {0, 1, 2} samples (DVB-S2), and a call's outputs fit the buffer;
//   * the cache key: equal exactly where make_rrc_taps returns the same floats, for the samples-per-symbol ratios and roll-offs the rounded key confused.
// Exit status 0: all checks passed; otherwise the failed checks are on stderr.
#include "rx_cfg_rules.h"

#include <cstdio>
#include <limits>

using namespace s2::rxcfg;

static int failures = 0;
#define CHECK(cond, ...)                                                          \
    do {                                                                          \
        if (!(cond)) { ++failures; fprintf(stderr, "FAILED %s: ", #cond); fprintf(stderr, __VA_ARGS__); fputc('\n', stderr); } \
    } while (0)

static const float NaN = std::numeric_limits<float>::quiet_NaN(), Inf = std::numeric_limits<float>::infinity();
static float up(float x) { return std::nextafter(x, Inf); }
static float down(float x) { return std::nextafter(x, -Inf); }
static float below(double x) { float f = (float)x; return (double)f <= x ? f : down(f); }   // the largest float <= x
static float above(double x) { float f = (float)x; return (double)f > x ? f : up(f); }      // the smallest float > x

// main.cpp:64-73 of the plugin: CLOCK_RECOVERY_BW 0.00628, DAMPN_F 0.707, REL_LIM 0.02, 65 taps, roll-off 0.35, AGC 1e-4, Costas 0.00628, FLL 0.006
struct Plugin {
    float mu, omega_gain, lim = 0.02f, agc = 0.0001f, loop_bw = 0.00628f, fll_bw = 0.006f, alpha = 0.35f;
    int taps = 65;
    Plugin() {
        float bw = 0.00628f, damp = 0.707f;
        float den = (1.0f + 2.0 * damp * bw + bw * bw);
        mu = (4.0f * damp * bw) / den;
        omega_gain = (4.0f * bw * bw) / den;
    }
};
static const Plugin P;

static bool s2_ok(float lim, float mu, float og = P.omega_gain, float agc = P.agc, float lbw = P.loop_bw, float fbw = P.fll_bw) {
    return s2_loop_refusal(lim, mu, og, agc, lbw, fbw) == nullptr;
}
static bool dvbs_ok(double fs, double sr, float lim, float mu, int taps = 65, float og = P.omega_gain, float agc = P.agc, float lbw = P.loop_bw, float fbw = P.fll_bw) {
    return dvbs_loop_refusal(fs, sr, taps, lim, mu, og, agc, lbw, fbw) == nullptr;
}
static bool rrc_ok(int taps, float alpha, double fs, double sr) { return rrc_refusal(taps, alpha, fs, sr) == nullptr; }

// ---- the recurrence (PhaseControlLoop::advance behind the clamped error), in float like the kernels and the reference
struct Loop {
    float alpha, beta, phase, freq, minf, maxf;
    int offset = 0;
    int step(float e) {
        freq += beta * e;
        freq = freq > maxf ? maxf : (freq < minf ? minf : freq);
        phase += freq + alpha * e;
        const float d = floorf(phase);
        offset = (int)((float)offset + d);
        phase -= d;
        return (int)d;
    }
};

// a call of n samples through the DVB-S2 loop with every on-symbol error at `e`, period by period as form 2 (form4 = false) or form 4 walks it
static void s2_model(float lim, float mu, float e, int n, bool form4, const char* what) {
    Loop L{mu, P.omega_gain, 0.f, (float)(1.0 * (1.0 - lim)), (float)(1.0 * (1.0 - lim)), (float)(1.0 * (1.0 + lim))};
    int sps = 0;
    long long out = 0;
    int bad_step = 0, cut = 0, late = 0;
    auto one = [&](float err) { const int d = L.step(err); if (d < 0 || d > 2) ++bad_step; ++out; };
    const int back = form4 ? 2 : 3;
    for (int base = 0; base < n; base += S2_PERIOD) {
        const int lim_t = base + S2_PERIOD < n ? base + S2_PERIOD : n;
        int cnt = 0;
        if (L.offset < base - back) ++late;                                    // (the period before ended at offset >= its lim - back)
        if (sps == 1 && L.offset < lim_t) { one(0.f); ++cnt; sps = 0; }
        int symbols = 0;
        while (sps == 0 && L.offset < lim_t - back) {
            if (form4 ? symbols >= (S2_LIST - 4) / 2 : cnt >= S2_LIST - 2) { ++cut; break; }
            one(e); one(0.f); cnt += 2; ++symbols;
        }
        if (base + S2_PERIOD >= n) {
            int guard = 0;
            while (L.offset < n) {
                if (cnt >= S2_LIST || (form4 && guard >= 8)) { ++cut; break; }
                one(sps == 0 ? e : 0.f); sps ^= 1; ++cnt; ++guard;
            }
        }
    }
    CHECK(bad_step == 0, "%s: %d steps outside {0, 1, 2}", what, bad_step);
    CHECK(cut == 0 && late == 0, "%s: %d periods cut short by their list, %d started late", what, cut, late);
    CHECK(out <= s2_fe_out_capacity(n), "%s: %lld outputs of %d samples, capacity %lld", what, out, n, s2_fe_out_capacity(n));
    CHECK((double)out < (double)n / s2_a_avg(lim, mu) * (1.0 + 1e-6) + 2.0, "%s: %lld outputs exceed n / a_avg + 2", what, out);
}

// a call of n samples through the DVB-S loop with every error at `e`, tile by tile as dvbs_fd_kernel walks it
static void dvbs_model(double omega, float lim, float mu, float e, int n, const char* what) {
    Loop L{mu, P.omega_gain, 0.f, (float)(omega * (1.0 - lim)), (float)(omega * (1.0 - lim)), (float)(omega * (1.0 + lim))};
    long long out = 0;
    int full = 0, backwards = 0;
    for (int base = 0; base < n; base += FD_TILE_SAMPLES) {
        const int m = n - base < FD_TILE_SAMPLES ? n - base : FD_TILE_SAMPLES;
        int nout = 0;
        if (L.offset < base) ++backwards;
        while (L.offset < base + m) {
            if (nout >= FD_OCAP) { ++full; break; }
            if (L.step(e) < 0) ++backwards;
            ++nout;
        }
        out += nout;
    }
    CHECK(full == 0 && backwards == 0, "%s: %d tiles filled their stage, %d steps backwards", what, full, backwards);
    const size_t cap = dvbs_sym_cap(n, dvbs_a_min(omega, lim, mu));
    CHECK((size_t)out <= cap - 128, "%s: %lld symbols of %d samples, sym_cap %zu", what, out, n, cap);
}

static void test_s2_rule() {
    CHECK(s2_ok(P.lim, P.mu), "the plugin's configuration");
    CHECK(rrc_ok(P.taps, P.alpha, 55e6, 27.5e6), "the plugin's filter");
    // omega_rel_limit
    CHECK(s2_ok(0.f, P.mu) && !s2_ok(-1e-9f, P.mu) && !s2_ok(NaN, P.mu), "omega_rel_limit at 0");
    CHECK(s2_ok(0.05f, P.mu), "omega_rel_limit 0.05 with the plugin's gains (a_avg %.7f)", s2_a_avg(0.05f, P.mu));
    CHECK(!s2_ok(up(0.05f), 0.f) && !s2_ok(0.06f, 0.f) && !s2_ok(Inf, 0.f), "omega_rel_limit beyond 0.05");
    // clock_mu_gain: the last accepted and the first refused float, both signs, at three limits
    for (float lim : {0.f, 0.02f, 0.05f}) {
        const double m = s2_mu_gain_max(lim);
        CHECK(m > 0 && s2_ok(lim, below(m)) && s2_ok(lim, -below(m)), "clock_mu_gain +-%.9g at omega_rel_limit %g", m, lim);
        CHECK(!s2_ok(lim, above(m)) && !s2_ok(lim, -above(m)), "clock_mu_gain beyond +-%.9g at omega_rel_limit %g", m, lim);
        CHECK(s2_a_min(lim, below(m)) >= 0 && s2_a_max(lim, below(m)) <= 2, "a_min, a_max at the edge");
    }
    CHECK(!s2_ok(0.02f, 1.0f) && !s2_ok(0.02f, -1.0f) && !s2_ok(0.f, 2.0f), "gains that step backwards or by three samples");
    // the issue's reading: a_min = 1 - lim - |mu| = 0.932 at lim 0.05 is below 16/17, yet the outputs fit: a symbol has ONE output with an error
    CHECK(s2_a_min(0.05f, P.mu) < 16.0 / 17.0 && s2_a_avg(0.05f, P.mu) > 16.0 / 17.0, "per-output and per-symbol bounds at 0.05");
    // finite gains
    for (float bad : {NaN, Inf, -Inf}) {
        CHECK(!s2_ok(P.lim, bad) && !s2_ok(P.lim, P.mu, bad) && !s2_ok(P.lim, P.mu, P.omega_gain, bad) && !s2_ok(P.lim, P.mu, P.omega_gain, P.agc, bad) &&
              !s2_ok(P.lim, P.mu, P.omega_gain, P.agc, P.loop_bw, bad), "a non-finite gain");
    }
    CHECK(s2_ok(P.lim, P.mu, 1e30f, -5.f, 100.f, -3.f), "any finite clock_omega_gain, agc_rate, loop_bw, fll_bw");
    // what the rule promises, at its edge and at the plugin's point, in both forms, for whole and ragged calls
    for (float lim : {0.f, 0.02f, 0.05f}) {
        const float m = below(s2_mu_gain_max(lim));
        for (int n : {1, 15, 16, 17, 50, 4099, 30011, 1000003})
            for (int form4 = 0; form4 < 2; ++form4) {
                s2_model(lim, m, -1.f, n, form4, "edge, +mu, error -1");
                s2_model(lim, -m, 1.f, n, form4, "edge, -mu, error +1");
                s2_model(lim, m, 1.f, n, form4, "edge, +mu, error +1");
                s2_model(lim, P.mu, -1.f, n, form4, "plugin's gains, error -1");
            }
    }
}

static void test_dvbs_rule() {
    CHECK(dvbs_ok(4e6, 2e6, P.lim, P.mu) && rrc_ok(65, P.alpha, 4e6, 2e6), "the plugin's configuration");
    CHECK(!dvbs_ok(4e6, 2e6, P.lim, P.mu, 64) && !dvbs_ok(4e6, 2e6, P.lim, P.mu, 66) && !dvbs_ok(4e6, 2e6, P.lim, P.mu, 1), "tap counts other than 65");
    // samples per symbol and omega_rel_limit
    CHECK(dvbs_ok(3e6, 2e6, 0.f, P.mu) && !dvbs_ok(3e6 - 1, 2e6, 0.f, P.mu), "1.5 samples per symbol");
    CHECK(dvbs_ok(3.2e6, 2e6, 0.02f, P.mu) && !dvbs_ok(3.2e6, 2e6, 0.07f, P.mu), "1.6 samples per symbol: omega (1 - lim) >= 1.5");
    CHECK(dvbs_ok(128e6, 2e6, P.lim, P.mu) && !dvbs_ok(128e6 + 64, 2e6, P.lim, P.mu), "64 samples per symbol");
    CHECK(dvbs_ok(4e6, 2e6, 0.25f, P.mu) && !dvbs_ok(4e6, 2e6, up(0.25f), P.mu) && dvbs_ok(4e6, 2e6, 0.f, P.mu) && !dvbs_ok(4e6, 2e6, -1e-9f, P.mu) &&
          !dvbs_ok(4e6, 2e6, NaN, P.mu), "omega_rel_limit within [0, 0.25]");
    // the rates as ints (band-edge filters)
    CHECK(dvbs_ok(2.0, 1.0, P.lim, P.mu) && !dvbs_ok(1.0, 0.5, P.lim, P.mu) && !dvbs_ok(0.0, 1.0, P.lim, P.mu) && !dvbs_ok(4e6, 0.0, P.lim, P.mu) &&
          !dvbs_ok(-4e6, -2e6, P.lim, P.mu), "rates below 1");
    CHECK(dvbs_ok(2147483647.0, 1073741823.5, 0.f, P.mu) && !dvbs_ok(2147483648.0, 1073741824.0, 0.f, P.mu) && !dvbs_ok((double)Inf, 2e6, 0.f, P.mu) &&
          !dvbs_ok((double)NaN, 2e6, 0.f, P.mu) && !dvbs_ok(4e6, (double)NaN, 0.f, P.mu), "rates of 2^31 and beyond");
    // clock_mu_gain
    const struct { double fs, sr; float lim; } at[] = {{3e6, 2e6, 0.f}, {4e6, 2e6, 0.02f}, {4e6, 2e6, 0.25f}, {16e6, 2e6, 0.25f}, {128e6, 2e6, 0.02f}};
    for (auto& c : at) {
        const double omega = c.fs / c.sr, m = dvbs_mu_gain_max(omega, c.lim);
        CHECK(m > 0 && dvbs_ok(c.fs, c.sr, c.lim, below(m)) && dvbs_ok(c.fs, c.sr, c.lim, -below(m)), "clock_mu_gain +-%.9g at %g sps, limit %g", m, omega, c.lim);
        CHECK(!dvbs_ok(c.fs, c.sr, c.lim, above(m)) && !dvbs_ok(c.fs, c.sr, c.lim, -above(m)), "clock_mu_gain beyond +-%.9g at %g sps, limit %g", m, omega, c.lim);
        CHECK(dvbs_a_max(omega, c.lim, below(m)) <= 2 * omega, "a_max at the edge");
        for (int n : {1, 255, 256, 257, 30011, 1000003}) {
            dvbs_model(omega, c.lim, below(m), -1.f, n, "edge, +mu, error -1");
            dvbs_model(omega, c.lim, -below(m), 1.f, n, "edge, -mu, error +1");
            dvbs_model(omega, c.lim, P.mu, -1.f, n, "plugin's gains, error -1");
            dvbs_model(omega, c.lim, below(m), 1.f, n, "edge, +mu, error +1");
        }
    }
    for (float bad : {NaN, Inf, -Inf}) {
        CHECK(!dvbs_ok(4e6, 2e6, P.lim, bad) && !dvbs_ok(4e6, 2e6, P.lim, P.mu, 65, bad) && !dvbs_ok(4e6, 2e6, P.lim, P.mu, 65, P.omega_gain, bad) &&
              !dvbs_ok(4e6, 2e6, P.lim, P.mu, 65, P.omega_gain, P.agc, bad) && !dvbs_ok(4e6, 2e6, P.lim, P.mu, 65, P.omega_gain, P.agc, P.loop_bw, bad), "a non-finite gain");
    }
    // the capacity the buffers had for the plugin's point is not undercut
    CHECK(dvbs_sym_cap(16384, dvbs_a_min(2.0, P.lim, P.mu)) >= (size_t)(16384 / (2.0 * 0.98)) + 130, "sym_cap at the plugin's point");
}

static void test_rrc_rule() {
    CHECK(rrc_ok(1, 0.35f, 2, 1) && rrc_ok(129, 0.35f, 2, 1) && !rrc_ok(0, 0.35f, 2, 1) && !rrc_ok(130, 0.35f, 2, 1) && !rrc_ok(-5, 0.35f, 2, 1), "rrc_taps within [1, 129]");
    CHECK(rrc_ok(65, 0.f, 2, 1) && rrc_ok(65, 1.f, 2, 1) && !rrc_ok(65, -1e-9f, 2, 1) && !rrc_ok(65, up(1.f), 2, 1) && !rrc_ok(65, NaN, 2, 1) && !rrc_ok(65, Inf, 2, 1),
          "rrc_alpha within [0, 1]");
    CHECK(!rrc_ok(65, 0.35f, 0, 1) && !rrc_ok(65, 0.35f, 2, 0) && !rrc_ok(65, 0.35f, -2, -1) && !rrc_ok(65, 0.35f, (double)Inf, 1) && !rrc_ok(65, 0.35f, 2, (double)Inf) &&
          !rrc_ok(65, 0.35f, (double)NaN, 1) && !rrc_ok(65, 0.35f, 2, (double)NaN), "rates positive and finite");
    CHECK(!rrc_ok(65, 0.35f, 1e-300, 1e300) && !rrc_ok(65, 0.35f, 1e300, 1e-300), "a ratio that is 0 or infinite");
    CHECK(!rrc_ok(65, 0.35f, 1e-310, 1.0), "a subnormal ratio: non-finite taps");
    // every accepted filter of the catalogue's kind has finite taps, the singular points t = +-Ts / (4 alpha) included (alpha 0.25 at Ts 2, 4)
    for (int taps : {1, 2, 33, 64, 65, 128, 129})
        for (float a : {0.f, 0.05f, 0.2f, 0.25f, 0.35f, 0.5f, 1.f})
            for (double Ts : {1.5, 1.6, 2.0, 2.4, 2.5, 3.0, 4.0, 8.0, 12.0, 64.0}) {
                CHECK(rrc_ok(taps, a, Ts, 1.0), "%d taps, roll-off %g, %g samples per symbol", taps, a, Ts);
                for (float v : make_rrc_taps(taps, a, Ts)) CHECK(std::isfinite(v) && std::fabs(v) < 4.0f, "tap %g (%d taps, roll-off %g, Ts %g)", v, taps, a, Ts);
            }
}

static bool same_taps(int n, float a1, double t1, float a2, double t2) {
    const std::vector<float> x = make_rrc_taps(n, a1, t1), y = make_rrc_taps(n, a2, t2);
    return memcmp(x.data(), y.data(), sizeof(float) * n) == 0;
}

static void test_key() {
    const double Ts[] = {2.0, 2.4, 1.6, 12.0, 2.5, 55e6 / 27.5e6, 3.2e6 / 2e6};
    const float al[] = {0.35f, 0.3504f, 0.2f, 0.25f};
    const int nt[] = {65, 64, 129};
    for (int n1 : nt) for (float a1 : al) for (double t1 : Ts)
        for (int n2 : nt) for (float a2 : al) for (double t2 : Ts) {
            const bool same_args = n1 == n2 && a1 == a2 && t1 == t2;
            CHECK((rrc_key(n1, a1, t1) == rrc_key(n2, a2, t2)) == same_args, "key of (%d, %g, %g) against (%d, %g, %g)", n1, a1, t1, n2, a2, t2);
            if (n1 == n2) CHECK(same_taps(n1, a1, t1, a2, t2) == same_args, "taps of (%d, %g, %g) against (%g, %g)", n1, a1, t1, a2, t2);
        }
    // the pairs the issue names
    CHECK(rrc_key(65, 0.35f, 2.0) != rrc_key(65, 0.35f, 2.4) && rrc_key(65, 0.35f, 2.0) != rrc_key(65, 0.35f, 1.6) && rrc_key(65, 0.35f, 2.4) != rrc_key(65, 0.35f, 1.6) &&
          rrc_key(65, 0.35f, 2.0) != rrc_key(65, 0.35f, 12.0), "samples per symbol 2.0 / 2.4 / 1.6 / 12.0");
    CHECK(rrc_key(65, 0.35f, 2.0) != rrc_key(65, 0.3504f, 2.0), "roll-off 0.35 / 0.3504");
    CHECK(rrc_key(65, 0.35f, 55e6 / 27.5e6) == rrc_key(65, 0.35f, 4e6 / 2e6), "the same ratio from other rates is the same filter");
    // an ordered key: usable in std::map
    CHECK(rrc_key(65, 0.35f, 2.0) < rrc_key(65, 0.35f, 2.4) || rrc_key(65, 0.35f, 2.4) < rrc_key(65, 0.35f, 2.0), "keys are ordered");
}

int main() {
    test_s2_rule();
    test_dvbs_rule();
    test_rrc_rule();
    test_key();
    if (failures) { fprintf(stderr, "%d checks failed\n", failures); return 1; }
    printf("rx_cfg_rules: all checks passed\n");
    return 0;
}
