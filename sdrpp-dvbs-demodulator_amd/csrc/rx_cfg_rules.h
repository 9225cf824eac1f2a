// What a receiver configuration may be, stated once: the admissibility rule of the DVB-S2 handle (demod_configure: create, set_params) and of the
// DVB-S bank (dvbs2gpu_dvbs_demod_create), the capacity the DVB-S symbol buffers are sized with, the RRC tap generator and the key of the context's
// tap cache (get_rrc).  Nothing else decides.  No HIP header: tests/cpp/rx_cfg_rules_host.cpp checks every bound from both sides on the host.
//
// WHERE THE BOUNDS COME FROM.  Both timing loops are the same recurrence (PhaseControlLoop::advance behind a clamped error e in [-1, 1]):
//     freq = clamp(freq + clock_omega_gain * e, omega (1 - lim), omega (1 + lim));   phase += freq + clock_mu_gain * e;
//     step = floor(phase);   offset += step;   phase -= step                         (phase in [0, 1) before every output)
// so an output moves the read position by a = freq + clock_mu_gain * e samples, whatever clock_omega_gain is (the clamp holds freq).
//
// DVB-S2 (gardner.cpp, omega = 1, two outputs per symbol; s2_gardner2_kernel / s2_gardner_cand_kernel).  Only the on-symbol output carries an error;
// its follower advances by freq alone.  With m = |clock_mu_gain|:
//     one output:        a in [1 - lim - m, 1 + lim + m]                       (a_min, a_max)
//     a symbol (2 out.): at least 2 (1 - lim) - m samples, i.e. per output     a_avg = 1 - lim - m / 2
//   * steps: floor(phase + a) lies in {0, 1, 2} for every phase in [0, 1) exactly when 0 <= a_min and a_max <= 2: both are m <= 1 - lim.  (A negative
//     step walks the reference's loop backwards out of its buffer.)
//   * scratch: the outputs of a call of n samples go to fe_out[0 .. n + n/16 + 128) (fe_scratch_offset; the staged gains sit behind them, and the symbol
//     FIFO holds half of that plus its leftover).  The K-th output is taken at a position < n + 1 that K - 1 outputs have advanced to, whole symbols by
//     2 a_avg each and at most one odd output by a_min >= a_avg - m/2: K < n / a_avg + 2.  That fits every n exactly when a_avg >= 16/17.
//   * lists: a period of form 2 starts at offset >= base - 3 and takes symbols while offset < base + 13 and fewer than G2_LIST - 2 = 22 outputs are
//     listed: the P-th symbol needs (P - 1) 2 a_avg < 17, so P <= 11 symbols wherever a_avg >= 17/22; form 4 (offset >= base - 2, < base + 14, a budget
//     of (GC_LIST - 4) / 2 = 10 symbols) wherever a_avg >= 17/20; the last period of a slice (single steps up to the slice's end, at most 24 list words)
//     wherever a_avg >= 20/22.  No period is cut short, so the resolver never falls behind its ring of 4 (form 4: 8) periods.
//   All of it follows from a_avg >= 16/17 (0.9412): the rule is  0 <= lim <= 0.05  and  1 - lim - m/2 >= S2_A_AVG_MIN.  The plugin's gains (m = 0.0176) pass
//   up to lim = 0.05 (0.94120); the widest m is 0.1176 at lim = 0.
//   (S2_A_AVG_MIN is 16/17 plus 1e-6: the loop's float roundings -- of freq's limits, of every phase += a -- move an output by < 2^-22 of its position.)
//
// DVB-S (complex_fd.cpp, omega = samplerate / symbolrate, one output per symbol, every output carries an error; dvbs_fd_kernel):
//     a in [omega (1 - lim) - m, omega (1 + lim) + m]
//   * a_min > 0: the loop never steps backwards (the kernel's window index offset - base would leave the staged tile); any forward step is fine.
//   * tile: a 256-sample tile stages at most FD_OCAP = 200 symbols: the K-th symbol of a tile needs (K - 1) a_min < 257, K <= 198 wherever a_min >= 1.3.
//   * buffers: a call of n samples yields fewer than n / a_min + 2 symbols: sym_cap (and soft_cap from it) come from dvbs_sym_cap(n, a_min).
//   The rule keeps what the header documented (65 taps, omega <= 64, 0 <= lim <= 0.25, omega (1 - lim) >= 1.5) and adds a_min >= DVBS_A_MIN = 1.3.
//
// RRC (make_rrc_taps: SDR++ taps::rootRaisedCosine): rrc_alpha in [0, 1] -- the roll-off of a root-raised cosine; 0 is the sinc -- and Ts =
// samplerate / symbolrate finite and positive; whatever else makes a tap non-finite (a subnormal Ts) is refused by looking at the taps.
#pragma once
#include <cmath>
#include <cstdint>
#include <cstring>
#include <tuple>
#include <vector>

namespace s2 {
namespace rxcfg {

// ---- the device-side layout the rule is derived from (s2_rx_kernels.hip asserts that these are its own numbers)
constexpr int RRC_TAPS_MAX = 129;
constexpr int S2_PERIOD = 16;                 // samples per stream and period of both timing-recovery forms (G2_TILE, GC_T)
constexpr int S2_LIST = S2_PERIOD + 8;        // list words per stream and period (G2_LIST, GC_LIST)
constexpr long long s2_fe_out_capacity(long long n) { return n + n / 16 + 128; }   // fe_scratch_offset: outputs of a call of n samples
constexpr int FD_TILE_SAMPLES = 256;          // FD_TILE
constexpr int FD_OCAP = FD_TILE_SAMPLES / 2 + 72;   // symbols dvbs_fd_kernel stages per tile

constexpr float S2_LIM_MAX = 0.05f;               // (a float, like the field: 0.05f itself is accepted)
constexpr double S2_A_AVG_MIN = 16.0 / 17.0 + 1e-6;
constexpr double DVBS_LIM_MAX = 0.25, DVBS_OMEGA_MAX = 64.0, DVBS_OMEGA_MIN_FREQ = 1.5, DVBS_A_MIN = 1.3;
constexpr int DVBS_RRC_TAPS = 65;
static_assert(S2_A_AVG_MIN > 17.0 / 20.0 && S2_A_AVG_MIN > 20.0 / 22.0, "the scratch bound implies the list bounds of both forms");
static_assert(1.0 + (FD_TILE_SAMPLES + 1) / DVBS_A_MIN <= FD_OCAP, "DVBS_A_MIN keeps a tile's symbols inside its stage");

// ---- RRC taps and their cache key
inline std::vector<float> make_rrc_taps(int count, double beta, double Ts) {   // SDR++ taps::rootRaisedCosine
    const double PI = 3.14159265358979323846, SQ2 = 1.41421356237309504880;
    double limit = Ts / (4.0 * beta), half = (double)count / 2.0;
    std::vector<float> taps(count);
    for (int i = 0; i < count; i++) {
        double t = (double)i - half + 0.5, v;
        if (t == 0.0) v = (1.0 + beta * (4.0 / PI - 1.0)) / Ts;
        else if (t == limit || t == -limit)
            v = ((1.0 + 2.0 / PI) * sin(PI / (4.0 * beta)) + (1.0 - 2.0 / PI) * cos(PI / (4.0 * beta))) * beta / (Ts * SQ2);
        else
            v = ((sin((1.0 - beta) * PI * t / Ts) + cos((1.0 + beta) * PI * t / Ts) * 4.0 * beta * t / Ts) /
                 ((1.0 - (4.0 * beta * t / Ts) * (4.0 * beta * t / Ts)) * PI * t / Ts)) / Ts;
        taps[i] = (float)v;
    }
    return taps;
}

// exactly the arguments make_rrc_taps is called with: two configurations share a table when they are the same numbers (-0.0 and 0.0 are not, and get the
// same taps twice: harmless)
typedef std::tuple<int, uint32_t, uint64_t> RrcKey;
inline RrcKey rrc_key(int ntaps, float alpha, double Ts) {
    uint32_t a;
    uint64_t t;
    memcpy(&a, &alpha, sizeof(a));
    memcpy(&t, &Ts, sizeof(t));
    return RrcKey(ntaps, a, t);
}

// nullptr, or which bound the filter breaks
inline const char* rrc_refusal(int ntaps, float alpha, double samplerate, double symbolrate) {
    if (ntaps < 1 || ntaps > RRC_TAPS_MAX) return "rrc_taps must be within [1, 129]";
    if (!(samplerate > 0) || !(symbolrate > 0) || !std::isfinite(samplerate) || !std::isfinite(symbolrate)) return "samplerate and symbolrate must be positive and finite";
    if (!(alpha >= 0.f) || !(alpha <= 1.f)) return "rrc_alpha must be within [0, 1]";
    const double Ts = samplerate / symbolrate;
    if (!(Ts > 0) || !std::isfinite(Ts)) return "samplerate / symbolrate must be positive and finite";
    for (float v : make_rrc_taps(ntaps, alpha, Ts))
        if (!std::isfinite(v)) return "samplerate / symbolrate and rrc_alpha yield a non-finite RRC tap";
    return nullptr;
}

// ---- DVB-S2 timing loop
inline double s2_a_min(float lim, float mu) { return 1.0 - (double)lim - std::fabs((double)mu); }
inline double s2_a_max(float lim, float mu) { return 1.0 + (double)lim + std::fabs((double)mu); }
inline double s2_a_avg(float lim, float mu) { return 1.0 - (double)lim - std::fabs((double)mu) / 2.0; }
// the largest |clock_mu_gain| the rule accepts at this omega_rel_limit (a double; the float below it is accepted)
inline double s2_mu_gain_max(float lim) { return 2.0 * (1.0 - (double)lim - S2_A_AVG_MIN); }

inline const char* s2_loop_refusal(float omega_rel_limit, float clock_mu_gain, float clock_omega_gain, float agc_rate, float loop_bw, float fll_bw) {
    if (!(omega_rel_limit >= 0.f) || !(omega_rel_limit <= S2_LIM_MAX)) return "omega_rel_limit must be within [0, 0.05]";
    // (the kernels evaluate PCL::advance(0) as "freq unchanged" -- exact for finite gains only)
    if (!std::isfinite(clock_mu_gain) || !std::isfinite(clock_omega_gain) || !std::isfinite(agc_rate) || !std::isfinite(loop_bw) || !std::isfinite(fll_bw))
        return "loop gains must be finite";
    if (!(s2_a_avg(omega_rel_limit, clock_mu_gain) >= S2_A_AVG_MIN))
        return "1 - omega_rel_limit - |clock_mu_gain| / 2 must be >= 16/17 + 1e-6: the timing recovery's output buffer holds n + n/16 + 128 outputs of n samples";
    return nullptr;
}
static_assert(2.0 * (1.0 - S2_A_AVG_MIN) <= 1.0 - (double)S2_LIM_MAX, "the scratch bound implies |clock_mu_gain| <= 1 - omega_rel_limit: every step is 0, 1 or 2 samples");

// ---- DVB-S timing loop
inline double dvbs_a_min(double omega, float lim, float mu) { return omega * (1.0 - (double)lim) - std::fabs((double)mu); }
inline double dvbs_a_max(double omega, float lim, float mu) { return omega * (1.0 + (double)lim) + std::fabs((double)mu); }
inline double dvbs_mu_gain_max(double omega, float lim) { return omega * (1.0 - (double)lim) - DVBS_A_MIN; }
// symbols a call of n samples can yield (< n / a_min + 2), with the slack the buffers always had
inline size_t dvbs_sym_cap(int n, double a_min) { return (size_t)((double)n / a_min) + 130; }

inline const char* dvbs_loop_refusal(double samplerate, double symbolrate, int rrc_taps, float omega_rel_limit, float clock_mu_gain, float clock_omega_gain,
                                     float agc_rate, float loop_bw, float fll_bw) {
    if (rrc_taps != DVBS_RRC_TAPS) return "the DVB-S front end is built for the reference's 65-tap filters (RRC_TAP_COUNT)";
    // (the FLL's band-edge filters take both rates as ints, fll.cpp:61-95)
    if (!(samplerate >= 1.0) || !(symbolrate >= 1.0) || !(samplerate < 2147483648.0) || !(symbolrate < 2147483648.0)) return "samplerate and symbolrate must be within [1, 2^31)";
    const double omega = samplerate / symbolrate;
    if (!(omega_rel_limit >= 0.f) || !((double)omega_rel_limit <= DVBS_LIM_MAX) || !(omega * (1.0 - (double)omega_rel_limit) >= DVBS_OMEGA_MIN_FREQ) || !(omega <= DVBS_OMEGA_MAX))
        return "samplerate/symbolrate * (1 - omega_rel_limit) must be >= 1.5 (and the ratio <= 64, omega_rel_limit in [0, 0.25])";
    if (!std::isfinite(clock_mu_gain) || !std::isfinite(clock_omega_gain) || !std::isfinite(agc_rate) || !std::isfinite(loop_bw) || !std::isfinite(fll_bw))
        return "loop gains must be finite";
    if (!(dvbs_a_min(omega, omega_rel_limit, clock_mu_gain) >= DVBS_A_MIN))
        return "samplerate/symbolrate * (1 - omega_rel_limit) - |clock_mu_gain| must be >= 1.3: a 256-sample tile of the timing recovery stages at most 200 symbols";
    return nullptr;
}

}  // namespace rxcfg
}  // namespace s2
