/*
 * dvbs2gpu_host.hpp -- C++ host side above the C ABI (include/dvbs2gpu.h): the operator interface of the reference's hot path,
 * with the reference's names, argument meaning and error behaviour, for hosts that are C++ like the SDR++ plugin.
 *
 *   dvbs2gpu_host::dvbs2::DVBS2Demod       <->  dsp::dvbs2::DVBS2Demod        src/demod/dvbs2/module_dvbs2_demod.h:49-88
 *   dvbs2gpu_host::dvbs2::BBFrameTSParser  <->  dsp::dvbs2::BBFrameTSParser   src/demod/dvbs2/bbframe_ts_parser.h:68-80
 *   dvbs2gpu_host::dvbs::DVBSDemod         <->  dsp::dvbs::DVBSDemod          src/demod/dvbs/module_dvbs_demod.h:17-52
 *
 * What is NOT mirrored is SDR++'s block plumbing (Processor<>, stream<>, run(), tempStop/tempStart): those headers are not part of
 * the reference repository; INTEGRATION.md shows the same classes derived from Processor<> inside the plugin.  `process` has the
 * reference's signature and return value; the stream pointer argument of init() is dropped, everything else keeps its position.
 * Errors: the reference throws std::runtime_error for a bad MODCOD (modcod_to_cfg.cpp:11,135); every failing C-ABI call throws
 * std::runtime_error with dvbs2gpu_last_error() here.  There is no CPU fallback: without a gfx950 device init() throws.
 * Header-only; link with -ldvbs2gpu.
 */
#ifndef DVBS2GPU_HOST_HPP
#define DVBS2GPU_HOST_HPP

#include <dvbs2gpu.h>

#include <algorithm>
#include <cmath>
#include <memory>
#include <mutex>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

namespace dvbs2gpu_host {

struct complex_t {   // layout of SDR++'s dsp::complex_t: two floats
    float re, im;
};

constexpr int STREAM_BUFFER_SIZE = 1000000;   // SDR++ core: the largest count a process() call is handed

inline void check(int rc) {
    if (rc < 0) throw std::runtime_error(std::string("dvbs2gpu: ") + dvbs2gpu_last_error() + " (" + std::to_string(rc) + ")");
}

/* One engine context per device, shared by every block of the process (the reference's blocks share nothing; here they share the code
 * tables, the decoder plans and the FEC workspaces). */
class Engine {
public:
    static std::shared_ptr<Engine> get(int device = 0) {
        static std::mutex m;
        static std::weak_ptr<Engine> cache[16];
        if (device < 0 || device >= 16) throw std::runtime_error("dvbs2gpu: device index out of range");
        std::lock_guard<std::mutex> l(m);
        auto e = cache[device].lock();
        if (!e) {
            e.reset(new Engine(device));
            cache[device] = e;
        }
        return e;
    }
    ~Engine() { dvbs2gpu_destroy(ctx); }
    dvbs2gpu_ctx* ctx = nullptr;

private:
    explicit Engine(int device) { check(dvbs2gpu_create(device, &ctx)); }
    Engine(const Engine&) = delete;
};

namespace dvbs2 {

class DVBS2Demod {
public:
    DVBS2Demod() {}
    ~DVBS2Demod() { release(); }
    DVBS2Demod(const DVBS2Demod&) = delete;
    DVBS2Demod& operator=(const DVBS2Demod&) = delete;

    /* DVBS2Demod::init (module_dvbs2_demod.cpp:7-30) without the input stream; handler is called once per PL frame a call completes, with that
     * frame's symbols behind the PLL (the constellation display, :337), and may be null */
    void init(double symbolrate, double samplerate, float agc_rate, float rrc_alpha, int rrc_taps, float loop_bw, float fll_bw, double omegaGain,
              double muGain, void (*handler)(complex_t* data, int count, void* ctx), void* ctx, int modcod, bool shortframes, bool pilots,
              float sof_thresold, int max_ldpc_trials, double omegaRelLimit = 0.01, int device = 0) {
        release();
        eng = Engine::get(device);
        cfg.symbolrate = symbolrate; cfg.samplerate = samplerate; cfg.agc_rate = agc_rate; cfg.rrc_alpha = rrc_alpha; cfg.rrc_taps = rrc_taps;
        cfg.loop_bw = loop_bw; cfg.fll_bw = fll_bw; cfg.clock_omega_gain = (float)omegaGain; cfg.clock_mu_gain = (float)muGain;
        cfg.omega_rel_limit = (float)omegaRelLimit; cfg.modcod = modcod; cfg.shortframes = shortframes; cfg.pilots = pilots;
        cfg.sof_threshold = sof_thresold; cfg.max_ldpc_trials = max_ldpc_trials; cfg.force_ldpc_iters = 0;
        d_handler = handler; d_ctx = ctx;
        check(dvbs2gpu_demod_create(eng->ctx, &cfg, STREAM_BUFFER_SIZE, &h));
        if (quality_on) check(dvbs2gpu_demod_set_quality(h, 1));
    }
    void reset() { check(dvbs2gpu_demod_reset(need())); }
    /* per-frame Es/N0 and MER estimates (dvbs2gpu_demod_set_quality; an extension, off by default): esn0_db / mer_db and frameQuality() */
    void setQualityEstimation(bool on) {
        quality_on = on;
        if (h) check(dvbs2gpu_demod_set_quality(h, on ? 1 : 0));
    }
    void setDemodParams(int modcod, bool shortframes, bool pilots, float sof_thresold, int max_ldpc_trials) {
        check(dvbs2gpu_demod_set_params(need(), modcod, shortframes, pilots, sof_thresold, max_ldpc_trials));   // a bad MODCOD throws, old parameters stay
        cfg.modcod = modcod; cfg.shortframes = shortframes; cfg.pilots = pilots; cfg.sof_threshold = sof_thresold; cfg.max_ldpc_trials = max_ldpc_trials;
    }
    void setSymbolrate(double symbolrate) { cfg.symbolrate = symbolrate; rebuild(); }   // module_dvbs2_demod.cpp:153-166: new RRC taps, loops reset
    void setSamplerate(double samplerate) { cfg.samplerate = samplerate; rebuild(); }
    int getKBCH() { return dvbs2gpu_demod_get_kbch(need()); }

    /* module_dvbs2_demod.cpp:216: count samples in, the BBFRAMEs completed by this call out (getKBCH()/8 bytes each); returns bytes */
    int process(int count, const complex_t* in, uint8_t* out) {
        const int n = dvbs2gpu_demod_process(need(), count, reinterpret_cast<const float*>(in), out, STREAM_BUFFER_SIZE);
        check(n);
        // every PL frame this call completed (a call of STREAM_BUFFER_SIZE samples of short frames holds more than a fixed-size array would)
        const int k = dvbs2gpu_demod_get_stats(h, nullptr, 0);
        if (k > 0) {   // the public fields the plugin's menu polls (module_dvbs2_demod.h:82-87)
            stats.resize((size_t)k);
            dvbs2gpu_demod_get_stats(h, stats.data(), k);
            const dvbs2gpu_frame_stats& s = stats[(size_t)k - 1];
            detected_modcod = s.detected_modcod; detected_shortframes = s.detected_shortframes != 0; detected_pilots = s.detected_pilots != 0;
            pl_sync_best_match = s.pl_sync_best_match; ldpc_trials = (float)s.ldpc_trials; bch_corrections = (float)s.bch_corrections;
        }
        const int q = dvbs2gpu_demod_get_quality(h, nullptr, 0);
        check(q);
        quality.resize((size_t)q);
        if (q > 0) {   // one record per frame above; the polled figures from the call's last frame
            dvbs2gpu_demod_get_quality(h, quality.data(), q);
            esn0_db = quality[(size_t)q - 1].esn0_db; mer_db = quality[(size_t)q - 1].mer_db;
        }
        if (d_handler && k > 0) {
            // module_dvbs2_demod.cpp:337: the handler is called once per PL frame, with that frame's header + payload (+ pilot) symbols behind the PLL.
            // A CCM block's frames all have the configured MODCOD's PLFRAME length (dvbs2gpu_modcod_info): tap 2 holds k of them back to back.
            const int ns = dvbs2gpu_demod_get_tap(h, 2, nullptr, 0);
            dvbs2gpu_modcod_info mi;
            if (ns > 0 && dvbs2gpu_modcod_info_get(cfg.modcod, cfg.shortframes, cfg.pilots, &mi) == 0 && mi.plframe_symbols > 0 &&
                (long long)mi.plframe_symbols * k == ns) {
                tap.resize((size_t)ns);
                dvbs2gpu_demod_get_tap(h, 2, tap.data(), ns);
                for (int f = 0; f < k; ++f) d_handler(tap.data() + (size_t)f * mi.plframe_symbols, mi.plframe_symbols, d_ctx);
            }
        }
        return n;
    }

    int detected_modcod = -1;
    bool detected_shortframes = false;
    bool detected_pilots = false;
    float pl_sync_best_match = 0;
    float ldpc_trials = -1;
    float bch_corrections = -1;
    float esn0_db = NAN;      // with setQualityEstimation(true): the last frame's estimates (NaN until then)
    float mer_db = NAN;
    /* the quality records of the frames the last process() call completed, one per frame, in frame order */
    const std::vector<dvbs2gpu_frame_quality>& frameQuality() const { return quality; }

private:
    dvbs2gpu_demod* need() {
        if (!h) throw std::runtime_error("dvbs2gpu: DVBS2Demod used before init()");
        return h;
    }
    void rebuild() {
        if (!h) return;
        dvbs2gpu_demod* n = nullptr;
        check(dvbs2gpu_demod_create(eng->ctx, &cfg, STREAM_BUFFER_SIZE, &n));
        dvbs2gpu_demod_destroy(h);
        h = n;
        if (quality_on) check(dvbs2gpu_demod_set_quality(h, 1));
    }
    void release() {
        if (h) dvbs2gpu_demod_destroy(h);
        h = nullptr;
    }
    std::shared_ptr<Engine> eng;
    dvbs2gpu_demod_cfg cfg{};
    dvbs2gpu_demod* h = nullptr;
    void (*d_handler)(complex_t*, int, void*) = nullptr;
    void* d_ctx = nullptr;
    std::vector<complex_t> tap;
    std::vector<dvbs2gpu_frame_stats> stats;
    std::vector<dvbs2gpu_frame_quality> quality;
    bool quality_on = false;
};

struct BBHeader {   // bbframe_ts_parser.h:36-66
    int ts_gs = 0, sis_mis = 0, ccm_acm = 0, issyi = 0, npd = 0, ro = 0, isi = 0, upl = 0, dfl = 0, sync = 0, syncd = 0;
};

class BBFrameTSParser {
public:
    BBFrameTSParser() {}
    ~BBFrameTSParser() {
        if (h) dvbs2gpu_bbts_destroy(h);
    }
    BBFrameTSParser(const BBFrameTSParser&) = delete;
    BBFrameTSParser& operator=(const BBFrameTSParser&) = delete;

    void setFrameSize(int bbframe_size) {   // bbframe_ts_parser.cpp:31-42 (bits)
        if (!h) {
            eng = Engine::get(device);
            check(dvbs2gpu_bbts_create(eng->ctx, 1, bbframe_size, max_frames, &h));
        } else {
            check(dvbs2gpu_bbts_set_frame_size(h, bbframe_size));
        }
    }
    /* bbframe_ts_parser.cpp:104: cnt BBFRAMEs in, TS packets (or GSE PDUs) out; returns bytes.  buffer_outsize must be at least
     * cnt * kbch/8 + 376 (the reference's own "at least as big as bbframe"; it prints "BUFF OVF!" and stops otherwise: here the call throws) */
    int work(uint8_t* bbframe, int cnt, uint8_t* tsframes, int buffer_outsize) {
        if (!h) throw std::runtime_error("dvbs2gpu: BBFrameTSParser used before setFrameSize()");
        const int n = dvbs2gpu_bbts_work(h, bbframe, cnt, tsframes, buffer_outsize);
        check(n);
        int32_t s[15];
        check(dvbs2gpu_bbts_get_stats(h, 0, s, 15));
        last_header.ts_gs = s[0]; last_header.sis_mis = s[1]; last_header.ccm_acm = s[2]; last_header.issyi = s[3]; last_header.npd = s[4];
        last_header.ro = s[5]; last_header.isi = s[6]; last_header.upl = s[7]; last_header.dfl = s[8]; last_header.sync = s[9]; last_header.syncd = s[10];
        last_gse_crc_err = s[11] != 0; last_bb_cnt = s[12]; last_bb_proc = s[13]; last_ts_errs = s[14];
        return n;
    }

    /* ---- GSE (bbframe_ts_parser.cpp:212-383).  work() writes GRE packets back to back; the table has one row per packet of the last
     * work(): offset, bytes, protocol type, flags, so that a sink can send one datagram per PDU (main.cpp:551-555 sends one per call). */
    std::vector<dvbs2gpu_gse_pdu> pdu_table() {
        if (!h) throw std::runtime_error("dvbs2gpu: BBFrameTSParser used before setFrameSize()");
        int n = 0;
        check(dvbs2gpu_bbts_get_pdu_table(h, 0, nullptr, 0, &n));
        std::vector<dvbs2gpu_gse_pdu> rows(n);
        if (n > 0) check(dvbs2gpu_bbts_get_pdu_table(h, 0, rows.data(), n, &n));
        return rows;
    }
    dvbs2gpu_gse_stats gse_stats() {
        if (!h) throw std::runtime_error("dvbs2gpu: BBFrameTSParser used before setFrameSize()");
        dvbs2gpu_gse_stats s;
        check(dvbs2gpu_bbts_get_gse_stats(h, 0, &s));
        return s;
    }
    /* 0: GSE frames are parsed on the GPU (default); 1: by the library's host parser */
    void set_gse_path(int mode) {
        if (!h) throw std::runtime_error("dvbs2gpu: BBFrameTSParser used before setFrameSize()");
        check(dvbs2gpu_bbts_set_gse_path(h, mode));
    }

    /* ---- mode-adaptation mode (include/dvbs2gpu.h): multistream and ACM/VCM carriers.  Call after setFrameSize(); cfg == nullptr
     * switches it off again.  The reference-shaped work() above is not affected by it. */
    void setModeAdaptation(const dvbs2gpu_bbts_ma_cfg* cfg) {
        if (!h) throw std::runtime_error("dvbs2gpu: BBFrameTSParser used before setFrameSize()");
        check(dvbs2gpu_bbts_set_mode_adaptation(h, cfg));
    }
    /* the ISIs to deliver (at most 8): output k of the work() below is isi[k] */
    void selectISI(const uint8_t* isi, int n) {
        if (!h) throw std::runtime_error("dvbs2gpu: BBFrameTSParser used before setFrameSize()");
        check(dvbs2gpu_bbts_select_isi(h, 0, isi, n));
    }
    /* cnt BBFRAMEs back to back, frame_bytes[f] bytes each (nullptr: the size given to setFrameSize); tsframes[k] receives the
     * TS of the k-th selected ISI, out_bytes[k] its size (8 entries each; unused outputs may be nullptr).  Returns false, with the sizes
     * in needed[8] and nothing consumed, when buffer_outsize is too small for one of them: call again with larger buffers. */
    bool work(uint8_t* bbframes, const int* frame_bytes, int cnt, uint8_t* const* tsframes, int buffer_outsize, int* out_bytes, int* needed = nullptr) {
        if (!h) throw std::runtime_error("dvbs2gpu: BBFrameTSParser used before setFrameSize()");
        const int rc = dvbs2gpu_bbts_ma_work(h, bbframes, frame_bytes, cnt, tsframes, buffer_outsize, out_bytes, needed);
        if (rc == DVBS2GPU_ERR_CAPACITY) return false;
        check(rc);
        return true;
    }
    /* end of the stream: the packets held back for the CRC-8 that follows them */
    void flush(uint8_t* const* tsframes, int buffer_outsize, int* out_bytes) {
        if (!h) throw std::runtime_error("dvbs2gpu: BBFrameTSParser used before setFrameSize()");
        check(dvbs2gpu_bbts_ma_flush_host(h, tsframes, buffer_outsize, out_bytes));
    }
    /* GSE frames of the selected ISIs: decapsulated into output k like in work() of the reference mode, one reassembly context per
     * ISI (include/dvbs2gpu.h has the rules).  Off by default; needs setModeAdaptation() first. */
    void setModeAdaptationGSE(bool on) {
        if (!h) throw std::runtime_error("dvbs2gpu: BBFrameTSParser used before setFrameSize()");
        check(dvbs2gpu_bbts_ma_set_gse(h, on ? 1 : 0));
    }
    /* DVB-T2 high-efficiency-mode BBFRAMEs (those of a T2-MI feed) are parsed by their own rules (include/dvbs2gpu.h) instead of
     * being rejected.  Off by default; needs setModeAdaptation() first; the outputs start afresh. */
    void setModeAdaptationT2HEM(bool on) {
        if (!h) throw std::runtime_error("dvbs2gpu: BBFrameTSParser used before setFrameSize()");
        check(dvbs2gpu_bbts_ma_set_t2_hem(h, on ? 1 : 0));
    }
    dvbs2gpu_bbts_ma_gse_stats modeAdaptationGSEStats(int output) {
        dvbs2gpu_bbts_ma_gse_stats s;
        check(dvbs2gpu_bbts_ma_get_gse_stats(h, 0, output, &s));
        return s;
    }
    /* one row per GRE packet the last mode-adaptation work() wrote into output k; offsets are relative to tsframes[k] */
    std::vector<dvbs2gpu_gse_pdu> modeAdaptationPduTable(int output) {
        if (!h) throw std::runtime_error("dvbs2gpu: BBFrameTSParser used before setFrameSize()");
        int n = 0;
        check(dvbs2gpu_bbts_ma_get_pdu_table(h, 0, output, nullptr, 0, &n));
        std::vector<dvbs2gpu_gse_pdu> rows(n);
        if (n > 0) check(dvbs2gpu_bbts_ma_get_pdu_table(h, 0, output, rows.data(), n, &n));
        return rows;
    }
    dvbs2gpu_bbts_ma_stats modeAdaptationStats(int output) {
        dvbs2gpu_bbts_ma_stats s;
        check(dvbs2gpu_bbts_ma_get_stats(h, 0, output, &s));
        return s;
    }

    BBHeader last_header;
    bool last_gse_crc_err = 0;
    int last_bb_cnt = 0;
    int last_bb_proc = 0;
    int last_ts_errs = 0;

    int device = 0;
    int max_frames = 64;   // most BBFRAMEs one work() call may bring (the plugin's sink handler passes what one process() call produced)

private:
    std::shared_ptr<Engine> eng;
    dvbs2gpu_bbts* h = nullptr;
};

}   // namespace dvbs2

namespace dvbs {

class DVBSDemod {
public:
    DVBSDemod() {}
    ~DVBSDemod() { release(); }
    DVBSDemod(const DVBSDemod&) = delete;
    DVBSDemod& operator=(const DVBSDemod&) = delete;

    /* DVBSDemod::init (module_dvbs_demod.cpp:9-31) without the input stream; handler receives the symbols after the Costas loop (:33-37) */
    void init(double symbolrate, double samplerate, float agc_rate, float rrc_alpha, int rrc_taps, float loop_bw, float fll_bw, double omegaGain,
              double muGain, void (*handler)(complex_t* data, int count, void* ctx), void* ctx, double omegaRelLimit = 0.01, int device = 0) {
        release();
        eng = Engine::get(device);
        dvbs2gpu_dvbs_demod_default_cfg(&cfg);
        cfg.symbolrate = symbolrate; cfg.samplerate = samplerate; cfg.agc_rate = agc_rate; cfg.rrc_alpha = rrc_alpha; cfg.rrc_taps = rrc_taps;
        cfg.loop_bw = loop_bw; cfg.fll_bw = fll_bw; cfg.clock_omega_gain = (float)omegaGain; cfg.clock_mu_gain = (float)muGain;
        cfg.omega_rel_limit = (float)omegaRelLimit;
        d_handler = handler; d_ctx = ctx;
        build();
    }
    void reset() {   // module_dvbs_demod.cpp:58-64
        check(dvbs2gpu_dvbs_demod_reset(need()));
        check(dvbs2gpu_dvbs_tail_reset(t));
    }
    /* per-call Es/N0 (M2M4) and MER of the symbols after the Costas loop (dvbs2gpu_dvbs_demod_set_quality; an extension, off by default) */
    void setQualityEstimation(bool on) {
        quality_on = on;
        if (h) check(dvbs2gpu_dvbs_demod_set_quality(h, on ? 1 : 0));
    }
    void setSymbolrate(double symbolrate) { cfg.symbolrate = symbolrate; if (h) { release(); build(); } }
    void setSamplerate(double samplerate) { cfg.samplerate = samplerate; if (h) { release(); build(); } }

    /* module_dvbs_demod.cpp:78-117: count samples in, TS packets out (188 bytes each); returns bytes */
    int process(int count, const complex_t* in, uint8_t* out) {
        const int n = dvbs2gpu_dvbs_process_ts(need(), t, count, reinterpret_cast<const float*>(in), out, STREAM_BUFFER_SIZE);
        check(n);
        dvbs2gpu_viterbi_stats vs;
        check(dvbs2gpu_dvbs_demod_get_stats(h, &vs));
        stats_viterbi_ber = vs.ber; stats_viterbi_lock = vs.state;
        static const char* const names[5] = {"1/2", "2/3", "3/4", "5/6", "7/8"};
        stats_viterbi_rate = vs.rate >= 0 && vs.rate < 5 ? names[vs.rate] : "";
        int32_t ts[11];
        check(dvbs2gpu_dvbs_tail_get_stats(t, 0, ts));
        if (ts[0] > 0) {   // :115-116, from the last frame of the call
            int sum = 0;
            for (int i = 0; i < 8; ++i) sum += ts[3 + i];
            stats_rs_avg = (float)(sum / 8);   // (an integer mean in the reference too: int errors[8])
        }
        stats_deframer_err = std::min(ts[1], ts[2]);
        dvbs2gpu_dvbs_quality q;
        const int nq = dvbs2gpu_dvbs_demod_get_quality(h, &q);
        check(nq);
        if (nq > 0) { stats_esn0_db = q.esn0_db; stats_mer_db = q.mer_db; }
        if (d_handler) {
            const int ns = dvbs2gpu_dvbs_demod_get_tap(h, 0, 0, nullptr, 0);
            if (ns > 0) {
                tap.resize((size_t)ns);
                dvbs2gpu_dvbs_demod_get_tap(h, 0, 0, tap.data(), ns);
                d_handler(tap.data(), ns, d_ctx);
            }
        }
        return n;
    }

    float stats_viterbi_ber = 0;
    int stats_viterbi_lock = 0;
    std::string stats_viterbi_rate = "";
    float stats_rs_avg = 0;
    int stats_deframer_err = 0;
    float stats_esn0_db = NAN;   // with setQualityEstimation(true): the last call's estimates (NaN until then)
    float stats_mer_db = NAN;

private:
    dvbs2gpu_dvbs_demod* need() {
        if (!h) throw std::runtime_error("dvbs2gpu: DVBSDemod used before init()");
        return h;
    }
    void build() {
        check(dvbs2gpu_dvbs_demod_create(eng->ctx, &cfg, 1, STREAM_BUFFER_SIZE, &h));
        const int rc = dvbs2gpu_dvbs_tail_create(eng->ctx, 1, STREAM_BUFFER_SIZE + 4 * 8192, &t);
        if (rc < 0) { release(); check(rc); }
        if (quality_on) check(dvbs2gpu_dvbs_demod_set_quality(h, 1));
    }
    void release() {
        if (h) dvbs2gpu_dvbs_demod_destroy(h);
        if (t) dvbs2gpu_dvbs_tail_destroy(t);
        h = nullptr; t = nullptr;
    }
    std::shared_ptr<Engine> eng;
    dvbs2gpu_dvbs_cfg cfg{};
    dvbs2gpu_dvbs_demod* h = nullptr;
    dvbs2gpu_dvbs_tail* t = nullptr;
    void (*d_handler)(complex_t*, int, void*) = nullptr;
    void* d_ctx = nullptr;
    std::vector<complex_t> tap;
    bool quality_on = false;
};

}   // namespace dvbs

/* The transponders of one host over several GPUs (dvbs2gpu_fleet_*, include/dvbs2gpu.h): the reference runs one independent DVBS2Demod per transponder
 * (src/main.cpp:588,595); a Fleet places a table of them on its members -- one engine context + worker thread per device -- by the MODCOD-grouped
 * longest-processing-time rule and returns every call's BBFRAMEs in table order.  Every failing call throws std::runtime_error, as above. */
class Fleet {
public:
    explicit Fleet(const std::vector<int>& devices) { check(dvbs2gpu_fleet_create(devices.data(), (int)devices.size(), &f)); }
    ~Fleet() { dvbs2gpu_fleet_destroy(f); }
    Fleet(const Fleet&) = delete;
    Fleet& operator=(const Fleet&) = delete;

    /* one table entry per transponder: DVBS2Demod::init's parameters as the plugin sets them (main.cpp:64-73,134-140), cfg.modcod etc. per transponder */
    static dvbs2gpu_fleet_entry entry(int modcod, bool shortframes, bool pilots, int max_samples, int max_ldpc_trials = 16, int force_ldpc_iters = 0, double weight = 0.0) {
        dvbs2gpu_fleet_entry e{};
        dvbs2gpu_demod_default_cfg(modcod, shortframes, pilots, &e.cfg);
        e.cfg.max_ldpc_trials = max_ldpc_trials; e.cfg.force_ldpc_iters = force_ldpc_iters;
        e.weight = weight; e.max_samples = max_samples;
        return e;
    }
    /* places the table; returns the member of every transponder */
    std::vector<int> assign(const std::vector<dvbs2gpu_fleet_entry>& table, int out_cap, double tolerance = 0.25) {
        std::vector<int32_t> m(table.size());
        check(dvbs2gpu_fleet_assign(f, table.data(), (int)table.size(), out_cap, tolerance, m.data()));
        nt = (int)table.size(); cap = out_cap;
        return std::vector<int>(m.begin(), m.end());
    }
    void setPipelined(bool on) { check(dvbs2gpu_fleet_set_pipelined(f, on ? 1 : 0)); }
    void reset() { check(dvbs2gpu_fleet_reset(f)); }
    /* one call for all transponders, in table order: in[i] / count[i] samples of transponder i, out[i] receives its BBFRAMEs (capacity: assign's out_cap); returns the byte counts */
    std::vector<int> process(const std::vector<const complex_t*>& in, const std::vector<int>& count, const std::vector<uint8_t*>& out) {
        if ((int)in.size() != nt || (int)count.size() != nt || (int)out.size() != nt) throw std::runtime_error("dvbs2gpu: Fleet::process needs one entry per transponder");
        std::vector<int> nb((size_t)nt, 0);
        check(dvbs2gpu_fleet_process_batch(f, reinterpret_cast<const float* const*>(in.data()), count.data(), out.data(), cap, nb.data()));
        return nb;
    }
    int size() const { return dvbs2gpu_fleet_size(f); }

private:
    dvbs2gpu_fleet* f = nullptr;
    int nt = 0, cap = 0;
};

namespace detail {
/* What the bank classes below share: the engine, the handle and its destruction, need() for the calls that throw, and the sticky
 * status of the work() that does not.  A: the bank's  Handle,  name ("PsiBank")  and  destroy (a pointer to the C function). */
template <typename A>
class Bank {
public:
    Bank() {}
    ~Bank() { release(); }
    Bank(const Bank&) = delete;
    Bank& operator=(const Bank&) = delete;

    int status() const { return status_; }
    const std::string& error() const { return error_; }
    void clearStatus() { status_ = 0; error_.clear(); }

protected:
    void release() {
        if (h) A::destroy(h);
        h = nullptr;
    }
    typename A::Handle* need() {
        if (!h) throw std::runtime_error(std::string("dvbs2gpu: ") + A::name + " used before init()");
        return h;
    }
    /* a work() that failed with rc: the first failure is kept; returns 0 */
    int fail(int rc) noexcept {
        if (status_ == 0) {
            status_ = rc;
            try { error_ = h ? dvbs2gpu_last_error() : std::string(A::name) + " used before init()"; } catch (...) {}
        }
        return 0;
    }
    std::shared_ptr<Engine> eng;
    typename A::Handle* h = nullptr;

private:
    int status_ = 0;
    std::string error_;
};
struct TsmonApi { typedef dvbs2gpu_tsmon Handle; static constexpr const char* name = "TSMonitor"; static constexpr auto destroy = &dvbs2gpu_tsmon_destroy; };
struct PsiApi { typedef dvbs2gpu_psi Handle; static constexpr const char* name = "PsiBank"; static constexpr auto destroy = &dvbs2gpu_psi_destroy; };
struct IptsApi { typedef dvbs2gpu_ipts Handle; static constexpr const char* name = "IpTsBank"; static constexpr auto destroy = &dvbs2gpu_ipts_destroy; };
struct IpoutApi { typedef dvbs2gpu_ipout Handle; static constexpr const char* name = "IpOutBank"; static constexpr auto destroy = &dvbs2gpu_ipout_destroy; };
}   // namespace detail

/* TS monitor for one transport stream (dvbs2gpu_tsmon_*, include/dvbs2gpu.h; an extension, the reference has no counterpart): a block
 * behind BBFrameTSParser or DVBSDemod in a sink handler.  init() and the setters throw like everything above.  work() sits in the
 * data path and does NOT throw: a failing call returns 0 bytes and leaves its code in status() and its text in error(), where they
 * stay (sticky: the first failure is kept, later calls still run) until clearStatus(). */
class TSMonitor : public detail::Bank<detail::TsmonApi> {
public:
    void init(int max_packets, int device = 0) {
        release();
        eng = Engine::get(device);
        check(dvbs2gpu_tsmon_create(eng->ctx, 1, max_packets, &h));
    }
    void reset() { check(dvbs2gpu_tsmon_reset(need())); }
    /* mode 0 pass all, 1 pass the listed PIDs, 2 drop them */
    void setFilter(int mode, const std::vector<uint16_t>& pids, bool drop_null = false, bool drop_tei = false, bool drop_bad_sync = false) {
        const dvbs2gpu_tsmon_filter f = {mode, drop_null, drop_tei, drop_bad_sync};
        check(dvbs2gpu_tsmon_set_filter(need(), 0, &f, pids.data(), (int)pids.size()));
    }
    /* nbytes of whole TS packets in; the passing packets to `out` (nullptr: statistics and table only); returns the bytes written,
     * 0 on failure (see status()) */
    int work(const uint8_t* ts, int nbytes, uint8_t* out, int buffer_outsize) noexcept {
        const int n = h ? dvbs2gpu_tsmon_work(h, 0, ts, nbytes, out, buffer_outsize) : DVBS2GPU_ERR_ARG;
        return n >= 0 ? n : fail(n);
    }

    dvbs2gpu_tsmon_stats stats() {
        dvbs2gpu_tsmon_stats s;
        check(dvbs2gpu_tsmon_get_stats(need(), 0, &s));
        return s;
    }
    /* one row per PID of the last work(), ascending */
    std::vector<dvbs2gpu_tsmon_pid> pidTable() {
        int n = 0;
        check(dvbs2gpu_tsmon_get_pid_table(need(), 0, nullptr, 0, &n));
        std::vector<dvbs2gpu_tsmon_pid> rows((size_t)n);
        if (n > 0) check(dvbs2gpu_tsmon_get_pid_table(h, 0, rows.data(), n, &n));
        return rows;
    }
};

/* PSI section bank for one transport stream (dvbs2gpu_psi_*, include/dvbs2gpu.h; an extension): PAT / PMT / SI sections of up to 16
 * watched PIDs behind BBFrameTSParser, DVBSDemod or TSMonitor.  init() (a device bank) or initHost() (the library's host
 * implementation, no device) and the setters throw; work() sits in the data path and does NOT throw: a failing call returns 0 bytes
 * and leaves its code in status() and its text in error(), sticky until clearStatus(). */
class PsiBank : public detail::Bank<detail::PsiApi> {
public:
    void init(int max_packets, int max_sections, int device = 0) {
        release();
        eng = Engine::get(device);
        check(dvbs2gpu_psi_create(eng->ctx, 1, max_packets, max_sections, &h));
    }
    void initHost(int max_packets, int max_sections) {
        release();
        check(dvbs2gpu_psi_create_host(1, max_packets, max_sections, &h));
    }
    void reset() { check(dvbs2gpu_psi_reset(need())); }
    /* slot 0..15; pid -1 clears the slot; expect_table_id -1: any */
    void setWatch(int slot, int pid, int expect_table_id = -1) {
        check(dvbs2gpu_psi_set_watch(need(), 0, slot, pid, expect_table_id));
        watched[slot] = pid;
    }
    void setDeliver(int mode) { check(dvbs2gpu_psi_set_deliver(need(), 0, mode)); }
    /* slots 1..15 start afresh and watch the PMT PIDs of the PAT's programs (not program 0), expecting table_id 2, as far as the
     * slots go; returns the programs that did not fit */
    std::vector<dvbs2gpu_psi_program> followPat() {
        dvbs2gpu_psi_pat hdr;
        std::vector<dvbs2gpu_psi_program> left, seen;
        int slot = 1;
        for (int s = 1; s < 16; ++s) setWatch(s, -1);
        for (const dvbs2gpu_psi_program& p : programs(&hdr)) {
            if (p.program_number == 0 || p.pid == watched[0]) continue;   // (a PMT PID that slot 0 watches already stays there)
            if (std::any_of(seen.begin(), seen.end(), [&](const dvbs2gpu_psi_program& q) { return q.pid == p.pid; })) continue;
            if (slot >= 16) { left.push_back(p); continue; }
            seen.push_back(p);
            setWatch(slot++, p.pid, 2);
        }
        return left;
    }
    /* nbytes of whole TS packets in; the delivered sections to `out` (nullptr: rows and counters only); returns the bytes written,
     * 0 on failure (see status(); after DVBS2GPU_ERR_CAPACITY needed() holds the sizes) */
    int work(const uint8_t* ts, int nbytes, uint8_t* out, int buffer_outsize) noexcept {
        const int n = h ? dvbs2gpu_psi_work(h, 0, ts, nbytes, out, buffer_outsize) : DVBS2GPU_ERR_ARG;
        return n >= 0 ? n : fail(n);
    }
    void needed(int* bytes, int* rows) { check(dvbs2gpu_psi_get_needed(need(), 0, bytes, rows)); }

    dvbs2gpu_psi_stats stats(int slot = -1) {
        dvbs2gpu_psi_stats s;
        check(dvbs2gpu_psi_get_stats(need(), 0, slot, &s));
        return s;
    }
    /* one row per section of the last work(), in row order */
    std::vector<dvbs2gpu_psi_section> sectionTable() {
        int n = 0;
        check(dvbs2gpu_psi_get_section_table(need(), 0, nullptr, 0, &n));
        std::vector<dvbs2gpu_psi_section> rows((size_t)n);
        if (n > 0) check(dvbs2gpu_psi_get_section_table(h, 0, rows.data(), n, &n));
        return rows;
    }
    std::vector<dvbs2gpu_psi_program> programs(dvbs2gpu_psi_pat* hdr) {
        int n = 0;
        check(dvbs2gpu_psi_get_programs(need(), 0, hdr, nullptr, 0, &n));
        std::vector<dvbs2gpu_psi_program> rows((size_t)n);
        if (n > 0) check(dvbs2gpu_psi_get_programs(h, 0, hdr, rows.data(), n, &n));
        return rows;
    }
    std::vector<dvbs2gpu_psi_es> programMap(int slot, dvbs2gpu_psi_pmt* hdr) {
        int n = 0;
        check(dvbs2gpu_psi_get_program_map(need(), 0, slot, hdr, nullptr, 0, &n));
        std::vector<dvbs2gpu_psi_es> rows((size_t)n);
        if (n > 0) check(dvbs2gpu_psi_get_program_map(h, 0, slot, hdr, rows.data(), n, &n));
        return rows;
    }

private:
    void release() {
        Bank::release();
        std::fill(watched, watched + 16, -1);
        watched[0] = 0;                                    // a new bank watches the PAT in slot 0
    }
    int watched[16] = {0, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1};   // slot -> PID, as setWatch left them
};

namespace detail {
/* What PcrBank, PesBank, EsBank and AudBank share (the watched-PID banks: dvbs2gpu_pcr_*, dvbs2gpu_pes_*, dvbs2gpu_es_*, dvbs2gpu_aud_*): everything but
 * setWatch(), the rate and which PIDs of a PMT followPmts() takes.  A: the bank's C functions and types --  Handle, Stats, StreamStats,
 * Row;  name ("PcrBank");  create, create_host, destroy, reset, work, get_stats, get_stream_stats, get_row_table (pointers to the C
 * functions). */
template <typename A>
class WatchBank : public Bank<A> {
public:
    void init(int max_packets, int max_rows, int device = 0) {
        release();
        this->eng = Engine::get(device);
        check(A::create(this->eng->ctx, 1, max_packets, max_rows, &this->h));
    }
    void initHost(int max_packets, int max_rows) {
        release();
        check(A::create_host(1, max_packets, max_rows, &this->h));
    }
    void reset() { check(A::reset(this->need())); }
    /* nbytes of whole TS packets in; returns the rows of the call (PcrBank: the records, PCR packets of watched PIDs; PesBank: the
     * starts, PES packet starts on watched PIDs), 0 on failure (see status()) */
    int work(const uint8_t* ts, int nbytes) noexcept {
        const int n = this->h ? A::work(this->h, 0, ts, nbytes) : DVBS2GPU_ERR_ARG;
        return n >= 0 ? n : this->fail(n);
    }

    typename A::Stats stats(int slot = -1) {
        typename A::Stats s;
        check(A::get_stats(this->need(), 0, slot, &s));
        return s;
    }
    typename A::StreamStats streamStats() {
        typename A::StreamStats s;
        check(A::get_stream_stats(this->need(), 0, &s));
        return s;
    }

protected:
    /* the rows of the last work() (the first max_rows) */
    std::vector<typename A::Row> table() {
        int n = 0;
        check(A::get_row_table(this->need(), 0, nullptr, 0, &n));
        std::vector<typename A::Row> rows((size_t)n);
        if (n > 0) check(A::get_row_table(this->h, 0, rows.data(), n, &n));
        return rows;
    }
    /* followPmts(): for every PMT that `psi` holds decoded, in the order of its slots, pick(pmt, es, offer) calls offer(pid, extra) for
     * the PIDs the bank would watch; 0x1FFF and above and PIDs watched already are skipped, the others go to free slots through
     * set(slot, pid, extra); returns the PIDs that found no free slot */
    template <typename Pick, typename Set>
    std::vector<int> followWith(PsiBank& psi, Pick pick, Set set) {
        std::vector<int> left;
        for (int slot = 0; slot < 16; ++slot) {
            dvbs2gpu_psi_pmt pmt;
            const std::vector<dvbs2gpu_psi_es> es = psi.programMap(slot, &pmt);
            if (pmt.program_number < 0) continue;
            pick(pmt, es, [&](int pid, int extra) {
                if (pid >= 0x1FFF || std::find(watched, watched + 16, pid) != watched + 16 || std::find(left.begin(), left.end(), pid) != left.end()) return;
                int* free_slot = std::find(watched, watched + 16, -1);
                if (free_slot == watched + 16) left.push_back(pid);
                else set((int)(free_slot - watched), pid, extra);
            });
        }
        return left;
    }
    int watched[16] = {-1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1};   // slot -> PID, as setWatch left them

private:
    void release() {
        Bank<A>::release();
        std::fill(watched, watched + 16, -1);
    }
};
/* the A of a watched-PID bank: its types and C functions by prefix */
#define DVBS2GPU_WATCH_API(Api, cls, p)                                                                                                  \
    struct Api {                                                                                                                         \
        typedef dvbs2gpu_##p Handle; typedef dvbs2gpu_##p##_stats Stats; typedef dvbs2gpu_##p##_stream_stats StreamStats;                \
        typedef dvbs2gpu_##p##_row Row;                                                                                                  \
        static constexpr const char* name = cls;                                                                                         \
        static constexpr auto create = &dvbs2gpu_##p##_create, create_host = &dvbs2gpu_##p##_create_host;                                \
        static constexpr auto destroy = &dvbs2gpu_##p##_destroy;                                                                         \
        static constexpr auto reset = &dvbs2gpu_##p##_reset;                                                                             \
        static constexpr auto work = &dvbs2gpu_##p##_work;                                                                               \
        static constexpr auto get_stats = &dvbs2gpu_##p##_get_stats;                                                                     \
        static constexpr auto get_stream_stats = &dvbs2gpu_##p##_get_stream_stats;                                                       \
        static constexpr auto get_row_table = &dvbs2gpu_##p##_get_row_table;                                                             \
        static constexpr auto set_watch = &dvbs2gpu_##p##_set_watch;                                                                     \
    }
DVBS2GPU_WATCH_API(PcrApi, "PcrBank", pcr);
DVBS2GPU_WATCH_API(PesApi, "PesBank", pes);
DVBS2GPU_WATCH_API(EsWatchApi, "EsBank", es);
DVBS2GPU_WATCH_API(AudWatchApi, "AudBank", aud);
#undef DVBS2GPU_WATCH_API
struct EsApi : EsWatchApi {
    /* the codec of a PMT stream_type: 0x01 / 0x02 MPEG2, 0x1B H264, 0x24 H265, 0: none of them */
    static int codecOf(int stream_type) {
        return stream_type == 0x01 || stream_type == 0x02 ? DVBS2GPU_ES_MPEG2 : stream_type == 0x1B ? DVBS2GPU_ES_H264 : stream_type == 0x24 ? DVBS2GPU_ES_H265 : 0;
    }
};
struct AudApi : AudWatchApi {
    /* the codec of a PMT stream_type: 0x03 / 0x04 MPA, 0x0F ADTS, 0x81 / 0x87 AC3, 0: none of them.  The PMT views carry no
     * descriptors: DVB's AC-3 in private stream type 0x06 cannot be told, the caller names such a PID with setWatch() */
    static int codecOf(int stream_type) {
        return stream_type == 0x03 || stream_type == 0x04 ? DVBS2GPU_AUD_MPA : stream_type == 0x0F ? DVBS2GPU_AUD_ADTS
             : stream_type == 0x81 || stream_type == 0x87 ? DVBS2GPU_AUD_AC3 : 0;
    }
};
/* What EsBank and AudBank share beyond WatchBank (the banks that are told a codec per slot): setWatch() with the codec, codecOf(),
 * followPmts() by it and rows().  A adds set_watch and codecOf to what WatchBank asks for. */
template <typename A>
class CodecBank : public WatchBank<A> {
public:
    /* slot 0..15; pid -1 clears the slot; codec: one of the bank's DVBS2GPU_ES_* / DVBS2GPU_AUD_* codecs */
    void setWatch(int slot, int pid, int codec = 0) {
        check(A::set_watch(this->need(), 0, slot, pid, codec));
        this->watched[slot] = pid;
    }
    /* the codec of a PMT stream_type, 0: none of the bank's */
    static int codecOf(int stream_type) { return A::codecOf(stream_type); }
    /* watches the PIDs of the PMTs that `psi` holds decoded whose stream type codecOf() knows, in free slots, in the order of its
     * slots and then of each PMT's elementary streams; other stream types and PIDs watched already are skipped; returns the PIDs
     * that found no free slot */
    std::vector<int> followPmts(PsiBank& psi) {
        return this->followWith(psi, [](const dvbs2gpu_psi_pmt&, const std::vector<dvbs2gpu_psi_es>& es, auto offer) {
            for (const dvbs2gpu_psi_es& e : es)
                if (const int codec = A::codecOf(e.stream_type)) offer(e.elementary_pid, codec);
        }, [this](int slot, int pid, int codec) { setWatch(slot, pid, codec); });
    }
    /* the rows of the last work(), in row order (the first max_rows) */
    std::vector<typename A::Row> rows() { return this->table(); }
};
}   // namespace detail
/* PCR bank for one transport stream (dvbs2gpu_pcr_*, include/dvbs2gpu.h; an extension): PCR repetition, discontinuity and accuracy
 * checks on up to 16 watched PIDs behind BBFrameTSParser, DVBSDemod or TSMonitor.  init() (a device bank) or initHost() (the
 * library's host implementation, no device) and the setters throw; work() sits in the data path and does NOT throw: a failing call
 * returns 0 and leaves its code in status() and its text in error(), sticky until clearStatus(). */
class PcrBank : public detail::WatchBank<detail::PcrApi> {
public:
    /* slot 0..15; pid -1 clears the slot */
    void setWatch(int slot, int pid) {
        check(dvbs2gpu_pcr_set_watch(need(), 0, slot, pid));
        watched[slot] = pid;
    }
    /* 27 MHz ticks per 188-byte packet in Q24.24 (0: no accuracy check), the accuracy limit in 1/64 tick */
    void setRate(uint64_t ticks_per_packet_q24, int limit_q6 = 864) { check(dvbs2gpu_pcr_set_rate(need(), 0, ticks_per_packet_q24, limit_q6)); }
    /* watches the PCR PIDs of the PMTs that `psi` holds decoded, in free slots, in the order of its slots; 0x1FFF and PIDs watched
     * already are skipped; returns the PIDs that found no free slot */
    std::vector<int> followPmts(PsiBank& psi) {
        return followWith(psi, [](const dvbs2gpu_psi_pmt& pmt, const std::vector<dvbs2gpu_psi_es>&, auto offer) { if (pmt.pcr_pid >= 0) offer(pmt.pcr_pid, 0); },
                          [this](int slot, int pid, int) { setWatch(slot, pid); });
    }
    /* bit/s as the slot's PCRs give it; 0 with no pairs */
    double rate(int slot = -1) {
        double v = 0;
        check(dvbs2gpu_pcr_get_rate(need(), 0, slot, &v));
        return v;
    }
    /* one row per PCR of the last work(), in input order (the first max_rows) */
    std::vector<dvbs2gpu_pcr_row> rowTable() { return table(); }
};

/* PES bank for one transport stream (dvbs2gpu_pes_*, include/dvbs2gpu.h; an extension): PES packet starts, PES length checks and
 * PTS / DTS checks on up to 16 watched PIDs behind BBFrameTSParser, DVBSDemod or TSMonitor.  init() (a device bank) or initHost() (the
 * library's host implementation, no device) and the setters throw; work() sits in the data path and does NOT throw: a failing call
 * returns 0 and leaves its code in status() and its text in error(), sticky until clearStatus(). */
class PesBank : public detail::WatchBank<detail::PesApi> {
public:
    /* slot 0..15; pid -1 clears the slot */
    void setWatch(int slot, int pid) {
        check(dvbs2gpu_pes_set_watch(need(), 0, slot, pid));
        watched[slot] = pid;
    }
    /* 27 MHz ticks per 188-byte packet in Q24.24, the quantity of PcrBank::setRate (0: no PTS_LATE) */
    void setRate(uint64_t ticks_per_packet_q24) { check(dvbs2gpu_pes_set_rate(need(), 0, ticks_per_packet_q24)); }
    /* watches the elementary PIDs of the PMTs that `psi` holds decoded, in free slots, in the order of its slots and then of each
     * PMT's elementary streams; stream types that carry sections and PIDs watched already are skipped; returns the PIDs that found
     * no free slot */
    std::vector<int> followPmts(PsiBank& psi, const std::vector<int>& skip_types = {0x05, 0x0A, 0x0B, 0x0C, 0x0D, 0x86}) {
        return followWith(psi, [&](const dvbs2gpu_psi_pmt&, const std::vector<dvbs2gpu_psi_es>& es, auto offer) {
            for (const dvbs2gpu_psi_es& e : es)
                if (std::find(skip_types.begin(), skip_types.end(), (int)e.stream_type) == skip_types.end()) offer(e.elementary_pid, 0);
        }, [this](int slot, int pid, int) { setWatch(slot, pid); });
    }
    /* one row per start of the last work(), in input order (the first max_rows) */
    std::vector<dvbs2gpu_pes_row> rowTable() { return table(); }
};
/* ES bank for one transport stream (dvbs2gpu_es_*, include/dvbs2gpu.h; an extension): a picture, GOP and parameter-set index of up to
 * 16 watched video PIDs (MPEG-2, H.264, H.265) behind BBFrameTSParser, DVBSDemod or TSMonitor, one row per PES packet start and per
 * reported start code.  init() (a device bank) or initHost() (the library's host implementation, no device) and the setters throw;
 * work() sits in the data path and does NOT throw: a failing call returns 0 and leaves its code in status() and its text in error(),
 * sticky until clearStatus().  setWatch(slot, pid, codec) takes DVBS2GPU_ES_MPEG2, _H264 or _H265; followPmts() the video PIDs. */
class EsBank : public detail::CodecBank<detail::EsApi> {};
/* Audio bank for one transport stream (dvbs2gpu_aud_*, include/dvbs2gpu.h; an extension): a frame index of up to 16 watched audio PIDs
 * (MPEG audio, ADTS, AC-3 / E-AC-3) behind BBFrameTSParser, DVBSDemod or TSMonitor, one row per PES packet start, per frame and per
 * loss of framing.  init() (a device bank) or initHost() (the library's host implementation, no device) and the setters throw;
 * work() sits in the data path and does NOT throw: a failing call returns 0 and leaves its code in status() and its text in error(),
 * sticky until clearStatus().  setWatch(slot, pid, codec) takes DVBS2GPU_AUD_MPA, _ADTS or _AC3; followPmts() the audio PIDs. */
class AudBank : public detail::CodecBank<detail::AudApi> {};
namespace detail {
/* What MpeBank, UleBank and T2miBank share (the datagram banks: dvbs2gpu_mpe_*, dvbs2gpu_ule_*, dvbs2gpu_t2mi_*): everything but
 * setWatch() and what T2miBank has for the mode-adaptation packetiser.  A: the bank's C
 * functions and types --  Handle, Stats, Row;  name ("MpeBank");  create, create_host, destroy, reset, work, get_needed, get_stats,
 * get_row_table (pointers to the C functions). */
template <typename A>
class DatagramBank : public Bank<A> {
protected:
    using Bank<A>::eng;
    using Bank<A>::h;
    using Bank<A>::need;
    using Bank<A>::release;

public:
    void init(int max_packets, int max_rows, int device = 0) {
        release();
        eng = Engine::get(device);
        check(A::create(eng->ctx, 1, max_packets, max_rows, &h));
    }
    void initHost(int max_packets, int max_rows) {
        release();
        check(A::create_host(1, max_packets, max_rows, &h));
    }
    void reset() { check(A::reset(need())); }
    /* nbytes of whole TS packets in for one slot; datagrams (buffer_outsize bytes; nullptr: rows and counters only) receives the
     * slot's IP datagrams (T2miBank: BBFRAMEs) back to back; returns their bytes, 0 on failure (see status(); on
     * DVBS2GPU_ERR_CAPACITY needed() has the sizes and nothing was consumed) */
    int work(int slot, const uint8_t* ts, int nbytes, uint8_t* datagrams, int buffer_outsize) noexcept {
        const int n = h ? A::work(h, 0, slot, ts, nbytes, datagrams, buffer_outsize) : DVBS2GPU_ERR_ARG;
        return n >= 0 ? n : this->fail(n);
    }
    /* {bytes, rows} that the slot's last work() needed */
    std::pair<int, int> needed(int slot) {
        int b = 0, r = 0;
        check(A::get_needed(need(), 0, slot, &b, &r));
        return {b, r};
    }

    typename A::Stats stats(int slot = -1) {
        typename A::Stats s;
        check(A::get_stats(need(), 0, slot, &s));
        return s;
    }
    /* one row per unit (section, SNDU, T2-MI packet) of the slot's last work(), in row order */
    std::vector<typename A::Row> rowTable(int slot) {
        int n = 0;
        check(A::get_row_table(need(), 0, slot, nullptr, 0, &n));
        std::vector<typename A::Row> rows((size_t)n);
        if (n > 0) check(A::get_row_table(h, 0, slot, rows.data(), n, &n));
        return rows;
    }
};
struct MpeApi {
    typedef dvbs2gpu_mpe Handle; typedef dvbs2gpu_mpe_stats Stats; typedef dvbs2gpu_mpe_row Row;
    static constexpr const char* name = "MpeBank";
    static constexpr auto create = &dvbs2gpu_mpe_create, create_host = &dvbs2gpu_mpe_create_host;
    static constexpr auto destroy = &dvbs2gpu_mpe_destroy;
    static constexpr auto reset = &dvbs2gpu_mpe_reset;
    static constexpr auto work = &dvbs2gpu_mpe_work;
    static constexpr auto get_needed = &dvbs2gpu_mpe_get_needed;
    static constexpr auto get_stats = &dvbs2gpu_mpe_get_stats;
    static constexpr auto get_row_table = &dvbs2gpu_mpe_get_row_table;
};
struct UleApi {
    typedef dvbs2gpu_ule Handle; typedef dvbs2gpu_ule_stats Stats; typedef dvbs2gpu_ule_row Row;
    static constexpr const char* name = "UleBank";
    static constexpr auto create = &dvbs2gpu_ule_create, create_host = &dvbs2gpu_ule_create_host;
    static constexpr auto destroy = &dvbs2gpu_ule_destroy;
    static constexpr auto reset = &dvbs2gpu_ule_reset;
    static constexpr auto work = &dvbs2gpu_ule_work;
    static constexpr auto get_needed = &dvbs2gpu_ule_get_needed;
    static constexpr auto get_stats = &dvbs2gpu_ule_get_stats;
    static constexpr auto get_row_table = &dvbs2gpu_ule_get_row_table;
};
struct T2miApi {
    typedef dvbs2gpu_t2mi Handle; typedef dvbs2gpu_t2mi_stats Stats; typedef dvbs2gpu_t2mi_row Row;
    static constexpr const char* name = "T2miBank";
    static constexpr auto create = &dvbs2gpu_t2mi_create, create_host = &dvbs2gpu_t2mi_create_host;
    static constexpr auto destroy = &dvbs2gpu_t2mi_destroy;
    static constexpr auto reset = &dvbs2gpu_t2mi_reset;
    static constexpr auto work = &dvbs2gpu_t2mi_work;
    static constexpr auto get_needed = &dvbs2gpu_t2mi_get_needed;
    static constexpr auto get_stats = &dvbs2gpu_t2mi_get_stats;
    static constexpr auto get_row_table = &dvbs2gpu_t2mi_get_row_table;
};
}   // namespace detail
/* T2-MI bank for one transport stream (dvbs2gpu_t2mi_*, include/dvbs2gpu.h; an extension): the T2-MI packets of a PID behind
 * BBFrameTSParser or TSMonitor are reassembled and checked, and the DVB-T2 BBFRAMEs of the chosen PLP laid back to back for a second
 * BBFrameTSParser in mode-adaptation mode (feed()).  Four slots, each a (PID, PLP) pair and a reassembler of its own.  init() (a device
 * bank) or initHost() (the library's host implementation, no device) and the setters throw; work() sits in the data path and does NOT
 * throw: a failing call returns 0 and leaves its code in status() and its text in error(), sticky until clearStatus(). */
class T2miBank : public detail::DatagramBank<detail::T2miApi> {
public:
    /* slot 0..3; pid -1 empties the slot; plp -1: every PLP.  The same PID may sit in several slots. */
    void setWatch(int slot, int pid, int plp = -1) { check(dvbs2gpu_t2mi_set_watch(need(), 0, slot, pid, plp)); }
    /* the sizes of the BBFRAMEs that the slot's last work() delivered, in order */
    std::vector<int> frameBytes(int slot) {
        int n = 0;
        check(dvbs2gpu_t2mi_get_frame_bytes(need(), 0, slot, nullptr, 0, &n));
        std::vector<int> sizes((size_t)n);
        if (n > 0) check(dvbs2gpu_t2mi_get_frame_bytes(h, 0, slot, sizes.data(), n, &n));
        return sizes;
    }
    /* the BBFRAMEs that the slot's last work() wrote to `bbframes` into the mode-adaptation work() of `parser` (after its
     * setFrameSize() and setModeAdaptation()): tsframes[8], out_bytes[8], needed[8] as there; false: buffer_outsize was too small */
    bool feed(int slot, dvbs2::BBFrameTSParser& parser, uint8_t* bbframes, uint8_t* const* tsframes, int buffer_outsize, int* out_bytes, int* needed8 = nullptr) {
        const std::vector<int> sizes = frameBytes(slot);
        return parser.work(bbframes, sizes.data(), (int)sizes.size(), tsframes, buffer_outsize, out_bytes, needed8);
    }
};
/* MPE bank for one transport stream (dvbs2gpu_mpe_*, include/dvbs2gpu.h; an extension): the DSM-CC datagram_sections of a PID behind
 * BBFrameTSParser or TSMonitor are reassembled and checked and their IP datagrams laid back to back.  Four slots, each a (PID, MAC
 * value, MAC mask) and a reassembler of its own.  init() (a device bank) or initHost() (the library's host implementation, no device)
 * and the setters throw; work() sits in the data path and does NOT throw: a failing call returns 0 and leaves its code in status() and
 * its text in error(), sticky until clearStatus(). */
class MpeBank : public detail::DatagramBank<detail::MpeApi> {
public:
    /* slot 0..3; pid -1 empties the slot; mac_value / mac_mask: six bytes each in network order, nullptr: all zero (every address).
     * The same PID may sit in several slots. */
    void setWatch(int slot, int pid, const uint8_t* mac_value = nullptr, const uint8_t* mac_mask = nullptr) {
        check(dvbs2gpu_mpe_set_watch(need(), 0, slot, pid, mac_value, mac_mask));
    }
};
/* ULE bank for one transport stream (dvbs2gpu_ule_*, include/dvbs2gpu.h; an extension): the ULE SNDUs (RFC 4326) of a PID behind
 * BBFrameTSParser or TSMonitor are reassembled and checked and their IP datagrams laid back to back.  Four slots, each a (PID, NPA
 * value, NPA mask, accept_unaddressed) and a reassembler of its own.  init() (a device bank) or initHost() (the library's host
 * implementation, no device) and the setters throw; work() sits in the data path and does NOT throw: a failing call returns 0 and
 * leaves its code in status() and its text in error(), sticky until clearStatus(). */
class UleBank : public detail::DatagramBank<detail::UleApi> {
public:
    /* slot 0..3; pid -1 empties the slot; npa_value / npa_mask: six bytes each, nullptr: all zero (every address); accept_unaddressed:
     * SNDUs without a destination address pass.  The same PID may sit in several slots. */
    void setWatch(int slot, int pid, const uint8_t* npa_value = nullptr, const uint8_t* npa_mask = nullptr, bool accept_unaddressed = false) {
        check(dvbs2gpu_ule_set_watch(need(), 0, slot, pid, npa_value, npa_mask, accept_unaddressed ? 1 : 0));
    }
};
/* IP-TS bank for one stream (dvbs2gpu_ipts_*, include/dvbs2gpu.h; an extension): the UDP / RTP datagrams of up to four flows among the
 * IP datagrams that MpeBank::work or UleBank::work delivered (or a GSE path's GRE packets) are checked and their TS packets laid back to
 * back per flow slot, for TSMonitor and the banks behind it.  init() (a device bank) or initHost() (the library's host implementation,
 * no device) and the setters throw; work() sits in the data path and does NOT throw: a failing call returns false and leaves its code
 * in status() and its text in error(), sticky until clearStatus(). */
class IpTsBank : public detail::Bank<detail::IptsApi> {
public:
    void init(int max_rows, int device = 0) {
        release();
        eng = Engine::get(device);
        check(dvbs2gpu_ipts_create(eng->ctx, 1, max_rows, &h));
    }
    void initHost(int max_rows) {
        release();
        check(dvbs2gpu_ipts_create_host(1, max_rows, &h));
    }
    void reset() { check(dvbs2gpu_ipts_reset(need())); }
    /* slot 0..3; family 4 or 6 with the destination address (sixteen bytes, an IPv4 address in the first four) and UDP port; family 0
     * empties the slot.  The slot's counters and RTP state start afresh. */
    void setFlow(int slot, int family, const uint8_t* dst_addr = nullptr, int dst_port = 0) { check(dvbs2gpu_ipts_set_flow(need(), 0, slot, family, dst_addr, dst_port)); }
    /* The view of the rows of a bank's last work() over the host buffer that call filled: Row is dvbs2gpu_mpe_row, dvbs2gpu_ule_row
     * (kind RAW_IP) or dvbs2gpu_gse_pdu (kind GRE).  `rows` must outlive the work() call that takes the view. */
    template <typename Row>
    static dvbs2gpu_ipts_view view(const uint8_t* bytes, const std::vector<Row>& rows, int kind = DVBS2GPU_IPTS_KIND_RAW_IP) {
        return dvbs2gpu_ipts_view{rows.empty() ? nullptr : bytes, rows.empty() ? nullptr : rows.data(), (int32_t)sizeof(Row), (int32_t)offsetof(Row, offset),
                                  (int32_t)offsetof(Row, bytes), kind, (int32_t)rows.size(), 0};
    }
    /* ts[k] (buffer_outsize bytes each; nullptr for a slot without a flow; ts == nullptr: rows and counters only) receives the TS
     * packets of slot k, bytes[k] (may be nullptr) their byte counts; false on failure (see status(); on DVBS2GPU_ERR_CAPACITY
     * needed() has the sizes and nothing was consumed) */
    bool work(const dvbs2gpu_ipts_view& v, uint8_t* const ts[4], int buffer_outsize, int bytes[4]) noexcept {
        const int rc = h ? dvbs2gpu_ipts_work(h, 0, &v, ts, buffer_outsize, bytes) : DVBS2GPU_ERR_ARG;
        return rc >= 0 || fail(rc);
    }
    /* the bytes that the slot's last work() needed */
    int needed(int slot) {
        int b = 0;
        check(dvbs2gpu_ipts_get_needed(need(), 0, slot, &b));
        return b;
    }
    /* a slot's counters; -1: the stream's own and the sum over its slots */
    dvbs2gpu_ipts_stats stats(int slot = -1) {
        dvbs2gpu_ipts_stats s;
        check(dvbs2gpu_ipts_get_stats(need(), 0, slot, &s));
        return s;
    }
    /* one row per input row of the last work(), in row order */
    std::vector<dvbs2gpu_ipts_row> rowTable() {
        int n = 0;
        check(dvbs2gpu_ipts_get_row_table(need(), 0, nullptr, 0, &n));
        std::vector<dvbs2gpu_ipts_row> rows((size_t)n);
        if (n > 0) check(dvbs2gpu_ipts_get_row_table(h, 0, rows.data(), n, &n));
        return rows;
    }
};
/* IP output bank for one transport stream (dvbs2gpu_ipout_*, include/dvbs2gpu.h; an extension): a block behind TSMonitor's filter or any
 * TS source; the packets of up to four flows leave as UDP or RTP/MP2T datagrams with complete headers, back to back per flow slot, one
 * row each -- IpTsBank::view() over rowTable() reads them back.  init() (a device bank) or initHost() (the library's host
 * implementation, no device) and the setters throw; work() sits in the data path and does NOT throw: a failing call returns false and
 * leaves its code in status() and its text in error(), sticky until clearStatus(). */
class IpOutBank : public detail::Bank<detail::IpoutApi> {
public:
    void init(int max_packets, int device = 0) {
        release();
        eng = Engine::get(device);
        check(dvbs2gpu_ipout_create(eng->ctx, 1, max_packets, &h));
    }
    void initHost(int max_packets) {
        release();
        check(dvbs2gpu_ipout_create_host(1, max_packets, &h));
    }
    void reset() { check(dvbs2gpu_ipout_reset(need())); }
    /* slot 0..3; flow.family 0 empties the slot; pids: the list of pid_mode 1 and 2.  The slot's counters, held packets and sequence
     * start afresh. */
    void setFlow(int slot, const dvbs2gpu_ipout_flow& flow, const std::vector<uint16_t>& pids = {}) {
        check(dvbs2gpu_ipout_set_flow(need(), 0, slot, &flow, pids.data(), (int)pids.size()));
    }
    /* 27 MHz ticks per packet in Q24.24, the quantity of PCRBank's rate; 0: not set */
    void setRate(uint64_t ticks_per_packet_q24) { check(dvbs2gpu_ipout_set_rate(need(), 0, ticks_per_packet_q24)); }
    /* out[k] (buffer_outsize bytes each; nullptr for a slot without a flow) receives the datagrams of slot k, bytes[k] (may be nullptr)
     * their byte counts; false on failure (see status(); on DVBS2GPU_ERR_CAPACITY needed() has the sizes and nothing was consumed) */
    bool work(const uint8_t* ts, int nbytes, uint8_t* const out[4], int buffer_outsize, int bytes[4], bool flush = false) noexcept {
        const int rc = h ? dvbs2gpu_ipout_work(h, 0, ts, nbytes, out, buffer_outsize, bytes, flush ? 1 : 0) : DVBS2GPU_ERR_ARG;
        return rc >= 0 || fail(rc);
    }
    /* the bytes that the slot's last work() needed */
    int needed(int slot) {
        int b = 0;
        check(dvbs2gpu_ipout_get_needed(need(), 0, slot, &b));
        return b;
    }
    /* a slot's counters; -1: the stream's own and the sum over its slots */
    dvbs2gpu_ipout_stats stats(int slot = -1) {
        dvbs2gpu_ipout_stats s;
        check(dvbs2gpu_ipout_get_stats(need(), 0, slot, &s));
        return s;
    }
    /* one row per datagram of the slot's last work(), in output order */
    std::vector<dvbs2gpu_ipout_row> rowTable(int slot) {
        int n = 0;
        check(dvbs2gpu_ipout_get_row_table(need(), 0, slot, nullptr, 0, &n));
        std::vector<dvbs2gpu_ipout_row> rows((size_t)n);
        if (n > 0) check(dvbs2gpu_ipout_get_row_table(h, 0, slot, rows.data(), n, &n));
        return rows;
    }
};
}   // namespace dvbs2gpu_host
#endif
