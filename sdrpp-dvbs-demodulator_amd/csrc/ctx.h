// Engine context internals shared by capi.hip (FEC entry points) and s2_demod.hip (demodulator handles).
#pragma once
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstring>
#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <vector>
#include "../../include/dvbs2gpu.h"
#include "s2_params.h"
#include "ldpc_plan.h"
#include "ldpc_wave_plan.h"
#include "ldpc_split_plan.h"
#include <chrono>
#include "kernels.h"
#include "s2_rx.h"
#include "scratch_layout.h"
#include "rx_cfg_rules.h"
#include "dev_buf.h"
#include "s2_tx.h"
#include <type_traits>

namespace s2 {

std::string& last_error();
int fail_hip(hipError_t e, const char* what);
#define HIP_TRY(x)                                            \
    do {                                                      \
        hipError_t _e = (x);                                  \
        if (_e != hipSuccess) return s2::fail_hip(_e, #x);    \
    } while (0)
#define RC_TRY(x)                                             \
    do {                                                      \
        int _rc = (x);                                        \
        if (_rc) return _rc;                                  \
    } while (0)

// the table `v` on the device, held by `own` (an empty table still gets one element's worth, so the pointer is never null)
template <typename T>
inline int upload(const std::vector<T>& v, DevBuf<T>& own) {
    int rc = own.alloc(v.empty() ? 1 : v.size(), false, "hipMalloc(table)");
    if (rc) return rc;
    if (!v.empty()) HIP_TRY(hipMemcpy(own.get(), v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice));
    return 0;
}
// ... and `*view`, the raw pointer of a struct that a kernel reads, set to it
template <typename T, typename U>
inline int upload(const std::vector<T>& v, DevBuf<T>& own, U** view) {
    const int rc = upload(v, own);
    *view = own.get();
    return rc;
}

// Per-stage device times (hipEvent pairs on the stream a stage is enqueued on), accumulated until dvbs2gpu_get_stage_times reads them.
enum StageId { ST_FRONTEND = 0, ST_RRC, ST_PLSYNC, ST_LOOPS, ST_DEMAP, ST_LDPC, ST_BCH, ST_DELIVER, ST_COUNT };
struct StageTimers {
    bool on = false;
    std::mutex mtx;
    struct Span { int stage; hipEvent_t a, b; long units; };
    std::vector<Span> pending;
    std::vector<hipEvent_t> pool;
    double ms[ST_COUNT] = {};
    long launches[ST_COUNT] = {}, units[ST_COUNT] = {};
    hipEvent_t get() {
        if (!pool.empty()) { hipEvent_t e = pool.back(); pool.pop_back(); return e; }
        hipEvent_t e = nullptr;
        (void)hipEventCreate(&e);
        return e;
    }
};
// RAII span: records an event on `st` now and another when it goes out of scope (no-op while timing is off)
struct StageSpan {
    StageTimers* T; int stage; hipStream_t st; hipEvent_t a = nullptr; long units;
    StageSpan(StageTimers& t, int stage_, hipStream_t st_, long units_ = 0) : T(&t), stage(stage_), st(st_), units(units_) {
        if (!T->on) { T = nullptr; return; }
        { std::lock_guard<std::mutex> l(T->mtx); a = T->get(); }
        if (a) (void)hipEventRecord(a, st);
    }
    ~StageSpan() {
        if (!T || !a) return;
        std::lock_guard<std::mutex> l(T->mtx);
        hipEvent_t b = T->get();
        if (b) { (void)hipEventRecord(b, st); T->pending.push_back({stage, a, b, units}); }
    }
};

// the FEC stage's scratch buffers: one set per context, and one per configuration group for jobs that run side by side (s2_demod.hip)
struct FecWs { Workspace msg, hard, syn, misc; };
// per-call scratch of the S2 batch flows (s2_demod.hip), one struct per flow.  `deliver`: the destination table of a job's delivery
struct GroupWs {        // a CCM group (process_group)
    Workspace work,     // stream-work table + first[] + symbol counts + NCO + FIFO cur/fill
              found,    // PL-sync frame tables + counts
              frames,   // frame refs + stats + trials + corrections + slot indices
              pll, llr, bb, deliver,
              slot_stats,   // stage pipeline: per-slot frame stats
              quality;      // signal-quality descriptors + records (quality.hip)
};
// the buffers of one FEC job: LLRs | BBFRAMEs | frame refs + first[] + results (a CCM group's job), results + index list + destination table (a job in
// parts, fec_parts.h: ACM/VCM, mixed).  One set per slot and parity for the jobs of the throughput mode; a job in parts of a synchronous call uses its flow's own set
struct FecJobBufs { Workspace llr, bb, job; };
struct VcmWs {          // a group of ACM/VCM streams (process_vcm_group)
    Workspace work,     // stream-work table + first[] + counts + FIFO cur/fill + symbol counts + NCO
              found, frames /* frames + stats */, pll, llr, deliver, quality;
    FecJobBufs fec;     // the synchronous call's job
};
struct MixWs {          // a mixed CCM batch (process_mixed)
    Workspace work,     // stream-work table + per-stream configurations + symbol counts + NCO + FIFO cur/fill
              found, llr_of /* per-frame LLR pointers + slot indices */, pll, slot_stats, deliver, quality;
    FecJobBufs fec;     // the synchronous call's job
};

// the argument table of a bank call for n streams (dvbs_capi.hip, bbts.hip): input pointers | output pointers | counts in | bytes out
struct BankArgs {
    ScratchLayout L;
    ScratchPart<const uint8_t*> in; ScratchPart<uint8_t*> out; ScratchPart<int> cnt, ob;
    explicit BankArgs(size_t n) : in(L.add<const uint8_t*>(n)), out(L.add<uint8_t*>(n)), cnt(L.add<int>(n)), ob(L.add<int>(n)) {}
};

// What a kernel reads is a plain struct of raw pointers, passed by value or copied to the device; the context's caches hold it together
// with the owners of the tables it points to (a launch takes the plain part: `*C` slices to it).
static_assert(std::is_trivially_copyable_v<LdpcDeviceCode> && std::is_trivially_copyable_v<BchDeviceCode> && std::is_trivially_copyable_v<FecEncDeviceCode>, "kernel-visible structs stay plain");
static_assert(std::is_trivially_copyable_v<S2ConstelDev> && std::is_trivially_copyable_v<S2PlTablesDev>, "kernel-visible structs stay plain");
struct LdpcCode : LdpcDeviceCode {
    DevBuf<LdpcLayerDesc> layers;
    DevBuf<uint32_t> ents, rows, atab, wave_lanec, wave_layer_end, split_atab;
    DevBuf<uint16_t> wave_steps;
    DevBuf<LdpcSplitLayer> split_layers;
};
struct BchCode : BchDeviceCode { DevBuf<uint16_t> log, exp, imap, syn_tab; };
struct FecEncCode : FecEncDeviceCode { DevBuf<uint32_t> byte_tab, rows, layer_off, ent; };     // the encoder's tables of one code (fec_encode_rules.h)
struct ConstelTables {          // device tables of one constellation (type, gamma1, gamma2)
    S2ConstelDev dev;
    DevBuf<int8_t> bits;
    DevBuf<uint32_t> bits4;
    DevBuf<float> err;
    DevBuf<cf32> pts;
};
struct PlTables : S2PlTablesDev {       // PL header tables (s2_demod.hip: get_rx_tables)
    DevBuf<cf32> sof_own, plsc_own;
    DevBuf<uint64_t> plsc_code_own;
    DevBuf<uint8_t> rn_own;
};

}  // namespace s2

struct dvbs2gpu_ctx {
    int device = 0;
    int num_cus = 256;
    std::mutex mtx;                           // table caches (creation of LDPC / BCH / constellation / tap tables)
    // One context may serve several handles and host threads (include/dvbs2gpu_host.hpp shares one per device between all blocks of
    // the process), and every entry point below works in the context-wide workspaces (ws_*): whole calls are serialised by
    // call_mtx (recursive: the segment receivers call process_batch from inside their own entry point).  The asynchronous stage
    // entry points only ENQUEUE under the lock; ev_ws, recorded behind the last enqueued user of the shared FEC workspaces, makes a
    // later user on a different stream wait for the earlier one (the message records and the LDPC work counter live there).
    s2::StageTimers timers;
    std::recursive_mutex call_mtx;
    hipEvent_t ev_ws = nullptr;
    hipStream_t ws_stream = nullptr;
    bool ws_used = false;
    std::map<int, s2::LdpcCode> ldpc;         // by code_index
    std::map<int, s2::BchCode> bch;           // by m*100 + t
    s2::DevBuf<uint8_t> d_prbs;               // BB scrambler sequence, 8100 bytes
    s2::FecWs fws;                            // LDPC message records (+ work counter, sign scratch), hard decisions, BCH syndromes, trial counts
    // receive-chain tables (s2_demod.hip)
    s2::DevBuf<float> d_gardner_bank;
    s2::PlTables pl{};
    std::map<int, s2::ConstelTables> constel; // by modcod (gammas depend on it)
    std::map<s2::rxcfg::RrcKey, s2::DevBuf<float>> rrc;   // by the exact (ntaps, alpha, Ts) of make_rrc_taps (rx_cfg_rules.h)
    // (ws_rx.slot_stats also holds frontend_prepass's work table -- a pre-passed group is never staged; ws_rx.deliver also collects the jobs left in slots without a group)
    s2::GroupWs ws_rx;
    // ACM/VCM mode (s2_demod.hip): what every PLS code means + the constellations it points to, on the device; per-call scratch
    s2::DevBuf<s2::S2VcmMod> d_vcm_mods;
    s2::DevBuf<s2::S2ConstelDev> d_vcm_cons;
    std::vector<s2::S2VcmMod> h_vcm_mods;
    std::vector<s2::FecParams> h_vcm_fec;     // by PLS code
    s2::VcmWs ws_vcm;
    // mixed CCM batches through one launch per stage (s2_demod.hip, process_mixed): per-call scratch, and per FEC side stream and job parity the event behind its jobs
    s2::MixWs ws_mix;
    static constexpr int MIX_FEC_STREAMS = 4;           // side streams (grp_stream[0..3]) of process_mixed's FEC parts
    hipEvent_t ev_mix[MIX_FEC_STREAMS][2] = {};
    // pipelined FEC (s2_demod.hip): with pipeline_fec set, dvbs2gpu_demod_process_batch runs the FEC of call k on fec_stream
    // while call k+1's front end runs on fe_stream; BBFRAMEs of call k are delivered by call k+1
    int pipeline_fec = 0;
    hipStream_t fe_stream = nullptr, fec_stream = nullptr;
    hipEvent_t ev_llr = nullptr;
    hipEvent_t ev_in = nullptr;               // throughput mode: the call's own stream starts behind what the host has put on the legacy null stream (its input buffers)
    // one slot per configuration group of the batch (groups are formed in order of first appearance, so a slot keeps its
    // streams from call to call): the job in flight, its buffers (double-buffered) and the event that marks its completion
    static constexpr int MAX_PIPE_GROUPS = 16;
    void* pending_fec[MAX_PIPE_GROUPS] = {};              // s2::PendingFec*
    s2::FecJobBufs ws_fecbuf[MAX_PIPE_GROUPS][2];         // per parity
    int fec_parity[MAX_PIPE_GROUPS] = {};
    // what the bench's self-check reads back (dvbs2gpu_debug_last_fec_job): the pipelined CCM job a slot delivered last -- its LLR and BBFRAME buffers stay untouched until the
    // slot's next job of the same parity is started
    struct LastFecJob { const int8_t* d_llr = nullptr; const uint8_t* d_bb = nullptr; int nf = 0, n = 0, N = 0, kb = 0, rate = -1, shortframe = 0, max_trials = 0, force = 0; std::vector<int> first; std::vector<const void*> dm; };
    LastFecJob last_fec[MAX_PIPE_GROUPS];
    bool last_call_staged = false;            // the last CCM batch ran its post stages behind every front-end slice (the stage pipeline)
    hipEvent_t ev_fec[MAX_PIPE_GROUPS][2] = {};   // end of a group's FEC job, per job parity (the next job is enqueued before the previous one is delivered)
    hipEvent_t ev_fec_t0[MAX_PIPE_GROUPS][2] = {};   // ... and its start (timing events: the job's duration feeds the priority balancer)
    std::chrono::steady_clock::time_point fec_last_entry{};
    // several groups of one pipelined batch run their MODCOD-dependent stages side by side (one host thread and HIP stream each)
    s2::GroupWs ws_grp[MAX_PIPE_GROUPS];
    hipStream_t grp_stream[MAX_PIPE_GROUPS] = {};
    hipEvent_t ev_llr_grp[MAX_PIPE_GROUPS] = {};
    std::mutex fec_mtx;                                   // FEC jobs on the shared stream are enqueued whole, one at a time (shared FEC workspaces)
    // FEC jobs too small to fill the device (a group of a 64-transponder batch: a handful of decoder workgroups, 4-6 ms of latency each) run
    // SIDE BY SIDE instead: on the group's own stream (grp_stream) with a set of FEC workspaces per group
    s2::FecWs fws_grp[MAX_PIPE_GROUPS];
    // time-sliced front end (s2_rx_kernels.hip, s2_frontend_launch): per main stream one auxiliary stream + the slice events
    struct FeAux {      // (dvbs_*: the DVB-S receiver's stage streams: AGC, FLL, RRC, soft FIFO + Viterbi)
        hipStream_t aux = nullptr, aux2 = nullptr, aux3 = nullptr;
        hipEvent_t ev[s2::S2_FE_MAX_SLICES + 1] = {}, ev2[s2::S2_FE_MAX_SLICES + 1] = {}, ev3[2 * (s2::S2_FE_MAX_SLICES + 1)] = {};
        hipStream_t dvbs_aux[4] = {};
        hipEvent_t dvbs_ev[4][s2::DVBS_FE_MAX_SLICES + 1] = {};
        void release() {    // destroys the streams and events (the entry is dropped afterwards)
            for (hipStream_t s : {aux, aux2, aux3}) if (s) (void)hipStreamDestroy(s);
            for (hipEvent_t e : ev) if (e) (void)hipEventDestroy(e);
            for (hipEvent_t e : ev2) if (e) (void)hipEventDestroy(e);
            for (hipEvent_t e : ev3) if (e) (void)hipEventDestroy(e);
            for (hipStream_t s : dvbs_aux) if (s) (void)hipStreamDestroy(s);
            for (auto& row : dvbs_ev) for (hipEvent_t e : row) if (e) (void)hipEventDestroy(e);
        }
    };
    std::map<hipStream_t, FeAux> fe_aux;
    // development / test options (dvbs2gpu_set_option, or DVBS2GPU_OPTIONS="name=value,..." in the environment when the context is created)
    int gardner_form = 0;                     // 2 / 4: one form of the timing recovery (0: chosen by bank size)
    int gardner_cand_skew = 0;                // tests only: skews the candidate form's arm prediction so that it leaves its tables
    int ldpc_wave = -1;                       // short frames: 0 / 1 = lane-per-row / wave-per-frame decoder (-1: per code)
    int ldpc_split_fail_attempts = 0;         // tests only: every attempt of the half-row decoder's layers with shared bits is made to fail (ldpc_split_kernel.hip: the long way must give the same bits)
    int ldpc_split = 1;                       // 1: the half-row decoder for the normal frames it takes (ldpc_split_kernel.hip); 0: the lane-per-row decoder for every code
    int host_timing = 0;                      // 1: print where the host spends a batch call
    int stage_pipeline_launches = 0;          // option stage_loops: frame-loop launches per call (0 = chosen per call, s2_demod.hip)
    int stage_pipeline_min_duty = 2;          // option stage_min_duty: pipelined mode uses the stage pipeline only above this balancer setting (-1: always).
                                              // 2: with the frame loops at the decoder's base priority the two streams of a headline step are 6 ms apart, a stray
                                              // verdict of the balancer must not tip the step into the other flow (which costs it 3 %)
    unsigned stage_calls = 0;
    int stage_pipeline = 1;                   // option stage_pipeline: RRC, PL-sync walk and frame loops of a CCM call behind every timing-recovery slice (0: after the last one, frames pooled by the host first)
    int fe_slices = 0;                        // option fe_slices (0 = by mode: 4 pipelined, 8 synchronous; 1 = both stages back to back on the caller's stream)
    // balance of the two streams of the pipelined mode (s2_demod.hip): share of the timing loop's tiles that run one priority level up
    int g_prio_duty = 0, g_prio_trend = 0;
    int g_prio_hold = 0, g_prio_last_down = 0;      // the balancer's damper: calls during which no step down is tried / calls since the last step down (s2_demod.hip)
    long long g_prio_sig = -1;                // what the balance was found for (streams, MODCOD, frame kind, iteration setting of the batch): another configuration starts from 0 again
    bool g_prio_auto = true;                  // option g_prio_duty fixes the value
    int dvbs_bank_min = 2048;                 // option dvbs_bank_min: carriers from which a bank uses the four-streams-per-wave FLL (measured crossover with the written-out wave-per-stream loop: 2048 carriers 74.2 vs 74.8 ms, 1024: 46.2 vs 54.8, 4096: 128.8 vs 111.4; tests: 1)
    int dvbs_agc_stream = 1;                  // option dvbs_agc_stream: the AGC slices of a bank below dvbs_bank_min carriers on a third auxiliary stream (0: on the Viterbi stream)
    int dvbs_fe_slices = 24;                 // option dvbs_fe_slices: time slices of a DVB-S call (dvbs_demod.hip)
    // DVB-S front end (dvbs_demod.hip)
    s2::DevBuf<float> d_fd_bank;              // COMPLEX_FD interpolator bank, 256 x 256
    std::map<int, s2::DevBuf<s2::cf32>> bandedge;    // FLL band-edge taps [2][ntaps] by ntaps*100000 + round(alpha*1000)*10 + sps
    s2::Workspace ws_dvbs[4];
    // FEC encoder (fec_encode.hip): the tables of a code, by code_index
    std::map<int, s2::FecEncCode> fec_enc;
    // modulator (s2_tx.hip): constellation tables, the buffers of dvbs2gpu_s2_modulate_batch, the channel's table
    s2::TxState tx;
};

namespace s2 {
// serialises an entry point on its context; stage_* additionally order the shared FEC workspaces across streams
struct CallGuard {
    std::unique_lock<std::recursive_mutex> l;
    explicit CallGuard(dvbs2gpu_ctx* ctx) : l(ctx->call_mtx) {}
};
int ws_acquire(dvbs2gpu_ctx* ctx, hipStream_t st);   // before enqueuing work that uses the context's FEC workspaces (ctx->fws) on `st`
int ws_release(dvbs2gpu_ctx* ctx, hipStream_t st);   // after it
int ws_quiesce(dvbs2gpu_ctx* ctx);                   // host-side wait for the last asynchronous user (synchronous entry points)
bool fec_jobs_pending(dvbs2gpu_ctx* ctx);
int apply_option(dvbs2gpu_ctx* ctx, const char* name, int value);   // 0, or -1: unknown name / value out of range
int get_ldpc(dvbs2gpu_ctx* ctx, int code_index, LdpcDeviceCode** out);
int get_bch(dvbs2gpu_ctx* ctx, int m, int t, BchDeviceCode** out);
int get_prbs(dvbs2gpu_ctx* ctx);
int get_fec_enc(dvbs2gpu_ctx* ctx, const FecParams& f, FecEncDeviceCode** out);
// LLR -> BBFRAME for nframes frames of one code; all pointers device
std::vector<float> make_polyphase_bank(int phases, int taps_per_phase);
int get_rx_tables(dvbs2gpu_ctx* ctx);                // ctx->pl (and the timing recovery's bank), built on first use
int get_rrc(dvbs2gpu_ctx* ctx, int ntaps, float alpha, double Ts, float** out);
void critically_damped(float bw, float* alpha, float* beta);
int fec_run(dvbs2gpu_ctx* ctx, const FecParams& f, const int8_t* d_llr, int nframes, int max_trials, int force, uint8_t* d_bbframes,
            int32_t* d_trials, int32_t* d_corr, hipStream_t st, FecWs* ws = nullptr);     // ws: the FEC workspaces to use (null: the context's own set)
}  // namespace s2
