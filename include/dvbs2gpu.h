/*
 * dvbs2gpu -- C ABI of the MI355X (gfx950) DVB-S / DVB-S2 demodulation + FEC engine.
 *
 * This is the drop-in boundary for the hot path of cropinghigh/sdrpp-dvbs-demodulator: the SDR++ plugin
 * shell (src/main.cpp) stays host C++; the bodies of
 *     int DVBS2Demod::process(int count, const complex_t* in, uint8_t* out)   src/demod/dvbs2/module_dvbs2_demod.cpp:216
 *     int DVBSDemod::process(int count, const complex_t* in, uint8_t* out)    src/demod/dvbs/module_dvbs_demod.cpp:78
 * and every stage they call are replaced by the entry points below.  Plain C types only, no exceptions
 * cross this boundary (the reference throws std::runtime_error for a bad MODCOD, modcod_to_cfg.cpp:11,135;
 * here that is DVBS2GPU_ERR_MODCOD).
 *
 * Pointer convention: arguments named d_* are DEVICE pointers (hipMalloc / torch CUDA tensors); h_* are
 * host pointers.  `stream` is a hipStream_t passed as void* (NULL = default stream).  Batch entry points
 * enqueue work on the stream and return without synchronising unless stated otherwise.
 *
 * Every function returns 0 (or a non-negative count) on success and a negative DVBS2GPU_ERR_* code on error.
 */
#ifndef DVBS2GPU_H
#define DVBS2GPU_H

#include <stdint.h>
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DVBS2GPU_OK 0
#define DVBS2GPU_ERR_ARG (-1)      /* null pointer / bad size */
#define DVBS2GPU_ERR_MODCOD (-2)   /* MODCOD <= 0, >= 29, or short-frame 9/10 (does not exist) */
#define DVBS2GPU_ERR_HIP (-3)      /* a HIP call failed; dvbs2gpu_last_error() has the text */
#define DVBS2GPU_ERR_NODEVICE (-4) /* no gfx950 device visible: the engine has no CPU fallback */
#define DVBS2GPU_ERR_CAPACITY (-5) /* output buffer too small */

/* code rate index used throughout: 0=1/4 1=1/3 2=2/5 3=1/2 4=3/5 5=2/3 6=3/4 7=4/5 8=5/6 9=8/9 10=9/10 */

typedef struct dvbs2gpu_ctx dvbs2gpu_ctx;   /* one per device / host thread; owns tables + workspaces */

const char* dvbs2gpu_version(void);
const char* dvbs2gpu_last_error(void);
/* Optional, for hosts that want the engine's HIP streams on hardware queues of their own: sets GPU_MAX_HW_QUEUES=12 in the process environment unless the
 * variable is already there.  The HIP runtime reads it at the process's first HIP call, so call this BEFORE that call and before starting threads (setenv is
 * not thread-safe); loading the library changes nothing by itself.  Returns 1 = set, 0 = already present.  No reference counterpart. */
int dvbs2gpu_preinit(void);

/* Create a context on HIP device `device`.  Fails with DVBS2GPU_ERR_NODEVICE when no GPU is present. */
int dvbs2gpu_create(int device, dvbs2gpu_ctx** out);
/* HIP devices visible to the process (0: none -- there is no CPU fallback); what a multi-GPU host sizes its fleet with */
int dvbs2gpu_device_count(void);
void dvbs2gpu_destroy(dvbs2gpu_ctx* ctx);
/* Development / test options of a context (which of several bit-identical flows runs, time slicing, side streams ...; DESIGN.md section 11 lists them).  The same
 * pairs can be given as DVBS2GPU_OPTIONS="name=value,name=value" in the environment when the context is created -- the one variable the library reads.  Options that
 * choose a decoder plan (ldpc_wave, ldpc_split) must be set before the first frame of the code is decoded.  The reference has no counterpart (its behaviour is the default). */
int dvbs2gpu_set_option(dvbs2gpu_ctx* ctx, const char* name, int value);
/* Read-only introspection (no reference counterpart; bench.py records the run-time balancer's final state and the launches a drop-in call costs with it).
 * Names: "kernel_launches" (kernel launches of the whole library in this process so far), "g_prio_duty" / "g_prio_auto" / "g_prio_hold" (the pipelined mode's priority
 * share of the timing loop, whether it is balanced at run time, calls the balancer still rests), "stage_pipeline_on" (the last CCM batch ran its post stages behind
 * every front-end slice), "pipelined", "num_cus", "engine_streams" (HIP streams the context owns right now), "fec_part_on" (always 0: the FEC partition stream it reported is gone; kept because bench.py --full reads it). */
int dvbs2gpu_get_state(dvbs2gpu_ctx* ctx, const char* name, long long* value);
/* Test / bench aid: the pipelined CCM decoder job that configuration group `slot` (0 for a single-configuration batch) DELIVERED last -- what the decoder read and what it
 * wrote, still in place until the group starts another job of the same parity (two calls later).  out10 = {device pointer of the LLRs [nf][N] int8, device pointer of the
 * BBFRAMEs [nf][kb], nf frames, n streams, N, kb bytes per BBFRAME, code rate index, short frames, max_trials, forced}; h_first[n + 1]: first pooled frame of every stream
 * of the job; h_handles[n]: the streams' dvbs2gpu_demod handles (as the call that started the job listed them).  bench.py decodes sampled LLR frames with the CPU oracle
 * and compares them with the BBFRAMEs the engine delivered.  No reference counterpart. */
int dvbs2gpu_debug_last_fec_job(dvbs2gpu_ctx* ctx, int slot, long long* out10, int32_t* h_first, const void** h_handles, int cap);

/* Static parameter queries (no GPU needed).  Mirrors get_dvbs2_cfg (modcod_to_cfg.cpp:5-140),
 * BBFrameBCH::BBFrameBCH (bbframe_bch.cpp:39-161) and the PLFRAME size of dvbs2_pl_sync.cpp:14-31. */
typedef struct dvbs2gpu_modcod_info {
    int32_t constellation;   /* 0 QPSK, 1 8PSK, 2 16APSK, 3 32APSK */
    int32_t bits_per_symbol;
    int32_t rate;            /* code rate index */
    int32_t slots;           /* 90-symbol payload slots */
    int32_t pilot_blocks;
    int32_t plframe_symbols; /* 90 + 90*slots + 36*pilot_blocks */
    int32_t ldpc_n, ldpc_k;  /* codeword / information bits (ldpc_k = nbch) */
    int32_t kbch;            /* BBFRAME bits; output is kbch/8 bytes per frame (DVBS2Demod::getKBCH) */
    int32_t bch_t;
    int32_t ldpc_edges;      /* Tanner-graph edges (LINKS_TOTAL) */
    float g1, g2;
} dvbs2gpu_modcod_info;
int dvbs2gpu_modcod_info_get(int modcod, int shortframes, int pilots, dvbs2gpu_modcod_info* out);
int dvbs2gpu_fec_info_get(int rate, int shortframes, dvbs2gpu_modcod_info* out);

/* ------------------------------------------------------------------ FEC stages (DVB-S2)
 *
 * dvbs2gpu_ldpc_decode_batch  replaces  BBFrameLDPC::decode  (bbframe_ldpc.cpp:123-139), one call per
 * frame in the reference, here `nframes` frames per launch.
 *   d_llr     [nframes][N] int8, bit 1 <-> negative (module_dvbs2_demod.cpp:360)
 *   d_hard    [nframes][K/8] hard decisions of the K information bits, MSB first (the repack loop of
 *             module_dvbs2_demod.cpp:357-360), may be NULL
 *   d_post    [nframes][N] int8 posteriors in the reference's layout, may be NULL
 *   d_trials  [nframes] int32: iterations used, or -1 if not converged after max_trials
 *   force != 0: benchmark mode, no early exit, exactly max_trials iterations; trials = max_trials or -1.
 */
int dvbs2gpu_ldpc_decode_batch(dvbs2gpu_ctx* ctx, int rate, int shortframes, const int8_t* d_llr, int nframes,
                               int max_trials, int force, uint8_t* d_hard, int8_t* d_post, int32_t* d_trials, void* stream);

/* Introspection of the decoder plan of one code (for DESIGN.md / bench reporting):
 * out8 = {layers q, max row degree, message record dwords, sum of layer depths, resident workgroups per CU (both of the
 *         decoder that serves the code),
 *         CUs, Tanner edges, layers with intra-layer shared bits}. */
int dvbs2gpu_ldpc_plan_info(dvbs2gpu_ctx* ctx, int rate, int shortframes, int32_t* out8);

/* Which of the three LDPC decoder kernels serves the code under the context's options (bench / profile reporting):
 * 0 lane per row (ldpc_kernel.hip), 1 wave per frame (short frames, ldpc_wave_kernel.hip), 2 half a row per lane
 * (ldpc_split_kernel.hip).  All three restate layered_decoder.hh:46-74 and are bit-exact with each other. */
int dvbs2gpu_ldpc_decoder_form(dvbs2gpu_ctx* ctx, int rate, int shortframes);

/* Host-only dump of the decoder plan (no GPU needed; used by the CPU test-suite to check the intra-layer
 * ordering against the reference's sequential row order).  Call with NULL arrays to get the counts:
 * counts3 = {layers, link entries, per-row words}.  layers4: 4 uint32 per layer {first entry, degree,
 * depth | nc<<16, first row word}; ents: sp | r<<16; rows: level | late<<8 | early<<20 (ldpc_plan.h). */
int dvbs2gpu_ldpc_plan_dump(int rate, int shortframes, uint32_t* layers4, uint32_t* ents, uint32_t* rows, int32_t* counts3);
/* The same for the wave-per-frame decoder's plan (csrc/ldpc_wave_plan.h) and for the lane-per-row decoder's address table
 * (csrc/ldpc_plan.h; regular codes of degree 2, 8, 12, else empty).  NULL arrays: counts only.
 * counts6 = {link slots per lane LW, smallest row degree incl. parity links, steps per sweep, index of the absent masks inside
 * lanec, words in lanec, entries in steps}; lanec: [q][8][LW] thr | cA << 16, then [q][8] absent masks; steps: [..][8] row ids
 * (360 * layer + j, 0xffff = empty slot); layer_end: [q] chunk (4 steps) index at which a layer's steps end.
 * counts2 = {words in the table, words per row}; table: [q][384][words per row], two 16-bit byte offsets per word. */
int dvbs2gpu_ldpc_wave_plan_dump(int rate, int shortframes, uint32_t* lanec, uint16_t* steps, uint32_t* layer_end, int32_t* counts6);
int dvbs2gpu_ldpc_addr_table_dump(int rate, int shortframes, uint32_t* table, int32_t* counts2);
/* The half-row decoder's plan (csrc/ldpc_split_plan.h; codes it does not take: counts6[0] = 0, return value 0, and dvbs2gpu_last_error() says why -- irregular rows, a layer
 * with more than four shared links, ...).  A plan is listed for every code the PLAN takes; the decoder serves the normal frames of rates 1/4, 2/5, 1/2, 3/5, 2/3, 3/4
 * (dvbs2gpu_ldpc_decoder_form).
 * counts6 = {pseudo-layers, table words per thread, slots per row half, message-workspace dwords per workgroup, words in the table, record dwords};
 * layers4: 4 uint32 per pseudo-layer {kind | waves << 8 | flags, kind 1: chain step | steps << 16, kind 8: levels << 16, record offset, kind 1: first link entry, kind 8: word offset
 * of the layer's side entries in `table`}; table: [pseudo-layer][768][words] (two 16-bit LDS byte offsets per word, the row word behind the last slot), then the side entries of the
 * kind-8 layers [384 rows][2 words] (per shared slot: distance from the row's output cell back to the slot's source cell in bits 0..10, 0 = the bit itself; bit 15: a later row
 * of the layer touches the slot) -- `words in the table` counts both; row_of: [pseudo-layer][384] the row a lane pair updates (-1: idle);
 * layer_of: [pseudo-layer] its layer.  NULL arrays: counts only. */
int dvbs2gpu_ldpc_split_plan_dump(int rate, int shortframes, uint32_t* layers4, uint32_t* table, int32_t* row_of, int32_t* layer_of, int32_t* counts6);

/* Host-only dump of the physical-layer tables every receiver uploads (no GPU needed; the CPU test-suite compares them with what the
 * reference's s2_defs.h and s2_scrambling.cpp give): sof52 = the 26 SOF symbols (re, im), plsc_128x64x2 = the 64 symbols of each of the
 * 128 PLS codewords, codes128 = the codewords (bit 63 first), rn131072 = the Gold sequence of code number 0 as rotations 0..3.
 * NULL arrays are skipped. */
int dvbs2gpu_pl_tables_dump(float* sof52, float* plsc_128x64x2, uint64_t* codes128, uint8_t* rn131072);

/* replaces BBFrameBCH::decode (bbframe_bch.cpp:380-405).  d_frames [nframes][K/8] corrected in place;
 * d_corrections [nframes] int32: #bits corrected, 0 clean, -1 uncorrectable (frame left untouched). */
int dvbs2gpu_bch_decode_batch(dvbs2gpu_ctx* ctx, int rate, int shortframes, uint8_t* d_frames, int nframes,
                              int32_t* d_corrections, void* stream);

/* replaces BBFrameDescrambler::work + the copy of module_dvbs2_demod.cpp:364-366.
 * d_frames [nframes][K/8] -> d_out [nframes][kbch/8] */
int dvbs2gpu_bb_descramble_batch(dvbs2gpu_ctx* ctx, int rate, int shortframes, const uint8_t* d_frames, int nframes,
                                 uint8_t* d_out, void* stream);

/* LDPC -> repack -> BCH -> descramble for a batch (module_dvbs2_demod.cpp:349-366, with every frame
 * LDPC-decoded -- the reference only decodes SIMD lane 0).
 * d_bbframes [nframes][kbch/8]; d_trials, d_corrections [nframes] (either may be NULL). */
int dvbs2gpu_fec_decode_batch(dvbs2gpu_ctx* ctx, int rate, int shortframes, const int8_t* d_llr, int nframes,
                              int max_trials, int force, uint8_t* d_bbframes, int32_t* d_trials, int32_t* d_corrections,
                              void* stream);

/* ------------------------------------------------------------------ FEC encoder and per-frame channel BER
 * The transmit-side FEC of ETSI EN 302 307-1 on the device, stage by stage and as one call.  The reference has no usable counterpart (its
 * BBFrameLDPC::encode produces non-codewords for some rates), so each entry cites the clause of the standard it implements.  Frames are packed
 * bits, MSB first; a code word's bit order is the order dvbs2gpu_ldpc_decode_batch reads its d_llr in.  Errors: an unknown (rate, shortframes), a NULL
 * pointer, a negative frame count or a bad amplitude return DVBS2GPU_ERR_ARG with a dvbs2gpu_last_error() text, before anything is enqueued;
 * nframes == 0 succeeds without a launch. */

/* BB scrambling, clause 5.2.2: the inverse of dvbs2gpu_bb_descramble_batch (the same PRBS, XOR).
 * d_bbframes [nframes][kbch/8] -> d_out [nframes][K/8], the BCH parity area zeroed. */
int dvbs2gpu_bb_scramble_batch(dvbs2gpu_ctx* ctx, int rate, int shortframes, const uint8_t* d_bbframes, int nframes, uint8_t* d_out, void* stream);

/* BCH encoding, clause 5.3.1: the inverse of dvbs2gpu_bch_decode_batch.  d_frames [nframes][K/8]: the first kbch bits are the message,
 * the K - kbch parity bits m(x) x^(K - kbch) mod g(x) are written behind them in place. */
int dvbs2gpu_bch_encode_batch(dvbs2gpu_ctx* ctx, int rate, int shortframes, uint8_t* d_frames, int nframes, void* stream);

/* LDPC encoding, clause 5.3.2: the inverse of dvbs2gpu_ldpc_decode_batch's hard output.  d_info [nframes][K/8] -> d_code [nframes][N/8]:
 * the K information bits, then the parity bits. */
int dvbs2gpu_ldpc_encode_batch(dvbs2gpu_ctx* ctx, int rate, int shortframes, const uint8_t* d_info, int nframes, uint8_t* d_code, void* stream);

/* All three (clauses 5.2.2, 5.3.1, 5.3.2): the inverse of dvbs2gpu_fec_decode_batch.  d_bbframes [nframes][kbch/8] -> d_code [nframes][N/8].
 * With d_llr non-NULL also [nframes][N] int8: +amplitude for bit 0, -amplitude for bit 1 (1 <= amplitude <= 127) -- the decoder's input
 * with no host in between. */
int dvbs2gpu_fec_encode_batch(dvbs2gpu_ctx* ctx, int rate, int shortframes, const uint8_t* d_bbframes, int nframes, uint8_t* d_code,
                              int8_t* d_llr, int amplitude, void* stream);

/* Channel bit errors per frame: the BBFRAMEs a decoder delivered are encoded again (clauses 5.2.2, 5.3.1, 5.3.2 -- the inverse of the
 * dvbs2gpu_fec_decode_batch call that made them) and compared with the hard decisions of the LLRs that decoder read (bit 1 <=> negative).
 * d_llr [nframes][N], d_bbframes [nframes][kbch/8] -> d_counted [nframes]: LLRs that are not 0 (a 0 is an erasure and left out);
 * d_errors [nframes]: those among them whose sign is not the code bit.  d_corrections [nframes] or NULL: the decoder's BCH results; a frame
 * with a negative entry gets errors -1, counted 0 (its BBFRAME is not the transmitted one). */
int dvbs2gpu_fec_channel_ber_batch(dvbs2gpu_ctx* ctx, int rate, int shortframes, const int8_t* d_llr, const uint8_t* d_bbframes,
                                   const int32_t* d_corrections, int nframes, int32_t* d_errors, int32_t* d_counted, void* stream);

/* Host-only dump of the encoder's rules (csrc/fec_encode_rules.h; no GPU needed).  bch_generator (or NULL): the K - kbch + 1 coefficients of
 * g(x), x^0 first.  counts: int32 [80] = {BCH parity bits, BCH chunks per frame, bytes per chunk, frames per workgroup of the BCH kernel, of the
 * LDPC kernel, LDPC layers, information-bit links, workgroups per launch at the most, frames per pass of the channel BER, number of chunk seams,
 * 0 .. [16 + k]: frame bit at which the k-th chunk seam lies}. */
int dvbs2gpu_fec_encode_plan_dump(int rate, int shortframes, uint8_t* bch_generator, int32_t* counts);

/* ------------------------------------------------------------------ modulator: code words -> PLFRAME symbols -> 2-sps IQ -> channel
 * The transmit side behind the FEC encoder (ETSI EN 302 307-1 clauses 5.3.3 bit interleaver, 5.4 mapping, 5.5 PL framing with pilots and PL
 * scrambling, 5.6 root-raised-cosine shaping) and a small channel stage, so that a test signal is made where the receiver reads it.  The rules
 * are stated once in csrc/s2_tx_rules.h and run unchanged in the kernels and in dvbs2gpu_s2_tx_host.
 * A frame is named by its PLS code, pls = modcod << 2 | short << 1 | pilots; modcod 0 is the dummy PLFRAME (3330 symbols, no BBFRAME, no code
 * word).  The PLS list `pls` (host, [nframes]) is shared by the streams of a call.  Symbols and IQ are interleaved (re, im) float pairs.
 * Errors: a PLS code that names no frame (MODCODs 29..31, short 9/10, outside 0..127), a NULL pointer, a negative count, a roll-off other than
 * 0.35 / 0.25 / 0.20, a timing outside -2..2, an output that is not 16-byte aligned return DVBS2GPU_ERR_ARG with a dvbs2gpu_last_error() text
 * before anything is enqueued; a count of 0 succeeds without a launch. */

/* Host-only: the sizes of one stream's block for a PLS list.  Any output may be NULL. */
int dvbs2gpu_s2_tx_sizes(const int32_t* pls, int nframes, long long* symbols, long long* bbframe_bytes, long long* code_bytes);

/* Code words -> PL symbols, d_symbols [nstreams][symbols] (16-byte aligned).  The code word (N/8 bytes, packed MSB first, the bit order of
 * dvbs2gpu_fec_encode_batch) of frame f, stream s is read at d_code + code_off[f] + s * code_stride[f] (host arrays [nframes], bytes; entries of
 * dummy frames are ignored), so stream-major and frame-major buffers both work.  Both NULL: [nstreams][code_bytes], a stream's code words one
 * behind the other.  A code word may lie at any byte alignment: the kernel loads the aligned 32-bit words that hold it, so up to 3 bytes in
 * front of its first byte and up to 3 behind its last, inside those words, are read and discarded (never a word that holds no code byte). */
int dvbs2gpu_pl_frame_batch(dvbs2gpu_ctx* ctx, const int32_t* pls, int nframes, const uint8_t* d_code, const long long* code_off,
                            const long long* code_stride, int nstreams, float* d_symbols, void* stream);

/* Symbols [nstreams][symbols] -> IQ at 2 samples per symbol, d_iq [nstreams][2 * symbols] (16-byte aligned, not d_symbols).  Sample n sits at
 * symbol time (n - timing) / 2; the pulse is the unit-energy RRC of the given roll-off cut at +-16 symbols.  Symbols outside the block count
 * as 0, or wrap around with circular != 0 (the block can then be repeated as a seamless stream). */
int dvbs2gpu_pulse_shape_batch(dvbs2gpu_ctx* ctx, const float* d_symbols, int nstreams, long long symbols, double rolloff, double timing,
                               int circular, float* d_iq, void* stream);

/* Channel, in place on d_iq [nstreams][nsamples]: sample n of stream s is rotated by phase0[s] + cfo[s] * n (rad, rad/sample) and gets white
 * Gaussian noise of per-dimension sigma sqrt(10^(-esn0_db[s] / 10)) -- Es/N0 behind a unit-energy matched filter at 2 samples per symbol;
 * esn0_db >= 100: none; esn0_db >= -50, |cfo| <= 4, |phase0| <= 1e6 -- from a counter-based generator: the noise is a function of (seed[s], s, n) alone, the same for every launch shape.
 * The four arrays are host arrays [nstreams]. */
int dvbs2gpu_channel_batch(dvbs2gpu_ctx* ctx, float* d_iq, int nstreams, long long nsamples, const double* esn0_db, const double* cfo,
                           const double* phase0, const uint64_t* seed, void* stream);

typedef struct dvbs2gpu_tx_channel {    /* the channel's host arrays, [nstreams] each */
    const double* esn0_db;
    const double* cfo;
    const double* phase0;
    const uint64_t* seed;
} dvbs2gpu_tx_channel;

/* BBFRAMEs -> IQ in one call: dvbs2gpu_fec_encode_batch's stages, PL framing, shaping, and the channel when `channel` is not NULL.
 * d_bbframes is frame-major, [frame][stream][kbch_f / 8] (dummy frames take no bytes); d_iq [nstreams][2 * symbols].  Frames of one code that
 * follow one another share one set of encoder launches (a CCM call makes one).  The code words and symbols in between live in buffers of the
 * context. */
int dvbs2gpu_s2_modulate_batch(dvbs2gpu_ctx* ctx, const int32_t* pls, int nframes, const uint8_t* d_bbframes, int nstreams, double rolloff,
                               double timing, int circular, const dvbs2gpu_tx_channel* channel, float* d_iq, void* stream);

/* Host-only, no GPU: the same rules on the CPU for one stream, every pointer a host pointer.  code: the frames' code words one behind the
 * other (code_bytes of dvbs2gpu_s2_tx_sizes).  symbols [2 * symbols] floats and iq [4 * symbols] floats may each be NULL; channel (one entry
 * per array) may be NULL; stream_index is the s of dvbs2gpu_channel_batch. */
int dvbs2gpu_s2_tx_host(const int32_t* pls, int nframes, const uint8_t* code, double rolloff, double timing, int circular,
                        const dvbs2gpu_tx_channel* channel, long long stream_index, float* symbols, float* iq);

/* Host-only: the last two stages of dvbs2gpu_s2_tx_host on their own, for any block (host pointers).  Shaping: symbols [2 * nsymbols] floats
 * -> iq [4 * nsymbols] floats.  Channel: iq [2 * nsamples] floats in place, one entry per array of `channel`. */
int dvbs2gpu_pulse_shape_host(const float* symbols, long long nsymbols, double rolloff, double timing, int circular, float* iq);
int dvbs2gpu_channel_host(float* iq, long long nsamples, const dvbs2gpu_tx_channel* channel, long long stream_index);

/* ------------------------------------------------------------------ soft demap + bit de-interleave
 * replaces S2BBToSoft::process (dvbs2_bb_to_soft.cpp:7-33): constellation_t::demod_soft_lut per payload
 * symbol (constellation.cpp:293-322) followed by S2Deinterleaver::deinterleave (s2_deinterleaver.cpp:72-136).
 *   d_frames  [nframes][plframe_symbols] complex64 PLL output (header in [0,90), payload after it, pilot
 *             blocks at their standard positions when pilots != 0)
 *   d_llr     [nframes][N] int8 */
int dvbs2gpu_demap_batch(dvbs2gpu_ctx* ctx, int modcod, int shortframes, int pilots, const float* d_frames, int nframes,
                         int8_t* d_llr, void* stream);

/* S2Deinterleaver::deinterleave alone (s2_deinterleaver.cpp:72-136) on caller-supplied LLR frames, d_in / d_out [nframes][N]
 * int8, out of place: the index function of the fused demapper above as a stage of its own (the parity tests push the
 * reference's golden index ramps through it). */
int dvbs2gpu_deinterleave_batch(dvbs2gpu_ctx* ctx, int modcod, int shortframes, const int8_t* d_in, int nframes, int8_t* d_out,
                                void* stream);

/* ------------------------------------------------------------------ shared math definitions, evaluated on the device
 * The engine's float stages take sin/cos/atan2/exp/log from include/dvbs2gpu_math.h (where the reference calls libm:
 * freq_shift.cpp:6, dvbs2_pll.cpp:39,50-75, dvbs2_plhdr_demod.cpp:35, fll.cpp:137, constellation.cpp:226,250,259).  This
 * entry point evaluates those definitions element-wise on the GPU so that a test can compare them bit for bit with the
 * host evaluation of the same header.  func: 0 sincos(a) -> out0 = sin, out1 = cos; 1 atan2(a, b) -> out0; 2 exp(a);
 * 3 log(a); 4 the LLR clamp of constellation.cpp:263-270 (as float); 5 the LUT cell of the sample (a, b) = re_index * 256 + im_index
 * (constellation.cpp:295-301; the kernels' binary32 fast path with the double form as its guard).  Device pointers, n elements. */
int dvbs2gpu_math_eval(dvbs2gpu_ctx* ctx, int func, int n, const float* d_a, const float* d_b, float* d_out0, float* d_out1,
                       void* stream);

/* ------------------------------------------------------------------ per-stage device times
 * The reference exposes its health through the stats fields the GUI polls (module_dvbs2_demod.h:82-87); a batched GPU engine also
 * needs to show where a call's time goes.  With timing on, every stage of dvbs2gpu_demod_process[_batch] (and the FEC stage entry
 * points) is bracketed by a hipEvent pair on the stream it is enqueued on -- also in the pipelined mode, where the FEC of call k
 * runs beside the front end of call k+1, so ms[LDPC] is the decoder's time AS IT RAN inside the calls.  get_stage_times waits for
 * the outstanding events, returns the sums since the previous get and resets them.  units: frames (LDPC, BCH) or 0. */
#define DVBS2GPU_STAGE_FRONTEND 0  /* FastAGC + FreqShift + Gardner */
#define DVBS2GPU_STAGE_RRC 1       /* RRC FIR + /2 */
#define DVBS2GPU_STAGE_PLSYNC 2
#define DVBS2GPU_STAGE_LOOPS 3     /* coarse FED, PLL, PLHDR demod */
#define DVBS2GPU_STAGE_DEMAP 4     /* soft demap + bit de-interleave */
#define DVBS2GPU_STAGE_LDPC 5
#define DVBS2GPU_STAGE_BCH 6       /* BCH + BB descramble */
#define DVBS2GPU_STAGE_DELIVER 7   /* BBFRAMEs into the caller's buffers */
#define DVBS2GPU_STAGE_COUNT 8
typedef struct dvbs2gpu_stage_times {
    double ms[DVBS2GPU_STAGE_COUNT];
    int64_t launches[DVBS2GPU_STAGE_COUNT];
    int64_t units[DVBS2GPU_STAGE_COUNT];
} dvbs2gpu_stage_times;
int dvbs2gpu_set_stage_timing(dvbs2gpu_ctx* ctx, int on);
int dvbs2gpu_get_stage_times(dvbs2gpu_ctx* ctx, dvbs2gpu_stage_times* out);

/* ------------------------------------------------------------------ full DVB-S2 demodulator (one stream)
 *
 * Mirror of dsp::dvbs2::DVBS2Demod (module_dvbs2_demod.h:51-160).  A handle is one transponder stream:
 * it owns the loop state that the reference keeps in its member blocks (AGC gain, NCO phase/frequency,
 * Gardner delay line + PCL, RRC delay line, /2 decimator phase, PL-sync buffer and state machine, PLL and
 * PLHDR loops).  Not re-entrant per handle (the reference guards process() with ctrlMtx the same way).
 *
 * cfg mirrors the arguments of DVBS2Demod::init (module_dvbs2_demod.cpp:7-30) in the same units.
 *
 * ACCEPTED CONFIGURATIONS (one rule, csrc/rx_cfg_rules.h; everything else is DVBS2GPU_ERR_ARG from create, with a message that names the bound):
 *   rrc_taps 1 .. 129;  rrc_alpha within [0, 1] (0 = sinc);  samplerate, symbolrate positive and finite, their ratio positive and finite, and every
 *   RRC tap they yield finite;
 *   clock_mu_gain, clock_omega_gain, agc_rate, loop_bw, fll_bw finite;
 *   0 <= omega_rel_limit <= 0.05  and  1 - omega_rel_limit - |clock_mu_gain| / 2 >= 16/17 + 1e-6.
 * The last bound is the timing recovery's: of the two outputs per symbol one moves the loop by freq + clock_mu_gain * e (|e| <= 1), the other by freq, freq
 * within 1 -+ omega_rel_limit, so n samples yield fewer than n / (1 - omega_rel_limit - |clock_mu_gain| / 2) + 2 outputs, and the engine holds n + n/16 + 128
 * of them; it also keeps every step at 0, 1 or 2 samples and every period's outputs inside the resolvers' lists.  The plugin's gains (0.0176) pass up to
 * omega_rel_limit 0.05; at the plugin's 0.02, |clock_mu_gain| up to 0.0776. */
typedef struct dvbs2gpu_demod_cfg {
    double symbolrate, samplerate;       /* only their ratio matters (RRC taps); the plugin uses samplerate = 2*symbolrate */
    float agc_rate, rrc_alpha;
    int32_t rrc_taps;
    float loop_bw, fll_bw;
    float clock_omega_gain, clock_mu_gain, omega_rel_limit;   /* (see ACCEPTED CONFIGURATIONS above; finite gains: the timing-recovery kernels
                                          * evaluate PCL::advance(0) as "frequency unchanged") */
    int32_t modcod, shortframes, pilots;
    float sof_threshold;                 /* stored, unused in CCM mode -- as in the reference (dvbs2_pl_sync.cpp:140-142); ACM/VCM mode:
                                          * minimum SOF quality of a frame start */
    int32_t max_ldpc_trials;
    int32_t force_ldpc_iters;            /* 0 = normal early exit; n > 0 = benchmark mode, exactly n iterations */
    /* Extensions beyond the reference's behaviour, all 0 by default (= reference-compatible, parity-tested against it):
     * acm_vcm      SURVEY 8(f) rank 3.  The PL framing follows the PLS code of EVERY frame (soft RM(64,7) decode at the frame start
     *              names MODCOD, frame size and pilots, hence the frame's length and its demapper / LDPC / BCH code); modcod /
     *              shortframes / pilots above are ignored.  BBFRAMEs then differ in size: dvbs2gpu_frame_stats.bbframe_bytes.  The
     *              reference only reports what it detected (dvbs2_plhdr_demod.cpp:43-64) and lets the GUI re-configure the whole
     *              demodulator after 50 consistent sightings (main.cpp:375-408).
     * soft_plsc    SURVEY 8(f) rank 4.  The PLHDR demodulator decodes the PLS code by soft correlation over all 64 code bits instead
     *              of the reference's hard decisions compared on 60 bits (dvbs2_plhdr_demod.cpp:45-58,69-79).
     * pilot_aided  SURVEY 8(f) rank 4.  The known symbols (PL header, pilot blocks) give the PLL a block phase estimate that is
     *              applied at the end of each block, on top of the reference's decision-directed loop (dvbs2_pll.cpp:34-86): no
     *              rotational false locks.  Pilot symbols then also drive the loop with the data-aided error phase(descrambled x
     *              conj((1+j)/sqrt2)) at full gain; with 0 they use the reference's error, decision-directed on the sign-sliced
     *              QPSK point and divided by 10 (dvbs2_pll.cpp:58). */
    int32_t acm_vcm, soft_plsc, pilot_aided;
} dvbs2gpu_demod_cfg;

typedef struct dvbs2gpu_demod dvbs2gpu_demod;

/* Defaults of the plugin shell (main.cpp:64-73,134-140). */
void dvbs2gpu_demod_default_cfg(int modcod, int shortframes, int pilots, dvbs2gpu_demod_cfg* out);

/* max_samples: largest `count` a single process call may pass (SDR++ STREAM_BUFFER_SIZE = 1000000). */
int dvbs2gpu_demod_create(dvbs2gpu_ctx* ctx, const dvbs2gpu_demod_cfg* cfg, int max_samples, dvbs2gpu_demod** out);
void dvbs2gpu_demod_destroy(dvbs2gpu_demod* d);
int dvbs2gpu_demod_reset(dvbs2gpu_demod* d);                                            /* DVBS2Demod::reset */
int dvbs2gpu_demod_set_params(dvbs2gpu_demod* d, int modcod, int shortframes, int pilots, float sof_threshold,
                              int max_ldpc_trials);                                      /* DVBS2Demod::setDemodParams */
int dvbs2gpu_demod_get_kbch(dvbs2gpu_demod* d);                                          /* DVBS2Demod::getKBCH */

/* int DVBS2Demod::process(int count, const complex_t* in, uint8_t* out): h_iq = count interleaved (re,im)
 * float pairs at 2 samples/symbol, h_out receives the descrambled BBFRAMEs completed by this call
 * (kbch/8 bytes each, input order).  Returns bytes written (0 is legal) or a negative error.  Synchronous. */
int dvbs2gpu_demod_process(dvbs2gpu_demod* d, int count, const float* h_iq, uint8_t* h_out, int out_cap);

/* Same for `n` independent streams in one go (frames of all streams share the FEC launches).  d_iq[i] are
 * DEVICE pointers (inputs already resident in HBM), counts[i] samples each; d_out[i] DEVICE buffers of
 * out_cap bytes; out_bytes[i] (host) receives the byte count of stream i.  Synchronous. */
int dvbs2gpu_demod_process_batch(dvbs2gpu_demod* const* demods, int n, const float* const* d_iq, const int* counts,
                                 uint8_t* const* d_out, int out_cap, int* out_bytes);

/* Throughput mode for dvbs2gpu_demod_process_batch: with `on` != 0 the FEC (LDPC, BCH, descrambler) of call k runs on its own
 * HIP stream while call k+1 runs the front end, PL sync and frame loops of the next samples; the BBFRAMEs (and stats) of call
 * k are delivered by call k+1 into ITS output buffers (the reference delivers frames late as well: it holds them until 16 have
 * queued, module_dvbs2_demod.cpp:343-347).  The streams of a batch may change from call to call (transponders come and go, in any
 * order): a job is collected into the buffers of those of ITS streams that are part of the collecting call; a stream that joins has
 * nothing pending; the frames of a stream that is absent from the call after its own are dropped (pass it with count 0 once more
 * to collect them).  Streams of different configurations may share the batch (one FEC job per configuration group and call, at
 * most 16 groups); ACM/VCM streams too (one job per LDPC code present in the call, BBFRAMEs of differing size: per-frame sizes in
 * dvbs2gpu_frame_stats.bbframe_bytes).  A call with all counts 0 collects the last frames; switching the mode off drops
 * uncollected ones.
 * INPUT AND OUTPUT BUFFERS: as in the synchronous mode, device work the host has put on the legacy null stream before the call -- the copies or kernels that fill d_iq --
 * lies in front of the demodulator (the mode's own stream waits for it), and the buffers may be reused when the call returns; a host that fills them on a stream of
 * its own synchronises that stream before the call.  The delivered BBFRAMEs are complete when the call returns.  Switching the mode ON synchronises the device and
 * gives the context's internal streams back to the runtime (created again on demand). */
int dvbs2gpu_set_pipelined(dvbs2gpu_ctx* ctx, int on);

/* Stats of the frames completed by the last process call of this handle (the public fields the GUI polls,
 * module_dvbs2_demod.h:82-87, one record per frame). */
typedef struct dvbs2gpu_frame_stats {
    float pl_sync_best_match;
    int32_t detected_modcod, detected_shortframes, detected_pilots;
    float coarse_freq_err;
    int32_t ldpc_trials, bch_corrections;
    int32_t bbframe_bytes;               /* size of this frame's BBFRAME in the output (kbch/8; ACM/VCM: per frame, 0 for a dummy PLFRAME) */
} dvbs2gpu_frame_stats;
int dvbs2gpu_demod_get_stats(dvbs2gpu_demod* d, dvbs2gpu_frame_stats* h_out, int cap);
float dvbs2gpu_demod_get_nco_freq(dvbs2gpu_demod* d);
/* Where the frames FOUND by the last process call start: index of each frame's first symbol in the stream's symbol sequence
 * (after timing recovery, one per symbol) since the last reset.  Returns the frame count.  (In the synchronous mode these are the
 * frames the call delivered; in the throughput mode the ones the NEXT call will deliver.)  No reference counterpart: the segment
 * receiver below orders and de-duplicates frames with it. */
int dvbs2gpu_demod_get_frame_positions(dvbs2gpu_demod* d, int64_t* h_out, int cap);

/* Debug taps of the last process call (device->host copies; for parity tests and the constellation
 * display callback d_handler, module_dvbs2_demod.cpp:337).  which: 0 = 1-sps symbols entering PL sync,
 * 1 = aligned raw PLFRAMEs, 2 = PLL output, (complex64, count in complex samples); 3 = LLRs (int8).
 * Returns the element count; copies at most cap elements when h_dst != NULL.
 * Taps 2 and 3 lie in the context's per-call scratch: they are valid until the next call on the context, and in a batch whose configuration
 * groups run one after another (streams that differ in their front-end settings) they are those of the LAST group only -- the handles of
 * the other groups report 0 elements for them.  Taps 0 and 1, the statistics and the output are every handle's own. */
int dvbs2gpu_demod_get_tap(dvbs2gpu_demod* d, int which, void* h_dst, int cap);

/* Signal quality per frame (own extension; off by default).  With quality on, every frame the handle's front end
 * completes gets one record, computed on the device from the frame's PLL output (tap 2).  Its known symbols (|a| = 1) form two runs: the 90
 * header symbols (SOF + scrambled PLSC; they come from the header demodulator's own phase loop, whose phase is not the payload's) and, with
 * pilots, the P pilot symbols ((1+j)/sqrt2); K = 90 + P.  Each run gets its own complex gain h_r = sum y conj(a) / count_r.
 *   esn0_db          10 log10(g^2 / sigma^2), g^2 = (90 |h_hdr|^2 + P |h_pil|^2) / K, sigma^2 = sum over both runs of |y - h_r a|^2 / (K - runs)
 *   gain             g
 *   phase            arg h_pil; 0 without pilots (the payload is then referred to |h_hdr| at the PLL's own phase)
 *   mer_db           ETSI TR 101 290 9.1 over the payload: z = y conj(h) / |h|^2 with h = h_pil (no pilots: |h_hdr|), against the nearest
 *                    point d of the frame's constellation at unit mean energy, 10 log10(sum |d|^2 / sum |z - d|^2)
 *   known_symbols    K;  payload_symbols: slots * 90
 * A dummy PLFRAME (ACM/VCM) has no PLL output: every float is NaN and both counts are 0.
 * get_quality: one record per dvbs2gpu_demod_get_stats record, in the same order (so in the throughput mode they arrive with their frames,
 * one call late); 0 records while quality is off -- the setting in force when the frames' front end ran decides.  Returns the record count
 * and copies at most cap records when h_out != NULL.  Null handles and a negative cap: DVBS2GPU_ERR_ARG. */
typedef struct dvbs2gpu_frame_quality {
    float esn0_db, mer_db, gain, phase;
    int32_t known_symbols, payload_symbols;
} dvbs2gpu_frame_quality;
int dvbs2gpu_demod_set_quality(dvbs2gpu_demod* d, int on);
int dvbs2gpu_demod_get_quality(dvbs2gpu_demod* d, dvbs2gpu_frame_quality* h_out, int cap);

/* ------------------------------------------------------------------ fleet: the transponders of one host over several GPUs
 * The reference runs one independent DVBS2Demod instance per transponder (src/main.cpp:588,595: every plugin instance owns its demodulator and worker thread); nothing is
 * exchanged inside a frame or between streams.  A FLEET is what a C++ plugin host with several GPUs calls: `n` members -- one engine context + one worker thread per entry
 * of devices[] (a HIP device index may appear more than once: "logical devices", how the tests run a 4-member fleet on a 1-GPU box) -- and a transponder table placed on them
 * by dvbs2gpu_fleet_plan's rule: whole MODCOD groups by longest-processing-time first (every member's LDPC batches stay homogeneous) when no member ends up more than
 * `tolerance` above the average load, else the MODCOD-sorted list cut into n pieces of near-equal weight -- the rule of the multi-process harness
 * (sdrpp-dvbs-demodulator_amd/distribute.py: assign_transponders; tests/test_cabi_host.py holds the two against each other).  No device talks to another.
 *   dvbs2gpu_fleet_plan           the placement alone (no GPU): member_of[i] for nt transponders of given MODCOD and weight over `world` members.
 *   dvbs2gpu_fleet_assign         places `table` (a demodulator configuration, a weight -- <= 0: edges x iterations + 40 x PLFRAME symbols -- and the largest call in samples per
 *                                 transponder), creates every transponder's demodulator on its member (an earlier table's are destroyed), out_cap = bytes of the largest
 *                                 delivery of one transponder and call; member_of (optional) receives the placement.
 *   dvbs2gpu_fleet_process_batch  one call for ALL transponders: h_iq[i] / counts[i] HOST samples of transponder i (2 sps, interleaved floats), h_out[i] HOST buffers of out_cap
 *                                 bytes, out_bytes[i] the bytes delivered -- EGRESS IN TABLE ORDER whichever member decoded them.  The members copy, run
 *                                 dvbs2gpu_demod_process_batch and copy back side by side on their worker threads; the call returns when all are through; the first member
 *                                 error is the return code (dvbs2gpu_last_error() names the device), every member is waited for either way.
 *   dvbs2gpu_fleet_set_pipelined  the throughput mode of dvbs2gpu_set_pipelined on every member (frames one call late; a call with all counts 0 collects the last ones).
 *   dvbs2gpu_fleet_get_stats      dvbs2gpu_demod_get_stats of transponder i.      dvbs2gpu_fleet_reset: DVBS2Demod::reset of every transponder. */
typedef struct dvbs2gpu_fleet dvbs2gpu_fleet;
typedef struct dvbs2gpu_fleet_entry {
    dvbs2gpu_demod_cfg cfg;
    double weight;
    int32_t max_samples;
    int32_t reserved;
} dvbs2gpu_fleet_entry;
int dvbs2gpu_fleet_plan(const int32_t* modcods, const double* weights, int nt, int world, double tolerance, int32_t* member_of);
int dvbs2gpu_fleet_create(const int* devices, int n, dvbs2gpu_fleet** out);
void dvbs2gpu_fleet_destroy(dvbs2gpu_fleet* f);
int dvbs2gpu_fleet_size(const dvbs2gpu_fleet* f);
int dvbs2gpu_fleet_assign(dvbs2gpu_fleet* f, const dvbs2gpu_fleet_entry* table, int nt, int out_cap, double tolerance, int32_t* member_of);
int dvbs2gpu_fleet_set_pipelined(dvbs2gpu_fleet* f, int on);
int dvbs2gpu_fleet_reset(dvbs2gpu_fleet* f);
int dvbs2gpu_fleet_process_batch(dvbs2gpu_fleet* f, const float* const* h_iq, const int* counts, uint8_t* const* h_out, int out_cap, int* out_bytes);
int dvbs2gpu_fleet_get_stats(dvbs2gpu_fleet* f, int transponder, dvbs2gpu_frame_stats* h_out, int cap);

/* ------------------------------------------------------------------ segment receiver: ONE fast transponder
 * A stream's loops are serial recurrences (one stream: 0.69 Msym/s on MI355X), so a single 27.5 Msym/s transponder cannot be
 * followed sample by sample.  The segment receiver cuts a long chunk of one continuous IQ stream into `nsegments` overlapping
 * segments of `own_frames` PLFRAMEs each (+ `warm_frames` of warm-up in front, own_frames >= warm_frames), runs them as
 * independent streams of one dvbs2gpu_demod_process_batch call with freshly reset loops, orders the frames by the positions of
 * dvbs2gpu_demod_get_frame_positions, drops duplicates where neighbours overlap and returns the BBFRAMEs in stream order; the
 * tail of a chunk is the warm-up of the next call's first segment, so calls join without a gap.  No counterpart in the reference
 * (one DVBS2Demod per transponder, serial): it returns the same BBFRAMEs wherever the reference would decode them, but it is a
 * high-latency mode (a chunk is nsegments * own_frames frames long) and soft values are not bit-identical to a serial run.
 * d_iq: DEVICE pointer to `count` complex samples (interleaved floats) continuing the stream, count <= dvbs2gpu_segrx_chunk_samples;
 * d_out: DEVICE buffer; returns bytes written (kbch/8 per frame) or a negative error.  The context must be in synchronous mode. */
typedef struct dvbs2gpu_segrx dvbs2gpu_segrx;
int dvbs2gpu_segrx_create(dvbs2gpu_ctx* ctx, const dvbs2gpu_demod_cfg* cfg, int nsegments, int own_frames, int warm_frames, dvbs2gpu_segrx** out);
int dvbs2gpu_segrx_reset(dvbs2gpu_segrx* r);
void dvbs2gpu_segrx_destroy(dvbs2gpu_segrx* r);
long long dvbs2gpu_segrx_chunk_samples(dvbs2gpu_segrx* r);
int dvbs2gpu_segrx_process(dvbs2gpu_segrx* r, const float* d_iq, long long count, uint8_t* d_out, long long out_cap);
/* h_out3 = {frame sightings of the last call, frames returned, frames seen only inside a warm-up (not returned)} */
int dvbs2gpu_segrx_get_stats(dvbs2gpu_segrx* r, int32_t* h_out3);

/* ================================================================== DVB-S inner code (rows a18-a20)
 * All buffers are DEVICE pointers; calls are asynchronous on `stream`.  Handles keep per-stream state in HBM. */

/* replaces the conversion of DVBSymToSoftBlock::process (dvbs/dvbs_syms_to_soft.cpp:7-13,28-31):
 * d_soft[2i] = int8(clamp(re*100)), d_soft[2i+1] = int8(clamp(im*100)), truncation toward zero, clamp +-127.
 * The 8192-byte blocking of :33-39 is the caller's (blocks are contiguous in d_soft). */
int dvbs2gpu_dvbs_slice(dvbs2gpu_ctx* ctx, const float* d_iq, int nsymbols, int8_t* d_soft, void* stream);

/* replaces viterbi::CCDecoder (dvbs/viterbi/cc_decoder.cpp): `nstreams` independent K=7 r=1/2 (polys 79,109) block
 * decoders of `frame_size` bits with the reference's chaining (first block from all-31 metrics, every later block
 * biased to the start state returned by the previous chain-back).  work_batch runs CCDecoder::work (:304-314) on
 * `nblocks` consecutive blocks of every stream: block b of stream s is read at d_soft + s*stream_stride +
 * b*block_stride, 2*(frame_size+6) unsigned soft bytes (128 = erasure); d_bits [nstreams][nblocks][frame_size], one
 * bit per byte. */
typedef struct dvbs2gpu_ccdec dvbs2gpu_ccdec;
int dvbs2gpu_ccdec_create(dvbs2gpu_ctx* ctx, int nstreams, int frame_size, dvbs2gpu_ccdec** out);
void dvbs2gpu_ccdec_destroy(dvbs2gpu_ccdec* h);
int dvbs2gpu_ccdec_work_batch(dvbs2gpu_ccdec* h, const uint8_t* d_soft, int64_t stream_stride, int block_stride, int nblocks,
                              uint8_t* d_bits, void* stream);

/* replaces viterbi::Viterbi_DVBS (dvbs/viterbi_all.cpp:10-276) as created by DVBSDemod::init
 * (module_dvbs_demod.cpp:23: threshold 0.15, max_outsync 20, 8192-soft blocks, phases {0, 90}): one self-locking
 * punctured decoder per stream.  work_batch = DVBSVitBlock::process (dvbs_vit.cpp:6-12) for every stream: `nblocks`
 * consecutive Viterbi_DVBS::work calls.
 *   d_soft  [nstreams][nblocks][8192] int8 (not modified; the reference rotates it in place)
 *   d_bits  [nstreams][nblocks][8192] decoded bits, one per byte; the first d_nbits[s][b] of a block are that call's
 *           output (rate 5/6: bits [6799, nbits) are never written by the reference's decoder either -- stale bytes)
 *   d_nbits [nstreams][nblocks] return values of work (0 while IDLE)
 *   d_stats [nstreams][nblocks] or NULL: ber(), getState(), rate(), locked phase and shift after each call */
typedef struct dvbs2gpu_viterbi dvbs2gpu_viterbi;
typedef struct dvbs2gpu_viterbi_stats {
    float ber;
    int32_t state, rate, phase, shift;   /* state 0 IDLE / 1 SYNCED; rate 0..4 = 1/2,2/3,3/4,5/6,7/8 */
} dvbs2gpu_viterbi_stats;
int dvbs2gpu_viterbi_create(dvbs2gpu_ctx* ctx, int nstreams, float ber_threshold, int max_outsync, dvbs2gpu_viterbi** out);
int dvbs2gpu_viterbi_reset(dvbs2gpu_viterbi* h);
void dvbs2gpu_viterbi_destroy(dvbs2gpu_viterbi* h);
int dvbs2gpu_viterbi_work_batch(dvbs2gpu_viterbi* h, const int8_t* d_soft, int nblocks, uint8_t* d_bits, int32_t* d_nbits,
                                dvbs2gpu_viterbi_stats* d_stats, void* stream);

/* replaces DVBSInterleaving (dvbs/dvbs_interleaving.h:27-70): Forney de-interleaver I=12, M=17, one per stream.
 * d_in / d_out [nstreams][nbytes] (distinct buffers), nbytes a multiple of 12 (the reference handles 8*204 per call;
 * any number of such groups may be passed at once -- the FIFO state carries over exactly). */
typedef struct dvbs2gpu_forney dvbs2gpu_forney;
int dvbs2gpu_forney_create(dvbs2gpu_ctx* ctx, int nstreams, dvbs2gpu_forney** out);
void dvbs2gpu_forney_destroy(dvbs2gpu_forney* h);
int dvbs2gpu_forney_deinterleave_batch(dvbs2gpu_forney* h, const uint8_t* d_in, int nbytes, uint8_t* d_out, void* stream);

/* ------------------------------------------------------------------ DVB-S receiver bank (rows a17-a19)
 * Mirror of dsp::dvbs::DVBSDemod (module_dvbs_demod.h:14-60, module_dvbs_demod.cpp:9-117) from the input samples up to and
 * including vit.process: demod::QPSK_ALT (FastAGC, band-edge FLL, RRC, COMPLEX_FD timing recovery, Costas<4>;
 * common/dsp/demod/qpsk_alt.cpp:136-144), DVBSymToSoftBlock and Viterbi_DVBS, for `nstreams` independent streams.
 * The output of a call is what DVBSVitBlock::process hands to the TS deframer: decoded bits, one per byte (0 bytes while
 * the decoder is not locked).  cfg mirrors the arguments of DVBSDemod::init (module_dvbs_demod.cpp:9) in the same units.
 *
 * ACCEPTED CONFIGURATIONS (csrc/rx_cfg_rules.h; everything else is DVBS2GPU_ERR_ARG from create), with sps = samplerate / symbolrate:
 *   rrc_taps 65;  rrc_alpha within [0, 1];  samplerate and symbolrate within [1, 2^31) (the FLL's band-edge filters take them as ints);
 *   all gains and bandwidths finite;  sps <= 64;  0 <= omega_rel_limit <= 0.25;  sps * (1 - omega_rel_limit) >= 1.5;
 *   sps * (1 - omega_rel_limit) - |clock_mu_gain| >= 1.3.
 * The timing loop takes one symbol per freq + clock_mu_gain * e samples (|e| <= 1, freq within sps * (1 -+ omega_rel_limit)): the last bound keeps a
 * 256-sample tile of the kernel at 198 symbols or fewer (it stages 200), and the symbol and soft-bit buffers are sized from the same smallest step. */
typedef struct dvbs2gpu_dvbs_cfg {
    double symbolrate, samplerate;       /* the plugin uses samplerate = 2*symbolrate (main.cpp:139) */
    float agc_rate, rrc_alpha;
    int32_t rrc_taps;                    /* 65 (RRC_TAP_COUNT); other lengths are rejected */
    float loop_bw, fll_bw;               /* Costas and FLL loop bandwidths */
    float clock_omega_gain, clock_mu_gain, omega_rel_limit;
    float viterbi_ber_threshold;         /* 0.15 */
    int32_t viterbi_max_outsync;         /* 20   (module_dvbs_demod.cpp:23) */
} dvbs2gpu_dvbs_cfg;
typedef struct dvbs2gpu_dvbs_demod dvbs2gpu_dvbs_demod;
void dvbs2gpu_dvbs_demod_default_cfg(dvbs2gpu_dvbs_cfg* cfg);                 /* main.cpp:64-73,134-139 */
int dvbs2gpu_dvbs_demod_create(dvbs2gpu_ctx* ctx, const dvbs2gpu_dvbs_cfg* cfg, int nstreams, int max_samples, dvbs2gpu_dvbs_demod** out);
int dvbs2gpu_dvbs_demod_reset(dvbs2gpu_dvbs_demod* d);                        /* DVBSDemod::reset + a fresh Viterbi_DVBS */
void dvbs2gpu_dvbs_demod_destroy(dvbs2gpu_dvbs_demod* d);
/* DVBSDemod::process (module_dvbs_demod.cpp:78-81) for a bank with nstreams == 1: host buffers, returns the number of decoded
 * bits written to h_bits (one per byte) or a negative error.  Synchronous.  Rate 5/6 only: of the 6826-6827 bits a Viterbi block
 * advances the output by, the reference's decoder writes 6799 (viterbi_all.cpp:246-249, cc_decoder.cpp:304-314) and leaves the rest
 * of its caller's buffer as it was; here those 27-28 bits are written as 0. */
int dvbs2gpu_dvbs_demod_process(dvbs2gpu_dvbs_demod* d, int count, const float* h_iq, uint8_t* h_bits, int cap);
/* All streams of the bank in one go: d_iq[i] DEVICE pointers to counts[i] complex samples, d_bits[i] DEVICE buffers of cap
 * bytes; out_counts[i] (host) = bits written for stream i.  Synchronous. */
int dvbs2gpu_dvbs_demod_process_batch(dvbs2gpu_dvbs_demod* d, const float* const* d_iq, const int* counts, uint8_t* const* d_bits,
                                      int cap, int* out_counts);
/* stats_viterbi_ber / _lock / _rate of every stream (module_dvbs_demod.cpp:100-114); h_out [nstreams] */
int dvbs2gpu_dvbs_demod_get_stats(dvbs2gpu_dvbs_demod* d, dvbs2gpu_viterbi_stats* h_out);
/* which 0: symbols of the last call after the Costas loop (complex64; the constellation callback, module_dvbs_demod.cpp:35);
 * which 1: 8 floats of loop state (AGC gain, FLL phase/freq, timing phase/freq/offset, Costas phase/freq).  Returns the
 * element count; copies at most cap elements when h_dst != NULL. */
int dvbs2gpu_dvbs_demod_get_tap(dvbs2gpu_dvbs_demod* d, int stream, int which, void* h_dst, int cap);
/* Signal quality per stream and call (own extension; off by default), over the symbols after the Costas loop (tap 0):
 *   esn0_db     blind M2M4: M2 = mean |y|^2, M4 = mean |y|^4, S = sqrt(2 M2^2 - M4), N = M2 - S, 10 log10(S / N); NaN where undefined
 *   mer_db      QPSK decisions d = A (sgn Re y + j sgn Im y), 10 log10(sum |d|^2 / sum |y - d|^2)
 *   amplitude   A = mean(|Re y| + |Im y|) / 2;  symbols: how many symbols the call produced
 * get_quality: h_out [nstreams] of the last call; returns nstreams, or 0 when that call ran with quality off. */
typedef struct dvbs2gpu_dvbs_quality {
    float esn0_db, mer_db, amplitude;
    int32_t symbols;
} dvbs2gpu_dvbs_quality;
int dvbs2gpu_dvbs_demod_set_quality(dvbs2gpu_dvbs_demod* d, int on);
int dvbs2gpu_dvbs_demod_get_quality(dvbs2gpu_dvbs_demod* d, dvbs2gpu_dvbs_quality* h_out);

/* ------------------------------------------------------------------ DVB-S segment receiver: ONE fast DVB-S carrier
 * The DVB-S counterpart of dvbs2gpu_segrx_*: one continuous IQ stream is cut into `nsegments` overlapping segments of `own_symbols`
 * (+ `warm_symbols` of warm-up in front, own >= warm >= 8192) that run as the streams of one receiver-bank call with fresh loops and
 * a fresh Viterbi lock search; their decoded bit streams are joined where they overlap (the bits already handed out are searched for
 * in the next segment's output) and returned as ONE bit stream in order (one bit per byte), ready for dvbs2gpu_dvbs_tail_*.  A segment
 * that does not lock inside its overlap leaves a discontinuity (the deframer behind resynchronises); get_stats counts those.
 * d_iq: DEVICE pointer to `count` complex samples continuing the stream (count <= chunk_samples); d_bits: DEVICE buffer of cap bytes;
 * returns the number of bits written or a negative error.  No counterpart in the reference (one DVBSDemod per carrier, serial). */
typedef struct dvbs2gpu_dvbs_segrx dvbs2gpu_dvbs_segrx;
int dvbs2gpu_dvbs_segrx_create(dvbs2gpu_ctx* ctx, const dvbs2gpu_dvbs_cfg* cfg, int nsegments, int own_symbols, int warm_symbols, dvbs2gpu_dvbs_segrx** out);
int dvbs2gpu_dvbs_segrx_reset(dvbs2gpu_dvbs_segrx* r);
void dvbs2gpu_dvbs_segrx_destroy(dvbs2gpu_dvbs_segrx* r);
long long dvbs2gpu_dvbs_segrx_chunk_samples(dvbs2gpu_dvbs_segrx* r);
int dvbs2gpu_dvbs_segrx_process(dvbs2gpu_dvbs_segrx* r, const float* d_iq, long long count, uint8_t* d_bits, long long cap);
/* h_out4 = {segments of the last call, joined by a match, without a match, bits returned} */
int dvbs2gpu_dvbs_segrx_get_stats(dvbs2gpu_dvbs_segrx* r, int32_t* h_out4);
/* The join rule by itself, on HOST buffers (one bit per byte), no device work: where in bits[0, nbits) the stream whose last ntail bits
 * are tail[] continues (the index of the first new bit), -1 when it is not found; *inverted = 1 when the match is on the complemented
 * bits.  The last 256 bits of the tail must occur with at most 6 mismatches, anchored on one of three 64-bit keys inside them. */
long long dvbs2gpu_dvbs_segrx_find_join(const uint8_t* h_tail, long long ntail, const uint8_t* h_bits, long long nbits, int* inverted);

/* ------------------------------------------------------------------ DVB-S tail (row f: after the Viterbi decoder)
 * Replaces DVBSDefra::process / DVBS_TS_Deframer::work (dvbs/dvbs_defra.cpp:5-9, dvbs_ts_deframer.cpp:37-92), the per-frame
 * loop of DVBSDemod::process (module_dvbs_demod.cpp:83-99): DVBSInterleaving::deinterleave, 8 x DVBSReedSolomon::decode
 * (dvbs_reedsolomon.h:26-47 over libcorrect, common/correct/reed-solomon/decode.c:299-380), DVBSScrambling::descramble
 * (dvbs_scrambling.h:28-42) and the 188-byte copies, for `nstreams` independent streams with persistent state.
 * d_bits[i]: DEVICE pointer to counts[i] decoded bits (one per byte, the Viterbi output); d_ts[i]: DEVICE buffer of cap bytes that
 * receives the 188-byte TS packets of every frame found; out_bytes[i] (host).  Frame k of a call is taken at byte offset
 * 1632*k of the deframer output (the reference indexes 204*k, SURVEY Q5: wrong for k >= 1).  On a failed RS decode the
 * reference's wrapper emits the previous packet's message; so does this.  Synchronous on `stream`.
 * CAPACITY: a handle holds max_bits / 13056 + 3 frames per stream and call.  A stream of real traffic has at most one frame per
 * 13 056 bits, so it never gets there; a stream with more sync-pattern hits than that in one call (the reference's deframer delivers
 * every one) has the first max_bits / 13056 + 3 of them delivered, in order, and the rest counted: dvbs2gpu_dvbs_tail_get_dropped.
 * The deframer's history and errors_nor / errors_inv (those of the true last hit) are what they would be had nothing been dropped. */
typedef struct dvbs2gpu_dvbs_tail dvbs2gpu_dvbs_tail;
int dvbs2gpu_dvbs_tail_create(dvbs2gpu_ctx* ctx, int nstreams, int max_bits, dvbs2gpu_dvbs_tail** out);
int dvbs2gpu_dvbs_tail_reset(dvbs2gpu_dvbs_tail* t);
void dvbs2gpu_dvbs_tail_destroy(dvbs2gpu_dvbs_tail* t);
int dvbs2gpu_dvbs_tail_process_batch(dvbs2gpu_dvbs_tail* t, const uint8_t* const* d_bits, const int* counts, uint8_t* const* d_ts, int cap,
                                     int* out_bytes, void* stream);
/* h_out11 = {frames of the last call, errors_nor, errors_inv, RS error counts of the last frame's 8 packets} */
int dvbs2gpu_dvbs_tail_get_stats(dvbs2gpu_dvbs_tail* t, int stream, int32_t* h_out11);
/* *h_dropped = sync-pattern hits of the last process_batch call that this stream found beyond the handle's capacity (see CAPACITY
 * above) and did not deliver; 0 for every call that fits, after dvbs2gpu_dvbs_tail_reset and after dvbs2gpu_dvbs_tail_rs_stage */
int dvbs2gpu_dvbs_tail_get_dropped(dvbs2gpu_dvbs_tail* t, int stream, int32_t* h_dropped);
/* Stage taps of the last call for one stream (host copies; returns the byte count, h_dst may be NULL to query it):
 *   0  frames found by the deframer, 1632 bytes each (DVBS_TS_Deframer::work output, dvbs_ts_deframer.cpp:37-92)
 *   1  the same frames after the Forney de-interleaver and the in-place RS correction, 8 x 204 bytes each
 *   2  per packet: 1 = libcorrect produced a message, 0 = it gave up (decode.c:299-380)
 *   3  per packet (int32): message bytes changed, the value DVBSReedSolomon::decode returns (dvbs_reedsolomon.h:26-47) */
int dvbs2gpu_dvbs_tail_get_tap(dvbs2gpu_dvbs_tail* t, int stream, int which, void* h_dst, int cap);
/* Stage entry (parity tests): RS(204,188) + the wrapper's stale-output rule + energy dispersal removal on `npackets` (a multiple of
 * 8) 204-byte packets supplied by the caller as stream 0's de-interleaved frames -- DVBSReedSolomon::decode and
 * DVBSScrambling::descramble without the deframer and the de-interleaver in front.  skip_rs != 0: the packets are taken as decoded
 * (descrambler alone).  npackets is at most 8 * (max_bits / 13056 + 3), the frames one call on this handle can hold (DVBS2GPU_ERR_ARG
 * beyond).  HOST pointers; returns the TS bytes written to h_ts (188 per packet); taps 1-3 above then hold the
 * corrected packets, the decoder status and the error counts.  Advances stream 0's dispersal / last-message state and overwrites the
 * handle's de-interleaved packets, status and frame counts: TEST HOOK, to be called on a handle of its own, never on one that is
 * receiving (calls are serialised per context like every other entry point). */
int dvbs2gpu_dvbs_tail_rs_stage(dvbs2gpu_dvbs_tail* t, const uint8_t* h_packets, int npackets, int skip_rs, uint8_t* h_ts, int cap);
/* Stage entry (parity tests): the de-puncturers and the soft rotation that run inside the Viterbi kernel, on HOST buffers.
 *   mode 0  Depunc23 / Depunc56 ::depunc_static (depunc.h:16-38,108-137), period 3 / 6, h_state4[1] = shift
 *   mode 1  ::depunc_cont (:46-80,139-185) with h_state4 = {is_first, changing_shift, got_extra, buf} carried across calls
 *           (set_shift(s): {s > period - 1, s, 0, 128})
 *   mode 2  rotate_soft (common/codings/rotation.cpp:4-63) for h_state4[0] = 0 / 1 (PHASE_0 / PHASE_90), signed bytes in and out
 * h_out (out_cap >= 2*size + 2 bytes) keeps the caller's fill where the stage does not write.  Returns the output count. */
int dvbs2gpu_dvbs_depuncture(dvbs2gpu_ctx* ctx, int period, int mode, const uint8_t* h_in, int size, uint8_t* h_out, int out_cap,
                             int32_t* h_state4);
/* int DVBSDemod::process(int count, const complex_t* in, uint8_t* out) as a whole (module_dvbs_demod.cpp:78-99), host buffers, for a
 * one-stream receiver bank `d` and a one-stream tail `t` (created with max_bits >= the bank's bit capacity: max_samples is enough):
 * count complex samples in, the TS packets completed by this call out (188 bytes each); the decoded bits stay in HBM between the
 * two halves.  Returns the bytes written or a negative error; packets that do not fit into cap are dropped, as by the tail.  Synchronous. */
int dvbs2gpu_dvbs_process_ts(dvbs2gpu_dvbs_demod* d, dvbs2gpu_dvbs_tail* t, int count, const float* h_iq, uint8_t* h_ts, int cap);

/* ------------------------------------------------------------------ BBFRAME -> MPEG-TS / GSE parser (row f, rank 1)
 * Replaces dsp::dvbs2::BBFrameTSParser (dvbs2/bbframe_ts_parser.h:68-112, .cpp:31-390), which the reference's sink handler runs
 * on DVBS2Demod's output (main.cpp:532-558), for `nstreams` independent streams with persistent state (synchronisation,
 * the TS packet cut by a frame boundary, three GSE reassembly slots).  BBFRAMEs are kbch/8 bytes each, as the engine emits them.
 * MPEG-TS frames (TS/GS = 11) are packetised on the GPU: header CRC-8 / DFL / SYNCD checks, resynchronisation at SYNCD, one
 * 0x47 + 187-byte packet per 188 bytes of data field.  GSE frames (TS/GS = 01) are decapsulated on the GPU as well (GSE -> GRE,
 * fragment reassembly with CRC-32, .cpp:212-383); the library's native host parser follows the same rules on the same state and
 * runs a stream's call only where dvbs2gpu_bbts_set_gse_path or one of the two fallbacks below says so.
 * Where the reference is undefined the library does this: a GSE packet that would extend beyond the end of the input of the
 * call ends the parsing of its frame; a PDU that does not fit into the rest of the output buffer or whose reassembled length
 * is negative is dropped; a fragment overflowing the 64 KiB reassembly buffer frees its slot.
 * cap must be >= nframes*kbch/8 + 376, else DVBS2GPU_ERR_CAPACITY (the reference stops with "BUFF OVF!" when fewer than 189
 * bytes are left, .cpp:178,206; with this bound a TS-only call never gets there). */
typedef struct dvbs2gpu_bbts dvbs2gpu_bbts;
int dvbs2gpu_bbts_create(dvbs2gpu_ctx* ctx, int nstreams, int kbch_bits, int max_frames, dvbs2gpu_bbts** out);
/* BBFrameTSParser::setFrameSize (.cpp:31-42): new frame size, synchronisation of every stream forgotten */
int dvbs2gpu_bbts_set_frame_size(dvbs2gpu_bbts* b, int kbch_bits);
void dvbs2gpu_bbts_destroy(dvbs2gpu_bbts* b);
/* d_bb[i]: DEVICE pointer to nframes[i] BBFRAMEs; d_out[i]: DEVICE buffer of cap bytes; out_bytes[i] (host) = bytes produced
 * (work()'s return value per stream).  Synchronous on `stream`. */
int dvbs2gpu_bbts_process_batch(dvbs2gpu_bbts* b, const uint8_t* const* d_bb, const int* nframes, uint8_t* const* d_out, int cap,
                                int* out_bytes, void* stream);
/* BBFrameTSParser::work for a bank with nstreams == 1 and host buffers: returns the bytes written to h_ts or a negative error */
int dvbs2gpu_bbts_work(dvbs2gpu_bbts* b, const uint8_t* h_bb, int cnt, uint8_t* h_ts, int cap);
/* h_out[0..10] = last_header {ts_gs, sis_mis, ccm_acm, issyi, npd, ro, isi, upl, dfl, sync, syncd}, [11] last_gse_crc_err,
 * [12] last_bb_cnt, [13] last_bb_proc, [14] last_ts_errs (main.cpp reads these for its status lines); n_out >= 15;
 * with n_out >= 17 also [15] synched, [16] bytes of the carried partial packet */
int dvbs2gpu_bbts_get_stats(dvbs2gpu_bbts* b, int stream, int32_t* h_out, int n_out);

/* ---- GSE (the GSE branch of work(), .cpp:212-383).  Output per PDU: a GRE header 00 00, the protocol type in two more bytes
 * for IPv4 / IPv6 (0x0800 / 0x86DD, .cpp:258-275 and :355-371), then the PDU; packets back to back, nothing between them.
 * mode 0 (default): GSE frames are parsed by the GPU kernels.  mode 1: a stream that carries a GSE frame in a call is handed, for
 * that call, to the host parser (six blocking copies per stream and call; kept for comparison).  Both give the same bytes, state and
 * counters, and the mode may change between calls.  In mode 0 the host parser still runs a stream's call when
 *   (a) one of its frames holds more than 256 GSE packets (the per-frame record capacity), or
 *   (b) an output-capacity rule would fire in it: a GRE packet that does not fit into cap and is dropped, or no more than 188 bytes
 *       left after a TS frame (.cpp:178,206).  cap >= nframes*kbch/8 + 376 + the bytes of the reassemblies open before the call
 *       (at most 3 x 65536) keeps (b) away. */
int dvbs2gpu_bbts_set_gse_path(dvbs2gpu_bbts* b, int mode);
typedef struct dvbs2gpu_gse_stats {
    int64_t frames;               /* GSE frames whose data field was walked (.cpp:212: UPL 0, no ISSY, no NPD) */
    int64_t packets;              /* GSE packets taken from them (.cpp:224-252) */
    int64_t complete_pdus;        /* unfragmented PDUs written (.cpp:254-283) */
    int64_t reassembled_pdus;     /* PDUs written after reassembly with a good CRC-32 (.cpp:340-377) */
    int64_t crc_failures;         /* END packets whose CRC-32 did not match (.cpp:351) */
    int64_t dropped_no_slot;      /* START packets that found all three reassembly slots taken (.cpp:289-300) */
    int64_t dropped_overflow;     /* reassemblies given up because a fragment would pass 64 KiB */
    int64_t dropped_no_fit;       /* PDUs that did not fit into the rest of the output, or whose reassembled length was negative */
    int64_t bytes_delivered;      /* GRE bytes written, headers included */
    int64_t host_fallback_calls;  /* calls of this stream the host parser ran in mode 0 = the next two */
    int64_t fallback_records;     /* (a) */
    int64_t fallback_capacity;    /* (b) */
} dvbs2gpu_gse_stats;
int dvbs2gpu_bbts_get_gse_stats(dvbs2gpu_bbts* b, int stream, dvbs2gpu_gse_stats* h_out);
/* One row per GRE packet the LAST call wrote for the stream, in output order (the reference sends the whole call's output as one
 * datagram, main.cpp:551-555; with the rows a caller sends one per PDU).  The TS packets of a call that mixes TS and GSE frames are
 * not rows: they are the bytes of [0, out_bytes) that no row covers. */
#define DVBS2GPU_GSE_PDU_REASSEMBLED 1
#define DVBS2GPU_GSE_PDU_LABEL 2     /* the packet (the START packet) carried a 6-byte label (.cpp:236-244) */
typedef struct dvbs2gpu_gse_pdu {
    uint32_t offset;     /* of the GRE header in the stream's output buffer */
    uint32_t bytes;      /* GRE header + PDU */
    uint16_t protocol;   /* GSE protocol type; 0x0800 / 0x86DD: 4-byte GRE header, else 2 bytes */
    uint16_t flags;
    uint32_t reserved;
} dvbs2gpu_gse_pdu;
/* h_rows[cap] (host); *n = rows of the last call, of which min(*n, cap) are written */
int dvbs2gpu_bbts_get_pdu_table(dvbs2gpu_bbts* b, int stream, dvbs2gpu_gse_pdu* h_rows, int cap, int* n);
/* the same table in HBM, valid until the bank's next call: *d_rows is a DEVICE pointer (NULL when *n == 0) */
int dvbs2gpu_bbts_get_pdu_table_device(dvbs2gpu_bbts* b, int stream, const dvbs2gpu_gse_pdu** d_rows, int* n);
/* Host only, no device needed: a CRC-32/MPEG register (polynomial 0x04c11db7, MSB first, as .cpp:85-102) advanced over nbytes
 * zero bytes, = crc * x^(8 nbytes) mod P, with the arithmetic the GSE kernels use.  crc(a ++ b) = shift(crc(a), len b) ^ crc0(b),
 * crc0 = the CRC from a zero register. */
uint32_t dvbs2gpu_crc32_mpeg_shift(uint32_t crc, uint32_t nbytes);

/* ------------------------------------------------------------------ BBFRAME -> TS, mode-adaptation mode
 * What the reference's parser leaves out, for multiple-input-stream (MIS) and ACM/VCM carriers: ISI demultiplexing, ISSY and DNP
 * fields, null-packet reinsertion, the per-packet CRC-8, and BBFRAMEs whose size differs from frame to frame.  Off by default and
 * separate from the calls above, which keep the reference's behaviour and their own state whether the mode is on or not.
 *   Slot: [CRC-8 of the previous UP][187 UP bytes][ISSY: 0, 2 or 3 bytes, present iff ISSYI][DNP: 1 byte iff NPD].
 *   Frames: header CRC-8, DFL a whole number of bytes that fits the frame, SYNCD < DFL or 65535; others are counted in
 *     rejected_frames.  Frames with TS/GS != 11 or of an ISI that is not selected are counted in skipped_frames (SIS frames are ISI 0);
 *     with dvbs2gpu_bbts_ma_set_gse on, the GSE frames of a selected ISI are decapsulated instead (below).
 *   Framing is per frame: the first slot that starts in a frame starts SYNCD/8 bytes into the data field (65535: none does, the
 *     data field continues one slot), further ones every slot length.  A slot leaves when the byte after it -- the CRC-8 of its
 *     UP -- has arrived; what is left of a data field (1 .. slot length bytes) is carried to the next frame of the SAME ISI and
 *     completed only if carried + SYNCD/8 == slot length, else dropped and counted in broken_joins.
 *   Output per slot: DNP x (47 1F FF 10 + 184 x FF), then 0x47 + the 187 UP bytes; a CRC-8 mismatch sets the packet's
 *     transport_error_indicator and counts in ts_errs.  ISSY bytes are dropped, the last ISCR is reported.
 *   ISSY length: cfg.issy_bytes, or (0) from the first ISSY field that starts in a frame of that ISI: top bit 0 -> 2 bytes,
 *     top bits 10 -> 3 bytes, 11 decides nothing; until then the ISI's frames are dropped and counted in `undecided`.
 *   Capacity: every output size is computed first; if one exceeds cap the call returns DVBS2GPU_ERR_CAPACITY, no state has
 *     advanced and needed[] holds the sizes, so the same call can be repeated with larger buffers. */
typedef struct dvbs2gpu_bbts_ma_cfg {
    int32_t issy_bytes;      /* 0: from the stream (see above), 2 or 3 */
    int32_t crc_span;        /* 0: the CRC-8 covers the 187 UP bytes; 1: every byte of the slot after its first */
    int32_t reinsert_nulls;  /* 0: DNP is ignored */
    int32_t check_crc;       /* 0: no CRC-8 check, no transport_error_indicator */
} dvbs2gpu_bbts_ma_cfg;
typedef struct dvbs2gpu_bbts_ma_stats {
    int64_t packets, nulls, ts_errs;     /* user packets emitted, null packets put back, packets that left with TEI set */
    int32_t broken_joins, undecided, frames;   /* per selected ISI; frames = frames of this ISI parsed or dropped as undecided */
    int32_t skipped_frames, rejected_frames;   /* per stream (the same for all its slots) */
    int32_t issy_bytes;                  /* ISSY length in use, 0 while not known */
    int32_t iscr_valid;  uint32_t last_iscr;   /* last ISCR seen: 15 bits (short) or 22 bits (long) */
    int32_t carried;                     /* bytes of the partial (or held whole) slot waiting for the next frame of this ISI */
    int32_t selected, isi;               /* is this slot in use, and for which ISI (-1: none) */
    int32_t hem_frames;                  /* those of `frames` that were high-efficiency-mode frames (dvbs2gpu_bbts_ma_set_t2_hem) */
} dvbs2gpu_bbts_ma_stats;
void dvbs2gpu_bbts_ma_default_cfg(dvbs2gpu_bbts_ma_cfg* cfg);            /* {0, 0, 1, 1} */
/* out4 = {offset of the CRC-8, offset and length of the UP, offset of the ISSY field} inside a slot, as compiled in */
int dvbs2gpu_bbts_ma_get_layout(int32_t* out4);
/* a bank of one stream without a device: only the mode-adaptation calls that take host buffers work on it (ma_work, ma_flush,
 * select_isi, the statistics); everything runs in the library's host parser, which follows the same rules as the kernels */
int dvbs2gpu_bbts_create_host(int kbch_bits, int max_frames, dvbs2gpu_bbts** out);
/* cfg != NULL: mode on, every stream starts afresh with ISI 0 selected.  NULL: mode off; the reference-mode parser then continues
 * like a freshly created bank. */
int dvbs2gpu_bbts_set_mode_adaptation(dvbs2gpu_bbts* b, const dvbs2gpu_bbts_ma_cfg* cfg);
/* the ISIs of `stream` to deliver, n <= 8: slot k of the stream's outputs and statistics is isi[k].  The stream's slots start afresh. */
int dvbs2gpu_bbts_select_isi(dvbs2gpu_bbts* b, int stream, const uint8_t* isi, int n);
/* d_bb[i]: DEVICE pointer to nframes[i] (<= max_frames) BBFRAMEs back to back; frame_bytes NULL or frame_bytes[i] NULL: each is
 * kbch/8 bytes (CCM), else frame_bytes[i][f] is the size of frame f (10 .. 7274: dvbs2gpu_frame_stats.bbframe_bytes of an ACM/VCM
 * handle, zeros left out).  d_out[i*8 + k]: DEVICE buffer of cap bytes for slot k of stream i (unused slots may be NULL);
 * out_bytes[i*8 + k] and needed[i*8 + k] (host; needed may be NULL).  Synchronous on `stream`. */
int dvbs2gpu_bbts_process_ma_batch(dvbs2gpu_bbts* b, const uint8_t* const* d_bb, const int* const* frame_bytes, const int* nframes,
                                   uint8_t* const* d_out, int cap, int* out_bytes, int* needed, void* stream);
/* the same for a bank of one stream and host buffers: h_out[8], out_bytes[8], needed[8] or NULL.  Returns 0 or a negative error. */
int dvbs2gpu_bbts_ma_work(dvbs2gpu_bbts* b, const uint8_t* h_bb, const int* frame_bytes, int cnt, uint8_t* const* h_out, int cap,
                          int* out_bytes, int* needed);
/* end of input: a whole slot held back because the CRC-8 after it has not arrived leaves unchecked, with its null packets.
 * out[i*8 + k]: cap bytes each, DEVICE buffers (host buffers for a host bank); out_bytes[nstreams*8]. */
int dvbs2gpu_bbts_ma_flush(dvbs2gpu_bbts* b, uint8_t* const* out, int cap, int* out_bytes);
/* the same with HOST buffers for any bank (the companion of dvbs2gpu_bbts_ma_work) */
int dvbs2gpu_bbts_ma_flush_host(dvbs2gpu_bbts* b, uint8_t* const* h_out, int cap, int* out_bytes);
int dvbs2gpu_bbts_ma_get_stats(dvbs2gpu_bbts* b, int stream, int slot, dvbs2gpu_bbts_ma_stats* h_out);

/* ---- GSE in the mode-adaptation mode (TS 102 606-1): one reassembly context per (stream, selected ISI) lane.  Off by default; while
 * it is off every call above behaves as before and GSE frames count in skipped_frames.  Rules, where they differ from the reference
 * mode's above or where the standard (or memory of it) leaves room:
 *   Frames walked: header accepted as above, ISI selected, TS/GS = 01, UPL = 0, neither ISSYI nor NPD.  Other TS/GS = 01 frames of a
 *     selected ISI count in skipped_frames.  A walked frame counts in dvbs2gpu_bbts_ma_stats.frames of its lane.
 *   The walk starts at byte 0 of the data field and covers DFL/8 bytes.  SYNCD is not used: there is no "synchronised" state and no
 *     SYNCD/8 + 1 skip, so the result does not depend on how calls cut the frame sequence.  Frame sizes come from frame_bytes.
 *   Packet: S, E, LT and a 12-bit GSE length.  Fixed fields after the two header bytes: S=1 E=1 protocol type (2); S=1 E=0 frag id,
 *     total length, protocol type (5); S=0 frag id (1), and an END (S=0 E=1) ends with its CRC-32 (4 more).  Labels exist in S=1
 *     packets only: LT 00 six bytes, 01 three bytes, 10 none, 11 (re-use of the label before) none.  They are skipped, not filtered
 *     (DVBS2GPU_GSE_PDU_LABEL in a row says that label BYTES were present: a re-use packet reports "no label"),
 *     and LT is not looked at in S=0 packets.  S=0 E=0 LT=00 is padding and ends the frame's walk, also in the last byte of a data field.
 *   Malformed: a length field smaller than the fixed fields + label (for an END: + 4, so a reassembled length is never negative and
 *     dropped_no_fit stays 0 in this mode), a packet that would pass the end of the data field, or one byte left that is not padding.
 *     It ends the walk of ITS frame only and counts once in malformed_frames; the packets before it stand.  The reference mode's
 *     `& 0xffff` length arithmetic and its "past the end of the call's input" rule do not apply.  The total-length field of a START is
 *     covered by the CRC-32 and otherwise not used, as in the reference.
 *   Reassembly: three slots per lane, first fit; a START takes a free slot or the one that holds its frag id; other fragments go to
 *     the busy slot with their frag id or are ignored; a fragment that would pass 64 KiB frees the slot (dropped_overflow); CRC-32/MPEG
 *     over total length, protocol type, label and PDU; last_crc_err is the verdict of the lane's last END.  Slots belong to the lane:
 *     frames of another ISI never touch them.  dvbs2gpu_bbts_select_isi (for that stream), dvbs2gpu_bbts_set_mode_adaptation and
 *     switching GSE off start them afresh.
 *   Output: the GRE packets of the reference mode (00 00, + the protocol type for 0x0800 / 0x86DD, then the PDU) in the lane's own
 *     buffer d_out[i*8 + k].  A lane that receives TS and GSE frames writes both in FRAME ORDER: the concatenated output of any
 *     cutting of the sequence into calls is the same.
 *   Capacity: as for TS.  Sizes first, GRE bytes included; if one exceeds cap: DVBS2GPU_ERR_CAPACITY, needed[] filled, no state (TS or
 *     GSE) has advanced, the table of the call is empty.  No PDU is ever dropped for lack of room.
 *   The one host fallback: a frame with more than 256 packets.  That stream's call is then run by the library's host parser from
 *     the same state (counted in host_fallback_calls); bytes, rows and state are what an unbounded record table would have given.
 *   Memory (device banks): 3 x 64 KiB of slot storage per SELECTED lane plus 8 KiB of records and rows per frame of a call, allocated
 *     when the bank first meets a GSE frame with the switch on; a later selection with more lanes makes the pool grow. */
int dvbs2gpu_bbts_ma_set_gse(dvbs2gpu_bbts* b, int on);   /* needs the mode on */
typedef struct dvbs2gpu_bbts_ma_gse_stats {
    int64_t frames, packets, complete_pdus, reassembled_pdus, crc_failures, dropped_no_slot, dropped_overflow, dropped_no_fit,
            bytes_delivered;             /* as in dvbs2gpu_gse_stats, per lane */
    int64_t malformed_frames;            /* frames whose walk ended at a malformed packet */
    int64_t host_fallback_calls;         /* per stream (the same for all its slots) */
    int32_t open_slots;                  /* reassemblies open now, 0..3 */
    int32_t last_crc_err;
} dvbs2gpu_bbts_ma_gse_stats;
int dvbs2gpu_bbts_ma_get_gse_stats(dvbs2gpu_bbts* b, int stream, int slot, dvbs2gpu_bbts_ma_gse_stats* h_out);
/* the rows of the last call for slot `slot` of `stream`, in output order; offset is relative to that slot's buffer and
 * DVBS2GPU_GSE_PDU_LABEL means label bytes of any length (6 or 3; not set for label re-use, which carries none).  The TS packets of a lane that mixes both are the bytes no row covers. */
int dvbs2gpu_bbts_ma_get_pdu_table(dvbs2gpu_bbts* b, int stream, int slot, dvbs2gpu_gse_pdu* h_rows, int cap, int* n);
/* the same in HBM, valid until the bank's next call (device banks only; NULL when *n == 0) */
int dvbs2gpu_bbts_ma_get_pdu_table_device(dvbs2gpu_bbts* b, int stream, int slot, const dvbs2gpu_gse_pdu** d_rows, int* n);
/* ---- DVB-T2 high-efficiency mode (HEM) in the mode-adaptation mode: the BBFRAMEs of a T2-MI feed (the T2-MI bank below) are of this
 * kind on most networks.  Off by default; while it is off every call above behaves as before and a HEM frame counts in
 * rejected_frames.  The rules are written from memory of EN 302 755 5.1.7 and 5.1.8; the constants are in ONE struct of the library
 * and dvbs2gpu_bbts_ma_get_hem_layout reports them.
 *   Mode of a frame: c = CRC-8 of the first nine header bytes.  Byte 9 == c: normal mode, the rules above.  Byte 9 == c ^ MODE (1)
 *     and the switch on: HEM.  Anything else: rejected_frames.  DFL and SYNCD are checked as above; padding and in-band signalling
 *     behind DFL are never looked at.  TS/GS, SIS/MIS, ISSYI, NPD and the ISI (the PLP id) are read from the same bits.  A HEM frame
 *     with TS/GS != 11 or of an ISI that is not selected counts in skipped_frames: HEM GSE frames are not decapsulated, also with
 *     dvbs2gpu_bbts_ma_set_gse on.  A parsed HEM frame counts in `frames` and in `hem_frames` of its lane.
 *   Header: bytes 2-3 (UPL in normal mode) and byte 6 (SYNC) are neither; UPL is implied, 188 bytes.  With ISSYI = 1 the three are the
 *     ISSY field of the first UP that starts in this data field (bytes 2-3 its upper bytes, byte 6 its lowest): it gives iscr_valid /
 *     last_iscr, short or long, in frame order, from frames in which a slot starts only.  There is no ISSY field per UP, so the ISSY
 *     length question never arises: issy_bytes and `undecided` are not touched by HEM frames.
 *   Slot: [187 UP bytes][DNP: 1 byte iff NPD], 187 or 188 bytes; no sync byte and no CRC-8 in the data field.  Output per slot as
 *     above: DNP null packets if cfg.reinsert_nulls, then 0x47 + the 187 bytes.  No HEM slot ever sets TEI; ts_errs does not move.
 *   Framing is per frame: the first slot starts SYNCD/8 bytes in, further ones every slot length L.  A slot leaves as soon as its LAST
 *     byte is there: n = (DFL/8 - SYNCD/8) / L slots, and the 0 .. L-1 bytes behind them are carried (0: nothing is).  The carry joins
 *     the next frame of the same ISI only if carried + SYNCD/8 == L and the carried bytes are HEM bytes of the same L; else it is
 *     dropped and counted in broken_joins.  A normal-mode frame after a HEM carry and a HEM frame after a normal-mode carry count there
 *     once, too.  With SYNCD = 65535 the data field continues the carried slot.  With nothing carried, a frame whose SYNCD/8 > 0 starts
 *     at its first slot and the bytes before it are not counted: the rule of normal mode for a fresh lane.  The output does not depend
 *     on how calls cut the frame sequence.
 *   Flush: a HEM carry is a partial slot; dvbs2gpu_bbts_ma_flush emits nothing for it and clears it.  The one exception is a slot that a
 *     SYNCD = 65535 frame completed to its last byte: it is whole, waits for the next frame of its ISI like a held normal-mode slot and
 *     leaves with a flush.
 *   Capacity: as above. */
int dvbs2gpu_bbts_ma_set_t2_hem(dvbs2gpu_bbts* b, int on);   /* needs the mode on; device and host banks; every lane starts afresh */
/* out4 = {offset and length of the UP, offset of the DNP byte = slot length without NPD, MODE value XORed into the CRC-8} */
int dvbs2gpu_bbts_ma_get_hem_layout(int32_t* out4);
/* mask8: bit i of the 256-bit mask = a frame with a valid header and ISI i has been seen on `stream` since the mode was set */
int dvbs2gpu_bbts_get_isi_seen(dvbs2gpu_bbts* b, int stream, uint32_t* mask8);

/* ------------------------------------------------------------------ TS monitor bank (own extension)
 * Nothing in the reference does this: it hands the packets of dsp::dvbs2::BBFrameTSParser / dsp::dvbs::DVBSDemod on unlooked at.
 * For `nstreams` transport streams in HBM -- the output buffers of dvbs2gpu_bbts_process_batch, dvbs2gpu_bbts_process_ma_batch or
 * dvbs2gpu_dvbs_tail_process_batch -- a bank keeps the packet-header checks of ETSI TR 101 290 first priority (sync byte,
 * continuity count) per stream, reports which PIDs the last call brought, and compacts the packets a PID filter lets pass.
 *   Packet: 188 bytes at offset 188 k of a stream's input; no sync search (the packetisers emit whole packets from offset 0).
 *   Header (ISO/IEC 13818-1 2.4.3.2): sync b0, TEI b1>>7, PUSI (b1>>6)&1, PID (b1&0x1f)<<8|b2, TSC b3>>6, AFC (b3>>4)&3, CC b3&15;
 *     DI (discontinuity indicator) b5>>7, taken only when AFC&2 and b4 > 0, else 0.
 *   Classification, in this order: b0 != 0x47 a sync-byte error (nothing else of the packet counts); TEI set a TEI packet (header
 *     not trusted: no PID row, no continuity step); PID 0x1FFF a null packet (a PID row, no continuity step); else the continuity
 *     step of its PID.
 *   Continuity per (stream, PID), state seen / last (4 bits) / dup_used, in this order: never seen: seen=1, last=CC, row flag
 *     FIRST_SEEN, no verdict.  DI: last=CC, row flag DISCONTINUITY, counted in `discontinuities`, no verdict.  No payload (AFC 0 or
 *     2): an error if CC != last.  Payload: CC == last+1 (mod 16) is good; CC == last with dup_used clear is a duplicate and sets
 *     dup_used; anything else is a continuity error.  Every step ends with last=CC, and dup_used clear unless it was the duplicate.
 *     A duplicate is recognised by CC alone: the two packets' bytes are not compared.
 *   State survives from call to call: the result does not depend on how a stream is cut into calls.  reset forgets it (the
 *     counters too; the filters stay).
 *   Filter per stream: mode 0 every PID passes, 1 the listed PIDs, 2 all but the listed; drop_null / drop_tei / drop_bad_sync take
 *     those packets out whatever the list says.  A TEI packet or one with a bad sync byte has no trusted PID: it passes unless its
 *     flag drops it.  The statistics and the table do not depend on the filter, except passed_packets.
 *   Capacity: sizes first.  If the passing packets of one stream exceed cap the call returns DVBS2GPU_ERR_CAPACITY, out_bytes[]
 *     holds the sizes, no state or counter of any stream has advanced and the table of the call is empty: the same call can be
 *     repeated with larger buffers.
 *   Limits: max_packets <= 8192 per stream and call.  Memory (device banks): 8 KiB of continuity state and 1 KiB of filter per
 *     stream, 25 bytes per packet of max_packets for the table. */
typedef struct dvbs2gpu_tsmon dvbs2gpu_tsmon;
int dvbs2gpu_tsmon_create(dvbs2gpu_ctx* ctx, int nstreams, int max_packets, dvbs2gpu_tsmon** out);
/* a bank without a device: the library's native host implementation of the same rules, behind dvbs2gpu_tsmon_work only */
int dvbs2gpu_tsmon_create_host(int nstreams, int max_packets, dvbs2gpu_tsmon** out);
int dvbs2gpu_tsmon_reset(dvbs2gpu_tsmon* m);
void dvbs2gpu_tsmon_destroy(dvbs2gpu_tsmon* m);
typedef struct dvbs2gpu_tsmon_filter {
    int32_t mode;            /* 0 pass all, 1 pass listed, 2 drop listed */
    int32_t drop_null, drop_tei, drop_bad_sync;
} dvbs2gpu_tsmon_filter;
/* pids[n]: the list (each <= 0x1FFF; n may be 0).  A new bank passes everything. */
int dvbs2gpu_tsmon_set_filter(dvbs2gpu_tsmon* m, int stream, const dvbs2gpu_tsmon_filter* f, const uint16_t* pids, int n);
/* d_ts[i]: DEVICE pointer to nbytes[i] bytes (a multiple of 188, at most 188*max_packets) of stream i.  d_out NULL: statistics and
 * table only (out_bytes may be NULL too).  Else d_out[i]: DEVICE buffer of cap bytes that receives the passing packets in input
 * order, out_bytes[i] (host) their bytes; d_out[i] must not overlap d_ts[i].  Synchronous on `stream`: chained behind a packetiser
 * call on the same stream, the packets never visit the host. */
int dvbs2gpu_tsmon_process_batch(dvbs2gpu_tsmon* m, const uint8_t* const* d_ts, const int* nbytes, uint8_t* const* d_out, int cap,
                                 int* out_bytes, void* stream);
/* one stream of any bank with HOST buffers (h_out NULL: statistics only): returns the bytes written to h_out or a negative error.
 * The other streams of the bank receive an empty call. */
int dvbs2gpu_tsmon_work(dvbs2gpu_tsmon* m, int stream, const uint8_t* h_ts, int nbytes, uint8_t* h_out, int cap);
typedef struct dvbs2gpu_tsmon_stats {          /* since creation or reset */
    int64_t packets;             /* every 188 bytes handed in */
    int64_t null_packets, tei_packets, sync_byte_errors;
    int64_t cc_errors, duplicates, discontinuities;
    int64_t scrambled_packets;   /* trusted packets (null packets included) with TSC != 0 */
    int64_t passed_packets;      /* packets the filter let pass (also counted in calls without output buffers) */
    int64_t pids_seen;           /* PIDs whose `seen` bit is set */
} dvbs2gpu_tsmon_stats;
int dvbs2gpu_tsmon_get_stats(dvbs2gpu_tsmon* m, int stream, dvbs2gpu_tsmon_stats* h_out);
/* One row per PID among the trusted packets of the LAST call (the null PID included), ascending by PID. */
#define DVBS2GPU_TSMON_PID_FIRST_SEEN 1      /* the PID's first packet since reset came in this call */
#define DVBS2GPU_TSMON_PID_DISCONTINUITY 2   /* a packet of the PID announced a discontinuity in this call */
typedef struct dvbs2gpu_tsmon_pid {
    uint16_t pid, flags;
    uint32_t packets, cc_errors, duplicates, scrambled, pusi;
} dvbs2gpu_tsmon_pid;
/* h_rows[cap] (host); *n = rows of the last call, of which min(*n, cap) are written */
int dvbs2gpu_tsmon_get_pid_table(dvbs2gpu_tsmon* m, int stream, dvbs2gpu_tsmon_pid* h_rows, int cap, int* n);
/* the same table in HBM, valid until the bank's next call (device banks only): *d_rows is a DEVICE pointer (NULL when *n == 0) */
int dvbs2gpu_tsmon_get_pid_table_device(dvbs2gpu_tsmon* m, int stream, const dvbs2gpu_tsmon_pid** d_rows, int* n);

/* ------------------------------------------------------------------ PSI section bank (own extension)
 * Nothing in the reference does this.  For `nstreams` transport streams in HBM a bank reassembles the PSI/SI sections on up to 16
 * watched PIDs per stream, checks each section's CRC-32, writes the sections and one table row per section to device buffers and keeps
 * the decoded PAT and PMTs on the host.  The sequential form below is the definition (csrc/psi_rules.h, PsiHostStream::run); the
 * kernels give its results for every cutting of a stream into calls.  The section syntax (ISO/IEC 13818-1 2.4.4) is one struct of
 * offsets, dvbs2gpu_psi_layout.
 *   State per (stream, watched slot): the continuity byte of the TS monitor's automaton; a 4096-byte section buffer; fill, the bytes
 *     buffered (0: no section is open); the last four bytes of the last valid section and a flag that there has been one.
 *   Packet: 188 bytes at offset 188 k, classified as the TS monitor does.  Packets of unwatched PIDs, sync-byte errors and TEI packets
 *     are not looked at (the gap a TEI packet leaves shows in the next packet's continuity step); PID 0x1FFF cannot be watched.
 *   A packet of a watched PID, in this order.  "Drop" = the open section is forgotten; with fill > 0 it counts in dropped_sections.
 *     1. TSC != 0: scrambled_packets, drop, the continuity step; nothing more of the packet is used.
 *     2. The continuity step.  Duplicate: ignored.  Continuity error or announced discontinuity: drop, then go on with this packet
 *        (with nothing open only a PUSI packet starts anything).  No payload (AFC&1 = 0): done.
 *     3. The payload starts at 4, or at 5 + b4 when AFC&2.  >= 188: malformed_packets, drop, done.
 *     4. PUSI set: ptr = the first payload byte.  ptr > the bytes after it: malformed_packets, drop, done.  The ptr bytes after the
 *        pointer go to an open section: if they complete it, it is emitted and what is left of them is ignored; if it is still
 *        incomplete after them, it is dropped; with nothing open they are ignored.  Then section starts are parsed behind them (6).
 *     5. PUSI clear: the whole payload goes to an open section; if it completes it, it is emitted and the rest of the payload is
 *        ignored.  With nothing open the payload is ignored.
 *     6. At a section start, until the packet ends: a byte 0xFF ends the packet (stuffing).  Otherwise bytes are buffered; with three,
 *        total = 3 + (((b1 & 0x0F) << 8) | b2); section_length > 4093: malformed_sections, nothing is open, the rest of the packet is
 *        ignored (the same where an open section's header is completed by a later packet).  When the buffered bytes reach total the
 *        section is emitted and the next byte is a section start.  A section, or a header of one or two bytes, that the packet's end
 *        cuts stays open.
 *   Emitting.  ssi = b1 >> 7.  ssi set and total < 12: malformed_sections, no row, no bytes, nothing else.  Otherwise the section
 *     counts in `sections`, and in unexpected_table_id if the watch names another table_id.  ssi set: valid if CRC-32/MPEG (initial
 *     value 0xFFFFFFFF, polynomial 0x04C11DB7) over all its bytes is 0; else crc_errors and row flag CRC_ERROR, row and bytes still
 *     delivered.  ssi clear: valid.  A valid section is CHANGED when the slot has had no valid section, or its last four bytes (the
 *     CRC field with ssi set; of a 3-byte section all three) differ from the stored ones; the stored ones are then replaced.
 *     Consequence: a table of one section (a PAT, a PMT) is flagged once per version; the sections of a multi-section table flag
 *     each other.
 *   Row: one per emitted section, ordered by (packet that held its last byte, position in it): one order per stream across its PIDs.
 *   Deliver mode per stream: 0 the bytes of every emitted section, 1 only those of valid changed ones.  Rows and counters do not
 *     depend on it, except row.offset and bytes_delivered; a call without output buffers delivers nothing.
 *   State survives from call to call.  reset forgets it (counters and decoded views too; watches and deliver modes stay); changing a
 *     slot's watch starts that slot afresh.
 *   Capacity: sizes first.  If one stream's bytes exceed cap or its rows exceed max_sections the call returns DVBS2GPU_ERR_CAPACITY,
 *     out_bytes[] holds the byte sizes (-1 for a stream whose rows did not fit: its sections were not checked) and out_rows[] the row
 *     counts; no state or counter of any stream has advanced, the table of the call is empty, the call can be repeated.
 *   Decoded views: the host keeps, per slot, the bytes of its last valid CHANGED section with ssi, table_id 0 or 2 and current_next 1;
 *     a device bank copies them across in the call that flags them, and only then.  Nothing follows the PAT by itself: which PMT PIDs
 *     are watched is the caller's set_watch, so no result depends on where a call boundary fell.
 *   Limits: max_packets <= 4096 per stream and call.  Memory (device banks) per stream: 64 KiB of section buffers, 64 KiB of view
 *     staging, 6 bytes per packet of max_packets and 40 bytes per row of max_sections. */
typedef struct dvbs2gpu_psi dvbs2gpu_psi;
typedef struct dvbs2gpu_psi_layout {
    int32_t header_bytes, length_mask, max_section_length, max_section_bytes, min_long_section;
    int32_t ext_at, version_at, section_number_at, last_section_number_at, long_header_bytes, crc_bytes;
    int32_t pat_loop_at, pat_stride, pmt_pcr_at, pmt_info_length_at, pmt_loop_at, pmt_stride;
} dvbs2gpu_psi_layout;
int dvbs2gpu_psi_create(dvbs2gpu_ctx* ctx, int nstreams, int max_packets, int max_sections, dvbs2gpu_psi** out);
/* a bank without a device: the library's native host implementation of the same rules, behind dvbs2gpu_psi_work only */
int dvbs2gpu_psi_create_host(int nstreams, int max_packets, int max_sections, dvbs2gpu_psi** out);
int dvbs2gpu_psi_reset(dvbs2gpu_psi* b);
void dvbs2gpu_psi_destroy(dvbs2gpu_psi* b);
int dvbs2gpu_psi_get_layout(dvbs2gpu_psi_layout* h_out);
/* slot 0..15; pid 0..0x1FFE, or -1: the slot watches nothing; expect_table_id 0..255, or -1: any.  A new bank watches PID 0 in slot 0
 * of every stream, expecting table_id 0.  The same PID in two slots of a stream is DVBS2GPU_ERR_ARG. */
int dvbs2gpu_psi_set_watch(dvbs2gpu_psi* b, int stream, int slot, int pid, int expect_table_id);
int dvbs2gpu_psi_set_deliver(dvbs2gpu_psi* b, int stream, int mode);
/* d_ts[i]: DEVICE pointer to nbytes[i] bytes (a multiple of 188, at most 188*max_packets) of stream i.  d_out NULL: rows and counters
 * only (never a capacity failure for bytes; out_bytes may be NULL).  Else d_out[i]: DEVICE buffer of cap bytes for the delivered
 * sections, back to back in row order; out_bytes[i] (host) their bytes.  out_rows (host, may be NULL): the row counts.  Synchronous
 * on `stream`; chained behind a packetiser or monitor call on the same stream, no packet visits the host. */
int dvbs2gpu_psi_process_batch(dvbs2gpu_psi* b, const uint8_t* const* d_ts, const int* nbytes, uint8_t* const* d_out, int cap, int* out_bytes,
                               int* out_rows, void* stream);
/* one stream of any bank with HOST buffers (h_out NULL: rows and counters only): returns the bytes written to h_out or a negative
 * error.  The other streams of the bank receive an empty call. */
int dvbs2gpu_psi_work(dvbs2gpu_psi* b, int stream, const uint8_t* h_ts, int nbytes, uint8_t* h_out, int cap);
/* the byte and row sizes that the stream's last call needed, whether it succeeded or failed for capacity (what out_bytes / out_rows
 * held; the way to them behind dvbs2gpu_psi_work) */
int dvbs2gpu_psi_get_needed(dvbs2gpu_psi* b, int stream, int* bytes, int* rows);
typedef struct dvbs2gpu_psi_stats {            /* since creation or reset; kept on the host */
    int64_t packets;                 /* trusted packets of the watched PID */
    int64_t sections, valid, changed, crc_errors, dropped_sections, malformed_sections, malformed_packets, scrambled_packets,
            unexpected_table_id, bytes_delivered;
} dvbs2gpu_psi_stats;
/* slot -1: the sum over the stream's slots.  A slot's counters start again when its watch changes. */
int dvbs2gpu_psi_get_stats(dvbs2gpu_psi* b, int stream, int slot, dvbs2gpu_psi_stats* h_out);
#define DVBS2GPU_PSI_CRC_ERROR 1
#define DVBS2GPU_PSI_CHANGED 2
typedef struct dvbs2gpu_psi_section {
    uint16_t pid, flags;
    uint8_t table_id, ssi, version, current_next, section_number, last_section_number;   /* from version on: 0 when ssi is clear */
    uint16_t table_id_ext;
    int32_t length;                  /* total bytes */
    int32_t offset;                  /* into the stream's output buffer; -1: not delivered */
    int32_t first_packet;            /* index in this call of the packet that held its first byte; -1: an earlier call */
} dvbs2gpu_psi_section;
/* h_rows[cap] (host); *n = rows of the last call, of which min(*n, cap) are written */
int dvbs2gpu_psi_get_section_table(dvbs2gpu_psi* b, int stream, dvbs2gpu_psi_section* h_rows, int cap, int* n);
/* the same table in HBM, valid until the bank's next call (device banks only): *d_rows is a DEVICE pointer (NULL when *n == 0) */
int dvbs2gpu_psi_get_section_table_device(dvbs2gpu_psi* b, int stream, const dvbs2gpu_psi_section** d_rows, int* n);
/* Decoded views (host parsers, csrc/psi_rules.h; no device is touched).  A loop or descriptor length that runs past the section's
 * end makes the view empty and sets hdr.malformed; no byte outside the section is read. */
typedef struct dvbs2gpu_psi_program { uint16_t program_number, pid; } dvbs2gpu_psi_program;   /* program 0: the network PID */
typedef struct dvbs2gpu_psi_pat { int32_t transport_stream_id, version, malformed; } dvbs2gpu_psi_pat;   /* -1, -1, 0: no PAT held */
/* from the PAT held by the stream's lowest slot that holds one */
int dvbs2gpu_psi_get_programs(dvbs2gpu_psi* b, int stream, dvbs2gpu_psi_pat* hdr, dvbs2gpu_psi_program* h_rows, int cap, int* n);
typedef struct dvbs2gpu_psi_es { uint16_t stream_type, elementary_pid; } dvbs2gpu_psi_es;
typedef struct dvbs2gpu_psi_pmt { int32_t program_number, version, pcr_pid, malformed; } dvbs2gpu_psi_pmt;   /* program_number -1: no PMT held */
int dvbs2gpu_psi_get_program_map(dvbs2gpu_psi* b, int stream, int slot, dvbs2gpu_psi_pmt* hdr, dvbs2gpu_psi_es* h_rows, int cap, int* n);

/* ------------------------------------------------------------------ PCR bank (own extension)
 * Nothing in the reference does this.  For `nstreams` transport streams in HBM a bank checks the programme clock references of up to
 * 16 watched PIDs per stream: PCR repetition, PCR discontinuity and PCR accuracy of ETSI TR 101 290 second priority (2.3a, 2.3b, 2.4),
 * one table row per PCR.  The engine has no clock: a PCR is a 27 MHz clock, and on a constant-rate stream (DVB-S, DVB-S2 CCM) the
 * packet position is a second one, so every check is integer arithmetic on (PCR value, packet position) pairs and no result depends
 * on how a stream is cut into calls.  The sequential form below is the definition (csrc/pcr_rules.h, PcrHostStream::run).
 *   Watches: 16 slots per stream, each a PID 0..0x1FFE or nothing.  A new bank watches nothing.  Changing a slot's watch starts the
 *     slot afresh, state and counters.
 *   Packet: 188 bytes at offset 188 k, classified as the TS monitor does.  Sync-byte errors, TEI packets and null packets are not
 *     looked at.  Scrambling does not matter (the adaptation field is never scrambled); continuity is deliberately not consulted: a
 *     lost packet does not make a PCR wrong.
 *   A packet carries a PCR when AFC&2 is set, b4 (adaptation_field_length) >= 1 and b5 & 0x10 is set.  It is then malformed if
 *     b4 < 7, or b4 > 183 (> 182 with AFC = 3), or the extension is > 299; base is the 33 bits b6 b7 b8 b9 and the top bit of b10, the
 *     extension the low bit of b10 and b11.  A malformed packet of a watched PID is counted in its slot, gets no row and does not
 *     step the state; one of an unwatched PID is ignored.  Otherwise P = base * 300 + ext, the value modulo M = 2^33 * 300.
 *   A well-formed PCR packet of an unwatched PID adds to the stream's unwatched_pcr_packets; the PID of the call's first one in input
 *     order is first_unwatched_pid (-1: none): how a caller finds PCR PIDs it did not know of.
 *   Position: n = the stream's packet count since creation or reset + the packet's index in the call, 64 bits.  Every packet of
 *     every call counts, untrusted ones too.
 *   State per slot: seen; last_pcr; ref_n, the position that the next interval is measured from.
 *   Step for a record (P, n, DI), in this order:
 *     1. not seen: FIRST; state := (P, n).
 *     2. DI set: ANNOUNCED; state := (P, n).
 *     3. P == last_pcr: REPEATED; the state is unchanged (a legal duplicate packet does not shift the reference: the pair behind
 *        a run of equal values is measured from the run's first packet).
 *     4. dP = (P - last_pcr) mod M, dN = n - ref_n.  dP > 2 700 000 (100 ms): JUMP (2.3b; a backward step lands here).
 *        dP > 1 080 000 (40 ms): LATE (2.3a).  Else OK.  State := (P, n).
 *   Accuracy: LATE and OK pairs against the stream's rate, if one is set (ticks per 188-byte packet in Q24.24, tpp):
 *     e = (dP << 24) - min(dN, 32767) * tpp (int64), accuracy = e >> 18 (arithmetic) clamped to +-(2^31 - 1), in 1/64 tick.
 *     |accuracy| > limit: flag ACCURACY_ERROR.  dN > 32767: flag SATURATED.  No rate set: accuracy 0, no flag.
 *   Row: one per well-formed PCR packet of a watched PID, in input order across the slots.  delta_ticks = dP and delta_packets = dN
 *     saturate at 2^32 - 1; both are 0 for FIRST, ANNOUNCED and REPEATED.  The table holds the first max_rows rows of a call: a
 *     monitor does not fail for room.  out_rows[] carries the true count, rows_dropped accumulates the excess, and the counters
 *     cover every record, row or not.
 *   State survives from call to call.  reset forgets it (positions and counters too; watches and rates stay).
 *   Limits: max_packets <= 4096 per stream and call.  Memory (device banks) per stream: 400 bytes of state, 32 bytes per row of
 *     max_rows and a call record of 1 KiB. */
typedef struct dvbs2gpu_pcr dvbs2gpu_pcr;
int dvbs2gpu_pcr_create(dvbs2gpu_ctx* ctx, int nstreams, int max_packets, int max_rows, dvbs2gpu_pcr** out);
/* a bank without a device: the library's native host implementation of the same rules, behind dvbs2gpu_pcr_work only */
int dvbs2gpu_pcr_create_host(int nstreams, int max_packets, int max_rows, dvbs2gpu_pcr** out);
int dvbs2gpu_pcr_reset(dvbs2gpu_pcr* b);
void dvbs2gpu_pcr_destroy(dvbs2gpu_pcr* b);
/* slot 0..15; pid 0..0x1FFE, or -1: the slot watches nothing.  The same PID in two slots of a stream is DVBS2GPU_ERR_ARG. */
int dvbs2gpu_pcr_set_watch(dvbs2gpu_pcr* b, int stream, int slot, int pid);
/* ticks_per_packet_q24: 27 MHz ticks per 188-byte packet in Q24.24, round(1504 * 27e6 / bit rate * 2^24) (1000 << 24 at
 * 40.608 Mbit/s), < 2^48, 0: not set (a new bank).  limit_q6 >= 0 in 1/64 tick; a new bank has 864 = 13.5 ticks = 500 ns (TR 101 290
 * 2.4).  The slots' states and counters stay. */
int dvbs2gpu_pcr_set_rate(dvbs2gpu_pcr* b, int stream, uint64_t ticks_per_packet_q24, int limit_q6);
/* d_ts[i]: DEVICE pointer to nbytes[i] bytes (a multiple of 188, at most 188*max_packets) of stream i, of any alignment.  out_rows
 * (host, may be NULL): the records of the call per stream, of which the table holds the first max_rows.  One kernel launch.
 * Synchronous on `stream`; chained behind a packetiser or monitor call on the same stream, no packet visits the host. */
int dvbs2gpu_pcr_process_batch(dvbs2gpu_pcr* b, const uint8_t* const* d_ts, const int* nbytes, int* out_rows, void* stream);
/* one stream of any bank with a HOST buffer: returns the records of the call or a negative error.  The other streams of the bank
 * receive an empty call. */
int dvbs2gpu_pcr_work(dvbs2gpu_pcr* b, int stream, const uint8_t* h_ts, int nbytes);
typedef struct dvbs2gpu_pcr_stats {            /* of a slot, since creation, reset or the slot's last set_watch; kept on the host */
    int64_t pcr_packets;             /* records: first + announced + repeated + jumps + late + ok */
    int64_t first, announced, repeated, jumps, late, ok;
    int64_t malformed;
    int64_t accuracy_measured, accuracy_errors;
    int64_t sum_ticks, sum_packets;  /* over LATE and OK pairs that are not SATURATED */
    int64_t max_delta_ticks;         /* over LATE and OK pairs */
    int64_t max_abs_accuracy;
} dvbs2gpu_pcr_stats;
/* slot -1: the sum over the stream's slots (of the two maxima the larger) */
int dvbs2gpu_pcr_get_stats(dvbs2gpu_pcr* b, int stream, int slot, dvbs2gpu_pcr_stats* h_out);
typedef struct dvbs2gpu_pcr_stream_stats {
    int64_t packets;                 /* every 188 bytes handed in: the position of the next packet */
    int64_t unwatched_pcr_packets;
    int64_t rows_dropped;
    int32_t first_unwatched_pid;     /* of the last call; -1: none */
    int32_t reserved;
    int64_t packets_since_pcr[16];   /* per slot: `packets` minus the position of the slot's last record (1: the stream's last
                                        packet was it); -1: the slot has had none */
} dvbs2gpu_pcr_stream_stats;
int dvbs2gpu_pcr_get_stream_stats(dvbs2gpu_pcr* b, int stream, dvbs2gpu_pcr_stream_stats* h_out);
/* the transport-stream rate as the slot's PCRs give it: 1504 * 27e6 * sum_packets / sum_ticks in bit/s, 0 with no pairs (slot -1:
 * over all slots).  Host arithmetic. */
int dvbs2gpu_pcr_get_rate(dvbs2gpu_pcr* b, int stream, int slot, double* bits_per_s);
#define DVBS2GPU_PCR_FIRST 0
#define DVBS2GPU_PCR_ANNOUNCED 1
#define DVBS2GPU_PCR_REPEATED 2
#define DVBS2GPU_PCR_OK 3
#define DVBS2GPU_PCR_LATE 4
#define DVBS2GPU_PCR_JUMP 5
#define DVBS2GPU_PCR_ACCURACY_ERROR 1
#define DVBS2GPU_PCR_SATURATED 2
#pragma pack(push, 4)
typedef struct dvbs2gpu_pcr_row {              /* 32 bytes; pcr lies at offset 12 */
    uint16_t pid;
    uint8_t slot, kind;              /* DVBS2GPU_PCR_FIRST .. DVBS2GPU_PCR_JUMP */
    uint16_t flags, reserved;
    int32_t packet;                  /* index in this call */
    uint64_t pcr;                    /* P */
    uint32_t delta_ticks, delta_packets;
    int32_t accuracy;                /* 1/64 tick */
} dvbs2gpu_pcr_row;
#pragma pack(pop)
/* h_rows[cap] (host); *n = rows of the last call in the table, of which min(*n, cap) are written */
int dvbs2gpu_pcr_get_row_table(dvbs2gpu_pcr* b, int stream, dvbs2gpu_pcr_row* h_rows, int cap, int* n);
/* the same table in HBM, valid until the bank's next call (device banks only): *d_rows is a DEVICE pointer (NULL when *n == 0) */
int dvbs2gpu_pcr_get_row_table_device(dvbs2gpu_pcr* b, int stream, const dvbs2gpu_pcr_row** d_rows, int* n);

/* ------------------------------------------------------------------ PES bank (own extension)
 * Nothing in the reference does this.  For `nstreams` transport streams in HBM a bank looks at the elementary streams of up to 16
 * watched PIDs per stream: where PES packets start and what their headers say, whether the PES packets are whole (PES_packet_length
 * against the payload bytes that came, continuity in between), and the presentation and decoding timestamps -- PTS_error of ETSI
 * TR 101 290 second priority (2.5) among them.  One table row per PES packet start.  The engine has no clock: a timestamp is a 90 kHz
 * clock and on a constant-rate stream the packet position is a second one, so every check is integer arithmetic and no result depends
 * on how a stream is cut into calls.  The sequential form below is the definition (csrc/pes_rules.h, PesHostStream::run).
 *   Watches: 16 slots per stream, each a PID 0..0x1FFE or nothing.  A new bank watches nothing.  Changing a slot's watch starts the
 *     slot afresh, state and counters.
 *   Packet: 188 bytes at offset 188 k, classified as the TS monitor does.  Sync-byte errors, TEI packets, null packets and packets of
 *     unwatched PIDs are not looked at.  A remaining packet of a watched PID counts in `packets` and, in this order:
 *     1. takes the TS monitor's continuity step (dvbs2gpu_tsmon_*: one state byte per slot).  DUPLICATE: counted in duplicates, nothing
 *        more of the packet is used.  CC_ERROR (counted in cc_errors) or an announced discontinuity: the slot's open PES packet is
 *        marked GAP, and the packet goes on.
 *     2. No payload (AFC&1 clear): done.
 *     3. AFC = 3 and b4 (adaptation_field_length) > 182: malformed_packets, the open PES packet is marked GAP, done.
 *     4. The payload starts at byte 4 (AFC = 1) or 5 + b4 (AFC = 3) and holds L = 188 - start bytes.  L adds to payload_bytes; a packet
 *        with TSC != 0 adds to scrambled_packets, and its payload is not read.
 *     5. PUSI clear: L adds to the bytes of the open PES packet, 1 to its packets (both saturate at 2^32 - 1).  PUSI set: a start.
 *   Start: one row; the kind is the first of
 *       SCRAMBLED   TSC != 0
 *       SHORT       L < 6
 *       BAD_START   payload[0..2] != 00 00 01
 *       PLAIN       stream_id 0xBC, 0xBE, 0xBF, 0xF0, 0xF1, 0xF2, 0xF8 or 0xFF: a stream without the optional header
 *       SHORT       L < 9
 *       MALFORMED   (payload[6] & 0xC0) != 0x80, or PTS_DTS_flags = 01, or PES_header_data_length < 5 (flags 10) or < 10 (flags 11)
 *       SHORT       L < 14 (flags 10) or L < 19 (flags 11): the header is split over packets, which is legal and rare; it is not parsed
 *       MALFORMED   a marker bit of a timestamp is 0, or its 4-bit prefix is not 0010 (PTS alone), 0011 (PTS with DTS), 0001 (DTS)
 *       HEADER      anything else
 *     stream_id = payload[3] from BAD_START on (0 before).  declared = PES_packet_length, payload[4..5], from PLAIN on and for the
 *     second SHORT; 0 (unknown) for SCRAMBLED, the first SHORT and BAD_START.  pts / dts: the 33-bit values of a HEADER row, all ones
 *     where absent and in every other kind.  A HEADER start with declared = 0 and a stream_id outside 0xE0..0xEF has the flag
 *     UNBOUNDED_NONVIDEO (only video may leave the length open).
 *   Closing: a start closes the slot's open PES packet, if there is one: closed_bytes and closed_packets are that packet's (the
 *     start's own L is not among them), with the flag CLOSED and one of: CLOSED_GAP if it was marked GAP; else CLOSED_UNCHECKED if its
 *     declared length was 0; else CLOSED_MISMATCH if its bytes != declared + 6.  None of the three: the PES packet was whole.  The
 *     start then is the open PES packet: its declared, L bytes, 1 packet, no GAP.
 *   Timestamps: HEADER rows with a PTS.  T = the DTS if present, else the PTS.  DTS_AFTER_PTS: both present and (pts - dts) mod 2^33
 *     >= 2^32.  State per slot: seen, last_T, ref_n.  Not seen: flag TS_FIRST, no deltas.  Else dT = (T - last_T) mod 2^33 and dN =
 *     n - ref_n: dT >= 2^32: TS_BACKWARD; else dT > 63 000 (0.7 s at 90 kHz): TS_GAP; with a rate set and dN > late_packets: PTS_LATE
 *     (TR 101 290 2.5: a PTS repetition period of more than 700 ms), late_packets = floor((18 900 000 << 24) / ticks_per_packet_q24).
 *     delta_ts = dT as int32 (values >= 2^32 shown negative, dT - 2^33; clamped), delta_packets = dN saturating at 2^32 - 1.  Then
 *     state := (T, n).
 *   Position: n = the stream's packet count since creation or reset + the packet's index in the call, 64 bits.  Every packet of
 *     every call counts, untrusted ones too.
 *   Row: one per start, in input order across the slots.  The table holds the first max_rows rows of a call: a monitor does not fail
 *     for room.  out_rows[] carries the true count, rows_dropped accumulates the excess, and the counters cover every start.
 *   State survives from call to call.  reset forgets it (positions and counters too; watches and rates stay).
 *   Limits: max_packets <= 4096 per stream and call.  Memory (device banks) per stream: 512 bytes of state, 48 bytes per row of
 *     max_rows and a call record of 1552 bytes. */
typedef struct dvbs2gpu_pes dvbs2gpu_pes;
int dvbs2gpu_pes_create(dvbs2gpu_ctx* ctx, int nstreams, int max_packets, int max_rows, dvbs2gpu_pes** out);
/* a bank without a device: the library's native host implementation of the same rules, behind dvbs2gpu_pes_work only */
int dvbs2gpu_pes_create_host(int nstreams, int max_packets, int max_rows, dvbs2gpu_pes** out);
int dvbs2gpu_pes_reset(dvbs2gpu_pes* b);
void dvbs2gpu_pes_destroy(dvbs2gpu_pes* b);
/* slot 0..15; pid 0..0x1FFE, or -1: the slot watches nothing.  The same PID in two slots of a stream is DVBS2GPU_ERR_ARG. */
int dvbs2gpu_pes_set_watch(dvbs2gpu_pes* b, int stream, int slot, int pid);
/* ticks_per_packet_q24: the quantity of dvbs2gpu_pcr_set_rate (27 MHz ticks per 188-byte packet in Q24.24, < 2^48), 0: not set (a new
 * bank; no PTS_LATE).  The slots' states and counters stay. */
int dvbs2gpu_pes_set_rate(dvbs2gpu_pes* b, int stream, uint64_t ticks_per_packet_q24);
/* d_ts[i]: DEVICE pointer to nbytes[i] bytes (a multiple of 188, at most 188*max_packets) of stream i, of any alignment.  out_rows
 * (host, may be NULL): the starts of the call per stream, of which the table holds the first max_rows.  One kernel launch.
 * Synchronous on `stream`; chained behind a packetiser or monitor call on the same stream, no packet visits the host. */
int dvbs2gpu_pes_process_batch(dvbs2gpu_pes* b, const uint8_t* const* d_ts, const int* nbytes, int* out_rows, void* stream);
/* one stream of any bank with a HOST buffer: returns the starts of the call or a negative error.  The other streams of the bank
 * receive an empty call. */
int dvbs2gpu_pes_work(dvbs2gpu_pes* b, int stream, const uint8_t* h_ts, int nbytes);
typedef struct dvbs2gpu_pes_stats {            /* of a slot, since creation, reset or the slot's last set_watch; kept on the host */
    int64_t packets;                 /* trusted packets of the watched PID, duplicates among them */
    int64_t payload_bytes, duplicates, cc_errors, scrambled_packets, malformed_packets;
    int64_t starts;                  /* rows: the sum of the six kinds */
    int64_t starts_scrambled, starts_short, starts_bad_start, starts_plain, starts_malformed, starts_header;
    int64_t with_pts, with_dts;      /* HEADER starts */
    int64_t closed_ok;               /* CLOSED and none of the three flags below */
    int64_t closed_mismatch, closed_gap, closed_unchecked;
    int64_t ts_backward, ts_gap, pts_late, dts_after_pts;
    int64_t max_delta_packets;
} dvbs2gpu_pes_stats;
/* slot -1: the sum over the stream's slots (of the maximum the larger) */
int dvbs2gpu_pes_get_stats(dvbs2gpu_pes* b, int stream, int slot, dvbs2gpu_pes_stats* h_out);
typedef struct dvbs2gpu_pes_stream_stats {
    int64_t packets;                 /* every 188 bytes handed in: the position of the next packet */
    int64_t rows_dropped;
    int64_t packets_since_start[16]; /* per slot: `packets` minus the position of the slot's last start (1: the stream's last packet
                                        was it); -1: the slot has had none */
} dvbs2gpu_pes_stream_stats;
int dvbs2gpu_pes_get_stream_stats(dvbs2gpu_pes* b, int stream, dvbs2gpu_pes_stream_stats* h_out);
#define DVBS2GPU_PES_SCRAMBLED 0
#define DVBS2GPU_PES_SHORT 1
#define DVBS2GPU_PES_BAD_START 2
#define DVBS2GPU_PES_PLAIN 3
#define DVBS2GPU_PES_MALFORMED 4
#define DVBS2GPU_PES_HEADER 5
#define DVBS2GPU_PES_CLOSED 1
#define DVBS2GPU_PES_CLOSED_GAP 2
#define DVBS2GPU_PES_CLOSED_MISMATCH 4
#define DVBS2GPU_PES_CLOSED_UNCHECKED 8
#define DVBS2GPU_PES_UNBOUNDED_NONVIDEO 16
#define DVBS2GPU_PES_TS_FIRST 32
#define DVBS2GPU_PES_TS_BACKWARD 64
#define DVBS2GPU_PES_TS_GAP 128
#define DVBS2GPU_PES_PTS_LATE 256
#define DVBS2GPU_PES_DTS_AFTER_PTS 512
#pragma pack(push, 4)
typedef struct dvbs2gpu_pes_row {              /* 48 bytes */
    uint16_t pid;                    /* offset 0 */
    uint8_t slot, kind;              /* 2, 3: DVBS2GPU_PES_SCRAMBLED .. DVBS2GPU_PES_HEADER */
    uint16_t flags;                  /* 4 */
    uint8_t stream_id, reserved;     /* 6, 7 */
    int32_t packet;                  /* 8: index in this call */
    uint32_t declared;               /* 12: PES_packet_length, 0: unknown or unbounded */
    uint64_t pts, dts;               /* 16, 24: all ones: absent */
    uint32_t closed_bytes, closed_packets;   /* 32, 36: of the PES packet that this start closed */
    uint32_t delta_packets;          /* 40 */
    int32_t delta_ts;                /* 44: 90 kHz ticks */
} dvbs2gpu_pes_row;
#pragma pack(pop)
/* h_rows[cap] (host); *n = rows of the last call in the table, of which min(*n, cap) are written */
int dvbs2gpu_pes_get_row_table(dvbs2gpu_pes* b, int stream, dvbs2gpu_pes_row* h_rows, int cap, int* n);
/* the same table in HBM, valid until the bank's next call (device banks only): *d_rows is a DEVICE pointer (NULL when *n == 0) */
int dvbs2gpu_pes_get_row_table_device(dvbs2gpu_pes* b, int stream, const dvbs2gpu_pes_row** d_rows, int* n);

/* ------------------------------------------------------------------ ES bank (own extension)
 * Nothing in the reference does this.  For `nstreams` transport streams in HBM a bank reads every payload byte of up to 16 watched video
 * PIDs per stream and writes an index of what they hold: one table row per PES packet start and one per reported start code -- pictures
 * with their type, sequence headers / SPS, GOP headers, parameter sets, access unit delimiters, sequence ends -- with the position of
 * each in the elementary stream, so that picture sizes are differences of positions and the PTS of a picture is that of the PES row in
 * front of it.  The sequential form below is the definition (csrc/es_rules.h, EsHostStream::run); no result depends on how a stream is
 * cut into calls or on the alignment of the input.  The syntax is written from memory of ISO/IEC 13818-1, 13818-2, 14496-10 and
 * 23008-2 and pinned to no vector of theirs.
 *   Watches: 16 slots per stream, each empty or a PID 0..0x1FFE with a codec: DVBS2GPU_ES_MPEG2 (also MPEG-1 video), _H264, _H265.  A
 *     new bank watches nothing.  The same PID in two slots of a stream is an argument error.  Setting a watch starts the slot afresh,
 *     state and counters: UNSYNCED, have = 0.
 *   Packet: 188 bytes at offset 188 k, classified as the TS monitor does; only trusted packets of watched PIDs are looked at.  Such a
 *     packet counts in `packets` and, in this order:
 *     1. takes the TS monitor's continuity step.  DUPLICATE: counted in duplicates, nothing more of the packet is used.  CC_ERROR
 *        (counted in cc_errors) or an announced discontinuity: a RESET.
 *     2. No payload (AFC&1 clear): done.
 *     3. AFC = 3 and b4 (adaptation_field_length) > 182: malformed_packets, a reset, done.
 *     4. The payload is L bytes at 188 - L (184, or 183 - b4).  L adds to payload_bytes.
 *     5. TSC != 0: scrambled_packets, a reset, and the payload is not read.  With PUSI the packet still takes the start rule (kind
 *        SCRAMBLED); without, it is done.
 *     6. PUSI set: a START.
 *     7. Otherwise, if the slot is synced, the whole payload is the packet's SEGMENT of ES bytes; if not, L adds to bytes_unsynced.
 *     A reset: have := 0 and the slot's `lost` bit is set.  It does not unsync the slot.  `resets` counts the packets that reset (once
 *     each, whatever the number of reasons).
 *   Start: the kind, stream_id, PES_packet_length, PTS and DTS are those of the PES bank's start rule (above), not restated.  The start
 *     is VALID when its kind is HEADER and 9 + PES_header_data_length <= L: its segment is payload[9 + hdl .. L), which may be empty, and
 *     the slot is synced.  A valid start does NOT reset: the ES is contiguous across PES packets and a start code may straddle them.
 *     Every other start is invalid (pes_invalid): the slot is UNSYNCED, the scanner is reset and nothing of the payload is scanned; a
 *     HEADER whose header runs beyond the packet (legal and rare) has the flag SPLIT_HEADER (split_headers).  One row with unit PES per
 *     start, valid or not; the invalid start's reset comes behind its row.
 *   Scanner: per slot es_count (64 bits: the ES bytes accepted since the watch was set), the last 7 accepted bytes and have = min(7,
 *     bytes accepted since the last reset).  For every accepted byte in order: if have = 7, the 8-byte window is the 7 kept bytes plus
 *     this one, w0..w7; if w0 w1 w2 = 00 00 01 a CODE has been found with code = w3 and head = w4 w5 w6 w7 (w4 in the high byte), at
 *     es_offset = es_count - 7, the position of w0; `codes` counts it.  Then the byte is appended.  So whether a code is found is a
 *     pure function of the last 8 ES bytes: a code whose four head bytes never arrive (reset, end of stream) is never reported,
 *     emulation-prevention bytes inside the head are not removed, the leading zero of a 4-byte start code is not looked at.
 *   Classification by the slot's codec; a code without a row is only counted:
 *     MPEG2  code 00: PICTURE, detail from head >> 19 & 7 (1 I, 2 P, 3 B, else 0), KEY when I; B3: SEQUENCE; B8: GOP; B7: END; 01..AF:
 *            slices; anything else: other_codes.
 *     H264   code & 0x80: bad_codes.  t = code & 31: 1 or 5 with head >> 31 set (first_mb_in_slice = 0): PICTURE, KEY when t = 5, detail
 *            from slice_type, the ue(v) in the 7 bits behind that bit (0 to 3 leading zeros, values 0..14): mod 5 = 0 P, 1 B, 2 I; SP, SI,
 *            values above 9 and more leading zeros give 0.  1 or 5 with the bit clear: slices.  7: SEQUENCE; 8: PARAM; 9: AUD; 10 or 11:
 *            END; anything else: other_codes.
 *     H265   code & 0x80, or head >> 24 & 7 = 0 (nuh_temporal_id_plus1): bad_codes.  t = code >> 1 & 63: 0..9 or 16..21 with head >> 23 & 1
 *            set (first_slice_segment_in_pic_flag): PICTURE, t >= 16: KEY and detail I, else detail 0; with the bit clear: slices.
 *            33: SEQUENCE; 32 or 34: PARAM; 35: AUD; 36 or 37: END; anything else: other_codes.
 *   Row: `packet` of a code row is the packet that holds the window's LAST byte.  RESYNC is set on the first row a slot issues after
 *     `lost` was set, and clears it.  Order: by packet in input order across the slots; within a packet the PES row first, then the code
 *     rows by the completing byte's place.  The join: a code belongs to the last PES row of its slot, in row order, whose es_offset is <=
 *     its own -- per-picture PTS and picture sizes (differences of es_offset) without any carried timestamp.  The table holds the first
 *     max_rows rows of a call; out_rows[] carries the true count, rows_dropped accumulates the excess, the counters cover everything.
 *   State survives from call to call.  reset forgets it (positions and counters too; the watches stay).
 *   Limits: max_packets <= 4096 per stream and call, as in the PES bank: the banks chain on the same buffers.  Memory (device banks) per
 *     stream: 384 bytes of state, 128 of watches, 48 bytes per row of max_rows and a call record of 1680 bytes.
 *   NOT done: reassembly of split PES headers; parsing behind the four head bytes (SPS sizes, slice types of H.265, SEI); removal of
 *     emulation-prevention bytes; copying pictures out.  Audio PIDs are the audio bank's (below). */
typedef struct dvbs2gpu_es dvbs2gpu_es;
int dvbs2gpu_es_create(dvbs2gpu_ctx* ctx, int nstreams, int max_packets, int max_rows, dvbs2gpu_es** out);
/* a bank without a device: the library's native host implementation of the same rules, behind dvbs2gpu_es_work only */
int dvbs2gpu_es_create_host(int nstreams, int max_packets, int max_rows, dvbs2gpu_es** out);
int dvbs2gpu_es_reset(dvbs2gpu_es* b);
void dvbs2gpu_es_destroy(dvbs2gpu_es* b);
#define DVBS2GPU_ES_MPEG2 1
#define DVBS2GPU_ES_H264 2
#define DVBS2GPU_ES_H265 3
/* slot 0..15; pid 0..0x1FFE with a codec, or -1: the slot watches nothing (the codec is ignored) */
int dvbs2gpu_es_set_watch(dvbs2gpu_es* b, int stream, int slot, int pid, int codec);
/* d_ts[i]: DEVICE pointer to nbytes[i] bytes (a multiple of 188, at most 188*max_packets) of stream i, of any alignment.  out_rows
 * (host, may be NULL): the rows of the call per stream, of which the table holds the first max_rows.  One kernel launch.
 * Synchronous on `stream`; chained behind a packetiser or monitor call on the same stream, no packet visits the host. */
int dvbs2gpu_es_process_batch(dvbs2gpu_es* b, const uint8_t* const* d_ts, const int* nbytes, int* out_rows, void* stream);
/* one stream of any bank with a HOST buffer: returns the rows of the call or a negative error.  The other streams of the bank receive
 * an empty call. */
int dvbs2gpu_es_work(dvbs2gpu_es* b, int stream, const uint8_t* h_ts, int nbytes);
typedef struct dvbs2gpu_es_stats {             /* of a slot, since creation, reset or the slot's last set_watch; kept on the host */
    int64_t packets;                 /* trusted packets of the watched PID, duplicates among them */
    int64_t payload_bytes, es_bytes, bytes_unsynced, duplicates, cc_errors, scrambled_packets, malformed_packets, resets;
    int64_t pes_starts, pes_invalid, split_headers;
    int64_t codes;                   /* every code found; the sum of the counters from `pictures` on but the four picture kinds */
    int64_t pictures, pictures_i, pictures_p, pictures_b, key_pictures;
    int64_t sequences, gops, params, auds, ends, slices, other_codes, bad_codes;
} dvbs2gpu_es_stats;
/* slot -1: the sum over the stream's slots */
int dvbs2gpu_es_get_stats(dvbs2gpu_es* b, int stream, int slot, dvbs2gpu_es_stats* h_out);
typedef struct dvbs2gpu_es_stream_stats {
    int64_t packets;                 /* every 188 bytes handed in: the position of the next packet */
    int64_t rows_dropped;
} dvbs2gpu_es_stream_stats;
int dvbs2gpu_es_get_stream_stats(dvbs2gpu_es* b, int stream, dvbs2gpu_es_stream_stats* h_out);
#define DVBS2GPU_ES_UNIT_PES 0
#define DVBS2GPU_ES_UNIT_PICTURE 1
#define DVBS2GPU_ES_UNIT_SEQUENCE 2
#define DVBS2GPU_ES_UNIT_GOP 3
#define DVBS2GPU_ES_UNIT_PARAM 4
#define DVBS2GPU_ES_UNIT_AUD 5
#define DVBS2GPU_ES_UNIT_END 6
#define DVBS2GPU_ES_KEY 1
#define DVBS2GPU_ES_RESYNC 2
#define DVBS2GPU_ES_UNSYNCED 4
#define DVBS2GPU_ES_SPLIT_HEADER 8
#pragma pack(push, 4)
typedef struct dvbs2gpu_es_row {               /* 48 bytes */
    uint16_t pid;                    /* offset 0 */
    uint8_t slot, unit;              /* 2, 3: DVBS2GPU_ES_UNIT_PES .. DVBS2GPU_ES_UNIT_END */
    uint8_t code;                    /* 4: the code byte; PES rows: stream_id */
    uint8_t detail;                  /* 5: the picture type (1 I, 2 P, 3 B, 0 unknown); PES rows: the PES bank's kind */
    uint16_t flags;                  /* 6 */
    int32_t packet;                  /* 8: index in this call of the packet that holds the window's last byte; PES rows: the start */
    uint32_t head;                   /* 12: the four bytes behind the code byte; PES rows: PES_packet_length */
    uint64_t es_offset;              /* 16: of the code's first byte; PES rows: es_count before the start's segment */
    uint64_t pts, dts;               /* 24, 32: PES rows; all ones: absent, and in code rows */
    uint64_t reserved;               /* 40 */
} dvbs2gpu_es_row;
#pragma pack(pop)
/* h_rows[cap] (host); *n = rows of the last call in the table, of which min(*n, cap) are written */
int dvbs2gpu_es_get_row_table(dvbs2gpu_es* b, int stream, dvbs2gpu_es_row* h_rows, int cap, int* n);
/* the same table in HBM, valid until the bank's next call (device banks only): *d_rows is a DEVICE pointer (NULL when *n == 0) */
int dvbs2gpu_es_get_row_table_device(dvbs2gpu_es* b, int stream, const dvbs2gpu_es_row** d_rows, int* n);

/* ------------------------------------------------------------------ Audio bank (own extension)
 * Nothing in the reference does this.  For `nstreams` transport streams in HBM a bank follows the frames of up to 16 watched audio PIDs
 * per stream -- MPEG-1/2/2.5 audio layers I-III, AAC in ADTS, AC-3 and E-AC-3 -- and writes one table row per PES packet start, one
 * per frame (codec sub-kind, channel mode, sample rate, samples, bitrate, size, position in the elementary stream) and one per loss of
 * framing, so that a frame's PTS is that of the PES row in front of it and "is the framing intact" is a counter.  The sequential form
 * below is the definition (csrc/aud_rules.h, AudHostStream::run); no result depends on how a stream is cut into calls or on the
 * alignment of the input.  The header syntax is written from memory of ISO/IEC 11172-3, 13818-3, 13818-7 and ETSI TS 102 366 and
 * pinned to no vector of theirs.
 *   Watches: 16 slots per stream, each empty or a PID 0..0x1FFE with a codec: DVBS2GPU_AUD_MPA, _ADTS, _AC3 (E-AC-3 too: told apart by
 *     bsid).  A new bank watches nothing.  The same PID in two slots of a stream is an argument error.  Setting a watch starts the slot
 *     afresh, state and counters.
 *   Packet, start and segment: exactly steps 1-7 and the start rule of the ES bank (above), not restated: trusted packets of watched
 *     PIDs, the continuity step, duplicates ignored, CC_ERROR / DISC / malformed / scrambled -> a RESET, a valid PES start opens a
 *     segment and does not reset, an invalid start unsyncs the slot, SPLIT_HEADER, one PES row per start, bytes_unsynced.
 *   Accepted bytes: es_count, the last 7 accepted bytes and have as in the ES bank.  For every accepted byte with have = 7 the window
 *     w0..w7 lies at ES position q = es_count - 7.
 *   Framer: per slot `locked`, `next` (a 64-bit ES position) and `params` (the previous frame's parameter word; none since the
 *     acquisition).
 *     Acquire: a VALID start that finds the slot not locked sets locked, next := the ES position of its segment's first byte
 *       (acquisitions), and the coming FRAME or LOSS row is marked ACQUIRED.  Nothing is acquired elsewhere: lock is taken at PES payload
 *       starts only -- a departure from a free-running sync search, and what PES-aligned broadcast audio needs -- so that sync words
 *       inside payloads never count and no result depends on the cut into calls.
 *     Check: when locked and q = next, the window is parsed (below).  Valid: a FRAME row at es_offset = q, next += frame_bytes, and
 *       CHANGE if the parameter word differs from params (never on the first frame after an acquisition; param_changes).  Invalid: a LOSS
 *       row (es_offset = q, head = w0..w3), locked := 0, sync_losses.  A byte accepted while not locked adds to bytes_unlocked (the byte
 *       that completes a failing window was accepted while locked).
 *     A reset and an invalid start unlock without a row (and set `lost`: RESYNC on the next row, as in the ES bank).  A valid start
 *       while locked whose segment does not begin at next counts unaligned_starts and changes nothing: frames may straddle PES packets.
 *     A frame is reported by the packet that holds w7; a frame whose 8th byte never arrives is never reported.  next may lie any
 *       distance beyond the bytes received.  frame_bytes >= 7 and a LOSS unlocks: a packet yields at most 27 FRAME / LOSS rows.
 *   Parse, a pure function of the 8 bytes and the slot's codec:
 *     MPA   w0..w3 as the 32-bit header: 11 sync bits; version 3 MPEG-1, 2 MPEG-2, 0 MPEG-2.5, 1 invalid; layer 3 I, 2 II, 1 III, 0
 *           invalid; bitrate index 0 (free format) and 15 invalid, sampling index 3 invalid.  kbps by index 1..14 -- V1 L1 32..448 in
 *           steps of 32; V1 L2 32 48 56 64 80 96 112 128 160 192 224 256 320 384; V1 L3 32 40 48 56 64 80 96 112 128 160 192 224 256
 *           320; V2/2.5 L1 32 48 56 64 80 96 112 128 144 160 176 192 224 256; V2/2.5 L2, L3 8 16 24 32 40 48 56 64 80 96 112 128 144
 *           160.  fs 44100 / 48000 / 32000, halved for V2, quartered for V2.5.  Bytes (integer floor): L1 (12 br / fs + pad) 4; L2 and
 *           L3 of V1 144 br / fs + pad; L3 of V2/2.5 72 br / fs + pad.  Samples 384 / 1152 / 576 likewise.  code = version << 2 | layer
 *           (the header's bits), detail = mode (0 stereo, 1 joint, 2 dual, 3 mono).
 *     ADTS  12 sync bits, layer bits 0, sampling_frequency_index <= 12 (96000 88200 64000 48000 44100 32000 24000 22050 16000 12000
 *           11025 8000 7350); aac_frame_length: 13 bits, the low 2 of w3, w4, the top 3 of w5, valid when >= 7 (>= 9 with
 *           protection_absent = 0); samples 1024 (blocks + 1), blocks the low 2 bits of w6.  code = ID << 2 | profile, detail =
 *           channel_configuration.
 *     AC3   w0 w1 = 0B 77; bsid the top 5 bits of w5.  bsid <= 10, AC-3: fscod (top 2 bits of w4) 3 invalid, frmsizecod (the low 6)
 *           > 37 invalid; br = 32 40 48 56 64 80 96 112 128 160 192 224 256 320 384 448 512 576 640 [frmsizecod >> 1]; 16-bit words:
 *           2 br at 48 k, 3 br at 32 k, floor(320 br / 147) + (frmsizecod & 1) at 44.1 k; bytes twice that, samples 1536; detail =
 *           acmod.  bsid 11..16, E-AC-3: bytes 2 (frmsiz + 1), frmsiz the 11 bits behind strmtyp and substreamid, invalid under 7;
 *           fscod 3 selects fscod2 (24000 22050 16000, 6 blocks, 3 invalid), else numblkscod 1 2 3 6 blocks; samples 256 blocks;
 *           detail = acmod | lfeon << 3.  Any other bsid: invalid.  code = bsid.
 *     kbps of ADTS and E-AC-3, whose headers name none: floor(8 frame_bytes fs / (1000 samples)).  The parameter word holds everything
 *     named here but padding and length (the MPA mode extension, private and copyright bits are not parameters).
 *   Row: `packet` of a FRAME or LOSS row is the packet that holds w7.  Order: by packet in input order across the slots; within a
 *     packet the PES row first, then by the completing byte's place.  The joins are the ES bank's: a frame belongs to the last PES row
 *     of its slot whose es_offset is <= its own (its PTS; the first frame of an aligned PES packet has exactly that offset), and a
 *     frame's size is also the difference of neighbouring offsets.  The table holds the first max_rows rows of a call; out_rows[]
 *     carries the true count, rows_dropped accumulates the excess, the counters cover everything.
 *   State (32 bytes per slot) survives from call to call.  reset forgets it (positions and counters too; the watches stay).
 *   Limits: max_packets <= 4096 per stream and call, as in the ES bank: the banks chain on the same buffers.  Memory (device banks) per
 *     stream: 512 bytes of state, 128 of watches, 48 bytes per row of max_rows and a call record of 1296 bytes.
 *   NOT done: a sync search outside PES starts (a PID whose PES packets never begin with a frame is never locked); LATM/LOAS, DTS,
 *     AC-4; free-format MPA; CRC checks of frames; a check of the PTS step against the frames' duration; copying frames out.  DVB's AC-3
 *     in private stream type 0x06 is told by a descriptor, which the PSI bank's PMT view does not carry: the caller names such a PID
 *     with set_watch. */
typedef struct dvbs2gpu_aud dvbs2gpu_aud;
int dvbs2gpu_aud_create(dvbs2gpu_ctx* ctx, int nstreams, int max_packets, int max_rows, dvbs2gpu_aud** out);
/* a bank without a device: the library's native host implementation of the same rules, behind dvbs2gpu_aud_work only */
int dvbs2gpu_aud_create_host(int nstreams, int max_packets, int max_rows, dvbs2gpu_aud** out);
int dvbs2gpu_aud_reset(dvbs2gpu_aud* b);
void dvbs2gpu_aud_destroy(dvbs2gpu_aud* b);
#define DVBS2GPU_AUD_MPA 1
#define DVBS2GPU_AUD_ADTS 2
#define DVBS2GPU_AUD_AC3 3
/* slot 0..15; pid 0..0x1FFE with a codec, or -1: the slot watches nothing (the codec is ignored) */
int dvbs2gpu_aud_set_watch(dvbs2gpu_aud* b, int stream, int slot, int pid, int codec);
/* d_ts[i]: DEVICE pointer to nbytes[i] bytes (a multiple of 188, at most 188*max_packets) of stream i, of any alignment.  out_rows
 * (host, may be NULL): the rows of the call per stream, of which the table holds the first max_rows.  One kernel launch.
 * Synchronous on `stream`; chained behind a packetiser or monitor call on the same stream, no packet visits the host. */
int dvbs2gpu_aud_process_batch(dvbs2gpu_aud* b, const uint8_t* const* d_ts, const int* nbytes, int* out_rows, void* stream);
/* one stream of any bank with a HOST buffer: returns the rows of the call or a negative error.  The other streams of the bank receive
 * an empty call. */
int dvbs2gpu_aud_work(dvbs2gpu_aud* b, int stream, const uint8_t* h_ts, int nbytes);
typedef struct dvbs2gpu_aud_stats {            /* of a slot, since creation, reset or the slot's last set_watch; kept on the host */
    int64_t packets;                 /* trusted packets of the watched PID, duplicates among them */
    int64_t payload_bytes, es_bytes, bytes_unsynced, duplicates, cc_errors, scrambled_packets, malformed_packets, resets;
    int64_t pes_starts, pes_invalid, split_headers;
    int64_t frames, frame_bytes_total, samples_total;   /* FRAME rows, and the sums of their frame_bytes and samples */
    int64_t acquisitions, sync_losses, param_changes, unaligned_starts, bytes_unlocked;
} dvbs2gpu_aud_stats;
/* slot -1: the sum over the stream's slots */
int dvbs2gpu_aud_get_stats(dvbs2gpu_aud* b, int stream, int slot, dvbs2gpu_aud_stats* h_out);
typedef struct dvbs2gpu_aud_stream_stats {
    int64_t packets;                 /* every 188 bytes handed in: the position of the next packet */
    int64_t rows_dropped;
} dvbs2gpu_aud_stream_stats;
int dvbs2gpu_aud_get_stream_stats(dvbs2gpu_aud* b, int stream, dvbs2gpu_aud_stream_stats* h_out);
#define DVBS2GPU_AUD_UNIT_PES 0
#define DVBS2GPU_AUD_UNIT_FRAME 1
#define DVBS2GPU_AUD_UNIT_LOSS 2
#define DVBS2GPU_AUD_ACQUIRED 1
#define DVBS2GPU_AUD_RESYNC 2
#define DVBS2GPU_AUD_UNSYNCED 4
#define DVBS2GPU_AUD_SPLIT_HEADER 8
#define DVBS2GPU_AUD_CHANGE 16
#pragma pack(push, 4)
typedef struct dvbs2gpu_aud_row {              /* 48 bytes, laid out like dvbs2gpu_es_row (packet in 16 bits: it is below 4096) */
    uint16_t pid;                    /* offset 0 */
    uint8_t slot, unit;              /* 2, 3: DVBS2GPU_AUD_UNIT_PES, _FRAME, _LOSS */
    uint8_t code;                    /* 4: the codec's sub-kind (see Parse); PES rows: stream_id */
    uint8_t detail;                  /* 5: the channel mode (see Parse); PES rows: the PES bank's kind */
    uint16_t flags;                  /* 6 */
    uint16_t packet;                 /* 8: index in this call of the packet that holds w7; PES rows: the start */
    uint16_t kbps;                   /* 10: FRAME rows */
    uint32_t head;                   /* 12: w0..w3, w0 in the high byte; PES rows: PES_packet_length */
    uint64_t es_offset;              /* 16: of w0; PES rows: es_count before the start's segment */
    uint64_t pts, dts;               /* 24, 32: PES rows; all ones: absent, and in FRAME and LOSS rows */
    uint32_t sample_rate;            /* 40: FRAME rows, Hz */
    uint16_t frame_bytes, samples;   /* 44, 46: FRAME rows */
} dvbs2gpu_aud_row;
#pragma pack(pop)
/* h_rows[cap] (host); *n = rows of the last call in the table, of which min(*n, cap) are written */
int dvbs2gpu_aud_get_row_table(dvbs2gpu_aud* b, int stream, dvbs2gpu_aud_row* h_rows, int cap, int* n);
/* the same table in HBM, valid until the bank's next call (device banks only): *d_rows is a DEVICE pointer (NULL when *n == 0) */
int dvbs2gpu_aud_get_row_table_device(dvbs2gpu_aud* b, int stream, const dvbs2gpu_aud_row** d_rows, int* n);

/* ------------------------------------------------------------------ T2-MI bank (own extension)
 * Nothing in the reference does this.  A DVB-S2 carrier may carry a T2-MI stream (ETSI TS 102 773, the DVB-T2 modulator interface) on
 * one PID of an otherwise empty transport stream; the services lie one level down, in the DVB-T2 BBFRAMEs that the T2-MI packets hold.
 * For `nstreams` transport streams in HBM a bank reassembles the T2-MI packets of a PID, checks their CRC-32 and packet count, writes
 * one table row per T2-MI packet and lays the BBFRAMEs of the chosen PLP back to back in a device buffer: with their sizes
 * (dvbs2gpu_t2mi_get_frame_bytes) these are the d_bb[i], frame_bytes[i] and nframes[i] of dvbs2gpu_bbts_process_ma_batch.  The
 * sequential form below is the definition (csrc/t2mi_rules.h, T2miHostStream::run); the kernels give its results for every cutting
 * of a stream into calls.  The syntax is written from memory of TS 102 773; it is one struct, dvbs2gpu_t2mi_layout.
 *   T2-MI packet: bytes b0..b5, the payload, the CRC.  packet_type = b0, packet_count = b1, superframe_idx = b2 >> 4, t2mi_stream_id =
 *     b3 & 7 (the 9 bits between are rfu), payload_bits = b4 << 8 | b5.  total = 6 + ((payload_bits + 7) >> 3) + 4 bytes, 10 .. 8202.
 *     The last four bytes are a CRC-32/MPEG (initial value 0xFFFFFFFF, polynomial 0x04C11DB7) over everything before them: a packet is
 *     valid when the register over all `total` bytes is 0.  Every 16-bit length is legal: no header is malformed.
 *   BBFRAME payload (packet_type 0x00): payload byte 0 frame_idx, byte 1 plp_id, byte 2 >> 7 intl_frame_start; the BBFRAME follows from
 *     payload byte 3 and holds (payload_bits - 24) / 8 bytes.  Well-formed: payload_bits >= 24 + 80, (payload_bits - 24) % 8 == 0 and
 *     the BBFRAME at most 7274 bytes (Kbch 58 192); otherwise the row has BAD_PAYLOAD and nothing is delivered.
 *   Watches: 4 slots per stream, each empty or a pair (PID 0..0x1FFE, PLP -1 for every PLP or 0..255).  A new bank watches nothing.
 *     Unlike the other banks THE SAME PID MAY SIT IN SEVERAL SLOTS of a stream (two PLPs of one feed): every slot is a complete,
 *     independent reassembler with its own state, counters, rows and output buffer.  Changing a slot's watch starts it afresh.
 *   Packet: 188 bytes at offset 188 k, classified as the TS monitor does: sync-byte errors, TEI packets and null packets are not looked
 *     at.  A packet of the slot's PID counts in `packets` and, in this order ("drop" = the open T2-MI packet is forgotten; with fill > 0
 *     it counts in dropped_packets):
 *     1. TSC != 0: scrambled_packets, drop, the continuity step; done.
 *     2. The continuity step (dvbs2gpu_tsmon_*: one state byte per slot).  Duplicate: ignored.  Continuity error or announced
 *        discontinuity: drop, then go on with this packet.  No payload (AFC&1 = 0): done.
 *     3. The payload starts at 4, or at 5 + b4 when AFC&2.  >= 188: malformed_packets, drop, done.
 *     4. PUSI set: ptr = the first payload byte.  ptr > the bytes after it: malformed_packets, drop, done.  The ptr bytes after the
 *        pointer go to an open packet: if they complete it, it is emitted, and what is left of them is ignored and counts once in
 *        pointer_slack if not empty; if it is still incomplete after them (an open header of fewer than six bytes too) it is dropped;
 *        with nothing open they are ignored.  Then packet starts are parsed behind them (6).
 *     5. PUSI clear: the whole payload goes to an open packet; if it completes it, it is emitted and the rest of the payload is
 *        ignored.  With nothing open the payload is ignored.
 *     6. At a packet start, until the TS packet ends: bytes are buffered; with six, total is known; when the buffered bytes reach
 *        total the packet is emitted and the next byte is a packet start.  There is no stuffing rule: every byte behind a start is a
 *        header byte.  A packet, or a header of one to five bytes, that the TS packet's end cuts stays open, across calls too.
 *   Emitting: one row per emitted packet, valid or not; it counts in t2mi_packets.  CRC not zero: flag CRC_ERROR, crc_errors, and
 *     nothing more of the packet is used (plp_id, frame_idx and bbframe_bytes are 0).  A valid packet steps the packet-count check
 *     (state per slot: has_count, last_count): with has_count set and packet_count != (last_count + 1) & 255 the row has COUNT_ERROR
 *     and count_errors counts; then last_count := packet_count.  This runs over all packet types and all t2mi_stream_ids of the PID.
 *     A valid packet of type 0x00 with a well-formed payload has BBFRAME (and INTL_FRAME_START where that bit is set) and counts in
 *     bbframes; one with another payload has BAD_PAYLOAD and counts in bad_payload.  A BBFRAME packet is delivered when the call has
 *     output buffers and the slot's PLP is -1 or equals plp_id: its BBFRAME bytes go to the slot's output buffer, back to back in row
 *     order, row.offset and row.bbframe_bytes name them, bbframes_delivered and bytes_delivered count.  Every other row has offset -1.
 *   Row: ordered by the TS packet that held the T2-MI packet's last byte, then by position in it.  One table per (stream, slot).
 *   Capacity: sizes first.  If a slot's bytes exceed cap or its rows exceed max_rows the call returns DVBS2GPU_ERR_CAPACITY,
 *     out_bytes[] holds the byte sizes (-1 for a slot whose rows did not fit: its packets were not checked) and out_rows[] the row
 *     counts; no state or counter of any stream has advanced, the tables of the call are empty, the call can be repeated.
 *   State survives from call to call.  reset forgets state, positions and counters; watches stay.
 *   Limits: max_packets <= 4096 per stream and call.  Memory (device banks) per (stream, slot): an 8208-byte packet buffer, 6 bytes per
 *     packet of max_packets and 52 bytes per row of max_rows. */
typedef struct dvbs2gpu_t2mi dvbs2gpu_t2mi;
typedef struct dvbs2gpu_t2mi_layout {
    int32_t header_bytes, crc_bytes, min_packet_bytes, max_packet_bytes, bbframe_type, bbframe_prefix_bytes, min_bbframe_bytes,
            max_bbframe_bytes, stream_id_mask;
} dvbs2gpu_t2mi_layout;
int dvbs2gpu_t2mi_create(dvbs2gpu_ctx* ctx, int nstreams, int max_packets, int max_rows, dvbs2gpu_t2mi** out);
/* a bank without a device: the library's native host implementation of the same rules, behind dvbs2gpu_t2mi_work only */
int dvbs2gpu_t2mi_create_host(int nstreams, int max_packets, int max_rows, dvbs2gpu_t2mi** out);
int dvbs2gpu_t2mi_reset(dvbs2gpu_t2mi* b);
void dvbs2gpu_t2mi_destroy(dvbs2gpu_t2mi* b);
int dvbs2gpu_t2mi_get_layout(dvbs2gpu_t2mi_layout* h_out);
/* slot 0..3; pid 0..0x1FFE, or -1: the slot is empty; plp 0..255, or -1: every PLP */
int dvbs2gpu_t2mi_set_watch(dvbs2gpu_t2mi* b, int stream, int slot, int pid, int plp);
/* d_ts[i]: DEVICE pointer to nbytes[i] bytes (a multiple of 188, at most 188*max_packets) of stream i, of any alignment.  d_out NULL:
 * rows and counters only (never a capacity failure for bytes; out_bytes may be NULL).  Else d_out[i*4 + k]: DEVICE buffer of cap bytes
 * for the BBFRAMEs of slot k of stream i (NULL for an empty slot); out_bytes[i*4 + k] (host) their bytes.  out_rows[i*4 + k] (host, may
 * be NULL): the row counts.  Two kernel launches.  Synchronous on `stream`; chained behind a packetiser or monitor call and in front of
 * dvbs2gpu_bbts_process_ma_batch on the same stream, no packet visits the host. */
int dvbs2gpu_t2mi_process_batch(dvbs2gpu_t2mi* b, const uint8_t* const* d_ts, const int* nbytes, uint8_t* const* d_out, int cap, int* out_bytes,
                                int* out_rows, void* stream);
/* one stream and slot of any bank with HOST buffers (h_out NULL: rows and counters only): returns the bytes written to h_out or a
 * negative error.  Every other slot of the bank receives an empty call. */
int dvbs2gpu_t2mi_work(dvbs2gpu_t2mi* b, int stream, int slot, const uint8_t* h_ts, int nbytes, uint8_t* h_out, int cap);
/* the byte and row sizes that the slot's last call needed, whether it succeeded or failed for capacity */
int dvbs2gpu_t2mi_get_needed(dvbs2gpu_t2mi* b, int stream, int slot, int* bytes, int* rows);
typedef struct dvbs2gpu_t2mi_stats {           /* of a slot, since creation, reset or the slot's last set_watch; kept on the host */
    int64_t packets;                 /* trusted TS packets of the slot's PID */
    int64_t t2mi_packets;            /* rows */
    int64_t crc_errors, count_errors;
    int64_t bbframes, bad_payload;   /* valid packets of type 0x00 with a well-formed / another payload */
    int64_t bbframes_delivered, bytes_delivered;
    int64_t dropped_packets;         /* open T2-MI packets forgotten */
    int64_t malformed_packets, scrambled_packets;   /* TS packets */
    int64_t pointer_slack;           /* PUSI packets whose pointer bytes went on behind the end of the packet they completed */
} dvbs2gpu_t2mi_stats;
/* slot -1: the sum over the stream's slots */
int dvbs2gpu_t2mi_get_stats(dvbs2gpu_t2mi* b, int stream, int slot, dvbs2gpu_t2mi_stats* h_out);
#define DVBS2GPU_T2MI_CRC_ERROR 1
#define DVBS2GPU_T2MI_COUNT_ERROR 2
#define DVBS2GPU_T2MI_BBFRAME 4
#define DVBS2GPU_T2MI_INTL_FRAME_START 8
#define DVBS2GPU_T2MI_BAD_PAYLOAD 16
typedef struct dvbs2gpu_t2mi_row {             /* 32 bytes */
    uint8_t packet_type, packet_count, superframe_idx, stream_id;
    uint16_t flags;
    uint8_t plp_id, frame_idx;       /* of a valid packet of type 0x00 with payload_bits >= 24, else 0 */
    uint32_t payload_bits;
    int32_t length;                  /* total bytes */
    int32_t offset;                  /* of the BBFRAME in the slot's output buffer; -1: not delivered */
    int32_t bbframe_bytes;           /* of a BBFRAME row, delivered or not; else 0 */
    int32_t first_packet;            /* index in this call of the TS packet that held its first byte; -1: an earlier call */
    int32_t last_packet;             /* and of the one that held its last byte */
} dvbs2gpu_t2mi_row;
/* h_rows[cap] (host); *n = rows of the slot's last call, of which min(*n, cap) are written */
int dvbs2gpu_t2mi_get_row_table(dvbs2gpu_t2mi* b, int stream, int slot, dvbs2gpu_t2mi_row* h_rows, int cap, int* n);
/* the same table in HBM, valid until the bank's next call (device banks only): *d_rows is a DEVICE pointer (NULL when *n == 0) */
int dvbs2gpu_t2mi_get_row_table_device(dvbs2gpu_t2mi* b, int stream, int slot, const dvbs2gpu_t2mi_row** d_rows, int* n);
/* h_sizes[cap] (host): the sizes of the BBFRAMEs that the slot's last call delivered, in order; *n = how many there are.  With the
 * slot's output buffer: d_bb[i], frame_bytes[i] and nframes[i] of dvbs2gpu_bbts_process_ma_batch. */
int dvbs2gpu_t2mi_get_frame_bytes(dvbs2gpu_t2mi* b, int stream, int slot, int* h_sizes, int cap, int* n);

/* ------------------------------------------------------------------ MPE bank (own extension)
 * Nothing in the reference does this.  A transport-stream carrier may carry IP by Multi-Protocol Encapsulation (ETSI EN 301 192
 * section 7): IP datagrams inside DSM-CC datagram_sections (table_id 0x3E) on one or more PIDs.  For `nstreams` transport streams in
 * HBM a bank reassembles the sections of a PID, checks their CRC-32, applies a MAC address filter, finds the IPv4 or IPv6 datagram
 * behind the MPE header (and LLC/SNAP), checks its header, writes one table row per section and lays the datagrams back to back in a
 * device buffer.  The sequential form below is the definition (csrc/mpe_rules.h, MpeHostStream::run); the kernels give its results
 * for every cutting of a stream into calls.  The syntax is written from memory of EN 301 192, RFC 791, RFC 8200 and RFC 1042; it is
 * one struct, dvbs2gpu_mpe_layout.
 *   Section: bytes b0 b1 b2, then section_length = (b1 << 8 | b2) & 0x0FFF more bytes: total = 3 + section_length <= 4096.
 *     section_length > 4093 is the bad length.  datagram_section (b0 = 0x3E): b3 MAC_address_6, b4 MAC_address_5, b5 = 2 reserved |
 *     payload_scrambling_control 2 | address_scrambling_control 2 | LLC_SNAP_flag | current_next, b6 section_number,
 *     b7 last_section_number, b8 .. b11 MAC_address_4 .. MAC_address_1, the body from b12, the last four bytes a CRC-32/MPEG (initial
 *     value 0xFFFFFFFF, polynomial 0x04C11DB7; the register over all `total` bytes is 0) when section_syntax_indicator (b1 >> 7) is
 *     set, else a checksum.
 *   Watches: 4 slots per stream, each empty (pid -1) or (PID 0..0x1FFE, mac_value[6], mac_mask[6]) in network order; an all-zero mask
 *     means every address.  A new bank watches nothing.  THE SAME PID MAY SIT IN SEVERAL SLOTS of a stream (two MAC filters on one
 *     PID): every slot is a complete, independent reassembler with its own state, counters, rows and output buffer.  Changing a slot's
 *     watch starts it afresh.
 *   Packet: 188 bytes at offset 188 k, classified as the TS monitor does: sync-byte errors, TEI packets and null packets are not looked
 *     at.  A packet of the slot's PID counts in `packets` and, in this order ("drop" = the open section is forgotten; with fill > 0 it
 *     counts in dropped_sections) -- the rules of the PSI section bank, one slot per reassembler:
 *     1. TSC != 0: scrambled_packets, drop, the continuity step; done.
 *     2. The continuity step (dvbs2gpu_tsmon_*: one state byte per slot).  Duplicate: ignored.  Continuity error or announced
 *        discontinuity: drop, then go on with this packet.  No payload (AFC&1 = 0): done.
 *     3. The payload starts at 4, or at 5 + b4 when AFC&2.  >= 188: malformed_packets, drop, done.
 *     4. PUSI set: ptr = the first payload byte.  ptr > the bytes after it: malformed_packets, drop, done.  The ptr bytes after the
 *        pointer go to an open section: if they complete it, it is emitted and what is left of them is ignored; if it is still
 *        incomplete after them (an open header of one or two bytes too) it is dropped; if they complete a header with the bad length,
 *        malformed_sections counts and the header is forgotten; with nothing open they are ignored.  Then section starts are parsed
 *        behind them (6).
 *     5. PUSI clear: the whole payload goes to an open section; if it completes it, it is emitted and the rest of the payload is
 *        ignored; a header completed with the bad length counts in malformed_sections and is forgotten.  With nothing open the
 *        payload is ignored.
 *     6. At a section start, until the TS packet ends: the byte 0xFF is stuffing and ends the packet's chain.  Else bytes are buffered;
 *        with three, total is known: the bad length counts in malformed_sections, forgets the header and ends the packet's chain; when
 *        the buffered bytes reach total the section is emitted and the next byte is a section start.  A section, or a header of one or
 *        two bytes, that the TS packet's end cuts stays open, across calls too.
 *   Emitting: every emitted section is one row and counts in `sections`.  In this order; the first rule that fires ends the list (but
 *     UNCHECKED, which goes on), and the fields of the row that later rules would set are 0:
 *     1. b0 != 0x3E: flag OTHER_TABLE, other_table.  No CRC is taken.
 *     2. total < 16 (12 header bytes + 4): flag MALFORMED, malformed_sections.
 *     3. section_syntax_indicator set: the CRC-32 over all bytes must be 0, else flag CRC_ERROR, crc_errors.  Clear: the last four
 *        bytes are a checksum of ISO/IEC 13818-6 whose definition is not at hand; it is NOT verified: flag UNCHECKED, `unchecked`,
 *        and the list goes on.
 *     4. mac[0..5] = b11, b10, b9, b8, b4, b3; payload_scrambling = b5 >> 4 & 3, address_scrambling = b5 >> 2 & 3, llc_snap =
 *        b5 >> 1 & 1; section_number = b6, last_section_number = b7.
 *     5. Either scrambling field != 0: flag SCRAMBLED, scrambled_sections.
 *     6. ((mac[k] ^ mac_value[k]) & mac_mask[k]) != 0 for a k: flag FILTERED, `filtered`.
 *     7. section_number != 0 or last_section_number != 0: flag FRAGMENT, `fragments`.  A datagram over several sections is NOT put
 *        together; the rows carry both numbers.
 *     8. body = bytes [12, total - 4).  With llc_snap the body needs at least 8 bytes that start AA AA 03 00 00 00, else flag
 *        OTHER_PROTOCOL, other_protocol (ethertype stays 0); `ethertype` = the next two bytes, big-endian; 0x0800 / 0x86DD means IPv4 /
 *        IPv6 from body + 8 (the version nibble is not looked at); any other ethertype: OTHER_PROTOCOL.  Without llc_snap ethertype is
 *        0 and the high nibble of the first body byte says 4 / 6; any other value, or an empty body: OTHER_PROTOCOL.  avail = the body
 *        bytes from the IP header on.
 *     9. IPv4 (header bytes i0 ..): avail >= 20; IHL = i0 & 15 >= 5 and 4 IHL <= avail; total_length = i2 << 8 | i3 with 4 IHL <=
 *        total_length <= avail; the ones'-complement sum of the 2 IHL big-endian 16-bit header words, carries folded in, is 0xFFFF.
 *        If one does not hold: flag BAD_IP, bad_ip.  Else family 4, bytes = total_length, stuffing = avail - total_length, protocol =
 *        i9, src4 / dst4 = i12..i15 / i16..i19 as big-endian numbers; when protocol is 6 or 17, the fragment offset ((i6 << 8 | i7) &
 *        0x1FFF) is 0 and total_length >= 4 IHL + 4: src_port / dst_port = the two big-endian numbers at 4 IHL.
 *    10. IPv6: avail >= 40 and 40 + payload_length (i4 << 8 | i5) <= avail, else BAD_IP.  family 6, bytes = 40 + payload_length,
 *        stuffing the rest, protocol = next_header (i6); ports from i40 when it is 6 or 17 and payload_length >= 4 (extension headers
 *        are not followed).  src4 / dst4 stay 0: the addresses are in the delivered bytes.
 *    11. A row that reached 9 or 10 without BAD_IP has flag DATAGRAM and counts in `datagrams`.  It is delivered when the call has
 *        output buffers: its `bytes` (from the IP header on, without the stuffing) go to the slot's output buffer, back to back in
 *        row order, and row.offset names them; datagrams_delivered and bytes_delivered count.  Every other row has offset -1.
 *   Row: ordered by the TS packet that held the section's last byte, then by position in it.  One table per (stream, slot).
 *   Capacity: sizes first.  If a slot's bytes exceed cap or its rows exceed max_rows the call returns DVBS2GPU_ERR_CAPACITY,
 *     out_bytes[] holds the byte sizes (-1 for a slot whose rows did not fit: its sections were not checked) and out_rows[] the row
 *     counts; no state or counter of any stream has advanced, the tables of the call are empty, the call can be repeated.
 *   State survives from call to call.  reset forgets state, positions and counters; watches stay.
 *   Limits: max_packets <= 4096 per stream and call.  Memory (device banks) per (stream, slot): a 4096-byte section buffer, 6 bytes per
 *     packet of max_packets and 64 bytes per row of max_rows.
 *   NOT done: datagrams split over several sections; the 13818-6 checksum; MPE-FEC (table_id 0x78) and the time-slicing parameters
 *     that then stand in the MAC bytes; IP-level filters (the rows carry what a caller filters on); finding MPE PIDs by
 *     data_broadcast_id. */
typedef struct dvbs2gpu_mpe dvbs2gpu_mpe;
typedef struct dvbs2gpu_mpe_layout {
    int32_t header_bytes, length_mask, max_section_length, max_section_bytes, table_id, mpe_header_bytes, crc_bytes, min_section_bytes;
    int32_t mac_at[6];               /* of MAC_address_1 .. MAC_address_6 */
    int32_t flags_at, section_number_at, last_section_number_at, llc_snap_bytes, ethertype_at, ethertype_ipv4, ethertype_ipv6;
    int32_t ipv4_min_header, ipv4_total_length_at, ipv4_fragment_at, ipv4_protocol_at, ipv4_src_at, ipv4_dst_at;
    int32_t ipv6_header, ipv6_payload_length_at, ipv6_next_header_at;
    int32_t head_bytes;              /* the leading bytes of a section that decide its row, at most: 84 */
} dvbs2gpu_mpe_layout;
int dvbs2gpu_mpe_create(dvbs2gpu_ctx* ctx, int nstreams, int max_packets, int max_rows, dvbs2gpu_mpe** out);
/* a bank without a device: the library's native host implementation of the same rules, behind dvbs2gpu_mpe_work only */
int dvbs2gpu_mpe_create_host(int nstreams, int max_packets, int max_rows, dvbs2gpu_mpe** out);
int dvbs2gpu_mpe_reset(dvbs2gpu_mpe* b);
void dvbs2gpu_mpe_destroy(dvbs2gpu_mpe* b);
int dvbs2gpu_mpe_get_layout(dvbs2gpu_mpe_layout* h_out);
/* slot 0..3; pid 0..0x1FFE, or -1: the slot is empty; mac_value / mac_mask: six bytes each in network order, NULL: all zero */
int dvbs2gpu_mpe_set_watch(dvbs2gpu_mpe* b, int stream, int slot, int pid, const uint8_t mac_value[6], const uint8_t mac_mask[6]);
/* d_ts[i]: DEVICE pointer to nbytes[i] bytes (a multiple of 188, at most 188*max_packets) of stream i, of any alignment.  d_out NULL:
 * rows and counters only (never a capacity failure for bytes; out_bytes may be NULL).  Else d_out[i*4 + k]: DEVICE buffer of cap bytes
 * for the datagrams of slot k of stream i (NULL for an empty slot); out_bytes[i*4 + k] (host) their bytes.  out_rows[i*4 + k] (host, may
 * be NULL): the row counts.  Two kernel launches.  Synchronous on `stream`; chained behind a packetiser or monitor call on the same
 * stream, no packet visits the host. */
int dvbs2gpu_mpe_process_batch(dvbs2gpu_mpe* b, const uint8_t* const* d_ts, const int* nbytes, uint8_t* const* d_out, int cap, int* out_bytes,
                               int* out_rows, void* stream);
/* one stream and slot of any bank with HOST buffers (h_out NULL: rows and counters only): returns the bytes written to h_out or a
 * negative error.  Every other slot of the bank receives an empty call. */
int dvbs2gpu_mpe_work(dvbs2gpu_mpe* b, int stream, int slot, const uint8_t* h_ts, int nbytes, uint8_t* h_out, int cap);
/* the byte and row sizes that the slot's last call needed, whether it succeeded or failed for capacity */
int dvbs2gpu_mpe_get_needed(dvbs2gpu_mpe* b, int stream, int slot, int* bytes, int* rows);
typedef struct dvbs2gpu_mpe_stats {            /* of a slot, since creation, reset or the slot's last set_watch; kept on the host */
    int64_t packets;                 /* trusted TS packets of the slot's PID */
    int64_t sections;                /* rows */
    int64_t other_table, crc_errors, unchecked, scrambled_sections, filtered, fragments, other_protocol, bad_ip;
    int64_t datagrams;               /* rows with DATAGRAM, delivered or not */
    int64_t datagrams_delivered, bytes_delivered;
    int64_t dropped_sections;        /* open sections forgotten */
    int64_t malformed_sections;      /* the bad length, and rows with MALFORMED */
    int64_t malformed_packets, scrambled_packets;   /* TS packets */
} dvbs2gpu_mpe_stats;
/* slot -1: the sum over the stream's slots */
int dvbs2gpu_mpe_get_stats(dvbs2gpu_mpe* b, int stream, int slot, dvbs2gpu_mpe_stats* h_out);
#define DVBS2GPU_MPE_OTHER_TABLE 1
#define DVBS2GPU_MPE_MALFORMED 2
#define DVBS2GPU_MPE_CRC_ERROR 4
#define DVBS2GPU_MPE_UNCHECKED 8
#define DVBS2GPU_MPE_SCRAMBLED 16
#define DVBS2GPU_MPE_FILTERED 32
#define DVBS2GPU_MPE_FRAGMENT 64
#define DVBS2GPU_MPE_OTHER_PROTOCOL 128
#define DVBS2GPU_MPE_BAD_IP 256
#define DVBS2GPU_MPE_DATAGRAM 512
typedef struct dvbs2gpu_mpe_row {              /* 48 bytes */
    uint16_t flags;
    uint8_t family;                  /* 4 or 6 of a DATAGRAM row, else 0 */
    uint8_t protocol;                /* IPv4 protocol / IPv6 next_header */
    uint8_t mac[6];                  /* network order; of a row that reached rule 4 */
    uint8_t section_number, last_section_number;
    uint16_t src_port, dst_port;     /* of an unfragmented TCP or UDP datagram, else 0 */
    uint32_t src4, dst4;             /* IPv4 addresses as big-endian numbers; 0 for IPv6 */
    int32_t length;                  /* total bytes of the section */
    int32_t offset;                  /* of the datagram in the slot's output buffer; -1: not delivered */
    int32_t bytes;                   /* of the datagram of a DATAGRAM row, delivered or not; else 0 */
    int32_t first_packet;            /* index in this call of the TS packet that held its first byte; -1: an earlier call */
    int32_t last_packet;             /* and of the one that held its last byte */
    uint16_t ethertype;              /* of a right LLC/SNAP header, else 0 */
    uint16_t stuffing;               /* body bytes behind the datagram */
} dvbs2gpu_mpe_row;
/* h_rows[cap] (host); *n = rows of the slot's last call, of which min(*n, cap) are written */
int dvbs2gpu_mpe_get_row_table(dvbs2gpu_mpe* b, int stream, int slot, dvbs2gpu_mpe_row* h_rows, int cap, int* n);
/* the same table in HBM, valid until the bank's next call (device banks only): *d_rows is a DEVICE pointer (NULL when *n == 0) */
int dvbs2gpu_mpe_get_row_table_device(dvbs2gpu_mpe* b, int stream, int slot, const dvbs2gpu_mpe_row** d_rows, int* n);

/* ------------------------------------------------------------------ ULE bank (own extension)
 * Nothing in the reference does this.  A transport-stream carrier may carry IP by Unidirectional Lightweight Encapsulation (RFC 4326,
 * extension headers RFC 5163): SNDUs, length-prefixed units without DSM-CC sections around them, on a PID that the operator names
 * (there is no dependable PMT signalling).  For `nstreams` transport streams in HBM a bank reassembles the SNDUs of a PID, checks
 * their CRC-32, applies a filter on the destination address (NPA), follows optional extension headers and a bridged frame's MAC header,
 * checks the IPv4 or IPv6 header behind them, writes one table row per SNDU and lays the datagrams back to back in a device buffer.
 * The sequential form below is the definition (csrc/ule_rules.h, UleHostStream::run); the kernels give its results for every cutting of
 * a stream into calls.  The syntax is written from memory of RFC 4326, RFC 5163, RFC 791 and RFC 8200 and pinned to no vector of
 * theirs; it is one struct, dvbs2gpu_ule_layout.
 *   SNDU: bytes b0 b1 b2 b3: D = b0 >> 7 ("destination address absent"), Length = (b0 << 8 | b1) & 0x7FFF, Type = b2 << 8 | b3.
 *     Length counts the bytes behind Type, CRC included: total = 4 + Length <= 4096.  Length > 4092 is the bad length; with that cap
 *     0xFF is never a legal first byte.  With D = 0 the six bytes behind Type are the destination NPA address.  The last four bytes
 *     are a CRC-32/MPEG (initial value 0xFFFFFFFF, polynomial 0x04C11DB7; the register over all `total` bytes is 0).
 *   Watches: 4 slots per stream, each empty (pid -1) or (PID 0..0x1FFE, npa_value[6], npa_mask[6], accept_unaddressed); an all-zero
 *     mask means every address.  A new bank watches nothing.  THE SAME PID MAY SIT IN SEVERAL SLOTS of a stream: every slot is a
 *     complete, independent reassembler with its own state, counters, rows and output buffer.  Changing a slot's watch starts it afresh.
 *   Packet: 188 bytes at offset 188 k, classified as the TS monitor does: sync-byte errors, TEI packets and null packets are not looked
 *     at.  A packet of the slot's PID counts in `packets` and, in this order ("drop" = the open SNDU is forgotten; with fill > 0 it
 *     counts in dropped_sndus) -- the shared packet rules of the reassembling banks, one slot per reassembler:
 *     1. TSC != 0: scrambled_packets, drop, the continuity step; done.
 *     2. The continuity step (dvbs2gpu_tsmon_*: one state byte per slot).  Duplicate: ignored.  Continuity error or announced
 *        discontinuity: drop, then go on with this packet.  No payload (AFC&1 = 0): done.
 *     3. The payload starts at 4, or at 5 + b4 when AFC&2.  >= 188: malformed_packets, drop, done.
 *     4. PUSI set: ptr = the first payload byte, the payload pointer.  ptr > the bytes after it: malformed_packets, drop, done.  The
 *        ptr bytes after the pointer go to an open SNDU: if they complete it, it is emitted, and if bytes of them are left over `slack`
 *        counts (RFC 4326 discards the SNDU on such a pointer mismatch; this bank does NOT); if it is still incomplete after them (an
 *        open header of one byte too) it is dropped; if they complete a header with the bad length, malformed_sndus counts and the
 *        header is forgotten; with nothing open they are ignored.  Then SNDU starts are parsed behind them (6).
 *     5. PUSI clear: the whole payload goes to an open SNDU; if it completes it, it is emitted and the rest of the payload is ignored
 *        (a packet without PUSI starts nothing); a header completed with the bad length counts in malformed_sndus and is forgotten.
 *        With nothing open the payload is ignored.
 *     6. At an SNDU start, until the TS packet ends: the byte 0xFF ends the packet's chain (the End Indicator 0xFFFF and 0xFF padding
 *        alike).  Else bytes are buffered; with two, total is known: the bad length counts in malformed_sndus, forgets the header and
 *        ends the packet's chain; when the buffered bytes reach total the SNDU is emitted and the next byte is an SNDU start.  An
 *        SNDU, or a header of one byte, that the TS packet's end cuts stays open, across calls too.
 *   Emitting: every emitted SNDU is one row and counts in `sndus`.  In this order; a rule with a flag that is not called information
 *     ends the list, and the fields of the row that later rules would set are 0:
 *     1. Length < 4 with D = 1, or < 10 with D = 0: flag MALFORMED, malformed_sndus.
 *     2. The CRC-32 over all bytes must be 0, else flag CRC_ERROR, crc_errors.  It is always taken.
 *     3. D = 0: mac[0..5] = b4..b9, the body starts at 10; ((mac[k] ^ npa_value[k]) & npa_mask[k]) != 0 for a k: flag FILTERED,
 *        `filtered`.  D = 1: flag NO_ADDRESS (information), no_address, the body starts at 4; without accept_unaddressed: flag
 *        FILTERED, `filtered`.  body = bytes [start, total - 4).
 *     4. Optional extension headers: while Type < 1536 and H-LEN = Type >> 8 & 7 is not 0 (it is 1..5 then): the header is 2 H-LEN
 *        bytes of the body, whose last two are the next Type.  If the optional headers so far exceed 40 bytes or the header runs
 *        beyond the body: flag EXTENSION, `extension`, ethertype = the Type that asked for it.  extension_bytes = their sum.
 *     5. Type < 1536 now (H-LEN 0, a mandatory header): 0x0000 is a Test SNDU: flag TEST, `test`; its bytes go nowhere.  0x0001 is a
 *        bridged frame: it needs 14 body bytes (destination, source, EtherType), else EXTENSION as below; flag BRIDGED (information),
 *        `bridged`; with D = 1 mac = the bridged destination; Type = the frame's EtherType field, the body goes on behind the 14.  Any
 *        other (TS-Concat 0x0002, PRIV-Concat 0x0003, unknown ones): flag EXTENSION, `extension`, ethertype = that Type.  Extension
 *        headers are not looked for behind a bridged frame's MAC header.
 *     6. ethertype = Type.  0x0800 / 0x86DD means IPv4 / IPv6 from here (the version nibble is not looked at); any other value --
 *        an EtherType field below 1536 of a bridged frame, an LLC length, too: flag OTHER_PROTOCOL, other_protocol.  avail = the body
 *        bytes from the IP header on.
 *     7. IPv4 (header bytes i0 ..): avail >= 20; IHL = i0 & 15 >= 5 and 4 IHL <= avail; total_length = i2 << 8 | i3 with 4 IHL <=
 *        total_length <= avail; the ones'-complement sum of the 2 IHL big-endian 16-bit header words, carries folded in, is 0xFFFF.
 *        If one does not hold: flag BAD_IP, bad_ip.  Else family 4, bytes = total_length, stuffing = avail - total_length, protocol =
 *        i9, src4 / dst4 = i12..i15 / i16..i19 as big-endian numbers; when protocol is 6 or 17, the fragment offset ((i6 << 8 | i7) &
 *        0x1FFF) is 0 and total_length >= 4 IHL + 4: src_port / dst_port = the two big-endian numbers at 4 IHL.
 *     8. IPv6: avail >= 40 and 40 + payload_length (i4 << 8 | i5) <= avail, else BAD_IP.  family 6, bytes = 40 + payload_length,
 *        stuffing the rest, protocol = next_header (i6); ports from i40 when it is 6 or 17 and payload_length >= 4 (extension headers
 *        are not followed).  src4 / dst4 stay 0: the addresses are in the delivered bytes.
 *     9. A row that reached 7 or 8 without BAD_IP has flag DATAGRAM, counts in `datagrams`, and ip_at = where the datagram starts in
 *        the SNDU.  It is delivered when the call has output buffers: its `bytes` (from the IP header on, without the stuffing) go to
 *        the slot's output buffer, back to back in row order, and row.offset names them; datagrams_delivered and bytes_delivered
 *        count.  Every other row has offset -1.  (Rules 7 to 9 are the MPE bank's 9 to 11: csrc/ip_rules.h states them once.)
 *   A row is decided by its SNDU's first 4 + 6 + 40 + 14 + 60 + 4 = 128 bytes at most.
 *   Row: ordered by the TS packet that held the SNDU's last byte, then by position in it.  One table per (stream, slot).
 *   Capacity: sizes first.  If a slot's bytes exceed cap or its rows exceed max_rows the call returns DVBS2GPU_ERR_CAPACITY,
 *     out_bytes[] holds the byte sizes (-1 for a slot whose rows did not fit: its SNDUs were not checked) and out_rows[] the row
 *     counts; no state or counter of any stream has advanced, the tables of the call are empty, the call can be repeated.
 *   State survives from call to call.  reset forgets state, positions and counters; watches stay.
 *   Limits: max_packets <= 4096 per stream and call.  Memory (device banks) per (stream, slot): a 4096-byte SNDU buffer, 6 bytes per
 *     packet of max_packets and 64 bytes per row of max_rows.
 *   NOT done: SNDUs above 4096 bytes; the payloads of TS-Concat and PRIV-Concat; the RFC's discard on a pointer mismatch (see
 *     `slack`); security extensions; IP-level filters (the rows carry what a caller filters on). */
typedef struct dvbs2gpu_ule dvbs2gpu_ule;
typedef struct dvbs2gpu_ule_layout {
    int32_t header_bytes, length_bytes, d_bit, length_mask, max_length, max_sndu_bytes, type_at, npa_bytes, crc_bytes, min_length_d1, min_length_d0;
    int32_t type_test, type_bridged, type_ts_concat, type_priv_concat, ethertype_floor, hlen_shift, hlen_mask, max_hlen, max_extension_bytes;
    int32_t mac_header_bytes, bridged_ethertype_at, ethertype_ipv4, ethertype_ipv6;
    int32_t ipv4_min_header, ipv4_total_length_at, ipv4_fragment_at, ipv4_protocol_at, ipv4_src_at, ipv4_dst_at;
    int32_t ipv6_header, ipv6_payload_length_at, ipv6_next_header_at;
    int32_t head_bytes;              /* the leading bytes of an SNDU that decide its row, at most: 128 */
} dvbs2gpu_ule_layout;
int dvbs2gpu_ule_create(dvbs2gpu_ctx* ctx, int nstreams, int max_packets, int max_rows, dvbs2gpu_ule** out);
/* a bank without a device: the library's native host implementation of the same rules, behind dvbs2gpu_ule_work only */
int dvbs2gpu_ule_create_host(int nstreams, int max_packets, int max_rows, dvbs2gpu_ule** out);
int dvbs2gpu_ule_reset(dvbs2gpu_ule* b);
void dvbs2gpu_ule_destroy(dvbs2gpu_ule* b);
int dvbs2gpu_ule_get_layout(dvbs2gpu_ule_layout* h_out);
/* slot 0..3; pid 0..0x1FFE, or -1: the slot is empty; npa_value / npa_mask: six bytes each, NULL: all zero; accept_unaddressed != 0:
 * SNDUs with D = 1 pass the filter */
int dvbs2gpu_ule_set_watch(dvbs2gpu_ule* b, int stream, int slot, int pid, const uint8_t npa_value[6], const uint8_t npa_mask[6], int accept_unaddressed);
/* the arguments of dvbs2gpu_mpe_process_batch: d_ts[i], nbytes[i]; d_out NULL (rows and counters only) or d_out[i*4 + k] of cap bytes
 * for the datagrams of slot k of stream i (NULL for an empty slot); out_bytes[i*4 + k], out_rows[i*4 + k] (host).  Two kernel launches.
 * Synchronous on `stream`; chained behind a packetiser or monitor call on the same stream, no packet visits the host. */
int dvbs2gpu_ule_process_batch(dvbs2gpu_ule* b, const uint8_t* const* d_ts, const int* nbytes, uint8_t* const* d_out, int cap, int* out_bytes,
                               int* out_rows, void* stream);
/* one stream and slot of any bank with HOST buffers (h_out NULL: rows and counters only): returns the bytes written to h_out or a
 * negative error.  Every other slot of the bank receives an empty call. */
int dvbs2gpu_ule_work(dvbs2gpu_ule* b, int stream, int slot, const uint8_t* h_ts, int nbytes, uint8_t* h_out, int cap);
/* the byte and row sizes that the slot's last call needed, whether it succeeded or failed for capacity (bytes -1: the rows did not fit) */
int dvbs2gpu_ule_get_needed(dvbs2gpu_ule* b, int stream, int slot, int* bytes, int* rows);
typedef struct dvbs2gpu_ule_stats {            /* of a slot, since creation, reset or the slot's last set_watch; kept on the host */
    int64_t packets;                 /* trusted TS packets of the slot's PID */
    int64_t sndus;                   /* rows */
    int64_t crc_errors, filtered, no_address, test, bridged, extension, other_protocol, bad_ip;
    int64_t datagrams;               /* rows with DATAGRAM, delivered or not */
    int64_t datagrams_delivered, bytes_delivered;
    int64_t dropped_sndus;           /* open SNDUs forgotten */
    int64_t malformed_sndus;         /* the bad length, and rows with MALFORMED */
    int64_t slack;                   /* pointer bytes left over behind the end of the open SNDU */
    int64_t malformed_packets, scrambled_packets;   /* TS packets */
} dvbs2gpu_ule_stats;
/* slot -1: the sum over the stream's slots */
int dvbs2gpu_ule_get_stats(dvbs2gpu_ule* b, int stream, int slot, dvbs2gpu_ule_stats* h_out);
#define DVBS2GPU_ULE_MALFORMED 1
#define DVBS2GPU_ULE_CRC_ERROR 2
#define DVBS2GPU_ULE_FILTERED 4
#define DVBS2GPU_ULE_NO_ADDRESS 8
#define DVBS2GPU_ULE_TEST 16
#define DVBS2GPU_ULE_BRIDGED 32
#define DVBS2GPU_ULE_EXTENSION 64
#define DVBS2GPU_ULE_OTHER_PROTOCOL 128
#define DVBS2GPU_ULE_BAD_IP 256
#define DVBS2GPU_ULE_DATAGRAM 512
typedef struct dvbs2gpu_ule_row {              /* 48 bytes */
    uint16_t flags;
    uint8_t family;                  /* 4 or 6 of a DATAGRAM row, else 0 */
    uint8_t protocol;                /* IPv4 protocol / IPv6 next_header */
    uint8_t mac[6];                  /* the NPA where there was one, else a bridged frame's destination, else 0 */
    uint8_t ip_at;                   /* of a DATAGRAM row: where the datagram starts in the SNDU */
    uint8_t extension_bytes;         /* of the optional extension headers that were followed */
    uint16_t src_port, dst_port;     /* of an unfragmented TCP or UDP datagram, else 0 */
    uint32_t src4, dst4;             /* IPv4 addresses as big-endian numbers; 0 for IPv6 */
    int32_t length;                  /* total bytes of the SNDU */
    int32_t offset;                  /* of the datagram in the slot's output buffer; -1: not delivered */
    int32_t bytes;                   /* of the datagram of a DATAGRAM row, delivered or not; else 0 */
    int32_t first_packet;            /* index in this call of the TS packet that held its first byte; -1: an earlier call */
    int32_t last_packet;             /* and of the one that held its last byte */
    uint16_t ethertype;              /* the final Type / EtherType of a row that reached rule 6; the offending Type of EXTENSION */
    uint16_t stuffing;               /* body bytes behind the datagram */
} dvbs2gpu_ule_row;
/* h_rows[cap] (host); *n = rows of the slot's last call, of which min(*n, cap) are written */
int dvbs2gpu_ule_get_row_table(dvbs2gpu_ule* b, int stream, int slot, dvbs2gpu_ule_row* h_rows, int cap, int* n);
/* the same table in HBM, valid until the bank's next call (device banks only): *d_rows is a DEVICE pointer (NULL when *n == 0) */
int dvbs2gpu_ule_get_row_table_device(dvbs2gpu_ule* b, int stream, int slot, const dvbs2gpu_ule_row** d_rows, int* n);

/* ------------------------------------------------------------------ IP-TS bank (own extension)
 * Nothing in the reference does this.  The IP datagrams that the MPE bank, the ULE bank and the GSE paths leave in HBM, one table row
 * each, usually carry television again: an MPTS or SPTS in UDP or in RTP (RFC 2250, payload type 33), normally 7 x 188 bytes per
 * datagram, to a multicast group and port.  For `nstreams` streams a bank reads such a table where it lies, picks the UDP datagrams of
 * up to 4 flow slots per stream, verifies their UDP checksum, recognises raw TS or RTP/MP2T payloads, applies an RTP sequence rule per
 * slot, writes one row per input row and lays the TS packets of each slot back to back in a device buffer: a d_ts[i] / nbytes[i] of
 * dvbs2gpu_tsmon_process_batch and of the PSI, PCR, PES and T2-MI banks.  The sequential form below is the definition
 * (csrc/ipts_rules.h, IptsHostStream::run); the kernels give its results for every cutting of a datagram sequence into calls.  The
 * syntax is written from memory of RFC 768, RFC 791, RFC 8200, RFC 3550 and RFC 2250 and pinned to no vector of theirs; it is one
 * struct, dvbs2gpu_ipts_layout.
 *   Input: one view per stream and call (dvbs2gpu_ipts_view, below), the same for device and host banks: the datagram bytes, a table of
 *     n rows (0 <= n <= max_rows) of `stride` bytes, and where a row keeps its int32 offset into the bytes and its int32 byte count (a
 *     count below 0 is read as 0).  kind RAW_IP: a datagram starts at its IP header (MPE and ULE rows); kind GRE: it starts with the
 *     GRE header that the GSE paths write (dvbs2gpu_gse_pdu rows).  The bank writes exactly one row per input row, at the same index.
 *   Flows: 4 slots per stream, each empty (family 0) or (family 4 | 6, destination address, destination UDP port); an IPv4 address
 *     is the first four of the sixteen address bytes, in network order.  The match is exact on all three; where several slots match,
 *     the lowest wins.  A new bank has no flow.  set_flow clears the slot's counters and its RTP state.
 *   Rules per row, in table order; the first rule that fires ends the list, except where it says that the list goes on, and the
 *   fields of the row that later rules would set are 0 (slot and offset: -1):
 *     1. offset < 0 (its source did not deliver it): flag NOT_DELIVERED.
 *     2. Kind GRE: the row needs the 4 bytes 00 00 08 00 (family 4) or 00 00 86 DD (family 6), else flag NOT_IP; the IP header
 *        follows them (its version nibble is not looked at).  Kind RAW_IP: the family is the high nibble of the first byte, 4 or 6,
 *        else (or with no byte) NOT_IP.
 *     3. The IP header by the rules 9 and 10 of the MPE bank (csrc/ip_rules.h, shared), avail = the row's bytes from the IP header
 *        on: what is BAD_IP there is flag BAD_IP here.  Else `family` is set.  Bytes behind the IP length are ignored.
 *     4. IPv4 with MF set or a fragment offset != 0 ((i6 << 8 | i7) & 0x3FFF): flag FRAGMENT.  Protocol (IPv6: next_header) != 17:
 *        flag OTHER_PROTOCOL; IPv6 extension headers are not followed.
 *     5. The IP payload (behind 4 IHL or 40 header bytes, up to the IP length) needs 8 bytes, and the UDP length L = u4 << 8 | u5
 *        must be 8 <= L <= the IP payload bytes, else flag BAD_UDP.  src_port = u0 << 8 | u1, dst_port = u2 << 8 | u3; the payload
 *        is the L - 8 bytes from u8.
 *     6. No slot of the stream matches (family, destination address, dst_port): flag UNWATCHED; nothing more is read of the
 *        datagram.  Else `slot`.
 *     7. The transmitted checksum u6 << 8 | u7 of 0 means not computed on IPv4: flag NO_CHECKSUM, nothing is verified, the list goes
 *        on; on IPv6 it is flag BAD_CHECKSUM.  Else the ones'-complement sum, carries folded in, of the pseudo-header (IPv4: source,
 *        destination, 0, 17, L; IPv6: source, destination, L as 32 bits, 0 0 0 17) and of the L UDP bytes as big-endian 16-bit
 *        words, an odd last byte padded with a zero byte, must be 0xFFFF, else flag BAD_CHECKSUM.
 *     8. A payload whose length is a positive multiple of 188 with 0x47 at every k * 188 is raw TS: flag RAW, ts_at = where it
 *        starts in the row's bytes.  Any other payload is read as RTP (bytes p0 ..): fewer than 12 bytes or a version p0 >> 6 != 2:
 *        flag BAD_PAYLOAD.  The header is 12 + 4 CC (p0 & 15) bytes; with X (p0 >> 4 & 1) 4 more bytes follow, plus 4 x the 16-bit
 *        number in their last two; with P (p0 >> 5 & 1) the last payload byte is the pad count, which must be >= 1; any of these
 *        running beyond the payload: BAD_PAYLOAD.  payload_type = p1 & 127; != 33: flag OTHER_PAYLOAD.  What is left between header
 *        and padding must be a positive multiple of 188 with 0x47 at every k * 188, else BAD_PAYLOAD.  Flag RTP; rtp_seq = p2 << 8 |
 *        p3, rtp_timestamp = p4..p7, rtp_ssrc = p8..p11 as big-endian numbers; ts_at as above.  The marker bit is not looked at.
 *     9. RTP rows only; per slot the state (has, last_seq, ssrc) survives calls.  Nothing stored: accept.  Another SSRC than the
 *        stored one: flag NEW_SOURCE, accept.  Else d = (rtp_seq - last_seq - 1) mod 65536: 0: accept; 1 <= d < 0x8000: flag LOSS,
 *        lost = d, accept; d >= 0x8000 (a duplicate or a reordered packet): flag LATE, not delivered, the state unchanged.  Accepting
 *        stores (rtp_seq, rtp_ssrc).  RAW rows neither read nor write the state.
 *    10. A RAW row and an accepted RTP row have flag TS, packets = their TS packets and bytes = 188 packets.  When the call has output
 *        buffers the packets go to the slot's buffer, back to back in row order, and row.offset names them.  Every other row has
 *        offset -1.
 *   Counters: one per flag; those of rules 1 to 6 and `rows` per stream, those of rules 7 to 10 and `matched` per slot, with ts_packets
 *     (the packets of TS rows), bytes_delivered (of calls with output buffers), lost (the sum of row.lost) and loss_events (the rows with
 *     LOSS).  Kept on the host in 64 bits.
 *   Capacity: sizes first.  If a slot's bytes exceed cap the call returns DVBS2GPU_ERR_CAPACITY, out_bytes[] holds the needed sizes; no
 *     state or counter of any stream has advanced, the tables of the call are empty, the call can be repeated.  A view of more than
 *     max_rows rows is an argument error.
 *   State survives from call to call.  reset forgets state and counters; the flows stay.
 *   Limits: max_rows <= 16384 per stream and call.  Memory (device banks): 40 bytes per row of max_rows and 0.5 KB per stream.
 *   NOT done: RFC 2733 / SMPTE 2022-1 FEC; reordering of LATE packets; IPv4 reassembly; IPv6 extension headers; address masks and
 *     source filters; RTCP. */
typedef struct dvbs2gpu_ipts dvbs2gpu_ipts;
#define DVBS2GPU_IPTS_KIND_RAW_IP 0
#define DVBS2GPU_IPTS_KIND_GRE 1
typedef struct dvbs2gpu_ipts_view {            /* 40 bytes */
    const uint8_t* bytes;            /* the datagram bytes, of any alignment (process_batch: a DEVICE pointer; work: a host pointer) */
    const void* rows;                /* n rows of `stride` bytes, at a multiple of 4 (device / host like bytes) */
    int32_t stride;                  /* a multiple of 4 */
    int32_t offset_at, bytes_at;     /* where a row keeps its int32 offset into `bytes` and its int32 byte count: multiples of 4 */
    int32_t kind;                    /* DVBS2GPU_IPTS_KIND_* */
    int32_t n;                       /* rows, 0 .. max_rows (with 0 the pointers may be NULL) */
    int32_t reserved;
} dvbs2gpu_ipts_view;
/* built with offsetof from the calls that name a table in HBM and the buffer the rows point into:
 *   dvbs2gpu_mpe_get_row_table_device / dvbs2gpu_ule_get_row_table_device (kind RAW_IP; dvbs2gpu_mpe_row / dvbs2gpu_ule_row: offset, bytes;
 *     bytes = the slot's d_out), dvbs2gpu_bbts_get_pdu_table_device / dvbs2gpu_bbts_ma_get_pdu_table_device (kind GRE; dvbs2gpu_gse_pdu:
 *     offset, bytes; bytes = the stream's or the ISI lane's output buffer). */
typedef struct dvbs2gpu_ipts_layout {
    int32_t gre_header_bytes, ipv4_src_at, ipv6_src_at, ipv6_dst_at, ipv4_more_fragments, udp_protocol, udp_header_bytes, udp_length_at, udp_checksum_at;
    int32_t ts_packet_bytes, ts_sync, rtp_min_header, rtp_version, rtp_payload_type_mp2t, rtp_seq_at, rtp_timestamp_at, rtp_ssrc_at, late_from;
    int32_t head_bytes;              /* rules 2 to 6 read the first 72 bytes of a row at most; a wave keeps 128 */
    int32_t slots, row_bytes, view_bytes;
} dvbs2gpu_ipts_layout;
int dvbs2gpu_ipts_create(dvbs2gpu_ctx* ctx, int nstreams, int max_rows, dvbs2gpu_ipts** out);
/* a bank without a device: the library's native host implementation of the same rules, behind dvbs2gpu_ipts_work only */
int dvbs2gpu_ipts_create_host(int nstreams, int max_rows, dvbs2gpu_ipts** out);
int dvbs2gpu_ipts_reset(dvbs2gpu_ipts* b);
void dvbs2gpu_ipts_destroy(dvbs2gpu_ipts* b);
int dvbs2gpu_ipts_get_layout(dvbs2gpu_ipts_layout* h_out);
/* slot 0..3; family 4, 6, or 0: the slot is empty (dst_addr may be NULL then); dst_addr: sixteen bytes, an IPv4 address in the first four */
int dvbs2gpu_ipts_set_flow(dvbs2gpu_ipts* b, int stream, int slot, int family, const uint8_t dst_addr[16], int dst_port);
/* views[i] (a host array of views with DEVICE pointers): the datagrams of stream i.  d_out NULL: rows and counters only (never a
 * capacity failure; out_bytes may be NULL).  Else d_out[i*4 + k]: DEVICE buffer of cap bytes, of any alignment, for the TS packets of
 * slot k of stream i (NULL for an empty slot); out_bytes[i*4 + k] (host) their bytes.  out_rows[i] (host, may be NULL): the rows
 * written, views[i].n.  Two kernel launches.  Synchronous on `stream`; chained behind the call that wrote the datagrams and in front
 * of a TS bank's call on the same stream, no packet visits the host. */
int dvbs2gpu_ipts_process_batch(dvbs2gpu_ipts* b, const dvbs2gpu_ipts_view* views, uint8_t* const* d_out, int cap, int* out_bytes, int* out_rows,
                                void* stream);
/* one stream of any bank with HOST pointers in the view and HOST buffers h_out[k] of cap bytes (h_out NULL: rows and counters only);
 * out_bytes[4] (may be NULL): the bytes of each slot.  0 or a negative error.  Every other stream of the bank receives an empty call. */
int dvbs2gpu_ipts_work(dvbs2gpu_ipts* b, int stream, const dvbs2gpu_ipts_view* h_view, uint8_t* const* h_out, int cap, int* out_bytes);
/* the bytes that the slot's last call needed, whether it succeeded or failed for capacity (0 of a call without output buffers) */
int dvbs2gpu_ipts_get_needed(dvbs2gpu_ipts* b, int stream, int slot, int* bytes);
typedef struct dvbs2gpu_ipts_stats {           /* since creation or reset; a slot's since its last set_flow; kept on the host */
    /* the stream's own (0 when a slot >= 0 is asked for) */
    int64_t rows;
    int64_t not_delivered, not_ip, bad_ip, fragments, other_protocol, bad_udp, unwatched;
    /* a slot's */
    int64_t matched;                 /* rows of the slot's flow */
    int64_t bad_checksum, no_checksum, bad_payload, other_payload, raw, rtp, new_source, loss_events, late;
    int64_t ts;                      /* rows with TS, delivered or not */
    int64_t ts_packets;              /* their TS packets */
    int64_t bytes_delivered;
    int64_t lost;                    /* RTP packets missing before rows with LOSS */
} dvbs2gpu_ipts_stats;
/* slot 0..3: the slot's counters; slot -1: the stream's own counters and the sum over its slots */
int dvbs2gpu_ipts_get_stats(dvbs2gpu_ipts* b, int stream, int slot, dvbs2gpu_ipts_stats* h_out);
#define DVBS2GPU_IPTS_NOT_DELIVERED 1
#define DVBS2GPU_IPTS_NOT_IP 2
#define DVBS2GPU_IPTS_BAD_IP 4
#define DVBS2GPU_IPTS_FRAGMENT 8
#define DVBS2GPU_IPTS_OTHER_PROTOCOL 16
#define DVBS2GPU_IPTS_BAD_UDP 32
#define DVBS2GPU_IPTS_UNWATCHED 64
#define DVBS2GPU_IPTS_BAD_CHECKSUM 128
#define DVBS2GPU_IPTS_NO_CHECKSUM 256
#define DVBS2GPU_IPTS_BAD_PAYLOAD 512
#define DVBS2GPU_IPTS_OTHER_PAYLOAD 1024
#define DVBS2GPU_IPTS_RAW 2048
#define DVBS2GPU_IPTS_RTP 4096
#define DVBS2GPU_IPTS_NEW_SOURCE 8192
#define DVBS2GPU_IPTS_LOSS 16384
#define DVBS2GPU_IPTS_LATE 32768
#define DVBS2GPU_IPTS_TS 65536
typedef struct dvbs2gpu_ipts_row {             /* 40 bytes */
    uint32_t flags;
    int8_t slot;                     /* of a row that matched a flow, else -1 */
    uint8_t family;                  /* 4 or 6 of a row that passed rule 3, else 0 */
    uint8_t payload_type;            /* of an RTP header that passed its length checks */
    uint8_t reserved;
    uint16_t src_port, dst_port;     /* of a row that passed rule 5 */
    uint16_t rtp_seq;                /* of a row with RTP */
    uint16_t ts_at;                  /* of a row with RAW or RTP: where its TS packets start in the input row's bytes */
    uint32_t rtp_timestamp, rtp_ssrc;
    int32_t packets;                 /* TS packets of a TS row, delivered or not; else 0 */
    int32_t lost;                    /* of a row with LOSS */
    int32_t offset;                  /* of the TS packets in the slot's output buffer; -1: not delivered */
    int32_t bytes;                   /* 188 packets */
} dvbs2gpu_ipts_row;
/* h_rows[cap] (host); *n = rows of the stream's last call, of which min(*n, cap) are written */
int dvbs2gpu_ipts_get_row_table(dvbs2gpu_ipts* b, int stream, dvbs2gpu_ipts_row* h_rows, int cap, int* n);
/* the same table in HBM, valid until the bank's next call (device banks only): *d_rows is a DEVICE pointer (NULL when *n == 0) */
int dvbs2gpu_ipts_get_row_table_device(dvbs2gpu_ipts* b, int stream, const dvbs2gpu_ipts_row** d_rows, int* n);

/* ------------------------------------------------------------------ IP output bank (own extension)
 * Nothing in the reference does this.  It is the IP-TS bank's direction reversed: a head-end sends every selected service as MPEG-TS in
 * UDP or in RTP (RFC 2250, payload type 33, normally 7 x 188 bytes per datagram) to a multicast group.  For `nstreams` transport
 * streams in HBM -- the d_ts[i] / nbytes[i] of every TS bank -- a bank picks the packets of up to 4 flow slots per stream, groups each
 * slot's packets into datagrams with complete IPv4 / IPv6 + UDP (+ RTP) headers and checksums, lays each slot's datagrams back to back
 * in a device buffer and writes one table row per datagram: a dvbs2gpu_ipts_view of kind RAW_IP as it stands, which the IP-TS bank
 * reads back.  The sequential form below is the definition (csrc/ipout_rules.h, IpoutHostStream::run); the kernels give its results for
 * every cutting of a stream into calls.  The syntax is written from memory of RFC 768, RFC 791, RFC 8200, RFC 3550 and RFC 2250 and
 * pinned to no vector of theirs; the offsets are those of dvbs2gpu_ipts_layout and dvbs2gpu_mpe_layout, and what they do not name is
 * dvbs2gpu_ipout_layout.
 *   Packet: 188 bytes at offset 188 k.  b0 != 0x47: counted as bad_sync, it enters no slot.  Else PID = (b1 & 0x1F) << 8 | b2 as it
 *     stands; TEI and the scrambling bits are not looked at: the bank forwards, it does not judge.  The stream's position n (64 bits,
 *     since creation or reset) counts every 188 bytes handed in; it is the counter `packets`.
 *   Flow slot: 4 per stream, each empty (family 0) or a dvbs2gpu_ipout_flow with a PID list.  pid_mode 0: every PID enters; 1: the
 *     listed ones; 2: all but the listed ones; drop_null keeps PID 0x1FFF out whatever the list says (the monitor's filter).  The slots
 *     are independent: one packet may enter several.  A new bank has no flow.  set_flow clears the slot's counters, its held packets and
 *     its datagram count (the RTP sequence starts at seq_base again); the stream's clock stays.
 *   Clock: per stream (q, r), both 0 in a new bank and after reset, and the rate tpp of set_rate (0 in a new bank: q never moves), with
 *     D = 300 << 24.  The tick value of an input packet, good sync byte or not, is q before it; after it r += tpp, q += r / D (q mod
 *     2^32), r %= D.  So q counts 90 kHz ticks.  A rate change takes effect at the next call; q and r stay.
 *   Datagrams: a slot's passing packets, in input order, follow the 0 .. P-1 packets it holds from earlier calls; every full group of
 *     P = packets_per_datagram packets is a datagram, the rest is held with the tick value of its first packet.  With the call's flush
 *     flag a non-empty rest leaves as one SHORT datagram at the end of the call, also where the call brought the slot nothing.  Without
 *     flush the output is the same for every cutting of the stream into calls.  A set_flow with another P meets no held packets: it
 *     dropped them.
 *   Headers, all numbers big-endian:
 *     IPv4 (20 bytes): 45, dscp << 2, total length, identification 00 00, 40 00 (DF), ttl, 17, header checksum, source, destination.
 *     IPv6 (40 bytes): version 6, traffic class dscp << 2, flow label 0, payload length, next header 17, hop limit = ttl, source,
 *       destination.
 *     UDP (8): source port, destination port, length L, checksum: the ones' complement of the ones'-complement sum over the
 *       pseudo-header (as rule 7 of the IP-TS bank) and the L UDP bytes with a zero checksum field; always computed, on IPv4 too; a
 *       computed 0x0000 is sent as 0xFFFF.
 *     RTP (mode RTP, 12): 80, 21 (marker 0, payload type 33), seq = seq_base + the slot's datagrams so far (since set_flow or reset)
 *       mod 65536, timestamp = timestamp_base + the tick value of the datagram's first packet mod 2^32, ssrc.  Mode RAW has no RTP
 *       header; the row's rtp_seq and rtp_timestamp are 0.
 *     Then the datagram's packets, 188 bytes each, unchanged.
 *   Row: one per datagram, per slot, in output order (dvbs2gpu_ipout_row).  Flags RTP (the mode), SHORT (fewer than P packets), CARRIED
 *     (it begins with packets held from earlier calls).  first_packet: the index in this call's input of the first packet that the
 *     datagram takes from this call, -1 if it takes none.  udp_checksum: as sent.
 *   Counters, 64 bits on the host: per stream packets and bad_sync; per slot passed (packets that entered), datagrams, short_datagrams,
 *     ts_packets (in datagrams), bytes_delivered, and held: what the slot holds now, not a sum over calls.
 *   Capacity: sizes first.  If a slot's bytes exceed cap the call returns DVBS2GPU_ERR_CAPACITY, out_bytes[] holds the needed sizes; no
 *     state or counter of any stream has advanced, the clock neither, the tables of the call are empty, the call can be repeated.
 *   State survives from call to call.  reset forgets state (clock, held packets, datagram counts) and counters; flows and rates stay.
 *   Limits: max_packets <= 8192 per stream and call; a call makes at most max(1, packets) datagrams per slot.  Memory (device banks)
 *     per stream: the PID bitmaps, 1 KiB per slot; the held packets, 6 x 188 bytes per slot, not doubled (the commit kernel reads them
 *     for a slot's first datagram, meets a barrier and only then writes them); the row tables, 24 bytes x max_packets per slot; a
 *     list of the passing packets' indices, 2 bytes x max_packets per slot; 0.3 KB of flows and state.
 *   NOT done: FEC (SMPTE 2022-1); RTCP; IPv4 options and fragmentation; IPv6 extension headers; VLAN / Ethernet framing; pacing (the
 *     rows carry the timestamps a sender paces by); PCR-locked timestamps: the clock is the packet count at the set rate. */
typedef struct dvbs2gpu_ipout dvbs2gpu_ipout;
#define DVBS2GPU_IPOUT_MODE_RAW 0
#define DVBS2GPU_IPOUT_MODE_RTP 1
typedef struct dvbs2gpu_ipout_flow {           /* 56 bytes */
    int32_t family;                  /* 4, 6, or 0: the slot is empty and nothing else is read */
    uint8_t src_addr[16], dst_addr[16];        /* an IPv4 address in the first four bytes, network order */
    uint16_t src_port, dst_port;
    uint8_t ttl;                     /* the hop limit on IPv6 */
    uint8_t dscp;                    /* 0..63 */
    uint8_t mode;                    /* DVBS2GPU_IPOUT_MODE_* */
    uint8_t packets_per_datagram;    /* P, 1..7 */
    uint32_t ssrc, timestamp_base;
    uint16_t seq_base;
    uint8_t pid_mode;                /* 0 all, 1 listed, 2 all but listed */
    uint8_t drop_null;
} dvbs2gpu_ipout_flow;
typedef struct dvbs2gpu_ipout_layout {
    int32_t ipv4_version_ihl, ipv4_tos_at, ipv4_id_at, ipv4_dont_fragment, ipv4_ttl_at, ipv4_checksum_at, ipv6_hop_limit_at, rtp_first_byte;
    int32_t tick_divisor;            /* 27 MHz ticks per tick of the RTP clock: D = tick_divisor << 24 */
    int32_t max_packets_per_datagram, held_packets, pid_map_bytes, slots, row_bytes, flow_bytes;
} dvbs2gpu_ipout_layout;
int dvbs2gpu_ipout_create(dvbs2gpu_ctx* ctx, int nstreams, int max_packets, dvbs2gpu_ipout** out);
/* a bank without a device: the library's native host implementation of the same rules, behind dvbs2gpu_ipout_work only */
int dvbs2gpu_ipout_create_host(int nstreams, int max_packets, dvbs2gpu_ipout** out);
int dvbs2gpu_ipout_reset(dvbs2gpu_ipout* b);
void dvbs2gpu_ipout_destroy(dvbs2gpu_ipout* b);
int dvbs2gpu_ipout_get_layout(dvbs2gpu_ipout_layout* h_out);
/* slot 0..3; flow->family 0 (or flow NULL) empties the slot; pids[npids] (host, may be NULL with npids 0): the list of pid_mode 1 and 2,
 * each <= 0x1FFF.  DVBS2GPU_ERR_ARG for another family, P outside 1..7, dscp > 63, a mode or pid_mode out of range or a PID > 0x1FFF;
 * the slot is unchanged then. */
int dvbs2gpu_ipout_set_flow(dvbs2gpu_ipout* b, int stream, int slot, const dvbs2gpu_ipout_flow* flow, const uint16_t* pids, int npids);
/* ticks_per_packet_q24: the quantity of dvbs2gpu_pcr_set_rate (27 MHz ticks per 188-byte packet in Q24.24, < 2^48), 0: not set */
int dvbs2gpu_ipout_set_rate(dvbs2gpu_ipout* b, int stream, uint64_t ticks_per_packet_q24);
/* d_ts[i] (DEVICE), nbytes[i] (host): whole 188-byte packets of stream i, at most max_packets (d_ts[i] may be NULL with nbytes[i] 0).
 * d_out[i*4 + k]: DEVICE buffer of cap bytes, of any alignment, for the datagrams of slot k of stream i (NULL for an empty slot only);
 * out_bytes[i*4 + k] (host) their bytes; out_rows[i*4 + k] (host, may be NULL) their number.  flush != 0: every slot's held packets
 * leave (see above).  Two kernel launches.  Synchronous on `stream`; chained behind the call that wrote the TS and in front of
 * dvbs2gpu_ipts_process_batch on the same stream, no packet visits the host. */
int dvbs2gpu_ipout_process_batch(dvbs2gpu_ipout* b, const uint8_t* const* d_ts, const int* nbytes, uint8_t* const* d_out, int cap, int* out_bytes,
                                 int* out_rows, int flush, void* stream);
/* one stream of any bank with HOST buffers: h_ts[nbytes], h_out[k] of cap bytes (NULL for an empty slot only); out_bytes[4] (may be
 * NULL): the bytes of each slot.  0 or a negative error.  Every other stream of the bank receives an empty call without flush. */
int dvbs2gpu_ipout_work(dvbs2gpu_ipout* b, int stream, const uint8_t* h_ts, int nbytes, uint8_t* const* h_out, int cap, int* out_bytes, int flush);
/* the bytes that the slot's last call needed, whether it succeeded or failed for capacity */
int dvbs2gpu_ipout_get_needed(dvbs2gpu_ipout* b, int stream, int slot, int* bytes);
typedef struct dvbs2gpu_ipout_stats {          /* since creation or reset; a slot's since its last set_flow; kept on the host */
    int64_t packets, bad_sync;       /* the stream's own (0 when a slot >= 0 is asked for) */
    int64_t passed, datagrams, short_datagrams, ts_packets, bytes_delivered;
    int64_t held;                    /* now */
} dvbs2gpu_ipout_stats;
/* slot 0..3: the slot's counters; slot -1: the stream's own counters and the sum over its slots */
int dvbs2gpu_ipout_get_stats(dvbs2gpu_ipout* b, int stream, int slot, dvbs2gpu_ipout_stats* h_out);
#define DVBS2GPU_IPOUT_RTP 1
#define DVBS2GPU_IPOUT_SHORT 2
#define DVBS2GPU_IPOUT_CARRIED 4
typedef struct dvbs2gpu_ipout_row {            /* 24 bytes */
    int32_t offset;                  /* of the datagram, at its IP header, in the slot's output buffer */
    int32_t bytes;
    uint32_t rtp_timestamp;
    uint16_t rtp_seq;
    uint8_t packets;
    uint8_t flags;                   /* DVBS2GPU_IPOUT_* */
    int32_t first_packet;
    uint16_t udp_checksum;
    uint16_t reserved;
} dvbs2gpu_ipout_row;
/* h_rows[cap] (host); *n = rows of the slot's last call, of which min(*n, cap) are written */
int dvbs2gpu_ipout_get_row_table(dvbs2gpu_ipout* b, int stream, int slot, dvbs2gpu_ipout_row* h_rows, int cap, int* n);
/* the same table in HBM, valid until the bank's next call (device banks only): *d_rows is a DEVICE pointer (NULL when *n == 0) */
int dvbs2gpu_ipout_get_row_table_device(dvbs2gpu_ipout* b, int stream, int slot, const dvbs2gpu_ipout_row** d_rows, int* n);

#ifdef __cplusplus
}
#endif
#endif
