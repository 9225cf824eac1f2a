// The DVB-S2 modulator's device-side structs, its state in the context and what capi.hip calls (kernels and host code: s2_tx.hip; rules: s2_tx_rules.h).
#pragma once
#include <hip/hip_runtime.h>
#include <map>
#include "s2_tx_rules.h"
#include "dev_buf.h"

struct dvbs2gpu_ctx;

namespace s2 {

// one frame of a framing launch; FRAMES_PER_LAUNCH of them are the kernel's argument (no device table, nothing to upload)
struct TxFrameDev {
    long long code_off, code_stride;    // the code word of stream s: d_code + code_off + s * code_stride
    long long sym_off;                  // first symbol of the frame in a stream's block
    const cf32* tab;                    // transmit constellation, 32 entries (null: dummy frame)
    int pls, dummy, qpsk, bits, payload, pilot_blocks, code_bytes;
    int col[5];
};
struct TxFrameArgs { TxFrameDev f[s2tx::FRAMES_PER_LAUNCH]; };

// The modulator's part of the context: the transmit constellation tables by key, the buffers dvbs2gpu_s2_modulate_batch keeps its code words and symbols in, the
// channel's per-stream table.  The buffers are shared by all calls on the context: `ev` is recorded behind the last launch that uses them, and a call on
// another stream waits for it before it writes them again.
struct TxState {
    std::map<int, DevBuf<cf32>> constel;
    Workspace code, sym, chan;
    hipEvent_t ev = nullptr;
    bool ev_recorded = false;
    void* stage = nullptr;              // pinned host staging of the channel's table; ev_stage: behind the last copy out of it
    size_t stage_bytes = 0;
    hipEvent_t ev_stage = nullptr;
    bool stage_recorded = false;
    ~TxState() {
        if (ev) (void)hipEventDestroy(ev);
        if (ev_stage) (void)hipEventDestroy(ev_stage);
        if (stage) (void)hipHostFree(stage);
    }
};

int tx_buffers_enter(dvbs2gpu_ctx* ctx, hipStream_t st);
int tx_buffers_leave(dvbs2gpu_ctx* ctx, hipStream_t st);
// Every argument has been checked by the caller (capi.hip); all pointers device pointers except pls / code_off / code_stride and the channel's arrays.
int tx_pl_frame(dvbs2gpu_ctx* ctx, const int32_t* pls, int nframes, const uint8_t* d_code, const long long* code_off, const long long* code_stride, int nstreams,
                cf32* d_symbols, hipStream_t st);
int tx_pulse_shape(dvbs2gpu_ctx* ctx, const cf32* d_symbols, int nstreams, long long symbols, double rolloff, double timing, int circular, cf32* d_iq, hipStream_t st);
int tx_channel(dvbs2gpu_ctx* ctx, cf32* d_iq, int nstreams, long long nsamples, const double* esn0_db, const double* cfo, const double* phase0,
               const uint64_t* seed, hipStream_t st);
// the same rules on the CPU for one stream (host pointers; symbols / iq may be null)
void tx_host(const int32_t* pls, int nframes, const uint8_t* code, double rolloff, double timing, int circular, const double* esn0_db, const double* cfo,
             const double* phase0, const uint64_t* seed, long long stream, cf32* symbols, cf32* iq);
// ... its last two stages on their own, for any block
void tx_shape_host(const cf32* symbols, long long nsymbols, double rolloff, double timing, int circular, cf32* iq);
void tx_channel_host(cf32* iq, long long nsamples, double esn0_db, double cfo, double phase0, uint64_t seed, long long stream);

}  // namespace s2
