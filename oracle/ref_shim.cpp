// ORACLE support (test infrastructure, CPU only) -- not part of the shipped engine.
// extern "C" entry points around the reference's own, unmodified, self-contained FEC classes.
// This file is the only thing of ours in oracle/_ref/libdvbs2ref.so: the reference sources are compiled
// where they lie under /root/reference (see oracle/Makefile, target `ref`); nothing is copied.
// It exists so tests can (a) pin the restatement in oracle/*.cpp and (b) generate tests/golden/*.
#include <cstdint>
#include <cstring>
#include <map>
#include <mutex>
#include <vector>
#include "dvbs2/codings/bbframe_ldpc.h"
#include "dvbs2/codings/bbframe_bch.h"
#include "dvbs2/codings/bbframe_descramble.h"
#include "dvbs2/codings/s2_deinterleaver.h"

using namespace dsp::dvbs2;

static dvbs2_code_rate_t to_rate(int r) {
    // our rate index 0..10 = 1/4 1/3 2/5 1/2 3/5 2/3 3/4 4/5 5/6 8/9 9/10; the reference enum has C7_8 at 9
    static const dvbs2_code_rate_t map[11] = {C1_4, C1_3, C2_5, C1_2, C3_5, C2_3, C3_4, C4_5, C5_6, C8_9, C9_10};
    return map[r];
}
static dvbs2_framesize_t to_fs(int s) { return s ? FECFRAME_SHORT : FECFRAME_NORMAL; }

// The reference's GF(2^m) LOG/EXP tables are static pointers that every BBFrameBCH constructor re-allocates and every destructor
// frees (bch/galois_field.hh:128, bbframe_bch.cpp:183-185,375-377): objects of different threads would pull the tables from under
// each other.  The plugin only ever has one; for the multi-threaded CPU baseline keep one object per (thread, code), construct
// under a lock and never destroy it.
static BBFrameBCH& bch_for(int rate, int shortframe) {
    static std::mutex mtx;
    thread_local std::map<int, BBFrameBCH*> cache;
    BBFrameBCH*& p = cache[rate * 2 + shortframe];
    if (!p) {
        std::lock_guard<std::mutex> lk(mtx);
        p = new BBFrameBCH(to_fs(shortframe), to_rate(rate));
    }
    return *p;
}

extern "C" {

// BBFrameLDPC::decode exactly as the plugin calls it (one frame, lane 0).  bbframe_ldpc.cpp:123-139
int ref_ldpc_decode(int rate, int shortframe, int8_t* frame, int max_trials) {
    BBFrameLDPC ldpc(to_fs(shortframe), to_rate(rate));
    return ldpc.decode(frame, max_trials);
}

// Decode `nframes` frames one after the other with one decoder object (amortises table set-up).
void ref_ldpc_decode_many(int rate, int shortframe, int8_t* frames, int nframes, int max_trials, int* trials_out) {
    BBFrameLDPC ldpc(to_fs(shortframe), to_rate(rate));
    int n = shortframe ? 16200 : 64800;
    for (int f = 0; f < nframes; ++f) trials_out[f] = ldpc.decode(frames + (size_t)f * n, max_trials);
}

// The library used the way its SIMD type was designed for (bbframe_ldpc.h:21-22): 16 frames, one per
// int8 lane, one decoder call.  Used only as the "library-intended" CPU baseline.
// frames: 16 x N, frame-major.  Returns the decoder's raw `trials` value (remaining, or -1).
int ref_ldpc_decode_simd16(int rate, int shortframe, int8_t* frames, int max_trials, int reps) {
    BBFrameLDPC holder(to_fs(shortframe), to_rate(rate));
    LDPCDecoder<simd_type, algorithm_type> dec;
    dec.init(holder.get_instance());
    int n = shortframe ? 16200 : 64800;
    int k = holder.dataSize();
    const int W = simd_type::SIZE;
    std::vector<simd_type> buf(n);
    int last = 0;
    for (int rep = 0; rep < reps; ++rep) {
        for (int i = 0; i < n; ++i)
            for (int l = 0; l < W; ++l) reinterpret_cast<int8_t*>(&buf[i])[l] = frames[(size_t)l * n + i];
        last = dec(buf.data(), buf.data() + k, max_trials, W);
    }
    for (int i = 0; i < n; ++i)
        for (int l = 0; l < W; ++l) frames[(size_t)l * n + i] = reinterpret_cast<int8_t*>(&buf[i])[l];
    return last;
}

int ref_simd_width(void) { return simd_type::SIZE; }

// Persistent "library-intended" FEC object for the CPU baseline: tables built ONCE (BBFrameLDPC, LDPCDecoder::init, the thread's
// BBFrameBCH, BBFrameDescrambler), then every call = one 16-lane LDPC decode (input already lane-interleaved: lanes[i*16 + l] = LLR i
// of frame l, so no transposition is timed) + per frame the hard-decision repack of module_dvbs2_demod.cpp:357-360, BCH and descramble.
struct RefFec16 {
    BBFrameLDPC holder;
    LDPCDecoder<simd_type, algorithm_type> dec;
    BBFrameDescrambler descr;
    int rate, sh, n, k;
    std::vector<simd_type> buf;
    std::vector<uint8_t> frame;
    RefFec16(int r, int s) : holder(to_fs(s), to_rate(r)), descr(to_fs(s), to_rate(r)), rate(r), sh(s) {
        dec.init(holder.get_instance());
        n = s ? 16200 : 64800;
        k = holder.dataSize();
        buf.resize(n);
        frame.resize(n / 8);
    }
};
void* ref_fec16_create(int rate, int shortframe) { return new RefFec16(rate, shortframe); }
void ref_fec16_destroy(void* h) { delete (RefFec16*)h; }
// returns the decoder's raw trials value of the 16-lane call; bb_out (optional): 16 x kbch_bytes descrambled BBFRAMEs
int ref_fec16_run(void* h, const int8_t* lanes, int max_trials, uint8_t* bb_out, int kbch_bytes) {
    RefFec16* f = (RefFec16*)h;
    const int W = simd_type::SIZE;
    memcpy((void*)f->buf.data(), lanes, (size_t)f->n * W);
    const int ret = f->dec(f->buf.data(), f->buf.data() + f->k, max_trials, W);
    BBFrameBCH& bch = bch_for(f->rate, f->sh);
    for (int l = 0; l < W; ++l) {
        uint8_t* fr = f->frame.data();
        memset(fr, 0, f->frame.size());
        for (int i = 0; i < f->k; ++i) fr[i / 8] = (uint8_t)(fr[i / 8] << 1 | (reinterpret_cast<const int8_t*>(&f->buf[i])[l] < 0));
        bch.decode(fr);
        f->descr.work(fr);
        if (bb_out) memcpy(bb_out + (size_t)l * kbch_bytes, fr, kbch_bytes);
    }
    return ret;
}
const char* ref_build_flags(void) { return REF_BUILD_FLAGS; }

int ref_bch_decode(int rate, int shortframe, uint8_t* frame) { return bch_for(rate, shortframe).decode(frame); }

void ref_bch_decode_many(int rate, int shortframe, uint8_t* frames, int nframes, int nbch_bytes, int* corr_out) {
    BBFrameBCH& bch = bch_for(rate, shortframe);
    int nb = nbch_bytes;
    for (int f = 0; f < nframes; ++f) corr_out[f] = bch.decode(frames + (size_t)f * nb);
}

void ref_bch_encode(int rate, int shortframe, uint8_t* frame) {
    bch_for(rate, shortframe).encode(frame);
}

void ref_bb_descramble(int rate, int shortframe, uint8_t* frame) {
    BBFrameDescrambler d(to_fs(shortframe), to_rate(rate));
    d.work(frame);
}

void ref_deinterleave(int constel, int rate, int shortframe, int8_t* in, int8_t* out) {
    S2Deinterleaver d((dvbs2_constellation_t)constel, to_fs(shortframe), to_rate(rate));
    d.deinterleave(in, out);
}

}  // extern "C"

// ---------------------------------------------------------------------------------- DVB-S pieces that compile as is
#include "dvbs/depunc.h"
#include "dvbs/dvbs_interleaving.h"
#include "common/codings/rotation.h"

extern "C" {
void* ref_depunc23_create() { return new viterbi::Depunc23(); }
void* ref_depunc56_create() { return new viterbi::Depunc56(); }
int ref_depunc23_static(void* h, uint8_t* in, uint8_t* out, int size, int shift) { return ((viterbi::Depunc23*)h)->depunc_static(in, out, size, shift); }
int ref_depunc56_static(void* h, uint8_t* in, uint8_t* out, int size, int shift) { return ((viterbi::Depunc56*)h)->depunc_static(in, out, size, shift); }
void ref_depunc23_set_shift(void* h, int s) { ((viterbi::Depunc23*)h)->set_shift(s); }
void ref_depunc56_set_shift(void* h, int s) { ((viterbi::Depunc56*)h)->set_shift(s); }
int ref_depunc23_cont(void* h, uint8_t* in, uint8_t* out, int size) { return ((viterbi::Depunc23*)h)->depunc_cont(in, out, size); }
int ref_depunc56_cont(void* h, uint8_t* in, uint8_t* out, int size) { return ((viterbi::Depunc56*)h)->depunc_cont(in, out, size); }
void* ref_forney_create() { return new dsp::dvbs::DVBSInterleaving(); }
void ref_forney_deinterleave(void* h, uint8_t* in, uint8_t* out) { ((dsp::dvbs::DVBSInterleaving*)h)->deinterleave(in, out); }
void ref_rotate_soft(int8_t* soft, int size, int phase, int iqswap) { rotate_soft(soft, size, (phase_t)phase, iqswap != 0); }
}

// ---------------------------------------------------------------------------------- DVB-S tail: deframer, RS(204,188), descrambler
#include "dvbs/dvbs_ts_deframer.h"
#include "dvbs/dvbs_reedsolomon.h"
#include "dvbs/dvbs_scrambling.h"
extern "C" {
void* ref_tsdef_create() {
    auto* d = new deframing::DVBS_TS_Deframer();
    // the reference leaves its 13 056-bit shifter uninitialised; feed zeros so that runs are reproducible.  One bit per call: what the
    // shifter held may be anything, a recycled bit stream full of sync patterns included, and a bit brings at most one frame
    std::vector<uint8_t> o(2 * 1632);
    uint8_t z = 0;
    for (int i = 0; i < 1632 * 8; ++i) d->work(&z, 1, o.data());
    return d;
}
int ref_tsdef_work(void* h, uint8_t* bits, int size, uint8_t* out) { return ((deframing::DVBS_TS_Deframer*)h)->work(bits, size, out); }
void* ref_dvbsrs_create() { return new dsp::dvbs::DVBSReedSolomon(); }
int ref_dvbsrs_decode(void* h, uint8_t* data204) { return ((dsp::dvbs::DVBSReedSolomon*)h)->decode(data204); }
void* ref_dvbsdescr_create() { return new dsp::dvbs::DVBSScrambling(); }
void ref_dvbsdescr_work(void* h, uint8_t* frm) { ((dsp::dvbs::DVBSScrambling*)h)->descramble(frm); }
}

// ---------------------------------------------------------------------------------- DVB-S inner code: Viterbi_DVBS, CCDecoder, CCEncoder
// These translation units include VOLK and nng headers for a container, a kernel query and nothing else; oracle/shim/ stands
// in for those headers (no arithmetic there: the ACS kernel that runs is the reference's own volk_k7_r2_generic_fixed.h).
#include "dvbs/viterbi_all.h"
#include "dvbs/dvbs_defines.h"
#include <new>

// Viterbi_DVBS keeps the phase it locked on private, hands its shift out as a bool (viterbi_all.h:158) and its d_ber only
// while locked (ber() of an idle decoder is the smallest BER of the last search, viterbi_all.cpp:282-311).  Explicit
// instantiation may name private members, which gives read access without touching the reference's text.
template <class Tag, typename Tag::type M>
struct PrivateMember {
    friend typename Tag::type member_of(Tag) { return M; }
};
struct VitPhase { typedef phase_t viterbi::Viterbi_DVBS::*type; friend type member_of(VitPhase); };
struct VitShift { typedef int viterbi::Viterbi_DVBS::*type; friend type member_of(VitShift); };
template struct PrivateMember<VitPhase, &viterbi::Viterbi_DVBS::d_phase>;
template struct PrivateMember<VitShift, &viterbi::Viterbi_DVBS::d_shift>;
struct VitBer { typedef float viterbi::Viterbi_DVBS::*type; friend type member_of(VitBer); };
template struct PrivateMember<VitBer, &viterbi::Viterbi_DVBS::d_ber>;

extern "C" {
// Constructed exactly as module_dvbs_demod.cpp:23 does: VIT_BUF_SIZE and {PHASE_0, PHASE_90}.  NOT the class's default of four
// phases: work() indexes d_bers_*[2][12] with the phase (viterbi_all.cpp:91,115,140,164,189), so PHASE_180 / PHASE_270 write
// rows 2 and 3 of two-row arrays and overwrite the members that follow (seen under UBSan, and as a crash).
//
// The object is built in storage that was zeroed first, so that the members the constructor leaves alone read 0 instead of
// heap garbage: d_rate / d_phase / d_shift until the first lock (viterbi_all.h:44-46), and ber_depunc_buffer (:77), of which
// the rate-7/8 test decoder reads 2 * (1792 + 6) = 3596 bytes (cc_decoder.cpp:297 from viterbi_all.cpp:186) although no
// de-puncturer ever writes beyond byte 3584 of it.  Zero is what the oracle and the engine define for those bytes.
void* ref_viterbi_create(float thr, int max_outsync) {
    void* mem = operator new(sizeof(viterbi::Viterbi_DVBS));
    memset(mem, 0, sizeof(viterbi::Viterbi_DVBS));
    return new (mem) viterbi::Viterbi_DVBS(thr, max_outsync, VIT_BUF_SIZE, {PHASE_0, PHASE_90});
}
void ref_viterbi_destroy(void* h) { delete (viterbi::Viterbi_DVBS*)h; }
int ref_viterbi_buf_size(void) { return VIT_BUF_SIZE; }
// `input` is rotated in place when the decoder is locked (viterbi_all.cpp:211)
int ref_viterbi_work(void* h, int8_t* input, int size, uint8_t* output) { return ((viterbi::Viterbi_DVBS*)h)->work(input, size, output); }
float ref_viterbi_ber(void* h) { return ((viterbi::Viterbi_DVBS*)h)->ber(); }
int ref_viterbi_state(void* h) { return ((viterbi::Viterbi_DVBS*)h)->getState(); }
int ref_viterbi_rate(void* h) { return (int)((viterbi::Viterbi_DVBS*)h)->rate(); }
int ref_viterbi_getshift(void* h) { return ((viterbi::Viterbi_DVBS*)h)->getshift(); }
int ref_viterbi_phase(void* h) { return (int)(((viterbi::Viterbi_DVBS*)h)->*member_of(VitPhase())); }
int ref_viterbi_shift(void* h) { return ((viterbi::Viterbi_DVBS*)h)->*member_of(VitShift()); }
float ref_viterbi_d_ber(void* h) { return ((viterbi::Viterbi_DVBS*)h)->*member_of(VitBer()); }

// K = 7, r = 1/2, polynomials {79, 109}: the arguments of every decoder / encoder in viterbi_all.cpp:17-32
void* ref_ccdec_create(int frame) { return new viterbi::CCDecoder(frame, 7, 2, {79, 109}); }
void ref_ccdec_destroy(void* h) { delete (viterbi::CCDecoder*)h; }
void ref_ccdec_work(void* h, uint8_t* in, uint8_t* out) { ((viterbi::CCDecoder*)h)->work(in, out); }
void* ref_ccenc_create(int frame) { return new viterbi::CCEncoder(frame, 7, 2, {79, 109}); }
void ref_ccenc_destroy(void* h) { delete (viterbi::CCEncoder*)h; }
void ref_ccenc_work(void* h, uint8_t* in, uint8_t* out) { ((viterbi::CCEncoder*)h)->work(in, out); }
}

// ---------------------------------------------------------------------------------- BBFRAME -> TS / GSE parser
#include "dvbs2/bbframe_ts_parser.h"
namespace {
// The reference's parser trusts its input: a GSE length field can send its reads past the last BBFRAME of the call and its
// writes past `buffer_outsize` (bbframe_ts_parser.cpp:269,311,334,357,371 have no bound).  So that such a call neither faults
// nor goes unnoticed, work() runs on private copies with guard zones behind both buffers: the input guard is filled with a
// byte the caller chooses (two handles with different fills give different results exactly where out-of-bounds input
// mattered), the output guard with a canary that is checked afterwards.
struct RefBbTs {
    dsp::dvbs2::BBFrameTSParser* p;
    int kbch = 0, left_output = 0;
    uint8_t guard_fill;
    std::vector<uint8_t> in, out;
};
const size_t BBTS_GUARD = 1 << 20;
const uint8_t BBTS_CANARY = 0xC5;
}
extern "C" {
void* ref_bbts_create(int kbch_bits, int guard_fill) {
    auto* r = new RefBbTs();
    // BBFrameTSParser has no constructor and leaves count, synched, df_remaining, ... uninitialised (bbframe_ts_parser.h:79-89);
    // value-initialisation zeroes them so that runs are reproducible
    r->p = new dsp::dvbs2::BBFrameTSParser();
    r->guard_fill = (uint8_t)guard_fill;
    r->kbch = kbch_bits;
    r->p->setFrameSize(kbch_bits);
    return r;
}
void ref_bbts_destroy(void* h) { delete ((RefBbTs*)h)->p; delete (RefBbTs*)h; }
void ref_bbts_set_frame_size(void* h, int kbch_bits) { ((RefBbTs*)h)->kbch = kbch_bits; ((RefBbTs*)h)->p->setFrameSize(kbch_bits); }
// `out` holds `cap` bytes, pre-filled by the caller; at most `cap` bytes come back whatever the return value says
int ref_bbts_work(void* h, const uint8_t* bbframes, int cnt, uint8_t* out, int cap) {
    RefBbTs* r = (RefBbTs*)h;
    const size_t nin = (size_t)(r->kbch / 8) * cnt;
    r->in.assign(nin + BBTS_GUARD, r->guard_fill);
    memcpy(r->in.data(), bbframes, nin);
    r->out.assign((size_t)cap + BBTS_GUARD, BBTS_CANARY);
    memcpy(r->out.data(), out, cap);
    const int n = r->p->work(r->in.data(), cnt, r->out.data(), cap);
    memcpy(out, r->out.data(), cap);
    r->left_output = n > cap;
    for (size_t i = cap; i < r->out.size() && !r->left_output; ++i) r->left_output = r->out[i] != BBTS_CANARY;
    return n;
}
// 1 when the last work() wrote beyond `cap`
int ref_bbts_left_output(void* h) { return ((RefBbTs*)h)->left_output; }
// the public fields: {ts_gs, sis_mis, ccm_acm, issyi, npd, ro, isi, upl, dfl, sync, syncd, last_gse_crc_err, last_bb_cnt, last_bb_proc, last_ts_errs}
void ref_bbts_get_fields(void* h, int32_t* o15) {
    const dsp::dvbs2::BBFrameTSParser* p = ((RefBbTs*)h)->p;
    const dsp::dvbs2::BBHeader& q = p->last_header;
    const int v[15] = {q.ts_gs, q.sis_mis, q.ccm_acm, q.issyi, q.npd, q.ro, q.isi, q.upl, q.dfl, q.sync, q.syncd,
                       p->last_gse_crc_err, p->last_bb_cnt, p->last_bb_proc, p->last_ts_errs};
    for (int i = 0; i < 15; ++i) o15[i] = v[i];
}
}

// ---------------------------------------------------------------------------------- S2 physical layer: the integer tables
// MODCOD -> configuration (modcod_to_cfg.cpp), SOF word and PLS codewords (s2_defs.h), Gold sequence and the four rotations
// (s2_scrambling.cpp), over shim/dsp/types.h: complex_t as two float fields.  The float symbol tables of s2_defs.h and everything
// in constellation.cpp need SDR++ core's arithmetic and are not reached from here.
#include <stdexcept>
#include "dvbs2/codings/modcod_to_cfg.h"
#include "dvbs2/codings/s2_scrambling.h"
#include "dvbs2/s2_defs.h"
#include <memory>

// the reference's rate enum has C7_8 between C5_6 and C8_9, ours has not: by name, never by number
static int our_rate(dvbs2_code_rate_t r) {
    switch (r) {
        case C1_4: return 0; case C1_3: return 1; case C2_5: return 2; case C1_2: return 3; case C3_5: return 4; case C2_3: return 5;
        case C3_4: return 6; case C4_5: return 7; case C5_6: return 8; case C8_9: return 9; case C9_10: return 10;
        default: return -1;     // C7_8, or a field the reference left unset
    }
}
static int our_constel(dvbs2_constellation_t c) {
    switch (c) { case MOD_QPSK: return 0; case MOD_8PSK: return 1; case MOD_16APSK: return 2; case MOD_32APSK: return 3; default: return -1; }
}

extern "C" {
// get_dvbs2_cfg: out4 = {slot count, constellation 0..3, rate as OUR index 0..10, short frame 0/1}, g = {g1, g2}.
// dvb_cgf_holder is not initialised by the reference: g[0] is meaningful only for 16APSK and 32APSK, g[1] only for 32APSK
// (modcod_to_cfg.cpp:66-132); the others are returned as NaN so that nobody records or compares them by accident.
// Returns 0, or -1 where the reference throws (MODCOD <= 0 or >= 29, :11,135).
int ref_modcod_cfg(int modcod, int shortframes, int pilots, int* out4, float* g) {
    try {
        dvb_cgf_holder c = get_dvbs2_cfg(modcod, shortframes != 0, pilots != 0);
        out4[0] = c.frame_slot_count; out4[1] = our_constel(c.constellation); out4[2] = our_rate(c.coderate);
        out4[3] = c.framesize == FECFRAME_SHORT ? 1 : c.framesize == FECFRAME_NORMAL ? 0 : -1;
        const float nan = __builtin_nanf("");
        g[0] = c.constellation == MOD_16APSK || c.constellation == MOD_32APSK ? c.g1 : nan;
        g[1] = c.constellation == MOD_32APSK ? c.g2 : nan;
        return c.pilots == (pilots != 0) ? 0 : -2;
    } catch (const std::runtime_error&) {
        return -1;
    }
}
// get_dvbs2_modcod of what get_dvbs2_cfg returned: the reverse map (:142-221)
int ref_modcod_roundtrip(int modcod, int shortframes, int pilots) {
    try {
        return get_dvbs2_modcod(get_dvbs2_cfg(modcod, shortframes != 0, pilots != 0));
    } catch (const std::runtime_error&) {
        return -1;
    }
}
// s2_plscodes::codewords, and sof3 = {s2_sof::VALUE, MASK, LENGTH}
void ref_pls_codewords(uint64_t* out128, uint32_t* sof3) {
    std::unique_ptr<s2_plscodes> p(new s2_plscodes());
    for (int i = 0; i < s2_plscodes::COUNT; ++i) out128[i] = p->codewords[i];
    sof3[0] = s2_sof::VALUE; sof3[1] = s2_sof::MASK; sof3[2] = (uint32_t)s2_sof::LENGTH;
}
// Rn[0..131071] of S2Scrambling(codenum), read through the public interface: descramble() turns (1, 2) into one of four
// distinct pairs, one per rotation.  Entries that are none of the four come back as 255.
void ref_gold_sequence(int codenum, uint8_t* out131072) {
    std::unique_ptr<S2Scrambling> s(new S2Scrambling(codenum));
    s->reset();
    for (int i = 0; i < 131072; ++i) {
        dsp::complex_t p = {1.0f, 2.0f};
        dsp::complex_t q = s->descramble(p);
        out131072[i] = q.re == 1.0f && q.im == 2.0f ? 0 : q.re == 2.0f && q.im == -1.0f ? 1 : q.re == -1.0f && q.im == -2.0f ? 2
                     : q.re == -2.0f && q.im == 1.0f ? 3 : 255;
    }
}
// out16[4 * r + {0, 1, 2, 3}] = scramble((1, 2)).re, .im, descramble((1, 2)).re, .im at a position whose Rn is r (code number 0).
// Returns 0, or -1 when some r does not occur in `rn`, the sequence ref_gold_sequence(0) returned.
int ref_scramble_cases(const uint8_t* rn131072, float* out16) {
    std::unique_ptr<S2Scrambling> s(new S2Scrambling(0));
    for (int r = 0; r < 4; ++r) {
        int pos = 0;
        while (pos < 131072 && rn131072[pos] != r) ++pos;
        if (pos == 131072) return -1;
        dsp::complex_t p = {1.0f, 2.0f};
        s->setPos(pos);
        dsp::complex_t a = s->scramble(p);
        s->setPos(pos);
        dsp::complex_t b = s->descramble(p);
        out16[4 * r] = a.re; out16[4 * r + 1] = a.im; out16[4 * r + 2] = b.re; out16[4 * r + 3] = b.im;
    }
    return 0;
}
}
