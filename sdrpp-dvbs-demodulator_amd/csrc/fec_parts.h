// How the pooled frames of a call whose frames differ in LDPC code or iteration setting (ACM/VCM streams, mixed CCM batches) are divided
// into FEC parts -- one decoder job each -- and where every part lies in the job's three buffers:
//     LLRs      part after part, cnt * N bytes each
//     BBFRAMEs  part after part, cnt * kb bytes each, every part at a multiple of BB_PAD
//     results   per part trials[cnt] ++ corrections[cnt] (int32 words), followed in the same buffer by the index list and the destination table
// A part is (LDPC code, iteration limit, forced); parts come in order of first appearance in pooled-frame order (a part exists only with a frame in it).
// A frame without a part (a dummy PLFRAME) takes no room and has no results.
//     FecParts P;  per pooled frame: P.add(...) or P.add_none();  P.layout();
// Standard headers only: the host tests compile this file with a plain C++ compiler.
#pragma once
#include <cstddef>
#include <vector>

namespace s2 {

struct FecParts {
    static constexpr size_t BB_PAD = 64;
    struct Part {
        int code_index, max_trials, force, N, kb;
        std::vector<int> frames;                 // pooled frame indices, ascending
        size_t lo = 0, bo = 0, to = 0, io = 0;   // byte offset of the LLRs / of the BBFRAMEs, word offset of the results, offset into idx
        int cnt() const { return (int)frames.size(); }
    };
    std::vector<Part> parts;
    std::vector<int> part_of;                    // [nf] the frame's part, -1: none
    // layout()
    std::vector<int> idx;                        // the parts' frame lists, part after part
    std::vector<int> frame_tr, frame_co;         // [nf] where the frame's trial count / correction count lies in the results, -1: no part
    std::vector<size_t> frame_llr;               // [nf] byte offset of the frame's LLRs (no part: unused)
    size_t llr_bytes = 0, bb_bytes = 0, n_results = 0;

    int nf() const { return (int)part_of.size(); }
    void add_none() { part_of.push_back(-1); }
    void add(int code_index, int max_trials, int force, int N, int kb) {
        int p = part_of.empty() ? -1 : part_of.back();      // (the frames of a stream mostly follow one another in one part)
        if (p < 0 || !same(parts[p], code_index, max_trials, force))
            for (p = (int)parts.size() - 1; p >= 0 && !same(parts[p], code_index, max_trials, force); --p) {}
        if (p < 0) { p = (int)parts.size(); parts.push_back(Part{code_index, max_trials, force, N, kb, {}}); }
        parts[p].frames.push_back(nf());
        part_of.push_back(p);
    }
    void layout() {
        idx.clear(); frame_tr.assign(nf(), -1); frame_co.assign(nf(), -1); frame_llr.assign(nf(), 0);
        llr_bytes = bb_bytes = n_results = 0;
        for (Part& P : parts) {
            const size_t cnt = P.frames.size();
            P.lo = llr_bytes; P.bo = bb_bytes; P.to = n_results; P.io = idx.size();
            for (size_t k = 0; k < cnt; ++k) {
                const int f = P.frames[k];
                frame_tr[f] = (int)(P.to + k); frame_co[f] = (int)(P.to + cnt + k); frame_llr[f] = P.lo + k * (size_t)P.N;
                idx.push_back(f);
            }
            llr_bytes += cnt * (size_t)P.N;
            bb_bytes += (cnt * (size_t)P.kb + BB_PAD - 1) / BB_PAD * BB_PAD;
            n_results += 2 * cnt;
        }
    }

private:
    static bool same(const Part& P, int code_index, int max_trials, int force) { return P.code_index == code_index && P.max_trials == max_trials && P.force == force; }
};

}  // namespace s2
