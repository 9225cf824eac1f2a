// csrc/fec_parts.h on its own, no GPU: how the pooled frames of a call are divided into FEC parts and laid out in the job's buffers.  Over the cases of main():
// every frame with a part is exactly once in the index list, inside its part's range; the parts' LLR, BBFRAME and result ranges are pairwise disjoint and end
// within the totals; BBFRAME offsets are multiples of BB_PAD; frame_tr / frame_co lie in the trials / corrections half of the frame's part and are -1 exactly
// for the frames without a part; frame_llr is the frame's place among its part's LLRs; parts come in order of first appearance; the same input gives the same plan.
// Exit status 0: all checks passed; otherwise the failed checks are on stderr.
#include "fec_parts.h"

#include <cstdio>
#include <vector>

using s2::FecParts;

static int failures = 0;
#define CHECK(cond, ...)                                                          \
    do {                                                                          \
        if (!(cond)) { ++failures; fprintf(stderr, "FAILED %s: ", #cond); fprintf(stderr, __VA_ARGS__); fputc('\n', stderr); } \
    } while (0)

struct Code { int code_index, N, kb; };
// (N, kbch / 8) of the ten short codes, rates 1/4 .. 8/9, and of three normal ones (1/2, 3/4, 9/10); code_index as the library numbers them does not matter here
static const Code SHORT[] = {{11, 16200, 384}, {12, 16200, 654}, {13, 16200, 789}, {14, 16200, 879}, {15, 16200, 1194},
                             {16, 16200, 1329}, {17, 16200, 1464}, {18, 16200, 1554}, {19, 16200, 1644}, {20, 16200, 1779}};
static const Code NORMAL[] = {{3, 64800, 4026}, {6, 64800, 6051}, {10, 64800, 7274}};

struct Frame { bool has; Code c; int mt, force; };
static Frame none() { return Frame{false, Code{-1, 0, 0}, 0, 0}; }
static Frame of(const Code& c, int mt = 16, int force = 0) { return Frame{true, c, mt, force}; }

static FecParts plan_of(const std::vector<Frame>& frames) {
    FecParts P;
    for (const Frame& f : frames) {
        if (f.has) P.add(f.c.code_index, f.mt, f.force, f.c.N, f.c.kb);
        else P.add_none();
    }
    P.layout();
    return P;
}

static bool disjoint(size_t a0, size_t a1, size_t b0, size_t b1) { return a1 <= b0 || b1 <= a0; }

static void check(const std::vector<Frame>& frames, const char* what) {
    const FecParts P = plan_of(frames);
    const int nf = (int)frames.size();
    CHECK(P.nf() == nf && (int)P.part_of.size() == nf && (int)P.frame_tr.size() == nf && (int)P.frame_co.size() == nf && (int)P.frame_llr.size() == nf, "%s: per-frame tables of %d frames", what, nf);
    if (P.nf() != nf || (int)P.frame_tr.size() != nf) return;
    // the index list: every frame with a part once, inside its part's range; none of the others
    std::vector<int> seen(nf, 0);
    size_t with_part = 0;
    for (int f = 0; f < nf; ++f) with_part += frames[f].has;
    CHECK(P.idx.size() == with_part, "%s: index list of %zu entries for %zu frames with a part", what, P.idx.size(), with_part);
    for (int x : P.idx) {
        CHECK(x >= 0 && x < nf && frames[x].has, "%s: index list names frame %d", what, x);
        if (x >= 0 && x < nf) ++seen[x];
    }
    size_t first_seen = 0;
    for (size_t p = 0; p < P.parts.size(); ++p) {
        const FecParts::Part& A = P.parts[p];
        const size_t cnt = A.frames.size();
        CHECK(cnt > 0 && (size_t)A.cnt() == cnt, "%s: part %zu is empty", what, p);
        if (!cnt) continue;
        // first-appearance order: the first frame of each part comes behind the first frame of the part before it, and no earlier frame has this part's key
        CHECK(p == 0 || (size_t)A.frames[0] > first_seen, "%s: part %zu first appears at frame %d, not behind part %zu's", what, p, A.frames[0], p - 1);
        first_seen = (size_t)A.frames[0];
        for (int f = 0; f < A.frames[0]; ++f)
            CHECK(!(frames[f].has && frames[f].c.code_index == A.code_index && frames[f].mt == A.max_trials && frames[f].force == A.force), "%s: frame %d belongs to part %zu, which starts at %d", what, f, p, A.frames[0]);
        CHECK(A.io + cnt <= P.idx.size(), "%s: part %zu's index range ends behind the list", what, p);
        CHECK(A.bo % FecParts::BB_PAD == 0, "%s: part %zu's BBFRAMEs at %zu", what, p, A.bo);
        CHECK(A.lo + cnt * A.N <= P.llr_bytes && A.bo + cnt * A.kb <= P.bb_bytes && A.to + 2 * cnt <= P.n_results, "%s: part %zu ends behind a total", what, p);
        for (size_t q = p + 1; q < P.parts.size(); ++q) {
            const FecParts::Part& B = P.parts[q];
            const size_t cb = B.frames.size();
            CHECK(!(A.code_index == B.code_index && A.max_trials == B.max_trials && A.force == B.force), "%s: parts %zu and %zu share a key", what, p, q);
            CHECK(disjoint(A.lo, A.lo + cnt * A.N, B.lo, B.lo + cb * B.N), "%s: LLRs of parts %zu and %zu overlap", what, p, q);
            CHECK(disjoint(A.bo, A.bo + cnt * A.kb, B.bo, B.bo + cb * B.kb), "%s: BBFRAMEs of parts %zu and %zu overlap", what, p, q);
            CHECK(disjoint(A.to, A.to + 2 * cnt, B.to, B.to + 2 * cb), "%s: results of parts %zu and %zu overlap", what, p, q);
            CHECK(disjoint(A.io, A.io + cnt, B.io, B.io + cb), "%s: index ranges of parts %zu and %zu overlap", what, p, q);
        }
        for (size_t k = 0; k < cnt && A.io + cnt <= P.idx.size(); ++k) {
            const int f = A.frames[k];
            CHECK(P.idx[A.io + k] == f, "%s: part %zu's list entry %zu is %d, its frame %d", what, p, k, P.idx[A.io + k], f);
            if (f < 0 || f >= nf) continue;
            CHECK(P.part_of[f] == (int)p && frames[f].has && frames[f].c.code_index == A.code_index && frames[f].c.N == A.N && frames[f].c.kb == A.kb &&
                  frames[f].mt == A.max_trials && frames[f].force == A.force, "%s: frame %d in part %zu", what, f, p);
            CHECK(P.frame_llr[f] == A.lo + k * A.N, "%s: frame %d's LLRs at %zu", what, f, P.frame_llr[f]);
        }
    }
    for (int f = 0; f < nf; ++f) {
        CHECK(seen[f] == (frames[f].has ? 1 : 0), "%s: frame %d is %d times in the index list", what, f, seen[f]);
        if (!frames[f].has) {
            CHECK(P.part_of[f] == -1 && P.frame_tr[f] == -1 && P.frame_co[f] == -1, "%s: frame %d has no part but (%d, %d, %d)", what, f, P.part_of[f], P.frame_tr[f], P.frame_co[f]);
            continue;
        }
        const int p = P.part_of[f];
        CHECK(p >= 0 && p < (int)P.parts.size(), "%s: frame %d in part %d", what, f, p);
        if (p < 0 || p >= (int)P.parts.size()) continue;
        const long to = (long)P.parts[p].to, cnt = P.parts[p].cnt();
        CHECK(P.frame_tr[f] >= to && P.frame_tr[f] < to + cnt, "%s: frame %d's trial count at %d, its part's at [%ld, %ld)", what, f, P.frame_tr[f], to, to + cnt);
        CHECK(P.frame_co[f] >= to + cnt && P.frame_co[f] < to + 2 * cnt, "%s: frame %d's correction count at %d, its part's at [%ld, %ld)", what, f, P.frame_co[f], to + cnt, to + 2 * cnt);
        CHECK(P.frame_co[f] - P.frame_tr[f] == cnt, "%s: frame %d's two results are %d apart", what, f, P.frame_co[f] - P.frame_tr[f]);
    }
    if (with_part == 0) CHECK(P.parts.empty() && P.llr_bytes == 0 && P.bb_bytes == 0 && P.n_results == 0, "%s: no frame has a part, yet there are %zu parts", what, P.parts.size());
    // the same input gives the same plan; and layout() again changes nothing
    FecParts Q = plan_of(frames);
    Q.layout();
    bool same = Q.parts.size() == P.parts.size() && Q.idx == P.idx && Q.frame_tr == P.frame_tr && Q.frame_co == P.frame_co && Q.frame_llr == P.frame_llr &&
                Q.part_of == P.part_of && Q.llr_bytes == P.llr_bytes && Q.bb_bytes == P.bb_bytes && Q.n_results == P.n_results;
    for (size_t p = 0; same && p < P.parts.size(); ++p)
        same = Q.parts[p].frames == P.parts[p].frames && Q.parts[p].lo == P.parts[p].lo && Q.parts[p].bo == P.parts[p].bo && Q.parts[p].to == P.parts[p].to && Q.parts[p].io == P.parts[p].io;
    CHECK(same, "%s: the same input gave another plan", what);
}

int main() {
    check({}, "no frames");
    check({none(), none(), none()}, "frames that all have no part");
    check({none()}, "one frame, no part");
    check({of(SHORT[3])}, "one part of one frame");
    // several parts with odd counts (3, 5, 1), interleaved, dummy frames between them: parts in order 1329, 1644, 879
    check({of(SHORT[5]), none(), of(SHORT[8]), of(SHORT[5]), of(SHORT[8]), of(SHORT[3]), of(SHORT[8]), none(), of(SHORT[5]), of(SHORT[8]), of(SHORT[8])}, "three parts, odd counts");
    {
        const FecParts P = plan_of({of(SHORT[5]), none(), of(SHORT[8]), of(SHORT[5]), of(SHORT[3])});
        CHECK(P.parts.size() == 3 && P.parts[0].kb == 1329 && P.parts[1].kb == 1644 && P.parts[2].kb == 879, "first-appearance order: %zu parts", P.parts.size());
        CHECK(P.llr_bytes == 4 * 16200 && P.n_results == 8 && P.bb_bytes == 2688 + 1664 + 896, "totals %zu / %zu / %zu", P.llr_bytes, P.bb_bytes, P.n_results);
        CHECK(P.idx == (std::vector<int>{0, 3, 2, 4}), "index list in part order");
    }
    // the same code with two iteration settings (and a forced one): three parts
    check({of(SHORT[3], 16, 0), of(SHORT[3], 25, 0), of(SHORT[3], 16, 0), of(SHORT[3], 25, 1), of(SHORT[3], 25, 0)}, "one code, three iteration settings");
    CHECK(plan_of({of(SHORT[3], 16, 0), of(SHORT[3], 25, 0), of(SHORT[3], 25, 1)}).parts.size() == 3, "iteration settings are part of the key");
    // every short code, 1 .. 10 frames each, stream-major as a mixed batch pools them; then one frame each in turn as an ACM/VCM stream does
    {
        std::vector<Frame> a, b;
        for (int c = 0; c < 10; ++c)
            for (int k = 0; k <= c; ++k) a.push_back(of(SHORT[c]));
        for (int k = 0; k < 3; ++k)
            for (int c = 9; c >= 0; --c) { b.push_back(of(SHORT[c])); if (c % 4 == 0) b.push_back(none()); }
        check(a, "all short codes, stream-major");
        check(b, "all short codes, cycling");
        // odd kb (879, 1329, 1779) with odd counts: the next part's BBFRAMEs still start at a multiple of BB_PAD
        check({of(SHORT[3]), of(SHORT[9]), of(SHORT[5]), of(SHORT[9]), of(SHORT[9])}, "odd BBFRAME sizes");
    }
    // normal codes, alone and beside short ones
    check({of(NORMAL[1]), of(NORMAL[1]), of(NORMAL[1])}, "one normal code");
    check({of(NORMAL[0]), of(SHORT[3]), none(), of(NORMAL[2]), of(NORMAL[0]), of(SHORT[9]), of(NORMAL[1])}, "normal and short codes");
    if (failures) fprintf(stderr, "%d checks failed\n", failures);
    return failures ? 1 : 0;
}
