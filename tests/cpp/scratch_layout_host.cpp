// csrc/scratch_layout.h on its own, no GPU: for layouts that mix 1-, 2-, 4-, 8- and 16-byte element types (and an over-aligned one) with
// counts 0, 1, odd and large, every resolved pointer meets max(alignof(T), 16), no two non-empty sub-arrays overlap, the last one ends
// at or before bytes(), a zero-count array adds no bytes, and a second base gives the same offsets.
// Exit status 0: all checks passed; otherwise the failed checks are on stderr.
#include "scratch_layout.h"

#include <cstdint>
#include <cstdio>
#include <vector>

using s2::ScratchLayout;
using s2::ScratchPart;

static int failures = 0;
#define CHECK(cond, ...)                                                          \
    do {                                                                          \
        if (!(cond)) { ++failures; fprintf(stderr, "FAILED %s: ", #cond); fprintf(stderr, __VA_ARGS__); fputc('\n', stderr); } \
    } while (0)

struct Span { size_t off, bytes, align; };

// two bases, aligned like device allocations; they are only resolved against, never dereferenced (the large counts need no memory)
static char* const base_a = reinterpret_cast<char*>((uintptr_t)1 << 40);
static char* const base_b = reinterpret_cast<char*>(((uintptr_t)5 << 40) + 256 * 7);

template <typename T>
static void add(ScratchLayout& L, std::vector<Span>& spans, size_t count, const char* what) {
    const size_t before = L.bytes();
    const ScratchPart<T> h = L.add<T>(count);
    const size_t align = alignof(T) > 16 ? alignof(T) : 16;
    T* pa = h(base_a);
    T* pb = h(base_b);
    const size_t off = (size_t)((char*)pa - base_a);
    CHECK(off % align == 0 && (uintptr_t)pa % align == 0, "%s[%zu] at offset %zu, alignment %zu", what, count, off, align);
    CHECK((size_t)((char*)pb - base_b) == off, "%s[%zu]: the second base gives another offset", what, count);
    if (count == 0) {
        CHECK(L.bytes() == before, "%s[0] added %zu bytes", what, L.bytes() - before);
        return;
    }
    CHECK(off >= before, "%s[%zu] starts at %zu inside the %zu bytes declared before it", what, count, off, before);
    CHECK(off + count * sizeof(T) <= L.bytes(), "%s[%zu] ends at %zu, behind bytes() = %zu", what, count, off + count * sizeof(T), L.bytes());
    spans.push_back({off, count * sizeof(T), align});
}

static void check_disjoint(const std::vector<Span>& spans, size_t total, const char* what) {
    for (size_t i = 0; i < spans.size(); ++i) {
        CHECK(spans[i].off + spans[i].bytes <= total, "%s: sub-array %zu ends behind bytes()", what, i);
        for (size_t j = i + 1; j < spans.size(); ++j)
            CHECK(spans[i].off + spans[i].bytes <= spans[j].off || spans[j].off + spans[j].bytes <= spans[i].off, "%s: sub-arrays %zu and %zu overlap", what, i, j);
    }
}

struct alignas(16) Vec16 { float v[4]; };
struct alignas(256) Block256 { unsigned v[64]; };

// every element type at every position of a three-array layout, over the counts
template <typename A, typename B, typename C>
static void mix(const char* what) {
    const size_t counts[] = {0, 1, 3, 7, 1001, ((size_t)1 << 31) + 5};
    for (size_t ca : counts)
        for (size_t cb : counts)
            for (size_t cc : counts) {
                ScratchLayout L;
                std::vector<Span> spans;
                add<A>(L, spans, ca, what); add<B>(L, spans, cb, what); add<C>(L, spans, cc, what);
                check_disjoint(spans, L.bytes(), what);
                if (ca + cb + cc == 0) CHECK(L.bytes() == 0, "%s: an empty layout has %zu bytes", what, L.bytes());
                // offsets depend on the declared types and counts alone: the same declaration again gives the same size
                ScratchLayout M;
                std::vector<Span> again;
                add<A>(M, again, ca, what); add<B>(M, again, cb, what); add<C>(M, again, cc, what);
                CHECK(M.bytes() == L.bytes(), "%s: the same declaration gave %zu and %zu bytes", what, L.bytes(), M.bytes());
            }
}

// The frame buffer of the ACM/VCM flow (s2_demod.hip, process_vcm_group): frame records, frame stats, a table of POINTERS, ints.  Carved by hand
// the table's 8-byte alignment rested on the two struct sizes and on the parity of nf.  The real S2VcmFrame (40 bytes) and S2FrameStats (32 bytes)
// of csrc/s2_rx.h are multiples of 8 (s2_demod.hip asserts these sizes), so the real layout was never at risk; Frame44 / Stats36 are the
// synthetic case, sizes that are 4 mod 8, where nf = 1 and nf = 3 put the table at an odd multiple of 4 unless the layout aligns it.
struct Frame40 { const void* sym; int stream, pls; long long pll_off, llr_off; float sofq; int dst_index; };
struct Stats32 { float best_match; int modcod, shortf, pilots; float fed_err; int trials, corr, bytes; };
struct Frame44 { int w[11]; };
struct Stats36 { int w[9]; };
static_assert(sizeof(Frame40) == 40 && sizeof(Stats32) == 32, "mirrors of S2VcmFrame / S2FrameStats");
static_assert(sizeof(Frame44) % 8 == 4 && sizeof(Stats36) % 8 == 4 && alignof(Frame44) == 4, "the synthetic sizes are 4 mod 8");

template <typename F, typename S>
static void vcm_frames(size_t nf, const char* what) {
    ScratchLayout L;
    std::vector<Span> spans;
    add<F>(L, spans, nf, what); add<S>(L, spans, nf, what); add<uint8_t*>(L, spans, nf, what); add<int>(L, spans, nf, what);
    check_disjoint(spans, L.bytes(), what);
    CHECK(spans.size() == 4 && spans[2].off % alignof(uint8_t*) == 0, "%s, nf = %zu: pointer table at offset %zu", what, nf, spans.size() == 4 ? spans[2].off : 0);
}

int main() {
    mix<uint8_t, int32_t, uint8_t*>("bytes | ints | pointers");
    mix<int32_t, uint8_t*, Vec16>("ints | pointers | 16-byte vectors");
    mix<uint8_t*, uint16_t, int32_t>("pointers | halves | ints");
    mix<Vec16, uint8_t, double>("vectors | bytes | doubles");
    mix<uint8_t, Block256, uint32_t>("bytes | a 256-byte-aligned block | words");
    for (size_t nf : {(size_t)1, (size_t)3, (size_t)4, (size_t)1001}) {
        vcm_frames<Frame40, Stats32>(nf, "frame buffer, real sizes");
        vcm_frames<Frame44, Stats36>(nf, "frame buffer, sizes 4 mod 8");
    }
    if (failures) fprintf(stderr, "%d checks failed\n", failures);
    return failures ? 1 : 0;
}
