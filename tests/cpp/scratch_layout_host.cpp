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

// The job buffer of a FEC job in parts (s2_demod.hip, build_parts_job; the ACM/VCM and the mixed flow): int32 results[2 * nall] | int indices[nall] | a table
// of nf POINTERS, nall <= nf the frames that have a part.  Carved by hand the table would sit behind 3 * nall four-byte words: at an odd multiple of 4 for
// every odd nall (nf = 1 and nf = 3 among them) unless the layout aligns it.
static void vcm_frames(size_t nall, size_t nf, const char* what) {
    ScratchLayout L;
    std::vector<Span> spans;
    add<int32_t>(L, spans, 2 * nall, what); add<int>(L, spans, nall, what); add<uint8_t*>(L, spans, nf, what);
    check_disjoint(spans, L.bytes(), what);
    // (an empty array leaves no span: the table is the last one)
    const bool all_there = spans.size() == (nall ? 3u : 1u);
    CHECK(all_there && spans.back().off % alignof(uint8_t*) == 0, "%s, nall = %zu, nf = %zu: pointer table at offset %zu", what, nall, nf, all_there ? spans.back().off : 0);
}

int main() {
    mix<uint8_t, int32_t, uint8_t*>("bytes | ints | pointers");
    mix<int32_t, uint8_t*, Vec16>("ints | pointers | 16-byte vectors");
    mix<uint8_t*, uint16_t, int32_t>("pointers | halves | ints");
    mix<Vec16, uint8_t, double>("vectors | bytes | doubles");
    mix<uint8_t, Block256, uint32_t>("bytes | a 256-byte-aligned block | words");
    for (size_t nf : {(size_t)1, (size_t)3, (size_t)4, (size_t)1001}) {
        vcm_frames(nf, nf, "job buffer, every frame in a part");
        vcm_frames(nf | 1, (nf | 1) + 2, "job buffer, an odd count of frames in parts among dummy PLFRAMEs");
        vcm_frames(0, nf, "job buffer, dummy PLFRAMEs only");
    }
    if (failures) fprintf(stderr, "%d checks failed\n", failures);
    return failures ? 1 : 0;
}
