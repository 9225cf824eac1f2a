// The layout of one scratch buffer that holds several arrays: declared once, in order, as typed sub-arrays with their counts; the
// same declaration gives the buffer's size and every array's pointer.
//     ScratchLayout L;
//     const auto frames = L.add<S2FrameRef>(nf), first = L.add<int>(n + 1);     // handles: offsets, no memory yet
//     ws.ensure(L.bytes());
//     S2FrameRef* d_frames = frames(ws.p);                                      // resolved against any base, any number of times
// Every sub-array starts at a multiple of max(alignof(T), 16) bytes from the base (the base itself is a device allocation, aligned
// far beyond that): a pointer table behind an odd number of 4-byte elements is aligned by construction, and 16-byte vector accesses
// to any array are too.  A count of 0 takes no space.  Offsets depend on the declared types and counts alone.
// Standard headers only: the host tests compile this file with a plain C++ compiler.
#pragma once
#include <cstddef>

namespace s2 {

template <typename T>
struct ScratchPart {
    size_t off = 0;
    T* operator()(void* base) const { return reinterpret_cast<T*>(static_cast<char*>(base) + off); }
};

class ScratchLayout {
    size_t total_ = 0;      // a multiple of 16 between declarations
public:
    template <typename T>
    ScratchPart<T> add(size_t count) {
        constexpr size_t a = alignof(T) > 16 ? alignof(T) : 16;
        const size_t off = (total_ + a - 1) / a * a;
        if (count) total_ = (off + count * sizeof(T) + 15) / 16 * 16;
        return {off};
    }
    size_t bytes() const { return total_; }
};

}  // namespace s2
