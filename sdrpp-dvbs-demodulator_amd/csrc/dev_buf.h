// Ownership of device memory (HIP-free): DevBuf<T> owns one typed block, Workspace one growing scratch block.  Every handle and the context
// hold their device memory in these, so a destroy function (or a create function that fails half way) frees by deleting the struct.  Structs a
// kernel reads keep raw pointers; their owners live beside them.  The allocator itself is called in dev_alloc / dev_free (capi.hip) only.
#pragma once
#include <cstddef>
#include <utility>

namespace s2 {

// 0, or the project's error code with last_error() = "<what>: <the allocator's text>" (*p is then null).  zero: the block is zero-filled.
int dev_alloc(void** p, size_t bytes, bool zero, const char* what);
void dev_free(void* p);     // (null: nothing)

template <typename T>
struct DevBuf {
    T* p = nullptr;
    DevBuf() = default;
    DevBuf(const DevBuf&) = delete;
    DevBuf& operator=(const DevBuf&) = delete;
    DevBuf(DevBuf&& o) noexcept : p(o.p) { o.p = nullptr; }
    DevBuf& operator=(DevBuf&& o) noexcept {
        if (this != &o) { reset(); p = o.p; o.p = nullptr; }
        return *this;
    }
    ~DevBuf() { reset(); }
    // `count` elements (what it held before is freed first); `what` is the label of the error text, e.g. "hipMalloc(tsmon)"
    int alloc(size_t count, bool zero, const char* what) {
        reset();
        return dev_alloc((void**)&p, count * sizeof(T), zero, what);
    }
    void reset() { dev_free(p); p = nullptr; }
    T* get() const { return p; }
    operator T*() const { return p; }
};

// A scratch block that only grows: ensure(n) keeps what is there when it is large enough, else frees it and allocates n plus a quarter
// (so alternating sizes do not thrash).  The contents do not survive a growth.
struct Workspace {
    void* p = nullptr;
    size_t bytes = 0;
    Workspace() = default;
    Workspace(const Workspace&) = delete;
    Workspace& operator=(const Workspace&) = delete;
    Workspace(Workspace&& o) noexcept : p(o.p), bytes(o.bytes) { o.p = nullptr; o.bytes = 0; }
    Workspace& operator=(Workspace&& o) noexcept {
        if (this != &o) { release(); p = o.p; bytes = o.bytes; o.p = nullptr; o.bytes = 0; }
        return *this;
    }
    ~Workspace() { release(); }
    int ensure(size_t n) {
        if (n <= bytes) return 0;
        release();
        const size_t want = n + n / 4;
        const int rc = dev_alloc(&p, want, false, "hipMalloc(workspace)");
        if (rc == 0) bytes = want;
        return rc;
    }
    void release() { dev_free(p); p = nullptr; bytes = 0; }
};

}  // namespace s2
