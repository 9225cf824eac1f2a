// csrc/dev_buf.h on the host, under ASan + UBSan (tests/test_host_cpp_dev_buf.py): DevBuf<T> and Workspace over an allocator of this
// program's own -- counting malloc / free that can be told to fail the k-th request and that records double and foreign frees.  This is
// where the failure paths of the handles' create functions and of the context's table caches are tested; no GPU test asks a card for
// memory it does not have.
#include "../../sdrpp-dvbs-demodulator_amd/csrc/dev_buf.h"

#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <memory>
#include <set>
#include <string>
#include <type_traits>
#include <utility>

using namespace s2;

#define CHECK(c)                                                              \
    do {                                                                      \
        if (!(c)) { printf("FAILED line %d: %s\n", __LINE__, #c); exit(1); }  \
    } while (0)
#define RC_TRY(x)                  \
    do {                           \
        int _rc = (x);             \
        if (_rc) return _rc;       \
    } while (0)

namespace {
constexpr int ERR = -7;
constexpr unsigned char FILL = 0xA5;        // what a fresh block holds unless it was asked for zero-filled
struct Heap {
    std::map<void*, size_t> live;
    std::set<void*> freed;
    long requests = 0, fail_at = 0;         // fail_at: the request (counted from 1) that fails; 0: none
    long frees = 0, double_frees = 0, foreign_frees = 0;
    std::string last_what;
    void arm(long k) { requests = 0; fail_at = k; }
} H;
}  // namespace

namespace s2 {
int dev_alloc(void** p, size_t bytes, bool zero, const char* what) {
    *p = nullptr;
    if (++H.requests == H.fail_at) { H.last_what = what; return ERR; }
    void* q = malloc(bytes ? bytes : 1);
    memset(q, zero ? 0 : FILL, bytes);
    H.live[q] = bytes;
    H.freed.erase(q);
    *p = q;
    return 0;
}
void dev_free(void* p) {
    if (!p) return;
    const auto it = H.live.find(p);
    if (it == H.live.end()) { ++(H.freed.count(p) ? H.double_frees : H.foreign_frees); return; }
    H.live.erase(it);
    H.freed.insert(p);
    ++H.frees;
    free(p);
}
}  // namespace s2

namespace {

static_assert(!std::is_copy_constructible_v<DevBuf<int>> && !std::is_copy_assignable_v<DevBuf<int>>, "an owner is not copied");
static_assert(!std::is_copy_constructible_v<Workspace> && !std::is_copy_assignable_v<Workspace>, "an owner is not copied");
static_assert(std::is_nothrow_move_constructible_v<DevBuf<int>> && std::is_nothrow_move_assignable_v<DevBuf<int>>, "an owner moves");
static_assert(std::is_nothrow_move_constructible_v<Workspace> && std::is_nothrow_move_assignable_v<Workspace>, "an owner moves");

bool all_bytes(const void* p, size_t n, unsigned char v) {
    for (size_t i = 0; i < n; ++i) if (static_cast<const unsigned char*>(p)[i] != v) return false;
    return true;
}

// ---- a struct shaped like a handle: six owners, two lazy ones, a workspace
struct Handle {
    DevBuf<int> state;
    DevBuf<float> hist[2];
    DevBuf<uint8_t> rows, args;
    DevBuf<double> call;
    DevBuf<uint8_t> lazy_in, lazy_out;
    Workspace ws;
};
static_assert(!std::is_copy_constructible_v<Handle>, "a handle is not copied");
int handle_create(int n, Handle** out) {
    *out = nullptr;
    std::unique_ptr<Handle> h(new Handle());
    const char* what = "alloc(handle)";
    RC_TRY(h->state.alloc(n, true, what));
    for (auto& b : h->hist) RC_TRY(b.alloc(2 * n, false, what));
    RC_TRY(h->rows.alloc(16 * n, false, what));
    RC_TRY(h->args.alloc(24, true, what));
    RC_TRY(h->call.alloc(n, false, what));
    *out = h.release();
    return 0;
}
int handle_work(Handle* h, size_t n) {
    if (!h->lazy_in) RC_TRY(h->lazy_in.alloc(n, false, "alloc(handle staging)"));
    if (!h->lazy_out) RC_TRY(h->lazy_out.alloc(2 * n, false, "alloc(handle staging)"));
    return h->ws.ensure(n);
}
// create, two calls (the second grows the workspace), destroy; the first error ends it, as a caller would
int handle_life() {
    Handle* raw = nullptr;
    RC_TRY(handle_create(5, &raw));
    std::unique_ptr<Handle> h(raw);
    RC_TRY(handle_work(h.get(), 100));
    RC_TRY(handle_work(h.get(), 1000));
    return 0;
}

// ---- a cache value: the plain struct a kernel reads, and the owners of the tables it points to
struct PlainCode { int n; const int* d_a; const float* d_b; };
static_assert(std::is_trivially_copyable_v<PlainCode>, "the plain part stays plain");
struct Code : PlainCode { DevBuf<int> a; DevBuf<float> b; };
static_assert(!std::is_copy_constructible_v<Code>, "a cache value is not copied");
int code_get(std::map<int, Code>& cache, int key, const PlainCode** out) {
    auto it = cache.find(key);
    if (it == cache.end()) {
        Code C{};
        C.n = key;
        RC_TRY(C.a.alloc(key, true, "alloc(code)"));
        C.d_a = C.a;
        RC_TRY(C.b.alloc(key, false, "alloc(code)"));
        C.d_b = C.b;
        it = cache.emplace(key, std::move(C)).first;
    }
    *out = &it->second;
    return 0;
}

}  // namespace

int main() {
    // the recorder itself: a foreign and a double free are seen (and not passed on)
    {
        int local = 0;
        dev_free(&local);
        CHECK(H.foreign_frees == 1);
        void* p = nullptr;
        CHECK(dev_alloc(&p, 8, false, "x") == 0 && H.live.size() == 1);
        dev_free(p); dev_free(p);
        CHECK(H.double_frees == 1 && H.live.empty());
        H.foreign_frees = H.double_frees = 0;
    }
    // scope, zero flag, reset
    {
        DevBuf<int> z, f;
        CHECK(!z && z.get() == nullptr);
        CHECK(z.alloc(10, true, "z") == 0 && f.alloc(10, false, "f") == 0);
        CHECK(z && H.live.size() == 2 && H.live[z.get()] == 10 * sizeof(int));
        CHECK(all_bytes(z, 10 * sizeof(int), 0) && all_bytes(f, 10 * sizeof(int), FILL));
        int* raw = z;
        CHECK(raw == z.get() && z + 1 == raw + 1 && &z[3] == raw + 3);
        z.reset(); z.reset();
        CHECK(!z && H.live.size() == 1);
        CHECK(f.alloc(4, true, "f") == 0 && H.live.size() == 1 && H.live[f.get()] == 4 * sizeof(int));      // alloc on a full owner frees first
    }
    CHECK(H.live.empty());
    // move construction, move assignment, swap
    {
        DevBuf<float> a, b;
        CHECK(a.alloc(3, false, "a") == 0 && b.alloc(5, false, "b") == 0);
        float *pa = a, *pb = b;
        DevBuf<float> c(std::move(a));
        CHECK(!a && c.get() == pa && H.live.size() == 2);
        const long frees = H.frees;
        b = std::move(c);
        CHECK(!c && b.get() == pa && H.frees == frees + 1 && H.live.size() == 1 && !H.live.count(pb));
        DevBuf<float> d;
        CHECK(d.alloc(7, false, "d") == 0);
        float* pd = d;
        std::swap(b, d);
        CHECK(b.get() == pd && d.get() == pa && H.frees == frees + 1 && H.live.size() == 2);
    }
    CHECK(H.live.empty());
    // Workspace: a quarter of slack, grows by freeing the old block, a smaller size allocates nothing
    {
        Workspace w;
        H.arm(0);
        CHECK(w.ensure(1000) == 0 && w.bytes == 1250 && H.requests == 1 && H.live[w.p] == 1250);
        void* first = w.p;
        CHECK(w.ensure(500) == 0 && w.ensure(1250) == 0 && w.p == first && H.requests == 1);
        const long frees = H.frees;
        CHECK(w.ensure(2000) == 0 && w.bytes == 2500 && H.requests == 2 && H.frees == frees + 1 && H.live.size() == 1 && !H.live.count(first));
        Workspace v(std::move(w));
        CHECK(!w.p && w.bytes == 0 && v.bytes == 2500 && H.live.size() == 1);
        w = std::move(v);
        CHECK(!v.p && w.bytes == 2500 && H.live.size() == 1);
        H.arm(1);
        CHECK(w.ensure(5000) == ERR && !w.p && w.bytes == 0 && H.live.empty() && H.last_what == "hipMalloc(workspace)");      // (the old block is gone: the contents never survive a growth)
        H.arm(0);
        CHECK(w.ensure(10) == 0 && w.bytes == 12);
        w.release(); w.release();
        CHECK(H.live.empty());
    }
    CHECK(H.live.empty());
    // the handle: the allocator fails at request k, for every k
    H.arm(0);
    CHECK(handle_life() == 0 && H.live.empty());
    const long R = H.requests;
    CHECK(R == 6 + 2 + 2);          // six members, two lazy ones, the workspace twice
    for (long k = 1; k <= R; ++k) {
        H.arm(k);
        CHECK(handle_life() == ERR);
        CHECK(H.requests == k && H.live.empty());
        CHECK(H.last_what == (k <= 6 ? "alloc(handle)" : k <= 8 ? "alloc(handle staging)" : "hipMalloc(workspace)"));
    }
    {   // a lazy member that failed is asked for again by the next call; what the call had got stays
        Handle* raw = nullptr;
        H.arm(0);
        CHECK(handle_create(3, &raw) == 0);
        std::unique_ptr<Handle> h(raw);
        H.arm(2);
        CHECK(handle_work(raw, 50) == ERR && raw->lazy_in && !raw->lazy_out);
        uint8_t* kept = raw->lazy_in;
        H.arm(0);
        CHECK(handle_work(raw, 50) == 0 && raw->lazy_in.get() == kept && raw->lazy_out && H.requests == 2);
    }
    CHECK(H.live.empty());
    // the cache: entries own their tables; erase and clear free them; a build abandoned half way leaves nothing
    {
        std::map<int, Code> cache;
        const PlainCode* c3 = nullptr;
        H.arm(0);
        for (int key : {3, 5, 9}) { const PlainCode* c; CHECK(code_get(cache, key, &c) == 0 && c->n == key); if (key == 3) c3 = c; }
        CHECK(H.live.size() == 6 && H.requests == 6);
        const PlainCode* again = nullptr;
        CHECK(code_get(cache, 3, &again) == 0 && again == c3 && H.requests == 6);
        CHECK(c3->d_a == cache.at(3).a.get() && c3->d_b == cache.at(3).b.get() && all_bytes(c3->d_a, 3 * sizeof(int), 0));
        const PlainCode by_value = *c3;         // what a launch does: the plain part alone
        CHECK(by_value.d_a == c3->d_a && H.live.size() == 6);
        for (long k = 1; k <= 2; ++k) {
            H.arm(k);
            const PlainCode* c = nullptr;
            CHECK(code_get(cache, 7, &c) == ERR && !c && !cache.count(7) && H.live.size() == 6);
        }
        cache.erase(5);
        CHECK(H.live.size() == 4);
        cache.clear();
        CHECK(H.live.empty());
        H.arm(0);
        const PlainCode* c = nullptr;
        CHECK(code_get(cache, 4, &c) == 0 && H.live.size() == 2);
    }
    CHECK(H.live.empty() && H.double_frees == 0 && H.foreign_frees == 0);
    printf("dev buf run ok: %ld frees\n", H.frees);
    return 0;
}
