// CPU check of the scratch pool (csrc/dpk_scratch.inc) over a fake runtime: the few HIP names the pool uses,
// defined over malloc and free, with a count of live allocations, a log of sync / hook / free events and a
// switch that fails one coming allocation.  Prints one line per case; tests/test_scratch_cpu.py builds this
// with the host sanitizers (a leak or a double free ends it with an error) and compares the lines.
// Plain C++, no HIP: clang++ -std=c++17 -fsanitize=address,undefined
#include <stdio.h>
#include <stdlib.h>

#include <map>
#include <string>

typedef struct FakeStream* hipStream_t;
enum { hipSuccess = 0, hipErrorOutOfMemory = 2 };

static int live = 0;                 // allocations not yet freed
static int fail_in = 0;              // n > 0: the n-th allocation from now fails
static int last_error = hipSuccess;
static std::string events;           // "sync:<stream>", "hook:<buffer>", "free:<buffer>", comma separated
static std::map<const void*, std::string> names;   // buffers by order of allocation: b1, b2, ...
static int allocs = 0;

static void note(const std::string& e) { events += (events.empty() ? "" : ",") + e; }
static std::string name(const void* p) { return p ? names[p] : "null"; }

static int hipMalloc(float** p, size_t bytes) {
    if (fail_in > 0 && --fail_in == 0) {
        *p = nullptr;
        return last_error = hipErrorOutOfMemory;
    }
    *p = static_cast<float*>(malloc(bytes));
    names[*p] = "b" + std::to_string(++allocs);
    ++live;
    return hipSuccess;
}
static int hipFree(float* p) {
    note("free:" + name(p));
    free(p);
    --live;
    return hipSuccess;
}
static int hipStreamSynchronize(hipStream_t s) {
    note("sync:" + std::to_string((long)(size_t)s));
    return hipSuccess;
}
static int hipGetLastError() {
    const int e = last_error;
    last_error = hipSuccess;
    return e;
}

#include "../../diffpose-nw_amd/csrc/dpk_scratch.inc"

static int hook_ctx = 0;
static void hook(void* ctx, const float* old) { note(std::string(ctx == &hook_ctx ? "hook:" : "hook?:") + name(old)); }
static const char* word(ScratchStatus s) {
    return s == SCRATCH_OK ? "ok" : s == SCRATCH_NO_SPARE ? "no-spare" : "shared-too-small";
}
static void start(ScratchPool& pool) {   // a new handle's pool; buffer names and the log start over
    pool = ScratchPool{};
    pool.replaced = hook;
    pool.ctx = &hook_ctx;
    names.clear();
    allocs = 0;
    events.clear();
}

int main() {
    const hipStream_t A = (hipStream_t)(size_t)1, B = (hipStream_t)(size_t)2;
    ScratchPool pool;
    std::vector<ScratchBuf> held;
    ScratchBuf got;

    // a: a buffer per stream; growth syncs that stream only, then the hook, then the free
    start(pool);
    float* a1 = scratch_get(pool, A, 100);   // b1, spare b2
    float* a2 = scratch_get(pool, B, 100);   // b3
    float* a3 = scratch_get(pool, A, 50);
    events.clear();
    float* a4 = scratch_get(pool, A, 200);   // b4, spare b5 (b2 freed after it)
    printf("a different=%d same=%d grown=%d events=%s\n", a1 != a2, a1 == a3, a4 && a4 != a2, events.c_str());
    scratch_free_all(pool);

    // b: a request of n leaves a spare of at least n; a smaller one leaves it alone
    start(pool);
    scratch_get(pool, A, 100);
    const float* sp = pool.spare.p;
    const size_t cap_b = pool.spare.cap;
    scratch_get(pool, A, 40);
    scratch_get(pool, B, 40);
    printf("b spare_cap=%zu spare_same=%d\n", cap_b, sp && pool.spare.p == sp && pool.spare.cap == cap_b);
    scratch_free_all(pool);

    // c: a capture's first call on a stream takes the spare; the stream's later calls share it
    start(pool);
    scratch_get(pool, A, 100);
    sp = pool.spare.p;
    const ScratchStatus c1 = scratch_get_captured(pool, held, A, 100, got);
    const int took = got.p == sp && got.st == A && !pool.spare.p;
    const size_t cap_c = pool.spare.cap;
    const ScratchStatus c2 = scratch_get_captured(pool, held, A, 60, got);
    const int same = got.p == sp;
    const ScratchStatus c3 = scratch_get_captured(pool, held, A, 150, got);
    const size_t short3 = got.cap;
    const ScratchStatus c4 = scratch_get_captured(pool, held, B, 10, got);
    printf("c first=%s took_spare=%d spare_cap=%zu second=%s same=%d larger=%s(%zu) other_stream=%s(%zu) held=%zu\n",
           word(c1), took, cap_c, word(c2), same, word(c3), short3, word(c4), got.cap, held.size());

    // d: release.  The pool of (c): A's buffer and the capture's 100 floats live, no spare.
    scratch_reserve(pool, 50);
    const int d0 = live;                     // 3
    scratch_release(pool, held);             // 100 > 50: the capture's buffer is the spare now, the old one freed
    const int d1 = live, larger = pool.spare.p == sp && pool.spare.cap == 100 && held.empty();
    scratch_get_captured(pool, held, A, 100, got);
    scratch_reserve(pool, 200);
    const float* sp200 = pool.spare.p;
    const int d2 = live;                     // 3
    scratch_release(pool, held);             // 100 < 200: freed
    printf("d live=%d larger_becomes_spare=%d live=%d live=%d smaller_freed=%d live=%d\n", d0, larger, d1, d2,
           pool.spare.p == sp200 && pool.spare.cap == 200, live);
    scratch_free_all(pool);

    // e: the spare's allocation fails: the call is served, the old spare stays and serves a capture
    start(pool);
    scratch_get(pool, A, 100);
    sp = pool.spare.p;
    fail_in = 2;                             // the stream's new buffer, then the spare's
    float* e1 = scratch_get(pool, A, 200);
    const int kept = pool.spare.p == sp && pool.spare.cap == 100, cleared = hipGetLastError() == hipSuccess;
    const ScratchStatus e2 = scratch_get_captured(pool, held, A, 100, got);
    printf("e request=%s spare_kept=%d error_cleared=%d captured=%s from_old_spare=%d\n", e1 ? "ok" : "failed", kept,
           cleared, word(e2), got.p == sp);
    // ... and the stream's own allocation failing: the call fails, its error left for the caller
    fail_in = 1;
    float* e3 = scratch_get(pool, A, 400);
    printf("e2 request=%s error=%d stream_cap=%zu\n", e3 ? "ok" : "failed", hipGetLastError(), pool.bufs[0].cap);

    // f: free everything, one capture's list still held
    scratch_get(pool, A, 100);
    scratch_get(pool, B, 100);
    scratch_free_all(pool);
    const int f1 = live;
    scratch_free(held);
    printf("f after_pool=%d after_held=%d\n", f1, live);
    return live == 0 ? 0 : 1;
}
