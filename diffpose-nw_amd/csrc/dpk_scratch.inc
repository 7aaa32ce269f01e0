// dpk_scratch.inc — the device scratch of one handle: dpk_eps's per-pose timestep projections on the shipped
// shape, the activation scratch of the generic path (a handle is one or the other).  Five rules:
//   1. an uncaptured call uses the buffer of its stream: calls on different streams never share one, and
//      calls on one stream are ordered by the stream;
//   2. so a buffer grows after a sync of its stream only;
//   3. a captured call becomes a graph node that keeps its buffer's address for the graph's life and may
//      replay beside anything, so it cannot use a stream's buffer, and nothing can be allocated inside a
//      capture: the uncaptured calls keep a spare that no launch has seen;
//   4. the first captured call of a capturing stream takes the spare into the capture's list (CapRes), and the
//      later captured calls of that stream in the same capture (sequential graph nodes) share it;
//   5. when the graph is gone the buffer becomes the spare if it is the larger of the two, else it is freed.
// Capacities are in floats.  No handle and no capture bookkeeping in here, and of HIP only hipStream_t,
// hipMalloc, hipFree, hipStreamSynchronize, hipGetLastError and hipSuccess, so a CPU-only build that defines
// those over malloc compiles it too (tests/c/dpk_scratch_check.cpp).
#include <stddef.h>

#include <vector>

struct ScratchBuf {
    hipStream_t st = nullptr;   // the stream it serves (the spare: none)
    float* p = nullptr;
    size_t cap = 0;             // floats
};
struct ScratchPool {
    std::vector<ScratchBuf> bufs;   // per stream (uncaptured calls)
    ScratchBuf spare;               // for the next capture
    // called before a stream's buffer `old` is replaced (null: the stream's first), its stream synced: whoever
    // keeps things keyed by the address (the generic path's recorded loops) drops them here
    void (*replaced)(void* ctx, const float* old) = nullptr;
    void* ctx = nullptr;
};
enum ScratchStatus { SCRATCH_OK = 0, SCRATCH_NO_SPARE, SCRATCH_SHARED_TOO_SMALL };

// Keep a spare of at least n floats.  Only a later capture needs it, so a failed allocation is not the
// caller's failure: the error is cleared and the old spare stays (the new one is allocated before the old one
// is freed); a capture the spare cannot serve is refused then (SCRATCH_NO_SPARE).
static void scratch_reserve(ScratchPool& pool, size_t n) {
    if (pool.spare.cap >= n) return;
    float* p = nullptr;
    if (hipMalloc(&p, n * 4) != hipSuccess) {
        (void)hipGetLastError();
        return;
    }
    if (pool.spare.p) (void)hipFree(pool.spare.p);
    pool.spare = ScratchBuf{nullptr, p, n};
}

// An uncaptured call's n floats on `st`, the spare grown alongside.  Null when the runtime refused the sync,
// the free or the allocation (its error is left for the caller to read; the stream then has no buffer).
static float* scratch_get(ScratchPool& pool, hipStream_t st, size_t n) {
    ScratchBuf* b = nullptr;
    for (auto& x : pool.bufs)
        if (x.st == st) b = &x;
    if (!b) {
        pool.bufs.push_back(ScratchBuf{st, nullptr, 0});
        b = &pool.bufs.back();
    }
    if (b->cap < n) {
        // earlier calls on this stream may still read the old buffer
        if (hipStreamSynchronize(st) != hipSuccess) return nullptr;
        if (pool.replaced) pool.replaced(pool.ctx, b->p);
        if (b->p && hipFree(b->p) != hipSuccess) return nullptr;
        b->p = nullptr;
        b->cap = 0;
        if (hipMalloc(&b->p, n * 4) != hipSuccess) {
            b->p = nullptr;
            return nullptr;
        }
        b->cap = n;
    }
    scratch_reserve(pool, n);
    return b->p;
}

// A captured call's n floats on `st`, `held` being its capture's list.  `got`: the buffer (SCRATCH_OK), the
// one the capture's earlier calls on `st` share (too small), or the spare as it is (no spare).
static ScratchStatus scratch_get_captured(ScratchPool& pool, std::vector<ScratchBuf>& held, hipStream_t st, size_t n,
                                          ScratchBuf& got) {
    for (auto& b : held)
        if (b.st == st) {
            got = b;
            return b.cap < n ? SCRATCH_SHARED_TOO_SMALL : SCRATCH_OK;
        }
    got = pool.spare;
    if (pool.spare.cap < n) return SCRATCH_NO_SPARE;
    got.st = st;
    held.push_back(got);
    pool.spare = ScratchBuf{};
    return SCRATCH_OK;
}

// The buffers of a capture whose graph is gone (rule 5)
static void scratch_release(ScratchPool& pool, std::vector<ScratchBuf>& held) {
    for (auto& b : held) {
        if (pool.spare.p && pool.spare.cap >= b.cap) {
            (void)hipFree(b.p);
            continue;
        }
        if (pool.spare.p) (void)hipFree(pool.spare.p);
        pool.spare = ScratchBuf{nullptr, b.p, b.cap};
    }
    held.clear();
}

// Handle teardown: a live capture's list, and the pool
static void scratch_free(std::vector<ScratchBuf>& held) {
    for (auto& b : held)
        if (b.p) (void)hipFree(b.p);
    held.clear();
}
static void scratch_free_all(ScratchPool& pool) {
    scratch_free(pool.bufs);
    if (pool.spare.p) (void)hipFree(pool.spare.p);
    pool.spare = ScratchBuf{};
}
