// owned_check.cpp -- the owning types of gpusimilarity_amd/csrc/capi_owned.h against a counting allocator: this file is the
// HIP runtime (the few entry points the header calls, defined below; nothing links libamdhip64).  Every allocation is
// tracked; a free of something that is not live, a leak at the end, or a failed expectation ends the run with a
// message and a non-zero status.  tests/test_owned_host.py builds and runs it.
#include "../../gpusimilarity_amd/csrc/capi_owned.h"

#include <cstdio>
#include <cstdlib>
#include <map>

namespace
{
struct Counter {
    explicit Counter(const char* w) : what(w) {}
    const char* what;
    std::map<void*, int> live; // block -> times freed (0 while live)
    long made = 0, freed = 0, calls = 0;
    long fail_at = 0; // the fail_at-th call from now fails (0: none)
    void* make()
    {
        calls++;
        if (fail_at && --fail_at == 0) return nullptr;
        void* p = std::malloc(16);
        live[p] = 0;
        made++;
        return p;
    }
    void release(void* p)
    {
        calls++;
        auto it = live.find(p);
        if (it == live.end() || it->second != 0) {
            std::printf("FAIL: %s %p freed %s\n", what, p, it == live.end() ? "but never made" : "twice");
            std::exit(1);
        }
        it->second = 1;
        freed++;
    }
    long outstanding() const { return made - freed; }
};
Counter g_dev("device block"), g_host("pinned block"), g_event("event"), g_stream("stream");
unsigned g_last_host_flags = 0;
long g_last_error_reads = 0;
} // namespace

extern "C" {
hipError_t hipMalloc(void** p, size_t bytes)
{
    if (bytes == 0) {
        std::printf("FAIL: hipMalloc of 0 bytes\n");
        std::exit(1);
    }
    *p = g_dev.make();
    return *p ? hipSuccess : hipErrorOutOfMemory;
}
hipError_t hipFree(void* p)
{
    g_dev.release(p);
    return hipSuccess;
}
hipError_t hipHostMalloc(void** p, size_t bytes, unsigned flags)
{
    if (bytes == 0) {
        std::printf("FAIL: hipHostMalloc of 0 bytes\n");
        std::exit(1);
    }
    g_last_host_flags = flags;
    *p = g_host.make();
    return *p ? hipSuccess : hipErrorOutOfMemory;
}
hipError_t hipHostFree(void* p)
{
    g_host.release(p);
    return hipSuccess;
}
hipError_t hipEventCreateWithFlags(hipEvent_t* e, unsigned)
{
    *e = static_cast<hipEvent_t>(g_event.make());
    return *e ? hipSuccess : hipErrorOutOfMemory;
}
hipError_t hipEventDestroy(hipEvent_t e)
{
    g_event.release(e);
    return hipSuccess;
}
hipError_t hipStreamCreateWithFlags(hipStream_t* s, unsigned)
{
    *s = static_cast<hipStream_t>(g_stream.make());
    return *s ? hipSuccess : hipErrorOutOfMemory;
}
hipError_t hipStreamDestroy(hipStream_t s)
{
    g_stream.release(s);
    return hipSuccess;
}
hipError_t hipEventElapsedTime(float* ms, hipEvent_t, hipEvent_t)
{
    *ms = 1.5f;
    return hipSuccess;
}
hipError_t hipGetLastError(void)
{
    g_last_error_reads++;
    return hipSuccess;
}
}

#define CHECK(cond)                                                          \
    do {                                                                     \
        if (!(cond)) {                                                       \
            std::printf("FAIL: %s:%d: %s\n", __FILE__, __LINE__, #cond);     \
            std::exit(1);                                                    \
        }                                                                    \
    } while (0)

using namespace gsim_host;

// grow / grow_keep of one buffer type; C is its allocator's counter
template <class Buf> void check_buffer(Buf&& buf, Counter& C)
{
    const long base = C.outstanding();
    bool fresh = true;
    CHECK(!buf && buf.bytes() == 0);
    CHECK(buf.grow(100, &fresh) == hipSuccess && fresh && buf && buf.bytes() == 100 && C.outstanding() == base + 1);
    // a size already held: no allocator call, by either operation
    long calls = C.calls;
    CHECK(buf.grow(100, &fresh) == hipSuccess && !fresh && buf.grow(7) == hipSuccess && buf.grow_keep(100, &fresh) == hipSuccess && !fresh);
    CHECK(C.calls == calls && buf.bytes() == 100);
    // a successful grow: the old block freed exactly once (release() ends the run on a second free), the new size reported
    uint32_t* old = buf;
    long freed = C.freed;
    CHECK(buf.grow(200, &fresh) == hipSuccess && fresh && buf.bytes() == 200 && C.freed == freed + 1 && C.live[old] == 1 && C.outstanding() == base + 1);
    old = buf;
    freed = C.freed;
    CHECK(buf.grow_keep(300, &fresh) == hipSuccess && fresh && buf.bytes() == 300 && C.freed == freed + 1 && C.live[old] == 1 && C.outstanding() == base + 1);
    // a failed allocate-then-swap grow: pointer and size as they were
    old = buf;
    C.fail_at = 1;
    long reads = g_last_error_reads;
    CHECK(buf.grow_keep(400, &fresh) == hipErrorOutOfMemory && !fresh && buf == old && buf.bytes() == 300 && C.live[old] == 0 && C.outstanding() == base + 1);
    CHECK(g_last_error_reads == reads + 1); // (the sticky error is taken: the caller has the code)
    // a failed free-first grow: empty, size 0, nothing of it outstanding
    C.fail_at = 1;
    CHECK(buf.grow(400, &fresh) == hipErrorOutOfMemory && !fresh && !buf && buf.bytes() == 0 && C.outstanding() == base);
    // ... and the next, smaller request is served, not waved through on a stale capacity
    CHECK(buf.grow(50, &fresh) == hipSuccess && fresh && buf && buf.bytes() == 50 && C.outstanding() == base + 1);
    // a request of 0 bytes still yields a block (the allocator above refuses a 0-byte call)
    buf.reset();
    CHECK(!buf && buf.bytes() == 0 && C.outstanding() == base);
    CHECK(buf.grow(0, &fresh) == hipSuccess && fresh && buf && C.outstanding() == base + 1);
    calls = C.calls;
    CHECK(buf.grow(0) == hipSuccess && C.calls == calls);
    // moves: the source is empty and frees nothing, the target's old block goes exactly once
    old = buf;
    Buf other(std::move(buf));
    CHECK(!buf && buf.bytes() == 0 && other == old && C.outstanding() == base + 1);
    CHECK(buf.grow(10) == hipSuccess && C.outstanding() == base + 2);
    uint32_t* mine = buf;
    buf = std::move(other);
    CHECK(buf == old && !other && other.bytes() == 0 && C.live[mine] == 1 && C.outstanding() == base + 1);
    {
        Buf scoped;
        CHECK(scoped.grow(10) == hipSuccess && C.outstanding() == base + 2);
    } // (its destructor frees)
    CHECK(C.outstanding() == base + 1);
    buf.reset();
    CHECK(C.outstanding() == base);
}

// The shapes of the grow sites the types replace (capi_query.cpp, capi_batch.cpp, capi_folded.cpp), each with the allocation
// failure that used to leave them inconsistent.  Every scenario ends in: the buffer serves the request or reports less.
void check_scenarios()
{
    { // a result block: grow, a failing grow, then a smaller request (ensure_result_capacity, the h_bresult / d_bresult pair)
        DevBuf<> d;
        HostBuf<unsigned char> h(3u);
        CHECK(d.grow(1000) == hipSuccess && h.grow(1000) == hipSuccess && g_last_host_flags == 3u);
        g_dev.fail_at = 1;
        CHECK(d.grow(5000) != hipSuccess);
        CHECK(d.bytes() < 500 && !d);                               // "enough capacity" cannot be read off it ...
        CHECK(d.grow(500) == hipSuccess && d && d.bytes() >= 500);  // ... and the smaller k gets a block
        g_host.fail_at = 1;
        CHECK(h.grow(5000) != hipSuccess && !h && h.bytes() == 0);
        CHECK(h.grow(500) == hipSuccess && h && h.bytes() >= 500 && g_last_host_flags == 3u);
    }
    { // three buffers released, then allocated anew, beside a capacity counter (grow_batch_segments): the second allocation fails
        DevBuf<unsigned long long> cand;
        DevBuf<uint32_t> cb, q;
        uint32_t seg_cap = 0;
        auto first_use = [&](uint32_t cap) {
            if (cand.grow(cap * 8) != hipSuccess || cb.grow(cap * 4) != hipSuccess || q.grow(cap * 4) != hipSuccess) return false;
            seg_cap = cap;
            return true;
        };
        CHECK(first_use(16) && seg_cap == 16);
        cand.reset(), cb.reset(), q.reset();
        seg_cap = 0;
        g_dev.fail_at = 2;
        CHECK(!first_use(64) && seg_cap == 0); // (no live capacity beside an empty buffer)
        const long before = g_dev.outstanding();
        CHECK(first_use(16) && seg_cap == 16 && cand && cb && q && cand.bytes() >= 16 * 8 && cb.bytes() >= 16 * 4);
        CHECK(g_dev.outstanding() == before + 2); // (what the failed attempt had allocated is kept and counted, not allocated over)
    }
    { // many allocations behind one first-use guard (ensure_batch_buffers, ensure_classic_scratch, the folded re-score buffers): one
      // in the middle fails, the retry allocates the rest and leaks nothing
        DevBuf<uint32_t> b[6];
        bool ready = false;
        auto ensure = [&]() {
            if (ready) return true;
            for (auto& x : b)
                if (x.grow(64) != hipSuccess) return false;
            return ready = true;
        };
        g_dev.fail_at = 4;
        const long base = g_dev.outstanding();
        CHECK(!ensure() && g_dev.outstanding() == base + 3);
        CHECK(ensure() && g_dev.outstanding() == base + 6);
        for (auto& x : b) CHECK(x && x.bytes() == 64);
    }
    { // allocate-then-swap beside a geometry counter (the pair buffer, the row-set scratch): the failure changes nothing
        DevBuf<unsigned long long> keys;
        DevBuf<float> vals;
        uint64_t cap = 0;
        auto grow_to = [&](uint64_t n) {
            if (keys.grow_keep(n * 8) != hipSuccess || vals.grow_keep(n * 4) != hipSuccess) return false;
            cap = n;
            return true;
        };
        CHECK(grow_to(100));
        unsigned long long* k0 = keys;
        float* v0 = vals;
        g_dev.fail_at = 1;
        CHECK(!grow_to(1000) && cap == 100 && keys == k0 && vals == v0 && keys.bytes() == 800 && vals.bytes() == 400);
        g_dev.fail_at = 2; // (the second of the pair: the first is larger now, which the kernels never see -- they are given cap)
        CHECK(!grow_to(1000) && cap == 100 && vals == v0 && keys.bytes() >= cap * 8 && vals.bytes() >= cap * 4);
        CHECK(grow_to(1000) && cap == 1000 && keys.bytes() == 8000 && vals.bytes() == 4000);
    }
    { // two ensure functions share one buffer and its capacity counter (d_final / final_cap: ensure_classic_scratch grows it and a
      // second buffer, ensure_publish_scratch guards on the pointer): the second allocation of the first one fails
        DevBuf<unsigned long long> fin;
        DevBuf<uint32_t> fin_cb;
        uint32_t cap = 0;
        bool ready = false;
        auto ensure_small = [&]() { // (the pointer guard)
            if (fin) return true;
            if (fin.grow(16 * 8) != hipSuccess) return false;
            cap = 16;
            return true;
        };
        auto ensure_large = [&]() {
            if (ready) return true;
            if (fin.bytes() < 64 * 8) cap = 0; // (free-first below: no capacity beside an empty buffer should it fail)
            if (fin.grow(64 * 8) != hipSuccess) return false;
            cap = 64; // (with the buffer it counts, not behind the second one)
            if (fin_cb.grow(64 * 4) != hipSuccess) return false;
            return ready = true;
        };
        auto consistent = [&]() { return fin ? cap > 0 && fin.bytes() >= cap * 8u : cap == 0; };
        CHECK(ensure_small() && cap == 16 && consistent());
        g_dev.fail_at = 2;
        CHECK(!ensure_large() && consistent() && fin && cap == 64); // (the shared buffer stands: its capacity is live)
        CHECK(ensure_small() && consistent() && cap == 64);         // (the pointer guard passes: the capacity it passes on is the buffer's)
        g_dev.fail_at = 1;
        fin.reset(), cap = 0, ready = false;
        CHECK(ensure_small() == false && consistent());
        g_dev.fail_at = 1;
        CHECK(!ensure_large() && !fin && consistent());              // (the first allocation fails: empty, capacity 0)
        CHECK(ensure_small() && cap == 16 && ensure_large() && cap == 64 && fin_cb && consistent());
    }
}

void check_handles()
{
    {
        Event e;
        CHECK(!e && e.create(hipEventDisableTiming) == hipSuccess && e && g_event.outstanding() == 1);
        const long calls = g_event.calls;
        CHECK(e.create() == hipSuccess && g_event.calls == calls); // (made on first use only)
        hipEvent_t raw = e;
        Event f(std::move(e));
        CHECK(!e && f == raw && g_event.outstanding() == 1);
        e = std::move(f);
        CHECK(e == raw && !f && g_event.outstanding() == 1);
        Event g;
        CHECK(g.create() == hipSuccess && g_event.outstanding() == 2);
        g = std::move(e); // (g's own event is destroyed, once)
        CHECK(g == raw && g_event.outstanding() == 1);
        g_event.fail_at = 1;
        CHECK(e.create() != hipSuccess && !e);
        EventPair p;
        CHECK(p.create() == hipSuccess && g_event.outstanding() == 3 && p.ms() == 1.5);
        EventPair half;
        g_event.fail_at = 2;
        CHECK(half.create() != hipSuccess && g_event.outstanding() == 4); // (its first event is destroyed with it)
        Stream s;
        CHECK(s.create(hipStreamNonBlocking) == hipSuccess && s && g_stream.outstanding() == 1);
        Stream t(std::move(s));
        CHECK(!s && t && g_stream.outstanding() == 1);
    }
    CHECK(g_event.outstanding() == 0 && g_stream.outstanding() == 0);
}

int main()
{
    check_buffer(DevBuf<uint32_t>(), g_dev);
    check_buffer(HostBuf<uint32_t>(2u), g_host);
    check_scenarios();
    check_handles();
    // every allocation freed, and (release() checks it on the way) none of them twice
    for (const Counter* c : {&g_dev, &g_host, &g_event, &g_stream}) {
        CHECK(c->made > 0 && c->outstanding() == 0);
        for (const auto& kv : c->live) CHECK(kv.second == 1);
    }
    std::printf("ok %ld device %ld pinned %ld events %ld streams\n", g_dev.made, g_host.made, g_event.made, g_stream.made);
    return 0;
}
