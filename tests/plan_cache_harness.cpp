// tests/plan_cache_harness.cpp -- the container of parked analysis plans (ilupp_amd/csrc/plan_cache.h) on the CPU: blocks are heap
// allocations, the release callback frees them and counts, built with -fsanitize=address,undefined by tests/test_plan_cache_host.py.
// Exit code 0 = every check held; a block released twice, touched after its release or never released shows in the counts below and
// aborts under the sanitizers (a leak fails LeakSanitizer at exit).
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <atomic>
#include <map>
#include <mutex>
#include <thread>
#include <vector>

#include "plan_cache.h"

using namespace ilupp;

static std::mutex g_mu;
static std::map<void *, long> g_serial;       // live block -> the serial number of its allocation (the heap hands addresses out again)
static std::map<long, int> g_released;        // serial number -> times released
static long g_next = 0;
static std::atomic<long> g_live(0);

struct H { void *p; long id; };

static H block(size_t bytes)
{
    void *p = malloc(bytes);
    memset(p, 0x5a, bytes);
    ++g_live;
    std::lock_guard<std::mutex> lk(g_mu);
    const long id = ++g_next;
    g_serial[p] = id; g_released[id] = 0;
    return H{p, id};
}
static void release(void *p)
{
    {
        std::lock_guard<std::mutex> lk(g_mu);
        auto it = g_serial.find(p);
        if (it == g_serial.end()) { fprintf(stderr, "plan_cache_harness: release of %p, which is no live block\n", p); abort(); }
        ++g_released[it->second];
        g_serial.erase(it);
    }
    memset(p, 0, 1);
    free(p);
    --g_live;
}
static int times_released(const H &h)
{
    std::lock_guard<std::mutex> lk(g_mu);
    return g_released[h.id];
}

struct Payload { int tag = 0; std::vector<int> sizes; };
typedef PlanCache<Payload> Cache;

static PlanKey key(int dev, int32_t n, int64_t nnz, int32_t nx, int32_t ny, int32_t nz)
{
    PlanKey k;
    k.device = dev; k.n = n; k.nnz = nnz; k.nx = nx; k.ny = ny; k.nz = nz;
    return k;
}
// a plan of `nblocks` blocks of `each` bytes; the handles are appended to *handles
static Cache::Plan make(const PlanKey &k, int tag, int nblocks, size_t each, std::vector<H> *handles)
{
    Cache::Plan p;
    p.key = k; p.payload.tag = tag;
    for (int i = 0; i < nblocks; ++i) {
        const H h = block(each);
        p.blocks.push_back(PlanBlock{h.p, each});
        p.payload.sizes.push_back((int)each);
        if (handles) handles->push_back(h);
    }
    return p;
}
static void release_plan(Cache::Plan *p) { for (const PlanBlock &b : p->blocks) release(b.handle); p->blocks.clear(); }

#define CHECK(c) do { if (!(c)) { fprintf(stderr, "plan_cache_harness: check failed at line %d: %s\n", __LINE__, #c); return 1; } } while (0)

int main()
{
    const size_t big = (size_t)1 << 30;
    {
        // key equality: every field tells two plans apart
        const PlanKey a = key(0, 98304, 674816, 32, 64, 48);
        CHECK(a == key(0, 98304, 674816, 32, 64, 48));
        CHECK(!(a == key(1, 98304, 674816, 32, 64, 48)) && !(a == key(0, 98305, 674816, 32, 64, 48)) && !(a == key(0, 98304, 674817, 32, 64, 48)));
        CHECK(!(a == key(0, 98304, 674816, 64, 32, 48)) && !(a == key(0, 98304, 674816, 32, 48, 64)) && !(a == key(0, 98304, 674816, 32, 64, 49)));
    }
    {
        // park, take removes, a second take misses; the payload and the blocks come back as they went in
        Cache C(release, 2);
        std::vector<H> h;
        const PlanKey a = key(0, 100, 600, 4, 5, 5), b = key(0, 100, 600, 5, 4, 5);
        CHECK(C.park(make(a, 11, 3, 64, &h), big));
        CHECK(C.plans() == 1 && C.blocks() == 3 && C.bytes() == 192);
        Cache::Plan got;
        CHECK(!C.take(b, &got));                                   // (equal n and nnz, other dimensions)
        CHECK(C.take(a, &got));
        CHECK(got.payload.tag == 11 && got.blocks.size() == 3 && got.payload.sizes.size() == 3 && got.key == a);
        for (int i = 0; i < 3; ++i) CHECK(got.blocks[(size_t)i].handle == h[(size_t)i].p && times_released(h[(size_t)i]) == 0);
        CHECK(C.plans() == 0 && C.blocks() == 0 && C.bytes() == 0);
        CHECK(!C.take(a, &got));
        const Cache::Stats s = C.stats();
        CHECK(s.parked == 0 && s.taken == 1 && s.missed == 2 && s.dropped == 0);
        release_plan(&got);                                        // (the taker owns them)
        for (const H &p : h) CHECK(times_released(p) == 1);
        C.note_dropped();
        CHECK(C.stats().dropped == 1);
    }
    {
        // capacity per device, the least recently parked leaves first, every block of it released exactly once; a key parked twice
        // keeps the parked plan (now the most recent) and releases the newcomer
        Cache C(release, 2);
        std::vector<H> h1, h2, h3, h2b, hd;
        const PlanKey k1 = key(0, 1, 1, 1, 1, 1), k2 = key(0, 2, 2, 2, 1, 1), k3 = key(0, 3, 3, 3, 1, 1), kd = key(1, 1, 1, 1, 1, 1);
        CHECK(C.park(make(k1, 1, 4, 32, &h1), big) && C.park(make(k2, 2, 4, 32, &h2), big));
        CHECK(C.park(make(kd, 9, 2, 32, &hd), big));               // (another device: its own capacity)
        CHECK(C.plans() == 3);
        CHECK(!C.park(make(k1, 7, 4, 32, &h2b), big));             // k1 again: refused, and k1 is the most recent of device 0 now
        for (const H &p : h2b) CHECK(times_released(p) == 1);
        CHECK(C.plans() == 3 && C.stats().dropped == 0);
        CHECK(C.park(make(k3, 3, 4, 32, &h3), big));               // over the capacity of device 0: k2 leaves
        CHECK(C.plans() == 3 && C.blocks() == 10);
        for (const H &p : h2) CHECK(times_released(p) == 1);
        for (const H &p : h1) CHECK(times_released(p) == 0);
        for (const H &p : hd) CHECK(times_released(p) == 0);
        CHECK(C.stats().dropped == 1);
        Cache::Plan got;
        CHECK(!C.take(k2, &got) && C.take(k1, &got) && got.payload.tag == 1);
        release_plan(&got);
        // drop-all: everything that is left, once
        C.drop_all();
        CHECK(C.plans() == 0 && C.bytes() == 0 && C.blocks() == 0);
        for (const H &p : h3) CHECK(times_released(p) == 1);
        for (const H &p : hd) CHECK(times_released(p) == 1);
        CHECK(C.stats().dropped == 3);
    }
    {
        // the byte limit: a plan that does not fit beside what is parked is refused and released, nothing is evicted for it; a lower
        // limit (shrink_to) drops the least recently parked until the rest fits; room 0 parks nothing
        Cache C(release, 4);
        std::vector<H> ha, hb, hc, hz;
        const PlanKey a = key(0, 1, 1, 1, 1, 1), b = key(0, 2, 2, 2, 1, 1), c = key(0, 3, 3, 3, 1, 1);
        CHECK(C.park(make(a, 1, 2, 100, &ha), 500) && C.park(make(b, 2, 2, 100, &hb), 500));
        CHECK(!C.park(make(c, 3, 2, 100, &hc), 500));              // 400 parked + 200 > 500
        for (const H &p : hc) CHECK(times_released(p) == 1);
        CHECK(C.plans() == 2 && C.bytes() == 400);
        CHECK(!C.park(make(c, 3, 1, 8, &hz), 0));
        for (const H &p : hz) CHECK(times_released(p) == 1);
        C.shrink_to(400);
        CHECK(C.plans() == 2);
        C.shrink_to(399);
        CHECK(C.plans() == 1 && C.bytes() == 200);
        for (const H &p : ha) CHECK(times_released(p) == 1);
        for (const H &p : hb) CHECK(times_released(p) == 0);
        C.shrink_to(0);
        CHECK(C.plans() == 0);
        for (const H &p : hb) CHECK(times_released(p) == 1);
    }
    {
        // two threads park and take the same few keys: every plan is released by exactly one party (the cache or the taker), the
        // counts add up, nothing is left behind (the destructor drops what is parked at the end)
        const long before = g_live.load();
        std::atomic<long> parked(0), refused(0), took(0);
        {
            Cache C(release, 3);
            auto worker = [&](int id) {
                for (int r = 0; r < 2000; ++r) {
                    const PlanKey k = key(0, (r + id) % 5, 7, 1, 1, 1);
                    if ((r + id) % 3 != 0) {
                        if (C.park(make(k, r, 3, 48, nullptr), 3 * 48 * 3)) ++parked; else ++refused;
                    } else {
                        Cache::Plan got;
                        if (C.take(k, &got)) { ++took; release_plan(&got); }
                    }
                }
            };
            std::thread t1(worker, 0), t2(worker, 1);
            t1.join(); t2.join();
            const Cache::Stats s = C.stats();
            CHECK((long)s.taken == took.load());
            CHECK((long)(s.parked + s.taken + s.dropped) == parked.load());
            CHECK(C.blocks() == 3 * C.plans() && C.bytes() == 48 * C.blocks() && C.plans() <= 3);
            CHECK(g_live.load() - before == (long)C.blocks());
        }
        CHECK(g_live.load() == before);
    }
    CHECK(g_live.load() == 0);
    for (const auto &e : g_released) CHECK(e.second == 1);         // every block ever made: released once, by the cache or by its taker
    printf("plan_cache_harness: ok\n");
    return 0;
}
