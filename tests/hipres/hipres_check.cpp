// tests/hipres — TEST INFRASTRUCTURE ONLY: the owners of rtlsdrdiags_amd/csrc/iqd_hipres.h on the host, with a counting fake
// in place of the HIP release functions and malloc in place of the allocators.  No HIP call is made and no HIP library is
// linked; tests/test_hipres.py builds this with AddressSanitizer + UBSan, so a double release or a leak fails the run too.
#include <stdio.h>
#include <stdlib.h>

#include <utility>
#include <vector>

#include "iqd_hipres.h"

using namespace iqd;

static int failures = 0;
#define CHECK(cond)                                                        \
    do {                                                                   \
        if (!(cond)) {                                                     \
            printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);       \
            failures++;                                                    \
        }                                                                  \
    } while (0)

static std::vector<int> released;
static void fake_release(int h) { released.push_back(h); }
using Fake = Owned<int, fake_release>;
static Fake fake(int h)   // an owner of handle h, filled the way the create calls fill one
{
    Fake f;
    *f.put() = h;
    return f;
}

static std::vector<size_t> asked;   // what the growable buffer and the array asked their allocator for
struct FakeAlloc {
    static hipError_t alloc(void **p, size_t bytes)
    {
        asked.push_back(bytes);
        *p = malloc(bytes ? bytes : 1);
        return *p ? hipSuccess : hipErrorOutOfMemory;
    }
    static void release(void *p) { free(p); }
};
struct FailingAlloc {
    static hipError_t alloc(void **p, size_t)
    {
        *p = nullptr;
        return hipErrorOutOfMemory;
    }
    static void release(void *) { failures++; }   // nothing was allocated: nothing to release
};

static void owner_core()
{
    released.clear();
    {
        Fake a = fake(7);
        CHECK(a.get() == 7 && (int)a == 7);
    }
    CHECK(released == std::vector<int>{7});               // destruction releases once

    released.clear();
    {
        Fake a = fake(3);
        Fake b(std::move(a));
        CHECK(a.get() == 0 && b.get() == 3);              // empty after a move
    }
    CHECK(released == std::vector<int>{3});               // the moved-from owner released nothing

    released.clear();
    {
        Fake a = fake(1), b = fake(2);
        a = std::move(b);
        CHECK(released == std::vector<int>{1});           // move-assignment releases the old handle first
        CHECK(a.get() == 2 && b.get() == 0);
        Fake &self = a;
        a = std::move(self);
        CHECK(a.get() == 2 && released.size() == 1);
    }
    CHECK((released == std::vector<int>{1, 2}));

    released.clear();
    {
        Fake a;
        a.reset();                                        // reset() on an empty owner does nothing
        CHECK(released.empty());
        *a.put() = 5;
        a.reset();
        a.reset();
        CHECK(released == std::vector<int>{5});
        *a.put() = 6;
        *a.put() = 8;                                     // put() releases what the owner held
        CHECK((released == std::vector<int>{5, 6}));
    }
    CHECK((released == std::vector<int>{5, 6, 8}));

    released.clear();
    {
        std::vector<std::pair<Fake, Fake>> pool;          // as the engine keeps its profiling event pairs
        pool.emplace_back(fake(11), fake(12));
        pool.emplace_back(fake(13), fake(14));
        std::pair<Fake, Fake> taken = std::move(pool.back());
        pool.pop_back();
        CHECK(released.empty());
        pool.push_back(std::move(taken));
        CHECK(released.empty());
    }
    CHECK(released.size() == 4);
}

// the sizes the buffers of the parent commit allocated: DevBuf::ensure of the engine, Buf::ensure of the channelizer
static size_t engine_want(size_t bytes) { return bytes + bytes / 8 + 256; }
static size_t channelizer_want(size_t bytes) { return bytes; }

template <size_t (*Want)(size_t)>
static void growth(size_t (*parent_want)(size_t))
{
    const size_t requests[] = {1, 256, 257, 1000, (size_t)1 << 20, ((size_t)1 << 20) + 1, (size_t)3 << 20};
    GrowBuf<FakeAlloc, Want> b;
    asked.clear();
    size_t cap = 0, n_alloc = 0;
    for (size_t r : requests) {
        const void *before = b.p.get();
        CHECK(b.ensure(r) == hipSuccess);
        if (r <= cap) {
            CHECK(b.p.get() == before);                   // no more than the capacity: the pointer stays
        } else {
            cap = parent_want(r);
            n_alloc++;
            CHECK(asked.size() == n_alloc && asked.back() == cap);
        }
        CHECK(asked.size() == n_alloc && b.cap == cap && b.p.get() != nullptr);
        CHECK(b.template as<char>() == (char *)b.p.get());
    }
    const void *before = b.p.get();
    CHECK(b.ensure(cap) == hipSuccess && b.ensure(0) == hipSuccess && b.p.get() == before && asked.size() == n_alloc);
    for (size_t r : requests) {                           // each request on a buffer of its own
        GrowBuf<FakeAlloc, Want> one;
        asked.clear();
        CHECK(one.ensure(r) == hipSuccess && asked == std::vector<size_t>{parent_want(r)} && one.cap == parent_want(r));
    }
}

static void arrays()
{
    asked.clear();
    Array<unsigned, FakeAlloc> a;
    CHECK(a.n == 0 && !a);
    CHECK(a.alloc(10) == hipSuccess && a.n == 10 && asked == std::vector<size_t>{10 * sizeof(unsigned)});
    unsigned *p = a;
    p[9] = 1;
    CHECK(a[9] == 1 && a + 9 == p + 9);
    CHECK(a.alloc(20) == hipSuccess && a.n == 20 && asked.back() == 20 * sizeof(unsigned));   // (the old block was released: ASan)

    GrowBuf<FailingAlloc, grow_exact> f;
    CHECK(f.ensure(16) == hipErrorOutOfMemory && f.cap == 0 && f.p.get() == nullptr);
    Array<char, FailingAlloc> g;
    CHECK(g.alloc(16) == hipErrorOutOfMemory && g.n == 0 && !g);
}

int main()
{
    owner_core();
    growth<grow_headroom>(engine_want);
    growth<grow_exact>(channelizer_want);
    arrays();
    if (failures) {
        printf("%d checks failed\n", failures);
        return 1;
    }
    printf("hipres ok\n");
    return 0;
}
