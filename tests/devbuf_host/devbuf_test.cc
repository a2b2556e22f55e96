// Host-only check of the owner types in modelmesh_amd/csrc/devbuf.hpp.  The four HIP calls the header names are counting
// stand-ins over the heap: they keep the set of live pointers and abort on a double free or a free of a pointer they never gave
// out.  Exits non-zero at the first failed check.
#include <cstdio>
#include <cstdlib>
#include <set>
#include <utility>
#include <vector>

enum hipError_t { hipSuccess = 0, hipErrorOutOfMemory = 2 };

namespace fake {
std::set<void *> live_dev, live_pin;
int n_malloc = 0, n_free = 0, n_host_malloc = 0, n_host_free = 0;
bool fail_next = false;  // the next allocation fails (and writes nothing)

hipError_t alloc(std::set<void *> &live, int &count, void **p, size_t bytes)
{
    if (fail_next) {
        fail_next = false;
        return hipErrorOutOfMemory;
    }
    *p = malloc(bytes ? bytes : 1);
    if (!*p) abort();
    live.insert(*p);
    count++;
    return hipSuccess;
}
hipError_t free_of(std::set<void *> &live, int &count, void *p, const char *what)
{
    if (!live.erase(p)) {
        fprintf(stderr, "%s(%p): not a live allocation (double free, or never allocated)\n", what, p);
        abort();
    }
    free(p);
    count++;
    return hipSuccess;
}
size_t live() { return live_dev.size() + live_pin.size(); }
}  // namespace fake

hipError_t hipMalloc(void **p, size_t bytes) { return fake::alloc(fake::live_dev, fake::n_malloc, p, bytes); }
hipError_t hipFree(void *p) { return fake::free_of(fake::live_dev, fake::n_free, p, "hipFree"); }
hipError_t hipHostMalloc(void **p, size_t bytes, unsigned int) { return fake::alloc(fake::live_pin, fake::n_host_malloc, p, bytes); }
hipError_t hipHostFree(void *p) { return fake::free_of(fake::live_pin, fake::n_host_free, p, "hipHostFree"); }

#include "../../modelmesh_amd/csrc/devbuf.hpp"

#define CHECK(cond)                                                          \
    do {                                                                     \
        if (!(cond)) {                                                       \
            fprintf(stderr, "%s:%d: check failed: %s\n", __FILE__, __LINE__, #cond); \
            exit(1);                                                         \
        }                                                                    \
    } while (0)

namespace {

void test_ensure()
{
    const int m0 = fake::n_malloc, f0 = fake::n_free;
    {
        DevBuf b;
        CHECK(b.p == nullptr && b.cap == 0);
        CHECK(b.ensure(1) == hipSuccess);
        CHECK(b.p && b.cap == 256);  // at least 256 bytes, in multiples of 256
        void *p = b.p;
        CHECK(b.ensure(256) == hipSuccess && b.p == p && b.cap == 256);  // within capacity: the pointer stays
        CHECK(b.ensure(0) == hipSuccess && b.p == p);
        CHECK(fake::n_malloc == m0 + 1 && fake::n_free == f0);
        CHECK(b.ensure(257) == hipSuccess);  // beyond: one allocation freed, one made
        CHECK(b.cap == 512 && fake::n_malloc == m0 + 2 && fake::n_free == f0 + 1 && fake::live() == 1);
        CHECK(b.as<int>() == static_cast<int *>(b.p));
        fake::fail_next = true;  // growth frees first: a failed allocation leaves nothing
        CHECK(b.ensure(4096) == hipErrorOutOfMemory);
        CHECK(b.p == nullptr && b.cap == 0 && fake::live() == 0 && fake::n_free == f0 + 2);
        fake::fail_next = true;
        CHECK(b.alloc(100) == hipErrorOutOfMemory && b.p == nullptr && b.cap == 0);
        CHECK(b.alloc(100) == hipSuccess && b.cap == 100);  // alloc: exactly what was asked for
        CHECK(b.release_checked() == hipSuccess && b.p == nullptr && b.cap == 0);
        CHECK(b.release_checked() == hipSuccess);  // of an empty buffer: no call
        b.release();
        CHECK(fake::n_free == f0 + 3);
        CHECK(b.ensure(300) == hipSuccess && b.cap == 512);
    }
    CHECK(fake::live() == 0 && fake::n_malloc - m0 == fake::n_free - f0);  // the destructor freed the last one
}

void test_moves()
{
    {
        DevBuf a;
        CHECK(a.ensure(1000) == hipSuccess);
        void *pa = a.p;
        const size_t ca = a.cap;
        DevBuf b(std::move(a));  // move construction: the source is left empty
        CHECK(b.p == pa && b.cap == ca && a.p == nullptr && a.cap == 0);
        DevBuf d;
        CHECK(d.ensure(10) == hipSuccess);
        const int f0 = fake::n_free;
        d = std::move(b);  // move assignment onto a full buffer frees what it held
        CHECK(fake::n_free == f0 + 1 && fake::live() == 1);
        CHECK(d.p == pa && d.cap == ca && b.p == nullptr && b.cap == 0);
        DevBuf &alias = d;
        d = std::move(alias);  // onto itself: nothing happens
        CHECK(d.p == pa && d.cap == ca && fake::n_free == f0 + 1);
        std::swap(d, d);
        CHECK(d.p == pa && d.cap == ca && fake::n_free == f0 + 1);
        DevBuf e;
        std::swap(d, e);  // a full and an empty one
        CHECK(e.p == pa && e.cap == ca && d.p == nullptr && d.cap == 0 && fake::n_free == f0 + 1);
        std::swap(d, e);
        CHECK(d.p == pa && e.p == nullptr && fake::n_free == f0 + 1 && fake::live() == 1);
    }
    CHECK(fake::live() == 0);
}

void test_scoped()
{
    {
        DevBuf dst;
        {
            ScopedDevBuf s;
            CHECK(!s.move_into(dst) && dst.p == nullptr);  // nothing built: nothing published
            CHECK(s.b.ensure(64) == hipSuccess);
            void *ps = s.b.p;
            CHECK(s.move_into(dst));  // onto an empty destination
            CHECK(dst.p == ps && dst.cap == 256 && s.b.p == nullptr && s.b.cap == 0);
        }
        CHECK(fake::live() == 1);
        void *old = dst.p;
        const int f0 = fake::n_free;
        {
            ScopedDevBuf s;
            CHECK(s.b.ensure(1024) == hipSuccess);
            void *ps = s.b.p;
            CHECK(s.move_into(dst));  // onto a full one: it takes what it replaced ...
            CHECK(dst.p == ps && dst.cap == 1024 && s.b.p == old && s.b.cap == 256);
            CHECK(fake::n_free == f0 && fake::live() == 2);  // ... which stays allocated until the carrier ends
        }
        CHECK(fake::n_free == f0 + 1 && fake::live() == 1 && fake::live_dev.count(dst.p) == 1);
        {
            ScopedDevBuf s;  // never published: released when it ends; an explicit release before that is not a second free
            CHECK(s.b.ensure(8) == hipSuccess);
            s.release();
            CHECK(s.b.p == nullptr && fake::live() == 1);
            CHECK(s.b.ensure(8) == hipSuccess);
        }
        CHECK(fake::live() == 1);
    }
    CHECK(fake::live() == 0);
}

void test_vector()
{
    const int m0 = fake::n_malloc, f0 = fake::n_free;
    {
        std::vector<DevBuf> v;
        std::vector<void *> ptrs;
        for (int i = 0; i < 100; i++) {  // the vector reallocates several times: elements move, nothing is freed
            DevBuf b;
            CHECK(b.alloc(16 + i) == hipSuccess);
            ptrs.push_back(b.p);
            v.push_back(std::move(b));
            CHECK(b.p == nullptr);
        }
        CHECK(fake::n_free == f0 && fake::live() == 100);
        for (int i = 0; i < 100; i++) CHECK(v[i].p == ptrs[i] && v[i].cap == (size_t)(16 + i));
        v.erase(v.begin() + 10);  // the elements behind move down by assignment
        CHECK(fake::n_free == f0 + 1 && fake::live() == 99 && fake::live_dev.count(ptrs[10]) == 0);
        CHECK(v[10].p == ptrs[11] && v[98].p == ptrs[99]);
    }
    CHECK(fake::live() == 0 && fake::n_malloc - m0 == 100 && fake::n_free - f0 == 100);
}

void test_pinned()
{
    const int m0 = fake::n_host_malloc, f0 = fake::n_host_free, d0 = fake::n_malloc;
    {
        PinBuf<double> a;
        CHECK(a.p == nullptr);
        fake::fail_next = true;
        CHECK(a.alloc(8, 0) == hipErrorOutOfMemory && a.p == nullptr);
        CHECK(a.alloc(8, 0) == hipSuccess && a.p);
        a.p[7] = 1.0;  // count elements, not bytes
        double *pa = a.p;
        PinBuf<double> b(std::move(a));
        CHECK(b.p == pa && a.p == nullptr);
        PinBuf<double> d;
        CHECK(d.alloc(1, 0) == hipSuccess);
        d = std::move(b);
        CHECK(d.p == pa && b.p == nullptr && fake::n_host_free == f0 + 1 && fake::live() == 1);
        PinBuf<double> &alias = d;
        d = std::move(alias);
        std::swap(d, d);
        CHECK(d.p == pa && fake::n_host_free == f0 + 1);
        PinBuf<double> e;
        std::swap(d, e);
        CHECK(e.p == pa && d.p == nullptr && fake::n_host_free == f0 + 1);
        e.release();
        e.release();
        CHECK(e.p == nullptr && fake::n_host_free == f0 + 2 && fake::live() == 0);
        std::vector<PinBuf<int>> v;
        for (int i = 0; i < 40; i++) {
            PinBuf<int> x;
            CHECK(x.alloc(4, 0) == hipSuccess);
            v.push_back(std::move(x));
        }
        CHECK(fake::live_pin.size() == 40 && fake::n_host_free == f0 + 2);
    }
    CHECK(fake::live() == 0 && fake::n_host_malloc - m0 == fake::n_host_free - f0 && fake::n_malloc == d0);
}

// a context in small: a dozen members, some never allocated, one outgrown, retired buffers in a vector
struct Holder {
    DevBuf a, b, c, never1, d[2], never2;
    ScopedDevBuf s, never3;
    PinBuf<int> pin, never4;
    PinBuf<char> flags;
    std::vector<DevBuf> retired;
};

void test_holder()
{
    {
        Holder h;
        CHECK(h.a.ensure(10) == hipSuccess && h.b.ensure(1 << 16) == hipSuccess && h.c.alloc(12) == hipSuccess);
        CHECK(h.d[1].ensure(300) == hipSuccess && h.s.b.ensure(1) == hipSuccess);
        CHECK(h.pin.alloc(16, 0) == hipSuccess && h.flags.alloc(64, 0) == hipSuccess);
        CHECK(h.a.ensure(5000) == hipSuccess);
        h.retired.push_back(std::move(h.c));
        CHECK(h.c.alloc(24) == hipSuccess);
        h.retired.push_back(std::move(h.c));
        CHECK(fake::live_dev.size() == 6 && fake::live_pin.size() == 2);
    }
    CHECK(fake::live() == 0);
    CHECK(fake::n_malloc == fake::n_free && fake::n_host_malloc == fake::n_host_free);
}

}  // namespace

int main()
{
    test_ensure();
    test_moves();
    test_scoped();
    test_vector();
    test_pinned();
    test_holder();
    CHECK(fake::live() == 0);
    printf("devbuf_test ok: %d device and %d pinned allocations made and freed\n", fake::n_malloc, fake::n_host_malloc);
    return 0;
}
