// Stand-alone check of csrc/dev_buf.hpp (tests/test_dev_buf_host.py builds and runs it).  It links nothing of the engine:
// hip_check is this file's own and counts its calls, one per allocation or copy the buffer attempts.  Every check holds
// whichever way an allocation goes, so the program passes with and without a device.
#include "dev_buf.hpp"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <dlfcn.h>
#include <type_traits>

static int g_calls = 0, g_failed = 0, g_checks = 0;

// The program's own hipMalloc / hipFree / hipMemcpy stand in front of the runtime's.  Normally they pass on to it; while
// g_fake is set they serve host memory instead, and the g_fail_at-th allocation from then on (1-based) fails: the one way to
// see a group of buffers through "the first allocation succeeds, a later one fails" without a device.
static bool g_fake = false;
static int g_fake_allocs = 0, g_fail_at = 0;
template <typename F>
static F next_symbol(const char *name) { return reinterpret_cast<F>(dlsym(RTLD_NEXT, name)); }
extern "C" hipError_t hipMalloc(void **p, size_t bytes) {
    if (!g_fake) return next_symbol<hipError_t (*)(void **, size_t)>("hipMalloc")(p, bytes);
    if (++g_fake_allocs == g_fail_at) { *p = nullptr; return hipErrorOutOfMemory; }
    *p = std::malloc(bytes);
    return hipSuccess;
}
extern "C" hipError_t hipFree(void *p) {
    if (!g_fake) return next_symbol<hipError_t (*)(void *)>("hipFree")(p);
    std::free(p);
    return hipSuccess;
}
extern "C" hipError_t hipMemcpy(void *dst, const void *src, size_t bytes, hipMemcpyKind kind) {
    if (!g_fake) return next_symbol<hipError_t (*)(void *, const void *, size_t, hipMemcpyKind)>("hipMemcpy")(dst, src, bytes, kind);
    std::memcpy(dst, src, bytes);
    return hipSuccess;
}

namespace kge {
int hip_check(hipError_t e, const char *) {
    g_calls++;
    if (e == hipSuccess) return 0;
    (void)hipGetLastError();
    return 1000 + (int)e;
}
}  // namespace kge

#define CHECK(cond) do { g_checks++; if (!(cond)) { g_failed++; std::printf("FAILED line %d: %s\n", __LINE__, #cond); } } while (0)

// the state a call may leave behind: empty after a failure, exactly `need` elements after a success
template <typename T>
static bool settled(const kge::DevBuf<T> &b, int rc, int64_t need) {
    return rc != 0 ? (b.ptr() == nullptr && b.cap() == 0) : (b.ptr() != nullptr && b.cap() == need);
}

int main() {
    using kge::DevBuf;
    int allocated = 0;
    {
        DevBuf<float> b;
        CHECK(b.ptr() == nullptr && b.cap() == 0);
        bool grew = true;
        int before = g_calls;
        int rc = b.reserve(0, "nothing", &grew);   // need <= cap: no call, even on an empty buffer
        CHECK(rc == 0 && !grew && g_calls == before && b.ptr() == nullptr);

        rc = b.reserve(1000, "first", &grew);
        CHECK(g_calls == before + 1 && grew);
        CHECK(settled(b, rc, 1000));
        allocated += rc == 0;

        // a smaller request: served from the capacity without a call, or -- after a failure -- attempted again
        float *had = b.ptr();
        before = g_calls;
        const int rc2 = b.reserve(10, "smaller", &grew);
        if (rc == 0) CHECK(rc2 == 0 && !grew && g_calls == before && b.ptr() == had && b.cap() == 1000);
        else CHECK(grew && g_calls == before + 1 && settled(b, rc2, 10));

        // equal to the capacity: no call
        before = g_calls;
        const int64_t cap = b.cap();
        CHECK(b.reserve(cap, "equal", &grew) == 0 && !grew && g_calls == before && b.cap() == cap);

        // growth allocates exactly what is asked, no more
        before = g_calls;
        rc = b.reserve(cap + 7, "grow", &grew);
        CHECK(grew && g_calls == before + 1 && settled(b, rc, cap + 7));
        allocated += rc == 0;
    }
    {   // a failed regrow leaves no capacity behind: a request this size cannot be met on any device
        DevBuf<char> b;
        int rc = b.reserve(64, "small");
        CHECK(settled(b, rc, 64));
        int before = g_calls;
        bool grew = false;
        rc = b.reserve(int64_t(1) << 60, "impossible", &grew);
        CHECK(rc != 0 && grew && g_calls == before + 1);
        CHECK(b.ptr() == nullptr && b.cap() == 0);
        before = g_calls;
        rc = b.reserve(32, "after the failure", &grew);   // smaller than what it once held: allocated anew all the same
        CHECK(grew && g_calls == before + 1 && settled(b, rc, 32));
    }
    {   // replace always allocates, at least one element; upload is replace plus one copy
        DevBuf<int> b;
        int before = g_calls;
        int rc = b.replace(0, "empty");
        CHECK(g_calls == before + 1 && settled(b, rc, 1));
        before = g_calls;
        rc = b.replace(0, "empty again");
        CHECK(g_calls == before + 1 && settled(b, rc, 1));
        const int src[5] = {1, 2, 3, 4, 5};
        before = g_calls;
        rc = b.upload(src, 5, "upload");
        CHECK(g_calls == before + (rc == 0 ? 2 : 1) && settled(b, rc, 5));
        if (rc == 0) {
            int back[5] = {0, 0, 0, 0, 0};
            CHECK(hipMemcpy(back, b.ptr(), sizeof(back), hipMemcpyDeviceToHost) == hipSuccess && back[0] == 1 && back[4] == 5);
        }
        before = g_calls;
        rc = b.upload(src, 0, "upload nothing");   // no copy of zero elements, a pointer all the same
        CHECK(g_calls == before + 1 && settled(b, rc, 1));

        int *p = b.release();
        CHECK(b.ptr() == nullptr && b.cap() == 0);
        CHECK((p != nullptr) == (rc == 0));
        DevBuf<int> c;
        c.adopt(p, 1);
        CHECK(c.ptr() == p && c.cap() == (p ? 1 : 0));
        c.free();
        CHECK(c.ptr() == nullptr && c.cap() == 0);
    }
    {   // the scoped form frees on scope exit; the plain one has no destructor to run at process exit
        kge::ScopedDevBuf<double> t;
        const int rc = t.replace(16, "scoped");
        CHECK(settled(t, rc, 16));
        static_assert(std::is_trivially_destructible<DevBuf<double>>::value, "a workspace must not free from a static destructor");
        static_assert(!std::is_copy_constructible<DevBuf<double>>::value && !std::is_copy_assignable<DevBuf<double>>::value, "not copyable");
    }
    {   // A group of buffers behind one "ensure", written the way the engine writes them (csrc/transe_counts.hip
        // ensure_counts_work): ids are filled directly behind their own reserve, the scratch is sized when an array grew OR
        // while there is none.  Whichever allocation of the first call fails, the second call must end with ids filled and
        // a scratch present -- a fill or a sizing placed behind a later allocation that can fail would be skipped for good.
        struct Group {
            DevBuf<int> ids, other;
            DevBuf<char> scratch;
            int ensure(int64_t n) {
                bool grew, any;
                int rc = ids.reserve(n, "ids", &any);
                if (rc) return rc;
                if (any) for (int64_t i = 0; i < n; i++) ids.ptr()[i] = (int)i;      // (host memory under g_fake)
                if ((rc = other.reserve(n, "other", &grew))) return rc;
                any |= grew;
                if (any || !scratch) rc = scratch.reserve(16 * ids.cap(), "scratch");
                return rc;
            }
        };
        g_fake = true;
        for (int fail_at = 1; fail_at <= 3; fail_at++) {
            Group g;
            g_fake_allocs = 0; g_fail_at = fail_at;
            CHECK(g.ensure(100) != 0);
            g_fail_at = 0;
            CHECK(g.ensure(100) == 0);
            CHECK(g.ids.cap() == 100 && g.other.cap() == 100 && g.scratch.ptr() && g.scratch.cap() == 1600);
            bool filled = g.ids.ptr() != nullptr;
            for (int i = 0; filled && i < 100; i++) filled = g.ids.ptr()[i] == i;
            CHECK(filled);
            const int before = g_fake_allocs;
            CHECK(g.ensure(40) == 0 && g_fake_allocs == before);      // steady state: no allocation
            g.ids.free(); g.other.free(); g.scratch.free();
        }
        g_fake = false;
    }
    std::printf("checks %d failed %d calls %d allocated %d\n", g_checks, g_failed, g_calls, allocated);
    return g_failed ? 1 : 0;
}
