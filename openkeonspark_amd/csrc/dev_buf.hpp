// The one owner of device memory in the engine: a pointer and its element capacity, kept together.
//
// A DevBuf is a process-lifetime workspace: it only grows, its contents do not survive a regrow, and it
// is never freed at exit (no destructor: the HIP runtime may be gone before static destructors run).
// ScopedDevBuf is the same thing for a temporary that does free when it leaves scope.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

namespace kge {

int hip_check(hipError_t e, const char *what);   // 0, or an error code after recording `what`

// Bytes held by every DevBuf / ScopedDevBuf of the process (kge_workspace_bytes): hipMalloc is invisible to a caller's own
// allocator statistics, so the engine counts what it owns.  `peak` is the largest `live` since the last reset.  Inline variables:
// one total per process, header only.  The engine is driven from one host thread at a time, as its workspaces are.
struct DevBufBytes {
    int64_t live = 0, peak = 0;
    void add(int64_t bytes) {
        live += bytes;
        if (live > peak) peak = live;
    }
};
inline DevBufBytes g_dev_buf_bytes;

template <typename T>
class DevBuf {
public:
    DevBuf() = default;
    DevBuf(const DevBuf &) = delete;
    DevBuf &operator=(const DevBuf &) = delete;

    T *ptr() const { return p_; }
    operator T *() const { return p_; }
    int64_t cap() const { return cap_; }

    // Room for `need` elements.  need <= cap(): nothing happens, no HIP call.  Otherwise free, then allocate exactly
    // `need` (no geometric growth: peak and steady memory are what the caller asks for); *grew tells the caller that
    // the contents are gone.  On failure the buffer is empty (null, capacity 0) and the hip_check code comes back.
    int reserve(int64_t need, const char *what, bool *grew = nullptr) {
        if (grew) *grew = false;
        if (need <= cap_) return 0;
        if (grew) *grew = true;
        return alloc(need, what);
    }
    // Always free and allocate n elements (at least one, so the pointer is never null on success).
    int replace(int64_t n, const char *what) { return alloc(n > 0 ? n : 1, what); }
    // replace(n), then a synchronous copy of n elements from the host.
    int upload(const void *src, int64_t n, const char *what) {
        int rc = replace(n, what);
        if (!rc && n > 0 && (rc = hip_check(hipMemcpy(p_, src, sizeof(T) * (size_t)n, hipMemcpyHostToDevice), what))) free();
        return rc;
    }
    template <typename Vec>   // anything with data() and size(), elements of T's size
    int upload(const Vec &v, const char *what) {
        static_assert(sizeof(*v.data()) == sizeof(T), "element size mismatch");
        return upload(v.data(), (int64_t)v.size(), what);
    }
    void free() {
        if (p_) (void)hipFree(p_);
        p_ = nullptr;
        set_cap(0);
    }
    // hands the allocation to the caller
    T *release() {
        T *p = p_;
        p_ = nullptr;
        set_cap(0);
        return p;
    }
    // takes over an allocation of n elements (the other half of release()); what was held is freed
    void adopt(T *p, int64_t n) {
        free();
        p_ = p;
        set_cap(p ? n : 0);
    }

private:
    int alloc(int64_t n, const char *what) {
        free();
        int rc = hip_check(hipMalloc(&p_, sizeof(T) * (size_t)n), what);
        if (rc) p_ = nullptr;
        else set_cap(n);
        return rc;
    }
    // the one place the capacity changes: the process total follows it
    void set_cap(int64_t n) {
        g_dev_buf_bytes.add((int64_t)sizeof(T) * (n - cap_));
        cap_ = n;
    }
    T *p_ = nullptr;
    int64_t cap_ = 0;
};

template <typename T>
struct ScopedDevBuf : DevBuf<T> {
    ~ScopedDevBuf() { this->free(); }
};

}  // namespace kge
