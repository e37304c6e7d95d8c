// Evaluation lists on the device: what importTestFiles and ensure_eval_device (eval.hip) do with five std::sort calls on the
// host -- the union of train + valid + test in the (h,r,t), (t,r,h) and (h,t,r) orders, the test and validation lists in the
// (r,h,t) order (Reader.h:186-261, Triple.h:18-32) -- and what main_spark.py:209-290 n_n() does with Python dictionaries -- the
// distinct heads and tails of every relation -- done with rocPRIM radix sorts and a scan over packed 64-bit keys, as
// index_build.hip does for the sampler's index.
//
// Every array is bit-identical to the host build (tests/test_gpu_eval_arrays.py compares them all): the lists keep their
// duplicates and equal triples are interchangeable, so an unstable sort of the keys alone decides every bit.
//
//   triple (a,b,c) -> key = a << (bits_b + bits_c) | b << bits_c | c      (needs 2*bits(E) + bits(R) <= 64)
//   list:   pack the keys of one field order from the three splits where they lie, sort up to the bits in use, unpack into int4
//   types:  key = r << bits(E) | entity per side, sort, flag first-of-equal-key, scan, compact; a relation's [lef, rig) by bound search
#include "eval_dev.hpp"

#include <cstring>
#include <rocprim/rocprim.hpp>

namespace kge {

namespace {

int bits_for(int64_t count) {  // bits needed for values in [0, count)
    int b = 1;
    while ((int64_t(1) << b) < count) b++;
    return b;
}

constexpr int TPB = 256;
inline unsigned grid_for(int64_t n) {
    int64_t b = (n + TPB - 1) / TPB;
    if (b > 65536) b = 65536;
    if (b < 1) b = 1;
    return (unsigned)b;
}
#define KGE_GRID_LOOP(i, n) for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < (n); i += (long long)gridDim.x * blockDim.x)

// the union without a copy: entry i is a test, then a training, then a validation triple, each (h,t,r,0)
struct UnionSrc {
    const int4 *test, *train, *valid;
    long long n_test, n_train, n_valid;
};
__device__ __forceinline__ int4 union_at(const UnionSrc &s, long long i) {
    if (i < s.n_test) return s.test[i];
    i -= s.n_test;
    if (i < s.n_train) return s.train[i];
    return s.valid[i - s.n_train];
}

// field orders of a key, most significant first
enum { kOrderHRT = 0, kOrderTRH = 1, kOrderHTR = 2, kOrderRHT = 3 };

__global__ void pack_order_kernel(UnionSrc s, long long n, int order, int be, int br, uint64_t *__restrict__ keys) {
    KGE_GRID_LOOP(i, n) {
        const int4 p = union_at(s, i);   // (h, t, r)
        const uint64_t h = (uint32_t)p.x, t = (uint32_t)p.y, r = (uint32_t)p.z;
        uint64_t k;
        if (order == kOrderHRT) k = (h << (br + be)) | (r << be) | t;
        else if (order == kOrderTRH) k = (t << (br + be)) | (r << be) | h;
        else if (order == kOrderHTR) k = (h << (be + br)) | (t << br) | r;
        else k = (r << (2 * be)) | (h << be) | t;
        keys[i] = k;
    }
}

// sorted keys -> the list's int4: the fields in key order for the three union orders, (h,t,r,0) for the (r,h,t)-sorted lists
__global__ void unpack_order_kernel(const uint64_t *__restrict__ keys, long long n, int order, int be, int br, int4 *__restrict__ out) {
    const int wb = order == kOrderHTR || order == kOrderRHT ? be : br, wc = order == kOrderHTR ? br : be;
    const uint64_t mb = (uint64_t(1) << wb) - 1, mc = (uint64_t(1) << wc) - 1;
    KGE_GRID_LOOP(i, n) {
        const uint64_t k = keys[i];
        const int a = (int)(k >> (wb + wc)), b = (int)((k >> wc) & mb), c = (int)(k & mc);
        out[i] = order == kOrderRHT ? make_int4(b, c, a, 0) : make_int4(a, b, c, 0);
    }
}

// all = (h,r,t,0): key r << be | head (heads != 0) or tail
__global__ void type_keys_kernel(const int4 *__restrict__ all, long long n, int heads, int be, uint64_t *__restrict__ keys) {
    KGE_GRID_LOOP(i, n) {
        const int4 p = all[i];
        keys[i] = ((uint64_t)(uint32_t)p.y << be) | (uint64_t)(uint32_t)(heads ? p.x : p.z);
    }
}

__global__ void first_of_run_kernel(const uint64_t *__restrict__ keys, long long n, int32_t *__restrict__ flag) {
    KGE_GRID_LOOP(k, n) flag[k] = (k == 0 || keys[k] != keys[k - 1]) ? 1 : 0;
}

// uid = inclusive scan of the flags (1-based id of the distinct key); ids / rel [U]
__global__ void compact_kernel(const uint64_t *__restrict__ keys, const int32_t *__restrict__ uid, long long n, int be,
                               int32_t *__restrict__ ids, int32_t *__restrict__ rel) {
    const uint64_t me = (uint64_t(1) << be) - 1;
    KGE_GRID_LOOP(k, n) {
        if (k == 0 || keys[k] != keys[k - 1]) {
            const int32_t u = uid[k] - 1;
            ids[u] = (int32_t)(keys[k] & me);
            rel[u] = (int32_t)(keys[k] >> be);
        }
    }
}

// rel [U] is non-decreasing: relation r's list is [first entry >= r, first entry > r)
__global__ void rel_bounds_kernel(const int32_t *__restrict__ rel, int U, long long R, int32_t *__restrict__ lef, int32_t *__restrict__ rig) {
    KGE_GRID_LOOP(r, R) {
        int lo = 0, hi = U;
        while (lo < hi) { const int mid = (lo + hi) >> 1; if (rel[mid] < r) lo = mid + 1; else hi = mid; }
        lef[r] = lo;
        hi = U;
        while (lo < hi) { const int mid = (lo + hi) >> 1; if (rel[mid] <= r) lo = mid + 1; else hi = mid; }
        rig[r] = lo;
    }
}

struct Scratch {
    ScopedDevBuf<char> tmp;
    int ensure(size_t need) { return tmp.reserve((int64_t)need, "eval build: sort scratch"); }
};

int sort_keys(Scratch &sc, const uint64_t *kin, uint64_t *kout, size_t n, int bits) {
    size_t need = 0;
    int rc = hip_check(rocprim::radix_sort_keys(nullptr, need, kin, kout, n, 0, (unsigned)bits, nullptr), "eval sort size");
    if (rc) return rc;
    if ((rc = sc.ensure(need))) return rc;
    return hip_check(rocprim::radix_sort_keys(sc.tmp.ptr(), need, kin, kout, n, 0, (unsigned)bits, nullptr), "eval sort");
}

int scan_flags(Scratch &sc, int32_t *flags, size_t n) {
    size_t need = 0;
    int rc = hip_check(rocprim::inclusive_scan(nullptr, need, flags, flags, n, rocprim::plus<int32_t>(), nullptr), "eval scan size");
    if (rc) return rc;
    if ((rc = sc.ensure(need))) return rc;
    return hip_check(rocprim::inclusive_scan(sc.tmp.ptr(), need, flags, flags, n, rocprim::plus<int32_t>(), nullptr), "eval scan");
}

// one list: the n entries of `s` in the given order -> out [n]
int build_list(Scratch &sc, const UnionSrc &s, int64_t n, int order, int be, int br, uint64_t *keys_a, uint64_t *keys_b, ScopedDevBuf<int4> &out,
               const char *what) {
    int rc = out.replace(n, what);
    if (rc || n == 0) return rc;
    hipLaunchKernelGGL(pack_order_kernel, dim3(grid_for(n)), dim3(TPB), 0, nullptr, s, (long long)n, order, be, br, keys_a);
    if ((rc = sort_keys(sc, keys_a, keys_b, (size_t)n, 2 * be + br))) return rc;
    hipLaunchKernelGGL(unpack_order_kernel, dim3(grid_for(n)), dim3(TPB), 0, nullptr, keys_b, (long long)n, order, be, br, out.ptr());
    return KGE_OK;
}

}  // namespace

bool device_eval_build_supported(int64_t E, int64_t R, int64_t n_all) {
    return n_all > 0 && E > 0 && R > 0 && n_all < (int64_t(1) << 31) && E < (int64_t(1) << 31) && R < (int64_t(1) << 31) &&
           2 * bits_for(E) + bits_for(R) <= 64;
}

int build_eval_lists_device(int64_t E, int64_t R, const int4 *d_train, int64_t n_train, const std::vector<Int4> &valid,
                            const std::vector<Int4> &test, EvalTriplesBuilt &out) {
    const int64_t n_valid = (int64_t)valid.size(), n_test = (int64_t)test.size(), n_all = n_test + n_train + n_valid;
    if (!device_eval_build_supported(E, R, n_all)) return fail(KGE_ERR_UNSUPPORTED, "device evaluation build: sizes not supported");
    const int be = bits_for(E), br = bits_for(R);
    int rc;
    ScopedDevBuf<int4> src_valid, src_test;   // file-order uploads: the only host-to-device traffic of the build
    if ((rc = src_valid.upload(valid, "eval build: valid"))) return rc;
    if ((rc = src_test.upload(test, "eval build: test"))) return rc;
    Scratch sc;
    ScopedDevBuf<uint64_t> keys_a, keys_b;
    if ((rc = keys_a.replace(n_all, "eval build: keys"))) return rc;
    if ((rc = keys_b.replace(n_all, "eval build: keys"))) return rc;
    const UnionSrc all_src{src_test, d_train, src_valid, (long long)n_test, (long long)n_train, (long long)n_valid};
    if ((rc = build_list(sc, all_src, n_all, kOrderHRT, be, br, keys_a, keys_b, out.all, "eval build: all"))) return rc;
    if ((rc = build_list(sc, all_src, n_all, kOrderTRH, be, br, keys_a, keys_b, out.all_t, "eval build: all by tail"))) return rc;
    if ((rc = build_list(sc, all_src, n_all, kOrderHTR, be, br, keys_a, keys_b, out.all_ht, "eval build: all by pair"))) return rc;
    const UnionSrc test_src{src_test, nullptr, nullptr, (long long)n_test, 0, 0};
    if ((rc = build_list(sc, test_src, n_test, kOrderRHT, be, br, keys_a, keys_b, out.test, "eval build: test list"))) return rc;
    const UnionSrc valid_src{src_valid, nullptr, nullptr, (long long)n_valid, 0, 0};
    if ((rc = build_list(sc, valid_src, n_valid, kOrderRHT, be, br, keys_a, keys_b, out.valid, "eval build: valid list"))) return rc;
    if ((rc = hip_check(hipDeviceSynchronize(), "eval build"))) return rc;
    return hip_check(hipGetLastError(), "eval build launch");
}

int derive_type_lists_device(int64_t E, int64_t R, const int4 *d_all, int64_t n_all, TypeListsBuilt &out) {
    if (!device_eval_build_supported(E, R, n_all)) return fail(KGE_ERR_UNSUPPORTED, "device type-list build: sizes not supported");
    const int be = bits_for(E), br = bits_for(R);
    int rc;
    Scratch sc;
    ScopedDevBuf<uint64_t> keys_a, keys_b;
    ScopedDevBuf<int32_t> uid, rel;
    if ((rc = keys_a.replace(n_all, "type build: keys"))) return rc;
    if ((rc = keys_b.replace(n_all, "type build: keys"))) return rc;
    if ((rc = uid.replace(n_all, "type build: flags"))) return rc;
    for (int heads = 1; heads >= 0; heads--) {
        ScopedDevBuf<int32_t> &lef = heads ? out.head_lef : out.tail_lef, &rig = heads ? out.head_rig : out.tail_rig;
        ScopedDevBuf<int32_t> &ids = heads ? out.head_type : out.tail_type;
        hipLaunchKernelGGL(type_keys_kernel, dim3(grid_for(n_all)), dim3(TPB), 0, nullptr, d_all, (long long)n_all, heads, be, keys_a.ptr());
        if ((rc = sort_keys(sc, keys_a, keys_b, (size_t)n_all, be + br))) return rc;
        hipLaunchKernelGGL(first_of_run_kernel, dim3(grid_for(n_all)), dim3(TPB), 0, nullptr, keys_b.ptr(), (long long)n_all, uid.ptr());
        if ((rc = scan_flags(sc, uid, (size_t)n_all))) return rc;
        int32_t U = 0;
        if ((rc = hip_check(hipMemcpy(&U, uid + (n_all - 1), sizeof(int32_t), hipMemcpyDeviceToHost), "type build: distinct count"))) return rc;
        if (U < 1 || U > n_all) return fail(KGE_ERR_NO_DEVICE, "type build: distinct count out of range");
        if ((rc = ids.replace(U, "type build: ids"))) return rc;
        if ((rc = rel.replace(U, "type build: relations"))) return rc;
        if ((rc = lef.replace(R, "type build: lef"))) return rc;
        if ((rc = rig.replace(R, "type build: rig"))) return rc;
        hipLaunchKernelGGL(compact_kernel, dim3(grid_for(n_all)), dim3(TPB), 0, nullptr, keys_b.ptr(), uid.ptr(), (long long)n_all, be, ids.ptr(),
                           rel.ptr());
        hipLaunchKernelGGL(rel_bounds_kernel, dim3(grid_for(R)), dim3(TPB), 0, nullptr, rel.ptr(), (int)U, (long long)R, lef.ptr(), rig.ptr());
        (heads ? out.n_head : out.n_tail) = U;
        if ((rc = hip_check(hipDeviceSynchronize(), "type build"))) return rc;   // `rel` is reused by the other side
    }
    return hip_check(hipGetLastError(), "type build launch");
}

}  // namespace kge
