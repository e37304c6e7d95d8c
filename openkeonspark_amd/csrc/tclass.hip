// Triple classification on the device (kge_tc_fit / kge_tc_apply): the per-relation threshold grid search of
// getBestThreshold (eval.hip, Test.h:304-341) and the TP / TN / FP / FN counts of test_triple_classification (Test.h:347-387) over
// DEVICE score arrays, with the host routines' bits.
//
// The host tries every grid point g(i) = fmaf(i, 0.01f, min), i = 0..n_interval, against every validation score of the relation.
// g is non-decreasing in i (i < 2^24: the conversion, the product and the sum are monotone roundings), so a score s changes sides
// exactly once, at k(s) = min{ i : s <= g(i) }: a positive is correct from k(s) on, a negative before it.  With
// delta[k(pos)] += 1, delta[k(neg)] -= 1 the host's inner count is  correct(i) = n_r + sum_{j <= i} delta[j]  -- one pass that
// bins the scores, a prefix sum, an arg-max.  Scores above g(n_interval) land in bin n_interval + 1, which is never summed.
//
// Launches of a fit (one stream):
//   tc_init      min / max keys of every relation, status word
//   tc_minmax    one workgroup per CHUNK of a relation's range (a relation of many triples spans many workgroups); the float
//                order is kept by an unsigned key, so the merge is an integer atomicMin / atomicMax; non-finite scores are flagged
//   tc_prepare   per relation: min, n_interval (IEEE fp32 division), the path it takes, its offset in the global histogram
//   -- the host waits here for the 16-byte status: a non-finite score, n_interval >= 2^24 and the histogram's size decide
//      the return code and an allocation; nothing behind this point is waited for --
//   tc_bin       (relations on the global path) one workgroup per chunk bins into the library's global int32 histogram
//   tc_fit       one workgroup per relation: LDS path = zero, bin with LDS atomics, scan, arg-max; global path = scan, arg-max
// A relation takes the LDS path when its n_interval + 2 bins fit the 16 000-bin LDS histogram AND it has at most 4096
// validation triples; a relation with more triples (the skewed ones) or a wider grid takes the global path, where its
// binning is spread over one workgroup per 2048 triples and only the scan is left to a single workgroup.
//
// ROC curves and AUC (kge_tc_roc): get_TPFP (eval.hip, Test.h:410-444) counts, for every point of the SAME
// grid, the split's positives and negatives at or below it.  With hpos[k] / hneg[k] = the split's positives / negatives of bin
// k(s), TP(i) = sum_{k <= i} hpos[k] and FP(i) = sum_{k <= i} hneg[k]: the fit's binning pass with two counters and its scan
// carrying two sums.  Twice the trapezoid area under (0,0), (FP(i),TP(i))..., (n_r,n_r) is the integer
// area2 = sum_k hneg[k] * (2 * TPexcl[k] + hpos[k]) over all n_interval + 2 bins (the last bin is the closing segment).
// Launches of a ROC call (one stream): tc_init, tc_minmax, tc_prepare on the validation scores as above, then
//   tc_finite       flags a non-finite split score (before the wait, so that an error writes nothing)
//   tc_roc_prepare  per relation: the path by the SPLIT's triple count, its slice of the doubled global histogram and of d_tpfp
//   -- the one wait: status and every relation's n_interval (the host forms h_offsets from them) --
//   tc_roc_bin      (global path) one workgroup per chunk of the split's list, hpos then hneg in the relation's slice
//   tc_roc          one workgroup per relation: LDS path = zero, bin both sides into 16-bit halves of one word, scan, write;
//                   global path = scan, write; a relation without split triples gets zeros, one without validation (0, 0)
#include <cfloat>

#include "eval_dev.hpp"

namespace kge {
namespace {

constexpr int kChunk = 2048;            // triples per work item of the chunked kernels
constexpr int kThreads = 256;           // ... and their workgroup
constexpr int kFitThreads = 512;
constexpr int kFitWaves = kFitThreads / 64;
constexpr int kLdsBins = 16000;         // int32 bins of the LDS histogram (62.5 KB: two workgroups per CU)
constexpr int kFusedMaxTriples = 4096;  // LDS path: one workgroup bins the whole relation
constexpr long long kMaxGlobalBins = 1ll << 28;   // 1 GiB of int32 bins
constexpr long long kMaxInterval = 1ll << 24;     // (float)i is exact and g monotone below this
constexpr float kInterval = 0.01f;      // Setting.h:118
enum { kPathNone = 0, kPathLds = 1, kPathGlobal = 2, kPathEmpty = 3 };   // kPathEmpty (ROC): validation but no split triples
enum { kFlagNonFinite = 1, kFlagTooWide = 2, kFlagSplitNonFinite = 4 };

struct TcStatus {
    int32_t flags, pad;
    long long bins;       // int32 bins the global path needs
};

struct TcDev {
    bool ready = false;
    uint64_t generation = 0;
    int64_t R = 0, total[2] = {0, 0};
    DevBuf<int32_t> lef[2], rig[2];
    DevBuf<int4> items[2];                    // (relation, first position, count, 0): chunks of at most kChunk triples
    int n_items[2] = {0, 0};
    DevBuf<uint32_t> kmin, kmax;
    DevBuf<float> mn;
    DevBuf<int32_t> nint, path;
    DevBuf<long long> off;
    DevBuf<int32_t> hist;
    DevBuf<TcStatus> status;
    TcStatus *status_host = nullptr;
    hipEvent_t ev = nullptr;
    DevBuf<long long> out_off;                // ROC: every relation's first element of d_tpfp
    int32_t *nint_host = nullptr;             // ROC: pinned [R], read in the one wait
    std::vector<char> has_valid;              // ROC: host copy of lef[0][r] >= 0
};
TcDev g_tc;

// ---------------------------------------------------------------------------------------------
// floats as unsigned keys of the same order (-0 counted as +0: the grid is the same from either)
__device__ __forceinline__ uint32_t order_key(float s) {
    const uint32_t u = __float_as_uint(s + 0.0f);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float order_key_inv(uint32_t k) { return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k); }

// eval.hip:grid_point -- ONE rounding
__device__ __forceinline__ float grid_point(float mn, int i) { return __fmaf_rn((float)i, kInterval, mn); }

// k(s) = min{ i in [0, n] : s <= g(i) }, or n + 1 when s > g(n).  The quotient only says where to start looking.
__device__ __forceinline__ int grid_bin(float s, float mn, int n) {
    const float q = __fdiv_rn(__fsub_rn(s, mn), kInterval);
    int e = q >= (float)(n + 1) ? n + 1 : (q > 0.f ? (int)q : 0);
    while (e > 0 && s <= grid_point(mn, e - 1)) e--;
    while (e <= n && s > grid_point(mn, e)) e++;
    return e;
}

__global__ void tc_init_kernel(int64_t R, uint32_t *__restrict__ kmin, uint32_t *__restrict__ kmax, TcStatus *__restrict__ st) {
    const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r < R) { kmin[r] = 0xFFFFFFFFu; kmax[r] = 0u; }
    if (r == 0) { st->flags = 0; st->pad = 0; st->bins = 0; }
}

__global__ __launch_bounds__(kThreads) void tc_minmax_kernel(const int4 *__restrict__ items, const float *__restrict__ pos,
                                                             const float *__restrict__ neg, uint32_t *__restrict__ kmin,
                                                             uint32_t *__restrict__ kmax, TcStatus *__restrict__ st) {
    const int4 it = items[blockIdx.x];
    uint32_t lo = 0xFFFFFFFFu, hi = 0u;
    bool bad = false;
    for (int i = threadIdx.x; i < it.z; i += kThreads) {
        const float a = pos[it.y + i], b = neg[it.y + i];
        bad |= !(fabsf(a) <= FLT_MAX) || !(fabsf(b) <= FLT_MAX);
        const uint32_t ka = order_key(a), kb = order_key(b);
        lo = min(lo, min(ka, kb));
        hi = max(hi, max(ka, kb));
    }
    for (int o = 32; o > 0; o >>= 1) {
        lo = min(lo, (uint32_t)__shfl_xor((int)lo, o));
        hi = max(hi, (uint32_t)__shfl_xor((int)hi, o));
    }
    const bool any_bad = __any(bad);
    if ((threadIdx.x & 63) == 0) {
        if (lo <= hi) { atomicMin(&kmin[it.x], lo); atomicMax(&kmax[it.x], hi); }
        if (any_bad) atomicOr(&st->flags, kFlagNonFinite);
    }
}

// one workgroup: every relation's grid, its path and (an exclusive scan over the relations) its slice of the global histogram
__global__ __launch_bounds__(kThreads) void tc_prepare_kernel(int64_t R, const int32_t *__restrict__ lef, const int32_t *__restrict__ rig,
                                                              const uint32_t *__restrict__ kmin, const uint32_t *__restrict__ kmax,
                                                              float *__restrict__ mn_out, int32_t *__restrict__ nint,
                                                              int32_t *__restrict__ path, long long *__restrict__ off, TcStatus *__restrict__ st) {
    __shared__ long long seg_sum[kThreads];
    const int64_t seg = (R + kThreads - 1) / kThreads;
    const int64_t r0 = min((int64_t)threadIdx.x * seg, R), r1 = min(r0 + seg, R);
    long long need = 0;
    int flags = 0;
    for (int64_t r = r0; r < r1; r++) {
        int p = kPathNone;
        long long n = 0;
        if (lef[r] >= 0) {
            const float mn = order_key_inv(kmin[r]), mx = order_key_inv(kmax[r]);
            n = (long long)__fdiv_rn(__fsub_rn(mx, mn), kInterval);   // Test.h:322: (INT)((max - min) / interval)
            mn_out[r] = mn;
            if (n >= kMaxInterval || n < 0) { flags |= kFlagTooWide; n = 0; }
            else if (n + 2 <= kLdsBins && rig[r] - lef[r] + 1 <= kFusedMaxTriples) p = kPathLds;
            else { p = kPathGlobal; need += n + 2; }
        }
        nint[r] = (int32_t)n;
        path[r] = p;
    }
    seg_sum[threadIdx.x] = need;
    if (flags) atomicOr(&st->flags, flags);
    __syncthreads();
    if (threadIdx.x == 0) {
        long long run = 0;
        for (int i = 0; i < kThreads; i++) { const long long v = seg_sum[i]; seg_sum[i] = run; run += v; }
        st->bins = run;
    }
    __syncthreads();
    long long run = seg_sum[threadIdx.x];
    for (int64_t r = r0; r < r1; r++) {
        off[r] = run;
        if (path[r] == kPathGlobal) run += (long long)nint[r] + 2;
    }
}

__global__ __launch_bounds__(kThreads) void tc_bin_kernel(const int4 *__restrict__ items, const float *__restrict__ pos,
                                                          const float *__restrict__ neg, const float *__restrict__ mnv,
                                                          const int32_t *__restrict__ nint, const int32_t *__restrict__ path,
                                                          const long long *__restrict__ off, int32_t *__restrict__ hist) {
    const int4 it = items[blockIdx.x];
    if (path[it.x] != kPathGlobal) return;
    const float mn = mnv[it.x];
    const int n = nint[it.x];
    int32_t *h = hist + off[it.x];
    for (int i = threadIdx.x; i < it.z; i += kThreads) {
        atomicAdd(&h[grid_bin(pos[it.y + i], mn, n)], 1);
        atomicAdd(&h[grid_bin(neg[it.y + i], mn, n)], -1);
    }
}

// accuracy at grid point i with `correct` right answers out of `total`, as the host forms it (Test.h:333), packed so that the
// maximum is the host's winner: the LOWEST i whose float accuracy is strictly greater than all before it
__device__ __forceinline__ unsigned long long acc_key(long long correct, double total, int i) {
    const float acc = (float)(1.0 * (double)correct / total);
    return ((unsigned long long)__float_as_uint(acc) << 32) | (unsigned long long)(0xFFFFFFFFu - (uint32_t)i);
}

__global__ __launch_bounds__(kFitThreads) void tc_fit_kernel(const int32_t *__restrict__ lef, const int32_t *__restrict__ rig,
                                                             const float *__restrict__ pos, const float *__restrict__ neg,
                                                             const float *__restrict__ mnv, const int32_t *__restrict__ nint,
                                                             const int32_t *__restrict__ path, const long long *__restrict__ off,
                                                             const int32_t *__restrict__ hist, float *__restrict__ thresh) {
    __shared__ int32_t bins[kLdsBins];
    __shared__ int32_t wave_sum[kFitWaves];
    __shared__ unsigned long long wave_best[kFitWaves];
    const int r = blockIdx.x, p = path[r];
    if (p == kPathNone) return;
    const float mn = mnv[r];
    const int n = nint[r], lo = lef[r], n_r = rig[r] - lo + 1;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int32_t *h = hist + off[r];
    if (p == kPathLds) {
        for (int i = tid; i < n + 2; i += kFitThreads) bins[i] = 0;
        __syncthreads();
        for (int i = tid; i < n_r; i += kFitThreads) {
            atomicAdd(&bins[grid_bin(pos[lo + i], mn, n)], 1);
            atomicAdd(&bins[grid_bin(neg[lo + i], mn, n)], -1);
        }
        __syncthreads();
        h = bins;
    }
    long long carry = n_r;        // every negative is right, every positive wrong, below the first grid point
    const double total = 2.0 * (double)n_r;
    unsigned long long best = 0;
    for (int base = 0; base <= n; base += kFitThreads) {
        const int i = base + tid;
        int x = i <= n ? h[i] : 0;
        for (int o = 1; o < 64; o <<= 1) { const int y = __shfl_up(x, o); if (lane >= o) x += y; }
        if (lane == 63) wave_sum[wave] = x;
        __syncthreads();
        int before = 0, all = 0;
        for (int w = 0; w < kFitWaves; w++) { const int s = wave_sum[w]; if (w < wave) before += s; all += s; }
        if (i <= n) { const unsigned long long k = acc_key(carry + before + x, total, i); if (k > best) best = k; }
        carry += all;
        __syncthreads();
    }
    for (int o = 32; o > 0; o >>= 1) {
        const unsigned hi32 = __shfl_xor((unsigned)(best >> 32), o), lo32 = __shfl_xor((unsigned)best, o);
        const unsigned long long other = ((unsigned long long)hi32 << 32) | lo32;
        if (other > best) best = other;
    }
    if (lane == 0) wave_best[wave] = best;
    __syncthreads();
    if (tid == 0) {
        for (int w = 1; w < kFitWaves; w++) if (wave_best[w] > best) best = wave_best[w];
        thresh[r] = grid_point(mn, (int)(0xFFFFFFFFu - (uint32_t)best));
    }
}

// one workgroup per chunk of the split's list; a chunk lies inside one relation, so the threshold is uniform
__global__ __launch_bounds__(kThreads) void tc_apply_kernel(const int4 *__restrict__ items, const int32_t *__restrict__ valid_lef,
                                                            const float *__restrict__ thresh, const float *__restrict__ pos,
                                                            const float *__restrict__ neg, unsigned long long *__restrict__ counts,
                                                            unsigned long long *__restrict__ rel) {
    __shared__ int wave_tp[kThreads / 64], wave_tn[kThreads / 64];
    const int4 it = items[blockIdx.x];
    if (valid_lef[it.x] < 0) return;      // Test.h:353: only relations with validation AND test triples
    const float th = thresh[it.x];
    int tp = 0, tn = 0;
    for (int i = threadIdx.x; i < it.z; i += kThreads) {
        tp += pos[it.y + i] <= th ? 1 : 0;
        tn += neg[it.y + i] > th ? 1 : 0;
    }
    for (int o = 32; o > 0; o >>= 1) { tp += __shfl_xor(tp, o); tn += __shfl_xor(tn, o); }
    if ((threadIdx.x & 63) == 0) { wave_tp[threadIdx.x >> 6] = tp; wave_tn[threadIdx.x >> 6] = tn; }
    __syncthreads();
    if (threadIdx.x == 0) {
        tp = 0; tn = 0;
        for (int w = 0; w < kThreads / 64; w++) { tp += wave_tp[w]; tn += wave_tn[w]; }
        atomicAdd(&counts[0], (unsigned long long)tp);
        atomicAdd(&counts[1], (unsigned long long)tn);
        atomicAdd(&counts[2], (unsigned long long)(it.z - tn));
        atomicAdd(&counts[3], (unsigned long long)(it.z - tp));
        if (rel) {
            atomicAdd(&rel[2 * (size_t)it.x], (unsigned long long)(tp + tn));
            atomicAdd(&rel[2 * (size_t)it.x + 1], (unsigned long long)(2 * it.z));
        }
    }
}

// ---- ROC (kge_tc_roc) ----
__global__ __launch_bounds__(kThreads) void tc_finite_kernel(const float *__restrict__ pos, const float *__restrict__ neg, int64_t n,
                                                             TcStatus *__restrict__ st) {
    bool bad = false;
    for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < n; i += (int64_t)gridDim.x * kThreads)
        bad |= !(fabsf(pos[i]) <= FLT_MAX) || !(fabsf(neg[i]) <= FLT_MAX);
    if (__any(bad) && (threadIdx.x & 63) == 0) atomicOr(&st->flags, kFlagSplitNonFinite);
}

// one workgroup, behind tc_prepare (which has left the grid in mn / nint): the path of every relation by the SPLIT's side,
// its slice of the global histogram (hpos then hneg, n_interval + 2 bins each) and of the output (TP then FP, n_interval + 1 each)
__global__ __launch_bounds__(kThreads) void tc_roc_prepare_kernel(int64_t R, const int32_t *__restrict__ valid_lef,
                                                                  const int32_t *__restrict__ lef, const int32_t *__restrict__ rig,
                                                                  const int32_t *__restrict__ nint, int32_t *__restrict__ path,
                                                                  long long *__restrict__ off, long long *__restrict__ out_off,
                                                                  TcStatus *__restrict__ st) {
    __shared__ long long seg_need[kThreads], seg_out[kThreads];
    const int64_t seg = (R + kThreads - 1) / kThreads;
    const int64_t r0 = min((int64_t)threadIdx.x * seg, R), r1 = min(r0 + seg, R);
    long long need = 0, out = 0;
    for (int64_t r = r0; r < r1; r++) {
        int p = kPathNone;
        if (valid_lef[r] >= 0) {
            const long long n = nint[r];
            const int n_r = lef[r] >= 0 ? rig[r] - lef[r] + 1 : 0;
            out += 2 * (n + 1);
            if (n_r == 0) p = kPathEmpty;
            else if (n + 2 <= kLdsBins && n_r <= kFusedMaxTriples) p = kPathLds;
            else { p = kPathGlobal; need += 2 * (n + 2); }
        }
        path[r] = p;
    }
    seg_need[threadIdx.x] = need;
    seg_out[threadIdx.x] = out;
    __syncthreads();
    if (threadIdx.x == 0) {
        long long run = 0, run_out = 0;
        for (int i = 0; i < kThreads; i++) {
            const long long v = seg_need[i], w = seg_out[i];
            seg_need[i] = run; seg_out[i] = run_out;
            run += v; run_out += w;
        }
        st->bins = run;
    }
    __syncthreads();
    long long run = seg_need[threadIdx.x], run_out = seg_out[threadIdx.x];
    for (int64_t r = r0; r < r1; r++) {
        off[r] = run;
        out_off[r] = run_out;
        if (path[r] == kPathGlobal) run += 2 * ((long long)nint[r] + 2);
        if (path[r] != kPathNone) run_out += 2 * ((long long)nint[r] + 1);
    }
}

__global__ __launch_bounds__(kThreads) void tc_roc_bin_kernel(const int4 *__restrict__ items, const float *__restrict__ pos,
                                                              const float *__restrict__ neg, const float *__restrict__ mnv,
                                                              const int32_t *__restrict__ nint, const int32_t *__restrict__ path,
                                                              const long long *__restrict__ off, int32_t *__restrict__ hist) {
    const int4 it = items[blockIdx.x];
    if (path[it.x] != kPathGlobal) return;
    const float mn = mnv[it.x];
    const int n = nint[it.x];
    int32_t *hp = hist + off[it.x], *hn = hp + n + 2;
    for (int i = threadIdx.x; i < it.z; i += kThreads) {
        atomicAdd(&hp[grid_bin(pos[it.y + i], mn, n)], 1);
        atomicAdd(&hn[grid_bin(neg[it.y + i], mn, n)], 1);
    }
}

// lef / rig: the split's ranges.  On the LDS path a word of `bins` holds hpos in its low and hneg in its high 16 bits: a
// relation on that path has at most kFusedMaxTriples = 4096 triples, so neither half overflows.
__global__ __launch_bounds__(kFitThreads) void tc_roc_kernel(const int32_t *__restrict__ lef, const int32_t *__restrict__ rig,
                                                             const float *__restrict__ pos, const float *__restrict__ neg,
                                                             const float *__restrict__ mnv, const int32_t *__restrict__ nint,
                                                             const int32_t *__restrict__ path, const long long *__restrict__ off,
                                                             const int32_t *__restrict__ hist, const long long *__restrict__ out_off,
                                                             int64_t *__restrict__ tpfp, int64_t *__restrict__ auc2) {
    __shared__ uint32_t bins[kLdsBins];
    __shared__ int32_t wave_tp[kFitWaves], wave_fp[kFitWaves];
    __shared__ long long wave_area[kFitWaves];
    const int r = blockIdx.x, p = path[r];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int n = nint[r];
    int64_t *out = tpfp ? tpfp + out_off[r] : nullptr;
    if (p == kPathNone || p == kPathEmpty) {
        if (p == kPathEmpty && out)
            for (int i = tid; i < 2 * (n + 1); i += kFitThreads) out[i] = 0;
        if (tid == 0) { auc2[2 * (size_t)r] = 0; auc2[2 * (size_t)r + 1] = 0; }
        return;
    }
    const float mn = mnv[r];
    const int lo = lef[r], n_r = rig[r] - lo + 1;
    const int32_t *hp = hist + off[r], *hn = hp + n + 2;
    if (p == kPathLds) {
        for (int i = tid; i < n + 2; i += kFitThreads) bins[i] = 0u;
        __syncthreads();
        for (int i = tid; i < n_r; i += kFitThreads) {
            atomicAdd(&bins[grid_bin(pos[lo + i], mn, n)], 1u);
            atomicAdd(&bins[grid_bin(neg[lo + i], mn, n)], 1u << 16);
        }
        __syncthreads();
    }
    long long carry_tp = 0, carry_fp = 0, area = 0;
    for (int base = 0; base <= n + 1; base += kFitThreads) {
        const int i = base + tid;
        int a = 0, b = 0;     // hpos[i], hneg[i]
        if (i <= n + 1) {
            if (p == kPathLds) { const uint32_t v = bins[i]; a = (int)(v & 0xFFFFu); b = (int)(v >> 16); }
            else { a = hp[i]; b = hn[i]; }
        }
        int x = a, y = b;
        for (int o = 1; o < 64; o <<= 1) {
            const int xo = __shfl_up(x, o), yo = __shfl_up(y, o);
            if (lane >= o) { x += xo; y += yo; }
        }
        if (lane == 63) { wave_tp[wave] = x; wave_fp[wave] = y; }
        __syncthreads();
        int before_tp = 0, all_tp = 0, before_fp = 0, all_fp = 0;
        for (int w = 0; w < kFitWaves; w++) {
            const int s = wave_tp[w], t = wave_fp[w];
            if (w < wave) { before_tp += s; before_fp += t; }
            all_tp += s; all_fp += t;
        }
        if (i <= n + 1) {
            const long long tp = carry_tp + before_tp + x, fp = carry_fp + before_fp + y;
            area += (long long)b * (2 * (tp - a) + a);
            if (out && i <= n) { out[i] = tp; out[(size_t)n + 1 + i] = fp; }
        }
        carry_tp += all_tp;
        carry_fp += all_fp;
        __syncthreads();
    }
    for (int o = 32; o > 0; o >>= 1) area += __shfl_xor(area, o);
    if (lane == 0) wave_area[wave] = area;
    __syncthreads();
    if (tid == 0) {
        for (int w = 1; w < kFitWaves; w++) area += wave_area[w];
        auc2[2 * (size_t)r] = area;
        auc2[2 * (size_t)r + 1] = n_r;
    }
}

// ---------------------------------------------------------------------------------------------
// the range arrays and the chunk lists on the device: once per importTestFiles
int ensure_tc_device() {
    TcDev &d = g_tc;
    const int64_t R = engine().index.rel_total;
    if (d.ready && d.generation == eval_tc_generation() && d.R == R) return KGE_OK;
    TcLists l;
    int rc = eval_tc_lists(l);
    if (rc) return rc;
    d.ready = false;
    for (int s = 0; s < 2; s++) {
        if ((int64_t)l.lef[s]->size() != R) return fail(KGE_ERR_BAD_ARG, "triple classification: relation ranges do not match the training set's relations");
        if ((rc = d.lef[s].upload(*l.lef[s], "upload relation ranges"))) return rc;
        if ((rc = d.rig[s].upload(*l.rig[s], "upload relation ranges"))) return rc;
        std::vector<int4> items;
        for (int64_t r = 0; r < R; r++) {
            const int lo = (*l.lef[s])[(size_t)r], hi = (*l.rig[s])[(size_t)r];
            if (lo < 0) continue;
            if (hi < lo || hi >= l.total[s]) return fail(KGE_ERR_BAD_ARG, "triple classification: relation range outside its list");
            for (int at = lo; at <= hi; at += kChunk) items.push_back(make_int4((int)r, at, std::min(kChunk, hi - at + 1), 0));
        }
        if ((rc = d.items[s].upload(items, "upload classification chunks"))) return rc;
        d.n_items[s] = (int)items.size();
        d.total[s] = l.total[s];
    }
    if ((rc = d.kmin.replace(R, "alloc classification state"))) return rc;
    if ((rc = d.kmax.replace(R, "alloc classification state"))) return rc;
    if ((rc = d.mn.replace(R, "alloc classification state"))) return rc;
    if ((rc = d.nint.replace(R, "alloc classification state"))) return rc;
    if ((rc = d.path.replace(R, "alloc classification state"))) return rc;
    if ((rc = d.off.replace(R, "alloc classification state"))) return rc;
    if ((rc = d.out_off.replace(R, "alloc classification state"))) return rc;
    if (d.nint_host) { (void)hipHostFree(d.nint_host); d.nint_host = nullptr; }
    if ((rc = hip_check(hipHostMalloc(&d.nint_host, sizeof(int32_t) * (size_t)(R ? R : 1)), "alloc classification status"))) return rc;
    d.has_valid.assign((size_t)R, 0);
    for (int64_t r = 0; r < R; r++) d.has_valid[(size_t)r] = (*l.lef[0])[(size_t)r] >= 0;
    if ((rc = d.status.reserve(1, "alloc classification state"))) return rc;
    if (!d.status_host && (rc = hip_check(hipHostMalloc(&d.status_host, sizeof(TcStatus)), "alloc classification status"))) return rc;
    if (!d.ev && (rc = hip_check(hipEventCreateWithFlags(&d.ev, hipEventDisableTiming), "create event"))) return rc;
    d.generation = eval_tc_generation();
    d.R = R;
    d.ready = true;
    return KGE_OK;
}

}  // namespace
}  // namespace kge

using namespace kge;

extern "C" int kge_tc_fit(const float *d_pos, const float *d_neg, INT n_valid, float *d_thresh, int32_t *d_n_interval, void *stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (!d_pos || !d_neg || !d_thresh) return fail(KGE_ERR_BAD_ARG, "kge_tc_fit: null score or threshold array");
    if (!device_ok()) return fail(KGE_ERR_NO_DEVICE, "kge_tc_fit: no usable HIP device");
    int rc = ensure_tc_device();
    if (rc) return rc;
    TcDev &d = g_tc;
    if (n_valid != d.total[0]) return fail(KGE_ERR_BAD_ARG, "kge_tc_fit: n_valid is not the validation set's size");
    const unsigned rel_blocks = (unsigned)((d.R + kThreads - 1) / kThreads);
    tc_init_kernel<<<rel_blocks ? rel_blocks : 1, kThreads, 0, stream>>>(d.R, d.kmin, d.kmax, d.status);
    if (d.n_items[0] > 0)
        tc_minmax_kernel<<<d.n_items[0], kThreads, 0, stream>>>(d.items[0], d_pos, d_neg, d.kmin, d.kmax, d.status);
    tc_prepare_kernel<<<1, kThreads, 0, stream>>>(d.R, d.lef[0], d.rig[0], d.kmin, d.kmax, d.mn, d.nint, d.path, d.off, d.status);
    if ((rc = hip_check(hipMemcpyAsync(d.status_host, d.status, sizeof(TcStatus), hipMemcpyDeviceToHost, stream), "read classification status"))) return rc;
    if ((rc = hip_check(hipEventRecord(d.ev, stream), "record event"))) return rc;
    if ((rc = hip_check(hipEventSynchronize(d.ev), "wait for the score ranges"))) return rc;
    const TcStatus st = *d.status_host;
    if (st.flags & kFlagNonFinite) return fail(KGE_ERR_BAD_ARG, "kge_tc_fit: non-finite validation score (no threshold written)");
    if (st.flags & kFlagTooWide) return fail(KGE_ERR_UNSUPPORTED, "kge_tc_fit: a relation's grid has 2^24 points or more (no threshold written)");
    if (st.bins > kMaxGlobalBins) return fail(KGE_ERR_UNSUPPORTED, "kge_tc_fit: the relations' grids need more than 2^28 histogram bins (no threshold written)");
    // the caller's copy only now: on the error returns above d_n_interval is as untouched as d_thresh
    if (d_n_interval && (rc = hip_check(hipMemcpyAsync(d_n_interval, d.nint, sizeof(int32_t) * (size_t)d.R, hipMemcpyDeviceToDevice, stream), "copy n_interval"))) return rc;
    if (d.n_items[0] == 0) return KGE_OK;
    // at least one bin: tc_fit forms hist + off[r] on every path
    if ((rc = d.hist.reserve(st.bins > 0 ? st.bins : 1, "alloc classification histogram"))) return rc;
    if (st.bins > 0) {
        if ((rc = hip_check(hipMemsetAsync(d.hist, 0, sizeof(int32_t) * (size_t)st.bins, stream), "clear classification histogram"))) return rc;
        tc_bin_kernel<<<d.n_items[0], kThreads, 0, stream>>>(d.items[0], d_pos, d_neg, d.mn, d.nint, d.path, d.off, d.hist);
    }
    tc_fit_kernel<<<(unsigned)d.R, kFitThreads, 0, stream>>>(d.lef[0], d.rig[0], d_pos, d_neg, d.mn, d.nint, d.path, d.off, d.hist, d_thresh);
    return hip_check(hipGetLastError(), "kge_tc_fit launch");
}

extern "C" int kge_tc_apply(INT split, const float *d_thresh, const float *d_pos, const float *d_neg, INT n, int64_t *d_counts,
                            int64_t *d_rel, void *stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (!d_thresh || !d_pos || !d_neg || !d_counts) return fail(KGE_ERR_BAD_ARG, "kge_tc_apply: null threshold, score or count array");
    if (split != 0 && split != 1) return fail(KGE_ERR_BAD_ARG, "kge_tc_apply: split must be 0 (validation) or 1 (test)");
    if (!device_ok()) return fail(KGE_ERR_NO_DEVICE, "kge_tc_apply: no usable HIP device");
    int rc = ensure_tc_device();
    if (rc) return rc;
    TcDev &d = g_tc;
    if (n != d.total[split]) return fail(KGE_ERR_BAD_ARG, "kge_tc_apply: n is not the split's size");
    if ((rc = hip_check(hipMemsetAsync(d_counts, 0, sizeof(int64_t) * 4, stream), "clear counts"))) return rc;
    if (d_rel && (rc = hip_check(hipMemsetAsync(d_rel, 0, sizeof(int64_t) * 2 * (size_t)d.R, stream), "clear counts"))) return rc;
    if (d.n_items[split] > 0)
        tc_apply_kernel<<<d.n_items[split], kThreads, 0, stream>>>(d.items[split], d.lef[0], d_thresh, d_pos, d_neg,
                                                                   (unsigned long long *)d_counts, (unsigned long long *)d_rel);
    return hip_check(hipGetLastError(), "kge_tc_apply launch");
}

extern "C" int kge_tc_roc(const float *d_vpos, const float *d_vneg, INT n_valid, INT split, const float *d_pos, const float *d_neg,
                          INT n, int64_t *d_auc2, int64_t *d_tpfp, INT tpfp_capacity, int64_t *h_offsets, void *stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (!d_vpos || !d_vneg || !d_pos || !d_neg || !d_auc2 || !h_offsets) return fail(KGE_ERR_BAD_ARG, "kge_tc_roc: null score, result or offset array");
    if (split != 0 && split != 1) return fail(KGE_ERR_BAD_ARG, "kge_tc_roc: split must be 0 (validation) or 1 (test)");
    if (!device_ok()) return fail(KGE_ERR_NO_DEVICE, "kge_tc_roc: no usable HIP device");
    int rc = ensure_tc_device();
    if (rc) return rc;
    TcDev &d = g_tc;
    if (n_valid != d.total[0]) return fail(KGE_ERR_BAD_ARG, "kge_tc_roc: n_valid is not the validation set's size");
    if (n != d.total[split]) return fail(KGE_ERR_BAD_ARG, "kge_tc_roc: n is not the split's size");
    const unsigned rel_blocks = (unsigned)((d.R + kThreads - 1) / kThreads);
    tc_init_kernel<<<rel_blocks ? rel_blocks : 1, kThreads, 0, stream>>>(d.R, d.kmin, d.kmax, d.status);
    if (d.n_items[0] > 0)
        tc_minmax_kernel<<<d.n_items[0], kThreads, 0, stream>>>(d.items[0], d_vpos, d_vneg, d.kmin, d.kmax, d.status);
    tc_prepare_kernel<<<1, kThreads, 0, stream>>>(d.R, d.lef[0], d.rig[0], d.kmin, d.kmax, d.mn, d.nint, d.path, d.off, d.status);
    if (n > 0)
        tc_finite_kernel<<<(unsigned)std::min<int64_t>((n + kChunk - 1) / kChunk, 1024), kThreads, 0, stream>>>(d_pos, d_neg, n, d.status);
    tc_roc_prepare_kernel<<<1, kThreads, 0, stream>>>(d.R, d.lef[0], d.lef[split], d.rig[split], d.nint, d.path, d.off, d.out_off, d.status);
    if ((rc = hip_check(hipMemcpyAsync(d.status_host, d.status, sizeof(TcStatus), hipMemcpyDeviceToHost, stream), "read classification status"))) return rc;
    if (d.R > 0 && (rc = hip_check(hipMemcpyAsync(d.nint_host, d.nint, sizeof(int32_t) * (size_t)d.R, hipMemcpyDeviceToHost, stream), "read n_interval"))) return rc;
    if ((rc = hip_check(hipEventRecord(d.ev, stream), "record event"))) return rc;
    if ((rc = hip_check(hipEventSynchronize(d.ev), "wait for the score ranges"))) return rc;
    const TcStatus st = *d.status_host;
    if (st.flags & kFlagNonFinite) return fail(KGE_ERR_BAD_ARG, "kge_tc_roc: non-finite validation score (nothing written)");
    if (st.flags & kFlagSplitNonFinite) return fail(KGE_ERR_BAD_ARG, "kge_tc_roc: non-finite score in the split (nothing written)");
    if (st.flags & kFlagTooWide) return fail(KGE_ERR_UNSUPPORTED, "kge_tc_roc: a relation's grid has 2^24 points or more (nothing written)");
    if (st.bins > kMaxGlobalBins) return fail(KGE_ERR_UNSUPPORTED, "kge_tc_roc: the relations' grids need more than 2^28 histogram bins (nothing written)");
    h_offsets[0] = 0;
    for (int64_t r = 0; r < d.R; r++)
        h_offsets[r + 1] = h_offsets[r] + (d.has_valid[(size_t)r] ? 2 * ((int64_t)d.nint_host[r] + 1) : 0);
    if (d_tpfp && tpfp_capacity < h_offsets[d.R]) return fail(KGE_ERR_BAD_ARG, "kge_tc_roc: tpfp_capacity is below h_offsets[rel_total] (nothing written)");
    if (d.R == 0) return KGE_OK;
    // at least one bin: tc_roc forms hist + off[r] on every path
    if ((rc = d.hist.reserve(st.bins > 0 ? st.bins : 1, "alloc classification histogram"))) return rc;
    if (st.bins > 0) {
        if ((rc = hip_check(hipMemsetAsync(d.hist, 0, sizeof(int32_t) * (size_t)st.bins, stream), "clear classification histogram"))) return rc;
        tc_roc_bin_kernel<<<d.n_items[split], kThreads, 0, stream>>>(d.items[split], d_pos, d_neg, d.mn, d.nint, d.path, d.off, d.hist);
    }
    tc_roc_kernel<<<(unsigned)d.R, kFitThreads, 0, stream>>>(d.lef[split], d.rig[split], d_pos, d_neg, d.mn, d.nint, d.path, d.off, d.hist,
                                                            d.out_off, d_tpfp, d_auc2);
    return hip_check(hipGetLastError(), "kge_tc_roc launch");
}
