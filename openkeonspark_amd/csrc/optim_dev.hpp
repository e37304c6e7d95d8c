// Optimiser sweeps as device functions (same arithmetic for the one-launch-per-step kernels of optim.hip and for the
// persistent multi-step launch of persist.hip): SGD p -= lr*g and TF1-semantics Adam (_apply_sparse_shared op order); and
// TF1-semantics Adagrad, which the dense sweep of optim.hip and the touched-rows kernels of transe_counts.hip share; and row-wise
// Adagrad (one accumulator per table row), shared the same way.
#pragma once
#include "engine.hpp"
#include "team.hpp"

namespace kge {

// up to four tables per launch: blockIdx.y selects the table (one launch per optimizer step instead of one per table)
struct SweepTables {
    float *p[4], *g[4], *m[4], *v[4];   // Adagrad: m = the accumulators, v unused
    long long n[4];
};

// p -= lr * g; g = 0 over one table, threads tid, tid + stride, ... (16 B per lane; untouched 16-byte groups are skipped).
// U groups per thread are loaded before any is processed (U x 16 B in flight per lane): the one-launch kernel has enough
// threads to cover the memory latency with U = 1; the persistent launch (one workgroup per CU) needs the bytes in flight per
// thread instead.  Same arithmetic per element whatever U.
template <int U = 1>
__device__ __forceinline__ void sgd_sweep(float *__restrict__ p, float *__restrict__ g, long long n, float lr, long long tid, long long stride) {
    const long long n4 = n >> 2;
    float4 *p4 = reinterpret_cast<float4 *>(p);
    float4 *g4 = reinterpret_cast<float4 *>(g);
    for (long long i0 = tid; i0 < n4; i0 += stride * U) {
        float4 gv[U], pv[U];
        bool live[U];
#pragma unroll
        for (int u = 0; u < U; u++) {
            const long long i = i0 + stride * u;
            gv[u] = g4[i < n4 ? i : i0];
            live[u] = i < n4 && (gv[u].x != 0.f || gv[u].y != 0.f || gv[u].z != 0.f || gv[u].w != 0.f);  // untouched rows: p - lr*0 == p, skip the stores
        }
#pragma unroll
        for (int u = 0; u < U; u++) pv[u] = p4[live[u] ? i0 + stride * u : i0];
#pragma unroll
        for (int u = 0; u < U; u++) {
            if (live[u]) {
                const long long i = i0 + stride * u;
                pv[u].x -= lr * gv[u].x; pv[u].y -= lr * gv[u].y; pv[u].z -= lr * gv[u].z; pv[u].w -= lr * gv[u].w;
                p4[i] = pv[u];
                g4[i] = make_float4(0.f, 0.f, 0.f, 0.f);
            }
        }
    }
    for (long long i = (n4 << 2) + tid; i < n; i += stride) {
        p[i] -= lr * g[i];
        g[i] = 0.f;
    }
}

__device__ __forceinline__ void adam_one(float &p, float &m, float &v, float g, float lr_t, float b1, float b2, float eps) {
    // TF1 op order, each product rounded before the add.  HIP's __fmul_rn / __fadd_rn are plain `*` / `+` (__clang_hip_math.h) and
    // would be contracted into fma where the optimizer sees fit -- differently from one inlining context to the next: contraction is
    // switched off for this body, so every caller gets the same bits
#pragma clang fp contract(off)
    float mi = mul_rn(m, b1);
    float vi = mul_rn(v, b2);
    if (g != 0.f) {
        mi = add_rn(mi, mul_rn(g, 1.0f - b1));
        vi = add_rn(vi, mul_rn(mul_rn(g, g), 1.0f - b2));
    }
    m = mi; v = vi;
    p = sub_rn(p, __fdiv_rn(mul_rn(lr_t, mi), add_rn(__fsqrt_rn(vi), eps)));
}

__device__ __forceinline__ void adam_sweep(float *__restrict__ p, float *__restrict__ m, float *__restrict__ v, float *__restrict__ g, long long n,
                                           float lr_t, float b1, float b2, float eps, long long tid, long long stride) {
    const long long n4 = n >> 2;
    float4 *p4 = reinterpret_cast<float4 *>(p), *m4 = reinterpret_cast<float4 *>(m);
    float4 *v4 = reinterpret_cast<float4 *>(v), *g4 = reinterpret_cast<float4 *>(g);
    for (long long i = tid; i < n4; i += stride) {
        float4 pv = p4[i], mv = m4[i], vv = v4[i], gv = g4[i];
        adam_one(pv.x, mv.x, vv.x, gv.x, lr_t, b1, b2, eps);
        adam_one(pv.y, mv.y, vv.y, gv.y, lr_t, b1, b2, eps);
        adam_one(pv.z, mv.z, vv.z, gv.z, lr_t, b1, b2, eps);
        adam_one(pv.w, mv.w, vv.w, gv.w, lr_t, b1, b2, eps);
        p4[i] = pv; m4[i] = mv; v4[i] = vv;
        if (gv.x != 0.f || gv.y != 0.f || gv.z != 0.f || gv.w != 0.f) g4[i] = make_float4(0.f, 0.f, 0.f, 0.f);
    }
    for (long long i = (n4 << 2) + tid; i < n; i += stride) {
        adam_one(p[i], m[i], v[i], g[i], lr_t, b1, b2, eps);
        g[i] = 0.f;
    }
}

// TF1 AdagradOptimizer, one element: a += g*g; p -= lr * g / sqrt(a) -- no epsilon (the accumulators start at a positive value,
// Config.adagrad_initial_accumulator).  An element with zero gradient keeps p and a bit for bit, which is the plain formula
// wherever a > 0 and safe whatever a holds: updating only the rows a step touches IS the dense rule.  Contraction off, as above.
__device__ __forceinline__ void adagrad_one(float &p, float &a, float g, float lr) {
#pragma clang fp contract(off)
    if (g != 0.f) {
        a = add_rn(a, mul_rn(g, g));
        p = sub_rn(p, __fdiv_rn(mul_rn(lr, g), __fsqrt_rn(a)));
    }
}

// the dense form: 16-byte groups whose gradient is all zero are skipped (nothing of theirs changes), the gradient consumed is zeroed
__device__ __forceinline__ void adagrad_sweep(float *__restrict__ p, float *__restrict__ a, float *__restrict__ g, long long n, float lr,
                                              long long tid, long long stride) {
    const long long n4 = n >> 2;
    float4 *p4 = reinterpret_cast<float4 *>(p), *a4 = reinterpret_cast<float4 *>(a), *g4 = reinterpret_cast<float4 *>(g);
    for (long long i = tid; i < n4; i += stride) {
        const float4 gv = g4[i];
        if (gv.x == 0.f && gv.y == 0.f && gv.z == 0.f && gv.w == 0.f) continue;
        float4 pv = p4[i], av = a4[i];
        adagrad_one(pv.x, av.x, gv.x, lr);
        adagrad_one(pv.y, av.y, gv.y, lr);
        adagrad_one(pv.z, av.z, gv.z, lr);
        adagrad_one(pv.w, av.w, gv.w, lr);
        p4[i] = pv; a4[i] = av;
        g4[i] = make_float4(0.f, 0.f, 0.f, 0.f);
    }
    for (long long i = (n4 << 2) + tid; i < n; i += stride) {
        const float gi = g[i];
        if (gi == 0.f) continue;
        adagrad_one(p[i], a[i], gi, lr);
        g[i] = 0.f;
    }
}

// Row-wise Adagrad (PyTorch-BigGraph's RowAdagrad): ONE accumulator per table row, which takes the row's mean squared gradient,
//     q = sum_j g[j]^2;  a += q / len;  s = sqrt(a);  p[j] -= (lr * g[j]) / s  where g[j] != 0
// in fp32 with contraction off, no epsilon (the accumulators start at Config.adagrad_initial_accumulator > 0; PBG's own form
// starts at 0 and adds 1e-10 to the root).  A row whose gradient is all zero has q = 0 and keeps p and a bit for bit, so the
// touched rows are all the dense rule moves.  The three pieces below are shared by the dense kernel of optim.hip and the
// touched-rows kernels of transe_counts.hip; each caller sums the squares in one fixed order of its own (a lane's elements in
// index order through rowadagrad_sq, then team_sum), the same in every run.
__device__ __forceinline__ float rowadagrad_sq(float q, float g) {
#pragma clang fp contract(off)
    return add_rn(q, mul_rn(g, g));
}
// a += q / len; returns sqrt(a).  q is the row's complete sum (the same value in every lane); len <= 2^24 is exact as a float.
__device__ __forceinline__ float rowadagrad_root(float &a, float q, int len) {
#pragma clang fp contract(off)
    a = add_rn(a, __fdiv_rn(q, (float)len));
    return __fsqrt_rn(a);
}
__device__ __forceinline__ float rowadagrad_one(float p, float g, float lr, float root) {
#pragma clang fp contract(off)
    return sub_rn(p, __fdiv_rn(mul_rn(lr, g), root));
}

// The dense form over ONE table of `rows` rows of `len` elements: T = 64 threads (a wave; four rows per workgroup) or T = 256 (the
// workgroup) per row, V = 4: float4 accesses (len % 4 == 0, 16-byte aligned tables) or V = 1.  Pass 1 sums the squares -- thread t
// takes the groups t, t + T, ... in order, the wave sums through team_sum<64>, the workgroup adds its four waves in wave order --
// and notes whether any element is non-zero; a row without gradient is left here: nothing of p, a or g is written.  Pass 2
// re-reads g (rows may be as long as a 512 x 512 matrix: it loops), moves the elements whose gradient is not zero and zeroes
// the gradient it consumed.
template <int T, int V>
__device__ __forceinline__ void rowadagrad_rows(float *__restrict__ p, float *__restrict__ acc, float *__restrict__ g, long long rows, int len,
                                                float lr, float *wave_q) {
    constexpr int RPB = 256 / T;
    const int t = threadIdx.x % T;
    // (T = 256: `row` is the same for the whole workgroup, which the barriers below need; the bound is rounded up to it)
    for (long long row = (long long)blockIdx.x * RPB + threadIdx.x / T; row < rows; row += (long long)gridDim.x * RPB) {
        float *gr = g + row * len, *pr = p + row * len;
        const float a_old = acc[row];       // read by every thread before thread 0 may write it (behind the barrier where T = 256)
        float q = 0.f;
        bool any = false;
        for (int j = t * V; j < len; j += T * V) {
            if constexpr (V == 4) {
                const float4 gv = *reinterpret_cast<const float4 *>(gr + j);
                q = rowadagrad_sq(rowadagrad_sq(rowadagrad_sq(rowadagrad_sq(q, gv.x), gv.y), gv.z), gv.w);
                any = any || gv.x != 0.f || gv.y != 0.f || gv.z != 0.f || gv.w != 0.f;
            } else {
                const float gj = gr[j];
                q = rowadagrad_sq(q, gj);
                any = any || gj != 0.f;
            }
        }
        q = team_sum<64>(q);
        if constexpr (T == 256) {
            if (threadIdx.x % 64 == 0) wave_q[threadIdx.x / 64] = q;
            any = __syncthreads_or(any) != 0;
            q = add_rn(add_rn(add_rn(wave_q[0], wave_q[1]), wave_q[2]), wave_q[3]);
        } else {
            any = __ballot(any) != 0;
        }
        if (any) {
            float a = a_old;
            const float root = rowadagrad_root(a, q, len);
            for (int j = t * V; j < len; j += T * V) {
                if constexpr (V == 4) {
                    const float4 gv = *reinterpret_cast<const float4 *>(gr + j);
                    if (gv.x == 0.f && gv.y == 0.f && gv.z == 0.f && gv.w == 0.f) continue;
                    float4 pv = *reinterpret_cast<const float4 *>(pr + j);
                    if (gv.x != 0.f) pv.x = rowadagrad_one(pv.x, gv.x, lr, root);
                    if (gv.y != 0.f) pv.y = rowadagrad_one(pv.y, gv.y, lr, root);
                    if (gv.z != 0.f) pv.z = rowadagrad_one(pv.z, gv.z, lr, root);
                    if (gv.w != 0.f) pv.w = rowadagrad_one(pv.w, gv.w, lr, root);
                    *reinterpret_cast<float4 *>(pr + j) = pv;
                    *reinterpret_cast<float4 *>(gr + j) = make_float4(0.f, 0.f, 0.f, 0.f);
                } else {
                    const float gj = gr[j];
                    if (gj == 0.f) continue;
                    pr[j] = rowadagrad_one(pr[j], gj, lr, root);
                    gr[j] = 0.f;
                }
            }
            if (t == 0 && q != 0.f) acc[row] = a;     // (q == 0 with a non-zero element -- squares that underflow -- leaves a as it is)
        }
        if constexpr (T == 256) __syncthreads();      // wave_q is read by all before the next row's sums are written
    }
}

}  // namespace kge
