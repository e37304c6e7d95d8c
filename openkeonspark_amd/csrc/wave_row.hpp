// A wave's view of one embedding row, shared by the kernels that give a whole wave one row at every width (shared_proj.hip,
// shared_transr.hip): loads and stores in global memory and LDS, the reductions, normalise and its backward, and the TransH /
// TransD side projection with its backward.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/kge_mi355.h"
#include "team.hpp"

namespace kge {

__device__ __forceinline__ int sgn_i(float e) { return (e > 0.f ? 1 : 0) - (e < 0.f ? 1 : 0); }

// A wave's view of one row of width D: lane l holds elements 4 (l + 64 q) .. + 3, q < Q; elements from D on are zero.
template <int Q, bool VEC>
struct WaveRow {
    static constexpr int V = 4 * Q;
    int lane, D, RS;
    __device__ __forceinline__ bool has(int q) const { return 4 * (lane + 64 * q) < RS; }
    template <typename T>
    __device__ __forceinline__ void load(const T *__restrict__ p, T (&x)[V]) const {
        typedef T T4 __attribute__((ext_vector_type(4)));
#pragma unroll
        for (int q = 0; q < Q; q++) {
            const int e0 = 4 * (lane + 64 * q);
            if constexpr (VEC) {
                T4 v = {0, 0, 0, 0};
                if (has(q)) v = *reinterpret_cast<const T4 *>(p + e0);
                x[4 * q] = v.x; x[4 * q + 1] = v.y; x[4 * q + 2] = v.z; x[4 * q + 3] = v.w;
            } else {
#pragma unroll
                for (int i = 0; i < 4; i++) x[4 * q + i] = e0 + i < D ? p[e0 + i] : T(0);
            }
        }
    }
    template <typename T>
    __device__ __forceinline__ void store(T *__restrict__ p, const T (&x)[V]) const {
        typedef T T4 __attribute__((ext_vector_type(4)));
#pragma unroll
        for (int q = 0; q < Q; q++) {
            const int e0 = 4 * (lane + 64 * q);
            if constexpr (VEC) {
                if (has(q)) { T4 v = {x[4 * q], x[4 * q + 1], x[4 * q + 2], x[4 * q + 3]}; *reinterpret_cast<T4 *>(p + e0) = v; }
            } else {
#pragma unroll
                for (int i = 0; i < 4; i++) if (e0 + i < D) p[e0 + i] = x[4 * q + i];
            }
        }
    }
    // rows in LDS have stride RS and zeros from D on: one 16-byte access per q at every width
    template <typename T>
    __device__ __forceinline__ void load_lds(const T *p, T (&x)[V]) const {
        typedef T T4 __attribute__((ext_vector_type(4)));
#pragma unroll
        for (int q = 0; q < Q; q++) {
            T4 v = {0, 0, 0, 0};
            if (has(q)) v = *reinterpret_cast<const T4 *>(p + 4 * (lane + 64 * q));
            x[4 * q] = v.x; x[4 * q + 1] = v.y; x[4 * q + 2] = v.z; x[4 * q + 3] = v.w;
        }
    }
    template <typename T>
    __device__ __forceinline__ void store_lds(T *p, const T (&x)[V]) const {
        typedef T T4 __attribute__((ext_vector_type(4)));
#pragma unroll
        for (int q = 0; q < Q; q++)
            if (has(q)) { T4 v = {x[4 * q], x[4 * q + 1], x[4 * q + 2], x[4 * q + 3]}; *reinterpret_cast<T4 *>(p + 4 * (lane + 64 * q)) = v; }
    }
    __device__ __forceinline__ float dot(const float (&a)[V], const float (&b)[V]) const {
        float s = 0.f;
#pragma unroll
        for (int c = 0; c < V; c++) s = __builtin_fmaf(a[c], b[c], s);
        return team_sum<64>(s);
    }
    // Team::normalize / normalize_bwd (team.hpp) in this layout: x rsqrt(max(sum x^2, 1e-12)); clipped: the backward is inv * gy
    __device__ __forceinline__ void normalize(const float (&x)[V], float (&y)[V], float &inv, bool &unclipped) const {
        const float ss = dot(x, x);
        unclipped = ss >= 1e-12f;
        inv = 1.0f / sqrtf(unclipped ? ss : 1e-12f);
#pragma unroll
        for (int c = 0; c < V; c++) y[c] = x[c] * inv;
    }
    __device__ __forceinline__ void normalize_bwd(const float (&y)[V], const float (&gy)[V], float inv, bool unclipped, float (&gx)[V]) const {
        float d = dot(y, gy);
        if (!unclipped) d = 0.f;
#pragma unroll
        for (int c = 0; c < V; c++) gx[c] = inv * (gy[c] - d * y[c]);
    }
    // side_project<MODEL> (models_dev.hpp).  TransH: a = x . w^, x^ = l2n(x - a w^), cw = w^ (xt is not read).
    // TransD: a = x . x_p, x^ = l2n(x + a r_p), xt = x_p, cw = r_p
    template <int MODEL>
    __device__ __forceinline__ void project(const float (&x)[V], const float (&xt)[V], const float (&cw)[V], float (&xn)[V], float &a, float &inv,
                                            bool &unclipped) const {
        float xp[V];
        if constexpr (MODEL == KGE_TRANSD) {
            a = dot(x, xt);
#pragma unroll
            for (int c = 0; c < V; c++) xp[c] = x[c] + a * cw[c];
        } else {
            a = dot(x, cw);
#pragma unroll
            for (int c = 0; c < V; c++) xp[c] = x[c] - a * cw[c];
        }
        normalize(xp, xn, inv, unclipped);
    }
    // row `id` of the entity table (TransD: and of ent_transfer), projected and normalised
    template <int MODEL>
    __device__ __forceinline__ void gather_project(const float *__restrict__ ent, const float *__restrict__ entp, long long id, const float (&cw)[V],
                                                   float (&x)[V], float (&xt)[V], float (&xn)[V], float &a, float &inv, bool &unclipped) const {
        load(ent + id * D, x);
        if constexpr (MODEL == KGE_TRANSD) load(entp + id * D, xt);
        project<MODEL>(x, xt, cw, xn, a, inv, unclipped);
    }
    __device__ __forceinline__ bool any_nonzero(const int (&g)[V]) const {
        int o = 0;
#pragma unroll
        for (int c = 0; c < V; c++) o |= g[c];
        return __ballot(o != 0) != 0;
    }
    // side_backward<MODEL> of unit * G: the row's gradient record (TransD: and its transfer row's, into out_t), and its share of
    // d/dw^ (TransD: d/dr_p) into acw
    template <int MODEL>
    __device__ __forceinline__ void side_record(const float (&x)[V], const float (&xt)[V], const float (&xn)[V], float a, float inv, bool unclipped,
                                                const int (&G)[V], float unit, const float (&cw)[V], float (&acw)[V], float *__restrict__ out,
                                                float *__restrict__ out_t) const {
        float g[V], gxp[V];
#pragma unroll
        for (int c = 0; c < V; c++) g[c] = unit * (float)G[c];
        normalize_bwd(xn, g, inv, unclipped, gxp);
        const float d = dot(gxp, cw);
        if constexpr (MODEL == KGE_TRANSD) {
#pragma unroll
            for (int c = 0; c < V; c++) g[c] = d * x[c];
            store(out_t, g);
#pragma unroll
            for (int c = 0; c < V; c++) {
                g[c] = gxp[c] + d * xt[c];
                acw[c] += a * gxp[c];
            }
        } else {
#pragma unroll
            for (int c = 0; c < V; c++) {
                g[c] = gxp[c] - d * cw[c];
                acw[c] -= d * x[c] + a * gxp[c];
            }
        }
        store(out, g);
    }
};

}  // namespace kge
