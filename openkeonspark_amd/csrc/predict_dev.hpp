// kge_predict's score written out operation by operation, for the kernels that must return its bits from another inlining
// context (rank_cand.hip's fused ranker, bf16_eval.hip's predict on stored bf16 rows).  predict_kernel (models.hip) leaves
// e = hn + rn - tn to the compiler's contraction licence, and as compiled (all 21 instantiations read in the ISA) it is
//     e = fma(-xt, inv_t, fma(r_raw, inv_r, hn))        hn = xh * inv_h rounded on its own
// with xh / xt the projected, un-normalised sides (TransH: fma(-a, w, raw); TransD: fma(a, r_p, raw)), inv_* = 1 / sqrt(max(ss,
// 1e-12)) from Team::dot, the per-lane sum of |e| in index order, team_sum<L> and lane 0's value; TransE divides by (float)D.
// Every product and sum here is a __builtin_fmaf, mul_rn or add_rn, so the bits do not hang on the including file's optimiser.
#pragma once
#include "../../include/kge_mi355.h"
#include "team.hpp"

namespace kge {

// the projected, un-normalised vector of an entity row and 1 / |it|: side_project's operations (models_dev.hpp), with the
// products it leaves to contraction written as the fma predict_kernel compiles them to
template <int MODEL, int L, int C>
__device__ __forceinline__ void project_row(const Team<L, C> &tm, const float (&raw)[C], const float (&aux)[C], const float (&cw)[C],
                                            float (&xp)[C], float &inv) {
    if constexpr (MODEL == KGE_TRANSH) {
        const float a = tm.dot(raw, cw);
#pragma unroll
        for (int c = 0; c < C; c++) xp[c] = __builtin_fmaf(-a, cw[c], raw[c]);
    } else if constexpr (MODEL == KGE_TRANSD) {
        const float a = tm.dot(raw, aux);
#pragma unroll
        for (int c = 0; c < C; c++) xp[c] = __builtin_fmaf(a, cw[c], raw[c]);
    } else {
#pragma unroll
        for (int c = 0; c < C; c++) xp[c] = raw[c];
    }
    const float ss = tm.dot(xp, xp);
    inv = 1.0f / sqrtf(ss >= 1e-12f ? ss : 1e-12f);
}

// predict_kernel's score of (head, relation, tail) from the head's normalised vector hn, the relation's raw row and 1 / |row|,
// and the tail's projected vector and 1 / |it|; lane 0's team_sum value in every lane of the team
template <int MODEL, int L, int C>
__device__ __forceinline__ float predict_score(const float (&hn)[C], const float (&rr)[C], float inv_r, const float (&xt)[C], float inv_t, int D) {
    float s = 0.f;
#pragma unroll
    for (int c = 0; c < C; c++) s = add_rn(s, fabsf(__builtin_fmaf(-xt[c], inv_t, __builtin_fmaf(rr[c], inv_r, hn[c]))));
    s = team_sum<L>(s);
    if constexpr (L != 64) s = __shfl(s, 0, L);
    if constexpr (MODEL == KGE_TRANSE) s = s / (float)D;
    return s;
}

}  // namespace kge
