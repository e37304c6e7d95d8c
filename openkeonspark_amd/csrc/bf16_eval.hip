// EVALUATION ON bf16 TABLES (include/kge_mi355.h, "Evaluation on bf16 tables"): the evaluators whose cost is the rows they gather
// read the stored bf16 rows themselves, so no float32 view of a table exists.  This file holds the rule of what is accepted
// (kge_bf16_eval_supported) and kge_predict_bf16; kge_rank_candidates_bf16 is rank_cand.hip's fused kernel under BF16.
//
// predict_bf16_kernel: one team per triple on predict_kernel's team shape and grid.  A row is loaded by Team::load's bf16 overload
// (lane l: elements l, l + L, ..., each widened exactly) and the score is predict_dev.hpp's written-out form of predict_kernel, so
// the result has kge_predict's bits on the widened tables and does not depend on how this file's optimiser contracts.
#include "engine.hpp"
#include "predict_dev.hpp"
#include "team.hpp"
#include "team_shape.hpp"

namespace kge {

namespace {

template <int L, int C>
__global__ __launch_bounds__(256) void predict_bf16_kernel(const uint16_t *__restrict__ ent, const uint16_t *__restrict__ rel,
                                                           const int32_t *__restrict__ bh, const int32_t *__restrict__ bt,
                                                           const int32_t *__restrict__ br, int D, long long n, float *__restrict__ out) {
    constexpr int TEAMS = 256 / L;
    Team<L, C> tm;
    tm.lane = threadIdx.x % L;
    tm.D = D;
    for (long long i = (long long)blockIdx.x * TEAMS + threadIdx.x / L; i < n; i += (long long)gridDim.x * TEAMS) {
        float raw[C], rr[C], hn[C], xt[C], inv_r, inv_h, inv_t;
        tm.load(rel, br[i], raw);
        project_row<KGE_TRANSE, L, C>(tm, raw, raw, raw, rr, inv_r);      // (TransE: the row itself and 1 / |row|)
        tm.load(ent, bh[i], raw);
        project_row<KGE_TRANSE, L, C>(tm, raw, raw, raw, hn, inv_h);
#pragma unroll
        for (int c = 0; c < C; c++) hn[c] = mul_rn(hn[c], inv_h);
        tm.load(ent, bt[i], raw);
        project_row<KGE_TRANSE, L, C>(tm, raw, raw, raw, xt, inv_t);
        const float s = predict_score<KGE_TRANSE, L, C>(hn, rr, inv_r, xt, inv_t, D);
        if (tm.lane == 0) out[i] = s;
    }
}

}  // namespace

// the storage rule of "bf16 table storage", without the limits that belong to a training step
const char *bf16_eval_refusal(const kge_model_desc *m) {
    if (!m) return "no model descriptor";
    if (m->model != KGE_TRANSE) return "evaluation on bf16 tables is built for TransE only";
    if (m->ent_dim != m->rel_dim) return "evaluation on bf16 tables: entity and relation widths differ";
    if (m->ent_dim % 8 != 0 || m->ent_dim < 8) return "evaluation on bf16 tables needs a width that is a multiple of 8 (rows of 16-byte chunks)";
    if (m->ent_dim > 1024) return "evaluation on bf16 tables: widths up to 1024";
    return nullptr;
}

// dispatch_predict's grid (models.hip): one team per triple, at most 8192 workgroups, a grid-stride loop beyond
int launch_predict_bf16(const kge_model_desc &m, const uint16_t *d_ent, const uint16_t *d_rel, const int32_t *d_h, const int32_t *d_t,
                        const int32_t *d_r, int64_t n, float *d_out, hipStream_t stream) {
    if (!device_ok()) return fail(KGE_ERR_NO_DEVICE, "kge_predict_bf16: no usable HIP device");
    if (n <= 0) return KGE_OK;
    const bool shaped = for_team_shape((int)m.ent_dim, [&](auto t) {
        constexpr int L = decltype(t)::L, C = decltype(t)::C;
        long long blocks = (n + (256 / L) - 1) / (256 / L);
        if (blocks > 8192) blocks = 8192;
        hipLaunchKernelGGL((predict_bf16_kernel<L, C>), dim3((unsigned)blocks), dim3(256), 0, stream, d_ent, d_rel, d_h, d_t, d_r, (int)m.ent_dim,
                           (long long)n, d_out);
    });
    if (!shaped) return fail(KGE_ERR_UNSUPPORTED, "kge_predict_bf16: embedding dimension > 1024");
    return hip_check(hipGetLastError(), "bf16 predict launch");
}

}  // namespace kge

using namespace kge;

extern "C" {

int kge_bf16_eval_supported(const kge_model_desc *m) { return bf16_eval_refusal(m) ? 0 : 1; }

int kge_predict_bf16(const kge_model_desc *m, const uint16_t *d_ent, const uint16_t *d_rel, const int32_t *d_h, const int32_t *d_t,
                     const int32_t *d_r, INT n, float *d_out, void *stream) {
    if (!m || !d_ent || !d_rel || !d_out) return fail(KGE_ERR_BAD_ARG, "kge_predict_bf16: null argument");
    if (const char *why = bf16_eval_refusal(m)) return fail(KGE_ERR_UNSUPPORTED, std::string("kge_predict_bf16: ") + why);
    return launch_predict_bf16(*m, d_ent, d_rel, d_h, d_t, d_r, n, d_out, (hipStream_t)stream);
}

}  // extern "C"
