// Relation prediction on the device: the k best relations of (h, ?, t) for many queries (kge_topk_relations) and the rank of
// the true relation of every test triple, raw / filtered / typed / filtered + typed (kge_relation_prediction).
//
// Stage 1 scores a chunk of queries against every relation into a [chunk x R] fp32 block (at most "relpred_chunk_bytes").
//  - TransE / TransH / TransD (relpred_score_kernel): a workgroup copies the raw h / t rows of up to 32 queries (TransD: also
//    their transfer rows; TransE: the normalised rows) into LDS once; each team of L lanes walks relations, forms the
//    relation context once (ctx_forward) and scores it against every query of the block with predict_kernel's own functions
//    (side_project, l1_score), so a relation row is read once per query block.  The scores are kge_predict's up to the
//    contraction of products the compiler chooses in each inlining context (topk.hip's header).
//  - TransR: the projections l2n(M_r e) are formed once per DISTINCT entity of the chunk, not once per query slot.  The chunk's
//    entities are deduplicated on the device (relpred_dedup_kernel: a slot map over all entities, kept at -1 between calls),
//    then for each block of relations relpred_project_kernel multiplies the distinct rows by each M_r on the exact-fp32 MFMA
//    (v_mfma_f32_16x16x4_f32: a k-ordered fma chain per element, so a row's projection does not depend on its neighbours or
//    its slot), relpred_norm_kernel normalises them and relpred_score_transr_kernel scores the queries against l2n(rel[r]).
//    The buffer holds (distinct entities) x Dr x (relations per block).  Each relation uses its OWN matrix; kge_predict
//    differs from these scores only in its projection's summation order.  Nothing here touches transr.hip's training workspace.
// Stage 2 works on each query's row of R scores, one workgroup per query:
//  - relpred_topk_kernel: the k smallest (score, id) keys (select_dev.hpp: kge_topk_entities' packing and LDS buffers) of the
//    eligible relations -- not forming a known triple (h, r', t) (KGE_TOPK_FILTERED: a search in the (h,t,r)-sorted union) and
//    / or having h in r''s head and t in r''s tail type list (KGE_TOPK_TYPED) -- padded with id -1 / score +inf.
//  - relpred_rank_kernel: the relations r' != r scoring strictly below the true relation's score (NaN never counts, as in
//    rank_kernel), raw, filtered, typed and filtered + typed.
// No host synchronisation between chunks or relation blocks; kge_relation_prediction copies its counts back once at the end.
// kge_relation_prediction_rows (TransE, a sharded entity table) runs the same two stages on h / t rows the caller supplies and
// leaves its counts on the device.
#include <algorithm>
#include <cstring>
#include <vector>

#include "eval_dev.hpp"
#include "models_dev.hpp"
#include "select_dev.hpp"
#include "team_shape.hpp"

namespace kge {

namespace {

constexpr int kQueriesPerBlock = 32;            // queries per workgroup of the vector-model score kernel (LDS permitting)
constexpr int kScoreLdsBytes = 48 << 10;        // their rows in LDS
constexpr int kTransrQueries = 16;              // queries per workgroup of the TransR score kernel
constexpr int kProjTile = 64;                   // rows x columns of one projection workgroup
constexpr int kProjK = 16;                      // k per LDS stage of the projection

struct RelScoreArgs {
    FbArgs fa;                    // tables (ent, rel, auxr, auxe) and D (TransR: Dr)
    const int32_t *qh, *qt;       // query h / t ids: element i at qh[i * qs]
    int qs;
    long long n, R, E;
    int qn;                       // queries per workgroup
    float *S;                     // [n][R] scores
    // TransR
    const float *P;               // [rb][ucap][Dr] l2n(M_r e) of the distinct entities
    const int32_t *uh, *ut;       // [n] slot of h / t among the distinct entities (-1: id out of range)
    long long ucap;
    int r0, rb;                   // relation block [r0, r0 + rb)
};

__device__ __forceinline__ bool ent_ok(int e, long long E) { return e >= 0 && e < E; }

template <int MODEL, int L, int C>
__global__ __launch_bounds__(256) void relpred_score_kernel(RelScoreArgs a) {
    constexpr int TEAMS = 256 / L;
    constexpr int NV = MODEL == KGE_TRANSD ? 4 : 2;   // LDS rows per query: h, t (+ h_p, t_p)
    extern __shared__ float s_rows[];                   // [qn][NV][D]
    __shared__ int s_ok[kQueriesPerBlock];
    Team<L, C> tm;
    tm.lane = threadIdx.x % L;
    tm.D = a.fa.D;
    const int D = a.fa.D;
    const int team = threadIdx.x / L;
    const long long q0 = (long long)blockIdx.x * a.qn;
    const int nb = (int)min((long long)a.qn, a.n - q0);
    float zero[C];
#pragma unroll
    for (int c = 0; c < C; c++) zero[c] = 0.f;
    for (int q = team; q < nb; q += TEAMS) {
        const int h = a.qh[(q0 + q) * a.qs], t = a.qt[(q0 + q) * a.qs];
        const bool ok = ent_ok(h, a.E) && ent_ok(t, a.E);
        if (tm.lane == 0) s_ok[q] = ok;
        if (!ok) continue;
        float *rows = s_rows + (long long)q * NV * D;
        for (int side = 0; side < 2; side++) {
            Side<C> s;
            tm.load(a.fa.ent, side ? t : h, s.raw);
            if constexpr (MODEL == KGE_TRANSE) {
                side_project<MODEL, L, C>(tm, zero, s);   // no relation context: the normalised row, once per query
                tm.store(rows, side, s.nrm);
            } else {
                tm.store(rows, side, s.raw);
            }
            if constexpr (MODEL == KGE_TRANSD) {
                tm.load(a.fa.auxe, side ? t : h, s.aux);
                tm.store(rows, 2 + side, s.aux);
            }
        }
    }
    __syncthreads();
    const float nan = __uint_as_float(0x7FC00000u);
    for (long long r = team; r < a.R; r += TEAMS) {
        Ctx<C> cx;
        ctx_forward<MODEL, L, C>(tm, a.fa, r, cx);
        for (int q = 0; q < nb; q++) {
            float s = nan;
            if (s_ok[q]) {
                const float *rows = s_rows + (long long)q * NV * D;
                float sg[C];
                if constexpr (MODEL == KGE_TRANSE) {
                    float hn[C], tn[C];
                    tm.load(rows, 0, hn);
                    tm.load(rows, 1, tn);
                    s = l1_score<L, C>(tm, hn, cx.rn, tn, sg) / (float)D;
                } else {
                    Side<C> sh, st;
                    tm.load(rows, 0, sh.raw);
                    tm.load(rows, 1, st.raw);
                    if constexpr (MODEL == KGE_TRANSD) {
                        tm.load(rows, 2, sh.aux);
                        tm.load(rows, 3, st.aux);
                    }
                    side_project<MODEL, L, C>(tm, cx.cw, sh);
                    side_project<MODEL, L, C>(tm, cx.cw, st);
                    s = l1_score<L, C>(tm, sh.nrm, cx.rn, st.nrm, sg);
                }
            }
            if (tm.lane == 0) a.S[(q0 + q) * a.R + r] = s;
        }
    }
}

// The distinct entities of the chunk: slot_of[e] = -1 for every e between calls; the first query slot to claim e appends it
// to uent.  Ids out of range are skipped (their queries score NaN).
__global__ void relpred_dedup_kernel(const int32_t *__restrict__ qh, const int32_t *__restrict__ qt, int qs, long long n, long long E,
                                     int32_t *__restrict__ slot_of, int32_t *__restrict__ uent, int32_t *__restrict__ ucount) {
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < 2 * n; i += (long long)gridDim.x * blockDim.x) {
        const int e = (i & 1) ? qt[(i >> 1) * qs] : qh[(i >> 1) * qs];
        if (!ent_ok(e, E)) continue;
        if (atomicCAS(&slot_of[e], -1, -2) == -1) {
            const int u = atomicAdd(ucount, 1);
            uent[u] = e;
            slot_of[e] = u;
        }
    }
}

__global__ void relpred_slots_kernel(const int32_t *__restrict__ qh, const int32_t *__restrict__ qt, int qs, long long n, long long E,
                                     const int32_t *__restrict__ slot_of, int32_t *__restrict__ uh, int32_t *__restrict__ ut) {
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
        const int h = qh[i * qs], t = qt[i * qs];
        const bool ok = ent_ok(h, E) && ent_ok(t, E);
        uh[i] = ok ? slot_of[h] : -1;
        ut[i] = ok ? slot_of[t] : -1;
    }
}

// back to slot_of[e] = -1 for the chunk's entities, and no entity claimed
__global__ void relpred_undedup_kernel(int32_t *__restrict__ slot_of, const int32_t *__restrict__ uent, int32_t *__restrict__ ucount,
                                       long long ucap) {
    const long long nu = *ucount;
    for (long long u = (long long)blockIdx.x * blockDim.x + threadIdx.x; u < ucap; u += (long long)gridDim.x * blockDim.x)
        if (u < nu) slot_of[uent[u]] = -1;
}

typedef float f32x4 __attribute__((ext_vector_type(4)));

// P[rr][u][j] = sum_k ent[uent[u]][k] * M_{r0+rr}[k][j] (TransR.py's matmul(e, M_r)) for a 64 x 64 tile (u, j); each wave
// owns a 32 x 32 quarter as 2 x 2 tiles of v_mfma_f32_16x16x4_f32 (A[i=l&15][k=l>>4], B[k=l>>4][j=l&15], D[4(l>>4)+v][l&15])
__global__ __launch_bounds__(256) void relpred_project_kernel(const float *__restrict__ ent, const float *__restrict__ mat,
                                                              const int32_t *__restrict__ uent, const int32_t *__restrict__ ucount,
                                                              int De, int Dr, int r0, long long ucap, float *__restrict__ P) {
    const int nu = *ucount;
    const int row0 = blockIdx.x * kProjTile;
    if (row0 >= nu) return;
    const int rr = blockIdx.y;
    const int col0 = blockIdx.z * kProjTile;
    __shared__ float As[kProjTile][kProjK + 1];
    __shared__ float Bs[kProjK][kProjTile + 4];
    __shared__ int s_ent[kProjTile];
    const int tid = threadIdx.x;
    if (tid < kProjTile) s_ent[tid] = row0 + tid < nu ? uent[row0 + tid] : -1;
    __syncthreads();
    const float *M = mat + (long long)(r0 + rr) * De * Dr;
    const int wave = tid >> 6, lane = tid & 63;
    const int wr = (wave >> 1) * 32, wc = (wave & 1) * 32;
    f32x4 acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; i++)
#pragma unroll
        for (int j = 0; j < 2; j++) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int k0 = 0; k0 < De; k0 += kProjK) {
        for (int idx = tid; idx < kProjTile * kProjK; idx += 256) {
            const int i = idx / kProjK, kk = idx - i * kProjK, kg = k0 + kk;
            As[i][kk] = (s_ent[i] >= 0 && kg < De) ? ent[(long long)s_ent[i] * De + kg] : 0.f;
        }
        for (int idx = tid; idx < kProjK * kProjTile; idx += 256) {
            const int kk = idx / kProjTile, j = idx - kk * kProjTile, kg = k0 + kk, cg = col0 + j;
            Bs[kk][j] = (kg < De && cg < Dr) ? M[(long long)kg * Dr + cg] : 0.f;
        }
        __syncthreads();
#pragma unroll
        for (int kk = 0; kk < kProjK; kk += 4) {
            float av[2], bv[2];
#pragma unroll
            for (int i = 0; i < 2; i++) av[i] = As[wr + 16 * i + (lane & 15)][kk + (lane >> 4)];
#pragma unroll
            for (int j = 0; j < 2; j++) bv[j] = Bs[kk + (lane >> 4)][wc + 16 * j + (lane & 15)];
#pragma unroll
            for (int i = 0; i < 2; i++)
#pragma unroll
                for (int j = 0; j < 2; j++) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[i], bv[j], acc[i][j], 0, 0, 0);
        }
        __syncthreads();
    }
    float *Pr = P + (long long)rr * ucap * Dr;
#pragma unroll
    for (int i = 0; i < 2; i++)
#pragma unroll
        for (int j = 0; j < 2; j++)
#pragma unroll
            for (int v = 0; v < 4; v++) {
                const int row = row0 + wr + 16 * i + 4 * (lane >> 4) + v, col = col0 + wc + 16 * j + (lane & 15);
                if (row < nu && col < Dr) Pr[(long long)row * Dr + col] = acc[i][j][v];
            }
}

// rows of P normalised in place (side_project's TransR case: tf.nn.l2_normalize of the projected row)
template <int L, int C>
__global__ __launch_bounds__(256) void relpred_norm_kernel(float *__restrict__ P, const int32_t *__restrict__ ucount, long long ucap, int rb, int Dr) {
    constexpr int TEAMS = 256 / L;
    Team<L, C> tm;
    tm.lane = threadIdx.x % L;
    tm.D = Dr;
    const long long nu = *ucount;
    const long long rows = (long long)rb * ucap;
    float zero[C];
#pragma unroll
    for (int c = 0; c < C; c++) zero[c] = 0.f;
    for (long long row = (long long)blockIdx.x * TEAMS + threadIdx.x / L; row < rows; row += (long long)gridDim.x * TEAMS) {
        if (row % ucap >= nu) continue;
        Side<C> s;
        tm.load(P, row, s.raw);
        side_project<KGE_TRANSR, L, C>(tm, zero, s);
        tm.store(P, row, s.nrm);
    }
}

template <int L, int C>
__global__ __launch_bounds__(256) void relpred_score_transr_kernel(RelScoreArgs a) {
    constexpr int TEAMS = 256 / L;
    __shared__ int s_uh[kTransrQueries], s_ut[kTransrQueries];
    Team<L, C> tm;
    tm.lane = threadIdx.x % L;
    tm.D = a.fa.D;
    const int team = threadIdx.x / L;
    const long long q0 = (long long)blockIdx.x * kTransrQueries;
    const int nb = (int)min((long long)kTransrQueries, a.n - q0);
    if ((int)threadIdx.x < nb) { s_uh[threadIdx.x] = a.uh[q0 + threadIdx.x]; s_ut[threadIdx.x] = a.ut[q0 + threadIdx.x]; }
    __syncthreads();
    const float nan = __uint_as_float(0x7FC00000u);
    for (int rr = team; rr < a.rb; rr += TEAMS) {
        const long long r = a.r0 + rr;
        Ctx<C> cx;
        ctx_forward<KGE_TRANSR, L, C>(tm, a.fa, r, cx);
        const float *Pr = a.P + (long long)rr * a.ucap * a.fa.D;
        for (int q = 0; q < nb; q++) {
            float s = nan;
            const int uh = s_uh[q], ut = s_ut[q];
            if (uh >= 0 && ut >= 0) {
                float hn[C], tn[C], sg[C];
                tm.load(Pr, uh, hn);
                tm.load(Pr, ut, tn);
                s = l1_score<L, C>(tm, hn, cx.rn, tn, sg);
            }
            if (tm.lane == 0) a.S[(q0 + q) * a.R + r] = s;
        }
    }
}

struct RelSelectArgs {
    const float *S;               // [n][R] scores of the chunk
    const int32_t *qh, *qt, *qr;  // query ids at stride qs (qr: the true relation, ranks only)
    int qs;
    long long n, R;
    int k, cap, flags;
    EvalFilterView ev;
    int32_t *ids;                 // [n][k] (top-k)
    float *scores;
    long long *counts;            // [n][4] (ranks)
};

// r is eligible for (h, t): known / typed as rank_kernel defines them
__device__ __forceinline__ bool rel_known(const EvalFilterView &ev, long long klo, long long khi, int r) { return in_range(ev.all_ht, klo, khi, r); }
__device__ __forceinline__ bool in_list(const int32_t *types, int lo, int hi, int x) {
    const int end = hi;
    while (lo < hi) { const int mid = (lo + hi) >> 1; if (types[mid] < x) lo = mid + 1; else hi = mid; }
    return lo < end && types[lo] == x;
}
__device__ __forceinline__ bool rel_typed(const EvalFilterView &ev, int h, int t, int r) {
    return in_list(ev.head_type, ev.head_lef[r], ev.head_rig[r], h) && in_list(ev.tail_type, ev.tail_lef[r], ev.tail_rig[r], t);
}

__global__ __launch_bounds__(256) void relpred_topk_kernel(RelSelectArgs a) {
    extern __shared__ uint64_t s_keys[];
    __shared__ uint64_t s_thr[1];
    __shared__ int s_cnt[1];
    __shared__ long long s_known[2];
    const long long q = blockIdx.x;
    const int h = a.qh[q * a.qs], t = a.qt[q * a.qs];
    if (threadIdx.x == 0) {
        s_thr[0] = kNoKey; s_cnt[0] = 0;
        long long lo = 0, hi = 0;
        if (a.flags & KGE_TOPK_FILTERED) pair_range(a.ev.all_ht, a.ev.n_all, h, t, lo, hi);
        s_known[0] = lo; s_known[1] = hi;
    }
    __syncthreads();
    const long long klo = s_known[0], khi = s_known[1];
    const float *row = a.S + q * a.R;
    uint64_t thr = kNoKey;
    for (long long base = 0; base < a.R; base += 256) {
        const long long r = base + threadIdx.x;
        if (r < a.R) {
            const uint64_t key = pack_key(row[r], (int)r);
            if (key < thr && !((a.flags & KGE_TOPK_FILTERED) && rel_known(a.ev, klo, khi, (int)r)) &&
                !((a.flags & KGE_TOPK_TYPED) && !rel_typed(a.ev, h, t, (int)r)))
                s_keys[atomicAdd(&s_cnt[0], 1)] = key;
        }
        __syncthreads();
        const bool need = s_cnt[0] > a.cap - 256;
        __syncthreads();
        if (need) {
            shrink_buffers(s_keys, a.cap, 1, 1u, a.k, s_cnt, s_thr);
            thr = s_thr[0];
        }
    }
    shrink_buffers(s_keys, a.cap, 1, 1u, a.k, s_cnt, s_thr);
    const int cnt = s_cnt[0];
    for (int i = threadIdx.x; i < a.k; i += blockDim.x) {
        int32_t id; float s;
        unpack_key(i < cnt ? s_keys[i] : kNoKey, id, s);
        a.ids[q * a.k + i] = id;
        a.scores[q * a.k + i] = s;
    }
}

__global__ __launch_bounds__(256) void relpred_rank_kernel(RelSelectArgs a) {
    __shared__ long long s_known[2];
    __shared__ long long s_c[4][256];
    const long long q = blockIdx.x;
    const int h = a.qh[q * a.qs], t = a.qt[q * a.qs], rt = a.qr[q * a.qs];
    if (threadIdx.x == 0) {
        long long lo, hi;
        pair_range(a.ev.all_ht, a.ev.n_all, h, t, lo, hi);
        s_known[0] = lo; s_known[1] = hi;
    }
    __syncthreads();
    const long long klo = s_known[0], khi = s_known[1];
    const float *row = a.S + q * a.R;
    const float minimal = rt >= 0 && rt < a.R ? row[rt] : __uint_as_float(0x7FC00000u);
    long long c[4] = {0, 0, 0, 0};
    for (long long r = threadIdx.x; r < a.R; r += 256) {
        if (r == rt || !(row[r] < minimal)) continue;
        const bool known = rel_known(a.ev, klo, khi, (int)r);
        const bool typed = rel_typed(a.ev, h, t, (int)r);
        c[0]++;
        if (!known) c[1]++;
        if (typed) { c[2]++; if (!known) c[3]++; }
    }
    for (int i = 0; i < 4; i++) s_c[i][threadIdx.x] = c[i];
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w)
            for (int i = 0; i < 4; i++) s_c[i][threadIdx.x] += s_c[i][threadIdx.x + w];
        __syncthreads();
    }
    if (threadIdx.x < 4) a.counts[q * 4 + threadIdx.x] = s_c[threadIdx.x][0];
}

unsigned pow2_at_least(unsigned x) { unsigned p = 1; while (p < x) p <<= 1; return p; }

// workspace of the calls, grown on demand
DevBuf<float> g_S, g_P;
DevBuf<int32_t> g_slot;        // [E] -1 between calls
DevBuf<int32_t> g_uent;        // [ucap] distinct entities, then [1] their count, then [2][chunk] query slots
DevBuf<long long> g_counts;
DevBuf<int32_t> g_qslot;       // [cap] = 0, 1, ..., cap-1: the query slots of kge_relation_prediction_rows' chunk rows

__global__ void relpred_iota_kernel(int32_t *__restrict__ out, long long n) {
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) out[i] = (int32_t)i;
}

template <int MODEL, int L, int C>
int launch_score_t(RelScoreArgs a, hipStream_t stream) {
    constexpr int NV = MODEL == KGE_TRANSD ? 4 : 2;
    a.qn = std::max(1, std::min(kQueriesPerBlock, kScoreLdsBytes / (NV * a.fa.D * (int)sizeof(float))));
    const long long blocks = (a.n + a.qn - 1) / a.qn;
    hipLaunchKernelGGL((relpred_score_kernel<MODEL, L, C>), dim3((unsigned)blocks), dim3(256), (size_t)a.qn * NV * a.fa.D * sizeof(float), stream, a);
    return hip_check(hipGetLastError(), "relation score launch");
}

template <int MODEL>
int launch_score_m(const RelScoreArgs &a, hipStream_t stream) {
    int rc = KGE_OK;
    const bool shaped = for_team_shape(a.fa.D, [&](auto t) { rc = launch_score_t<MODEL, decltype(t)::L, decltype(t)::C>(a, stream); });
    return shaped ? rc : fail(KGE_ERR_UNSUPPORTED, "relation prediction: embedding dimension > 1024");
}

template <int L, int C>
int launch_transr_t(const RelScoreArgs &a, hipStream_t stream) {
    long long rows = (long long)a.rb * a.ucap;
    long long nblocks = std::min<long long>((rows + (256 / L) - 1) / (256 / L), 8192);
    hipLaunchKernelGGL((relpred_norm_kernel<L, C>), dim3((unsigned)nblocks), dim3(256), 0, stream, const_cast<float *>(a.P),
                       g_uent + a.ucap, a.ucap, a.rb, a.fa.D);
    hipLaunchKernelGGL((relpred_score_transr_kernel<L, C>), dim3((unsigned)((a.n + kTransrQueries - 1) / kTransrQueries)), dim3(256), 0,
                       stream, a);
    return hip_check(hipGetLastError(), "relation score launch");
}

int launch_transr_stage(const RelScoreArgs &a, hipStream_t stream) {
    int rc = KGE_OK;
    const bool shaped = for_team_shape(a.fa.D, [&](auto t) { rc = launch_transr_t<decltype(t)::L, decltype(t)::C>(a, stream); });
    return shaped ? rc : fail(KGE_ERR_UNSUPPORTED, "relation prediction: relation dimension > 1024");
}

// scores of queries [0, n) of the chunk into g_S
int score_chunk(const kge_model_desc &m, const float *const tables[KGE_MAX_TABLES], const int32_t *qh, const int32_t *qt, int qs,
                int64_t n, hipStream_t stream) {
    RelScoreArgs a = {};
    a.fa.ent = tables[0]; a.fa.rel = tables[1]; a.fa.auxr = tables[2]; a.fa.auxe = tables[3];
    a.fa.D = m.model == KGE_TRANSR ? (int)m.rel_dim : (int)m.ent_dim;
    a.qh = qh; a.qt = qt; a.qs = qs;
    a.n = n; a.R = m.rel_total; a.E = m.ent_total;
    a.S = g_S;
    switch (m.model) {
        case KGE_TRANSE: return launch_score_m<KGE_TRANSE>(a, stream);
        case KGE_TRANSH: return launch_score_m<KGE_TRANSH>(a, stream);
        case KGE_TRANSD: return launch_score_m<KGE_TRANSD>(a, stream);
        case KGE_TRANSR: break;
        default: return fail(KGE_ERR_BAD_ARG, "unknown model id");
    }
    const int De = (int)m.ent_dim, Dr = (int)m.rel_dim;
    const int64_t R = m.rel_total, E = m.ent_total;
    const int64_t ucap = std::min<int64_t>(2 * n, E);
    int32_t *ucount = g_uent + ucap, *uh = ucount + 1, *ut = uh + n;
    int rc;
    if ((rc = hip_check(hipMemsetAsync(ucount, 0, sizeof(int32_t), stream), "clear distinct entities"))) return rc;
    unsigned blocks = (unsigned)std::min<int64_t>((2 * n + 255) / 256, 4096);
    hipLaunchKernelGGL(relpred_dedup_kernel, dim3(blocks), dim3(256), 0, stream, qh, qt, qs, (long long)n, (long long)E, g_slot, g_uent, ucount);
    hipLaunchKernelGGL(relpred_slots_kernel, dim3(blocks), dim3(256), 0, stream, qh, qt, qs, (long long)n, (long long)E, g_slot, uh, ut);
    blocks = (unsigned)std::min<int64_t>((ucap + 255) / 256, 4096);
    hipLaunchKernelGGL(relpred_undedup_kernel, dim3(blocks), dim3(256), 0, stream, g_slot, g_uent, ucount, (long long)ucap);
    if ((rc = hip_check(hipGetLastError(), "relation dedup launch"))) return rc;
    const int64_t per_rel = ucap * Dr;
    const int64_t rb_max = std::max<int64_t>(1, std::min<int64_t>(R, g_P.cap() / per_rel));
    a.P = g_P; a.uh = uh; a.ut = ut; a.ucap = ucap;
    for (int64_t r0 = 0; r0 < R; r0 += rb_max) {
        const int rb = (int)std::min<int64_t>(rb_max, R - r0);
        dim3 grid((unsigned)((ucap + kProjTile - 1) / kProjTile), (unsigned)rb, (unsigned)((Dr + kProjTile - 1) / kProjTile));
        hipLaunchKernelGGL(relpred_project_kernel, grid, dim3(256), 0, stream, tables[0], tables[2], g_uent, ucount, De, Dr, (int)r0,
                           (long long)ucap, g_P);
        a.r0 = (int)r0; a.rb = rb;
        if ((rc = launch_transr_stage(a, stream))) return rc;
    }
    return KGE_OK;
}

// shared front of both entry points: queries per chunk and the workspace
int prepare(const kge_model_desc &m, int64_t n, int64_t &chunk) {
    const int64_t R = m.rel_total, E = m.ent_total;
    const int D = m.model == KGE_TRANSR ? (int)m.rel_dim : (int)m.ent_dim;
    if (D < 1 || D > 1024) return fail(KGE_ERR_UNSUPPORTED, "relation prediction: the vector-model kernels take dimensions 1..1024");
    const int64_t budget = std::max<int64_t>(engine().relpred_chunk_bytes, 1);
    chunk = std::max<int64_t>(1, std::min<int64_t>(n, budget / (R * (int64_t)sizeof(float))));
    int rc;
    if ((rc = g_S.reserve(chunk * R, "alloc relation scores"))) return rc;
    if (m.model == KGE_TRANSR) {
        const int64_t ucap = std::min<int64_t>(2 * chunk, E);
        if ((rc = g_uent.reserve(ucap + 1 + 2 * chunk, "alloc distinct entities"))) return rc;
        bool grew;
        if ((rc = g_slot.reserve(E, "alloc entity slot map", &grew))) return rc;
        if (grew && (rc = hip_check(hipMemset(g_slot, 0xFF, sizeof(int32_t) * (size_t)E), "clear entity slot map"))) { g_slot.free(); return rc; }
        // projections of at least one relation, else of as many as fit the chunk budget
        const int64_t per_rel = ucap * m.rel_dim;
        const int64_t want = per_rel * std::max<int64_t>(1, std::min<int64_t>(R, budget / (per_rel * (int64_t)sizeof(float))));
        if (g_P.cap() > 2 * want) g_P.free();   // the one shrink rule: a chunk budget that fell leaves no oversized buffer behind
        if ((rc = g_P.reserve(want, "alloc relation projections"))) return rc;
    }
    return KGE_OK;
}

int check_model(const kge_model_desc *m, const float *const tables[KGE_MAX_TABLES], const char *who) {
    if (!m || !tables) return fail(KGE_ERR_BAD_ARG, std::string(who) + ": null model or tables");
    if (m->model != KGE_TRANSE && m->model != KGE_TRANSH && m->model != KGE_TRANSD && m->model != KGE_TRANSR)
        return fail(KGE_ERR_BAD_ARG, "unknown model id");
    if (m->ent_total < 1 || m->rel_total < 1) return fail(KGE_ERR_BAD_ARG, std::string(who) + ": empty model");
    const int64_t D = m->model == KGE_TRANSR ? m->rel_dim : m->ent_dim;
    if (D < 1 || D > 1024 || m->ent_dim < 1) return fail(KGE_ERR_UNSUPPORTED, std::string(who) + ": the vector-model kernels take dimensions 1..1024");
    if (!device_ok()) return fail(KGE_ERR_NO_DEVICE, std::string(who) + ": no usable HIP device");
    return KGE_OK;
}

}  // namespace

}  // namespace kge

using namespace kge;

extern "C" int kge_topk_relations(const kge_model_desc *m, const float *const tables[KGE_MAX_TABLES], const int32_t *d_h,
                                  const int32_t *d_t, INT n, INT k, INT flags, int32_t *d_ids, float *d_scores, void *stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (k < 1 || k > 1024) return fail(KGE_ERR_BAD_ARG, "kge_topk_relations: k must be in [1, 1024]");
    if (flags & ~(INT)(KGE_TOPK_FILTERED | KGE_TOPK_TYPED)) return fail(KGE_ERR_BAD_ARG, "kge_topk_relations: unknown flags");
    if (n < 0) return fail(KGE_ERR_BAD_ARG, "kge_topk_relations: negative query count");
    int rc = check_model(m, tables, "kge_topk_relations");
    if (rc) return rc;
    RelSelectArgs s = {};
    if (flags && (rc = eval_filter_view((flags & KGE_TOPK_TYPED) != 0, s.ev))) return rc;
    if (n == 0) return KGE_OK;
    if (!d_h || !d_t || !d_ids || !d_scores) return fail(KGE_ERR_BAD_ARG, "kge_topk_relations: null query or output array");
    int64_t chunk;
    if ((rc = prepare(*m, n, chunk))) return rc;
    s.S = g_S; s.qs = 1; s.R = m->rel_total; s.k = (int)k; s.flags = (int)flags;
    s.cap = (int)pow2_at_least((unsigned)(k + 256));
    for (int64_t c0 = 0; c0 < n; c0 += chunk) {
        const int64_t nc = std::min<int64_t>(chunk, n - c0);
        if ((rc = score_chunk(*m, tables, d_h + c0, d_t + c0, 1, nc, stream))) return rc;
        s.qh = d_h + c0; s.qt = d_t + c0; s.n = nc;
        s.ids = d_ids + c0 * k; s.scores = d_scores + c0 * k;
        hipLaunchKernelGGL(relpred_topk_kernel, dim3((unsigned)nc), dim3(256), (size_t)s.cap * sizeof(uint64_t), stream, s);
        if ((rc = hip_check(hipGetLastError(), "relation top-k launch"))) return rc;
    }
    return KGE_OK;
}

extern "C" int kge_relation_prediction(const kge_model_desc *m, const float *const tables[KGE_MAX_TABLES], INT first, INT count,
                                       int64_t *h_out, void *stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    int rc = check_model(m, tables, "kge_relation_prediction");
    if (rc) return rc;
    RelSelectArgs s = {};
    if ((rc = eval_filter_view(false, s.ev))) return rc;
    const int4 *test;
    int64_t total;
    if ((rc = eval_test_view(test, total))) return rc;
    if (!h_out || first < 0 || count < 0 || first + count > total) return fail(KGE_ERR_BAD_ARG, "kge_relation_prediction: bad range");
    if (count == 0) return KGE_OK;
    int64_t chunk;
    if ((rc = prepare(*m, count, chunk))) return rc;
    if ((rc = g_counts.reserve(4 * count, "alloc relation ranks"))) return rc;
    const int32_t *base = reinterpret_cast<const int32_t *>(test + first);   // (h, t, r, 0)
    s.S = g_S; s.qs = 4; s.R = m->rel_total;
    for (int64_t c0 = 0; c0 < count; c0 += chunk) {
        const int64_t nc = std::min<int64_t>(chunk, count - c0);
        const int32_t *qh = base + 4 * c0;
        if ((rc = score_chunk(*m, tables, qh, qh + 1, 4, nc, stream))) return rc;
        s.qh = qh; s.qt = qh + 1; s.qr = qh + 2; s.n = nc;
        s.counts = g_counts + 4 * c0;
        hipLaunchKernelGGL(relpred_rank_kernel, dim3((unsigned)nc), dim3(256), 0, stream, s);
        if ((rc = hip_check(hipGetLastError(), "relation rank launch"))) return rc;
    }
    if ((rc = hip_check(hipMemcpyAsync(h_out, g_counts, sizeof(int64_t) * 4 * (size_t)count, hipMemcpyDeviceToHost, stream), "copy relation ranks"))) return rc;
    return hip_check(hipStreamSynchronize(stream), "relation rank sync");
}

// kge_relation_prediction with the h / t rows supplied by the caller (a sharded entity table).  Each chunk's 2 * nc rows are
// scored as an entity table of their own -- a descriptor with ent_total = 2 * nc, tables[0] = the chunk's rows, query ids
// 2i / 2i+1 read from g_qslot at stride 2 -- by the same relpred_score_kernel instantiation on the same row values, so the
// scores, and the counts relpred_rank_kernel forms from them with the test set's global (h, t, r), are kge_relation_prediction's.
extern "C" int kge_relation_prediction_rows(const kge_model_desc *m, const float *const tables[KGE_MAX_TABLES], const float *d_query_rows,
                                            INT first, INT count, int64_t *d_counts, void *stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (!m || !tables) return fail(KGE_ERR_BAD_ARG, "kge_relation_prediction_rows: null model or tables");
    if (m->model != KGE_TRANSE) return fail(KGE_ERR_UNSUPPORTED, "kge_relation_prediction_rows: TransE only");
    if (m->ent_dim < 1 || m->ent_dim > 1024) return fail(KGE_ERR_UNSUPPORTED, "kge_relation_prediction_rows: embedding dimension must be in [1, 1024]");
    if (m->rel_total < 1) return fail(KGE_ERR_BAD_ARG, "kge_relation_prediction_rows: empty model");
    if (!device_ok()) return fail(KGE_ERR_NO_DEVICE, "kge_relation_prediction_rows: no usable HIP device");
    RelSelectArgs s = {};
    int rc = eval_filter_view(false, s.ev);
    if (rc) return rc;
    const int4 *test;
    int64_t total;
    if ((rc = eval_test_view(test, total))) return rc;
    if (first < 0 || count < 0 || first + count > total) return fail(KGE_ERR_BAD_ARG, "kge_relation_prediction_rows: bad range");
    if (count == 0) return KGE_OK;
    if (!d_query_rows || !d_counts || !tables[1]) return fail(KGE_ERR_BAD_ARG, "kge_relation_prediction_rows: null relation table, query or output array");
    int64_t chunk;
    if ((rc = prepare(*m, count, chunk))) return rc;
    bool grew;
    if ((rc = g_qslot.reserve(2 * chunk, "alloc relation query slots", &grew))) return rc;
    if (grew) {
        hipLaunchKernelGGL(relpred_iota_kernel, dim3((unsigned)std::min<int64_t>((g_qslot.cap() + 255) / 256, 4096)), dim3(256), 0, stream,
                           g_qslot, (long long)g_qslot.cap());
        if ((rc = hip_check(hipGetLastError(), "relation query slots launch"))) return rc;
    }
    const int64_t D = m->ent_dim;
    kge_model_desc mc = *m;
    const float *tabs[KGE_MAX_TABLES];
    for (int i = 0; i < KGE_MAX_TABLES; i++) tabs[i] = tables[i];
    const int32_t *base = reinterpret_cast<const int32_t *>(test + first);   // (h, t, r, 0)
    s.S = g_S; s.qs = 4; s.R = m->rel_total;
    for (int64_t c0 = 0; c0 < count; c0 += chunk) {
        const int64_t nc = std::min<int64_t>(chunk, count - c0);
        mc.ent_total = 2 * nc;
        tabs[0] = d_query_rows + 2 * c0 * D;
        if ((rc = score_chunk(mc, tabs, g_qslot, g_qslot + 1, 2, nc, stream))) return rc;
        const int32_t *qh = base + 4 * c0;
        s.qh = qh; s.qt = qh + 1; s.qr = qh + 2; s.n = nc;
        s.counts = (long long *)d_counts + 4 * c0;
        hipLaunchKernelGGL(relpred_rank_kernel, dim3((unsigned)nc), dim3(256), 0, stream, s);
        if ((rc = hip_check(hipGetLastError(), "relation rank launch"))) return rc;
    }
    return KGE_OK;
}
