// Batched top-k entity prediction (kge_topk_entities): the k best tails of (h, r, ?) / heads of (?, r, t) for many queries,
// scored and selected on the device without forming the [queries x E] score matrix of kge_link_prediction.
//
// Stage 1 (topk_select_kernel), grid (query block x candidate slice): a workgroup holds Q queries, each team of L lanes keeps
// the queries' fixed-side vectors in registers (lane l: elements l, l+L, ...), loads U candidate rows at a time -- from the
// candidate table T_r (models.hip lp_table_kernel) or computed on the fly with side_forward -- and scores every row against
// all Q queries, so a candidate byte is read once per workgroup, not once per query.  The score is kge_predict's up to the
// contraction of its products: predict_kernel leaves (hn + rn) - tn to the compiler (at D = 16 it fuses the relation's
// product, not the head's).  Here it is written out as fma(-xt, inv_t, fma(xh, inv_h, rn)) over the projected rows x and
// lane 0's 1/|x|, then per-lane sums over c and lane 0's team_sum<L> (the lane predict_kernel reports).  The table holds
// projected rows and inverse norms, so the table and on-the-fly paths give the same bits.
// Each query keeps its selection in an LDS buffer of packed 64-bit keys (orderable score bits << 32 | entity id) and a
// threshold, the current k-th key: a candidate at or above it is dropped with one compare; one below it is checked against the
// filter / type list (as rank_kernel counts them) and appended.  A buffer that may not take another round is sorted (bitonic,
// in LDS) back to its k smallest keys and the threshold is raised.  Each (query, slice) leaves k keys.
// Stage 2 (topk_merge_kernel), one workgroup per query: the same buffer logic over the slices' k-lists, then the unpack into
// ids / scores.  With one slice the first stage writes the ids / scores itself.
// Row range (kge_topk_entities_range, TransE; RANGE instantiations): the candidates are the rows of a shard of the table, global
// ids [row_lo, row_lo + rows), and the fixed sides come from the caller's rows, not from the table (their owner may be another
// rank).  The same side_xp, fma chain, team_sum and (L, C) bucket as the whole table, so every candidate's key carries the same
// bits; both stages leave packed keys.  kge_topk_merge_keys takes the k smallest of several sources' key lists and unpacks
// them: keys are unique per query (the id is the low word), so the k smallest of k-smallests over any cut is the whole table's.
// Stored bf16 tables (kge_topk_entities_bf16; TransE, the whole table): the BF16 instantiations of the table and select kernels
// read the entity and relation rows as uint16 and widen them exactly; everything after the load is the fp32 code, so ids and
// score bits are those of kge_topk_entities on the widened tables.  Only the [E] inverse norms and the partial lists are allocated.
#include <algorithm>
#include <cstring>
#include <vector>

#include "eval_dev.hpp"
#include "models_dev.hpp"
#include "select_dev.hpp"
#include "team_shape.hpp"

namespace kge {

namespace {

// The projected (not yet normalised) entity side x of `row` under the relation context cw, as side_project forms it, and
// 1/|x| from Team::normalize -- the two factors of predict_kernel's contracted score.
// BF16 (kge_topk_entities_bf16, TransE): a.ent is the stored bf16 table, cast here where it is read; the row is widened exactly
// in the same lane layout, so everything after the load has the bits it has on the widened table.
template <int MODEL, int L, int C, bool BF16 = false>
__device__ __forceinline__ float side_xp(const Team<L, C> &tm, const FbArgs &a, long long row, const float (&cw)[C], float (&xp)[C]) {
    static_assert(!BF16 || MODEL == KGE_TRANSE, "stored bf16 rows: TransE only");
    float raw[C];
    if constexpr (BF16) tm.load((const uint16_t *)a.ent, row, raw);
    else if constexpr (MODEL == KGE_TRANSR) tm.load(a.P, row, raw);
    else tm.load(a.ent, row, raw);
    if constexpr (MODEL == KGE_TRANSE || MODEL == KGE_TRANSR) {
#pragma unroll
        for (int c = 0; c < C; c++) xp[c] = raw[c];
    } else if constexpr (MODEL == KGE_TRANSH) {
        const float p = tm.dot(raw, cw);
#pragma unroll
        for (int c = 0; c < C; c++) xp[c] = raw[c] - p * cw[c];
    } else {
        float aux[C];
        tm.load(a.auxe, row, aux);
        const float p = tm.dot(raw, aux);
#pragma unroll
        for (int c = 0; c < C; c++) xp[c] = raw[c] + p * cw[c];
    }
    float y[C], inv;
    bool uc;
    tm.normalize(xp, y, inv, uc);
    return __shfl(inv, 0, L);   // lane 0's bits (team_sum may differ per lane in the last bit): the table stores the same
}

// candidate table of one relation: projected rows into T (nullptr for TransE / TransR, whose rows are the parameter /
// projection rows themselves) and 1/|row| into inv
// The relation context of a query on stored bf16 tables (a.rel is the bf16 relation table, cast here): ctx_forward's TransE case -- the
// row, Team::normalize, no projection vector -- on the widened row.
template <int L, int C>
__device__ __forceinline__ void ctx_forward_bf16(const Team<L, C> &tm, const FbArgs &a, long long r, Ctx<C> &cx) {
    float raw[C];
    tm.load((const uint16_t *)a.rel, r, raw);
    tm.normalize(raw, cx.rn, cx.inv_r, cx.uc_r);
    cx.inv_w = 1.f; cx.uc_w = true;
#pragma unroll
    for (int c = 0; c < C; c++) cx.cw[c] = 0.f;
}

template <int MODEL, int L, int C, bool BF16 = false>
__global__ __launch_bounds__(256) void topk_table_kernel(FbArgs a, long long r, long long E, float *__restrict__ T, float *__restrict__ inv) {
    constexpr int TEAMS = 256 / L;
    Team<L, C> tm;
    tm.lane = threadIdx.x % L;
    tm.D = a.D;
    Ctx<C> cx;
    if constexpr (BF16) {   // TransE has no projection vector, and the relation table is not read
#pragma unroll
        for (int c = 0; c < C; c++) cx.cw[c] = 0.f;
    } else {
        ctx_forward<MODEL, L, C>(tm, a, r, cx);
    }
    for (long long j = (long long)blockIdx.x * TEAMS + threadIdx.x / L; j < E; j += (long long)gridDim.x * TEAMS) {
        float xp[C];
        const float v = side_xp<MODEL, L, C, BF16>(tm, a, j, cx.cw, xp);
        if (T) tm.store(T, j, xp);
        if (tm.lane == 0) inv[j] = v;
    }
}

struct TopkArgs {
    FbArgs fa;                 // parameter tables (TransR: a.P = all entities projected by the launch's relation), D
    const float *T;            // candidate table [E][D] of projected rows, or nullptr: candidate sides computed on the fly
    const float *Tinv;         // [E] 1/|row| of T
    const int32_t *fixed, *rel, *head;   // the caller's query arrays
    const int32_t *order;      // caller index of launch position p (nullptr: p itself)
    long long nq, E, slice_len;
    int k, cap, qn, flags;     // qn: queries per workgroup (<= the kernel's Q)
    EvalFilterView ev;
    uint64_t *part;            // [nq][slices][k] keys by launch position, or nullptr: write ids / scores directly
    int32_t *ids;
    float *scores;
    long long row_lo;          // RANGE: global id of candidate row 0 (the candidate tables hold rows [row_lo, row_lo + E))
    const float *qrows;        // RANGE: [nq][D] raw rows of the queries' fixed sides
    uint64_t *keys;            // RANGE: [nq][k] keys out (with one slice the first stage writes them as its part)
};

__device__ __forceinline__ void emit_row(const TopkArgs &a, long long p, const uint64_t *b, int cnt) {
    const long long qi = a.order ? a.order[p] : p;
    for (int i = threadIdx.x; i < a.k; i += blockDim.x) {
        int32_t id; float s;
        unpack_key(i < cnt ? b[i] : kNoKey, id, s);
        a.ids[qi * a.k + i] = id;
        a.scores[qi * a.k + i] = s;
    }
}

// Known / typed test of candidate j for the lane's query (rank_kernel's definitions).
__device__ __forceinline__ bool eligible(const TopkArgs &a, bool hd, long long klo, long long khi, int tlo, int thi, int j) {
    if ((a.flags & KGE_TOPK_FILTERED) && in_range(hd ? a.ev.all_t : a.ev.all, klo, khi, j)) return false;
    if (a.flags & KGE_TOPK_TYPED) {
        const int32_t *types = hd ? a.ev.head_type : a.ev.tail_type;
        int lo = tlo, hi = thi;
        while (lo < hi) { const int mid = (lo + hi) >> 1; if (types[mid] < j) lo = mid + 1; else hi = mid; }
        if (!(lo < thi && types[lo] == j)) return false;
    }
    return true;
}

template <int MODEL, int L, int C, int Q, int U, bool DIRECT, bool RANGE, bool BF16 = false>
__global__ __launch_bounds__(256) void topk_select_kernel(TopkArgs a) {
    static_assert(!BF16 || (MODEL == KGE_TRANSE && !RANGE), "stored bf16 rows: TransE over the whole table only");
    constexpr int TEAMS = 256 / L;
    constexpr int ROUND = TEAMS * U;   // candidates per round: the most a buffer can grow between two checks
    extern __shared__ uint64_t s_keys[];
    __shared__ uint64_t s_thr[Q];
    __shared__ int s_cnt[Q];
    __shared__ long long s_klo[Q], s_khi[Q];
    __shared__ int s_tlo[Q], s_thi[Q];
    Team<L, C> tm;
    tm.lane = threadIdx.x % L;
    tm.D = a.fa.D;
    const int team = threadIdx.x / L;
    const long long p0 = (long long)blockIdx.x * a.qn;
    const int nb = (int)min((long long)a.qn, a.nq - p0);
    if ((int)threadIdx.x < Q) {
        const int q = threadIdx.x;
        s_cnt[q] = 0;
        s_thr[q] = q < nb ? kNoKey : 0;   // (an unused slot accepts nothing)
        s_klo[q] = s_khi[q] = 0; s_tlo[q] = s_thi[q] = 0;
        if (q < nb) {
            const long long qi = a.order ? a.order[p0 + q] : p0 + q;
            const int f = a.fixed[qi], r = a.rel[qi];
            const bool hd = a.head[qi] != 0;
            if (a.flags & KGE_TOPK_FILTERED) {
                long long lo, hi;
                if (hd) pair_range(a.ev.all_t, a.ev.n_all, f, r, lo, hi); else pair_range(a.ev.all, a.ev.n_all, f, r, lo, hi);
                s_klo[q] = lo; s_khi[q] = hi;
            }
            if (a.flags & KGE_TOPK_TYPED) {
                s_tlo[q] = hd ? a.ev.head_lef[r] : a.ev.tail_lef[r];
                s_thi[q] = hd ? a.ev.head_rig[r] : a.ev.tail_rig[r];
            }
        }
    }
    // the queries' vectors: tail query A = fma(xh, inv_h, rn) (the score's first operation), head query A = rn, B = xt, binv = inv_t
    float A[Q][C], B[Q][C], binv[Q];
    unsigned hdmask = 0;
    float cw0[C];
#pragma unroll
    for (int c = 0; c < C; c++) cw0[c] = 0.f;
#pragma unroll
    for (int q = 0; q < Q; q++) {
#pragma unroll
        for (int c = 0; c < C; c++) { A[q][c] = 0.f; B[q][c] = 0.f; }
        binv[q] = 0.f;
        if (q < nb) {
            const long long qi = a.order ? a.order[p0 + q] : p0 + q;
            const int f = a.fixed[qi], r = a.rel[qi];
            const bool hd = a.head[qi] != 0;
            Ctx<C> cx;
            if constexpr (BF16) ctx_forward_bf16<L, C>(tm, a.fa, r, cx);
            else ctx_forward<MODEL, L, C>(tm, a.fa, r, cx);
            if (q == 0) {
#pragma unroll
                for (int c = 0; c < C; c++) cw0[c] = cx.cw[c];   // one relation per launch for the projecting models
            }
            float fv[C], finv;
            if constexpr (RANGE) {
                FbArgs qa = a.fa;
                qa.ent = a.qrows;
                finv = side_xp<MODEL, L, C>(tm, qa, qi, cx.cw, fv);
            } else if constexpr (DIRECT) {
                finv = side_xp<MODEL, L, C, BF16>(tm, a.fa, f, cx.cw, fv);
            } else {
                if constexpr (BF16) tm.load((const uint16_t *)a.T, f, fv);   // (TransE: T is the entity table itself)
                else tm.load(a.T, f, fv);
                finv = a.Tinv[f];
            }
            if (hd) {
                hdmask |= 1u << q;
                binv[q] = finv;
#pragma unroll
                for (int c = 0; c < C; c++) { A[q][c] = cx.rn[c]; B[q][c] = fv[c]; }
            } else {
#pragma unroll
                for (int c = 0; c < C; c++) A[q][c] = __builtin_fmaf(fv[c], finv, cx.rn[c]);
            }
        }
    }
    __syncthreads();
    // lane 0 of each team selects for all queries: team_sum's rotations leave lane 0 (the lane predict_kernel reports)
    // with its own association of the partial sums, the other lanes of a 16-lane row may differ in the last bit
    uint64_t thr[Q];
#pragma unroll
    for (int q = 0; q < Q; q++) thr[q] = s_thr[q];
    const long long j0 = (long long)blockIdx.y * a.slice_len;
    const long long j1 = min(a.E, j0 + a.slice_len);
    const float dim = (float)a.fa.D;
    for (long long base = j0; base < j1; base += ROUND) {
#pragma unroll
        for (int u = 0; u < U; u++) {
            const long long j = base + (long long)team * U + u;
            float x[C], xinv = 0.f;
            if (j < j1) {
                if constexpr (DIRECT) {
                    xinv = side_xp<MODEL, L, C, BF16>(tm, a.fa, j, cw0, x);
                } else {
                    if constexpr (BF16) tm.load((const uint16_t *)a.T, j, x);
                    else tm.load(a.T, j, x);
                    xinv = a.Tinv[j];
                }
            } else {
#pragma unroll
                for (int c = 0; c < C; c++) x[c] = 0.f;
            }
#pragma unroll
            for (int q = 0; q < Q; q++) {
                if (q < nb) {
                    float s = 0.f;
                    const bool hd = (hdmask >> q) & 1u;
                    if (hd) {
#pragma unroll
                        for (int c = 0; c < C; c++) { const float e = __builtin_fmaf(-B[q][c], binv[q], __builtin_fmaf(x[c], xinv, A[q][c])); s += fabsf(e); }
                    } else {
#pragma unroll
                        for (int c = 0; c < C; c++) { const float e = __builtin_fmaf(-x[c], xinv, A[q][c]); s += fabsf(e); }
                    }
                    s = team_sum<L>(s);
                    if (tm.lane == 0 && j < j1) {
                        const int id = (int)(RANGE ? a.row_lo + j : j);
                        const uint64_t key = pack_key(MODEL == KGE_TRANSE ? s / dim : s, id);
                        if (key < thr[q] && eligible(a, hd, s_klo[q], s_khi[q], s_tlo[q], s_thi[q], id))
                            s_keys[(long long)q * a.cap + atomicAdd(&s_cnt[q], 1)] = key;
                    }
                }
            }
        }
        __syncthreads();
        unsigned need = 0;
        for (int q = 0; q < nb; q++) if (s_cnt[q] > a.cap - ROUND) need |= 1u << q;
        __syncthreads();   // every thread has read the counts before the next round adds to them
        if (need) {
            shrink_buffers(s_keys, a.cap, nb, need, a.k, s_cnt, s_thr);
#pragma unroll
            for (int q = 0; q < Q; q++) thr[q] = s_thr[q];
        }
    }
    shrink_buffers(s_keys, a.cap, nb, (1u << nb) - 1u, a.k, s_cnt, s_thr);
    for (int q = 0; q < nb; q++) {
        const uint64_t *b = s_keys + (long long)q * a.cap;
        const int cnt = s_cnt[q];
        if (RANGE || a.part) {
            uint64_t *o = a.part + ((p0 + q) * gridDim.y + blockIdx.y) * (long long)a.k;
            for (int i = threadIdx.x; i < a.k; i += blockDim.x) o[i] = i < cnt ? b[i] : kNoKey;
        } else {
            emit_row(a, p0 + q, b, cnt);
        }
    }
}

// one workgroup per query: the k smallest of its `slices` k-lists, [nq][slices][k] (stage 1's partial lists) or, IN_PARTS,
// [slices][nq][k] (kge_topk_merge_keys: one list per source); unpacked into ids / scores or, OUT_KEYS, written as keys
template <bool IN_PARTS, bool OUT_KEYS>
__global__ __launch_bounds__(256) void topk_merge_kernel(TopkArgs a, int slices) {
    extern __shared__ uint64_t s_keys[];
    __shared__ uint64_t s_thr[1];
    __shared__ int s_cnt[1];
    const long long p = blockIdx.x;
    if (threadIdx.x == 0) { s_thr[0] = kNoKey; s_cnt[0] = 0; }
    __syncthreads();
    const uint64_t *in = a.part + p * (long long)(IN_PARTS ? 1 : slices) * a.k;
    const long long total = (long long)slices * a.k;
    uint64_t thr = kNoKey;
    for (long long base = 0; base < total; base += 256) {
        const long long i = base + threadIdx.x;
        if (i < total) {
            const uint64_t key = IN_PARTS ? in[(i / a.k) * a.nq * a.k + i % a.k] : in[i];
            if (key < thr) s_keys[atomicAdd(&s_cnt[0], 1)] = key;
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
    if constexpr (OUT_KEYS) {
        for (int i = threadIdx.x; i < a.k; i += blockDim.x) a.keys[p * a.k + i] = i < s_cnt[0] ? s_keys[i] : kNoKey;
    } else {
        emit_row(a, p, s_keys, s_cnt[0]);
    }
}

unsigned pow2_at_least(unsigned x) { unsigned p = 1; while (p < x) p <<= 1; return p; }

// workspace of the calls, grown on demand
DevBuf<float> g_T, g_P, g_inv;
DevBuf<uint64_t> g_part;
DevBuf<int32_t> g_order;
std::vector<int32_t> g_order_host;   // source of the last order upload: rewritten only once g_order_done has passed
hipEvent_t g_order_done = nullptr;

int launch_table(int model, const FbArgs &a, int64_t r, int64_t E, float *T, float *inv, hipStream_t stream) {
    bool shaped = false;
    const bool known = for_model(model, [&](auto mt) {
        shaped = for_team_shape(a.D, [&](auto t) {
            constexpr int L = decltype(t)::L, C = decltype(t)::C;
            long long blocks = (E + (256 / L) - 1) / (256 / L);
            if (blocks > 4096) blocks = 4096;
            hipLaunchKernelGGL((topk_table_kernel<decltype(mt)::MODEL, L, C>), dim3((unsigned)blocks), dim3(256), 0, stream, a, (long long)r, (long long)E, T, inv);
        });
    });
    if (!known) return fail(KGE_ERR_BAD_ARG, "unknown model id");
    if (!shaped) return fail(KGE_ERR_UNSUPPORTED, "kge_topk_entities: embedding dimension > 1024");
    return hip_check(hipGetLastError(), "top-k table launch");
}

// 1/|row| of every row of a stored bf16 entity table (a.ent cast by the kernel) into inv
int launch_table_bf16(const FbArgs &a, int64_t E, float *inv, hipStream_t stream) {
    const bool shaped = for_team_shape(a.D, [&](auto t) {
        constexpr int L = decltype(t)::L, C = decltype(t)::C;
        long long blocks = (E + (256 / L) - 1) / (256 / L);
        if (blocks > 4096) blocks = 4096;
        hipLaunchKernelGGL((topk_table_kernel<KGE_TRANSE, L, C, true>), dim3((unsigned)blocks), dim3(256), 0, stream, a, 0LL, (long long)E, (float *)nullptr, inv);
    });
    if (!shaped) return fail(KGE_ERR_UNSUPPORTED, "kge_topk_entities_bf16: embedding dimension > 1024");
    return hip_check(hipGetLastError(), "top-k bf16 table launch");
}

constexpr int kSelectLdsBytes = 48 << 10;   // key buffers of one workgroup: two workgroups of 4 waves per CU

template <int MODEL, int L, int C, int Q, int U, bool DIRECT, bool RANGE, bool BF16 = false>
int launch_select_t(TopkArgs a, hipStream_t stream) {
    const int KP = (int)pow2_at_least((unsigned)std::max(a.k, 64));
    a.cap = 2 * KP;   // >= k + ROUND (ROUND <= 64)
    a.qn = std::max(1, std::min(Q, kSelectLdsBytes / (a.cap * 8)));
    const long long qblocks = (a.nq + a.qn - 1) / a.qn;
    // slices: enough workgroups for 256 CUs (two each), slices of at least 512 candidates
    long long slices = (512 + qblocks - 1) / qblocks;
    slices = std::max(1LL, std::min(slices, a.E / 512));
    a.slice_len = (a.E + slices - 1) / slices;
    slices = (a.E + a.slice_len - 1) / a.slice_len;
    int rc;
    if (slices > 1) {
        if ((rc = g_part.reserve(a.nq * slices * a.k, "alloc top-k partial lists"))) return rc;
        a.part = g_part;
    } else {
        a.part = RANGE ? a.keys : nullptr;
    }
    const size_t lds = (size_t)a.qn * a.cap * sizeof(uint64_t);
    if constexpr (BF16) hipLaunchKernelGGL((topk_select_kernel<MODEL, L, C, Q, U, DIRECT, RANGE, true>), dim3((unsigned)qblocks, (unsigned)slices), dim3(256), lds, stream, a);
    else hipLaunchKernelGGL((topk_select_kernel<MODEL, L, C, Q, U, DIRECT, RANGE>), dim3((unsigned)qblocks, (unsigned)slices), dim3(256), lds, stream, a);
    if ((rc = hip_check(hipGetLastError(), "top-k select launch"))) return rc;
    if (slices > 1) {
        a.cap = (int)pow2_at_least((unsigned)(a.k + 256));
        a.cap = std::max(a.cap, 2 * KP);
        hipLaunchKernelGGL((topk_merge_kernel<false, RANGE>), dim3((unsigned)a.nq), dim3(256), (size_t)a.cap * sizeof(uint64_t), stream, a, (int)slices);
        if ((rc = hip_check(hipGetLastError(), "top-k merge launch"))) return rc;
    }
    return KGE_OK;
}

// Q queries per workgroup and U rows per team so that the query vectors (2 Q C floats) and the rows in flight (U C) stay in
// registers: (16, 4) up to C = 4, then (8, 2), then (4, 1)
constexpr int select_q(int C) { return C <= 4 ? 16 : (C <= 8 ? 8 : 4); }
constexpr int select_u(int C) { return C <= 4 ? 4 : (C <= 8 ? 2 : 1); }

template <int MODEL, bool DIRECT, bool RANGE = false, bool BF16 = false>
int launch_select_d(const TopkArgs &a, hipStream_t stream) {
    int rc = KGE_OK;
    const bool shaped = for_team_shape(a.fa.D, [&](auto t) {
        constexpr int L = decltype(t)::L, C = decltype(t)::C;
        rc = launch_select_t<MODEL, L, C, select_q(C), select_u(C), DIRECT, RANGE, BF16>(a, stream);
    });
    return shaped ? rc : fail(KGE_ERR_UNSUPPORTED, "kge_topk_entities: embedding dimension > 1024");
}

int launch_select(int model, bool direct, const TopkArgs &a, hipStream_t stream) {
    int rc = KGE_OK;
    const bool known = for_model(model, [&](auto mt) {
        constexpr int MODEL = decltype(mt)::MODEL;
        rc = direct ? launch_select_d<MODEL, true>(a, stream) : launch_select_d<MODEL, false>(a, stream);
    });
    return known ? rc : fail(KGE_ERR_BAD_ARG, "unknown model id");
}

}  // namespace

}  // namespace kge

using namespace kge;

namespace {

// kge_topk_entities (`tables`) and kge_topk_entities_bf16 (`bf16`: tables == nullptr, d_ent / d_rel_tab are stored bf16 rows): one
// argument path.  The bf16 form allocates the [E] inverse norms (within the table budget) and the partial key lists, nothing else.
int topk_entities_call(const std::string &who, bool bf16, const kge_model_desc *m, const float *const tables[KGE_MAX_TABLES], const uint16_t *d_ent,
                       const uint16_t *d_rel_tab, const int32_t *d_fixed, const int32_t *d_rel, const int32_t *d_head, INT n, INT k, INT flags,
                       int32_t *d_ids, float *d_scores, hipStream_t stream) {
    if (!m || (bf16 ? !d_ent || !d_rel_tab : !tables)) return fail(KGE_ERR_BAD_ARG, who + ": null model or tables");
    if (k < 1 || k > 1024) return fail(KGE_ERR_BAD_ARG, who + ": k must be in [1, 1024]");
    if (flags & ~(INT)(KGE_TOPK_FILTERED | KGE_TOPK_TYPED)) return fail(KGE_ERR_BAD_ARG, who + ": unknown flags");
    if (n < 0) return fail(KGE_ERR_BAD_ARG, who + ": negative query count");
    if (bf16)
        if (const char *why = bf16_eval_refusal(m)) return fail(KGE_ERR_UNSUPPORTED, who + ": " + why);
    if (m->ent_total < 1 || m->rel_total < 1) return fail(KGE_ERR_BAD_ARG, who + ": empty model");
    if (!device_ok()) return fail(KGE_ERR_NO_DEVICE, who + ": no usable HIP device");
    TopkArgs a = {};
    if (flags) {
        int rc = eval_filter_view((flags & KGE_TOPK_TYPED) != 0, a.ev);
        if (rc) return rc;
    }
    if (n == 0) return KGE_OK;
    if (!d_fixed || !d_rel || !d_head || !d_ids || !d_scores) return fail(KGE_ERR_BAD_ARG, who + ": null query or output array");
    const int64_t E = m->ent_total;
    const int D = m->model == KGE_TRANSR ? (int)m->rel_dim : (int)m->ent_dim;
    if (bf16) { a.fa.ent = (const float *)d_ent; a.fa.rel = (const float *)d_rel_tab; }   // (read as uint16 rows by the BF16 instantiations)
    else { a.fa.ent = tables[0]; a.fa.rel = tables[1]; a.fa.auxr = tables[2]; a.fa.auxe = tables[3]; }
    a.fa.D = D;
    a.fixed = d_fixed; a.rel = d_rel; a.head = d_head;
    a.E = E; a.k = (int)k; a.flags = (int)flags;
    a.ids = d_ids; a.scores = d_scores;
    const int64_t budget = engine().topk_table_max_bytes;
    const bool table = budget > 0 && E * D * (int64_t)sizeof(float) <= budget;
    int rc;
    // projected rows are stored for TransH / TransD only: TransE's are the entity rows, TransR's the projection buffer
    const bool own_rows = m->model == KGE_TRANSH || m->model == KGE_TRANSD;
    if (table && own_rows && (rc = g_T.reserve(E * D, "alloc top-k candidate table"))) return rc;
    if (table && (rc = g_inv.reserve(E, "alloc top-k inverse norms"))) return rc;
    if (bf16) {   // TransE on the stored rows: the fp32 form's one launch, the same budget rule (counted in fp32 bytes, as there)
        if (table && (rc = launch_table_bf16(a.fa, E, g_inv, stream))) return rc;
        a.T = table ? a.fa.ent : nullptr;
        a.Tinv = table ? g_inv : nullptr;
        a.order = nullptr; a.nq = n;
        return table ? launch_select_d<KGE_TRANSE, false, false, true>(a, stream) : launch_select_d<KGE_TRANSE, true, false, true>(a, stream);
    }
    if (m->model == KGE_TRANSE) {
        // the candidates do not depend on the relation: all queries in the caller's order, one launch, no synchronisation
        if (table && (rc = launch_table(m->model, a.fa, 0, E, nullptr, g_inv, stream))) return rc;
        a.T = table ? a.fa.ent : nullptr;
        a.Tinv = table ? g_inv : nullptr;
        a.order = nullptr; a.nq = n;
        return launch_select(m->model, !table, a, stream);
    }
    // projecting models: one candidate side per relation -- the queries grouped by relation on the host (one synchronisation)
    std::vector<int32_t> rel((size_t)n);
    if ((rc = hip_check(hipMemcpyAsync(rel.data(), d_rel, sizeof(int32_t) * (size_t)n, hipMemcpyDeviceToHost, stream), "copy query relations"))) return rc;
    if ((rc = hip_check(hipStreamSynchronize(stream), "top-k sync"))) return rc;
    if (g_order_done && (rc = hip_check(hipEventSynchronize(g_order_done), "top-k order upload"))) return rc;
    std::vector<int32_t> &order = g_order_host;
    order.resize((size_t)n);
    for (int64_t i = 0; i < n; i++) order[(size_t)i] = (int32_t)i;
    std::stable_sort(order.begin(), order.end(), [&](int32_t x, int32_t y) { return rel[(size_t)x] < rel[(size_t)y]; });
    if ((rc = g_order.reserve(n, "alloc top-k query order"))) return rc;
    if ((rc = hip_check(hipMemcpyAsync(g_order, order.data(), sizeof(int32_t) * (size_t)n, hipMemcpyHostToDevice, stream), "upload query order"))) return rc;
    if (!g_order_done && (rc = hip_check(hipEventCreateWithFlags(&g_order_done, hipEventDisableTiming), "create top-k event"))) return rc;
    if ((rc = hip_check(hipEventRecord(g_order_done, stream), "record top-k order upload"))) return rc;
    if (m->model == KGE_TRANSR && (rc = g_P.reserve((E + 1) * D, "alloc top-k projections"))) return rc;
    for (int64_t q0 = 0; q0 < n;) {
        const int32_t r = rel[(size_t)order[(size_t)q0]];
        int64_t q1 = q0;
        while (q1 < n && rel[(size_t)order[(size_t)q1]] == r) q1++;
        if (m->model == KGE_TRANSR && (rc = transr_project_all(*m, tables, r, g_P, stream))) return rc;
        a.fa.P = g_P;
        if (table && (rc = launch_table(m->model, a.fa, r, E, own_rows ? g_T : nullptr, g_inv, stream))) return rc;
        a.T = table ? (own_rows ? g_T : g_P) : nullptr;
        a.Tinv = table ? g_inv : nullptr;
        a.order = g_order + q0; a.nq = q1 - q0;
        if ((rc = launch_select(m->model, !table, a, stream))) return rc;
        q0 = q1;
    }
    return KGE_OK;
}

}  // namespace

extern "C" int kge_topk_entities(const kge_model_desc *m, const float *const tables[KGE_MAX_TABLES], const int32_t *d_fixed,
                                 const int32_t *d_rel, const int32_t *d_head, INT n, INT k, INT flags, int32_t *d_ids,
                                 float *d_scores, void *stream) {
    return topk_entities_call("kge_topk_entities", false, m, tables, nullptr, nullptr, d_fixed, d_rel, d_head, n, k, flags, d_ids, d_scores,
                              (hipStream_t)stream);
}

extern "C" int kge_topk_entities_bf16(const kge_model_desc *m, const uint16_t *d_ent, const uint16_t *d_rel_tab, const int32_t *d_fixed,
                                      const int32_t *d_rel, const int32_t *d_head, INT n, INT k, INT flags, int32_t *d_ids,
                                      float *d_scores, void *stream) {
    return topk_entities_call("kge_topk_entities_bf16", true, m, nullptr, d_ent, d_rel_tab, d_fixed, d_rel, d_head, n, k, flags, d_ids, d_scores,
                              (hipStream_t)stream);
}

extern "C" int kge_topk_entities_range(const kge_model_desc *m, const float *const tables[KGE_MAX_TABLES], INT row_lo, INT rows,
                                       const float *d_query_rows, const int32_t *d_fixed, const int32_t *d_rel,
                                       const int32_t *d_head, INT n, INT k, INT flags, uint64_t *d_keys, void *stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (!m || !tables) return fail(KGE_ERR_BAD_ARG, "kge_topk_entities_range: null model or tables");
    if (m->model != KGE_TRANSE) return fail(KGE_ERR_UNSUPPORTED, "kge_topk_entities_range: TransE only");
    if (m->ent_dim < 1 || m->ent_dim > 1024) return fail(KGE_ERR_UNSUPPORTED, "kge_topk_entities_range: embedding dimension must be in [1, 1024]");
    if (k < 1 || k > 1024) return fail(KGE_ERR_BAD_ARG, "kge_topk_entities_range: k must be in [1, 1024]");
    if (flags & ~(INT)(KGE_TOPK_FILTERED | KGE_TOPK_TYPED)) return fail(KGE_ERR_BAD_ARG, "kge_topk_entities_range: unknown flags");
    if (n < 0) return fail(KGE_ERR_BAD_ARG, "kge_topk_entities_range: negative query count");
    if (m->ent_total < 1 || m->rel_total < 1) return fail(KGE_ERR_BAD_ARG, "kge_topk_entities_range: empty model");
    if (row_lo < 0 || rows < 0 || row_lo + rows > m->ent_total) return fail(KGE_ERR_BAD_ARG, "kge_topk_entities_range: row range outside the entity table");
    if (!device_ok()) return fail(KGE_ERR_NO_DEVICE, "kge_topk_entities_range: no usable HIP device");
    TopkArgs a = {};
    if (flags) {
        int rc = eval_filter_view((flags & KGE_TOPK_TYPED) != 0, a.ev);
        if (rc) return rc;
    }
    if (n == 0) return KGE_OK;
    if (!d_fixed || !d_rel || !d_head || !d_query_rows || !d_keys || !tables[1] || (rows > 0 && !tables[0]))
        return fail(KGE_ERR_BAD_ARG, "kge_topk_entities_range: null table, query or output array");
    int rc;
    if (rows == 0)   // an empty shard: nothing to offer, every key padding
        return hip_check(hipMemsetAsync(d_keys, 0xFF, sizeof(uint64_t) * (size_t)(n * k), stream), "top-k range padding");
    const int D = (int)m->ent_dim;
    a.fa.ent = tables[0]; a.fa.rel = tables[1];
    a.fa.D = D;
    a.fixed = d_fixed; a.rel = d_rel; a.head = d_head;
    a.order = nullptr; a.nq = n;
    a.E = rows; a.row_lo = row_lo; a.qrows = d_query_rows; a.keys = d_keys;
    a.k = (int)k; a.flags = (int)flags;
    const int64_t budget = engine().topk_table_max_bytes;
    const bool table = budget > 0 && rows * D * (int64_t)sizeof(float) <= budget;
    if (table) {
        if ((rc = g_inv.reserve(rows, "alloc top-k inverse norms"))) return rc;
        if ((rc = launch_table(KGE_TRANSE, a.fa, 0, rows, nullptr, g_inv, stream))) return rc;
        a.T = a.fa.ent;
        a.Tinv = g_inv;
        return launch_select_d<KGE_TRANSE, false, true>(a, stream);
    }
    return launch_select_d<KGE_TRANSE, true, true>(a, stream);
}

extern "C" int kge_topk_merge_keys(const uint64_t *d_keys, INT n, INT parts, INT k, int32_t *d_ids, float *d_scores, void *stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (k < 1 || k > 1024) return fail(KGE_ERR_BAD_ARG, "kge_topk_merge_keys: k must be in [1, 1024]");
    if (n < 0 || parts < 1) return fail(KGE_ERR_BAD_ARG, "kge_topk_merge_keys: negative query count or no key list");
    if (parts > (INT)1 << 20) return fail(KGE_ERR_BAD_ARG, "kge_topk_merge_keys: more than 2^20 key lists per query");
    if (!device_ok()) return fail(KGE_ERR_NO_DEVICE, "kge_topk_merge_keys: no usable HIP device");
    if (n == 0) return KGE_OK;
    if (!d_keys || !d_ids || !d_scores) return fail(KGE_ERR_BAD_ARG, "kge_topk_merge_keys: null key or output array");
    TopkArgs a = {};
    a.part = const_cast<uint64_t *>(d_keys);
    a.nq = n; a.k = (int)k;
    a.ids = d_ids; a.scores = d_scores;
    const int KP = (int)pow2_at_least((unsigned)std::max(a.k, 64));
    a.cap = std::max((int)pow2_at_least((unsigned)(a.k + 256)), 2 * KP);   // as launch_select_t's merge
    hipLaunchKernelGGL((topk_merge_kernel<true, false>), dim3((unsigned)n), dim3(256), (size_t)a.cap * sizeof(uint64_t), stream, a, (int)parts);
    return hip_check(hipGetLastError(), "top-k key merge launch");
}
