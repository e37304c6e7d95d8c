// Link prediction against a ROW RANGE of the entity table (kge_link_prediction_range / kge_link_prediction_finish): the
// evaluation of a table sharded by rows across ranks (Config._setup_shards), where no rank holds the whole table and the
// [n x E] score matrix of kge_link_prediction cannot be formed.  TransE.
//
// Stage 1 (lp_range_kernel), grid (block of Q test triples x candidate slice), candidate-major as topk_select_kernel: every
// team of L lanes holds the 2Q request vectors of its block in registers (lane l: elements l, l+L, ...) -- hn + rn for the
// tail side, rn - tn for the head side -- streams its share of the slice ONCE, computes each row's 1/|x| once and scores the
// row against all 2Q requests:
//     tail: sum_c |fma(x_c, -1/|x|, hn_c + rn_c)|        head: sum_c |fma(x_c, 1/|x|, rn_c - tn_c)|
// (the L1 distance: TransE's predict op divides it by D, a monotone step left out).  The team sum is `usum`, whose butterfly
// leaves the same bits in every lane, so lane q % L of each team owns request q: it compares, and only for a candidate strictly
// below the true triple's score (`minimal`) searches the filter and the type list.  `minimal` is the SAME function applied to
// the true entity's raw row from d_query_rows, so an entity whose row equals the target's row ties with it and is never
// counted, whichever range holds it.  Counts and arg-min keys (select_dev.hpp pack_key) reduce in LDS; one int64 atomicAdd per
// (request, column) and one 64-bit atomicMin per arg-min per workgroup.  Integer sums and a min: the result does not depend on
// the schedule, nor on how the table is cut into ranges.
// Stage 2 (lp_finish_kernel), one thread per (triple, side): arg-mins and ontology classes as rank_kernel resolves them.
//
// kge_rank_triples_range is the same scan for ANY device-resident triple list (d_h, d_t, d_r), counts only: lp_range_kernel's
// KEYS = false instantiation takes triple p from the three id arrays instead of the sorted test split, disables a triple
// whose ids are out of range before anything is indexed with them, and carries no arg-min keys (no s_key, no key registers, no
// 64-bit atomicMin, no stage 2).  usum / inv_norm / pair_score and the order of every operation are shared, so the counts of
// the test split's triples are kge_link_prediction_range's, bit for bit.  TransE's candidates do not depend on the relation:
// no grouping by relation, no host synchronisation.
#include <algorithm>
#include <cstring>
#include <type_traits>
#include <vector>

#include "eval_dev.hpp"
#include "select_dev.hpp"
#include "team.hpp"
#include "team_shape.hpp"

namespace kge {

namespace {

constexpr long long kNoArg = 0x7fffffffffffffffLL;   // d_keys entry without a candidate below the true triple

// Sum over the L lanes of a team with the same association in every lane (team_sum's row rotations give lane-dependent
// association): two quad butterflies, then half-row and row mirrors (lane l and its mirror add the same two partial sums, in
// either order), then the L = 32 / 64 steps of team_sum (commutative pairs / one lane read back).
template <int L>
__device__ __forceinline__ float usum(float v) {
    v += dpp_f<0xB1>(v);    // quad_perm [1,0,3,2]
    v += dpp_f<0x4E>(v);    // quad_perm [2,3,0,1]
    v += dpp_f<0x141>(v);   // row_half_mirror
    v += dpp_f<0x140>(v);   // row_mirror
    if constexpr (L == 32)
        v += __builtin_bit_cast(float, __builtin_amdgcn_ds_swizzle(__builtin_bit_cast(int, v), (0x10 << 10) | 0x1F));
    if constexpr (L == 64) {
        v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x142, 0xA, 0xF, false));
        v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x143, 0xC, 0xF, false));
        v = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), 63));
    }
    return v;
}

// 1/|x| (rsqrt(max(sum x^2, 1e-12)), tf.nn.l2_normalize) of a row in the team layout: ONE definition for candidates and targets
template <int L, int C>
__device__ __forceinline__ float inv_norm(const float (&x)[C]) {
    float s = 0.f;
#pragma unroll
    for (int c = 0; c < C; c++) s = __builtin_fmaf(x[c], x[c], s);
    s = usum<L>(s);
    return 1.0f / sqrtf(s >= 1e-12f ? s : 1e-12f);
}

// The score of row x (scale f = -1/|x| for a tail request, +1/|x| for a head request) against request vector v: ONE definition
// for candidates and for the true triple.  -0.0 canonicalised so that pack_key orders equal scores by id.
template <int L, int C>
__device__ __forceinline__ float pair_score(const float (&v)[C], const float (&x)[C], float f) {
    float s = 0.f;
#pragma unroll
    for (int c = 0; c < C; c++) s += fabsf(__builtin_fmaf(x[c], f, v[c]));
    s = usum<L>(s);
    return s == 0.f ? 0.f : s;
}

// The request whose compare / filter work lane `lane` of a team does, or -1.  The scores of a candidate are shifted through the
// lanes in request order (wave_shr:1 for L = 64, row_shr:1 within each 16-lane row for L = 16 / 32), so after all NR of them lane
// l holds request NR - 1 - l (L = 16 / 32: lanes of the team's first row).
template <int L, int NR>
__device__ __forceinline__ int owned_request(int lane) {
    static_assert(L == 64 ? NR <= 64 : NR == 16, "one request per lane; 16-lane rows shift exactly 16 requests");
    return lane < NR ? NR - 1 - lane : -1;
}

struct RangeArgs {
    const float *ent;          // rows [row_lo, row_lo + rows) of the entity table, row i = entity row_lo + i
    const float *rel;          // the whole relation table
    const float *qrows;        // [count][2][D]: raw h and t rows of the test triples
    const int4 *test;          // KEYS: (h, t, r) in kge_link_prediction's order, triple p at test[first + p]
    EvalFilterView ev;
    long long first, count, row_lo, rows, slice_len;
    int D, test_head;
    long long *counts, *keys;  // [count][2][4] (keys: KEYS only)
};
// the counts-only instantiation's arguments: the caller's triples in place of `test` / `first`
struct TripleRangeArgs : RangeArgs {
    const int32_t *h, *t, *r;  // triple p = (h[p], t[p], r[p]), ids unchecked
    long long E, R;            // the id bounds a triple is checked against
};
template <bool KEYS>
using RangeArgsOf = std::conditional_t<KEYS, RangeArgs, TripleRangeArgs>;

// Triple p of the call.  KEYS: from the library's own test split, in range by construction.  !KEYS: from the caller's arrays;
// false (and nothing may be indexed with the ids) when one of them is out of range.
template <bool KEYS>
__device__ __forceinline__ bool triple_at(const RangeArgsOf<KEYS> &a, long long p, int &h, int &t, int &r) {
    if constexpr (KEYS) {
        const int4 tt = a.test[a.first + p];
        h = tt.x; t = tt.y; r = tt.z;
        return true;
    } else {
        h = a.h[p]; t = a.t[p]; r = a.r[p];
        return h >= 0 && h < a.E && t >= 0 && t < a.E && r >= 0 && r < a.R;
    }
}

// Its relation alone, for the gather of the relation's row; false as triple_at.
template <bool KEYS>
__device__ __forceinline__ bool relation_at(const RangeArgsOf<KEYS> &a, long long p, int &r) {
    if constexpr (KEYS) {
        r = a.test[a.first + p].z;
        return true;
    } else {
        int h, t;
        return triple_at<false>(a, p, h, t, r);
    }
}

template <bool KEYS, int L, int C, int Q, int U>
__global__ __launch_bounds__(256) void lp_range_kernel(RangeArgsOf<KEYS> a) {
    constexpr int TEAMS = 256 / L;
    constexpr int NR = 2 * Q;               // requests: q < Q tail of triple q, q >= Q head of triple q - Q
    __shared__ int s_cnt[NR][4];
    __shared__ unsigned long long s_key[KEYS ? NR : 1][4];
    // per request, read on the slow path only: known range (and its first / last id), type range (and its first / last id)
    __shared__ long long s_klo[NR], s_khi[NR];
    __shared__ int s_kmin[NR], s_kmax[NR], s_tlo[NR], s_thi[NR], s_tmin[NR], s_tmax[NR], s_tgt[NR];
    Team<L, C> tm;
    tm.lane = threadIdx.x % L;
    tm.D = a.D;
    const int team = threadIdx.x / L;
    const long long p0 = (long long)blockIdx.x * Q;
    const int nb = (int)min((long long)Q, a.count - p0);
    if constexpr (KEYS) {
        for (int i = threadIdx.x; i < NR * 4; i += blockDim.x) { s_cnt[i / 4][i % 4] = 0; s_key[i / 4][i % 4] = kNoKey; }
    } else {
        for (int i = threadIdx.x; i < NR * 4; i += blockDim.x) s_cnt[i / 4][i % 4] = 0;
    }
    if ((int)threadIdx.x < NR) {
        const int q = threadIdx.x, p = q < Q ? q : q - Q;
        const bool head = q >= Q;
        s_tgt[q] = -1; s_klo[q] = s_khi[q] = 0; s_kmin[q] = s_kmax[q] = 0; s_tlo[q] = s_thi[q] = 0; s_tmin[q] = s_tmax[q] = 0;
        int h, t, r;
        if (p < nb && (!head || a.test_head) && triple_at<KEYS>(a, p0 + p, h, t, r)) {
            s_tgt[q] = head ? h : t;
            const int4 *known = head ? a.ev.all_t : a.ev.all;
            long long lo, hi;
            pair_range(known, a.ev.n_all, head ? t : h, r, lo, hi);
            s_klo[q] = lo; s_khi[q] = hi;
            if (hi > lo) { s_kmin[q] = known[lo].z; s_kmax[q] = known[hi - 1].z; }
            const int tl = head ? a.ev.head_lef[r] : a.ev.tail_lef[r], th = head ? a.ev.head_rig[r] : a.ev.tail_rig[r];
            const int32_t *types = head ? a.ev.head_type : a.ev.tail_type;
            s_tlo[q] = tl; s_thi[q] = th;
            if (th > tl) { s_tmin[q] = types[tl]; s_tmax[q] = types[th - 1]; }
        }
    }
    // request vectors (every team holds all of them) and the true triples' scores (the lane owning a request keeps its own)
    const int own = owned_request<L, NR>(tm.lane);
    float V[NR][C], mn = 0.f;
#pragma unroll
    for (int q = 0; q < Q; q++) {
#pragma unroll
        for (int c = 0; c < C; c++) { V[q][c] = 0.f; V[Q + q][c] = 0.f; }
        int r;
        if (q < nb && relation_at<KEYS>(a, p0 + q, r)) {   // (a disabled triple keeps zero vectors and no target)
            float xh[C], xt[C], xr[C];
            tm.load(a.qrows, 2 * (p0 + q), xh);
            tm.load(a.qrows, 2 * (p0 + q) + 1, xt);
            tm.load(a.rel, r, xr);
            const float ih = inv_norm<L, C>(xh), it = inv_norm<L, C>(xt), ir = inv_norm<L, C>(xr);
#pragma unroll
            for (int c = 0; c < C; c++) {
                const float hn = mul_rn(xh[c], ih), tn = mul_rn(xt[c], it), rn = mul_rn(xr[c], ir);
                V[q][c] = add_rn(hn, rn);
                V[Q + q][c] = sub_rn(rn, tn);
            }
            const float mt = pair_score<L, C>(V[q], xt, -it), mh = pair_score<L, C>(V[Q + q], xh, ih);
            if (own == q) mn = mt;
            if (own == Q + q) mn = mh;
        }
    }
    __syncthreads();
    const int tgt = own >= 0 ? s_tgt[own] : -1;   // -1: no request, or a padding / disabled one
    const bool hd = own >= Q;
    const int4 *known_arr = hd ? a.ev.all_t : a.ev.all;
    const int32_t *types = hd ? a.ev.head_type : a.ev.tail_type;
    int cnt[4] = {0, 0, 0, 0};
    unsigned long long key[4] = {kNoKey, kNoKey, kNoKey, kNoKey};   // (never read without KEYS)
    const long long j0 = (long long)blockIdx.y * a.slice_len;
    const long long j1 = min(a.rows, j0 + a.slice_len);
    const int nr = a.test_head ? NR : Q;   // (block-uniform: head requests are scored only when asked for)
    for (long long base = j0; base < j1; base += TEAMS * U) {
        float x[U][C];
#pragma unroll
        for (int u = 0; u < U; u++) {
            const long long j = base + (long long)team * U + u;
            if (j < j1) tm.load(a.ent, j, x[u]);
            else {
#pragma unroll
                for (int c = 0; c < C; c++) x[u][c] = 0.f;
            }
        }
#pragma unroll
        for (int u = 0; u < U; u++) {
            const long long j = base + (long long)team * U + u;
            const float xinv = inv_norm<L, C>(x[u]);
            // every request's score, each landing in the lane that owns the request (owned_request)
            float s = 0.f;
#pragma unroll
            for (int q = 0; q < NR; q++) {
                float v = 0.f;   // (a request not asked for still takes its shift: ownership counts all NR of them)
                if (q < nr) v = pair_score<L, C>(V[q], x[u], q < Q ? -xinv : xinv);
                // shift the scores up one lane (L = 64: wave_shr:1; L = 16 / 32: row_shr:1 in each 16-lane row), the new one
                // into the first lane
                s = __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, s), L == 64 ? 0x138 : 0x111, 0xF, 0xF, false));
                s = (L == 64 ? tm.lane : (tm.lane & 15)) == 0 ? v : s;
            }
            if (j >= j1 || tgt < 0) continue;
            const int id = (int)(a.row_lo + j);
            if (id == tgt || !(s < mn)) continue;
            const bool known = id >= s_kmin[own] && id <= s_kmax[own] && in_range(known_arr, s_klo[own], s_khi[own], id);
            bool typed = false;
            const int tl = s_tlo[own], th = s_thi[own];
            if (th > tl && id >= s_tmin[own] && id <= s_tmax[own]) {   // lower_bound in the relation's sorted type list
                int lo = tl, hi = th;
                while (lo < hi) { const int mid = (lo + hi) >> 1; if (types[mid] < id) lo = mid + 1; else hi = mid; }
                typed = lo < th && types[lo] == id;
            }
            if constexpr (KEYS) {
                const unsigned long long k = pack_key(s, id);
                cnt[0]++; key[0] = min(key[0], k);
                if (!known) cnt[1]++;
                if (hd || !known) key[1] = min(key[1], k);   // Test.h:69-74: the head side updates this arg-min outside the filter
                if (typed) {
                    cnt[2]++; key[2] = min(key[2], k);
                    if (!known) { cnt[3]++; key[3] = min(key[3], k); }
                }
            } else {
                cnt[0]++;
                if (!known) cnt[1]++;
                if (typed) { cnt[2]++; if (!known) cnt[3]++; }
            }
        }
    }
    if (tgt >= 0) {
#pragma unroll
        for (int i = 0; i < 4; i++) {
            if (cnt[i]) atomicAdd(&s_cnt[own][i], cnt[i]);
            if constexpr (KEYS) { if (key[i] != kNoKey) atomicMin(&s_key[own][i], key[i]); }
        }
    }
    __syncthreads();
    for (int i = threadIdx.x; i < NR * 4; i += blockDim.x) {
        const int q = i / 4, col = i % 4;
        if (s_tgt[q] < 0) continue;
        const long long o = ((p0 + (q < Q ? q : q - Q)) * 2 + (q >= Q ? 1 : 0)) * 4 + col;
        if (s_cnt[q][col]) atomicAdd((unsigned long long *)&a.counts[o], (unsigned long long)s_cnt[q][col]);
        // counted scores are >= +0, so their keys have the top bit set: as int64 they are negative and order as the unsigned keys do
        if constexpr (KEYS) { if (s_key[q][col] != kNoKey) atomicMin(&a.keys[o], (long long)s_key[q][col]); }
    }
}

__global__ void lp_range_init_kernel(long long *counts, long long *keys, long long n) {
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
        counts[i] = 0;
        keys[i] = kNoArg;
    }
}

struct FinishArgs {
    const int4 *test;
    EvalOntologyView ov;
    const long long *counts, *keys;
    long long first, count;
    int test_head;
    long long *out;            // [count][2][8]
};

__global__ void lp_finish_kernel(FinishArgs a) {
    const long long g = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= a.count * 2) return;
    const long long i = g / 2;
    const int side = (int)(g % 2);
    long long *o = a.out + g * 8;
    if (side == 1 && !a.test_head) {
        for (int c = 0; c < 8; c++) o[c] = 0;
        return;
    }
    const int4 tt = a.test[a.first + i];
    const int target = side ? tt.x : tt.y;
    int arg[4];
    for (int c = 0; c < 4; c++) {
        o[c] = a.counts[g * 4 + c];
        const long long k = a.keys[g * 4 + c];
        arg[c] = k == kNoArg ? target : (int)(uint32_t)(unsigned long long)k;
    }
    // ontology classes with the reference's shared, never-rewinding cursors (Test.h:113-135), as rank_kernel
    int lsup = a.ov.sup_lef[target], rsup = a.ov.sup_rig[target], lsub = a.ov.sub_lef[target], rsub = a.ov.sub_rig[target];
    for (int c = 0; c < 4; c++) {
        const int v = arg[c];
        long long cls = 3;
        if (v == target) cls = 0;
        else {
            while (lsup < rsup && a.ov.sup_type[lsup] < v) lsup++;
            if (lsup < rsup && a.ov.sup_type[lsup] == v) cls = 1;
            else {
                while (lsub < rsub && a.ov.sub_type[lsub] < v) lsub++;
                if (lsub < rsub && a.ov.sub_type[lsub] == v) cls = 2;
            }
        }
        o[4 + c] = cls;
    }
}

__global__ void test_entity_ids_kernel(const int4 *test, long long first, long long count, int32_t *ids) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < count) { const int4 tt = test[first + i]; ids[2 * i] = tt.x; ids[2 * i + 1] = tt.y; }
}

// about 2 048 workgroups (eight per CU) over the (triple block x slice) grid, slices of at least 1 024 rows
template <bool KEYS, int L, int C, int Q, int U>
int launch_range_t(RangeArgsOf<KEYS> a, hipStream_t stream) {
    const long long qblocks = (a.count + Q - 1) / Q;
    long long slices = (2048 + qblocks - 1) / qblocks;
    slices = std::max(1LL, std::min(slices, a.rows / 1024));
    a.slice_len = (a.rows + slices - 1) / slices;
    slices = (a.rows + a.slice_len - 1) / a.slice_len;
    hipLaunchKernelGGL((lp_range_kernel<KEYS, L, C, Q, U>), dim3((unsigned)qblocks, (unsigned)slices), dim3(256), 0, stream, a);
    return hip_check(hipGetLastError(), "lp range launch");
}

// Q triples per workgroup so that the 2Q request vectors (2 Q C floats) stay at 128 registers, U rows per team in flight:
// (Q, U) = (8, 4), (8, 4), (8, 2), (8, 2), (16, 2), (8, 2), (4, 1) by rung
constexpr int range_q(int L, int C) { return L == 64 && C == 4 ? 16 : (C == 16 ? 4 : 8); }
constexpr int range_u(int C) { return C <= 2 ? 4 : (C == 16 ? 1 : 2); }

template <bool KEYS>
int launch_range(const RangeArgsOf<KEYS> &a, hipStream_t stream) {
    int rc = KGE_OK;
    const bool shaped = for_team_shape(a.D, [&](auto t) {
        constexpr int L = decltype(t)::L, C = decltype(t)::C;
        rc = launch_range_t<KEYS, L, C, range_q(L, C), range_u(C)>(a, stream);
    });
    return shaped ? rc : fail(KGE_ERR_UNSUPPORTED, "link prediction over a row range: embedding dimension > 1024");
}

DevBuf<long long> g_out;

}  // namespace

}  // namespace kge

using namespace kge;

extern "C" {

int kge_link_prediction_range(const kge_model_desc *m, const float *const tables[KGE_MAX_TABLES], INT row_lo, INT rows,
                              const float *d_query_rows, INT first, INT count, INT test_head, int64_t *d_counts, int64_t *d_keys,
                              void *stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (!m || !tables) return fail(KGE_ERR_BAD_ARG, "kge_link_prediction_range: null model or tables");
    if (m->model != KGE_TRANSE) return fail(KGE_ERR_UNSUPPORTED, "kge_link_prediction_range: TransE only");
    if (m->ent_dim < 1 || m->ent_dim > 1024) return fail(KGE_ERR_UNSUPPORTED, "kge_link_prediction_range: embedding dimension must be in [1, 1024]");
    if (row_lo < 0 || rows < 0 || row_lo + rows > m->ent_total) return fail(KGE_ERR_BAD_ARG, "kge_link_prediction_range: row range outside the entity table");
    if (!device_ok()) return fail(KGE_ERR_NO_DEVICE, "kge_link_prediction_range: no usable HIP device");
    RangeArgs a = {};
    int rc = eval_filter_view(false, a.ev);
    if (rc) return rc;
    int64_t total = 0;
    if ((rc = eval_test_view(a.test, total))) return rc;
    if (first < 0 || count < 0 || first + count > total) return fail(KGE_ERR_BAD_ARG, "kge_link_prediction_range: bad test range");
    if (count == 0) return KGE_OK;
    if (!d_counts || !d_keys || !d_query_rows || (rows > 0 && (!tables[0] || !tables[1])))
        return fail(KGE_ERR_BAD_ARG, "kge_link_prediction_range: null table, query or output array");
    const long long n = count * 8;
    hipLaunchKernelGGL(lp_range_init_kernel, dim3((unsigned)std::min<long long>((n + 255) / 256, 1024)), dim3(256), 0, stream,
                       (long long *)d_counts, (long long *)d_keys, n);
    if ((rc = hip_check(hipGetLastError(), "lp range init launch"))) return rc;
    if (rows == 0) return KGE_OK;
    a.ent = tables[0]; a.rel = tables[1]; a.qrows = d_query_rows;
    a.first = first; a.count = count; a.row_lo = row_lo; a.rows = rows;
    a.D = (int)m->ent_dim; a.test_head = test_head ? 1 : 0;
    a.counts = (long long *)d_counts; a.keys = (long long *)d_keys;
    return launch_range<true>(a, stream);
}

int kge_rank_triples_range(const kge_model_desc *m, const float *const tables[KGE_MAX_TABLES], INT row_lo, INT rows,
                           const float *d_query_rows, const int32_t *d_h, const int32_t *d_t, const int32_t *d_r, INT n, INT test_head,
                           int64_t *d_counts, void *stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (!m || !tables) return fail(KGE_ERR_BAD_ARG, "kge_rank_triples_range: null model or tables");
    if (m->model != KGE_TRANSE) return fail(KGE_ERR_UNSUPPORTED, "kge_rank_triples_range: TransE only");
    if (m->ent_dim < 1 || m->ent_dim > 1024) return fail(KGE_ERR_UNSUPPORTED, "kge_rank_triples_range: embedding dimension must be in [1, 1024]");
    if (row_lo < 0 || rows < 0 || row_lo + rows > m->ent_total) return fail(KGE_ERR_BAD_ARG, "kge_rank_triples_range: row range outside the entity table");
    if (n < 0) return fail(KGE_ERR_BAD_ARG, "kge_rank_triples_range: negative triple count");
    if (n >= (INT(1) << 30)) return fail(KGE_ERR_BAD_ARG, "kge_rank_triples_range: more than 2^30 triples in one call");
    if (!device_ok()) return fail(KGE_ERR_NO_DEVICE, "kge_rank_triples_range: no usable HIP device");
    TripleRangeArgs a = {};
    int rc = eval_filter_view(false, a.ev);
    if (rc) return rc;
    if (n == 0) return KGE_OK;
    if (!d_counts || !d_query_rows || !d_h || !d_t || !d_r || (rows > 0 && (!tables[0] || !tables[1])))
        return fail(KGE_ERR_BAD_ARG, "kge_rank_triples_range: null table, query, triple or output array");
    if ((rc = hip_check(hipMemsetAsync(d_counts, 0, sizeof(int64_t) * 8 * (size_t)n, stream), "zero rank range counts"))) return rc;
    if (rows == 0) return KGE_OK;
    a.ent = tables[0]; a.rel = tables[1]; a.qrows = d_query_rows;
    a.h = d_h; a.t = d_t; a.r = d_r;
    a.count = n; a.row_lo = row_lo; a.rows = rows; a.E = m->ent_total; a.R = m->rel_total;
    a.D = (int)m->ent_dim; a.test_head = test_head ? 1 : 0;
    a.counts = (long long *)d_counts;
    return launch_range<false>(a, stream);
}

int kge_link_prediction_finish(INT first, INT count, INT test_head, const int64_t *d_counts, const int64_t *d_keys, int64_t *h_out,
                               void *stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (!device_ok()) return fail(KGE_ERR_NO_DEVICE, "kge_link_prediction_finish: no usable HIP device");
    FinishArgs a = {};
    int64_t total = 0;
    int rc = eval_test_view(a.test, total);
    if (rc) return rc;
    if ((rc = eval_ontology_view(a.ov))) return rc;
    if (first < 0 || count < 0 || first + count > total) return fail(KGE_ERR_BAD_ARG, "kge_link_prediction_finish: bad test range");
    if (count == 0) return KGE_OK;
    if (!d_counts || !d_keys || !h_out) return fail(KGE_ERR_BAD_ARG, "kge_link_prediction_finish: null array");
    if ((rc = g_out.reserve(16 * count, "alloc lp finish out"))) return rc;
    a.counts = (const long long *)d_counts; a.keys = (const long long *)d_keys;
    a.first = first; a.count = count; a.test_head = test_head ? 1 : 0; a.out = g_out;
    hipLaunchKernelGGL(lp_finish_kernel, dim3((unsigned)((2 * count + 255) / 256)), dim3(256), 0, stream, a);
    if ((rc = hip_check(hipGetLastError(), "lp finish launch"))) return rc;
    if ((rc = hip_check(hipMemcpyAsync(h_out, g_out, sizeof(long long) * 16 * (size_t)count, hipMemcpyDeviceToHost, stream), "copy ranks"))) return rc;
    return hip_check(hipStreamSynchronize(stream), "lp finish sync");
}

int kge_test_entity_ids(INT first, INT count, int32_t *d_ids, void *stream_) {
    if (!device_ok()) return fail(KGE_ERR_NO_DEVICE, "kge_test_entity_ids: no usable HIP device");
    const int4 *test = nullptr;
    int64_t total = 0;
    int rc = eval_test_view(test, total);
    if (rc) return rc;
    if (first < 0 || count < 0 || first + count > total) return fail(KGE_ERR_BAD_ARG, "kge_test_entity_ids: bad test range");
    if (count == 0) return KGE_OK;
    if (!d_ids) return fail(KGE_ERR_BAD_ARG, "kge_test_entity_ids: null array");
    hipLaunchKernelGGL(test_entity_ids_kernel, dim3((unsigned)((count + 255) / 256)), dim3(256), 0, (hipStream_t)stream_, test, (long long)first,
                       (long long)count, d_ids);
    return hip_check(hipGetLastError(), "test entity ids launch");
}

}  // extern "C"
