// Filtered ranks of caller-supplied triples (kge_rank_triples): for triple i and each side, how many candidate entities other
// than the target score strictly below the true triple -- raw, filtered, typed, filtered + typed, rank_kernel's columns 0..3
// (eval.hip) -- for any list of triples on the device: any order, any mix of relations, duplicates.  All four models.
//
// Fused and candidate-major, like topk_select_kernel and lp_range_kernel: no [requests x E] score block is written.  A REQUEST
// is (triple, side).  The host groups the requests by (relation, side) -- the call's one synchronisation -- and cuts each
// group into blocks of NR requests; the grid is (request block x candidate slice).  Every team of L lanes holds the NR request
// vectors of its block in registers (lane l: elements l, l+L, ...), streams its share of the slice of the relation's candidate
// table T_r (models.hip lp_table_kernel) ONCE and scores each row against all NR requests.
//
// The scores are lp_score_kernel's bits (so kge_predict's, and the counts rank_kernel's):
//   * the same table T_r, the same normalised relation vector rn (Team::normalize of the relation's row), the same rung of
//     for_team_shape;
//   * l1_score sums |hn + rn - tn| over the lane's elements in index order and reduces with team_sum<L>, with rn = raw * inv
//     inlined from the normalisation.  Tail side: hn is the request's fixed row and hn + rn is loop-invariant in
//     lp_score_kernel, where the compiler contracts it into fma(raw, inv, hn); it is formed the same way here, once per
//     request, and the candidate subtracted.  Head side: hn is the candidate, lp_score_kernel adds the rounded product rn
//     inside its loop, so (x + rn) is formed once per row with separately rounded operations and the request's fixed row
//     subtracted; the kernel forms fixed - (x + rn) instead, the exact negation, and only the absolute value is used;
//   * team_sum<16> / <32> leave association-dependent bits in each lane and lp_score_kernel reports lane 0's, so lane 0's value
//     is what travels to the lane that owns the request (a DPP shift per request, lp_range_kernel's scheme).  At L = 64 four
//     requests share one reduction: team_sum4 (team.hpp) returns team_sum<64>'s bits for each of its four values;
//   * TransE's predict op divides by (float)D.  The quotient of neighbouring sums can tie, and rank_kernel compares after the
//     division, so the owning lane divides too -- once per candidate row, after the shifts;
//   * the true triple's score is the same code applied to row T_r[target].
// After a row's NR scores have landed, lane q of the team's first lanes owns request q: it compares, and only for a candidate
// strictly below the true triple searches the filter (pair_range once per request, in_range per hit) and the relation's type
// list.  Counts reduce in LDS; one 64-bit atomicAdd per (request, column) and workgroup into the zeroed d_counts.  Integer sums:
// the result does not depend on the schedule nor on the number of slices.
//
// Stored bf16 tables (kge_rank_triples_bf16; TransE): the kernel's BF16 instantiations read the entity table itself in place of T
// and normalise every row they load (load_cand_row), so no [E, D] table is built and the counts are those of the fp32 kernel
// on the widened tables.
#include <algorithm>
#include <cstring>
#include <vector>

#include "eval_dev.hpp"
#include "team.hpp"
#include "team_shape.hpp"

namespace kge {

namespace {

struct RankTriplesArgs {
    const float *rel;          // rel_embeddings (BF16 instantiations: stored bf16 rows, cast where they are read)
    const float *T;            // T_r [E][D]: every entity's projected + normalised vector under the blocks' relation
                               // (BF16 instantiations: the stored bf16 entity table itself, normalised row by row as it is read)
    EvalFilterView ev;
    const int4 *req;           // (fixed entity, target entity, 2 * triple + side, 0), grouped by (relation, side)
    const int4 *blk;           // per request block: (first request, requests, relation, side)
    long long E, slice_len;
    int D;
    long long *counts;         // [n][2][4]
};

// The request whose compare / filter work lane `lane` of a team does, or -1.  The scores of a candidate are shifted through the
// lanes in request order.  L = 16 / 32: row_shr:1 within each 16-lane row, so after all NR of them lane l holds request
// NR - 1 - l (L = 32: lanes of the team's first row only).
// L = 64: the scores come four at a time in lanes 60..63 (team_sum4) and are shifted down the wave's last row four lanes at a
// time (row_shl:4), so lane 64 - NR + q holds request q.
template <int L, int NR>
__device__ __forceinline__ int owned_request(int lane) {
    static_assert(L == 64 ? (NR <= 16 && NR % 4 == 0) : NR == 16, "one request per lane; a 16-lane row holds the shifted scores");
    if constexpr (L == 64) return lane >= 64 - NR ? lane - (64 - NR) : -1;
    else return lane < NR ? NR - 1 - lane : -1;
}

// sum_c |v_c - y_c| over the team: l1_score's per-lane sum and reduction (models_dev.hpp), the value of each lane
template <int C>
__device__ __forceinline__ float l1_lane(const float (&v)[C], const float (&y)[C]) {
    float s = 0.f;
#pragma unroll
    for (int c = 0; c < C; c++) { const float e = v[c] - y[c]; s += fabsf(e); }
    return s;
}
template <int L, int C>
__device__ __forceinline__ float l1_against(const float (&v)[C], const float (&y)[C]) {
    return team_sum<L>(l1_lane<C>(v, y));
}

// Row `row` of the candidate table.  BF16 (kge_rank_triples_bf16, TransE): there is no T; the stored bf16 row is loaded in the same
// lane layout, widened exactly, and normalised here as lp_table_kernel normalises it into T -- Team::normalize's inv (each
// lane its own: team_sum<16> / <32> leave lane-dependent bits) and the ROUNDED product x * inv, which is what a stored T holds;
// left to the optimiser, v - x * inv would come out as one fma.
template <bool BF16, int L, int C>
__device__ __forceinline__ void load_cand_row(const Team<L, C> &tm, const float *T, long long row, float (&x)[C]) {
    if constexpr (BF16) {
        float raw[C], y[C], inv;
        bool uc;
        tm.load((const uint16_t *)T, row, raw);
        tm.normalize(raw, y, inv, uc);
#pragma unroll
        for (int c = 0; c < C; c++) x[c] = mul_rn(raw[c], inv);
    } else {
        tm.load(T, row, x);
    }
}

template <bool MEAN, int L, int C, int NR, int U, bool BF16 = false>
__global__ __launch_bounds__(256) void rank_triples_kernel(RankTriplesArgs a) {
    static_assert(!BF16 || MEAN, "stored bf16 rows: TransE only");
    constexpr int TEAMS = 256 / L;
    __shared__ int s_cnt[NR][4];
    // per request, read on the slow path only: known range (and its first / last id), type range (and its first / last id)
    __shared__ long long s_klo[NR], s_khi[NR];
    __shared__ int s_kmin[NR], s_kmax[NR], s_tlo[NR], s_thi[NR], s_tmin[NR], s_tmax[NR], s_tgt[NR], s_out[NR];
    Team<L, C> tm;
    tm.lane = threadIdx.x % L;
    tm.D = a.D;
    const int team = threadIdx.x / L;
    const int4 bd = a.blk[blockIdx.x];
    const int q0 = bd.x, nb = bd.y, r = bd.z;
    const bool hd = bd.w != 0;
    const int4 *known_arr = hd ? a.ev.all_t : a.ev.all;
    const int32_t *types = hd ? a.ev.head_type : a.ev.tail_type;
    for (int i = threadIdx.x; i < NR * 4; i += blockDim.x) s_cnt[i / 4][i % 4] = 0;
    if ((int)threadIdx.x < NR) {
        const int q = threadIdx.x;
        s_tgt[q] = -1; s_out[q] = 0; s_klo[q] = s_khi[q] = 0; s_kmin[q] = s_kmax[q] = 0; s_tlo[q] = s_thi[q] = 0; s_tmin[q] = s_tmax[q] = 0;
        if (q < nb) {
            const int4 rq = a.req[q0 + q];
            s_tgt[q] = rq.y; s_out[q] = rq.z;
            long long lo, hi;
            pair_range(known_arr, a.ev.n_all, rq.x, r, lo, hi);   // known tails of (h, r) / known heads of (t, r)
            s_klo[q] = lo; s_khi[q] = hi;
            if (hi > lo) { s_kmin[q] = known_arr[lo].z; s_kmax[q] = known_arr[hi - 1].z; }
            const int tl = hd ? a.ev.head_lef[r] : a.ev.tail_lef[r], th = hd ? a.ev.head_rig[r] : a.ev.tail_rig[r];
            s_tlo[q] = tl; s_thi[q] = th;
            if (th > tl) { s_tmin[q] = types[tl]; s_tmax[q] = types[th - 1]; }
        }
    }
    // the relation vector as ctx_forward normalises it: rn = raw * inv.  lp_score_kernel's compiled form (every model and rung)
    // contracts the tail side's loop-invariant hn + rn into fma(raw, inv, hn) and adds the ROUNDED product on the head side,
    // where x + rn sits inside its loop; both are written out here so that the bits do not hang on this kernel's optimiser.
    float rr[C], rn[C], rinv;
    {
        float nrm[C]; bool uc;
        if constexpr (BF16) tm.load((const uint16_t *)a.rel, r, rr);
        else tm.load(a.rel, r, rr);
        tm.normalize(rr, nrm, rinv, uc);
#pragma unroll
        for (int c = 0; c < C; c++) rn[c] = mul_rn(rr[c], rinv);
    }
    // request vectors (every team holds all of them) and the true triples' scores (the lane owning a request keeps its own)
    const int own = owned_request<L, NR>(tm.lane);
    float V[NR][C], mn = 0.f;
#pragma unroll
    for (int q = 0; q < NR; q++) {
#pragma unroll
        for (int c = 0; c < C; c++) V[q][c] = 0.f;
        if (q < nb) {
            const int4 rq = a.req[q0 + q];
            float f[C], y[C];
            if constexpr (BF16) { load_cand_row<true>(tm, a.T, rq.x, f); load_cand_row<true>(tm, a.T, rq.y, y); }
            else { tm.load(a.T, rq.x, f); tm.load(a.T, rq.y, y); }
#pragma unroll
            for (int c = 0; c < C; c++) {
                V[q][c] = hd ? f[c] : __builtin_fmaf(rr[c], rinv, f[c]);
                if (hd) y[c] = add_rn(y[c], rn[c]);
            }
            float s = l1_against<L, C>(V[q], y);
            if constexpr (L != 64) s = __shfl(s, 0, L);   // lane 0's bits
            if constexpr (MEAN) s = s / (float)a.D;
            if (own == q) mn = s;
        }
    }
    __syncthreads();
    const int tgt = own >= 0 ? s_tgt[own] : -1;   // -1: no request, or a padding one
    int cnt[4] = {0, 0, 0, 0};
    const long long j0 = (long long)blockIdx.y * a.slice_len;
    const long long j1 = min(a.E, j0 + a.slice_len);
    for (long long base = j0; base < j1; base += TEAMS * U) {
        float x[U][C];
#pragma unroll
        for (int u = 0; u < U; u++) {
            const long long j = base + (long long)team * U + u;
            if (j < j1) {
                if constexpr (BF16) load_cand_row<true>(tm, a.T, j, x[u]);
                else tm.load(a.T, j, x[u]);
            } else {
#pragma unroll
                for (int c = 0; c < C; c++) x[u][c] = 0.f;
            }
        }
#pragma unroll
        for (int u = 0; u < U; u++) {
            const long long j = base + (long long)team * U + u;
            if (hd) {
#pragma unroll
                for (int c = 0; c < C; c++) x[u][c] = add_rn(x[u][c], rn[c]);
            }
            // every request's score, each landing in the lane that owns the request (owned_request)
            float s = 0.f;
            if constexpr (L == 64) {
                // four requests per reduction: team_sum4 leaves their totals, each with team_sum<64>'s bits, in lanes 60..63; the
                // earlier groups move four lanes down the row (row_shl:4) to make room
                const bool odd = tm.lane & 1, hi2 = tm.lane & 2;
#pragma unroll
                for (int g = 0; g < NR / 4; g++) {
                    float v = 0.f;   // (a group of padding requests still takes its shift: ownership counts all NR of them)
                    if (4 * g < nb)
                        v = team_sum4(l1_lane<C>(V[4 * g], x[u]), l1_lane<C>(V[4 * g + 1], x[u]), l1_lane<C>(V[4 * g + 2], x[u]),
                                      l1_lane<C>(V[4 * g + 3], x[u]), odd, hi2);
                    s = __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, s), 0x104, 0xF, 0xF, false));
                    s = tm.lane >= 60 ? v : s;
                }
            } else {
#pragma unroll
                for (int q = 0; q < NR; q++) {
                    float v = 0.f;   // (a padding request still takes its shift: ownership counts all NR of them)
                    if (q < nb) v = l1_against<L, C>(V[q], x[u]);
                    // shift the scores up one lane (row_shr:1 in each 16-lane row), the new one -- lane 0's -- into the first lane
                    s = __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, s), 0x111, 0xF, 0xF, false));
                    s = (tm.lane & 15) == 0 ? v : s;
                }
            }
            if constexpr (MEAN) s = s / (float)a.D;
            if (j >= j1 || tgt < 0) continue;
            const int id = (int)j;
            if (id == tgt || !(s < mn)) continue;
            const bool known = id >= s_kmin[own] && id <= s_kmax[own] && in_range(known_arr, s_klo[own], s_khi[own], id);
            bool typed = false;
            const int tl = s_tlo[own], th = s_thi[own];
            if (th > tl && id >= s_tmin[own] && id <= s_tmax[own]) {   // lower_bound in the relation's sorted type list
                int lo = tl, hi = th;
                while (lo < hi) { const int mid = (lo + hi) >> 1; if (types[mid] < id) lo = mid + 1; else hi = mid; }
                typed = lo < th && types[lo] == id;
            }
            cnt[0]++;
            if (!known) cnt[1]++;
            if (typed) { cnt[2]++; if (!known) cnt[3]++; }
        }
    }
    if (tgt >= 0) {
#pragma unroll
        for (int i = 0; i < 4; i++)
            if (cnt[i]) atomicAdd(&s_cnt[own][i], cnt[i]);
    }
    __syncthreads();
    for (int i = threadIdx.x; i < NR * 4; i += blockDim.x) {
        const int q = i / 4, col = i % 4;
        if (s_tgt[q] < 0 || !s_cnt[q][col]) continue;
        atomicAdd((unsigned long long *)&a.counts[(long long)s_out[q] * 4 + col], (unsigned long long)s_cnt[q][col]);
    }
}

// requests per workgroup and rows per team in flight, so that the request vectors (NR C floats) stay at 64 registers: a 16- or
// 32-lane team shifts exactly 16 requests through a row; L = 64: 16 / 8 / 4 at C = 4 / 8 / 16
constexpr int rank_nr(int L, int C) { return L != 64 ? 16 : (C <= 4 ? 16 : (C <= 8 ? 8 : 4)); }
constexpr int rank_u(int C) { return C == 16 ? 1 : 2; }

int requests_per_block(int D) {
    int nr = 0;
    for_team_shape(D, [&](auto t) { nr = rank_nr(decltype(t)::L, decltype(t)::C); });
    return nr;
}

// about 2 048 workgroups (eight per CU) over the (request block x slice) grid, slices of at least 1 024 rows
template <bool BF16 = false>
int launch_rank(bool mean, RankTriplesArgs a, long long nblocks, hipStream_t stream) {
    long long slices = engine().rank_slices;
    if (slices <= 0) {
        slices = (2048 + nblocks - 1) / nblocks;
        slices = std::min(slices, a.E / 1024);
    }
    slices = std::max(1LL, std::min({slices, (long long)a.E, 65535LL}));
    a.slice_len = (a.E + slices - 1) / slices;
    slices = (a.E + a.slice_len - 1) / a.slice_len;
    // a launch takes fewer than 2^32 threads along x: at most 2^23 request blocks of 256 threads each, the rest in further launches
    constexpr long long kMaxBlocks = 1LL << 23;
    const bool shaped = for_team_shape(a.D, [&](auto t) {
        constexpr int L = decltype(t)::L, C = decltype(t)::C;
        const int4 *blk = a.blk;
        for (long long b0 = 0; b0 < nblocks; b0 += kMaxBlocks) {
            a.blk = blk + b0;
            const dim3 grid((unsigned)std::min(kMaxBlocks, nblocks - b0), (unsigned)slices);
            if constexpr (BF16) hipLaunchKernelGGL((rank_triples_kernel<true, L, C, rank_nr(L, C), rank_u(C), true>), grid, dim3(256), 0, stream, a);
            else if (mean) hipLaunchKernelGGL((rank_triples_kernel<true, L, C, rank_nr(L, C), rank_u(C)>), grid, dim3(256), 0, stream, a);
            else hipLaunchKernelGGL((rank_triples_kernel<false, L, C, rank_nr(L, C), rank_u(C)>), grid, dim3(256), 0, stream, a);
        }
    });
    if (!shaped) return fail(KGE_ERR_UNSUPPORTED, "kge_rank_triples: embedding dimension > 1024");
    return hip_check(hipGetLastError(), "rank triples launch");
}

// workspace of the calls, grown on demand; this file's own
DevBuf<float> g_T, g_P;
DevBuf<int4> g_req;
std::vector<Int4> g_req_host;   // source of the last upload: rewritten only once g_req_done has passed
hipEvent_t g_req_done = nullptr;

}  // namespace

}  // namespace kge

using namespace kge;

namespace {

// kge_rank_triples (`tables`) and kge_rank_triples_bf16 (`bf16`: tables == nullptr, d_ent / d_rel are stored bf16 rows): one argument
// path, one grouping of the requests.  The bf16 form builds no candidate table: its kernel normalises the stored rows as it reads them.
int rank_triples_call(const std::string &who, bool bf16, const kge_model_desc *m, const float *const tables[KGE_MAX_TABLES], const uint16_t *d_ent,
                      const uint16_t *d_rel, const int32_t *d_h, const int32_t *d_t, const int32_t *d_r, INT n, INT test_head, int64_t *d_counts,
                      hipStream_t stream) {
    if (!m || (bf16 ? !d_ent || !d_rel : !tables) || !d_h || !d_t || !d_r || !d_counts) return fail(KGE_ERR_BAD_ARG, who + ": null model, tables, triple or output array");
    if (n < 0) return fail(KGE_ERR_BAD_ARG, who + ": negative triple count");
    if (n >= (INT(1) << 30)) return fail(KGE_ERR_BAD_ARG, who + ": more than 2^30 triples in one call");
    bool known_model = for_model(m->model, [](auto) {});
    if (!known_model) return fail(KGE_ERR_BAD_ARG, "unknown model id");
    if (bf16)
        if (const char *why = bf16_eval_refusal(m)) return fail(KGE_ERR_UNSUPPORTED, who + ": " + why);
    const int64_t E = m->ent_total;
    const int D = m->model == KGE_TRANSR ? (int)m->rel_dim : (int)m->ent_dim;
    if (D < 1 || E < 1 || m->rel_total < 1) return fail(KGE_ERR_BAD_ARG, who + ": empty model");
    if (D > 1024) return fail(KGE_ERR_UNSUPPORTED, who + ": embedding dimension > 1024");
    if (!device_ok()) return fail(KGE_ERR_NO_DEVICE, who + ": no usable HIP device");
    RankTriplesArgs a = {};
    int rc = eval_filter_view(false, a.ev);
    if (rc) return rc;
    if (n == 0) return KGE_OK;
    if (!bf16 && (!tables[0] || !tables[1])) return fail(KGE_ERR_BAD_ARG, who + ": null table");
    // the one synchronisation: the triples come to the host to be grouped by (relation, side)
    std::vector<int32_t> ids((size_t)n * 3);
    if ((rc = hip_check(hipMemcpyAsync(ids.data(), d_h, sizeof(int32_t) * (size_t)n, hipMemcpyDeviceToHost, stream), "copy heads"))) return rc;
    if ((rc = hip_check(hipMemcpyAsync(ids.data() + n, d_t, sizeof(int32_t) * (size_t)n, hipMemcpyDeviceToHost, stream), "copy tails"))) return rc;
    if ((rc = hip_check(hipMemcpyAsync(ids.data() + 2 * n, d_r, sizeof(int32_t) * (size_t)n, hipMemcpyDeviceToHost, stream), "copy relations"))) return rc;
    if ((rc = hip_check(hipStreamSynchronize(stream), "rank triples sync"))) return rc;
    if (g_req_done && (rc = hip_check(hipEventSynchronize(g_req_done), "rank triples request upload"))) return rc;
    const int32_t *hh = ids.data(), *ht = hh + n, *hr = ht + n;
    const int sides = test_head ? 2 : 1;
    const int64_t R = m->rel_total, n_req = n * sides;
    for (int64_t i = 0; i < n; i++)
        if (hr[i] < 0 || hr[i] >= R) return fail(KGE_ERR_BAD_ARG, who + ": relation id out of range");
    // counting sort by key = 2 * relation + side
    std::vector<int64_t> start((size_t)(2 * R + 1), 0);
    for (int64_t i = 0; i < n; i++)
        for (int s = 0; s < sides; s++) start[(size_t)(2 * hr[i] + s) + 1]++;
    for (int64_t k = 0; k < 2 * R; k++) start[(size_t)k + 1] += start[(size_t)k];
    const int NR = requests_per_block(D);
    int64_t n_blocks = 0;
    for (int64_t k = 0; k < 2 * R; k++) n_blocks += (start[(size_t)k + 1] - start[(size_t)k] + NR - 1) / NR;
    // one upload: the requests, then the block descriptors
    std::vector<Int4> &host = g_req_host;
    host.resize((size_t)(n_req + n_blocks));
    {
        std::vector<int64_t> at(start.begin(), start.end() - 1);
        for (int64_t i = 0; i < n; i++)
            for (int s = 0; s < sides; s++) {
                const int64_t p = at[(size_t)(2 * hr[i] + s)]++;
                host[(size_t)p] = s ? Int4{ht[i], hh[i], (int32_t)(2 * i + 1), 0} : Int4{hh[i], ht[i], (int32_t)(2 * i), 0};
            }
    }
    std::vector<int64_t> rel_block((size_t)R + 1, 0);   // the blocks of relation r: [rel_block[r], rel_block[r + 1])
    {
        int64_t b = 0;
        for (int64_t k = 0; k < 2 * R; k++) {
            if (k % 2 == 0) rel_block[(size_t)(k / 2)] = b;
            for (int64_t p = start[(size_t)k]; p < start[(size_t)k + 1]; p += NR)
                host[(size_t)(n_req + b++)] = Int4{(int32_t)p, (int32_t)std::min<int64_t>(NR, start[(size_t)k + 1] - p), (int32_t)(k / 2), (int32_t)(k % 2)};
        }
        rel_block[(size_t)R] = b;
    }
    if ((rc = g_req.reserve(n_req + n_blocks, "alloc rank requests"))) return rc;
    if (!bf16 && (rc = g_T.reserve(E * D, "alloc rank candidate table"))) return rc;
    if (m->model == KGE_TRANSR && (rc = g_P.reserve((E + 1) * D, "alloc rank projections"))) return rc;
    if (!g_req_done && (rc = hip_check(hipEventCreateWithFlags(&g_req_done, hipEventDisableTiming), "create rank event"))) return rc;
    if ((rc = hip_check(hipMemcpyAsync(g_req, host.data(), sizeof(Int4) * host.size(), hipMemcpyHostToDevice, stream), "upload rank requests"))) return rc;
    if ((rc = hip_check(hipEventRecord(g_req_done, stream), "record rank request upload"))) return rc;
    if ((rc = hip_check(hipMemsetAsync(d_counts, 0, sizeof(int64_t) * 8 * (size_t)n, stream), "zero rank counts"))) return rc;
    a.req = g_req; a.E = E; a.D = D; a.counts = (long long *)d_counts;
    if (bf16) {   // TransE on the stored rows: no T, one launch over every block
        a.rel = (const float *)d_rel; a.T = (const float *)d_ent;   // (read as uint16 rows by the BF16 instantiations)
        a.blk = g_req + n_req;
        return launch_rank<true>(true, a, n_blocks, stream);
    }
    a.rel = tables[1]; a.T = g_T;
    const bool mean = m->model == KGE_TRANSE;
    if (mean) {   // TransE's candidates do not depend on the relation: one table, one launch over every block
        if ((rc = launch_lp_table(*m, tables, nullptr, hr[0], g_T, stream))) return rc;
        a.blk = g_req + n_req;
        return launch_rank(true, a, n_blocks, stream);
    }
    for (int64_t r = 0; r < R; r++) {
        const int64_t b0 = rel_block[(size_t)r], b1 = rel_block[(size_t)r + 1];
        if (b1 == b0) continue;
        if (m->model == KGE_TRANSR && (rc = transr_project_all(*m, tables, r, g_P, stream))) return rc;
        if ((rc = launch_lp_table(*m, tables, g_P, r, g_T, stream))) return rc;
        a.blk = g_req + n_req + b0;
        if ((rc = launch_rank(false, a, b1 - b0, stream))) return rc;
    }
    return KGE_OK;
}

}  // namespace

extern "C" int kge_rank_triples(const kge_model_desc *m, const float *const tables[KGE_MAX_TABLES], const int32_t *d_h, const int32_t *d_t,
                                const int32_t *d_r, INT n, INT test_head, int64_t *d_counts, void *stream) {
    return rank_triples_call("kge_rank_triples", false, m, tables, nullptr, nullptr, d_h, d_t, d_r, n, test_head, d_counts, (hipStream_t)stream);
}

extern "C" int kge_rank_triples_bf16(const kge_model_desc *m, const uint16_t *d_ent, const uint16_t *d_rel, const int32_t *d_h, const int32_t *d_t,
                                     const int32_t *d_r, INT n, INT test_head, int64_t *d_counts, void *stream) {
    return rank_triples_call("kge_rank_triples_bf16", true, m, nullptr, d_ent, d_rel, d_h, d_t, d_r, n, test_head, d_counts, (hipStream_t)stream);
}
