// Ranks of triples against candidate LISTS (kge_rank_candidates): per (triple, side) how many of its n_cand candidates, other
// than the target id, score strictly below the true triple -- raw and filtered.  The list is the caller's (one per triple, or
// one shared by all) or is drawn inside the kernel from a counter hash, so that a drawn list never exists in memory.
//
// Fused form (TransE / TransH / TransD): a REQUEST is (triple, side) and a team of L lanes takes it, (L, C) from for_team_shape.
// The team loads the relation context and the fixed side once, scores the true triple and walks its slice of the list:
// candidate ids arrive L at a time in one coalesced load (or one hash per lane), are handed out by lane broadcast, and U rows
// are gathered into registers before the first is consumed.  No T_r, no score block: the cost is n x n_cand x D.
//
// The scores are kge_predict's bits: predict_kernel's compiled form, written out operation by operation in predict_dev.hpp
// (project_row, predict_score), so that the bits do not hang on this kernel's optimiser -- here the fixed side is loop-invariant
// and the compiler would contract differently.  The true triple's score is the same code applied to the target's row.
//
// Two-stage form (TransR; every model with option rankc_fused = 0; the fused kernel's reference): chunks of at most 2^22
// (triple, candidate) pairs are spelled out as id arrays in a bounded workspace, scored by launch_predict (TransR: groups of 16
// pairs of one triple share a projection tile, so each pair is projected by its own relation's matrix) and compared with the
// target's score by a small count kernel that does the same filter search.
//
// Row-range form (kge_rank_candidates_range; TransE, a table sharded by rows across ranks): the fused kernel's RANGE
// instantiations rank against the candidates whose rows one shard holds; the comment on the kernel has the rest.
//
// Stored bf16 tables (kge_rank_candidates_bf16; TransE, the list form): the fused kernel's BF16 instantiations read `ent` and
// `rel` as uint16 rows through Team::load's widening overload -- same team shape, same operations after the load, so the counts
// are those of the fp32 kernel on the widened tables.  Its two-stage form scores the pairs with launch_predict_bf16.
#include <algorithm>
#include <type_traits>

#include "eval_dev.hpp"
#include "mix_dev.hpp"
#include "models_dev.hpp"
#include "predict_dev.hpp"
#include "team.hpp"
#include "team_shape.hpp"

namespace kge {

namespace {

enum { kList = 0, kDrawn = 1, kDrawnTyped = 2 };

struct RankCandArgs {
    const void *ent, *rel;     // fp32 rows; stored bf16 rows (uint16) for the kernel's BF16 instantiations
    const float *auxr, *auxe;
    EvalFilterView ev;
    const int32_t *h, *t, *r;
    const int32_t *cand[2];    // per side; null = not ranked (list mode)
    long long stride[2];
    long long n, n_req, n_cand, slice_len;
    long long E, R;
    int D;
    int nsides, side0;         // request q -> triple q / nsides, side nsides == 2 ? q % 2 : side0
    int filtered, atomic;
    unsigned long long seed;
    long long *counts;         // [n][2][2]
};

// candidate k of (triple i, side s) as an index into a list of `len` entries (the header has the formula)
__host__ __device__ inline long long drawn_index(unsigned long long seed, long long i, int s, long long k, long long len) {
    const unsigned long long c = ((unsigned long long)(2 * i + s) << 32) | (unsigned long long)k;
    return (long long)mix_scale(mix64(seed + (c + 1ULL) * kMixGamma), (unsigned long long)len);
}

// The row-range form (kge_rank_candidates_range): `ent` holds the rows of the global ids [row_lo, row_lo + rows) only, and the
// raw h and t row of triple i come from qrows [n][2][D] instead of the table.
struct RankCandRangeArgs : RankCandArgs {
    const float *qrows;
    long long row_lo, rows;
};

// the id of candidate k of request (i, side), or -1: list entry, or drawn (MODE) from all entities / the relation's type list
template <int MODE>
__device__ __forceinline__ int candidate_id(const RankCandArgs &a, long long i, int side, int r, long long k) {
    int id;
    if constexpr (MODE == kList) {
        id = a.cand[side][i * a.stride[side] + k];
    } else {
        id = (int)drawn_index(a.seed, i, side, k, a.E);
        if constexpr (MODE == kDrawnTyped) {
            const int lo = side ? a.ev.head_lef[r] : a.ev.tail_lef[r], hi = side ? a.ev.head_rig[r] : a.ev.tail_rig[r];
            if (hi > lo) id = (side ? a.ev.head_type : a.ev.tail_type)[lo + drawn_index(a.seed, i, side, k, hi - lo)];
        }
    }
    return (id >= 0 && id < a.E) ? id : -1;
}

// BF16: `ent` and `rel` are stored bf16 rows (uint16), widened exactly as they are loaded; TransE without RANGE only.
// RANGE: the candidates with a global id in [row_lo, row_lo + rows) only, gathered at their local row.  Every team still
// walks the whole list (the ids cost a load or a hash each), but gathers and scores what it owns: the owned ids of a batch are
// compacted to the low lanes (a ballot masked to the team's own lanes, a prefix count, one ds_permute) behind the `p` ids left
// pending from the batches before, rounds of U rows are drawn from that queue while it holds U, and the last round is padded.
template <int MODEL, int L, int C, int U, int MODE, bool RANGE, bool BF16 = false>
__global__ __launch_bounds__(256) void rank_cand_kernel(std::conditional_t<RANGE, RankCandRangeArgs, RankCandArgs> a) {
    constexpr int TEAMS = 256 / L;
    static_assert(L % U == 0, "a batch of ids is handed out U at a time");
    static_assert(!BF16 || (MODEL == KGE_TRANSE && !RANGE), "stored bf16 rows: TransE's list form only");
    using Tab = std::conditional_t<BF16, uint16_t, float>;      // (a.ent / a.rel are cast where they are read, as the fp32 kernel reads them)
    Team<L, C> tm;
    tm.lane = threadIdx.x % L;
    tm.D = a.D;
    const long long q = (long long)blockIdx.x * TEAMS + threadIdx.x / L;
    if (q >= a.n_req) return;
    const long long i = q / a.nsides;
    const int side = a.nsides == 2 ? (int)(q % 2) : a.side0;
    const int h = a.h[i], t = a.t[i], r = a.r[i];
    if (h < 0 || h >= a.E || t < 0 || t >= a.E || r < 0 || r >= a.R) return;   // disabled: the zeroed counts stay
    const bool hd = side != 0;
    const int fixed = hd ? t : h, target = hd ? h : t;
    // relation context: the raw relation row and 1 / |row|; TransH's normalised normal vector / TransD's r_p
    float rr[C], cw[C], inv_r;
    tm.load((const Tab *)a.rel, r, rr);
    {
        const float ss = tm.dot(rr, rr);
        inv_r = 1.0f / sqrtf(ss >= 1e-12f ? ss : 1e-12f);
    }
    if constexpr (MODEL == KGE_TRANSH) {
        float w[C];
        tm.load(a.auxr, r, w);
        const float ss = tm.dot(w, w);
        const float inv_w = 1.0f / sqrtf(ss >= 1e-12f ? ss : 1e-12f);
#pragma unroll
        for (int c = 0; c < C; c++) cw[c] = mul_rn(w[c], inv_w);
    } else if constexpr (MODEL == KGE_TRANSD) {
        tm.load(a.auxr, r, cw);
    } else {
#pragma unroll
        for (int c = 0; c < C; c++) cw[c] = 0.f;
    }
    // the fixed side: as the head (tail requests) its normalised vector, as the tail (head requests) its projected vector
    float fx[C], inv_f;
    {
        float raw[C], aux[C];
        if constexpr (RANGE) tm.load(a.qrows, 2 * i + (hd ? 1 : 0), raw);
        else tm.load((const Tab *)a.ent, fixed, raw);
        if constexpr (MODEL == KGE_TRANSD) tm.load(a.auxe, fixed, aux);
        project_row<MODEL, L, C>(tm, raw, aux, cw, fx, inv_f);
        if (!hd) {
#pragma unroll
            for (int c = 0; c < C; c++) fx[c] = mul_rn(fx[c], inv_f);
        }
    }
    // the score of request (fixed, candidate row): the candidate is the tail (tail requests) or the head
    auto score = [&](const float (&raw)[C], const float (&aux)[C]) {
        float xp[C], inv, hn[C], xt[C];
        project_row<MODEL, L, C>(tm, raw, aux, cw, xp, inv);
#pragma unroll
        for (int c = 0; c < C; c++) {
            hn[c] = hd ? mul_rn(xp[c], inv) : fx[c];
            xt[c] = hd ? fx[c] : xp[c];
        }
        return predict_score<MODEL, L, C>(hn, rr, inv_r, xt, hd ? inv_f : inv, a.D);
    };
    float mn;
    {
        float raw[C], aux[C];
        if constexpr (RANGE) tm.load(a.qrows, 2 * i + (hd ? 0 : 1), raw);
        else tm.load((const Tab *)a.ent, target, raw);
        if constexpr (MODEL == KGE_TRANSD) tm.load(a.auxe, target, aux);
        mn = score(raw, aux);
    }
    // the known tails of (h, r) / heads of (t, r): found on the first candidate below the target (lane 0 only)
    const int4 *known_arr = hd ? a.ev.all_t : a.ev.all;
    bool have_range = false;
    long long klo = 0, khi = 0;
    int kmin = 0, kmax = -1;
    long long c0 = 0, c1 = 0;
    const long long k_lo = (long long)blockIdx.y * a.slice_len;
    const long long k_hi = min(a.n_cand, k_lo + a.slice_len);
    if constexpr (RANGE) {
        static_assert(MODEL == KGE_TRANSE, "only TransE shards its entity table");
        const int tbase = (threadIdx.x % 64) / L * L;                        // the team's first lane in its wave
        const unsigned long long tmask = L == 64 ? ~0ULL : (1ULL << (L % 64)) - 1;
        const long long r_lo = a.row_lo, r_hi = a.row_lo + a.rows;
        // one round: U owned ids (global; -1 pads the last round and gathers local row 0), gathered, scored and counted
        auto round = [&](const int (&id)[U]) {
            float x[U][C];
#pragma unroll
            for (int u = 0; u < U; u++) tm.load((const Tab *)a.ent, id[u] >= 0 ? id[u] - r_lo : 0, x[u]);
#pragma unroll
            for (int u = 0; u < U; u++) {
                const float s = score(x[u], x[u]);
                if (tm.lane != 0 || id[u] < 0 || id[u] == target || !(s < mn)) continue;
                c0++;
                if (!a.filtered) continue;
                if (!have_range) {
                    have_range = true;
                    pair_range(known_arr, a.ev.n_all, fixed, r, klo, khi);
                    if (khi > klo) { kmin = known_arr[klo].z; kmax = known_arr[khi - 1].z; }
                }
                if (!(id[u] >= kmin && id[u] <= kmax && in_range(known_arr, klo, khi, id[u]))) c1++;
            }
        };
        int pend = -1, p = 0;      // the queue: lane j < p holds a pending owned id; p < U between batches
        for (long long k0 = k_lo; k0 < k_hi; k0 += L) {
            const long long k = k0 + tm.lane;
            const int mine = k < k_hi ? candidate_id<MODE>(a, i, side, r, k) : -1;
            const bool own = mine >= r_lo && mine < r_hi;
            const unsigned long long owned = (__ballot(own) >> tbase) & tmask;       // this team's lanes only
            const int m = __popcll(owned), below = __popcll(owned & ((1ULL << tm.lane) - 1));
            // a permutation of the team: the owned ids to lanes 0 .. m-1 in list order, the others behind them
            const int fresh = __builtin_amdgcn_ds_permute((tbase + (own ? below : m + tm.lane - below)) << 2, mine);
            int s = 0;             // queue entry e: pend's lane e while e < p, then fresh's lane e - p
            for (; p + m - s >= U; s += U) {
                int id[U];
#pragma unroll
                for (int u = 0; u < U; u++) {
                    const int e = s + u;
                    id[u] = team_bcast<L>(e < p ? pend : fresh, e < p ? e : e - p);
                }
                round(id);
            }
            const int src = s + tm.lane;       // what is left (fewer than U) moves to the queue's front
            const int moved = __shfl(fresh, src >= p ? src - p : 0, L);
            if (src >= p) pend = moved;
            p += m - s;
        }
        if (p > 0) {
            int id[U];
#pragma unroll
            for (int u = 0; u < U; u++) {
                const int v = team_bcast<L>(pend, u);
                id[u] = u < p ? v : -1;
            }
            round(id);
        }
    } else {
        for (long long k0 = k_lo; k0 < k_hi; k0 += L) {
            const long long k = k0 + tm.lane;
            const int mine = k < k_hi ? candidate_id<MODE>(a, i, side, r, k) : -1;
            const int nk = (int)min((long long)L, k_hi - k0);
            for (int j = 0; j < nk; j += U) {
                int id[U];
                float x[U][C], ax[U][C];
#pragma unroll
                for (int u = 0; u < U; u++) {
                    id[u] = team_bcast<L>(mine, j + u);
                    const long long row = id[u] >= 0 ? id[u] : 0;   // a skipped id still loads a row: no branch around the gathers
                    tm.load((const Tab *)a.ent, row, x[u]);
                    if constexpr (MODEL == KGE_TRANSD) tm.load(a.auxe, row, ax[u]);
                }
#pragma unroll
                for (int u = 0; u < U; u++) {
                    const float s = score(x[u], ax[u]);
                    if (tm.lane != 0 || id[u] < 0 || id[u] == target || !(s < mn)) continue;
                    c0++;
                    if (!a.filtered) continue;
                    if (!have_range) {
                        have_range = true;
                        pair_range(known_arr, a.ev.n_all, fixed, r, klo, khi);
                        if (khi > klo) { kmin = known_arr[klo].z; kmax = known_arr[khi - 1].z; }
                    }
                    if (!(id[u] >= kmin && id[u] <= kmax && in_range(known_arr, klo, khi, id[u]))) c1++;
                }
            }
        }
    }
    if (tm.lane != 0) return;
    if (!a.filtered) c1 = c0;
    long long *out = a.counts + (2 * i + side) * 2;
    if (a.atomic) {
        if (c0) atomicAdd((unsigned long long *)out, (unsigned long long)c0);
        if (c1) atomicAdd((unsigned long long *)out + 1, (unsigned long long)c1);
    } else {
        out[0] = c0;
        out[1] = c1;
    }
}

// candidate rows in flight per team: four, two where a row is 16 registers (and TransD gathers two rows per candidate)
template <int MODEL> constexpr int rankc_u(int C) { return C >= 16 ? (MODEL == KGE_TRANSD ? 1 : 2) : (C >= 8 && MODEL == KGE_TRANSD ? 2 : 4); }

// slices of a list over the grid's y: about 2 048 workgroups, no slice shorter than four batches of ids
long long rankc_slices(long long nblocks, long long n_cand, int L) {
    long long slices = engine().rankc_slices;
    if (slices <= 0) {
        slices = (2048 + nblocks - 1) / nblocks;
        slices = std::min(slices, n_cand / (4 * L));
    }
    return std::max(1LL, std::min({slices, n_cand, 65535LL}));
}

template <int MODEL, bool BF16 = false>
int launch_fused(RankCandArgs a, int mode, hipStream_t stream) {
    const bool shaped = for_team_shape(a.D, [&](auto t) {
        constexpr int L = decltype(t)::L, C = decltype(t)::C, U = rankc_u<MODEL>(C);
        constexpr long long TEAMS = 256 / L;
        const long long nblocks = (a.n_req + TEAMS - 1) / TEAMS;
        long long slices = rankc_slices(nblocks, a.n_cand, L);
        a.slice_len = (a.n_cand + slices - 1) / slices;
        slices = (a.n_cand + a.slice_len - 1) / a.slice_len;
        a.atomic = slices > 1;
        const dim3 grid((unsigned)nblocks, (unsigned)slices);   // n < 2^30: at most 2^31 / TEAMS blocks along x
        if (mode == kList) hipLaunchKernelGGL((rank_cand_kernel<MODEL, L, C, U, kList, false, BF16>), grid, dim3(256), 0, stream, a);
        else if (mode == kDrawn) hipLaunchKernelGGL((rank_cand_kernel<MODEL, L, C, U, kDrawn, false, BF16>), grid, dim3(256), 0, stream, a);
        else hipLaunchKernelGGL((rank_cand_kernel<MODEL, L, C, U, kDrawnTyped, false, BF16>), grid, dim3(256), 0, stream, a);
    });
    if (!shaped) return fail(KGE_ERR_UNSUPPORTED, "kge_rank_candidates: embedding dimension > 1024");
    return hip_check(hipGetLastError(), "rank candidates launch");
}

// the row-range form (TransE): the same grid, slices and U
int launch_range(RankCandRangeArgs a, int mode, hipStream_t stream) {
    const bool shaped = for_team_shape(a.D, [&](auto t) {
        constexpr int L = decltype(t)::L, C = decltype(t)::C, U = rankc_u<KGE_TRANSE>(C);
        constexpr long long TEAMS = 256 / L;
        const long long nblocks = (a.n_req + TEAMS - 1) / TEAMS;
        long long slices = rankc_slices(nblocks, a.n_cand, L);
        a.slice_len = (a.n_cand + slices - 1) / slices;
        slices = (a.n_cand + a.slice_len - 1) / a.slice_len;
        a.atomic = slices > 1;
        const dim3 grid((unsigned)nblocks, (unsigned)slices);
        if (mode == kList) hipLaunchKernelGGL((rank_cand_kernel<KGE_TRANSE, L, C, U, kList, true>), grid, dim3(256), 0, stream, a);
        else if (mode == kDrawn) hipLaunchKernelGGL((rank_cand_kernel<KGE_TRANSE, L, C, U, kDrawn, true>), grid, dim3(256), 0, stream, a);
        else hipLaunchKernelGGL((rank_cand_kernel<KGE_TRANSE, L, C, U, kDrawnTyped, true>), grid, dim3(256), 0, stream, a);
    });
    if (!shaped) return fail(KGE_ERR_UNSUPPORTED, "kge_rank_candidates_range: embedding dimension > 1024");
    return hip_check(hipGetLastError(), "rank candidates range launch");
}

// ---- two-stage form -------------------------------------------------------------------------------------------------------
// Pair g of the call: request g / Cp, position g % Cp of its list (positions n_cand .. Cp - 1 are padding: Cp rounds the list up
// to whole projection tiles for TransR).  With `targets` the "list" of a request is its own target, G entries wide.
struct SpellArgs {
    RankCandArgs a;
    int mode, targets;
    long long Cp, g0, len;
    int32_t *ph, *pt, *pr, *pc;   // [len]: the pair's triple (0, 0, r for a pair that is not scored) and its candidate id or -1
};

__device__ __forceinline__ void request_of(const RankCandArgs &a, long long q, long long &i, int &side) {
    i = q / a.nsides;
    side = a.nsides == 2 ? (int)(q % 2) : a.side0;
}

__global__ __launch_bounds__(256) void spell_kernel(SpellArgs s) {
    const RankCandArgs &a = s.a;
    for (long long x = (long long)blockIdx.x * blockDim.x + threadIdx.x; x < s.len; x += (long long)gridDim.x * blockDim.x) {
        const long long g = s.g0 + x, q = g / s.Cp, k = g % s.Cp;
        long long i; int side;
        request_of(a, q, i, side);
        const int h = a.h[i], t = a.t[i], r = a.r[i];
        const bool ok = h >= 0 && h < a.E && t >= 0 && t < a.E && r >= 0 && r < a.R;
        int id = -1;
        if (ok && s.targets) id = k == 0 ? (side ? h : t) : -1;
        else if (ok && k < a.n_cand)
            id = s.mode == kList ? candidate_id<kList>(a, i, side, r, k)
                                 : (s.mode == kDrawn ? candidate_id<kDrawn>(a, i, side, r, k) : candidate_id<kDrawnTyped>(a, i, side, r, k));
        s.pc[x] = id;
        s.ph[x] = id < 0 ? 0 : (side ? id : h);
        s.pt[x] = id < 0 ? 0 : (side ? t : id);
        s.pr[x] = ok ? r : 0;
    }
}

struct CountArgs {
    RankCandArgs a;
    long long Cp, G, g0, len;
    const int32_t *pc;
    const float *sc, *tgt;   // the chunk's scores; the targets' scores, request q at q * G
};

__global__ __launch_bounds__(256) void count_kernel(CountArgs s) {
    const RankCandArgs &a = s.a;
    for (long long x = (long long)blockIdx.x * blockDim.x + threadIdx.x; x < s.len; x += (long long)gridDim.x * blockDim.x) {
        const int id = s.pc[x];
        if (id < 0) continue;
        const long long q = (s.g0 + x) / s.Cp;
        long long i; int side;
        request_of(a, q, i, side);
        const int fixed = side ? a.t[i] : a.h[i], target = side ? a.h[i] : a.t[i];
        if (id == target || !(s.sc[x] < s.tgt[q * s.G])) continue;
        bool known = false;
        if (a.filtered) {
            const int4 *known_arr = side ? a.ev.all_t : a.ev.all;
            long long lo, hi;
            pair_range(known_arr, a.ev.n_all, fixed, a.r[i], lo, hi);
            known = in_range(known_arr, lo, hi, id);
        }
        unsigned long long *out = (unsigned long long *)(a.counts + (2 * i + side) * 2);
        atomicAdd(out, 1ULL);
        if (!known) atomicAdd(out + 1, 1ULL);
    }
}

// workspace of the two-stage form, grown on demand; this file's own
DevBuf<int32_t> g_ids;
DevBuf<float> g_sc, g_tgt;

unsigned blocks_for(long long len) { return (unsigned)std::max(1LL, std::min((len + 255) / 256, 8192LL)); }

// bf16: a.ent / a.rel are stored bf16 tables (kge_rank_candidates_bf16) and `tables` is not read
int score_pairs(const kge_model_desc &m, bool bf16, const float *const tables[4], const RankCandArgs &a, const int32_t *ph, const int32_t *pt,
                const int32_t *pr, long long len, float *out, hipStream_t stream) {
    if (bf16) return launch_predict_bf16(m, (const uint16_t *)a.ent, (const uint16_t *)a.rel, ph, pt, pr, len, out, stream);
    if (m.model == KGE_TRANSR) return launch_predict_transr_grouped(m, tables, ph, pt, pr, len, out, stream);
    return launch_predict(m, tables, ph, pt, pr, len, out, stream);
}

int two_stage(const kge_model_desc &m, bool bf16, const float *const tables[4], const RankCandArgs &a, int mode, hipStream_t stream) {
    const bool tr = m.model == KGE_TRANSR;
    const long long G = tr ? 16 : 1;
    const long long Cp = (a.n_cand + G - 1) / G * G;
    // pairs per chunk: 2^22, fewer while TransR's projections (two rows of rel_dim floats per pair) would pass 1 GiB
    long long chunk = 1LL << 22;
    if (tr) chunk = std::max(16LL, std::min(chunk, ((1LL << 30) / (8LL * m.rel_dim)) / 16 * 16));
    int rc;
    if ((rc = g_ids.reserve(4 * chunk, "alloc rank candidate pairs"))) return rc;
    if ((rc = g_sc.reserve(chunk, "alloc rank candidate scores"))) return rc;
    if ((rc = g_tgt.reserve(a.n_req * G, "alloc rank candidate targets"))) return rc;
    SpellArgs sp = {};
    sp.a = a; sp.mode = mode;
    sp.ph = g_ids; sp.pt = g_ids + chunk; sp.pr = g_ids + 2 * chunk; sp.pc = g_ids + 3 * chunk;
    // the true triples' scores
    sp.targets = 1; sp.Cp = G;
    for (long long g0 = 0; g0 < a.n_req * G; g0 += chunk) {
        sp.g0 = g0; sp.len = std::min(chunk, a.n_req * G - g0);
        hipLaunchKernelGGL(spell_kernel, dim3(blocks_for(sp.len)), dim3(256), 0, stream, sp);
        if ((rc = score_pairs(m, bf16, tables, a, sp.ph, sp.pt, sp.pr, sp.len, g_tgt + g0, stream))) return rc;
    }
    sp.targets = 0; sp.Cp = Cp;
    CountArgs ca = {};
    ca.a = a; ca.Cp = Cp; ca.G = G; ca.pc = sp.pc; ca.sc = g_sc; ca.tgt = g_tgt;
    const long long total = a.n_req * Cp;
    for (long long g0 = 0; g0 < total; g0 += chunk) {
        sp.g0 = ca.g0 = g0; sp.len = ca.len = std::min(chunk, total - g0);
        hipLaunchKernelGGL(spell_kernel, dim3(blocks_for(sp.len)), dim3(256), 0, stream, sp);
        if ((rc = score_pairs(m, bf16, tables, a, sp.ph, sp.pt, sp.pr, sp.len, g_sc, stream))) return rc;
        hipLaunchKernelGGL(count_kernel, dim3(blocks_for(ca.len)), dim3(256), 0, stream, ca);
    }
    return hip_check(hipGetLastError(), "rank candidates two-stage launch");
}

// kge_rank_candidates (`tables`) and kge_rank_candidates_bf16 (`bf16`: tables == nullptr, d_ent / d_rel are stored bf16 rows): one
// argument path, one order of checks
int rank_candidates_call(const std::string &who, bool bf16, const kge_model_desc *m, const float *const tables[KGE_MAX_TABLES],
                         const uint16_t *d_ent, const uint16_t *d_rel, const int32_t *d_h, const int32_t *d_t, const int32_t *d_r, INT n,
                         const int32_t *d_tail_cand, INT tail_stride, const int32_t *d_head_cand, INT head_stride, INT n_cand, INT flags,
                         uint64_t seed, int64_t *d_counts, hipStream_t stream) {
    if (!m || (bf16 ? !d_ent || !d_rel : !tables) || !d_h || !d_t || !d_r || !d_counts) return fail(KGE_ERR_BAD_ARG, who + ": null model, tables, triple or output array");
    if (n < 0 || n >= (INT(1) << 30)) return fail(KGE_ERR_BAD_ARG, who + ": triple count outside [0, 2^30)");
    if (n_cand < 0 || n_cand >= (INT(1) << 31)) return fail(KGE_ERR_BAD_ARG, who + ": candidate count outside [0, 2^31)");
    if (flags & ~(INT)(KGE_RANKC_FILTERED | KGE_RANKC_DRAWN | KGE_RANKC_TYPED | KGE_RANKC_NO_HEAD)) return fail(KGE_ERR_BAD_ARG, who + ": unknown flags");
    const bool drawn = flags & KGE_RANKC_DRAWN, typed = flags & KGE_RANKC_TYPED, no_head = flags & KGE_RANKC_NO_HEAD, filtered = flags & KGE_RANKC_FILTERED;
    if (drawn && (d_tail_cand || d_head_cand)) return fail(KGE_ERR_BAD_ARG, who + ": a candidate list together with KGE_RANKC_DRAWN");
    if (!drawn && (typed || no_head)) return fail(KGE_ERR_BAD_ARG, who + ": KGE_RANKC_TYPED / KGE_RANKC_NO_HEAD without KGE_RANKC_DRAWN");
    if (!drawn && !d_tail_cand && !d_head_cand) return fail(KGE_ERR_BAD_ARG, who + ": no candidate list and no KGE_RANKC_DRAWN");
    if ((d_tail_cand && tail_stride != 0 && tail_stride < n_cand) || (d_head_cand && head_stride != 0 && head_stride < n_cand))
        return fail(KGE_ERR_BAD_ARG, who + ": a list stride must be 0 (shared list) or at least n_cand");
    bool known_model = for_model(m->model, [](auto) {});
    if (!known_model) return fail(KGE_ERR_BAD_ARG, "unknown model id");
    const int64_t E = m->ent_total;
    const int D = m->model == KGE_TRANSR ? (int)m->rel_dim : (int)m->ent_dim;
    if (D < 1 || m->ent_dim < 1 || E < 1 || E >= (INT(1) << 31) || m->rel_total < 1) return fail(KGE_ERR_BAD_ARG, who + ": empty model");
    if (D > 1024) return fail(KGE_ERR_UNSUPPORTED, who + ": embedding dimension > 1024");
    if (bf16)
        if (const char *why = bf16_eval_refusal(m)) return fail(KGE_ERR_UNSUPPORTED, who + ": " + why);
    if (!device_ok()) return fail(KGE_ERR_NO_DEVICE, who + ": no usable HIP device");
    RankCandArgs a = {};
    int rc;
    if ((filtered || typed) && (rc = eval_filter_view(typed, a.ev))) return rc;
    const int n_tables = m->model == KGE_TRANSE ? 2 : (m->model == KGE_TRANSD ? 4 : 3);
    for (int k = 0; k < n_tables && !bf16; k++)
        if (!tables[k]) return fail(KGE_ERR_BAD_ARG, who + ": null table");
    if (n == 0) return KGE_OK;
    if ((rc = hip_check(hipMemsetAsync(d_counts, 0, sizeof(int64_t) * 4 * (size_t)n, stream), "zero rank candidate counts"))) return rc;
    if (n_cand == 0) return KGE_OK;
    if (bf16) { a.ent = d_ent; a.rel = d_rel; }
    else { a.ent = tables[0]; a.rel = tables[1]; a.auxr = tables[2]; a.auxe = tables[3]; }
    a.h = d_h; a.t = d_t; a.r = d_r;
    a.cand[0] = d_tail_cand; a.cand[1] = d_head_cand; a.stride[0] = tail_stride; a.stride[1] = head_stride;
    const bool tail_side = drawn || d_tail_cand, head_side = drawn ? !no_head : d_head_cand != nullptr;
    a.nsides = tail_side && head_side ? 2 : 1;
    a.side0 = tail_side ? 0 : 1;
    a.n = n; a.n_req = n * a.nsides; a.n_cand = n_cand;
    a.E = E; a.R = m->rel_total; a.D = D;
    a.filtered = filtered; a.seed = seed; a.counts = (long long *)d_counts;
    const int mode = !drawn ? kList : (typed ? kDrawnTyped : kDrawn);
    if (m->model == KGE_TRANSR || !engine().rankc_fused) {
        a.atomic = 1;
        return two_stage(*m, bf16, tables, a, mode, stream);
    }
    if (bf16) return launch_fused<KGE_TRANSE, true>(a, mode, stream);
    switch (m->model) {
        case KGE_TRANSE: return launch_fused<KGE_TRANSE>(a, mode, stream);
        case KGE_TRANSH: return launch_fused<KGE_TRANSH>(a, mode, stream);
        default: return launch_fused<KGE_TRANSD>(a, mode, stream);
    }
}

}  // namespace

}  // namespace kge

using namespace kge;

extern "C" int kge_rank_candidates(const kge_model_desc *m, const float *const tables[KGE_MAX_TABLES], const int32_t *d_h, const int32_t *d_t,
                                   const int32_t *d_r, INT n, const int32_t *d_tail_cand, INT tail_stride, const int32_t *d_head_cand,
                                   INT head_stride, INT n_cand, INT flags, uint64_t seed, int64_t *d_counts, void *stream) {
    return rank_candidates_call("kge_rank_candidates", false, m, tables, nullptr, nullptr, d_h, d_t, d_r, n, d_tail_cand, tail_stride, d_head_cand,
                                head_stride, n_cand, flags, seed, d_counts, (hipStream_t)stream);
}

extern "C" int kge_rank_candidates_bf16(const kge_model_desc *m, const uint16_t *d_ent, const uint16_t *d_rel, const int32_t *d_h,
                                        const int32_t *d_t, const int32_t *d_r, INT n, const int32_t *d_tail_cand, INT tail_stride,
                                        const int32_t *d_head_cand, INT head_stride, INT n_cand, INT flags, uint64_t seed, int64_t *d_counts,
                                        void *stream) {
    return rank_candidates_call("kge_rank_candidates_bf16", true, m, nullptr, d_ent, d_rel, d_h, d_t, d_r, n, d_tail_cand, tail_stride, d_head_cand,
                                head_stride, n_cand, flags, seed, d_counts, (hipStream_t)stream);
}

extern "C" int kge_rank_candidates_range(const kge_model_desc *m, const float *const tables[KGE_MAX_TABLES], INT row_lo, INT rows,
                                         const float *d_query_rows, const int32_t *d_h, const int32_t *d_t, const int32_t *d_r, INT n,
                                         const int32_t *d_tail_cand, INT tail_stride, const int32_t *d_head_cand, INT head_stride,
                                         INT n_cand, INT flags, uint64_t seed, int64_t *d_counts, void *stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (!m || !tables || !d_h || !d_t || !d_r || !d_counts) return fail(KGE_ERR_BAD_ARG, "kge_rank_candidates_range: null model, tables, triple or output array");
    if (n < 0 || n >= (INT(1) << 30)) return fail(KGE_ERR_BAD_ARG, "kge_rank_candidates_range: triple count outside [0, 2^30)");
    if (n_cand < 0 || n_cand >= (INT(1) << 31)) return fail(KGE_ERR_BAD_ARG, "kge_rank_candidates_range: candidate count outside [0, 2^31)");
    if (flags & ~(INT)(KGE_RANKC_FILTERED | KGE_RANKC_DRAWN | KGE_RANKC_TYPED | KGE_RANKC_NO_HEAD)) return fail(KGE_ERR_BAD_ARG, "kge_rank_candidates_range: unknown flags");
    const bool drawn = flags & KGE_RANKC_DRAWN, typed = flags & KGE_RANKC_TYPED, no_head = flags & KGE_RANKC_NO_HEAD, filtered = flags & KGE_RANKC_FILTERED;
    if (drawn && (d_tail_cand || d_head_cand)) return fail(KGE_ERR_BAD_ARG, "kge_rank_candidates_range: a candidate list together with KGE_RANKC_DRAWN");
    if (!drawn && (typed || no_head)) return fail(KGE_ERR_BAD_ARG, "kge_rank_candidates_range: KGE_RANKC_TYPED / KGE_RANKC_NO_HEAD without KGE_RANKC_DRAWN");
    if (!drawn && !d_tail_cand && !d_head_cand) return fail(KGE_ERR_BAD_ARG, "kge_rank_candidates_range: no candidate list and no KGE_RANKC_DRAWN");
    if ((d_tail_cand && tail_stride != 0 && tail_stride < n_cand) || (d_head_cand && head_stride != 0 && head_stride < n_cand))
        return fail(KGE_ERR_BAD_ARG, "kge_rank_candidates_range: a list stride must be 0 (shared list) or at least n_cand");
    bool known_model = for_model(m->model, [](auto) {});
    if (!known_model) return fail(KGE_ERR_BAD_ARG, "unknown model id");
    if (m->model != KGE_TRANSE) return fail(KGE_ERR_UNSUPPORTED, "kge_rank_candidates_range: TransE only");
    const int64_t E = m->ent_total;
    const int D = (int)m->ent_dim;
    if (m->ent_dim < 1 || E < 1 || E >= (INT(1) << 31) || m->rel_total < 1) return fail(KGE_ERR_BAD_ARG, "kge_rank_candidates_range: empty model");
    if (m->ent_dim > 1024) return fail(KGE_ERR_UNSUPPORTED, "kge_rank_candidates_range: embedding dimension > 1024");
    if (row_lo < 0 || rows < 0 || row_lo > E || rows > E - row_lo) return fail(KGE_ERR_BAD_ARG, "kge_rank_candidates_range: row range outside the entity table");
    if (n > 0 && !d_query_rows) return fail(KGE_ERR_BAD_ARG, "kge_rank_candidates_range: null query rows");
    if (!device_ok()) return fail(KGE_ERR_NO_DEVICE, "kge_rank_candidates_range: no usable HIP device");
    RankCandRangeArgs a = {};
    int rc;
    if ((filtered || typed) && (rc = eval_filter_view(typed, a.ev))) return rc;
    if (!tables[1] || (rows > 0 && !tables[0])) return fail(KGE_ERR_BAD_ARG, "kge_rank_candidates_range: null table");
    if (n == 0) return KGE_OK;
    if ((rc = hip_check(hipMemsetAsync(d_counts, 0, sizeof(int64_t) * 4 * (size_t)n, stream), "zero rank candidate range counts"))) return rc;
    if (n_cand == 0 || rows == 0) return KGE_OK;
    a.ent = tables[0]; a.rel = tables[1];
    a.qrows = d_query_rows; a.row_lo = row_lo; a.rows = rows;
    a.h = d_h; a.t = d_t; a.r = d_r;
    a.cand[0] = d_tail_cand; a.cand[1] = d_head_cand; a.stride[0] = tail_stride; a.stride[1] = head_stride;
    const bool tail_side = drawn || d_tail_cand, head_side = drawn ? !no_head : d_head_cand != nullptr;
    a.nsides = tail_side && head_side ? 2 : 1;
    a.side0 = tail_side ? 0 : 1;
    a.n = n; a.n_req = n * a.nsides; a.n_cand = n_cand;
    a.E = E; a.R = m->rel_total; a.D = D;
    a.filtered = filtered; a.seed = seed; a.counts = (long long *)d_counts;
    return launch_range(a, !drawn ? kList : (typed ? kDrawnTyped : kDrawn), stream);
}
