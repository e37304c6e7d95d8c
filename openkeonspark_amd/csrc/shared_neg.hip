// TransE on negatives SHARED by a chunk of positives (NON-PARITY, opt-in; the definition is in include/kge_mi355.h).
//
// A chunk of P consecutive positives scores the same N candidate entities, so it gathers 3 P + N table rows instead of
// P (3 + N); the P x N distances are formed on chip.  Two kernels:
//
//   shared_draw_kernel   one thread per (positive, candidate) pair and per candidate: the counter hashes of the definition, and the
//                        mask -- is the corrupted triple a training triple? -- by the sampler's bisection (sampler_dev.hpp
//                        bisect_count) in the sorted tails of (h, r) / heads of (t, r).  The sampler finds those lists through the
//                        training triple it picked; here only the ids are known, so the (h, r) and (t, r) groups are found by the
//                        same bisection in a directory of the groups' keys (GroupDir: one key and one span per group of the
//                        index, taken from its group records once per imported training set).
//   shared_emit_kernel   one workgroup per chunk.  The chunk's candidates are normalised once into LDS (tiles of T candidates
//                        when N rows do not fit the budget); a wave then owns one positive at a time -- h, t, r normalised in
//                        registers, lane l holding elements 4 (l + 64 q) .. + 3 -- and walks the tile: distance from the LDS row,
//                        one wave reduction, hinge.  An active pair adds its signs to the positive's three integer vectors in
//                        registers and, transposed, to the candidate's: one LDS add per dword on byte fields that hold
//                        sum (g + 1), g in {-1, 0, 1} -- at most 2 P <= 254, so no field carries into its neighbour -- from which
//                        the tile's end subtracts the candidate's number of active pairs.  Records leave in
//                        kge_transe_emit_records' format for the width's team shape (natural element order at multiples of 4,
//                        the strided team order elsewhere), through an element-ordered byte image in LDS.
//                        With more than one tile a positive's records are completed tile by tile: the wave that wrote them adds
//                        the next tile's share to its own earlier stores.
// The loss is summed per wave in candidate order, per chunk in wave order and over the chunks in index order: a step is
// reproducible bit for bit.
// Chunk membership is a property of the GLOBAL batch position: position p belongs to chunk p / P.  The `_at` entry points take a
// call that begins at any position -- a rank's slice of the batch -- so its first and last chunks may be partial; both kernels
// carry that as one offset (first_position % P, zero for the older entry points) in their chunk arithmetic.
// RELATION-GROUPED chunks (kge_shared_order_by_relation / kge_shared_negatives_draw_grouped / kge_transe_emit_records_shared_chunks;
// the section near the end of this file): the batch is ordered by relation, chunks never cross a relation boundary and are
// stated by a table of (first sorted position, length); a candidate has one side for its chunk and may come from the relation's
// type list.  The emit kernel is the same body with its positions read from the table (template parameter TABLE).
// IN-CHUNK candidates (kge_shared_negatives_draw_grouped_mixed, behind the grouped draw): K more columns of a chunk's lists are the
// chunk's own heads / tails at rotated positions; a sibling of the grouped draw kernel writes them, the emit kernels take the wider
// lists as they take any.
// bf16 TABLES (kge_transe_emit_records_shared_bf16 / _shared_chunks_bf16; include/kge_mi355.h, "Shared negatives on bf16 tables"): the
// emit kernel under BF16 reads rows of stored bf16 -- a lane's four elements in one 8-byte load, widened exactly -- and is the
// fp32 kernel from there on, so it writes what that kernel writes on the widened tables bit for bit.
#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

#include <rocprim/rocprim.hpp>

#include "bf16_dev.hpp"
#include "engine.hpp"
#include "mix_dev.hpp"
#include "sampler_dev.hpp"
#include "team.hpp"

namespace kge {

void transe_team_shape(int D, int &L, int &C);   // models.hip

namespace {

// ---- the (h, r) / (t, r) groups of the index by key ------------------------------------------------
struct GroupDir {
    DevBuf<long long> hr_key, tr_key;    // anchor * rel_total + relation, increasing
    DevBuf<int2> hr_span, tr_span;       // (offset, length) into tails_hr / heads_tr
    int n_hr = 0, n_tr = 0;
    unsigned long long generation = ~0ull;
};
GroupDir g_dir;
DevBuf<float> g_partials;

int ensure_group_dir() {
    Engine &e = engine();
    if (g_dir.generation == e.index_generation && g_dir.hr_key) return KGE_OK;
    const KgIndex &ix = e.index;
    struct Ent { long long key; int off, len; };
    std::vector<Ent> hr((size_t)ix.train_dup), tr((size_t)ix.train_dup);
    for (int64_t i = 0; i < ix.train_dup; i++) {
        const Int4 &p = ix.pos[(size_t)i], &g = ix.grp[(size_t)i];
        hr[(size_t)i] = {(long long)p.x * ix.rel_total + p.z, g.x, g.y};
        tr[(size_t)i] = {(long long)p.y * ix.rel_total + p.z, g.z, g.w};
    }
    int rc;
    auto put = [&](std::vector<Ent> &v, DevBuf<long long> &keys, DevBuf<int2> &spans, int &n) -> int {
        std::sort(v.begin(), v.end(), [](const Ent &a, const Ent &b) { return a.key < b.key; });
        v.erase(std::unique(v.begin(), v.end(), [](const Ent &a, const Ent &b) { return a.key == b.key; }), v.end());
        std::vector<long long> k(v.size());
        std::vector<Int2> s(v.size());
        for (size_t i = 0; i < v.size(); i++) { k[i] = v[i].key; s[i] = {v[i].off, v[i].len}; }
        n = (int)v.size();
        if ((rc = keys.upload(k, "upload group keys"))) return rc;
        return spans.upload(s, "upload group spans");
    };
    g_dir.generation = ~0ull;
    if ((rc = put(hr, g_dir.hr_key, g_dir.hr_span, g_dir.n_hr))) return rc;
    if ((rc = put(tr, g_dir.tr_key, g_dir.tr_span, g_dir.n_tr))) return rc;
    g_dir.generation = e.index_generation;
    return KGE_OK;
}

struct DrawArgs {
    const int32_t *h, *t, *r;
    long long n_pos, first_position, n_chunks;
    int P, N;
    unsigned long long S;            // the step key
    int ent_total, rel_total, bern;
    const float *bern_prob;
    const int32_t *tails_hr, *heads_tr;
    const long long *hr_key, *tr_key;
    const int2 *hr_span, *tr_span;
    int n_hr, n_tr;
    int32_t *cand;
    uint8_t *pair;
};

__device__ __forceinline__ int shared_candidate(unsigned long long S, long long chunk, int k, int ent_total) {
    const unsigned long long c = ((unsigned long long)chunk << 8) | (unsigned long long)k;
    return (int)mix_scale(mix64(S + (c + 1ULL) * kMixGamma), (unsigned long long)ent_total);
}

__global__ __launch_bounds__(256) void shared_draw_kernel(DrawArgs a) {
    const long long n_pair = a.n_pos * a.N, n_all = n_pair + a.n_chunks * a.N;
    const long long chunk0 = a.first_position / a.P;
    const long long off = a.first_position - chunk0 * a.P;      // positions of global chunk chunk0 that lie before the call's first
    for (long long g = (long long)blockIdx.x * 256 + threadIdx.x; g < n_all; g += (long long)gridDim.x * 256) {
        if (g >= n_pair) {
            const long long j = (g - n_pair) / a.N;
            const int k = (int)((g - n_pair) % a.N);
            a.cand[g - n_pair] = shared_candidate(a.S, chunk0 + j, k, a.ent_total);
            continue;
        }
        const long long b = g / a.N;
        const int k = (int)(g % a.N);
        const int c = shared_candidate(a.S, chunk0 + (off + b) / a.P, k, a.ent_total);
        const int h = a.h[b], t = a.t[b], r = a.r[b];
        const bool r_ok = r >= 0 && r < a.rel_total;
        // the head-or-tail coin of sample_slot with v in the place of rand % 1000: same threshold, same float comparison
        const unsigned long long pc = ((unsigned long long)(a.first_position + b) << 8) | 128ULL | (unsigned long long)k;
        const unsigned long long v = mix_scale(mix64(a.S + (pc + 1ULL) * kMixGamma), 1000ULL);
        const float prob = (a.bern && r_ok) ? a.bern_prob[r] : 500.0f;
        const bool keep_head = (float)v < prob;      // true: new tail
        const int anchor = keep_head ? h : t;
        bool masked = false;
        if (r_ok && anchor >= 0 && anchor < a.ent_total) {
            const long long key = (long long)anchor * a.rel_total + r;
            const long long *keys = keep_head ? a.hr_key : a.tr_key;
            const int n = keep_head ? a.n_hr : a.n_tr;
            const int at = bisect_count(n, [&](int mid) { return keys[mid] < key; });
            if (at < n && keys[at] == key) {
                const int2 sp = (keep_head ? a.hr_span : a.tr_span)[at];
                masked = sorted_contains((keep_head ? a.tails_hr : a.heads_tr) + sp.x, sp.y, c);
            }
        }
        a.pair[g] = (uint8_t)((keep_head ? 0 : 1) | (masked ? 2 : 0));
    }
}

// ---- the emit kernel -----------------------------------------------------------------------------
struct SharedEmitArgs {
    const float *ent, *rel;      // (BF16 instantiations: rows of D stored bf16, uint16_t each)
    const int32_t *h, *t, *r;
    const int32_t *cand;
    const uint8_t *pair;
    long long n_pos, n_chunks;
    int off;                     // first_position % P: workgroup j holds the call's positions [j P - off, (j + 1) P - off)
    int P, N, T, n_tiles;        // candidates per tile, tiles
    int D, RS;                   // width; LDS row stride in floats (D rounded up to 4)
    int RD, L, nat;              // record dwords; the width's team shape; natural element order
    int ent_total, rel_total;
    float margin;
    uint32_t *rec;
    int32_t *dst;
    float *partials;
    const int2 *chunks;          // TABLE instantiations: [gridDim.x] (first position, length) per workgroup
};

__device__ __forceinline__ uint32_t padd8(uint32_t x, uint32_t y) {  // per-byte add, no carry across bytes
    return ((x & 0x7F7F7F7Fu) + (y & 0x7F7F7F7Fu)) ^ ((x ^ y) & 0x80808080u);
}
// element held by byte j of record dword w
__device__ __forceinline__ int record_element(const SharedEmitArgs &a, int w, int j) {
    return a.nat ? 4 * w + j : (w % a.L) + a.L * (4 * (w / a.L) + j);
}
__device__ __forceinline__ void wave_lds_order() {   // LDS traffic inside one wave: stores before the loads that follow
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}
__device__ __forceinline__ int sgn_i(float e) { return (e > 0.f ? 1 : 0) - (e < 0.f ? 1 : 0); }

// TABLE: workgroup j reads its positions from a.chunks[j] (relation-grouped chunks, kge_transe_emit_records_shared_chunks) instead
// of computing them from j, P and off; a slot of length 0 blanks its N candidate keys, leaves a zero partial and is done.
// BF16: a.ent / a.rel are bf16 tables (widths that are multiples of 8, so VEC): load_row widens, nothing else differs.
template <int Q, bool VEC, bool TABLE = false, bool BF16 = false>
__global__ __launch_bounds__(256) void shared_emit_kernel(SharedEmitArgs a) {
    static_assert(!BF16 || VEC, "bf16 rows are read four elements at a time");
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
    const int T = a.T, RS = a.RS, D = a.D;
    float *crow = reinterpret_cast<float *>(lds);                                  // [T][RS] normalised candidate rows
    uint32_t *ccnt = reinterpret_cast<uint32_t *>(lds + (size_t)T * RS * 4);       // [T][RS / 4] byte fields sum (g + 1)
    int *nact = reinterpret_cast<int *>(lds + (size_t)T * RS * 5);                 // [T] active pairs
    int *cid = nact + T;                                                           // [T] id, -1 = outside the table
    uint8_t *stage_all = reinterpret_cast<uint8_t *>(cid + T);                     // [4 waves][3][RS] element-ordered bytes
    float *wl = reinterpret_cast<float *>(stage_all + 4 * 3 * RS);                 // [4] wave losses
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint8_t *stage = stage_all + wave * 3 * RS;
    const long long j = blockIdx.x;
    long long b0;
    int Pc;
    if constexpr (TABLE) {
        const int2 c = a.chunks[j];
        const bool in = c.x >= 0 && c.x < a.n_pos && c.y > 0;       // (a slot that points outside the call is an empty one)
        b0 = in ? c.x : 0;
        Pc = in ? (int)min((long long)c.y, a.n_pos - b0) : 0;
        if (Pc == 0) {
            if ((int)threadIdx.x < a.N) a.dst[3 * a.n_pos + j * a.N + threadIdx.x] = -1;
            if (threadIdx.x == 0) a.partials[j] = 0.f;
            return;
        }
    } else {
        b0 = max(0LL, j * a.P - a.off);
        Pc = (int)(min(a.n_pos, (j + 1) * a.P - a.off) - b0);
    }
    bool valid[Q];
#pragma unroll
    for (int q = 0; q < Q; q++) valid[q] = 4 * (lane + 64 * q) < RS;
    auto load_row = [&](const float *__restrict__ tab, long long row, float (&x)[4 * Q]) {
        if constexpr (BF16) {      // elements e0 .. e0 + 3 are two dwords of the stored row: (e0, e0 + 1) and (e0 + 2, e0 + 3)
            const uint16_t *p = reinterpret_cast<const uint16_t *>(tab) + row * D;
#pragma unroll
            for (int q = 0; q < Q; q++) {
                const int e0 = 4 * (lane + 64 * q);
                const uint2 v = valid[q] ? *reinterpret_cast<const uint2 *>(p + e0) : make_uint2(0u, 0u);
                x[4 * q] = bf16_widen_lo(v.x); x[4 * q + 1] = bf16_widen_hi(v.x);
                x[4 * q + 2] = bf16_widen_lo(v.y); x[4 * q + 3] = bf16_widen_hi(v.y);
            }
            return;
        }
        const float *p = tab + row * D;
#pragma unroll
        for (int q = 0; q < Q; q++) {
            const int e0 = 4 * (lane + 64 * q);
            if constexpr (VEC) {
                const float4 v = valid[q] ? *reinterpret_cast<const float4 *>(p + e0) : make_float4(0.f, 0.f, 0.f, 0.f);
                x[4 * q] = v.x; x[4 * q + 1] = v.y; x[4 * q + 2] = v.z; x[4 * q + 3] = v.w;
            } else {
#pragma unroll
                for (int i = 0; i < 4; i++) x[4 * q + i] = e0 + i < D ? p[e0 + i] : 0.f;
            }
        }
    };
    auto normalise = [&](float (&x)[4 * Q]) {
        float ss = 0.f;
#pragma unroll
        for (int c = 0; c < 4 * Q; c++) ss = __builtin_fmaf(x[c], x[c], ss);
        ss = team_sum<64>(ss);
        const float inv = 1.0f / sqrtf(ss >= 1e-12f ? ss : 1e-12f);
#pragma unroll
        for (int c = 0; c < 4 * Q; c++) x[c] *= inv;
    };
    float lsum = 0.f;
    for (int tile = 0; tile < a.n_tiles; tile++) {
        const int k0 = tile * T;
        const int Tc = min(T, a.N - k0);
        // ---- the tile's candidates: normalised rows into LDS, counters cleared ----
        for (int i = threadIdx.x; i < T * (RS / 4); i += 256) ccnt[i] = 0;
        if ((int)threadIdx.x < T) nact[threadIdx.x] = 0;
        for (int kt = wave; kt < Tc; kt += 4) {
            const int id = a.cand[j * a.N + k0 + kt];
            const bool ok = id >= 0 && id < a.ent_total;
            float x[4 * Q];
            load_row(a.ent, ok ? id : 0, x);
            normalise(x);
#pragma unroll
            for (int q = 0; q < Q; q++)
                if (valid[q])
                    *reinterpret_cast<float4 *>(crow + (size_t)kt * RS + 4 * (lane + 64 * q)) =
                        ok ? make_float4(x[4 * q], x[4 * q + 1], x[4 * q + 2], x[4 * q + 3]) : make_float4(0.f, 0.f, 0.f, 0.f);
            if (lane == 0) cid[kt] = ok ? id : -1;
        }
        __syncthreads();
        // ---- positives: one wave each ----
        for (int pp = wave; pp < Pc; pp += 4) {
            const long long b = b0 + pp;
            const int h = a.h[b], t = a.t[b], r = a.r[b];
            const bool ids_ok = h >= 0 && h < a.ent_total && t >= 0 && t < a.ent_total && r >= 0 && r < a.rel_total;
            int my_pb = 2;
            if (lane < Tc) my_pb = a.pair[b * a.N + k0 + lane];
            float B0[4 * Q], B1[4 * Q];       // new head: e = c^ + (r^ - t^);  new tail: e = (h^ + r^) - c^
            int sp[4 * Q], Ah[4 * Q], At[4 * Q], Ar[4 * Q];
            float p_score;
            {
                float H[4 * Q], Tn[4 * Q], R[4 * Q];
                load_row(a.ent, ids_ok ? h : 0, H); load_row(a.ent, ids_ok ? t : 0, Tn); load_row(a.rel, ids_ok ? r : 0, R);
                normalise(H); normalise(Tn); normalise(R);
                float acc = 0.f;
#pragma unroll
                for (int c = 0; c < 4 * Q; c++) {
                    B0[c] = R[c] - Tn[c];
                    B1[c] = H[c] + R[c];
                    const float e = H[c] + R[c] - Tn[c];
                    acc += fabsf(e);
                    sp[c] = sgn_i(e);
                    Ah[c] = 0; At[c] = 0; Ar[c] = 0;
                }
                p_score = team_sum<64>(acc);
            }
            int cnt = 0;
            if (ids_ok) {
                for (int kt = 0; kt < Tc; kt++) {
                    const int pb = __builtin_amdgcn_readlane(my_pb, kt);
                    if ((pb & 2) || cid[kt] < 0) continue;
                    const bool new_head = pb & 1;
                    float e[4 * Q];
                    float acc = 0.f;
#pragma unroll
                    for (int q = 0; q < Q; q++) {
                        float4 c4 = make_float4(0.f, 0.f, 0.f, 0.f);
                        if (valid[q]) c4 = *reinterpret_cast<const float4 *>(crow + (size_t)kt * RS + 4 * (lane + 64 * q));
                        const float cv[4] = {c4.x, c4.y, c4.z, c4.w};
#pragma unroll
                        for (int i = 0; i < 4; i++) {
                            const int c = 4 * q + i;
                            e[c] = new_head ? cv[i] + B0[c] : B1[c] - cv[i];
                            acc += fabsf(e[c]);
                        }
                    }
                    const float n_score = team_sum<64>(acc);
                    const float v = p_score - n_score + a.margin;
                    if (!(v >= 0.f)) continue;     // a tie is active
                    cnt++; lsum += v;
#pragma unroll
                    for (int q = 0; q < Q; q++) {
                        uint32_t f = 0;
#pragma unroll
                        for (int i = 0; i < 4; i++) {
                            const int c = 4 * q + i;
                            const int s = sgn_i(e[c]);
                            // new head: the candidate takes -s, the kept t +s, r -s;  new tail: the candidate +s, the kept h -s, r -s
                            const int g = new_head ? -s : s;
                            if (new_head) At[c] += s; else Ah[c] -= s;
                            Ar[c] -= s;
                            f |= (uint32_t)(g + 1) << (8 * i);
                        }
                        if (valid[q]) atomicAdd(ccnt + (size_t)kt * (RS / 4) + lane + 64 * q, f);
                    }
                    if (lane == 0) atomicAdd(nact + kt, 1);
                }
            }
            // ---- the positive's three records: this tile's share, in element order, then in the record's dword order ----
#pragma unroll
            for (int q = 0; q < Q; q++) {
                if (!valid[q]) continue;
                uint32_t wh = 0, wt = 0, wr = 0;
#pragma unroll
                for (int i = 0; i < 4; i++) {
                    const int c = 4 * q + i, v = cnt * sp[c];
                    wh |= (uint32_t)((Ah[c] + v) & 0xFF) << (8 * i);
                    wt |= (uint32_t)((At[c] - v) & 0xFF) << (8 * i);
                    wr |= (uint32_t)((Ar[c] + v) & 0xFF) << (8 * i);
                }
                uint32_t *s32 = reinterpret_cast<uint32_t *>(stage);
                s32[lane + 64 * q] = wh; s32[RS / 4 + lane + 64 * q] = wt; s32[2 * (RS / 4) + lane + 64 * q] = wr;
            }
            wave_lds_order();
            const bool last = tile == a.n_tiles - 1;
            bool any[3] = {false, false, false};
#pragma unroll
            for (int s = 0; s < 3; s++) {
                uint32_t *out = a.rec + ((long long)s * a.n_pos + b) * (long long)a.RD;
                for (int w = lane; w < a.RD; w += 64) {
                    uint32_t word = 0;
#pragma unroll
                    for (int i = 0; i < 4; i++) {
                        const int el = record_element(a, w, i);
                        if (el < D) word |= (uint32_t)stage[s * RS + el] << (8 * i);
                    }
                    if (tile > 0) word = padd8(word, out[w]);
                    out[w] = word;
                    any[s] = any[s] || word != 0;
                }
            }
            wave_lds_order();     // (the image is rewritten for the wave's next positive)
            if (last) {
                const bool nz_h = __ballot(any[0]) != 0, nz_t = __ballot(any[1]) != 0, nz_r = __ballot(any[2]) != 0;
                if (lane == 0) {
                    a.dst[b] = nz_h ? h : -1;
                    a.dst[a.n_pos + b] = nz_t ? t : -1;
                    a.dst[2 * a.n_pos + b] = nz_r ? a.ent_total + r : -1;
                }
            }
        }
        __syncthreads();
        // ---- the tile's candidate records ----
        for (int i = threadIdx.x; i < Tc * a.RD; i += 256) {
            const int kt = i / a.RD, w = i % a.RD;
            const int n = nact[kt];
            const uint8_t *fields = reinterpret_cast<const uint8_t *>(ccnt + (size_t)kt * (RS / 4));
            uint32_t word = 0;
#pragma unroll
            for (int q = 0; q < 4; q++) {
                const int el = record_element(a, w, q);
                if (el < D) word |= (uint32_t)(((int)fields[el] - n) & 0xFF) << (8 * q);
            }
            a.rec[(3 * a.n_pos + j * a.N + k0 + kt) * (long long)a.RD + w] = word;
        }
        if ((int)threadIdx.x < Tc) a.dst[3 * a.n_pos + j * a.N + k0 + threadIdx.x] = nact[threadIdx.x] > 0 ? cid[threadIdx.x] : -1;
        __syncthreads();
    }
    if (lane == 0) wl[wave] = lsum;
    __syncthreads();
    if (threadIdx.x == 0) a.partials[j] = ((wl[0] + wl[1]) + wl[2]) + wl[3];
}

// fixed-order sum of the chunks' partial hinge sums -> loss = sum / denom
__global__ __launch_bounds__(256) void shared_loss_kernel(const float *__restrict__ partials, long long n, float unit, float *out) {
    __shared__ float sh[256];
    float s = 0.f;
    for (long long i = threadIdx.x; i < n; i += 256) s += partials[i];
    sh[threadIdx.x] = s;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) sh[threadIdx.x] += sh[threadIdx.x + w];
        __syncthreads();
    }
    if (threadIdx.x == 0) out[0] = sh[0] * unit;
}

constexpr int kLdsBudget = 60 * 1024;   // per workgroup: two chunks per CU at the widest shapes, five at the headline shape

// The two entry points of each kernel share these: `who` names the caller in the messages, `aligned` is the older entry points'
// rule that the call begins on a chunk boundary.
int draw_call(const char *who, bool aligned, const int32_t *d_h, const int32_t *d_t, const int32_t *d_r, INT n_pos, INT first_position, INT P,
              INT N, uint64_t seed, INT step, int32_t *d_cand, uint8_t *d_pair, hipStream_t stream) {
    const std::string w(who);
    if (P < 1 || P > 127) return fail(KGE_ERR_BAD_ARG, w + ": the chunk must hold 1..127 positives (a candidate's count is within +-P, an int8)");
    if (N < 1 || N > 63) return fail(KGE_ERR_BAD_ARG, w + ": 1..63 negatives per positive (a positive's count is within +-2N, an int8)");
    if (n_pos < 0 || first_position < 0 || (aligned && first_position % P != 0) || step < 0 || !d_h || !d_t || !d_r || !d_cand || !d_pair)
        return fail(KGE_ERR_BAD_ARG, w + (aligned ? ": bad arguments (first_position must be a multiple of the chunk)" : ": bad arguments"));
    int rc = ensure_device_index();
    if (rc) return rc;
    if ((rc = ensure_group_dir())) return rc;
    if (n_pos == 0) return KGE_OK;
    Engine &e = engine();
    DrawArgs a = {};
    a.h = d_h; a.t = d_t; a.r = d_r;
    a.n_pos = n_pos; a.first_position = first_position; a.n_chunks = (first_position % P + n_pos + P - 1) / P; a.P = (int)P; a.N = (int)N;
    a.S = mix64((unsigned long long)seed + ((unsigned long long)step + 1ULL) * kMixGamma);
    a.ent_total = (int)e.index.ent_total; a.rel_total = (int)e.index.rel_total; a.bern = e.bern ? 1 : 0;
    a.bern_prob = e.dev.bern_prob; a.tails_hr = e.dev.tails_hr; a.heads_tr = e.dev.heads_tr;
    a.hr_key = g_dir.hr_key; a.tr_key = g_dir.tr_key; a.hr_span = g_dir.hr_span; a.tr_span = g_dir.tr_span;
    a.n_hr = g_dir.n_hr; a.n_tr = g_dir.n_tr;
    a.cand = d_cand; a.pair = d_pair;
    long long nb = ((n_pos + a.n_chunks) * N + 255) / 256;
    if (nb > 65536) nb = 65536;
    hipLaunchKernelGGL(shared_draw_kernel, dim3((unsigned)nb), dim3(256), 0, stream, a);
    return hip_check(hipGetLastError(), "shared negatives draw launch");
}

// what the bf16 entry points accept, as a reason where they do not (kge_bf16_shared_supported is this, host only)
const char *bf16_shared_refusal(const kge_model_desc *m, INT N) {
    if (!m) return "no model descriptor";
    if (m->model != KGE_TRANSE) return "shared negatives on bf16 tables: TransE only (the tables of TransH, TransD and TransR stay fp32)";
    if (m->negative_rel != 0) return "shared negatives on bf16 tables: relation negatives are not supported (negative_rel must be 0)";
    if (N < 1 || N > 63) return "shared negatives on bf16 tables: 1..63 negatives per positive (a positive's count is within +-2N, an int8)";
    if (m->ent_dim < 8 || m->ent_dim % 8 != 0)
        return "shared negatives on bf16 tables: a width that is a multiple of 8 (a lane reads four stored values in one 8-byte load)";
    if (m->ent_dim > 512) return "shared negatives on bf16 tables: the shared emit kernel holds embedding widths up to 512";
    if (!kge_transe_counts_supported(m, N)) return "shared negatives on bf16 tables: the sign-count path's shapes only (TransE, equal widths, rows below 2^30)";
    return nullptr;
}

// `chunks` null: chunks of P by position, as above.  Not null: the `cap` slots of a chunk table (relation-grouped chunks) -- one
// workgroup and one loss partial per slot, P and first_position unused.  bf16: d_ent / d_rel are tables of stored bf16.
int emit_call(const char *who, const kge_model_desc *m, const void *d_ent, const void *d_rel, const int32_t *d_h, const int32_t *d_t,
              const int32_t *d_r, INT n_pos, INT stride, INT first_position, INT P, const int2 *chunks, INT cap, const int32_t *d_cand, INT N,
              const uint8_t *d_pair, INT denom, uint32_t *d_rec, int32_t *d_dst, float *d_loss, hipStream_t stream, bool bf16 = false) {
    const std::string w(who);
    if (!device_ok()) return fail(KGE_ERR_NO_DEVICE, w + ": no usable HIP device");
    if (bf16)
        if (const char *why = bf16_shared_refusal(m, N)) return fail(KGE_ERR_UNSUPPORTED, w + ": " + why);
    if (!m || m->model != KGE_TRANSE) return fail(KGE_ERR_UNSUPPORTED, "shared negatives: TransE only");
    if (m->negative_rel != 0) return fail(KGE_ERR_UNSUPPORTED, "shared negatives: relation negatives are not supported (negative_rel must be 0)");
    if (!chunks && (P < 1 || P > 127)) return fail(KGE_ERR_UNSUPPORTED, "shared negatives: the chunk must hold 1..127 positives (a candidate's count is within +-P, an int8)");
    if (N < 1 || N > 63) return fail(KGE_ERR_UNSUPPORTED, "shared negatives: 1..63 negatives per positive (a positive's count is within +-2N, an int8)");
    if (!kge_transe_counts_supported(m, N)) return fail(KGE_ERR_UNSUPPORTED, "shared negatives: the sign-count path's shapes only (TransE, equal widths, rows below 2^30)");
    if (m->ent_dim > 512) return fail(KGE_ERR_UNSUPPORTED, "shared negatives: the shared emit kernel holds embedding widths up to 512");
    if (n_pos < 0 || stride < n_pos || first_position < 0 || denom <= 0 || !d_ent || !d_rel || !d_h || !d_t || !d_r || !d_cand || !d_pair || !d_rec ||
        !d_dst || !d_loss)
        return fail(KGE_ERR_BAD_ARG, w + ": bad arguments");
    if (n_pos == 0) return hip_check(hipMemsetAsync(d_loss, 0, sizeof(float), stream), "zero loss");
    const long long off = chunks ? 0 : first_position % P;
    const long long n_chunks = chunks ? cap : (off + n_pos + P - 1) / P;
    if (3 * n_pos + n_chunks * N >= (INT(1) << 31) || n_chunks >= (INT(1) << 31)) return fail(KGE_ERR_UNSUPPORTED, "shared negatives: batch too large");
    int rc = g_partials.reserve(n_chunks, "shared negatives loss partials");
    if (rc) return rc;
    SharedEmitArgs a = {};
    a.ent = static_cast<const float *>(d_ent); a.rel = static_cast<const float *>(d_rel); a.h = d_h; a.t = d_t; a.r = d_r; a.cand = d_cand; a.pair = d_pair;
    a.n_pos = n_pos; a.n_chunks = n_chunks; a.off = (int)off; a.P = (int)P; a.N = (int)N;
    a.D = m->ent_dim; a.RS = (a.D + 3) / 4 * 4;
    int L, C;
    transe_team_shape(a.D, L, C);
    a.L = L; a.RD = L * ((C + 3) / 4); a.nat = a.D % 4 == 0;
    a.ent_total = (int)m->ent_total; a.rel_total = (int)m->rel_total; a.margin = m->margin;
    a.rec = d_rec; a.dst = d_dst; a.partials = g_partials; a.chunks = chunks;
    const int per_cand = a.RS * 5 + 8, fixed = 12 * a.RS + 16;
    const int t_max = (kLdsBudget - fixed) / per_cand;     // >= 21 at width 512
    a.n_tiles = ((int)N + t_max - 1) / t_max;
    a.T = ((int)N + a.n_tiles - 1) / a.n_tiles;
    const size_t lds_bytes = (size_t)a.T * per_cand + fixed;
    const dim3 grid((unsigned)n_chunks), block(256);
    const bool vec = a.D % 4 == 0;
    if (bf16) {
        if (chunks) {
            if (a.D <= 256) hipLaunchKernelGGL((shared_emit_kernel<1, true, true, true>), grid, block, lds_bytes, stream, a);
            else hipLaunchKernelGGL((shared_emit_kernel<2, true, true, true>), grid, block, lds_bytes, stream, a);
        } else {
            if (a.D <= 256) hipLaunchKernelGGL((shared_emit_kernel<1, true, false, true>), grid, block, lds_bytes, stream, a);
            else hipLaunchKernelGGL((shared_emit_kernel<2, true, false, true>), grid, block, lds_bytes, stream, a);
        }
    } else if (chunks) {
        if (a.D <= 256) {
            if (vec) hipLaunchKernelGGL((shared_emit_kernel<1, true, true>), grid, block, lds_bytes, stream, a);
            else hipLaunchKernelGGL((shared_emit_kernel<1, false, true>), grid, block, lds_bytes, stream, a);
        } else {
            if (vec) hipLaunchKernelGGL((shared_emit_kernel<2, true, true>), grid, block, lds_bytes, stream, a);
            else hipLaunchKernelGGL((shared_emit_kernel<2, false, true>), grid, block, lds_bytes, stream, a);
        }
    } else if (a.D <= 256) {
        if (vec) hipLaunchKernelGGL((shared_emit_kernel<1, true>), grid, block, lds_bytes, stream, a);
        else hipLaunchKernelGGL((shared_emit_kernel<1, false>), grid, block, lds_bytes, stream, a);
    } else {
        if (vec) hipLaunchKernelGGL((shared_emit_kernel<2, true>), grid, block, lds_bytes, stream, a);
        else hipLaunchKernelGGL((shared_emit_kernel<2, false>), grid, block, lds_bytes, stream, a);
    }
    hipLaunchKernelGGL(shared_loss_kernel, dim3(1), dim3(256), 0, stream, (const float *)g_partials.ptr(), n_chunks, 1.0f / (float)denom, d_loss);
    return hip_check(hipGetLastError(), "shared negatives emit launch");
}

// ---- relation-grouped chunks (include/kge_mi355.h, "Shared negatives on relation-grouped chunks") -------------------------
// Order: a stable radix sort of (relation or rel_total, batch position) -- rocPRIM's, the index build's.  One kernel gathers the
// ids into sorted order and marks the run starts; a max-scan carries every position's run start; a position is a chunk start
// when its distance from the run start is a multiple of P, and a plus-scan numbers the chunks; the LAST position of a chunk
// knows its number, its first position and its length and writes the table entry.  No size branch of the engine's own (rocPRIM
// chooses its sort and scan shapes by size); every launch is sized by n_pos or cap, and n_chunks stays on the device.
struct OrderScratch {
    DevBuf<uint32_t> key, key2;
    DevBuf<int32_t> pos, start, idx;
    DevBuf<char> tmp;
};
OrderScratch g_ord;

__global__ __launch_bounds__(256) void order_keys_kernel(const int32_t *__restrict__ r, long long n, int rel_total, uint32_t *__restrict__ key,
                                                         int32_t *__restrict__ pos) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int v = r[i];
    key[i] = (v >= 0 && v < rel_total) ? (uint32_t)v : (uint32_t)rel_total;
    pos[i] = (int32_t)i;
}

__global__ __launch_bounds__(256) void order_gather_kernel(const int32_t *__restrict__ h, const int32_t *__restrict__ t, const int32_t *__restrict__ r,
                                                           const uint32_t *__restrict__ key2, const int32_t *__restrict__ perm, long long n,
                                                           int32_t *__restrict__ h2, int32_t *__restrict__ t2, int32_t *__restrict__ r2,
                                                           int32_t *__restrict__ start) {
    const long long b = (long long)blockIdx.x * 256 + threadIdx.x;
    if (b >= n) return;
    const int p = perm[b];
    h2[b] = h[p]; t2[b] = t[p]; r2[b] = r[p];
    start[b] = (b > 0 && key2[b] != key2[b - 1]) ? (int32_t)b : 0;      // (max-scanned: the first position of b's run)
}

__global__ __launch_bounds__(256) void order_flags_kernel(const int32_t *__restrict__ start, long long n, int P, int32_t *__restrict__ idx) {
    const long long b = (long long)blockIdx.x * 256 + threadIdx.x;
    if (b < n) idx[b] = (b - start[b]) % P == 0 ? 1 : 0;
}

__global__ __launch_bounds__(256) void order_table_kernel(const uint32_t *__restrict__ key2, const int32_t *__restrict__ start,
                                                          const int32_t *__restrict__ idx, long long n, long long cap, int P,
                                                          int2 *__restrict__ chunks, int32_t *__restrict__ n_chunks) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    const int total = idx[n - 1];
    if (i == 0) n_chunks[0] = total;
    if (i < n) {
        const int in_run = (int)(i - start[i]);
        const bool last = i == n - 1 || key2[i + 1] != key2[i] || (in_run + 1) % P == 0;
        const int j = idx[i] - 1;
        if (last && j >= 0 && j < cap) chunks[j] = make_int2((int)i - in_run % P, in_run % P + 1);
    }
    if (i >= total && i < cap) chunks[i] = make_int2((int)n, 0);
}

long long chunk_cap(long long n_pos, long long P, long long rel_total) {
    return (n_pos + P - 1) / P + std::min(rel_total + 1, n_pos);
}

struct GroupedDrawArgs {
    const int32_t *h, *t, *r;        // in sorted order
    const int2 *chunks;
    long long n_pos, cap;
    int N, typed;
    unsigned long long S;
    int ent_total, rel_total, bern;
    const float *bern_prob;
    const int4 *type_bounds;
    const int32_t *type_tails, *type_heads;
    const int32_t *tails_hr, *heads_tr;
    const long long *hr_key, *tr_key;
    const int2 *hr_span, *tr_span;
    int n_hr, n_tr;
    int32_t *cand;
    uint8_t *pair;
};

// side and id of candidate k of chunk j, whose relation is r (any value; outside the table: an even coin, all entities)
__device__ __forceinline__ int grouped_candidate(const GroupedDrawArgs &a, long long j, int k, int r, bool &new_tail) {
    const bool r_ok = r >= 0 && r < a.rel_total;
    const unsigned long long c = ((unsigned long long)j << 8) | (unsigned long long)k;
    const unsigned long long v = mix_scale(mix64(a.S + ((c | 128ULL) + 1ULL) * kMixGamma), 1000ULL);
    const float prob = (a.bern && r_ok) ? a.bern_prob[r] : 500.0f;
    new_tail = (float)v < prob;
    const unsigned long long z = mix64(a.S + (c + 1ULL) * kMixGamma);
    if (a.typed && r_ok) {
        const int4 tb = a.type_bounds[r];
        const int off = new_tail ? tb.x : tb.z, len = new_tail ? tb.y : tb.w;
        if (len > 0) return (new_tail ? a.type_tails : a.type_heads)[off + (int)mix_scale(z, (unsigned long long)len)];
    }
    return (int)mix_scale(z, (unsigned long long)a.ent_total);
}

__global__ __launch_bounds__(256) void grouped_draw_kernel(GroupedDrawArgs a) {
    const long long n_pair = a.n_pos * a.N, n_all = n_pair + a.cap * a.N;
    for (long long g = (long long)blockIdx.x * 256 + threadIdx.x; g < n_all; g += (long long)gridDim.x * 256) {
        bool new_tail;
        if (g >= n_pair) {
            const long long j = (g - n_pair) / a.N;
            const int k = (int)((g - n_pair) % a.N);
            const int2 ch = a.chunks[j];
            const bool used = ch.y > 0 && ch.x >= 0 && ch.x < a.n_pos;
            a.cand[g - n_pair] = used ? grouped_candidate(a, j, k, a.r[ch.x], new_tail) : -1;
            continue;
        }
        const long long b = g / a.N;
        const int k = (int)(g % a.N);
        // the chunk of sorted position b: the last used slot that begins at or before it (used slots come first, in position order)
        const int j = bisect_count((int)a.cap, [&](int mid) { const int2 ch = a.chunks[mid]; return ch.y > 0 && ch.x <= b; }) - 1;
        const int h = a.h[b], t = a.t[b], r = a.r[b];
        if (j < 0) { a.pair[g] = 2; continue; }        // (a table that does not cover b: the pair takes no part)
        const int c = grouped_candidate(a, j, k, r, new_tail);
        const bool r_ok = r >= 0 && r < a.rel_total;
        const int anchor = new_tail ? h : t;
        bool masked = false;
        if (r_ok && anchor >= 0 && anchor < a.ent_total) {
            const long long key = (long long)anchor * a.rel_total + r;
            const long long *keys = new_tail ? a.hr_key : a.tr_key;
            const int n = new_tail ? a.n_hr : a.n_tr;
            const int at = bisect_count(n, [&](int mid) { return keys[mid] < key; });
            if (at < n && keys[at] == key) {
                const int2 sp = (new_tail ? a.hr_span : a.tr_span)[at];
                masked = sorted_contains((new_tail ? a.tails_hr : a.heads_tr) + sp.x, sp.y, c);
            }
        }
        a.pair[g] = (uint8_t)((new_tail ? 0 : 1) | (masked ? 2 : 0));
    }
}

// ---- in-chunk candidates (include/kge_mi355.h, "In-chunk candidates") -------------------------------------------------------
// A sibling of grouped_draw_kernel with its own argument block, so that kernel keeps its instruction stream: the lists are
// Nt = N + K wide, columns below N are grouped_candidate's, column N + i is the entity at rotated position i of the chunk on the
// column's side.  Still a thread per pair and per candidate: a pair thread has its slot from the bisection, reads the slot's
// (first, length), hashes the rotation and gathers one more id.
struct MixedDrawArgs {
    GroupedDrawArgs g;
    int K;
};

// side of column k of slot j (grouped_candidate's coin), without an id
__device__ __forceinline__ bool grouped_side(const GroupedDrawArgs &a, long long j, int k, int r) {
    const bool r_ok = r >= 0 && r < a.rel_total;
    const unsigned long long c = ((unsigned long long)j << 8) | 128ULL | (unsigned long long)k;
    const unsigned long long v = mix_scale(mix64(a.S + (c + 1ULL) * kMixGamma), 1000ULL);
    return (float)v < ((a.bern && r_ok) ? a.bern_prob[r] : 500.0f);
}

// id of in-chunk column i of the used slot j = (first, len) whose relation is r: -1 past the chunk's length and for a relation
// outside the table (the trailing run's positives take no part, and its ids would be another relation's entities)
__device__ __forceinline__ int in_chunk_candidate(const GroupedDrawArgs &a, long long j, int2 ch, int i, int r, bool new_tail) {
    const int len = (int)min((long long)ch.y, a.n_pos - ch.x);
    if (i >= len || r < 0 || r >= a.rel_total) return -1;
    const unsigned long long c = ((unsigned long long)j << 8) | 64ULL;
    const int o = (int)mix_scale(mix64(a.S + (c + 1ULL) * kMixGamma), (unsigned long long)len);
    const long long q = ch.x + (o + i) % len;
    return (new_tail ? a.t : a.h)[q];
}

__global__ __launch_bounds__(256) void grouped_draw_mixed_kernel(MixedDrawArgs m) {
    const GroupedDrawArgs &a = m.g;
    const int Nt = a.N + m.K;
    const long long n_pair = a.n_pos * Nt, n_all = n_pair + a.cap * Nt;
    for (long long g = (long long)blockIdx.x * 256 + threadIdx.x; g < n_all; g += (long long)gridDim.x * 256) {
        bool new_tail;
        if (g >= n_pair) {
            const long long j = (g - n_pair) / Nt;
            const int k = (int)((g - n_pair) % Nt);
            const int2 ch = a.chunks[j];
            const bool used = ch.y > 0 && ch.x >= 0 && ch.x < a.n_pos;
            int id = -1;
            if (used) {
                const int r = a.r[ch.x];
                if (k < a.N) id = grouped_candidate(a, j, k, r, new_tail);
                else id = in_chunk_candidate(a, j, ch, k - a.N, r, grouped_side(a, j, k, r));
            }
            a.cand[g - n_pair] = id;
            continue;
        }
        const long long b = g / Nt;
        const int k = (int)(g % Nt);
        const int j = bisect_count((int)a.cap, [&](int mid) { const int2 ch = a.chunks[mid]; return ch.y > 0 && ch.x <= b; }) - 1;
        const int h = a.h[b], t = a.t[b], r = a.r[b];
        if (j < 0) { a.pair[g] = 2; continue; }
        int c;
        bool masked = false;
        if (k < a.N) {
            c = grouped_candidate(a, j, k, r, new_tail);
        } else {
            new_tail = grouped_side(a, j, k, r);
            c = in_chunk_candidate(a, j, a.chunks[j], k - a.N, r, new_tail);
            masked = c < 0 || c == (new_tail ? t : h);      // no candidate; the entity it would replace
        }
        const bool r_ok = r >= 0 && r < a.rel_total;
        const int anchor = new_tail ? h : t;
        if (!masked && r_ok && anchor >= 0 && anchor < a.ent_total) {
            const long long key = (long long)anchor * a.rel_total + r;
            const long long *keys = new_tail ? a.hr_key : a.tr_key;
            const int n = new_tail ? a.n_hr : a.n_tr;
            const int at = bisect_count(n, [&](int mid) { return keys[mid] < key; });
            if (at < n && keys[at] == key) {
                const int2 sp = (new_tail ? a.hr_span : a.tr_span)[at];
                masked = sorted_contains((new_tail ? a.tails_hr : a.heads_tr) + sp.x, sp.y, c);
            }
        }
        a.pair[g] = (uint8_t)((new_tail ? 0 : 1) | (masked ? 2 : 0));
    }
}

}  // namespace
}  // namespace kge

using namespace kge;

extern "C" {

int kge_shared_negatives_draw(const int32_t *d_h, const int32_t *d_t, const int32_t *d_r, INT n_pos, INT first_position, INT P, INT N,
                              uint64_t seed, INT step, int32_t *d_cand, uint8_t *d_pair, void *stream) {
    return draw_call("kge_shared_negatives_draw", true, d_h, d_t, d_r, n_pos, first_position, P, N, seed, step, d_cand, d_pair, (hipStream_t)stream);
}

int kge_shared_negatives_draw_at(const int32_t *d_h, const int32_t *d_t, const int32_t *d_r, INT n_pos, INT first_position, INT P, INT N,
                                 uint64_t seed, INT step, int32_t *d_cand, uint8_t *d_pair, void *stream) {
    return draw_call("kge_shared_negatives_draw_at", false, d_h, d_t, d_r, n_pos, first_position, P, N, seed, step, d_cand, d_pair,
                     (hipStream_t)stream);
}

int kge_transe_emit_records_shared(const kge_model_desc *m, const float *d_ent, const float *d_rel, const int32_t *d_h, const int32_t *d_t,
                                   const int32_t *d_r, INT n_pos, INT stride, INT P, const int32_t *d_cand, INT N, const uint8_t *d_pair,
                                   INT denom, uint32_t *d_rec, int32_t *d_dst, float *d_loss, void *stream) {
    return emit_call("kge_transe_emit_records_shared", m, d_ent, d_rel, d_h, d_t, d_r, n_pos, stride, 0, P, nullptr, 0, d_cand, N, d_pair, denom, d_rec,
                     d_dst, d_loss, (hipStream_t)stream);
}

int kge_transe_emit_records_shared_at(const kge_model_desc *m, const float *d_ent, const float *d_rel, const int32_t *d_h, const int32_t *d_t,
                                      const int32_t *d_r, INT n_pos, INT stride, INT first_position, INT P, const int32_t *d_cand, INT N,
                                      const uint8_t *d_pair, INT denom, uint32_t *d_rec, int32_t *d_dst, float *d_loss, void *stream) {
    return emit_call("kge_transe_emit_records_shared_at", m, d_ent, d_rel, d_h, d_t, d_r, n_pos, stride, first_position, P, nullptr, 0, d_cand, N, d_pair,
                     denom, d_rec, d_dst, d_loss, (hipStream_t)stream);
}

INT kge_shared_chunk_cap(INT n_pos, INT P, INT rel_total) {
    if (n_pos < 0 || P < 1 || rel_total < 0) return fail(KGE_ERR_BAD_ARG, "kge_shared_chunk_cap: n_pos >= 0, P >= 1 and rel_total >= 0");
    return chunk_cap(n_pos, P, rel_total);
}

int kge_shared_order_by_relation(const int32_t *d_h, const int32_t *d_t, const int32_t *d_r, INT n_pos, INT P, int32_t *d_perm, int32_t *d_h2,
                                 int32_t *d_t2, int32_t *d_r2, int32_t *d_chunks, int32_t *d_n_chunks, void *stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (!device_ok()) return fail(KGE_ERR_NO_DEVICE, "kge_shared_order_by_relation: no usable HIP device");
    if (P < 1 || P > 127) return fail(KGE_ERR_BAD_ARG, "kge_shared_order_by_relation: the chunk must hold 1..127 positives (a candidate's count is within +-P, an int8)");
    if (n_pos < 0 || n_pos >= (INT(1) << 31) || !d_h || !d_t || !d_r || !d_perm || !d_h2 || !d_t2 || !d_r2 || !d_chunks || !d_n_chunks)
        return fail(KGE_ERR_BAD_ARG, "kge_shared_order_by_relation: bad arguments");
    Engine &e = engine();
    if (!e.index.loaded) return fail(KGE_ERR_NO_DATASET, "kge_shared_order_by_relation: no training set imported (rel_total is the imported set's)");
    int rc;
    if (n_pos == 0) return hip_check(hipMemsetAsync(d_n_chunks, 0, sizeof(int32_t), stream), "zero chunk count");
    const int rel_total = (int)e.index.rel_total;
    const long long cap = chunk_cap(n_pos, P, rel_total);
    if ((rc = g_ord.key.reserve(n_pos, "relation order keys")) || (rc = g_ord.key2.reserve(n_pos, "relation order keys")) ||
        (rc = g_ord.pos.reserve(n_pos, "relation order positions")) || (rc = g_ord.start.reserve(n_pos, "relation order run starts")) ||
        (rc = g_ord.idx.reserve(n_pos, "relation order chunk numbers")))
        return rc;
    unsigned bits = 1;
    while ((1ULL << bits) <= (unsigned long long)rel_total) bits++;
    const size_t n = (size_t)n_pos;
    size_t need_sort = 0, need_max = 0, need_sum = 0;
    if ((rc = hip_check(rocprim::radix_sort_pairs(nullptr, need_sort, g_ord.key.ptr(), g_ord.key2.ptr(), g_ord.pos.ptr(), d_perm, n, 0, bits, stream),
                        "relation order sort size")) ||
        (rc = hip_check(rocprim::inclusive_scan(nullptr, need_max, g_ord.start.ptr(), g_ord.start.ptr(), n, rocprim::maximum<int32_t>(), stream),
                        "relation order scan size")) ||
        (rc = hip_check(rocprim::inclusive_scan(nullptr, need_sum, g_ord.idx.ptr(), g_ord.idx.ptr(), n, rocprim::plus<int32_t>(), stream),
                        "relation order scan size")))
        return rc;
    const size_t need = std::max(need_sort, std::max(need_max, need_sum));
    if ((rc = g_ord.tmp.reserve((int64_t)std::max(need, (size_t)1), "relation order scratch"))) return rc;
    const dim3 grid((unsigned)((n_pos + 255) / 256)), block(256);
    hipLaunchKernelGGL(order_keys_kernel, grid, block, 0, stream, d_r, (long long)n_pos, rel_total, g_ord.key.ptr(), g_ord.pos.ptr());
    if ((rc = hip_check(rocprim::radix_sort_pairs(g_ord.tmp.ptr(), need_sort, g_ord.key.ptr(), g_ord.key2.ptr(), g_ord.pos.ptr(), d_perm, n, 0, bits, stream),
                        "relation order sort")))
        return rc;
    hipLaunchKernelGGL(order_gather_kernel, grid, block, 0, stream, d_h, d_t, d_r, (const uint32_t *)g_ord.key2.ptr(), (const int32_t *)d_perm,
                       (long long)n_pos, d_h2, d_t2, d_r2, g_ord.start.ptr());
    if ((rc = hip_check(rocprim::inclusive_scan(g_ord.tmp.ptr(), need_max, g_ord.start.ptr(), g_ord.start.ptr(), n, rocprim::maximum<int32_t>(), stream),
                        "relation order run scan")))
        return rc;
    hipLaunchKernelGGL(order_flags_kernel, grid, block, 0, stream, (const int32_t *)g_ord.start.ptr(), (long long)n_pos, (int)P, g_ord.idx.ptr());
    if ((rc = hip_check(rocprim::inclusive_scan(g_ord.tmp.ptr(), need_sum, g_ord.idx.ptr(), g_ord.idx.ptr(), n, rocprim::plus<int32_t>(), stream),
                        "relation order chunk scan")))
        return rc;
    const dim3 grid2((unsigned)((std::max((long long)n_pos, cap) + 255) / 256));
    hipLaunchKernelGGL(order_table_kernel, grid2, block, 0, stream, (const uint32_t *)g_ord.key2.ptr(), (const int32_t *)g_ord.start.ptr(),
                       (const int32_t *)g_ord.idx.ptr(), (long long)n_pos, cap, (int)P, reinterpret_cast<int2 *>(d_chunks), d_n_chunks);
    return hip_check(hipGetLastError(), "relation order launch");
}

int kge_shared_negatives_draw_grouped(const int32_t *d_h2, const int32_t *d_t2, const int32_t *d_r2, INT n_pos, const int32_t *d_chunks, INT cap,
                                      INT N, INT typed, uint64_t seed, INT step, int32_t *d_cand, uint8_t *d_pair, void *stream) {
    if (N < 1 || N > 63) return fail(KGE_ERR_BAD_ARG, "kge_shared_negatives_draw_grouped: 1..63 negatives per positive (a positive's count is within +-2N, an int8)");
    if (n_pos < 0 || cap < 0 || cap >= (INT(1) << 31) || step < 0 || !d_h2 || !d_t2 || !d_r2 || !d_chunks || !d_cand || !d_pair)
        return fail(KGE_ERR_BAD_ARG, "kge_shared_negatives_draw_grouped: bad arguments");
    int rc = ensure_device_index();
    if (rc) return rc;
    if ((rc = ensure_group_dir())) return rc;
    if (typed && (rc = ensure_typed_index(true))) return rc;
    if (n_pos == 0 && cap == 0) return KGE_OK;
    Engine &e = engine();
    GroupedDrawArgs a = {};
    a.h = d_h2; a.t = d_t2; a.r = d_r2; a.chunks = reinterpret_cast<const int2 *>(d_chunks);
    a.n_pos = n_pos; a.cap = cap; a.N = (int)N; a.typed = typed ? 1 : 0;
    a.S = mix64((unsigned long long)seed + ((unsigned long long)step + 1ULL) * kMixGamma);
    a.ent_total = (int)e.index.ent_total; a.rel_total = (int)e.index.rel_total; a.bern = e.bern ? 1 : 0;
    a.bern_prob = e.dev.bern_prob; a.tails_hr = e.dev.tails_hr; a.heads_tr = e.dev.heads_tr;
    a.type_bounds = e.dev.type_bounds; a.type_tails = e.dev.type_tails; a.type_heads = e.dev.type_heads;
    a.hr_key = g_dir.hr_key; a.tr_key = g_dir.tr_key; a.hr_span = g_dir.hr_span; a.tr_span = g_dir.tr_span;
    a.n_hr = g_dir.n_hr; a.n_tr = g_dir.n_tr;
    a.cand = d_cand; a.pair = d_pair;
    long long nb = ((n_pos + cap) * N + 255) / 256;
    if (nb > 65536) nb = 65536;
    hipLaunchKernelGGL(grouped_draw_kernel, dim3((unsigned)nb), dim3(256), 0, (hipStream_t)stream, a);
    return hip_check(hipGetLastError(), "grouped shared negatives draw launch");
}

int kge_shared_negatives_draw_grouped_mixed(const int32_t *d_h2, const int32_t *d_t2, const int32_t *d_r2, INT n_pos, const int32_t *d_chunks,
                                            INT cap, INT N, INT K, INT typed, uint64_t seed, INT step, int32_t *d_cand, uint8_t *d_pair,
                                            void *stream) {
    if (N < 1 || K < 0 || N + K > 63)
        return fail(KGE_ERR_BAD_ARG, "kge_shared_negatives_draw_grouped_mixed: 1 <= N, 0 <= K and N + K <= 63 candidates per positive (a positive's count is within +-2 (N + K), an int8)");
    if (n_pos < 0 || cap < 0 || cap >= (INT(1) << 31) || step < 0 || !d_h2 || !d_t2 || !d_r2 || !d_chunks || !d_cand || !d_pair)
        return fail(KGE_ERR_BAD_ARG, "kge_shared_negatives_draw_grouped_mixed: bad arguments");
    if (K == 0) return kge_shared_negatives_draw_grouped(d_h2, d_t2, d_r2, n_pos, d_chunks, cap, N, typed, seed, step, d_cand, d_pair, stream);
    int rc = ensure_device_index();
    if (rc) return rc;
    if ((rc = ensure_group_dir())) return rc;
    if (typed && (rc = ensure_typed_index(true))) return rc;
    if (n_pos == 0 && cap == 0) return KGE_OK;
    Engine &e = engine();
    MixedDrawArgs m = {};
    GroupedDrawArgs &a = m.g;
    m.K = (int)K;
    a.h = d_h2; a.t = d_t2; a.r = d_r2; a.chunks = reinterpret_cast<const int2 *>(d_chunks);
    a.n_pos = n_pos; a.cap = cap; a.N = (int)N; a.typed = typed ? 1 : 0;
    a.S = mix64((unsigned long long)seed + ((unsigned long long)step + 1ULL) * kMixGamma);
    a.ent_total = (int)e.index.ent_total; a.rel_total = (int)e.index.rel_total; a.bern = e.bern ? 1 : 0;
    a.bern_prob = e.dev.bern_prob; a.tails_hr = e.dev.tails_hr; a.heads_tr = e.dev.heads_tr;
    a.type_bounds = e.dev.type_bounds; a.type_tails = e.dev.type_tails; a.type_heads = e.dev.type_heads;
    a.hr_key = g_dir.hr_key; a.tr_key = g_dir.tr_key; a.hr_span = g_dir.hr_span; a.tr_span = g_dir.tr_span;
    a.n_hr = g_dir.n_hr; a.n_tr = g_dir.n_tr;
    a.cand = d_cand; a.pair = d_pair;
    long long nb = ((n_pos + cap) * (N + K) + 255) / 256;
    if (nb > 65536) nb = 65536;
    hipLaunchKernelGGL(grouped_draw_mixed_kernel, dim3((unsigned)nb), dim3(256), 0, (hipStream_t)stream, m);
    return hip_check(hipGetLastError(), "mixed shared negatives draw launch");
}

int kge_transe_emit_records_shared_chunks(const kge_model_desc *m, const float *d_ent, const float *d_rel, const int32_t *d_h2, const int32_t *d_t2,
                                          const int32_t *d_r2, INT n_pos, INT stride, const int32_t *d_chunks, INT cap, const int32_t *d_cand, INT N,
                                          const uint8_t *d_pair, INT denom, uint32_t *d_rec, int32_t *d_dst, float *d_loss, void *stream) {
    if (!d_chunks || cap < 0 || (cap < 1 && n_pos > 0)) return fail(KGE_ERR_BAD_ARG, "kge_transe_emit_records_shared_chunks: bad arguments (a chunk table of at least one slot)");
    return emit_call("kge_transe_emit_records_shared_chunks", m, d_ent, d_rel, d_h2, d_t2, d_r2, n_pos, stride, 0, 0,
                     reinterpret_cast<const int2 *>(d_chunks), cap, d_cand, N, d_pair, denom, d_rec, d_dst, d_loss, (hipStream_t)stream);
}

// ---- shared negatives on bf16 tables (include/kge_mi355.h, "Shared negatives on bf16 tables") ----
int kge_bf16_shared_supported(const kge_model_desc *m, INT N) { return bf16_shared_refusal(m, N) ? 0 : 1; }

int kge_transe_emit_records_shared_bf16(const kge_model_desc *m, const uint16_t *d_ent, const uint16_t *d_rel, const int32_t *d_h, const int32_t *d_t,
                                        const int32_t *d_r, INT n_pos, INT stride, INT P, const int32_t *d_cand, INT N, const uint8_t *d_pair,
                                        INT denom, uint32_t *d_rec, int32_t *d_dst, float *d_loss, void *stream) {
    return emit_call("kge_transe_emit_records_shared_bf16", m, d_ent, d_rel, d_h, d_t, d_r, n_pos, stride, 0, P, nullptr, 0, d_cand, N, d_pair, denom,
                     d_rec, d_dst, d_loss, (hipStream_t)stream, true);
}

int kge_transe_emit_records_shared_chunks_bf16(const kge_model_desc *m, const uint16_t *d_ent, const uint16_t *d_rel, const int32_t *d_h2,
                                               const int32_t *d_t2, const int32_t *d_r2, INT n_pos, INT stride, const int32_t *d_chunks, INT cap,
                                               const int32_t *d_cand, INT N, const uint8_t *d_pair, INT denom, uint32_t *d_rec, int32_t *d_dst,
                                               float *d_loss, void *stream) {
    if (!d_chunks || cap < 0 || (cap < 1 && n_pos > 0))
        return fail(KGE_ERR_BAD_ARG, "kge_transe_emit_records_shared_chunks_bf16: bad arguments (a chunk table of at least one slot)");
    return emit_call("kge_transe_emit_records_shared_chunks_bf16", m, d_ent, d_rel, d_h2, d_t2, d_r2, n_pos, stride, 0, 0,
                     reinterpret_cast<const int2 *>(d_chunks), cap, d_cand, N, d_pair, denom, d_rec, d_dst, d_loss, (hipStream_t)stream, true);
}

}  // extern "C"

