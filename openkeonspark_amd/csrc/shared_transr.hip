// TransR on negatives SHARED by relation-grouped chunks of positives (NON-PARITY, opt-in; the definition is in
// include/kge_mi355.h, "TransR on relation-grouped chunks").
//
// TransR's cost per scored row is a De x Dr matrix product, and a chunk of one relation has ONE matrix: its 2 len positive rows and
// its N candidates are projected once each, 2 P + N rows through the three row GEMMs where the unshared step puts P (2 + N).  The
// GEMMs are transr.hip's, unchanged, over a job list in the plain layout; this file adds what stands around them:
//   shared_transr_jobs_kernel   the job list from the chunk table, with no scan and no sort: the used slots come first, in position
//                        order, and cover the positions without a gap, so slot c begins at row 2 first_c + c N and holds its head
//                        rows, its tail rows and its N candidates; the slots are in relation order, so the rows are.  One wave per
//                        row finds the row's slot by bisection over that start and writes its key (the slot's relation; rel_total,
//                        the bucket the GEMMs skip, for a row no slot owns), its entity, and -- for a row no slot owns -- a zero GP
//                        row.  transr.hip's bounds_kernel turns the keys into bucket starts and the tile map.
//   shared_transr_walk_kernel   the pair walk of shared_proj_emit_kernel (shared_proj.hip) on PROJECTED rows: one workgroup of four
//                        waves per chunk slot, r^ normalised by every wave for itself, the tile's projected candidates normalised
//                        once into LDS with 1 / |.| and the clipped flag, a wave owning one positive at a time, normalising its two
//                        projected rows in registers and walking the candidates with packed sign arithmetic.  The epilogue is the
//                        normalise-backward alone: every row's count vector becomes its GP row (zeros for a zero count vector:
//                        dgrad and wgrad read every row of a bucket).  With more than one candidate tile a positive's two count
//                        vectors wait as int32 in its own GP rows until the last tile.
// The loss partials are summed per wave in candidate order, per chunk in wave order and over all cap slots in index order; the
// chunk's relation-row gradient is added to g_rel with fp32 atomics (several chunks share a relation), as dgrad and wgrad add theirs.
#include <algorithm>
#include <string>

#include "engine.hpp"
#include "team.hpp"
#include "team_shape.hpp"
#include "wave_row.hpp"

namespace kge {
namespace {

DevBuf<float> g_partials;

constexpr int kMaxChunk = 127;      // a candidate's byte fields hold sum (g + 1) <= 2 len

// What slot j of the chunk table owns: len == 0 = no row (an empty slot, a length above 127, one that points outside [0, n_pos),
// a relation outside the table).  row0 is monotone over a table whose used slots come first in position order.
struct Slot {
    long long b0, row0;
    int len, rho;
};
__device__ __forceinline__ Slot slot_of(const int2 *__restrict__ chunks, const int32_t *__restrict__ r, long long j, long long n_pos, int N,
                                        int rel_total) {
    const int2 ch = chunks[j];
    Slot s;
    s.b0 = n_pos; s.len = 0; s.rho = rel_total;
    if (ch.x >= 0 && ch.x < n_pos && ch.y > 0 && ch.y <= kMaxChunk) {
        const int rho = r[ch.x];
        if (rho >= 0 && rho < rel_total) { s.b0 = ch.x; s.len = (int)min((long long)ch.y, n_pos - ch.x); s.rho = rho; }
    }
    s.row0 = 2 * s.b0 + j * N;      // (+ 2 len + N <= 2 n_pos + cap N for every slot)
    return s;
}

struct JobArgs {
    const int2 *chunks;
    const int32_t *h, *t, *r, *cand;      // in sorted order
    long long n_pos, cap, J;
    int N, ent_total, rel_total, Dr;
    int32_t *keys, *slots, *job_ent, *rec_dst;
    float *GP;
};

__global__ __launch_bounds__(256) void shared_transr_jobs_kernel(JobArgs a) {
    const int lane = threadIdx.x & 63;
    for (long long p = (long long)blockIdx.x * 4 + (threadIdx.x >> 6); p < a.J; p += (long long)gridDim.x * 4) {
        long long lo = 0, hi = a.cap;      // the first slot that begins behind row p
        while (lo < hi) {
            const long long mid = (lo + hi) >> 1;
            if (slot_of(a.chunks, a.r, mid, a.n_pos, a.N, a.rel_total).row0 <= p) lo = mid + 1; else hi = mid;
        }
        int key = a.rel_total, ent = 0;
        if (lo > 0) {
            const Slot s = slot_of(a.chunks, a.r, lo - 1, a.n_pos, a.N, a.rel_total);
            const long long off = p - s.row0;
            if (s.len > 0 && off < 2 * s.len + a.N) {
                const int id = off < s.len ? a.h[s.b0 + off] : off < 2 * s.len ? a.t[s.b0 + off - s.len] : a.cand[(lo - 1) * a.N + (off - 2 * s.len)];
                key = s.rho;
                ent = id >= 0 && id < a.ent_total ? id : 0;      // (an id outside the table: row 0 is projected, the pair walk gives it no gradient)
            }
        }
        if (lane == 0) {
            a.keys[p] = key; a.slots[p] = (int32_t)p; a.job_ent[p] = ent;
            if (a.rec_dst) a.rec_dst[p] = -1;      // dgrad's record mode: a row no tile covers carries no record
        }
        if (key == a.rel_total)
            for (int i = lane; i < a.Dr; i += 64) a.GP[p * a.Dr + i] = 0.f;
    }
}

struct WalkArgs {
    const float *P, *rel;            // projected rows [J][D]; rel_embeddings
    float *GP, *g_rel;
    const int32_t *h, *t, *r;        // in sorted order
    const int32_t *cand;
    const uint8_t *pair;
    const int2 *chunks;              // [gridDim.x] (first sorted position, length)
    long long n_pos, cap;
    int N, T, n_tiles;               // candidates per positive, per tile; tiles
    int D, RS;                       // rel_dim; LDS row stride in floats (D rounded up to 4)
    int ent_total, rel_total;
    float margin, unit;              // unit = 1 / denom
    float *partials;
};

template <int Q, bool VEC>
__global__ __launch_bounds__(256) void shared_transr_walk_kernel(WalkArgs a) {
    constexpr int V = 4 * Q;
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
    const int T = a.T, RS = a.RS, D = a.D, N = a.N;
    float *wl = reinterpret_cast<float *>(lds);                                    // [4] wave losses
    unsigned char *body = lds + 16;
    float *crow = reinterpret_cast<float *>(body);                                 // [T][RS] normalised projected candidate rows
    uint32_t *ccnt = reinterpret_cast<uint32_t *>(body + (size_t)T * RS * 4);      // [T][RS / 4] byte fields sum (g + 1)
    int *nact = reinterpret_cast<int *>(body + (size_t)T * RS * 5);                // [T] active pairs
    int *cok = nact + T;                                                           // [T] 1 = the id lies inside the table
    float *cinv = reinterpret_cast<float *>(cok + T);                              // [T] 1 / |c . M|
    int *cuc = reinterpret_cast<int *>(cinv + T);                                  // [T] 0 = the norm was clipped
    int *fgr = reinterpret_cast<int *>(body);                                      // after the last tile, over the same bytes: [4][RS] r counts per wave
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long long j = blockIdx.x;
    const Slot s = slot_of(a.chunks, a.r, j, a.n_pos, N, a.rel_total);
    if (s.len == 0) {      // (its rows, if the table gives it any, have the key rel_total and the job list's zero GP rows)
        if (threadIdx.x == 0) a.partials[j] = 0.f;
        return;
    }
    const int Pc = s.len, rho = s.rho;
    const long long row_h = s.row0, row_t = s.row0 + Pc, row_c = s.row0 + 2 * Pc;
    WaveRow<Q, VEC> rw;
    rw.lane = lane; rw.D = D; rw.RS = RS;
    float RN[V];
    float inv_r;
    bool uc_r;
    {
        float x[V];
        rw.load(a.rel + (long long)rho * D, x);
        rw.normalize(x, RN, inv_r, uc_r);
    }
    int GR[V];
#pragma unroll
    for (int c = 0; c < V; c++) GR[c] = 0;
    float lsum = 0.f;
    for (int tile = 0; tile < a.n_tiles; tile++) {
        const int k0 = tile * T;
        const int Tc = min(T, N - k0);
        const bool last = tile == a.n_tiles - 1;
        // ---- the tile's candidates: normalised projected rows into LDS, counters cleared ----
        for (int i = threadIdx.x; i < T * (RS / 4); i += 256) ccnt[i] = 0;
        if ((int)threadIdx.x < T) nact[threadIdx.x] = 0;
        for (int kt = wave; kt < Tc; kt += 4) {
            const int id = a.cand[j * N + k0 + kt];
            const bool ok = id >= 0 && id < a.ent_total;
            float x[V], xn[V], inv;
            bool uc;
            rw.load(a.P + (row_c + k0 + kt) * D, x);
            rw.normalize(x, xn, inv, uc);
            if (!ok) {
#pragma unroll
                for (int c = 0; c < V; c++) xn[c] = 0.f;
            }
            rw.store_lds(crow + (size_t)kt * RS, xn);
            if (lane == 0) { cok[kt] = ok ? 1 : 0; cinv[kt] = inv; cuc[kt] = uc ? 1 : 0; }
        }
        __syncthreads();
        // ---- positives: one wave each ----
        for (int pp = wave; pp < Pc; pp += 4) {
            const long long b = s.b0 + pp;
            const int h = a.h[b], t = a.t[b];
            const bool ids_ok = h >= 0 && h < a.ent_total && t >= 0 && t < a.ent_total;
            int my_pb = 2;
            if (lane < Tc) my_pb = a.pair[b * N + k0 + lane];
            float Hn[V], Tn[V], inv_h, inv_t;
            bool uc_h, uc_t;
            {
                float x[V];
                rw.load(a.P + (row_h + pp) * D, x);
                rw.normalize(x, Hn, inv_h, uc_h);
                rw.load(a.P + (row_t + pp) * D, x);
                rw.normalize(x, Tn, inv_t, uc_t);
            }
            float B0[V], B1[V];       // new head: e = c^ + (r^ - t^);  new tail: e = (h^ + r^) - c^
            int sp[V], Ah[V], At[V];       // (the r count of a pair is -s as well: the positive's is Ah - At)
            float p_score;
            {
                float acc = 0.f;
#pragma unroll
                for (int c = 0; c < V; c++) {
                    B0[c] = RN[c] - Tn[c];
                    B1[c] = Hn[c] + RN[c];
                    const float e = Hn[c] + RN[c] - Tn[c];
                    acc += fabsf(e);
                    sp[c] = sgn_i(e);
                    Ah[c] = 0; At[c] = 0;
                }
                p_score = team_sum<64>(acc);
            }
            int cnt = 0;
            if (ids_ok) {
                for (int kt = 0; kt < Tc; kt++) {
                    const int pb = __builtin_amdgcn_readlane(my_pb, kt);
                    if ((pb & 2) || !cok[kt]) continue;
                    const bool new_head = pb & 1;
                    float e[V];
                    float acc = 0.f;
#pragma unroll
                    for (int q = 0; q < Q; q++) {
                        float4 c4 = make_float4(0.f, 0.f, 0.f, 0.f);
                        if (rw.has(q)) c4 = *reinterpret_cast<const float4 *>(crow + (size_t)kt * RS + 4 * (lane + 64 * q));
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
                            const int sg = sgn_i(e[c]);
                            // new head: the candidate takes -s, the kept t +s, r -s;  new tail: the candidate +s, the kept h -s, r -s
                            const int g = new_head ? -sg : sg;
                            if (new_head) At[c] += sg; else Ah[c] -= sg;
                            f |= (uint32_t)(g + 1) << (8 * i);
                        }
                        if (rw.has(q)) atomicAdd(ccnt + (size_t)kt * (RS / 4) + lane + 64 * q, f);
                    }
                    if (lane == 0) atomicAdd(nact + kt, 1);
                }
            }
            // ---- this tile's share of the positive's count vectors; the last tile turns the sums into GP rows ----
#pragma unroll
            for (int c = 0; c < V; c++) {
                const int v = cnt * sp[c];
                GR[c] += Ah[c] - At[c] + v;
                Ah[c] += v; At[c] -= v;
            }
            float *gp_h = a.GP + (row_h + pp) * D, *gp_t = a.GP + (row_t + pp) * D;
            if (a.n_tiles > 1) {      // (the lanes that stored a row's counts are the ones that reload them)
                if (tile > 0) {
                    int prev[V];
                    rw.load(reinterpret_cast<const int *>(gp_h), prev);
#pragma unroll
                    for (int c = 0; c < V; c++) Ah[c] += prev[c];
                    rw.load(reinterpret_cast<const int *>(gp_t), prev);
#pragma unroll
                    for (int c = 0; c < V; c++) At[c] += prev[c];
                }
                if (!last) {
                    rw.store(reinterpret_cast<int *>(gp_h), Ah);
                    rw.store(reinterpret_cast<int *>(gp_t), At);
                    continue;
                }
            }
            float g[V], gx[V];
            const bool nz_h = rw.any_nonzero(Ah), nz_t = rw.any_nonzero(At);
#pragma unroll
            for (int c = 0; c < V; c++) { g[c] = a.unit * (float)Ah[c]; gx[c] = 0.f; }
            if (nz_h) rw.normalize_bwd(Hn, g, inv_h, uc_h, gx);
            rw.store(gp_h, gx);
#pragma unroll
            for (int c = 0; c < V; c++) { g[c] = a.unit * (float)At[c]; gx[c] = 0.f; }
            if (nz_t) rw.normalize_bwd(Tn, g, inv_t, uc_t, gx);
            rw.store(gp_t, gx);
        }
        __syncthreads();
        // ---- the tile's candidate GP rows: one wave each ----
        for (int kt = wave; kt < Tc; kt += 4) {
            const int n = nact[kt];
            int G[V];
#pragma unroll
            for (int q = 0; q < Q; q++) {
                const uint32_t f = rw.has(q) ? ccnt[(size_t)kt * (RS / 4) + lane + 64 * q] : 0x01010101u * (uint32_t)n;
#pragma unroll
                for (int i = 0; i < 4; i++) G[4 * q + i] = (int)((f >> (8 * i)) & 0xFF) - n;
            }
            float g[V], gx[V];
#pragma unroll
            for (int c = 0; c < V; c++) { g[c] = a.unit * (float)G[c]; gx[c] = 0.f; }
            if (n > 0 && rw.any_nonzero(G)) {
                float xn[V];
                rw.load_lds(crow + (size_t)kt * RS, xn);
                rw.normalize_bwd(xn, g, cinv[kt], cuc[kt] != 0, gx);
            }
            rw.store(a.GP + (row_c + k0 + kt) * D, gx);
        }
        __syncthreads();
    }
    // ---- the chunk's relation-row gradient: the four waves' counts folded in LDS, one row of atomics ----
    rw.store_lds(fgr + (size_t)wave * RS, GR);
    if (lane == 0) wl[wave] = lsum;
    __syncthreads();
    if (wave != 0) return;
    int gsum[V];
#pragma unroll
    for (int c = 0; c < V; c++) gsum[c] = 0;
#pragma unroll
    for (int w = 0; w < 4; w++) {
        int g[V];
        rw.load_lds(fgr + (size_t)w * RS, g);
#pragma unroll
        for (int c = 0; c < V; c++) gsum[c] += g[c];
    }
    if (rw.any_nonzero(gsum)) {
        float g[V], out[V];
#pragma unroll
        for (int c = 0; c < V; c++) g[c] = a.unit * (float)gsum[c];
        rw.normalize_bwd(RN, g, inv_r, uc_r, out);
        float *pr = a.g_rel + (long long)rho * D;
#pragma unroll
        for (int c = 0; c < V; c++) {
            const int e = 4 * (lane + 64 * (c >> 2)) + (c & 3);
            if (e < D) atomicAdd(pr + e, out[c]);
        }
    }
    if (lane == 0) a.partials[j] = ((wl[0] + wl[1]) + wl[2]) + wl[3];
}

// fixed-order sum of the slots' partial hinge sums -> loss = sum / denom (shared_neg.hip's, for this file's partials)
__global__ __launch_bounds__(256) void shared_transr_loss_kernel(const float *__restrict__ partials, long long n, float unit, float *out) {
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

constexpr int kLdsBudget = 60 * 1024;   // per workgroup, as the TransH kernel's: two chunks per CU of 160 KB at the widest shapes

// null: the entry point takes the shape; otherwise the limit it breaks
const char *transr_shape_limit(const kge_model_desc &m, INT N) {
    if (m.model != KGE_TRANSR)
        return "shared negatives through dense gradient tables are built for TransR (TransE: kge_transe_emit_records_shared_chunks; TransH: "
               "kge_transh_emit_records_shared_chunks; TransD: kge_transd_emit_records_shared_chunks)";
    if (m.negative_rel != 0) return "shared negatives: relation negatives are not supported (negative_rel must be 0)";
    if (N < 1 || N > 63) return "shared negatives: 1..63 negatives per positive (a positive's count is within +-2N, an int8)";
    if (m.rel_dim < 1 || m.rel_dim > 512) return "shared negatives: the TransR pair walk holds a rel_dim up to 512";
    if (m.ent_dim < 1) return "shared negatives: TransR needs an ent_dim of at least 1";
    return nullptr;
}

}  // namespace
}  // namespace kge

using namespace kge;

extern "C" {

int kge_shared_transr_supported(const kge_model_desc *m, INT N) { return m && !transr_shape_limit(*m, N) ? 1 : 0; }

int kge_transr_forward_backward_shared_chunks(const kge_model_desc *m, const float *const tables[KGE_MAX_TABLES], const int32_t *d_h2,
                                              const int32_t *d_t2, const int32_t *d_r2, INT n_pos, INT stride, const int32_t *d_chunks, INT cap,
                                              const int32_t *d_cand, INT N, const uint8_t *d_pair, INT denom, float *const grads[KGE_MAX_TABLES],
                                              float *d_loss, void *stream_) {
    const std::string w = "kge_transr_forward_backward_shared_chunks";
    hipStream_t stream = (hipStream_t)stream_;
    if (!device_ok()) return fail(KGE_ERR_NO_DEVICE, w + ": no usable HIP device");
    if (!m) return fail(KGE_ERR_BAD_ARG, w + ": null argument");
    if (const char *limit = transr_shape_limit(*m, N)) return fail(KGE_ERR_UNSUPPORTED, limit);
    if (!tables || !tables[0] || !tables[1] || !tables[2])
        return fail(KGE_ERR_BAD_ARG, w + ": null table (ent_embeddings, rel_embeddings and transfer_matrix are needed)");
    if (!grads || !grads[0] || !grads[1] || !grads[2]) return fail(KGE_ERR_BAD_ARG, w + ": null gradient table (one per table is needed)");
    if (!d_chunks || cap < 0 || (cap < 1 && n_pos > 0)) return fail(KGE_ERR_BAD_ARG, w + ": bad arguments (a chunk table of at least one slot)");
    if (n_pos < 0 || stride < n_pos || denom <= 0 || !d_h2 || !d_t2 || !d_r2 || !d_cand || !d_pair || !d_loss) return fail(KGE_ERR_BAD_ARG, w + ": bad arguments");
    const long long J = 2 * n_pos + cap * N;
    if (n_pos >= (INT(1) << 30) || cap >= (INT(1) << 31) || J >= (INT(1) << 31)) return fail(KGE_ERR_UNSUPPORTED, "shared negatives: batch too large (2 n_pos + cap N rows must stay below 2^31)");
    if (n_pos == 0) return hip_check(hipMemsetAsync(d_loss, 0, sizeof(float), stream), "zero loss");
    int rc;
    if ((rc = g_partials.reserve(cap, "shared negatives loss partials"))) return rc;
    TransrSharedRows rows;
    if ((rc = transr_shared_workspace(*m, J, rows))) return rc;
    const int stages = engine().shared_transr_stages;      // (measurement hook: stop behind that many of the five stages)
    // 1. the job list
    JobArgs ja = {};
    ja.chunks = reinterpret_cast<const int2 *>(d_chunks); ja.h = d_h2; ja.t = d_t2; ja.r = d_r2; ja.cand = d_cand;
    ja.n_pos = n_pos; ja.cap = cap; ja.J = J; ja.N = (int)N; ja.ent_total = (int)m->ent_total; ja.rel_total = (int)m->rel_total; ja.Dr = m->rel_dim;
    ja.keys = rows.keys; ja.slots = rows.slots; ja.job_ent = rows.job_ent; ja.rec_dst = rows.rec_dst; ja.GP = rows.GP;
    hipLaunchKernelGGL(shared_transr_jobs_kernel, dim3((unsigned)std::min<long long>((J + 3) / 4, 1 << 16)), dim3(256), 0, stream, ja);
    if (stages == 1) return hip_check(hipGetLastError(), "shared transr job list launch");
    // 2. P = ent . M_rho over the job list
    if ((rc = launch_transr_shared_project(*m, tables, rows, J, stream))) return rc;
    if (stages == 2) return KGE_OK;
    // 3. the pair walk: P -> GP, g_rel, loss
    WalkArgs a = {};
    a.P = rows.P; a.rel = tables[1]; a.GP = rows.GP; a.g_rel = grads[1];
    a.h = d_h2; a.t = d_t2; a.r = d_r2; a.cand = d_cand; a.pair = d_pair; a.chunks = reinterpret_cast<const int2 *>(d_chunks);
    a.n_pos = n_pos; a.cap = cap; a.N = (int)N;
    a.D = m->rel_dim; a.RS = (a.D + 3) / 4 * 4;
    a.ent_total = (int)m->ent_total; a.rel_total = (int)m->rel_total; a.margin = m->margin; a.unit = 1.0f / (float)denom;
    a.partials = g_partials;
    // LDS: 16 bytes of wave losses, then per candidate its row, its byte fields and four words -- or, when that is less, the 16 RS
    // bytes the closing fold of the four waves lays over the same space
    const int per_cand = a.RS * 5 + 16;
    const int t_max = (kLdsBudget - 16) / per_cand;     // 23 at width 512, 60 at width 200
    a.n_tiles = ((int)N + t_max - 1) / t_max;
    a.T = ((int)N + a.n_tiles - 1) / a.n_tiles;
    const size_t lds_bytes = 16 + std::max((size_t)a.T * per_cand, (size_t)16 * a.RS);
    const dim3 grid((unsigned)cap), block(256);
    const bool vec = a.D % 4 == 0;
    // a wave owns a row at every width: the ladder's wave-wide rungs, four or eight elements per lane
    for_team_shape(std::max(a.D, 129), [&](auto ts) {
        constexpr int Q = decltype(ts)::C / 4;
        if constexpr (decltype(ts)::L == 64 && Q <= 2) {
            if (vec) hipLaunchKernelGGL((shared_transr_walk_kernel<Q, true>), grid, block, lds_bytes, stream, a);
            else hipLaunchKernelGGL((shared_transr_walk_kernel<Q, false>), grid, block, lds_bytes, stream, a);
        }
    });
    hipLaunchKernelGGL(shared_transr_loss_kernel, dim3(1), dim3(256), 0, stream, (const float *)g_partials.ptr(), (long long)cap, a.unit, d_loss);
    if ((rc = hip_check(hipGetLastError(), "shared transr pair walk launch")) || stages == 3) return rc;
    // 4. g_ent += GP . M_rho^T, 5. g_mat[rho] += X^T . GP
    if ((rc = launch_transr_shared_dgrad(*m, tables, grads, rows, J, stream)) || stages == 4) return rc;
    return launch_transr_shared_wgrad(*m, tables, grads, rows, J, stream);
}

}  // extern "C"
