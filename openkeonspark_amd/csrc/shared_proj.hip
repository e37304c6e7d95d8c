// TransH on negatives SHARED by relation-grouped chunks of positives (NON-PARITY, opt-in; the definition is in
// include/kge_mi355.h, "TransH on relation-grouped chunks").
//
// Every positive of a relation-grouped chunk has the chunk's relation rho, so the chunk has ONE normalised normal vector w^ and
// ONE r^, and a candidate's projection c - (c . w^) w^ and its normalisation depend on the candidate alone: they are formed N
// times per chunk where the unshared step forms them P N times.  The per-pair work is shared_emit_kernel's (shared_neg.hip), on
// projected vectors: the gradient with respect to a NORMALISED PROJECTED vector is an integer sign count.  What TransH adds is
//   a prologue   rows are projected and normalised (candidates once per tile into LDS, h and t in the owning wave's registers);
//   an epilogue  a row's count vector G becomes one float gradient record: normalise-backward, projection-backward, and the
//                row's share of the gradient of w^ into the wave's accumulator.
//   shared_proj_emit_kernel   one workgroup of four waves per chunk slot.  Lane l of a wave holds elements 4 (l + 64 q) .. + 3 of
//                        a row.  w^ and r^ are normalised by every wave for itself and stay in its registers for the whole chunk
//                        (8 VGPRs up to width 256, 16 up to 512: cheaper than an LDS read per use, and no barrier).  Per tile the
//                        candidates go into LDS projected and normalised, with a, 1 / |c_perp| and the clipped flag beside them; a
//                        wave then owns one positive at a time and walks the tile exactly as the TransE kernel does.  With more
//                        than one tile a positive's two count vectors wait as int32 in its own record slots -- the same lanes
//                        store and reload them -- until the last tile turns them into floats; a candidate's counts are complete
//                        when its tile ends.  The raw rows are gathered again for the epilogue (the d x term).
// Fixed orders everywhere, no global atomics: a wave adds its rows' shares of d/dw^ in the order it meets them, the four waves are
// folded in index order, the loss is summed per wave in candidate order, per chunk in wave order and over all cap slots in index
// order.  A step is reproducible bit for bit.
//
// TransD on the same chunks (include/kge_mi355.h, "TransD on relation-grouped chunks") is the same kernel under MODEL = KGE_TRANSD:
// the chunk's context vector is the RAW rel_transfer row r_p, an entity gathers its ent_transfer row x_p beside its row x,
// a = x . x_p and x^ = l2n(x + a r_p).  The pair walk does not change.  An entity writes TWO records (gxp + d x_p for its row,
// d x for its transfer row, d = gxp . r_p), a wave's accumulator takes a gxp, and the closing fold stores the sum as the
// rel_transfer record without a normalise-backward.  A positive's waiting count vectors sit in its two ent_embeddings slots.
#include <algorithm>
#include <string>

#include "engine.hpp"
#include "team.hpp"
#include "team_shape.hpp"
#include "wave_row.hpp"

namespace kge {
namespace {

DevBuf<float> g_partials;

struct ProjEmitArgs {
    const float *ent, *rel, *nrm;    // ent_embeddings, rel_embeddings, the context table (normal_vectors; TransD: rel_transfer)
    const int32_t *h, *t, *r;        // in sorted order
    const int32_t *cand;
    const uint8_t *pair;
    const int2 *chunks;              // [gridDim.x] (first sorted position, length)
    long long n_pos, cap;
    int N, T, n_tiles;               // candidates per positive, per tile; tiles
    int D, RS;                       // width; LDS row stride in floats (D rounded up to 4)
    int ent_total, rel_total;
    float margin, unit;              // unit = 1 / denom
    long long hub_base;              // virtual rows of the relation side: hub_base + (j % hub_k) 2 R + { rho | R + rho }
    int hub_k;
    float *rec;
    int32_t *dst;
    float *partials;
    const float *entp;               // TransD: ent_transfer
};

template <int MODEL, int Q, bool VEC>
__global__ __launch_bounds__(256) void shared_proj_emit_kernel(ProjEmitArgs a) {
    constexpr int V = 4 * Q;
    constexpr bool TD = MODEL == KGE_TRANSD;
    constexpr int EW = TD ? 2 : 1;       // records per entity: TransD's transfer row follows n_pos (a candidate's: cap N) later
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
    const int T = a.T, RS = a.RS, D = a.D, N = a.N;
    float *wl = reinterpret_cast<float *>(lds);                                    // [4] wave losses
    int *wany = reinterpret_cast<int *>(lds + 16);                                 // [4] did the wave write an entity record?
    unsigned char *body = lds + 32;
    float *crow = reinterpret_cast<float *>(body);                                 // [T][RS] projected, normalised candidate rows
    uint32_t *ccnt = reinterpret_cast<uint32_t *>(body + (size_t)T * RS * 4);      // [T][RS / 4] byte fields sum (g + 1)
    int *nact = reinterpret_cast<int *>(body + (size_t)T * RS * 5);                // [T] active pairs
    int *cid = nact + T;                                                           // [T] id, -1 = outside the table
    float *ca = reinterpret_cast<float *>(cid + T);                                // [T] c . w^
    float *cinv = ca + T;                                                          // [T] 1 / |c_perp|
    int *cuc = reinterpret_cast<int *>(cinv + T);                                  // [T] 0 = the norm was clipped
    float *facw = reinterpret_cast<float *>(body);                                 // after the last tile, over the same bytes:
    int *fgr = reinterpret_cast<int *>(body + (size_t)16 * RS);                    //   [4][RS] d/dw^ (d/dr_p) and [4][RS] r counts per wave
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long long j = blockIdx.x;
    const long long m_rel = 2 * EW * a.n_pos + j, m_nrm = m_rel + a.cap, m_c0 = 2 * EW * a.n_pos + 2 * a.cap + j * N;
    const long long ct_off = a.cap * N;       // TransD: a candidate's transfer record lies this far behind its row's
    const long long E = a.ent_total;          // TransD: key of a transfer row = E + id
    const int2 ch = a.chunks[j];
    const bool in = ch.x >= 0 && ch.x < a.n_pos && ch.y > 0;       // (a slot that points outside the call is an empty one)
    const long long b0 = in ? ch.x : 0;
    const int Pc = in ? (int)min((long long)ch.y, a.n_pos - b0) : 0;
    if (Pc == 0) {
        if ((int)threadIdx.x < N) {
            a.dst[m_c0 + threadIdx.x] = -1;
            if constexpr (TD) a.dst[m_c0 + ct_off + threadIdx.x] = -1;
        }
        if (threadIdx.x == 0) { a.dst[m_rel] = -1; a.dst[m_nrm] = -1; a.partials[j] = 0.f; }
        return;
    }
    const int rho = a.r[b0];
    const bool rho_ok = rho >= 0 && rho < a.rel_total;
    WaveRow<Q, VEC> rw;
    rw.lane = lane; rw.D = D; rw.RS = RS;
    float WN[V], RN[V];
    float inv_w, inv_r;
    bool uc_w, uc_r;
    {
        float x[V];
        if constexpr (TD) {      // r_p raw (ctx_forward<KGE_TRANSD>)
            rw.load(a.nrm + (long long)(rho_ok ? rho : 0) * D, WN);
            inv_w = 1.f; uc_w = true;
        } else {
            rw.load(a.nrm + (long long)(rho_ok ? rho : 0) * D, x);
            rw.normalize(x, WN, inv_w, uc_w);
        }
        rw.load(a.rel + (long long)(rho_ok ? rho : 0) * D, x);
        rw.normalize(x, RN, inv_r, uc_r);
    }
    float ACW[V];
    int GR[V];
#pragma unroll
    for (int c = 0; c < V; c++) { ACW[c] = 0.f; GR[c] = 0; }
    bool any_ent = false;
    float lsum = 0.f;
    for (int tile = 0; tile < a.n_tiles; tile++) {
        const int k0 = tile * T;
        const int Tc = min(T, N - k0);
        const bool last = tile == a.n_tiles - 1;
        // ---- the tile's candidates: projected, normalised rows into LDS, counters cleared ----
        for (int i = threadIdx.x; i < T * (RS / 4); i += 256) ccnt[i] = 0;
        if ((int)threadIdx.x < T) nact[threadIdx.x] = 0;
        for (int kt = wave; kt < Tc; kt += 4) {
            const int id = a.cand[j * N + k0 + kt];
            const bool ok = id >= 0 && id < a.ent_total;
            float x[V], xt[V], xn[V], ax, inv;
            bool uc;
            rw.template gather_project<MODEL>(a.ent, a.entp, ok ? id : 0, WN, x, xt, xn, ax, inv, uc);
            if (!ok) {
#pragma unroll
                for (int c = 0; c < V; c++) xn[c] = 0.f;
            }
            rw.store_lds(crow + (size_t)kt * RS, xn);
            if (lane == 0) { cid[kt] = ok ? id : -1; ca[kt] = ax; cinv[kt] = inv; cuc[kt] = uc ? 1 : 0; }
        }
        __syncthreads();
        // ---- positives: one wave each ----
        for (int pp = wave; pp < Pc; pp += 4) {
            const long long b = b0 + pp;
            const int h = a.h[b], t = a.t[b];
            const bool ids_ok = rho_ok && h >= 0 && h < a.ent_total && t >= 0 && t < a.ent_total;
            int my_pb = 2;
            if (lane < Tc) my_pb = a.pair[b * N + k0 + lane];
            float B0[V], B1[V];       // new head: e = c^ + (r^ - t^);  new tail: e = (h^ + r^) - c^
            int sp[V], Ah[V], At[V];       // (the r count of a pair is -s as well: the positive's is Ah - At)
            float p_score;
            {
                float x[V], xt[V], Hn[V], Tn[V], ax, inv;
                bool uc;
                rw.template gather_project<MODEL>(a.ent, a.entp, ids_ok ? h : 0, WN, x, xt, Hn, ax, inv, uc);
                rw.template gather_project<MODEL>(a.ent, a.entp, ids_ok ? t : 0, WN, x, xt, Tn, ax, inv, uc);
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
                    if ((pb & 2) || cid[kt] < 0) continue;
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
                            const int s = sgn_i(e[c]);
                            // new head: the candidate takes -s, the kept t +s, r -s;  new tail: the candidate +s, the kept h -s, r -s
                            const int g = new_head ? -s : s;
                            if (new_head) At[c] += s; else Ah[c] -= s;
                            f |= (uint32_t)(g + 1) << (8 * i);
                        }
                        if (rw.has(q)) atomicAdd(ccnt + (size_t)kt * (RS / 4) + lane + 64 * q, f);
                    }
                    if (lane == 0) atomicAdd(nact + kt, 1);
                }
            }
            // ---- this tile's share of the positive's count vectors; the last tile turns the sums into records ----
#pragma unroll
            for (int c = 0; c < V; c++) {
                const int v = cnt * sp[c];
                GR[c] += Ah[c] - At[c] + v;
                Ah[c] += v; At[c] -= v;
            }
            float *rec_h = a.rec + b * (long long)D, *rec_t = a.rec + (EW * a.n_pos + b) * (long long)D;
            float *rec_hp = rec_h + a.n_pos * (long long)D, *rec_tp = rec_t + a.n_pos * (long long)D;       // TransD only
            if (a.n_tiles > 1) {      // (the lanes that stored a slot's counts are the ones that reload them)
                if (tile > 0) {
                    int prev[V];
                    rw.load(reinterpret_cast<const int *>(rec_h), prev);
#pragma unroll
                    for (int c = 0; c < V; c++) Ah[c] += prev[c];
                    rw.load(reinterpret_cast<const int *>(rec_t), prev);
#pragma unroll
                    for (int c = 0; c < V; c++) At[c] += prev[c];
                }
                if (!last) {
                    rw.store(reinterpret_cast<int *>(rec_h), Ah);
                    rw.store(reinterpret_cast<int *>(rec_t), At);
                    continue;
                }
            }
            const bool nz_h = rw.any_nonzero(Ah), nz_t = rw.any_nonzero(At);
            if (nz_h) {
                float x[V], xt[V], xn[V], ax, inv;
                bool uc;
                rw.template gather_project<MODEL>(a.ent, a.entp, h, WN, x, xt, xn, ax, inv, uc);
                rw.template side_record<MODEL>(x, xt, xn, ax, inv, uc, Ah, a.unit, WN, ACW, rec_h, rec_hp);
            }
            if (nz_t) {
                float x[V], xt[V], xn[V], ax, inv;
                bool uc;
                rw.template gather_project<MODEL>(a.ent, a.entp, t, WN, x, xt, xn, ax, inv, uc);
                rw.template side_record<MODEL>(x, xt, xn, ax, inv, uc, At, a.unit, WN, ACW, rec_t, rec_tp);
            }
            any_ent = any_ent || nz_h || nz_t;
            if (lane == 0) {
                a.dst[b] = nz_h ? h : -1; a.dst[EW * a.n_pos + b] = nz_t ? t : -1;
                if constexpr (TD) { a.dst[a.n_pos + b] = nz_h ? (int32_t)(E + h) : -1; a.dst[3 * a.n_pos + b] = nz_t ? (int32_t)(E + t) : -1; }
            }
        }
        __syncthreads();
        // ---- the tile's candidate records: one wave each ----
        for (int kt = wave; kt < Tc; kt += 4) {
            const int n = nact[kt], id = cid[kt];
            const long long m = m_c0 + k0 + kt;
            int G[V];
#pragma unroll
            for (int q = 0; q < Q; q++) {
                const uint32_t f = rw.has(q) ? ccnt[(size_t)kt * (RS / 4) + lane + 64 * q] : 0x01010101u * (uint32_t)n;
#pragma unroll
                for (int i = 0; i < 4; i++) G[4 * q + i] = (int)((f >> (8 * i)) & 0xFF) - n;
            }
            const bool nz = n > 0 && rw.any_nonzero(G);
            if (nz) {
                float x[V], xt[V], xn[V];
                rw.load(a.ent + (long long)id * D, x);
                if constexpr (TD) rw.load(a.entp + (long long)id * D, xt);
                rw.load_lds(crow + (size_t)kt * RS, xn);
                rw.template side_record<MODEL>(x, xt, xn, ca[kt], cinv[kt], cuc[kt] != 0, G, a.unit, WN, ACW, a.rec + m * (long long)D,
                                               a.rec + (m + ct_off) * (long long)D);
                any_ent = true;
            }
            if (lane == 0) {
                a.dst[m] = nz ? id : -1;
                if constexpr (TD) a.dst[m + ct_off] = nz ? (int32_t)(E + id) : -1;
            }
        }
        __syncthreads();
    }
    // ---- the chunk's two relation-side records: the four waves folded in index order ----
    rw.store_lds(facw + (size_t)wave * RS, ACW);
    rw.store_lds(fgr + (size_t)wave * RS, GR);
    if (lane == 0) { wl[wave] = lsum; wany[wave] = any_ent ? 1 : 0; }
    __syncthreads();
    if (wave != 0) return;
    float f[4][V];
    int gsum[V];
#pragma unroll
    for (int c = 0; c < V; c++) gsum[c] = 0;
#pragma unroll
    for (int w = 0; w < 4; w++) {
        int g[V];
        rw.load_lds(facw + (size_t)w * RS, f[w]);
        rw.load_lds(fgr + (size_t)w * RS, g);
#pragma unroll
        for (int c = 0; c < V; c++) gsum[c] += g[c];
    }
    const bool nz_r = rw.any_nonzero(gsum);
    const bool any = (wany[0] | wany[1] | wany[2] | wany[3]) != 0;
    float g[V], out[V];
    if (nz_r) {
#pragma unroll
        for (int c = 0; c < V; c++) g[c] = a.unit * (float)gsum[c];
        rw.normalize_bwd(RN, g, inv_r, uc_r, out);
        rw.store(a.rec + m_rel * (long long)D, out);
    }
    if (any) {
#pragma unroll
        for (int c = 0; c < V; c++) g[c] = ((f[0][c] + f[1][c]) + f[2][c]) + f[3][c];
        if constexpr (TD) rw.store(a.rec + m_nrm * (long long)D, g);      // d/dr_p: r_p is used raw
        else {
            rw.normalize_bwd(WN, g, inv_w, uc_w, out);
            rw.store(a.rec + m_nrm * (long long)D, out);
        }
    }
    if (lane == 0) {
        const long long hub = a.hub_base + (j % a.hub_k) * 2LL * a.rel_total;
        a.dst[m_rel] = nz_r ? (int32_t)(hub + rho) : -1;
        a.dst[m_nrm] = any ? (int32_t)(hub + a.rel_total + rho) : -1;
        a.partials[j] = ((wl[0] + wl[1]) + wl[2]) + wl[3];
    }
}

// fixed-order sum of the slots' partial hinge sums -> loss = sum / denom (shared_neg.hip's, for this file's partials)
__global__ __launch_bounds__(256) void shared_proj_loss_kernel(const float *__restrict__ partials, long long n, float unit, float *out) {
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

constexpr int kLdsBudget = 60 * 1024;   // per workgroup, as the TransE kernel's: two chunks per CU at the widest shapes

// null: the shape is taken by the entry point built for `model` (KGE_TRANSH or KGE_TRANSD); otherwise the limit it breaks
const char *float_shape_limit(const kge_model_desc &m, INT N, int model) {
    if (model == KGE_TRANSD) {
        if (m.model != KGE_TRANSD) return "shared float records with transfer rows are built for TransD (TransH: kge_transh_emit_records_shared_chunks; "
                                          "TransE: kge_transe_emit_records_shared_chunks; TransR: kge_transr_forward_backward_shared_chunks)";
    } else {
        if (m.model == KGE_TRANSE) return "shared float records are built for TransH: TransE has its int8 records (kge_transe_emit_records_shared_chunks)";
        if (m.model == KGE_TRANSD) return "shared float records are built for TransH: TransD needs its transfer rows as well (kge_transd_emit_records_shared_chunks)";
        if (m.model != KGE_TRANSH) return "shared float records are built for TransH: TransR trains through dense gradient tables (kge_transr_forward_backward_shared_chunks)";
    }
    if (m.negative_rel != 0) return "shared negatives: relation negatives are not supported (negative_rel must be 0)";
    if (N < 1 || N > 63) return "shared negatives: 1..63 negatives per positive (a positive's count is within +-2N, an int8)";
    if (m.ent_dim != m.rel_dim) return model == KGE_TRANSD ? "shared negatives: TransD needs ent_dim == rel_dim" : "shared negatives: TransH needs ent_dim == rel_dim";
    if (m.ent_dim < 1 || m.ent_dim > 512) return "shared negatives: the shared emit kernel holds embedding widths up to 512";
    return nullptr;
}

// the body of both entry points; MODEL picks the instantiations and the record layout
template <int MODEL>
int emit_shared_chunks(const std::string &w, const kge_model_desc *m, const float *const tables[KGE_MAX_TABLES], const int32_t *d_h2, const int32_t *d_t2,
                       const int32_t *d_r2, INT n_pos, INT stride, const int32_t *d_chunks, INT cap, const int32_t *d_cand, INT N, const uint8_t *d_pair,
                       INT denom, INT n_pos_total, float *d_rec, int32_t *d_dst, float *d_loss, hipStream_t stream) {
    constexpr bool TD = MODEL == KGE_TRANSD;
    if (!device_ok()) return fail(KGE_ERR_NO_DEVICE, w + ": no usable HIP device");
    if (!m) return fail(KGE_ERR_BAD_ARG, w + ": null argument");
    if (const char *limit = float_shape_limit(*m, N, MODEL)) return fail(KGE_ERR_UNSUPPORTED, limit);
    if (!tables || !tables[0] || !tables[1] || !tables[2] || (TD && !tables[3]))
        return fail(KGE_ERR_BAD_ARG, w + (TD ? ": null table (ent_embeddings, rel_embeddings, rel_transfer and ent_transfer are needed)"
                                             : ": null table (ent_embeddings, rel_embeddings and normal_vectors are needed)"));
    if (!d_chunks || cap < 0 || (cap < 1 && n_pos > 0)) return fail(KGE_ERR_BAD_ARG, w + ": bad arguments (a chunk table of at least one slot)");
    if (n_pos < 0 || stride < n_pos || denom <= 0 || n_pos_total < n_pos || !d_h2 || !d_t2 || !d_r2 || !d_cand || !d_pair || !d_rec || !d_dst || !d_loss)
        return fail(KGE_ERR_BAD_ARG, w + ": bad arguments");
    const long long M = TD ? 4 * n_pos + cap * (2 * N + 2) : 2 * n_pos + cap * (N + 2);
    int64_t hub_base, hub_k, rows;
    float_record_hubs(*m, n_pos_total, N, hub_base, hub_k, rows);
    if (M >= (INT(1) << 31) || cap >= (INT(1) << 31) || rows >= (INT(1) << 31) - 1) return fail(KGE_ERR_UNSUPPORTED, "shared negatives: batch or row space too large");
    int rc;
    // (a position no slot covers, and every slot's records until its workgroup says otherwise: no record)
    if (M > 0 && (rc = hip_check(hipMemsetAsync(d_dst, 0xff, sizeof(int32_t) * (size_t)M, stream), "blank record keys"))) return rc;
    if (n_pos == 0) return hip_check(hipMemsetAsync(d_loss, 0, sizeof(float), stream), "zero loss");
    if ((rc = g_partials.reserve(cap, "shared negatives loss partials"))) return rc;
    ProjEmitArgs a = {};
    a.ent = tables[0]; a.rel = tables[1]; a.nrm = tables[2]; a.entp = TD ? tables[3] : nullptr;
    a.h = d_h2; a.t = d_t2; a.r = d_r2; a.cand = d_cand; a.pair = d_pair; a.chunks = reinterpret_cast<const int2 *>(d_chunks);
    a.n_pos = n_pos; a.cap = cap; a.N = (int)N;
    a.D = m->ent_dim; a.RS = (a.D + 3) / 4 * 4;
    a.ent_total = (int)m->ent_total; a.rel_total = (int)m->rel_total; a.margin = m->margin; a.unit = 1.0f / (float)denom;
    a.hub_base = hub_base; a.hub_k = (int)hub_k;
    a.rec = d_rec; a.dst = d_dst; a.partials = g_partials;
    // LDS: 32 bytes of wave slots, then per candidate its row, its byte fields and five words -- or, when that is less, the
    // 32 RS bytes the closing fold of the four waves lays over the same space (TransD keeps no more per candidate than TransH)
    const int per_cand = a.RS * 5 + 20;
    const int t_max = (kLdsBudget - 32) / per_cand;     // 23 at width 512 (the TransE kernel: 21)
    a.n_tiles = ((int)N + t_max - 1) / t_max;
    a.T = ((int)N + a.n_tiles - 1) / a.n_tiles;
    const size_t lds_bytes = 32 + std::max((size_t)a.T * per_cand, (size_t)32 * a.RS);
    const dim3 grid((unsigned)cap), block(256);
    const bool vec = a.D % 4 == 0;
    // a wave owns a row at every width: the ladder's wave-wide rungs, four or eight elements per lane
    for_team_shape(std::max(a.D, 129), [&](auto ts) {
        constexpr int Q = decltype(ts)::C / 4;
        if constexpr (decltype(ts)::L == 64 && Q <= 2) {
            if (vec) hipLaunchKernelGGL((shared_proj_emit_kernel<MODEL, Q, true>), grid, block, lds_bytes, stream, a);
            else hipLaunchKernelGGL((shared_proj_emit_kernel<MODEL, Q, false>), grid, block, lds_bytes, stream, a);
        }
    });
    hipLaunchKernelGGL(shared_proj_loss_kernel, dim3(1), dim3(256), 0, stream, (const float *)g_partials.ptr(), (long long)cap, a.unit, d_loss);
    return hip_check(hipGetLastError(), "shared projected emit launch");
}

}  // namespace
}  // namespace kge

using namespace kge;

extern "C" {

int kge_shared_float_supported(const kge_model_desc *m, INT N) { return m && !float_shape_limit(*m, N, KGE_TRANSH) ? 1 : 0; }
int kge_shared_transd_supported(const kge_model_desc *m, INT N) { return m && !float_shape_limit(*m, N, KGE_TRANSD) ? 1 : 0; }

int kge_transh_emit_records_shared_chunks(const kge_model_desc *m, const float *const tables[KGE_MAX_TABLES], const int32_t *d_h2, const int32_t *d_t2,
                                          const int32_t *d_r2, INT n_pos, INT stride, const int32_t *d_chunks, INT cap, const int32_t *d_cand, INT N,
                                          const uint8_t *d_pair, INT denom, INT n_pos_total, float *d_rec, int32_t *d_dst, float *d_loss, void *stream) {
    return emit_shared_chunks<KGE_TRANSH>("kge_transh_emit_records_shared_chunks", m, tables, d_h2, d_t2, d_r2, n_pos, stride, d_chunks, cap, d_cand, N,
                                          d_pair, denom, n_pos_total, d_rec, d_dst, d_loss, (hipStream_t)stream);
}

int kge_transd_emit_records_shared_chunks(const kge_model_desc *m, const float *const tables[KGE_MAX_TABLES], const int32_t *d_h2, const int32_t *d_t2,
                                          const int32_t *d_r2, INT n_pos, INT stride, const int32_t *d_chunks, INT cap, const int32_t *d_cand, INT N,
                                          const uint8_t *d_pair, INT denom, INT n_pos_total, float *d_rec, int32_t *d_dst, float *d_loss, void *stream) {
    return emit_shared_chunks<KGE_TRANSD>("kge_transd_emit_records_shared_chunks", m, tables, d_h2, d_t2, d_r2, n_pos, stride, d_chunks, cap, d_cand, N,
                                          d_pair, denom, n_pos_total, d_rec, d_dst, d_loss, (hipStream_t)stream);
}

}  // extern "C"
