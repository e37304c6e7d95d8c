// bf16 TABLE STORAGE for TransE on the one-rank int8-record touched-rows step (NON-PARITY, opt-in; the definition is in
// include/kge_mi355.h, "bf16 table storage").  The tables THEMSELVES are bf16 -- this is not a shadow copy beside fp32 tables.
// Three kernels of their own, no existing kernel is touched:
//   transe_emit_bf16_kernel   gather / score / hinge on rows of eight bf16 per 16-byte load, records in kge_transe_emit_records'
//                             format (natural element order), so kge_transe_reduce_records serves unchanged;
//   apply_rows_bf16_kernel    the row-list SGD / row-wise Adagrad rule from the int32 counts on the widened row, stored by
//                             stochastic rounding (bf16_dev.hpp);
//   round_bf16_kernel         the rounding rule alone, for the tests.
#include "bf16_dev.hpp"
#include "models_dev.hpp"
#include "optim_dev.hpp"
#include "team_shape.hpp"

namespace kge {

// models.hip: the deferral list of the emit kernels (kge_transe_deferred_groups reads its counter), restarted on `stream`
int transe_defer_buffers(int64_t n_pos, hipStream_t stream, int32_t *&list, int32_t *&count);

namespace {

// The int8 record of a positive's row holds sums of up to 2 * (active negatives) signs: beyond 63 active negatives a byte could
// wrap, so such a group is deferred like one that is not sampler-shaped (keys -1, listed, counted) instead of written wrong.
constexpr int kMaxActive = 63;

// ---- the emit kernel ---------------------------------------------------------------------------------------------------------
// A TEAM of L lanes owns one group; lane l holds the 16-byte chunks w = l + L q (q < Q) of a row: elements 8w .. 8w + 7, widened
// with a shift (even elements) and a mask (odd elements).  K negatives side by side -- 4 where the wave is the team, 2 for the
// narrower teams -- so a wave keeps 4 (L = 64, 32) or 8 (L = 16) row gathers in flight.  Per negative the work is transe_emit_vec_body's without the inverse-norm
// table: the norm from the gathered row, e = fma(f, x, B) against the group constants, sign(e) from the bit pattern, packed int16
// sign sums.  Record dwords 2w and 2w + 1 (elements 8w .. 8w + 7, one byte each) leave as one 8-byte store.
template <int L, int Q>
__global__ __launch_bounds__(256, Q == 1 ? 3 : 2) void transe_emit_bf16_kernel(FbArgs a, const uint16_t *__restrict__ ent, const uint16_t *__restrict__ rel,
                                                               int rec_dw) {
    constexpr int TEAMS = 256 / L;
    constexpr int K = L == 64 ? 4 : 2;      // negatives side by side per team: at least four rows in flight per wave
    constexpr int N = 8 * Q;      // elements per lane
    constexpr int P = 4 * Q;      // packed sign pairs per lane
    __shared__ float red[TEAMS];
    const int lane = threadIdx.x % L;
    const int team_in_block = threadIdx.x / L;
    const int D = a.D;
    bool valid[Q];
#pragma unroll
    for (int q = 0; q < Q; q++) valid[q] = 8 * (lane + L * q) < D;
    auto load8 = [&](const uint16_t *__restrict__ tab, long long row, uint4 (&x)[Q]) {
        const uint16_t *p = tab + row * D;
#pragma unroll
        for (int q = 0; q < Q; q++)
            x[q] = valid[q] ? *reinterpret_cast<const uint4 *>(p + 8 * (lane + L * q)) : make_uint4(0u, 0u, 0u, 0u);
    };
    auto widen = [&](const uint4 (&x)[Q], float (&f)[N]) {
#pragma unroll
        for (int q = 0; q < Q; q++) {
            f[8 * q] = bf16_widen_lo(x[q].x); f[8 * q + 1] = bf16_widen_hi(x[q].x);
            f[8 * q + 2] = bf16_widen_lo(x[q].y); f[8 * q + 3] = bf16_widen_hi(x[q].y);
            f[8 * q + 4] = bf16_widen_lo(x[q].z); f[8 * q + 5] = bf16_widen_hi(x[q].z);
            f[8 * q + 6] = bf16_widen_lo(x[q].w); f[8 * q + 7] = bf16_widen_hi(x[q].w);
        }
    };
    auto ssq = [&](const float (&f)[N]) {
        float s = 0.f;
#pragma unroll
        for (int i = 0; i < N; i++) s += f[i] * f[i];
        return s;
    };
    auto inv_of = [](float ss) { return 1.0f / sqrtf(ss >= 1e-12f ? ss : 1e-12f); };      // eps inside the max
    auto store_rec = [&](long long m, const uint32_t (&w)[2 * Q]) {
        uint32_t *p = a.rec + m * (long long)rec_dw;
#pragma unroll
        for (int q = 0; q < Q; q++)
            if (valid[q]) *reinterpret_cast<uint2 *>(p + 2 * (lane + L * q)) = make_uint2(w[2 * q], w[2 * q + 1]);
    };
    float lsum = 0.f;
    for (long long b = (long long)blockIdx.x * TEAMS + team_in_block; b < a.n_pos; b += (long long)gridDim.x * TEAMS) {
        const int h = a.bh[b], t = a.bt[b], r = a.br[b];
        const int rel_row0 = a.ent_total;
        // ---- negatives' ids: one per lane (first round), classified once ----
        int my_code = 0, my_row = 0;
        float bad = 0.f;
        for (int k = lane; k < (int)a.n_neg; k += L) {
            const long long j = b + (long long)(k + 1) * a.stride;
            const int nh = a.bh[j], nt = a.bt[j], nr = a.br[j];
            const NegClass nc = classify_negative<KGE_TRANSE>(h, t, r, nh, nt, nr, a.negative_rel);
            if (!nc.fast) bad = 1.f;
            if (k < L) {
                my_code = !nc.same_h ? 0 : (!nc.same_t ? 1 : 2);
                my_row = !nc.same_h ? nh : (!nc.same_t ? nt : nr);
            }
        }
        bool defer = team_sum<L>(bad) != 0.f;      // not sampler-shaped: no record, the group is listed
        float B0[N], B1[N], B2[N];
        float p = 0.f;
        s16x2 sp[P];
        s16x2 Ah[P], At[P], Ar[P];
        int cnt = 0;
        float gsum = 0.f;
        if (!defer) {
            // ---- the positive: B0 = r^-t^, B1 = h^+r^, B2 = h^-t^ (free of negative zeros, see transe_emit_vec_body) ----
            {
                uint4 hr[Q], tr[Q], rr[Q];
                load8(ent, h, hr); load8(ent, t, tr); load8(rel, r, rr);
                float hf[N], tf[N], rf[N];
                widen(hr, hf); widen(tr, tf); widen(rr, rf);
                const float ih = inv_of(team_sum<L>(ssq(hf))), it = inv_of(team_sum<L>(ssq(tf))), ir = inv_of(team_sum<L>(ssq(rf)));
                float acc = 0.f;
#pragma unroll
                for (int i = 0; i < N; i += 2) {
                    const float H0 = hf[i] * ih, T0 = tf[i] * it, R0 = rf[i] * ir;
                    const float H1 = hf[i + 1] * ih, T1 = tf[i + 1] * it, R1 = rf[i + 1] * ir;
                    B0[i] = R0 - T0 + 0.0f; B0[i + 1] = R1 - T1 + 0.0f;
                    B1[i] = H0 + R0 + 0.0f; B1[i + 1] = H1 + R1 + 0.0f;
                    B2[i] = H0 - T0 + 0.0f; B2[i + 1] = H1 - T1 + 0.0f;
                    const float e0 = H0 + R0 - T0 + 0.0f, e1 = H1 + R1 - T1 + 0.0f;
                    acc += fabsf(e0) + fabsf(e1);
                    sp[i / 2] = pack16(sign_of_bits(e0), sign_of_bits(e1));
                }
                p = team_sum<L>(acc);
            }
#pragma unroll
            for (int i = 0; i < P; i++) { Ah[i] = 0; At[i] = 0; Ar[i] = 0; }
            for (int k0 = 0; k0 < (int)a.n_neg; k0 += L) {
                if (k0 > 0) {   // later rounds (n_neg > L): fetch and classify this round's ids
                    const int my_k = k0 + lane;
                    my_code = 0; my_row = 0;
                    if (my_k < (int)a.n_neg) {
                        const long long j = b + (long long)(my_k + 1) * a.stride;
                        const int nh = a.bh[j], nt = a.bt[j], nr = a.br[j];
                        const NegClass nc = classify_negative<KGE_TRANSE>(h, t, r, nh, nt, nr, a.negative_rel);
                        my_code = !nc.same_h ? 0 : (!nc.same_t ? 1 : 2);
                        my_row = !nc.same_h ? nh : (!nc.same_t ? nt : nr);
                    }
                }
                const int in_round = min(L, (int)a.n_neg - k0);
                int my_dst = -1;
                for (int kk = 0; kk < in_round; kk += K) {
                    int code[K], row[K];
                    uint4 x[K][Q];
#pragma unroll
                    for (int u = 0; u < K; u++) {
                        const int src = min(kk + u, in_round - 1);
                        code[u] = team_bcast<L>(my_code, src);
                        row[u] = team_bcast<L>(my_row, src);
                    }
#pragma unroll
                    for (int u = 0; u < K; u++) load8(code[u] == 2 ? rel : ent, row[u], x[u]);      // K gathers in flight (a padded slot re-reads a valid row)
                    float f[K];
#pragma unroll
                    for (int u = 0; u < K; u++) {
                        float xf[N];
                        widen(x[u], xf);
                        f[u] = ssq(xf);
                    }
#pragma unroll
                    for (int u = 0; u < K; u++) {
                        const float iv = inv_of(team_sum<L>(f[u]));
                        f[u] = code[u] == 1 ? -iv : iv;
                    }
                    float sc[K];
                    s16x2 sg[K][P];
#pragma unroll
                    for (int u = 0; u < K; u++) {
                        float xf[N];
                        widen(x[u], xf);
                        float acc = 0.f;
                        auto apply = [&](const float (&Bs)[N]) {
#pragma unroll
                            for (int i = 0; i < N; i += 2) {
                                const float e0 = fmaf(f[u], xf[i], Bs[i]), e1 = fmaf(f[u], xf[i + 1], Bs[i + 1]);
                                acc += fabsf(e0) + fabsf(e1);
                                sg[u][i / 2] = pack16(sign_of_bits(e0), sign_of_bits(e1));
                            }
                        };
                        if (code[u] == 0) apply(B0); else if (code[u] == 1) apply(B1); else apply(B2);
                        sc[u] = acc;
                    }
#pragma unroll
                    for (int u = 0; u < K; u++) sc[u] = team_sum<L>(sc[u]);
#pragma unroll
                    for (int u = 0; u < K; u++) {
                        if (kk + u >= in_round) continue;
                        const float v = p - sc[u] + a.margin;
                        if (v >= 0.f) {      // a hinge tie is active
                            cnt++; gsum += v;
                            const long long m = (long long)(3 + k0 + kk + u) * a.n_pos + b;
                            // new head (0): -s, kept t gets +s, r gets -s;  new tail (1): +s, kept h gets -s, r gets -s;
                            // new relation vector (2): -s, h gets -s, t gets +s -- as small multipliers, branch-free
                            const int c = code[u];
                            const s16x2 kh = pack16(c == 0 ? 0 : -1, c == 0 ? 0 : -1), kt = pack16(c == 1 ? 0 : 1, c == 1 ? 0 : 1);
                            const s16x2 kr = pack16(c == 2 ? 0 : -1, c == 2 ? 0 : -1), kx = pack16(c == 1 ? 1 : -1, c == 1 ? 1 : -1);
                            uint32_t rec[2 * Q];
#pragma unroll
                            for (int i = 0; i < P; i += 2) {
                                rec[i / 2] = bytes_of(sg[u][i] * kx, sg[u][i + 1] * kx);
                                Ah[i] += sg[u][i] * kh; Ah[i + 1] += sg[u][i + 1] * kh;
                                At[i] += sg[u][i] * kt; At[i + 1] += sg[u][i + 1] * kt;
                                Ar[i] += sg[u][i] * kr; Ar[i + 1] += sg[u][i + 1] * kr;
                            }
                            store_rec(m, rec);
                            if (lane == kk + u) my_dst = c == 2 ? rel_row0 + row[u] : row[u];
                        }
                    }
                }
                // destinations of this round's negatives: one store instruction for the whole round
                if (k0 + lane < (int)a.n_neg) a.dst[(long long)(3 + k0 + lane) * a.n_pos + b] = my_dst;
            }
            defer = cnt > kMaxActive;
        }
        if (defer) {
            for (long long sl = lane; sl < 3 + a.n_neg; sl += L) a.dst[sl * a.n_pos + b] = -1;
            if (lane == 0 && a.group_list) a.group_list[atomicAdd(a.group_count, 1)] = (int32_t)b;
            continue;
        }
        lsum += gsum;
        if (cnt > 0) {
            uint32_t rh[2 * Q], rt[2 * Q], rr[2 * Q];
            const s16x2 c2 = pack16(cnt, cnt);
#pragma unroll
            for (int i = 0; i < P; i += 2) {
                const s16x2 v0 = sp[i] * c2, v1 = sp[i + 1] * c2;
                rh[i / 2] = bytes_of(Ah[i] + v0, Ah[i + 1] + v1);
                rt[i / 2] = bytes_of(At[i] - v0, At[i + 1] - v1);
                rr[i / 2] = bytes_of(Ar[i] + v0, Ar[i + 1] + v1);
            }
            store_rec(b, rh);
            store_rec(a.n_pos + b, rt);
            store_rec(2 * a.n_pos + b, rr);
        }
        if (lane == 0) {
            a.dst[b] = cnt > 0 ? (int32_t)h : -1;
            a.dst[a.n_pos + b] = cnt > 0 ? (int32_t)t : -1;
            a.dst[2 * a.n_pos + b] = cnt > 0 ? (int32_t)(rel_row0 + r) : -1;
        }
    }
    finish_loss<TEAMS>(a, red, lsum, lane, team_in_block);
}

// the emit kernel's own ladder: 16-byte chunks per row = D / 8 -> (lanes per team, chunks per lane)
template <class F>
inline bool for_bf16_emit_shape(int D, F &&f) {
    if (D <= 128) f(TeamShape<16, 1>{});
    else if (D <= 256) f(TeamShape<32, 1>{});
    else if (D <= 512) f(TeamShape<64, 1>{});
    else if (D <= 1024) f(TeamShape<64, 2>{});
    else return false;
    return true;
}

// ---- the apply kernel --------------------------------------------------------------------------------------------------------
struct Bf16ApplyArgs {
    uint16_t *ent, *rel;
    float *acc_ent, *acc_rel;     // row-wise Adagrad: one float per row; null for SGD
    const int32_t *row_list, *S, *n_rows;
    long long E;
    int D;
    float unit, lr;
    unsigned long long k;         // bf16_step_key(seed, step)
};

// One team per listed row, on the team shape of apply_rows_rowadagrad_kernel (lane l: elements l, l + L, ...), so that the
// gradient g has that kernel's bits on the widened row: counts through the normalisation's backward (count_grad's operations,
// each rounded on its own).  Then SGD or the row-wise Adagrad rule, and every element of the row is stored through
// bf16_round_stochastic -- an element that did not move is a bf16 value and keeps its bits whatever its random bits are.  A
// listed row whose counts are all zero is skipped, accumulator included.
template <int L, int C, bool ROWADAGRAD>
__global__ __launch_bounds__(256) void apply_rows_bf16_kernel(Bf16ApplyArgs a) {
#pragma clang fp contract(off)
    constexpr int TEAMS = 256 / L;
    Team<L, C> tm;
    tm.lane = threadIdx.x % L;
    tm.D = a.D;
    const long long n_rows = (long long)a.n_rows[0];
    const unsigned long long quarter = (unsigned long long)(a.D / 4);
    for (long long i = (long long)blockIdx.x * TEAMS + threadIdx.x / L; i < n_rows; i += (long long)gridDim.x * TEAMS) {
        const long long key = (long long)a.row_list[i];
        long long row = key;
        uint16_t *table = a.ent;
        float *at = a.acc_ent;
        if (row >= a.E) { row -= a.E; table = a.rel; at = a.acc_rel; }
        const int32_t *Sp = a.S + i * a.D;
        float s[C];
        float touched = 0.f;
#pragma unroll
        for (int c = 0; c < C; c++) {
            const int e = tm.lane + L * c;
            s[c] = (float)(e < a.D ? Sp[e] : 0);
            touched += s[c] != 0.f ? 1.f : 0.f;
        }
        touched = team_sum<L>(touched);
        if (touched == 0.f) continue;           // (the same for every lane of the team)
        uint16_t *pp = table + row * a.D;
        float x[C], xn[C], g[C], inv;
        bool uc;
#pragma unroll
        for (int c = 0; c < C; c++) { const int e = tm.lane + L * c; x[c] = e < a.D ? bf16_widen(pp[e]) : 0.f; }
        tm.normalize(x, xn, inv, uc);
        float d = tm.dot(xn, s);
        if (!uc) d = 0.f;
        float q = 0.f;
#pragma unroll
        for (int c = 0; c < C; c++) {           // lanes past the row's end: s = xn = 0, so g = 0
            g[c] = add_rn(mul_rn(mul_rn(a.unit, inv), sub_rn(s[c], mul_rn(d, xn[c]))), 0.f);      // count_grad (transe_counts.hip)
            if constexpr (ROWADAGRAD) q = rowadagrad_sq(q, g[c]);
        }
        float root = 1.f;
        if constexpr (ROWADAGRAD) {
            float acc = at[row];                // read by every lane before lane 0 writes it below
            q = team_sum<L>(q);
            const float a_old = acc;
            root = rowadagrad_root(acc, q, a.D);
            if (tm.lane == 0 && __builtin_bit_cast(unsigned, acc) != __builtin_bit_cast(unsigned, a_old)) at[row] = acc;
        }
#pragma unroll
        for (int c = 0; c < C; c++) {
            const int e = tm.lane + L * c;
            if (e >= a.D || g[c] == 0.f) continue;      // zero gradient: the stored bits stay
            const float y = ROWADAGRAD ? rowadagrad_one(x[c], g[c], a.lr, root) : sub_rn(x[c], mul_rn(a.lr, g[c]));
            pp[e] = bf16_round_stochastic(y, bf16_round_bits(a.k, (unsigned long long)key, quarter, (unsigned)e));
        }
    }
}

__global__ __launch_bounds__(256) void round_bf16_kernel(const float *__restrict__ y, long long rows, int D, unsigned long long first_key,
                                                         unsigned long long k, uint16_t *__restrict__ out) {
    const unsigned long long quarter = (unsigned long long)(D / 4);
    const long long n = rows * D;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
        const long long row = i / D;
        const unsigned j = (unsigned)(i - row * D);
        out[i] = bf16_round_stochastic(y[i], bf16_round_bits(k, first_key + (unsigned long long)row, quarter, j));
    }
}

const char *bf16_refusal(const kge_model_desc *m, INT n_neg) {
    if (!m) return "no model descriptor";
    if (m->model != KGE_TRANSE) return "bf16 table storage is built for TransE only";
    if (m->ent_dim != m->rel_dim) return "bf16 table storage: entity and relation widths differ";
    if (m->ent_dim % 8 != 0 || m->ent_dim < 8) return "bf16 table storage needs a width that is a multiple of 8 (rows of 16-byte chunks)";
    if (m->ent_dim > 1024) return "bf16 table storage: widths up to 1024";
    if (n_neg < 1 || n_neg > 127) return "bf16 table storage: 1 to 127 negatives per positive";
    if (m->ent_total + m->rel_total >= (int64_t(1) << 30)) return "bf16 table storage: fewer than 2^30 rows";
    return nullptr;
}

int apply_rows_bf16(const char *who, bool rowadagrad, const kge_model_desc *m, uint16_t *d_ent, uint16_t *d_rel, float *d_acc_ent,
                    float *d_acc_rel, const int32_t *d_rows, const int32_t *d_row_counts, const int32_t *d_n_rows, INT max_rows, INT denom,
                    float lr, uint64_t seed, uint64_t step, hipStream_t stream) {
    if (!device_ok()) return fail(KGE_ERR_NO_DEVICE, std::string(who) + ": no usable HIP device");
    if (!m || !d_ent || !d_rel || !d_rows || !d_row_counts || !d_n_rows || denom <= 0 || (rowadagrad && (!d_acc_ent || !d_acc_rel)))
        return fail(KGE_ERR_BAD_ARG, std::string(who) + ": bad arguments");
    if (const char *why = bf16_refusal(m, 1)) return fail(KGE_ERR_UNSUPPORTED, std::string(who) + ": " + why);
    if (max_rows <= 0) return KGE_OK;
    Bf16ApplyArgs a = {};
    a.ent = d_ent; a.rel = d_rel; a.acc_ent = d_acc_ent; a.acc_rel = d_acc_rel;
    a.row_list = d_rows; a.S = d_row_counts; a.n_rows = d_n_rows;
    a.E = m->ent_total; a.D = m->ent_dim; a.unit = 1.0f / (float)denom; a.lr = lr; a.k = bf16_step_key(seed, step);
    for_transe_team_shape(a.D, [&](auto t) {
        constexpr int L = decltype(t)::L, C = decltype(t)::C;
        long long nb = (max_rows + (256 / L) - 1) / (256 / L);
        if (nb > 8192) nb = 8192;
        if (rowadagrad) hipLaunchKernelGGL((apply_rows_bf16_kernel<L, C, true>), dim3((unsigned)nb), dim3(256), 0, stream, a);
        else hipLaunchKernelGGL((apply_rows_bf16_kernel<L, C, false>), dim3((unsigned)nb), dim3(256), 0, stream, a);
    });
    return hip_check(hipGetLastError(), "bf16 apply rows launch");
}

}  // namespace
}  // namespace kge

using namespace kge;

extern "C" {

int kge_bf16_tables_supported(const kge_model_desc *m, INT n_neg) { return bf16_refusal(m, n_neg) ? 0 : 1; }

int kge_transe_emit_records_bf16(const kge_model_desc *m, const uint16_t *d_ent, const uint16_t *d_rel, const int32_t *d_h, const int32_t *d_t,
                                 const int32_t *d_r, INT n_pos, INT n_neg, INT stride, INT denom, uint32_t *d_rec, int32_t *d_dst,
                                 float *d_loss, void *stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (!device_ok()) return fail(KGE_ERR_NO_DEVICE, "kge_transe_emit_records_bf16: no usable HIP device");
    if (const char *why = bf16_refusal(m, n_neg)) return fail(KGE_ERR_UNSUPPORTED, std::string("kge_transe_emit_records_bf16: ") + why);
    if (n_pos < 0 || stride < n_pos || denom <= 0 || !d_ent || !d_rel || !d_h || !d_t || !d_r || !d_rec || !d_dst || !d_loss)
        return fail(KGE_ERR_BAD_ARG, "kge_transe_emit_records_bf16: bad arguments");
    if (n_pos == 0) return hip_check(hipMemsetAsync(d_loss, 0, sizeof(float), stream), "zero loss");
    Engine &e = engine();
    int rc = ensure_loss_buffers();
    if (rc) return rc;
    FbArgs a = {};
    if ((rc = transe_defer_buffers(n_pos, stream, a.group_list, a.group_count))) return rc;
    a.bh = d_h; a.bt = d_t; a.br = d_r;
    a.n_pos = n_pos; a.n_neg = n_neg; a.stride = stride;
    a.D = m->ent_dim; a.margin = m->margin; a.unit = 1.0f / (float)denom;
    a.loss_partials = e.dev.loss_partials; a.loss_out = d_loss; a.loss_ticket = e.dev.loss_ticket;
    a.negative_rel = m->negative_rel;
    a.rec = d_rec; a.dst = d_dst; a.ent_total = (int)m->ent_total; a.rel_total = (int)m->rel_total; a.krel = 1;
    const int rec_dw = (int)kge_transe_record_dwords(m);
    guard_loss_stream(stream);
    for_bf16_emit_shape(a.D, [&](auto t) {
        constexpr int L = decltype(t)::L, Q = decltype(t)::C, TEAMS = 256 / L;
        long long blocks = (n_pos + TEAMS - 1) / TEAMS;
        if (blocks > kMaxLossBlocks) blocks = kMaxLossBlocks;
        hipLaunchKernelGGL((transe_emit_bf16_kernel<L, Q>), dim3((unsigned)blocks), dim3(256), 0, stream, a, d_ent, d_rel, rec_dw);
    });
    return hip_check(hipGetLastError(), "bf16 transe emit launch");
}

int kge_transe_apply_rows_sgd_bf16(const kge_model_desc *m, uint16_t *d_ent, uint16_t *d_rel, const int32_t *d_rows, const int32_t *d_row_counts,
                                   const int32_t *d_n_rows, INT max_rows, INT denom, float lr, uint64_t seed, uint64_t step, void *stream) {
    return apply_rows_bf16("kge_transe_apply_rows_sgd_bf16", false, m, d_ent, d_rel, nullptr, nullptr, d_rows, d_row_counts, d_n_rows, max_rows,
                           denom, lr, seed, step, (hipStream_t)stream);
}

int kge_transe_apply_rows_rowadagrad_bf16(const kge_model_desc *m, uint16_t *d_ent, uint16_t *d_rel, float *d_acc_ent, float *d_acc_rel,
                                          const int32_t *d_rows, const int32_t *d_row_counts, const int32_t *d_n_rows, INT max_rows, INT denom,
                                          float lr, uint64_t seed, uint64_t step, void *stream) {
    return apply_rows_bf16("kge_transe_apply_rows_rowadagrad_bf16", true, m, d_ent, d_rel, d_acc_ent, d_acc_rel, d_rows, d_row_counts, d_n_rows,
                           max_rows, denom, lr, seed, step, (hipStream_t)stream);
}

int kge_bf16_round_stochastic(const float *d_y, INT rows, INT D, INT first_key, uint64_t seed, uint64_t step, uint16_t *d_out, void *stream) {
    if (!device_ok()) return fail(KGE_ERR_NO_DEVICE, "kge_bf16_round_stochastic: no usable HIP device");
    if (!d_y || !d_out || rows < 0 || first_key < 0 || D < 8 || D % 8 != 0 || D > 1024)
        return fail(KGE_ERR_BAD_ARG, "kge_bf16_round_stochastic: bad arguments (a width that is a multiple of 8 up to 1024)");
    if (rows == 0) return KGE_OK;
    long long nb = (rows * D + 255) / 256;
    if (nb > 8192) nb = 8192;
    hipLaunchKernelGGL(round_bf16_kernel, dim3((unsigned)nb), dim3(256), 0, (hipStream_t)stream, d_y, (long long)rows, (int)D,
                       (unsigned long long)first_key, bf16_step_key(seed, step), d_out);
    return hip_check(hipGetLastError(), "bf16 rounding launch");
}

}  // extern "C"
