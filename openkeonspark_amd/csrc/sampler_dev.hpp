// Device side of the negative sampler shared by sampler.hip (one launch per batch) and persist.hip (sampling inside a
// persistent multi-step launch): the 64-bit LCG with jump-ahead (Random.h:16-34), exact modulo without 64-bit division,
// the closed form of the filtered pick (Corrupt.h:25-36), and one scored triple of a batch (Base.cpp:95-140).
#pragma once
#include "engine.hpp"

namespace kge {

static __constant__ LcgJumpTable c_jump;     // one copy per translation unit that samples (sampler.hip, persist.hip)
static bool g_jump_uploaded = false;

static inline int upload_jump_table() {
    if (g_jump_uploaded) return KGE_OK;
    int rc = hip_check(hipMemcpyToSymbol(HIP_SYMBOL(c_jump), &engine().jump, sizeof(LcgJumpTable)), "upload jump table");
    if (rc == KGE_OK) g_jump_uploaded = true;
    return rc;
}

struct SamplerArgs {
    const int4 *pos;
    const int4 *grp;
    const int2 *ht;
    const int32_t *tails_hr, *heads_tr, *rels_ht;
    const float *bern_prob;
    const uint64_t *streams;
    uint64_t *streams_next;   // sample_kernel: every stream's state after this batch (null: not written)
    long long W, B;           // virtual threads, global batch (for streams_next)
    int32_t *out_h, *out_t, *out_r;
    // sample_block only, null = not written: pack[(b << kshift) + k] says in one word what the TransE emit kernel needs of slot k
    // of local positive b -- bits 0..27 the row it gathers, bits 28..29 the corruption (0 new head, 1 new tail, 2 new relation),
    // bit 31 not a single-slot corruption; slot 0 and the padding slots are 0.  A group's negatives are one contiguous run (one
    // 128-byte line at 25 negatives) where the h/t/r arrays hold them out_stride words apart.
    int32_t *pack;
    long long per_thread;  // positions per virtual thread: B/W, or B/W+1 when W does not divide B
    long long pos_lo;      // first global batch position written by this launch
    long long n_local;     // positions written by this launch
    long long out_stride;
    long long train_dup, new_batch;
    unsigned long long pick_div, pick_magic;   // divisor of the positive pick and floor((2^64-1)/divisor)
    int ent_total, rel_total;
    int neg, negrel, bern;
    int kshift;            // log2 of the lane slots per positive
    // a PART of the sampler's grid riding in another kernel's launch (take_attached_sampler): the rider's extra workgroup i runs
    // workgroup ride_first + i of ride_total
    unsigned ride_first, ride_total;
    // tables of the device index (DeviceIndex): the LCG's jumps by 9-bit digits (kg_index.hpp make_jump_digit_table) and the
    // multiply-high constants of the filtered pick's modulus for group lengths below magic_len (KgIndex::ent_magic / rel_magic)
    const LcgAffine *jump_digits;
    const uint64_t *ent_magic, *rel_magic;
    int magic_len;
};

// where build_sampler / the persistent launch take them from
static inline void set_sampler_tables(SamplerArgs &a) {
    const Engine &e = engine();
    a.jump_digits = e.dev.jump_digits; a.ent_magic = e.dev.ent_magic; a.rel_magic = e.dev.rel_magic;
    a.magic_len = (int)e.sampler_magic_len;
}

// Type-constrained sampling: what the TYPED instantiations read on top of that -- the arrays of KgIndex's typed part.  A type of
// its own, so that SamplerArgs, a by-value argument of every kernel a sampler rides in, stays as it is: those kernels are
// compiled from the untyped body and do not change with this mode.
struct TypedSamplerArgs : SamplerArgs {
    const int2 *typed_len = nullptr;          // [train_dup], loaded together with pos / grp
    const int4 *type_bounds = nullptr;        // [rel_total]
    const int32_t *type_tails = nullptr, *type_heads = nullptr, *typed_pos_hr = nullptr, *typed_pos_tr = nullptr;
};
template <bool TYPED> struct SamplerArgsOf { using type = SamplerArgs; };
template <> struct SamplerArgsOf<true> { using type = TypedSamplerArgs; };

__device__ __forceinline__ uint64_t lcg_step(uint64_t s) { return s * kLcgMul + kLcgAdd; }

__device__ __forceinline__ uint64_t lcg_skip(uint64_t s, uint64_t n) {
    for (int j = 0; n != 0; ++j, n >>= 1)
        if (n & 1) s = c_jump.mulA[j] * s + c_jump.addC[j];
    return s;
}

// The same jump from the digit tables: a 16-byte entry and a multiply-add per digit instead of a data-dependent loop over the
// bits, and every entry is requested before the first multiply.  The tables never change while a kernel runs and are read
// through the constant address space, so a wave-uniform n (sample_block) takes scalar loads and a per-lane n (sample_slot) vector
// loads.  Counts beyond the tables (2^36) keep the bit loop.
typedef unsigned long long u64x2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ u64x2 jump_digit(const LcgAffine *dig, int level, unsigned d) {
    return ((const __attribute__((address_space(4))) u64x2 *)dig)[(level << kJumpDigitBits) + (int)(d & ((1u << kJumpDigitBits) - 1u))];
}
// (requested and applied in two steps, so that a caller can put other requests between them)
struct LcgJump { u64x2 e0, e1, e2, e3; };
__device__ __forceinline__ LcgJump lcg_jump_request(const LcgAffine *dig, uint64_t n) {
    LcgJump j;
    j.e0 = jump_digit(dig, 0, (unsigned)n); j.e1 = jump_digit(dig, 1, (unsigned)(n >> kJumpDigitBits));
    j.e2 = j.e3 = u64x2{1ull, 0ull};
    if (n >> (2 * kJumpDigitBits)) {
        j.e2 = jump_digit(dig, 2, (unsigned)(n >> (2 * kJumpDigitBits))); j.e3 = jump_digit(dig, 3, (unsigned)(n >> (3 * kJumpDigitBits)));
    }
    return j;
}
__device__ __forceinline__ uint64_t lcg_jump_apply(const LcgJump &j, uint64_t s, uint64_t n) {
    if (n >> (kJumpDigitBits * kJumpDigitLevels)) return lcg_skip(s, n);
    s = j.e1.x * (j.e0.x * s + j.e0.y) + j.e1.y;
    if (n >> (2 * kJumpDigitBits)) s = j.e3.x * (j.e2.x * s + j.e2.y) + j.e3.y;
    return s;
}
__device__ __forceinline__ uint64_t lcg_skip_tab(const LcgAffine *dig, uint64_t s, uint64_t n) {
    return lcg_jump_apply(lcg_jump_request(dig, n), s, n);
}

// s % d for a 64-bit LCG state, exact, without the 64-bit division sequence (~100 instructions each, three per thread):
// d known on the host -> multiply-high by m = floor((2^64-1)/d), at most two corrections
__device__ __forceinline__ uint64_t mod_magic(uint64_t s, uint64_t d, uint64_t m) {
    uint64_t r = s - __umul64hi(s, m) * d;
    while (r >= d) r -= d;
    return r;
}
// d < 2^31 known only per thread: two rounds of fp64 reciprocal division; each quotient is < 2^32, so the fp64
// estimate is within one of the truth and one correction step each makes it exact
__device__ __forceinline__ uint32_t mod_u64_u32(uint64_t s, uint32_t d) {
    if (d == 0) return 0;   // a group that already contains every candidate: the reference divides by zero (SIGFPE) here
    const double rcp = 1.0 / (double)d;
    const uint32_t hi = (uint32_t)(s >> 32), lo = (uint32_t)s;
    uint32_t q1 = (uint32_t)((double)hi * rcp);
    int64_t r1 = (int64_t)hi - (int64_t)q1 * d;
    if (r1 < 0) r1 += d;
    if (r1 >= (int64_t)d) r1 -= d;
    const uint64_t x = ((uint64_t)r1 << 32) | lo;                  // < d * 2^32
    const double xd = (double)(uint32_t)r1 * 4294967296.0 + (double)lo;
    uint64_t q2 = (uint64_t)(xd * rcp);
    int64_t r2 = (int64_t)(x - q2 * d);
    if (r2 < 0) r2 += d;
    if (r2 < 0) r2 += d;
    if (r2 >= (int64_t)d) r2 -= d;
    if (r2 >= (int64_t)d) r2 -= d;
    return (uint32_t)r2;
}

// Corrupt.h:25-36 in closed form: the tmp-th id (0-based) that is NOT in the strictly increasing
// list vals[0..len) is tmp + #{j : vals[j] - j <= tmp}; the predicate is monotone in j.
// The bisection itself: how many of the positions [0, len) a monotone predicate (true, ..., true, false, ..., false) holds for.
template <class Pred>
__device__ __forceinline__ int bisect_count(int len, Pred pred) {
    int lo = 0, hi = len;
    while (lo < hi) {
        int mid = (lo + hi) >> 1;
        if (pred(mid)) lo = mid + 1; else hi = mid;
    }
    return lo;
}
__device__ __forceinline__ int filtered_pick(const int32_t *__restrict__ vals, int len, long long tmp) {
    return (int)(tmp + bisect_count(len, [&](int mid) { return (long long)vals[mid] - mid <= tmp; }));
}
// Is `id` one of the strictly increasing vals[0..len)?  The membership form of the same search (kge_shared_negatives_draw's mask).
__device__ __forceinline__ bool sorted_contains(const int32_t *__restrict__ vals, int len, int id) {
    const int at = bisect_count(len, [&](int mid) { return vals[mid] < id; });
    return at < len && vals[at] == id;
}

// The draw of one corruption (Corrupt.h:25-36): tmp = s mod (total - len), then the same pick by an (M + 1)-ary search -- a level
// requests its M pivots together (clamped, unconditional), counts the true ones of the monotone predicate and keeps the one
// part of the range the answer can still lie in, so a list of up to M ids takes one memory round trip, up to (M + 1)^2 - 1 two,
// where the bisection takes one per bit.  The first level's pivots do not depend on tmp: they are requested together with
// the modulus' constant magic[len] (len < magic_len; longer groups keep mod_u64_u32).  total - len = 0 gives tmp = 0 as there.
constexpr int kPickFan =
#ifdef KGE_PICK_FAN
    KGE_PICK_FAN;
#else
    4;
#endif
template <int M>
__device__ __forceinline__ int filtered_pick_wide(const int32_t *__restrict__ vals, int len, int total, const uint64_t *__restrict__ magic,
                                                  int magic_len, uint64_t s) {
    int lo = 0, hi = len, v[M];
    int step = (len + M) / (M + 1);
    const int last = len > 0 ? len - 1 : 0;   // (a group has at least one slot, so slot 0 can always be read)
#pragma unroll
    for (int j = 0; j < M; j++) v[j] = vals[min((j + 1) * step - 1 < 0 ? 0 : (j + 1) * step - 1, last)];
    const uint32_t d = (uint32_t)(total - len);
    int tmp;
    if (len < magic_len) {
        const uint64_t m = magic[len];
        uint64_t r = s - __umul64hi(s, m) * d;   // < 3 d
        if (r >= d) r -= d;
        if (r >= d) r -= d;
        tmp = d == 0 ? 0 : (int)r;
    } else
        tmp = (int)mod_u64_u32(s, d);
    while (lo < hi) {
        int t = 0;
#pragma unroll
        for (int j = 0; j < M; j++) {
            const int p = lo + (j + 1) * step - 1;
            t += (p < hi && v[j] - p <= tmp) ? 1 : 0;   // (ids and positions are below 2^31 and v[j] >= p)
        }
        lo += t * step;                               // pivots below lo are true,
        if (t < M) hi = min(hi, lo + step - 1);       // the first false one bounds the count from above
        if (lo >= hi) break;
        step = (hi - lo + M) / (M + 1);
#pragma unroll
        for (int j = 0; j < M; j++) v[j] = vals[min(lo + (j + 1) * step - 1, hi - 1)];
    }
    return tmp + lo;
}

// Type-constrained corruption: the replacement comes from the relation's own tail (new_tail) or head type list L, minus the known
// tails of (h, r) / heads of (t, r) that occur in it.  K' = the increasing positions inside L of those known ids (typed_pos_hr /
// typed_pos_tr, `len` of them at the group's offset), c = |L| - |K'|: the pick is filtered_pick's closed form on POSITIONS with
// tmp = s mod c, then one gather L[pos] -- the only load that depends on the others.  SHORT: up to four positions are requested
// together with the relation's bounds (clamped, unconditional: a group has at least one slot, so slot 0 can always be read).
// Returns -1 when c = 0 (no list, or the group exhausts it): the caller then makes the reference's untyped draw from the same s.
template <bool SHORT>
__device__ __forceinline__ int typed_pick(const TypedSamplerArgs &a, uint64_t s, bool new_tail, int r, const int4 &gq, const int2 &tl) {
    const int32_t *__restrict__ vals = new_tail ? a.typed_pos_hr + gq.x : a.typed_pos_tr + gq.z;
    const int len = new_tail ? tl.x : tl.y;
    int v[4] = {0, 0, 0, 0};
    if (SHORT) {
        const int last = len > 0 ? len - 1 : 0;
#pragma unroll
        for (int j = 0; j < 4; j++) v[j] = vals[j < last ? j : last];
    }
    const int4 tb = a.type_bounds[r];
    const int loff = new_tail ? tb.x : tb.z, llen = new_tail ? tb.y : tb.w;
    const int c = llen - len;
    if (c <= 0) return -1;
    const long long tmp = (long long)mod_u64_u32(s, (uint32_t)c);
    int pos;
    if (SHORT && len <= 4) {
        int lo = 0;
#pragma unroll
        for (int j = 0; j < 4; j++) lo += (j < len && (long long)v[j] - j <= tmp) ? 1 : 0;
        pos = (int)(tmp + lo);
    } else
        pos = filtered_pick(vals, len, tmp);
    pos = min(pos, llen - 1);   // (never binding for a consistent index)
    return (new_tail ? a.type_tails : a.type_heads)[loff + pos];
}

// One scored triple of the batch: slot k of the positive at global batch position p (k = 0 the positive, 1..neg entity
// negatives, then relation negatives), drawn exactly as virtual thread `id` of the reference draws it (Base.cpp:95-140).
// `skip_batches` whole batches of this thread's slice are skipped first (a persistent launch samples step s from the
// states the launch started with).  TYPED: entity negatives by typed_pick (the random stream is the same either way).
template <bool TYPED = false>
__device__ __forceinline__ void sample_slot(const typename SamplerArgsOf<TYPED>::type &a, long long p, long long k, unsigned long long skip_draws, int &oh, int &ot,
                                            int &orr) {
    const long long id = (long long)((unsigned)p / (unsigned)a.per_thread);   // owning virtual thread (Base.cpp:85-92); B < 2^31
    const long long off = p - id * a.per_thread;  // index inside its slice
    const unsigned long long draws = 1ull + 2ull * a.neg + a.negrel;
    uint64_t s = lcg_skip_tab(a.jump_digits, a.streams[id], skip_draws + (unsigned long long)off * draws);
    s = lcg_step(s);  // Base.cpp:101-106: which training triple
    long long i = (long long)mod_magic(s, a.pick_div, a.pick_magic) + (a.new_batch > 0 ? a.train_dup - a.new_batch : 0);
    const int4 tr = a.pos[i];  // (h, t, r, -)
    const int4 gq = a.grp[i];  // loaded together with it (not after the coin): one memory latency instead of two
    int2 tl = make_int2(0, 0);
    if constexpr (TYPED) tl = a.typed_len[i];
    oh = tr.x; ot = tr.y; orr = tr.z;
    if (k >= 1 && k <= a.neg) {
        s = lcg_skip_tab(a.jump_digits, s, 2ull * (unsigned long long)(k - 1));
        s = lcg_step(s);  // Base.cpp:118: head-or-tail coin, compared in float
        const float prob = a.bern ? a.bern_prob[orr] : 500.0f;
        const bool keep_head = (float)(s % 1000ull) < prob;
        s = lcg_step(s);  // Corrupt.h:25: the one draw of the corruption
        if constexpr (TYPED) {
            const int typed_id = typed_pick<false>(a, s, keep_head, orr, gq, tl);
            if (typed_id >= 0) {
                if (keep_head) ot = typed_id; else oh = typed_id;
                return;
            }
        }
        if (keep_head) {  // corrupt_head(h, r): new TAIL outside tails(h,r)
            long long tmp = (long long)mod_u64_u32(s, (uint32_t)(a.ent_total - gq.y));
            ot = min(filtered_pick(a.tails_hr + gq.x, gq.y, tmp), a.ent_total - 1);   // (clamp: only reachable in that degenerate case)
        } else {          // corrupt_tail(t, r): new HEAD outside heads(t,r)
            long long tmp = (long long)mod_u64_u32(s, (uint32_t)(a.ent_total - gq.w));
            oh = min(filtered_pick(a.heads_tr + gq.z, gq.w, tmp), a.ent_total - 1);
        }
    } else if (k > a.neg) {  // Base.cpp:133-139: corrupt_rel(h, t)
        s = lcg_skip_tab(a.jump_digits, s, 2ull * a.neg + (unsigned long long)(k - 1 - a.neg));
        s = lcg_step(s);
        const int2 g = a.ht[i];
        long long tmp = (long long)mod_u64_u32(s, (uint32_t)(a.rel_total - g.y));
        orr = min(filtered_pick(a.rels_ht + g.x, g.y, tmp), a.rel_total - 1);
    }
}

// every stream's state after this batch, into the OTHER half of the double buffer (the launch reads only the current half,
// so no ordering between blocks is needed and no separate launch either); the host swaps the halves
__device__ __forceinline__ void write_next_streams(const SamplerArgs &a, int kp, long long block, long long n_blocks) {
    for (long long id = block * 256 + threadIdx.x; id < a.W; id += n_blocks * 256) {
        long long lef = id * a.per_thread, rig = lef + a.per_thread;
        if (rig > a.B) rig = a.B;
        if (lef > a.B) lef = a.B;
        a.streams_next[id] = lcg_skip(a.streams[id], (unsigned long long)(rig - lef) * (unsigned long long)(kp + a.neg));
    }
}

// More than 64 slots per positive (over 63 negatives): one independent thread per slot, each with its own full jump.
template <bool TYPED = false>
__device__ __forceinline__ void sample_block_wide(const typename SamplerArgsOf<TYPED>::type &a, long long block, long long n_blocks) {
    const int kshift = a.kshift, kp = 1 + a.neg + a.negrel;
    write_next_streams(a, kp, block, n_blocks);
    for (long long g = block * 256 + threadIdx.x; (g >> kshift) < a.n_local; g += n_blocks * 256) {
        const long long b = g >> kshift;
        const long long k = g & ((1 << kshift) - 1);
        if (k >= kp) continue;
        int oh, ot, orr;
        sample_slot<TYPED>(a, a.pos_lo + b, k, 0ull, oh, ot, orr);
        const long long o = b + k * a.out_stride;
        a.out_h[o] = oh; a.out_t[o] = ot; a.out_r[o] = orr;
    }
}

constexpr int kBernLds = 2048;

// Up to 64 slots per positive (the usual case).  The 1+neg+negrel draws of one positive sit in ADJACENT lanes (k = 0 the
// positive, 1..neg entity negatives, then relation negatives; padded to a power of two <= 64): they read the same pos / grp
// record and search the same groups, so those loads coalesce.  What the slots of a WAVE share is computed once:
//   * the long jump (lcg_skip_tab: slice offset x draws per positive) is done for the wave's FIRST positive only, on
//     wave-uniform values (scalar unit); a lane then advances by the few draws between that state and its own slot -- at
//     most 64 positives' worth, two digits of the jump tables -- instead of repeating the long jump;
//   * the training-triple pick of a positive (one 64-bit modulo) is made by its k = 0 lane and handed to the others;
//   * the Bernoulli table sits in LDS (one dependent global load less per negative).
// Same draws in the same order as Base.cpp:95-140, so the batch is bit-identical to sample_slot's.
// `block` of `n_blocks` 256-thread workgroups: the body of sample_kernel, also run by workgroups that ride along in another
// kernel's launch (transe_counts.hip: the bucket scatter carries the NEXT batch's sampler, see kge_sampling_attach).
// TYPED: entity negatives by typed_pick; only sampler.hip's own kernels instantiate it -- every rider is the untyped body.
template <bool TYPED = false>
__device__ __forceinline__ void sample_block(const typename SamplerArgsOf<TYPED>::type &a, long long block, long long n_blocks, float *bern_lds) {
    const int kshift = a.kshift, kp = 1 + a.neg + a.negrel, kmask = (1 << kshift) - 1;
    const unsigned long long draws = 1ull + 2ull * a.neg + a.negrel;
    write_next_streams(a, kp, block, n_blocks);
    const int lane = threadIdx.x & 63;
    const long long total = a.n_local << kshift;
    const long long wave0 = block * 256 + (__builtin_amdgcn_readfirstlane(threadIdx.x) & ~63);
    // What 64 slots starting at g0 need before anything that depends on memory: the state of the wave's first positive's virtual
    // thread and the digits of its long jump (wave-uniform: scalar loads), and per lane the two digits of its short jump, all
    // requested side by side.
    struct Slots {
        unsigned long long n0;      // draws between the stream's state and the wave's first positive
        uint64_t st0, st;           // that stream's state; the lane's own stream's where it is another one
        LcgJump jump0;
        u64x2 j0, j1;
        long long b;
        int k, kk;
        bool live, same;
    };
    auto request = [&](long long g0) {
        Slots w;
        // ---- wave-uniform: state in front of the first draw of the wave's first positive ----
        const long long p0 = a.pos_lo + (g0 >> kshift);
        const long long id0 = (long long)((unsigned)p0 / (unsigned)a.per_thread);   // owning virtual thread (Base.cpp:85-92); B < 2^31
        const long long off0 = p0 - id0 * a.per_thread;
        w.n0 = (unsigned long long)off0 * draws;
        w.jump0 = lcg_jump_request(a.jump_digits, w.n0);
        // (a launch reads the current half of the stream states and writes the other one: constant while it runs, so this is a
        // scalar load like the digits' and not a vector load whose wait would stand in front of the requests below)
        w.st0 = ((const __attribute__((address_space(4))) uint64_t *)a.streams)[id0];
        // ---- per lane ----
        const long long g = g0 + lane;
        w.b = g >> kshift;
        w.k = (int)(g & kmask);
        w.live = w.b < a.n_local && w.k < kp;
        if (w.b >= a.n_local) w.b = a.n_local - 1;
        w.kk = w.k < kp ? w.k : kp - 1;
        const long long p = a.pos_lo + w.b;
        const long long id = (long long)((unsigned)p / (unsigned)a.per_thread);
        const long long off = p - id * a.per_thread;
        w.same = id == id0;                  // (a wave may cross into the next virtual thread's slice)
        unsigned ahead = (unsigned)((w.same ? off - off0 : off) * (long long)draws);   // < 64 positives' draws
        // draw 0 of a positive picks the training triple; entity negative k uses draws 1 + 2(k-1) (coin) and the next one
        // (corruption); relation negative k uses draw 1 + 2 neg + (k - 1 - neg)   (Base.cpp:101-139)
        if (w.kk >= 1) ahead += w.kk <= a.neg ? 1u + 2u * (unsigned)(w.kk - 1) : 1u + 2u * (unsigned)a.neg + (unsigned)(w.kk - 1 - a.neg);
        // ahead < 2^18 (65 positives of at most 127 draws): two digits
        w.j0 = jump_digit(a.jump_digits, 0, ahead); w.j1 = jump_digit(a.jump_digits, 1, ahead >> kJumpDigitBits);
        w.st = 0;
        if (!w.same) w.st = a.streams[id];
        return w;
    };
    // the first 64 slots' requests go out before the Bernoulli table's, so the two waits are one
    Slots w = request(wave0 < total ? wave0 : 0);
    const bool bern_in_lds = a.bern && a.rel_total <= kBernLds;
    if (bern_in_lds) {
        for (int i = threadIdx.x; i < a.rel_total; i += 256) bern_lds[i] = a.bern_prob[i];
        __syncthreads();
    }
    for (long long g0 = wave0; g0 < total; g0 += n_blocks * 256) {
        if (g0 != wave0) w = request(g0);
        const long long g = g0 + lane, b = w.b;
        const int k = w.k, kk = w.kk;
        const bool live = w.live;
        uint64_t s = w.same ? lcg_jump_apply(w.jump0, w.st0, w.n0) : w.st;
        s = w.j1.x * (w.j0.x * s + w.j0.y) + w.j1.y;
        s = lcg_step(s);                              // k = 0: the pick; entity negative: the coin; relation negative: its draw
        const long long pick = (long long)mod_magic(s, a.pick_div, a.pick_magic) + (a.new_batch > 0 ? a.train_dup - a.new_batch : 0);
        const long long i = __shfl((int)pick, lane & ~kmask);      // the positive's k = 0 lane holds the real one (train_dup < 2^31)
        const int4 tr = a.pos[i];  // (h, t, r, -)
        int4 gq = a.grp[i];        // loaded together with it (not after the coin): one memory latency instead of two
        int2 gr = make_int2(0, 0);
        if (a.negrel > 0) gr = a.ht[i];
        // (only the negatives' lanes use the group records, and the compiler sinks a load into the branch of its only use, behind the
        // wait for pos: a second round trip.  Values that must exist here keep the requests side by side.)
        asm volatile("" : "+v"(gq.x), "+v"(gq.y), "+v"(gq.z), "+v"(gq.w), "+v"(gr.x), "+v"(gr.y));
        int2 tl = make_int2(0, 0);
        if constexpr (TYPED) tl = a.typed_len[i];
        int oh = tr.x, ot = tr.y, orr = tr.z;
        if (kk >= 1) {
            // one path for a new tail (corrupt_head(h, r): outside tails(h,r)), a new head (corrupt_tail(t, r): outside
            // heads(t,r)) and a new relation (Base.cpp:133-139 corrupt_rel(h, t)): the list, its length and the modulus' table are
            // selected, one modulo and one search follow, and selects route the result
            const bool ent = kk <= a.neg;
            bool keep_head = false;
            int typed_id = -1;
            if (ent) {
                const float prob = a.bern ? (bern_in_lds ? bern_lds[orr] : a.bern_prob[orr]) : 500.0f;
                keep_head = (float)(s % 1000ull) < prob;      // Base.cpp:118: compared in float
                s = lcg_step(s);                               // Corrupt.h:25: the one draw of the corruption
                if constexpr (TYPED) typed_id = typed_pick<true>(a, s, keep_head, orr, gq, tl);
            }
            int v = typed_id;
            if (typed_id < 0) {
                const int32_t *vals = !ent ? a.rels_ht + gr.x : (keep_head ? a.tails_hr + gq.x : a.heads_tr + gq.z);
                const int len = !ent ? gr.y : (keep_head ? gq.y : gq.w);
                const int total = ent ? a.ent_total : a.rel_total;
                v = min(filtered_pick_wide<kPickFan>(vals, len, total, ent ? a.ent_magic : a.rel_magic, a.magic_len, s), total - 1);   // (clamp: only reachable when the group holds every candidate)
            }
            orr = ent ? orr : v;
            ot = ent && keep_head ? v : ot;
            oh = ent && !keep_head ? v : oh;
        }
        if (live) {
            const long long o = b + (long long)k * a.out_stride;
            a.out_h[o] = oh; a.out_t[o] = ot; a.out_r[o] = orr;
        }
        if (a.pack && g < total) {   // the wave's 64 consecutive words; classified by the emit kernel's own function, not from the coin
            int w = 0;
            if (live && k >= 1) {
                const NegClass nc = classify_negative<KGE_TRANSE>(tr.x, tr.y, tr.z, oh, ot, orr, 0);
                const int code = !nc.same_h ? 0 : (!nc.same_t ? 1 : 2);
                const int row = !nc.same_h ? oh : (!nc.same_t ? ot : orr);
                w = row | (code << kPackRowBits) | (nc.fast ? 0 : (int)0x80000000u);
            }
            a.pack[g] = w;
        }
    }
}


// workgroup `i` of the part of an armed sampler that rides in this launch
__device__ __forceinline__ void sample_block_ride(const SamplerArgs &a, long long i, float *bern_lds) {
    sample_block<false>(a, (long long)a.ride_first + i, (long long)a.ride_total, bern_lds);
}

}  // namespace kge
