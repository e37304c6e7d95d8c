// Host-side knowledge-graph loader and filter-index builder.
//
// Produces the arrays the device sampler reads.  The reference keeps five copies of the training
// set as 24-byte {h,r,t} structs plus six per-entity range arrays and runs three binary searches
// per corruption (base/Reader.h:82-158, base/Corrupt.h:7-37).  Here the two searches that only
// locate the (anchor, relation) group are done ONCE at load time: every file-order triple carries
// the [offset,length] of its (h,r), (t,r) and (h,t) groups inside three flat int32 value arrays, so
// the device does one 16-byte record load and one monotone search per corruption.
#pragma once
#include <cstdint>
#include <string>
#include <vector>

namespace kge {

struct Int4 { int32_t x, y, z, w; };
struct Int2 { int32_t x, y; };

struct KgIndex {
    int64_t ent_total = 0, rel_total = 0;
    int64_t train_dup = 0;   // trainTotal_  (Reader.h:77)
    int64_t train_uniq = 0;  // trainTotal after dedup (Reader.h:106-123)
    int64_t new_batch = 0;   // newBatchTotal (Reader.h:61-67)
    std::vector<Int4> pos;       // [train_dup]  (h,t,r,0) in file order      == trainList_no
    std::vector<Int4> grp;       // [train_dup]  (hr_off,hr_len,tr_off,tr_len)
    std::vector<Int2> ht;        // [train_dup]  (ht_off,ht_len)
    std::vector<int32_t> tails_hr;  // [train_uniq] == trainHead[].t
    std::vector<int32_t> heads_tr;  // [train_uniq] == trainTail[].h
    std::vector<int32_t> rels_ht;   // [train_uniq] == trainRel[].r
    std::vector<float> left_mean, right_mean, bern_prob;  // [rel_total]
    // moduli of the filtered pick by multiply-high (build_magic_tables): [T] entries each,
    // ent_magic[len] = floor((2^64-1) / (ent_total - len)), rel_magic the same for rel_total; 0 where the divisor is 0 (never used)
    std::vector<uint64_t> ent_magic, rel_magic;
    bool loaded = false;
    // Type-constrained negative sampling (build_typed_index; empty until typed sampling is switched on).  L_tail(r) / L_head(r):
    // relation r's tail / head type list, sorted, duplicates removed.
    std::vector<int32_t> type_tails, type_heads;   // every L_tail(r) / L_head(r), back to back
    std::vector<Int4> type_bounds;                 // [rel_total]  (tail_off,tail_len,head_off,head_len) into the two arrays above
    // [train_uniq], at the offsets of tails_hr / heads_tr: a group's first typed_len entries are the increasing POSITIONS inside
    // L_tail(r) / L_head(r) of its known tails / heads that occur in the list; the rest of the group's slots hold -1
    std::vector<int32_t> typed_pos_hr, typed_pos_tr;
    std::vector<Int2> typed_len;                   // [train_dup]  (positions of the (h,r) group, positions of the (t,r) group)
    bool typed_built = false;
};

// Reader.h:27-100 text parse (first line of relation2id/entity2id/batch2id, N + N lines "h t r").
// Returns an empty string on success, else the reference's "`path` does not exist" style message.
std::string load_openke_dir(const std::string &dir, int64_t &ent_total, int64_t &rel_total, int64_t &new_batch,
                            std::vector<int64_t> &h, std::vector<int64_t> &t, std::vector<int64_t> &r);

// every whitespace-separated integer of a text file (fscanf("%ld") semantics); false if it cannot be opened
bool read_all_longs(const std::string &path, std::vector<int64_t> &out);

// Reader.h:102-177: dedup, the three sort orders, group ranges, tails-per-head / heads-per-tail.
std::string build_index(KgIndex &ix, int64_t ent_total, int64_t rel_total, int64_t new_batch, int64_t n,
                        const int64_t *h, const int64_t *t, const int64_t *r);

// Reader.h:160-177 + Base.cpp:117 from the three per-relation integer counts (shared by the host and device builds)
void relation_means(KgIndex &ix, const std::vector<int64_t> &freq_rel, const std::vector<int64_t> &groups_hr,
                    const std::vector<int64_t> &groups_tr);

// The arrays of type-constrained sampling from the imported type lists (importTypeFiles: per relation [lef, rig) into
// head_type / tail_type, each range sorted, duplicates kept).  One binary search per known (group, entity).  Returns an empty
// string on success.
std::string build_typed_index(KgIndex &ix, const std::vector<int32_t> &head_lef, const std::vector<int32_t> &head_rig,
                              const std::vector<int32_t> &head_type, const std::vector<int32_t> &tail_lef,
                              const std::vector<int32_t> &tail_rig, const std::vector<int32_t> &tail_type);

// Evaluation lists from arrays (kge_import_eval_arrays; what importTestFiles builds from the three text files, Reader.h:186-261):
// `all` = test + train + valid as (h,r,t,0) sorted by (h,r,t), `test` and `valid` as (h,t,r,0) sorted by (r,h,t) (Triple.h:18-32),
// duplicates kept.  train = KgIndex::pos, the file-order training triples.  The ids were range-checked by the caller.
void build_eval_lists(const std::vector<Int4> &train, int64_t n_valid, const int64_t *vh, const int64_t *vt, const int64_t *vr,
                      int64_t n_test, const int64_t *th, const int64_t *tt, const int64_t *tr, std::vector<Int4> &all,
                      std::vector<Int4> &test, std::vector<Int4> &valid);

// Per-relation type lists derived from `all` (main_spark.py:209-290 n_n()): the distinct heads and the distinct tails of every
// relation, each list increasing, as [lef[r], rig[r]) into head_type / tail_type; a relation without triples gets lef == rig ==
// the running offset.
void derive_type_lists(const std::vector<Int4> &all, int64_t rel_total, std::vector<int32_t> &head_lef, std::vector<int32_t> &head_rig,
                       std::vector<int32_t> &head_type, std::vector<int32_t> &tail_lef, std::vector<int32_t> &tail_rig,
                       std::vector<int32_t> &tail_type);

// glibc rand() with the default seed, continuing across calls (Random.h:9-13 never calls srand).
class LibcRand {
   public:
    LibcRand();
    int32_t next();

   private:
    uint32_t s_[31];
    int f_, r_;
};

// 64-bit LCG of Random.h:16-19 and its jump-ahead table: after 2^j steps x -> mulA[j]*x + addC[j].
constexpr uint64_t kLcgMul = 25214903917ULL;
constexpr uint64_t kLcgAdd = 11ULL;
struct LcgJumpTable { uint64_t mulA[64]; uint64_t addC[64]; };
LcgJumpTable make_jump_table();
uint64_t lcg_jump(const LcgJumpTable &tab, uint64_t state, uint64_t steps);
// The same jumps by 9-bit digits: entry [k * 512 + d] is the map x -> mul * x + add of d * 512^k steps (d = 0: the identity),
// four levels, so any count below 2^36 is at most four multiply-adds whose table entries can all be requested at once.
constexpr int kJumpDigitBits = 9, kJumpDigitLevels = 4;
struct LcgAffine { uint64_t mul, add; };
std::vector<LcgAffine> make_jump_digit_table(const LcgJumpTable &tab);
// KgIndex::ent_magic / rel_magic for group lengths below T
void build_magic_tables(KgIndex &ix, int64_t T);

// Base.cpp:85-92: half-open slice [lef,rig) of batch positions owned by virtual thread `id`.
inline void thread_slice(int64_t batch, int64_t threads, int64_t id, int64_t &lef, int64_t &rig) {
    if (batch % threads == 0) {
        lef = id * (batch / threads);
        rig = (id + 1) * (batch / threads);
    } else {
        lef = id * (batch / threads + 1);
        rig = (id + 1) * (batch / threads + 1);
        if (rig > batch) rig = batch;
        if (lef > batch) lef = batch;
    }
}

}  // namespace kge
