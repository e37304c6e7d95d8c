// The evaluation filter on the device, shared by the rankers (eval.hip, lp_shard.hip) and the top-k selection (topk.hip): the union of
// train + valid + test sorted by (h,r,t), by (t,r,h) and by (h,t,r), and the per-relation head / tail type lists.
#pragma once
#include "engine.hpp"

namespace kge {

// device copies uploaded by eval.hip (importTestFiles / importTypeFiles); read-only for their users
struct EvalFilterView {
    const int4 *all, *all_t;   // (h,r,t,0) sorted by (h,r,t); (t,r,h,0) sorted by (t,r,h)
    const int4 *all_ht;        // (h,t,r,0) sorted by (h,t,r): the known relations of an (h, t) pair are one range
    long long n_all;
    const int32_t *head_lef, *head_rig, *tail_lef, *tail_rig, *head_type, *tail_type;
};
// fills `v` with the uploaded arrays (uploading them on first use); KGE_ERR_NO_DATASET when importTestFiles, or with
// need_types importTypeFiles, has not been called
int eval_filter_view(bool need_types, EvalFilterView &v);
// the uploaded test triples (h,t,r,0) in importTestFiles' (r,h,t) order -- the order kge_link_prediction's [first, first+count)
// indexes -- and their number; KGE_ERR_NO_DATASET before importTestFiles
int eval_test_view(const int4 *&test, int64_t &total);
// the ontology lists of importOntologyFiles (per entity: [sup_lef, sup_rig) of sup_type, [sub_lef, sub_rig) of sub_type, all
// empty without the file), read-only, for resolving arg-min classes as rank_kernel does; KGE_ERR_NO_DATASET before importTestFiles
struct EvalOntologyView {
    const int32_t *sup_lef, *sup_rig, *sub_lef, *sub_rig, *sup_type, *sub_type;
};
int eval_ontology_view(EvalOntologyView &v);

// triple classification (tclass.hip): the per-relation ranges [lef[r], rig[r]] (-1 / -1 without triples) of the validation
// (index 0) and test (index 1) lists sorted by relation, as getBestThreshold / test_triple_classification read them, and the
// lists' lengths.  Host vectors owned by eval.hip, rebuilt by the call; KGE_ERR_NO_DATASET (with the host routines' message)
// before importTestFiles.  eval_tc_generation changes with every importTestFiles.
struct TcLists {
    const std::vector<int32_t> *lef[2], *rig[2];
    int64_t total[2];
};
int eval_tc_lists(TcLists &v);
uint64_t eval_tc_generation();

// Device build of the evaluation lists and of derived type lists (eval_build.hip), bit for bit the host builds of kg_index.cpp
// (build_eval_lists plus ensure_eval_device's two further orders; derive_type_lists).  Triples are packed into 64-bit keys, one
// field order per list, radix-sorted up to the bits in use and unpacked straight into the int4 arrays the views hand out:
//   (a,b,c) -> a << (bits(b) + bits(c)) | b << bits(c) | c       needs 2 bits(E) + bits(R) <= 64, as the training index does
bool device_eval_build_supported(int64_t E, int64_t R, int64_t n_all);
struct EvalTriplesBuilt { ScopedDevBuf<int4> all, all_t, all_ht, test, valid; };
// d_train: the file-order training triples (h,t,r,0) on the device; valid / test: (h,t,r,0) on the host, ids already range-checked
int build_eval_lists_device(int64_t E, int64_t R, const int4 *d_train, int64_t n_train, const std::vector<Int4> &valid,
                            const std::vector<Int4> &test, EvalTriplesBuilt &out);
struct TypeListsBuilt {
    ScopedDevBuf<int32_t> head_lef, head_rig, tail_lef, tail_rig, head_type, tail_type;   // lef / rig [R]; the id arrays [n_head] / [n_tail]
    int64_t n_head = 0, n_tail = 0;
};
// d_all: (h,r,t,0), any order.  Keys r << bits(E) | entity per side: sort, flag the first of each equal run, scan, compact, and a
// bound search per relation for [lef, rig)
int derive_type_lists_device(int64_t E, int64_t R, const int4 *d_all, int64_t n_all, TypeListsBuilt &out);

// [lo, hi) of the entries whose first two fields are (a, b) in an array sorted by (x, y, z): the third fields of that
// range are the known tails of (h, r) in `all`, the known heads of (t, r) in `all_t`, or the known relations of (h, t) in
// `all_ht`, in increasing order
__device__ __forceinline__ void pair_range(const int4 *__restrict__ arr, long long n, int a, int b, long long &lo, long long &hi) {
    long long l = 0, r = n;
    while (l < r) { const long long mid = (l + r) >> 1; const int4 m = arr[mid]; if (m.x < a || (m.x == a && m.y < b)) l = mid + 1; else r = mid; }
    lo = l;
    r = n;
    while (l < r) { const long long mid = (l + r) >> 1; const int4 m = arr[mid]; if (m.x < a || (m.x == a && m.y <= b)) l = mid + 1; else r = mid; }
    hi = l;
}
__device__ __forceinline__ bool in_range(const int4 *__restrict__ arr, long long lo, long long hi, int j) {
    const long long end = hi;
    while (lo < hi) { const long long mid = (lo + hi) >> 1; if (arr[mid].z < j) lo = mid + 1; else hi = mid; }
    return lo < end && arr[lo].z == j;
}

}  // namespace kge
