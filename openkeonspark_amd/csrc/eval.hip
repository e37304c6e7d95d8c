// Link-prediction evaluation: the inputs of base/Reader.h:186-449 and the
// ranker of base/Test.h:11-249, with the Base.so entry points kept (importTestFiles, importTypeFiles,
// importOntologyFiles, getHeadBatch, getTailBatch, testHead, testTail) and a device-native batch
// entry (kge_link_prediction) that never moves the E-long score vectors over PCIe.
//
// Ranker on the device: one workgroup per (test triple, side).  Every thread walks candidates
// j = tid, tid+256, ...; a candidate scoring strictly lower than the expected entity bumps the raw
// count, the filtered count unless (j,r,t)/(h,r,j) is a known triple (binary search in the
// (h,r,t)-sorted union of train+valid+test, Corrupt.h:104-115), and the type-constrained counts when
// j is in the relation's sorted head/tail type list.  The four arg-mins are lexicographic minima
// over (score, j) -- the sequential loop's strict `<` keeps the first (smallest j) minimum -- and
// their ontology classes are resolved by one thread with the reference's non-rewinding cursors.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>

#include "eval_dev.hpp"

namespace kge {

struct EvalHost {
    bool loaded = false, types = false, onto = false;
    // kge_import_eval_arrays / kge_derive_type_lists on the device (eval_build.hip): EvalDev already holds the five triple lists /
    // the six type arrays, and ensure_eval_device uploads only the rest
    bool dev_triples = false, dev_types = false;
    int64_t test_total = 0, valid_total = 0, triple_total = 0;
    std::vector<Int4> test;         // (h,t,r,0) sorted by (r,h,t)   Reader.h:256
    std::vector<Int4> all;          // (h,r,t,0) sorted by (h,r,t)   Reader.h:255
    std::vector<int32_t> head_lef, head_rig, tail_lef, tail_rig, head_type, tail_type;
    std::vector<int32_t> sup_lef, sup_rig, sub_lef, sub_rig, sup_type, sub_type;
};

struct EvalDev {
    bool uploaded = false;
    DevBuf<int4> test, all, all_t;   // all_t: the same triples as (t,r,h,0) sorted by (t,r,h)
    DevBuf<int4> all_ht;             // ... and as (h,t,r,0) sorted by (h,t,r) (relation prediction's filter)
    DevBuf<int4> valid;              // device build only: the validation list, (h,t,r,0) sorted by (r,h,t)
    DevBuf<int32_t> head_lef, head_rig, tail_lef, tail_rig, head_type, tail_type;
    DevBuf<int32_t> sup_lef, sup_rig, sub_lef, sub_rig, sup_type, sub_type;
    DevBuf<float> scores;         // staging for testHead/testTail and kge_link_prediction
    DevBuf<int32_t> cand;         // link_prediction_v1: [3][requests x E] candidate ids
    DevBuf<long long> out;        // 8 * requests
    DevBuf<int32_t> req_one;      // testHead/testTail: (test index, head flag)
    DevBuf<int32_t> req_v1;       // link_prediction_v1: [2][64] test index, head flag
    DevBuf<int32_t> req;          // kge_link_prediction: [3][requests] test index, head flag, fixed entity
    DevBuf<float> T, P;           // kge_link_prediction: the relation's candidate table, TransR's projections
};

static EvalHost g_eh;
static EvalDev g_ed;
// triple classification: valid triples (h,t,r) sorted by (r,h,t) (Reader.h:257) and the per-relation
// ranges of the sorted valid / test lists (Reader.h:263-291)
static std::vector<Int4> g_valid;
static std::vector<int32_t> g_valid_lef, g_valid_rig, g_test_lef, g_test_rig;
// bumped by every importTestFiles: tclass.hip keeps device copies of the four range arrays for as long as it stands
static uint64_t g_tc_generation = 0;

static int ensure_eval_device() {
    if (!g_eh.loaded) return fail(KGE_ERR_NO_DATASET, "importTestFiles has not been called");
    if (!device_ok()) return fail(KGE_ERR_NO_DEVICE, "no usable HIP device: the ranker has no CPU fallback");
    if (g_ed.uploaded) return KGE_OK;
    int rc;
    const int64_t E = engine().index.ent_total, R = engine().index.rel_total;
    if (g_eh.head_lef.empty()) { g_eh.head_lef.assign(R, 0); g_eh.head_rig.assign(R, 0); g_eh.tail_lef.assign(R, 0); g_eh.tail_rig.assign(R, 0); }
    if (g_eh.sup_lef.empty()) { g_eh.sup_lef.assign(E, 0); g_eh.sup_rig.assign(E, 0); g_eh.sub_lef.assign(E, 0); g_eh.sub_rig.assign(E, 0); }
    if (!g_eh.dev_triples) {
        if ((rc = g_ed.test.upload(g_eh.test, "upload test"))) return rc;
        if ((rc = g_ed.all.upload(g_eh.all, "upload triples"))) return rc;
        {   // second order for head requests: the known heads of a (t, r) pair are then contiguous
            std::vector<Int4> by_tail(g_eh.all.size());
            for (size_t i = 0; i < by_tail.size(); i++) by_tail[i] = Int4{g_eh.all[i].z, g_eh.all[i].y, g_eh.all[i].x, 0};
            std::sort(by_tail.begin(), by_tail.end(), [](const Int4 &a, const Int4 &b) {
                if (a.x != b.x) return a.x < b.x; if (a.y != b.y) return a.y < b.y; return a.z < b.z; });
            if ((rc = g_ed.all_t.upload(by_tail, "upload triples by tail"))) return rc;
        }
        {   // third order for relation prediction: the known relations of an (h, t) pair are then contiguous
            std::vector<Int4> by_pair(g_eh.all.size());
            for (size_t i = 0; i < by_pair.size(); i++) by_pair[i] = Int4{g_eh.all[i].x, g_eh.all[i].z, g_eh.all[i].y, 0};
            std::sort(by_pair.begin(), by_pair.end(), [](const Int4 &a, const Int4 &b) {
                if (a.x != b.x) return a.x < b.x; if (a.y != b.y) return a.y < b.y; return a.z < b.z; });
            if ((rc = g_ed.all_ht.upload(by_pair, "upload triples by pair"))) return rc;
        }
    }
    if (!g_eh.dev_types) {
        if ((rc = g_ed.head_lef.upload(g_eh.head_lef, "upload types"))) return rc;
        if ((rc = g_ed.head_rig.upload(g_eh.head_rig, "upload types"))) return rc;
        if ((rc = g_ed.tail_lef.upload(g_eh.tail_lef, "upload types"))) return rc;
        if ((rc = g_ed.tail_rig.upload(g_eh.tail_rig, "upload types"))) return rc;
        if ((rc = g_ed.head_type.upload(g_eh.head_type, "upload types"))) return rc;
        if ((rc = g_ed.tail_type.upload(g_eh.tail_type, "upload types"))) return rc;
    }
    if ((rc = g_ed.sup_lef.upload(g_eh.sup_lef, "upload ontology"))) return rc;
    if ((rc = g_ed.sup_rig.upload(g_eh.sup_rig, "upload ontology"))) return rc;
    if ((rc = g_ed.sub_lef.upload(g_eh.sub_lef, "upload ontology"))) return rc;
    if ((rc = g_ed.sub_rig.upload(g_eh.sub_rig, "upload ontology"))) return rc;
    if ((rc = g_ed.sup_type.upload(g_eh.sup_type, "upload ontology"))) return rc;
    if ((rc = g_ed.sub_type.upload(g_eh.sub_type, "upload ontology"))) return rc;
    g_ed.uploaded = true;
    return KGE_OK;
}

int eval_filter_view(bool need_types, EvalFilterView &v) {
    if (!g_eh.loaded) return fail(KGE_ERR_NO_DATASET, "importTestFiles has not been called: no known triples to filter by");
    if (need_types && !g_eh.types) return fail(KGE_ERR_NO_DATASET, "importTypeFiles has not been called: no relation type lists");
    int rc = ensure_eval_device();
    if (rc) return rc;
    v.all = g_ed.all; v.all_t = g_ed.all_t; v.all_ht = g_ed.all_ht; v.n_all = (long long)g_eh.all.size();
    v.head_lef = g_ed.head_lef; v.head_rig = g_ed.head_rig; v.tail_lef = g_ed.tail_lef; v.tail_rig = g_ed.tail_rig;
    v.head_type = g_ed.head_type; v.tail_type = g_ed.tail_type;
    return KGE_OK;
}

bool eval_type_lists_host(TypeListsHost &v) {
    v = TypeListsHost{&g_eh.head_lef, &g_eh.head_rig, &g_eh.head_type, &g_eh.tail_lef, &g_eh.tail_rig, &g_eh.tail_type};
    return g_eh.types;
}

int eval_test_view(const int4 *&test, int64_t &total) {
    int rc = ensure_eval_device();
    if (rc) return rc;
    test = g_ed.test;
    total = g_eh.test_total;
    return KGE_OK;
}

int eval_ontology_view(EvalOntologyView &v) {
    int rc = ensure_eval_device();
    if (rc) return rc;
    v.sup_lef = g_ed.sup_lef; v.sup_rig = g_ed.sup_rig; v.sub_lef = g_ed.sub_lef; v.sub_rig = g_ed.sub_rig;
    v.sup_type = g_ed.sup_type; v.sub_type = g_ed.sub_type;
    return KGE_OK;
}

// ---------------------------------------------------------------------------------------------
struct RankArgs {
    const float *scores;     // [n_req][E]
    const int4 *test, *all, *all_t;
    long long n_all;
    const int32_t *head_lef, *head_rig, *tail_lef, *tail_rig, *head_type, *tail_type;
    const int32_t *sup_lef, *sup_rig, *sub_lef, *sub_rig, *sup_type, *sub_type;
    const int32_t *req_index;  // [n_req] test triple index
    const int32_t *req_head;   // [n_req] 1 = replace head, 0 = replace tail
    long long *out;            // [n_req][8]
    int E;
};

struct MinPair { float v; int j; };
__device__ __forceinline__ void take(MinPair &a, float v, int j) { if (v < a.v || (v == a.v && j < a.j)) { a.v = v; a.j = j; } }

__global__ __launch_bounds__(256) void rank_kernel(RankArgs a) {
    const int req = blockIdx.x;
    const float *con = a.scores + (long long)req * a.E;
    const int4 tt = a.test[a.req_index[req]];  // (h, t, r)
    const bool head = a.req_head[req] != 0;
    const int h = tt.x, t = tt.y, r = tt.z;
    const int target = head ? h : t;
    const float minimal = con[target];
    const int lef = head ? a.head_lef[r] : a.tail_lef[r], rig = head ? a.head_rig[r] : a.tail_rig[r];
    const int32_t *types = head ? a.head_type : a.tail_type;
    // the filter (Corrupt.h:104-115 `_find` over train+valid+test): the known tails of (h, r) / heads of (t, r) are one
    // contiguous, sorted range, located once per request; a candidate then costs a search in that short range
    __shared__ long long s_known[2];
    if (threadIdx.x == 0) {
        long long lo, hi;
        if (head) pair_range(a.all_t, a.n_all, t, r, lo, hi); else pair_range(a.all, a.n_all, h, r, lo, hi);
        s_known[0] = lo; s_known[1] = hi;
    }
    __syncthreads();
    const long long known_lo = s_known[0], known_hi = s_known[1];
    const int4 *known_arr = head ? a.all_t : a.all;
    long long c[4] = {0, 0, 0, 0};
    // arg-min candidates start at (minimal, target); a candidate must be STRICTLY lower to replace it
    MinPair m[4];
    for (int i = 0; i < 4; i++) { m[i].v = minimal; m[i].j = 0x7fffffff; }
    for (int j = threadIdx.x; j < a.E; j += 256) {
        if (j == target) continue;
        const float value = con[j];
        if (!(value < minimal)) continue;
        const bool known = in_range(known_arr, known_lo, known_hi, j);
        bool typed = false;
        {   // lower_bound in the relation's sorted type list
            int lo = lef, hi = rig;
            while (lo < hi) { const int mid = (lo + hi) >> 1; if (types[mid] < j) lo = mid + 1; else hi = mid; }
            typed = lo < rig && types[lo] == j;
        }
        c[0]++; take(m[0], value, j);
        if (!known) c[1]++;
        if (head || !known) take(m[1], value, j);   // Test.h:69-74: the head version updates this arg-min outside the filter
        if (typed) { c[2]++; take(m[2], value, j); if (!known) { c[3]++; take(m[3], value, j); } }
    }
    __shared__ long long sc[4][256];
    __shared__ float sv[4][256];
    __shared__ int sj[4][256];
    for (int i = 0; i < 4; i++) { sc[i][threadIdx.x] = c[i]; sv[i][threadIdx.x] = m[i].v; sj[i][threadIdx.x] = m[i].j; }
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) {
            for (int i = 0; i < 4; i++) {
                sc[i][threadIdx.x] += sc[i][threadIdx.x + w];
                MinPair x = {sv[i][threadIdx.x], sj[i][threadIdx.x]};
                take(x, sv[i][threadIdx.x + w], sj[i][threadIdx.x + w]);
                sv[i][threadIdx.x] = x.v; sj[i][threadIdx.x] = x.j;
            }
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        long long *o = a.out + (long long)req * 8;
        int arg[4];
        for (int i = 0; i < 4; i++) { o[i] = sc[i][0]; arg[i] = sv[i][0] < minimal ? sj[i][0] : target; }
        // ontology classes with the reference's shared, never-rewinding cursors (Test.h:113-135)
        int lsup = a.sup_lef[target], rsup = a.sup_rig[target], lsub = a.sub_lef[target], rsub = a.sub_rig[target];
        for (int i = 0; i < 4; i++) {
            const int v = arg[i];
            long long cls = 3;
            if (v == target) cls = 0;
            else {
                while (lsup < rsup && a.sup_type[lsup] < v) lsup++;
                if (lsup < rsup && a.sup_type[lsup] == v) cls = 1;
                else {
                    while (lsub < rsub && a.sub_type[lsub] < v) lsub++;
                    if (lsub < rsub && a.sub_type[lsub] == v) cls = 2;
                }
            }
            o[4 + i] = cls;
        }
    }
}

// candidates of getTailBatch / getHeadBatch (Test.h:11-26) for a batch of requests, on the device
__global__ void candidates_kernel(const int4 *__restrict__ test, const int32_t *__restrict__ req_index,
                                  const int32_t *__restrict__ req_head, int n_req, int E, int32_t *__restrict__ ch,
                                  int32_t *__restrict__ ct, int32_t *__restrict__ cr) {
    const long long total = (long long)n_req * E;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        const int q = (int)(i / E), j = (int)(i - (long long)q * E);
        const int4 tt = test[req_index[q]];
        const bool head = req_head[q] != 0;
        ch[i] = head ? j : tt.x;
        ct[i] = head ? tt.y : j;
        cr[i] = tt.z;
    }
}

static int rank_requests(const float *d_scores, const std::vector<int32_t> &index, const std::vector<int32_t> &head,
                         long long *h_out, hipStream_t stream, const int32_t *d_req_index, const int32_t *d_req_head) {
    const int n = (int)index.size();
    { int rc = g_ed.out.reserve(8 * (int64_t)n, "alloc rank out"); if (rc) return rc; }
    RankArgs a;
    a.scores = d_scores; a.test = g_ed.test; a.all = g_ed.all; a.all_t = g_ed.all_t; a.n_all = (long long)g_eh.all.size();
    a.head_lef = g_ed.head_lef; a.head_rig = g_ed.head_rig; a.tail_lef = g_ed.tail_lef; a.tail_rig = g_ed.tail_rig;
    a.head_type = g_ed.head_type; a.tail_type = g_ed.tail_type;
    a.sup_lef = g_ed.sup_lef; a.sup_rig = g_ed.sup_rig; a.sub_lef = g_ed.sub_lef; a.sub_rig = g_ed.sub_rig;
    a.sup_type = g_ed.sup_type; a.sub_type = g_ed.sub_type;
    a.req_index = d_req_index; a.req_head = d_req_head; a.out = g_ed.out; a.E = (int)engine().index.ent_total;
    hipLaunchKernelGGL(rank_kernel, dim3(n), dim3(256), 0, stream, a);
    int rc = hip_check(hipMemcpyAsync(h_out, g_ed.out, sizeof(long long) * 8 * (size_t)n, hipMemcpyDeviceToHost, stream), "copy ranks");
    if (rc) return rc;
    return hip_check(hipStreamSynchronize(stream), "rank sync");
}

}  // namespace kge

using namespace kge;

extern "C" {

static bool ensure_classification_lists();

void importTestFiles(void) {
    Engine &e = engine();
    g_eh = EvalHost();
    g_ed.uploaded = false;
    e.index.typed_built = false;   // the type lists go with the rest: typed sampling needs importTypeFiles again
    g_valid.clear();
    g_tc_generation++;
    std::vector<int64_t> te, tr, va, tmp;
    const std::string &d = e.in_path;
    if (!read_all_longs(d + "relation2id.txt", tmp)) { set_error("`" + d + "relation2id.txt` does not exist"); return; }
    if (!read_all_longs(d + "entity2id.txt", tmp)) { set_error("`" + d + "entity2id.txt` does not exist"); return; }
    if (!read_all_longs(d + "test2id.txt", te)) { set_error("`" + d + "test2id.txt` does not exist"); return; }
    if (!read_all_longs(d + "train2id.txt", tr)) { set_error("`" + d + "train2id.txt` does not exist"); return; }
    if (!read_all_longs(d + "valid2id.txt", va)) { set_error("`" + d + "valid2id.txt` does not exist"); return; }
    const int64_t T = te.empty() ? 0 : te[0], Tr = tr.empty() ? 0 : tr[0], V = va.empty() ? 0 : va[0];
    if ((int64_t)te.size() < 1 + 3 * T || (int64_t)tr.size() < 1 + 3 * Tr || (int64_t)va.size() < 1 + 3 * V) { set_error("importTestFiles: truncated triple file"); return; }
    g_eh.test_total = T; g_eh.valid_total = V; g_eh.triple_total = T + Tr + V;
    auto push = [&](const std::vector<int64_t> &src, int64_t n, bool is_test) {
        for (int64_t i = 0; i < n; i++) {  // on disk: head, tail, relation
            const int32_t h = (int32_t)src[1 + 3 * i], t = (int32_t)src[2 + 3 * i], r = (int32_t)src[3 + 3 * i];
            g_eh.all.push_back(Int4{h, r, t, 0});
            if (is_test) g_eh.test.push_back(Int4{h, t, r, 0});
        }
    };
    push(te, T, true); push(tr, Tr, false); push(va, V, false);
    std::sort(g_eh.all.begin(), g_eh.all.end(), [](const Int4 &a, const Int4 &b) {        // Triple.h:18-20
        if (a.x != b.x) return a.x < b.x; if (a.y != b.y) return a.y < b.y; return a.z < b.z; });
    std::sort(g_eh.test.begin(), g_eh.test.end(), [](const Int4 &a, const Int4 &b) {      // Triple.h:30-32 (r,h,t)
        if (a.z != b.z) return a.z < b.z; if (a.x != b.x) return a.x < b.x; return a.y < b.y; });
    std::printf("The total of test triples is %ld.\n", (long)T);
    std::printf("The total of valid triples is %ld.\n", (long)V);
    g_eh.loaded = true;
}

void importTypeFiles(void) {
    Engine &e = engine();
    std::vector<int64_t> a;
    if (!read_all_longs(e.in_path + "type_constrain.txt", a)) { set_error("`" + e.in_path + "type_constrain.txt` does not exist"); return; }
    const int64_t R = e.index.rel_total;
    g_eh.head_lef.assign(R, 0); g_eh.head_rig.assign(R, 0); g_eh.tail_lef.assign(R, 0); g_eh.tail_rig.assign(R, 0);
    g_eh.head_type.clear(); g_eh.tail_type.clear();
    e.index.typed_built = false;   // typed sampling rebuilds its index from the new lists on next use
    size_t p = 1;
    for (int64_t i = 0; i < R && p + 1 < a.size(); i++) {   // Reader.h:344-362
        int64_t rel = a[p], tot = a[p + 1]; p += 2;
        if (rel < 0 || rel >= R || p + tot > a.size()) { set_error("type_constrain.txt: malformed"); return; }
        g_eh.head_lef[rel] = (int32_t)g_eh.head_type.size();
        for (int64_t j = 0; j < tot; j++) g_eh.head_type.push_back((int32_t)a[p++]);
        g_eh.head_rig[rel] = (int32_t)g_eh.head_type.size();
        std::sort(g_eh.head_type.begin() + g_eh.head_lef[rel], g_eh.head_type.end());
        if (p + 1 >= a.size()) break;
        rel = a[p]; tot = a[p + 1]; p += 2;
        if (rel < 0 || rel >= R || p + tot > a.size()) { set_error("type_constrain.txt: malformed"); return; }
        g_eh.tail_lef[rel] = (int32_t)g_eh.tail_type.size();
        for (int64_t j = 0; j < tot; j++) g_eh.tail_type.push_back((int32_t)a[p++]);
        g_eh.tail_rig[rel] = (int32_t)g_eh.tail_type.size();
        std::sort(g_eh.tail_type.begin() + g_eh.tail_lef[rel], g_eh.tail_type.end());
    }
    g_eh.types = true;
    g_eh.dev_types = false;
    g_ed.uploaded = false;
}

void importOntologyFiles(void) {
    Engine &e = engine();
    std::printf("Reading %sontology_constrain.txt\n", e.in_path.c_str());
    std::vector<int64_t> a;
    if (!read_all_longs(e.in_path + "ontology_constrain.txt", a)) { set_error("`" + e.in_path + "ontology_constrain.txt` does not exist"); return; }
    const int64_t E = e.index.ent_total;
    g_eh.sup_lef.assign(E, 0); g_eh.sup_rig.assign(E, 0); g_eh.sub_lef.assign(E, 0); g_eh.sub_rig.assign(E, 0);
    g_eh.sup_type.clear(); g_eh.sub_type.clear();
    const int64_t n = a.empty() ? 0 : a[0];
    size_t p = 1;
    for (int64_t i = 0; i < n && p + 1 < a.size(); i++) {   // Reader.h:425-446
        int64_t ent = a[p], tot = a[p + 1]; p += 2;
        if (ent < 0 || ent >= E || p + tot > a.size()) { set_error("ontology_constrain.txt: malformed"); return; }
        g_eh.sup_lef[ent] = (int32_t)g_eh.sup_type.size();
        for (int64_t j = 0; j < tot; j++) g_eh.sup_type.push_back((int32_t)a[p++]);
        g_eh.sup_rig[ent] = (int32_t)g_eh.sup_type.size();
        std::sort(g_eh.sup_type.begin() + g_eh.sup_lef[ent], g_eh.sup_type.end());
        if (p + 1 >= a.size()) break;
        ent = a[p]; tot = a[p + 1]; p += 2;
        if (ent < 0 || ent >= E || p + tot > a.size()) { set_error("ontology_constrain.txt: malformed"); return; }
        g_eh.sub_lef[ent] = (int32_t)g_eh.sub_type.size();
        for (int64_t j = 0; j < tot; j++) g_eh.sub_type.push_back((int32_t)a[p++]);
        g_eh.sub_rig[ent] = (int32_t)g_eh.sub_type.size();
        std::sort(g_eh.sub_type.begin() + g_eh.sub_lef[ent], g_eh.sub_type.end());
    }
    g_eh.onto = true;
    g_ed.uploaded = false;
}

// ---- evaluation from arrays, type lists without a file (include/kge_mi355.h) ----------------------------------------------
static int bad_id(const char *split, INT n, const INT *h, const INT *t, const INT *r, int64_t E, int64_t R) {
    if (n < 0 || (n > 0 && (!h || !t || !r))) return fail(KGE_ERR_BAD_ARG, std::string("kge_import_eval_arrays: ") + split + ": bad count or null array");
    for (INT i = 0; i < n; i++)
        if (h[i] < 0 || h[i] >= E || t[i] < 0 || t[i] >= E || r[i] < 0 || r[i] >= R)
            return fail(KGE_ERR_BAD_ARG, std::string("kge_import_eval_arrays: ") + split + ": id out of range at index " + std::to_string((long long)i));
    return KGE_OK;
}

// what importTestFiles resets, before the new lists move in
static void reset_eval_state() {
    g_eh = EvalHost();
    g_ed.uploaded = false;
    engine().index.typed_built = false;
    g_valid.clear();
    g_tc_generation++;
}

static int download_int4(std::vector<Int4> &dst, const int4 *src, int64_t n, const char *what) {
    dst.resize((size_t)n);
    if (n == 0) return KGE_OK;
    return hip_check(hipMemcpy(dst.data(), src, sizeof(int4) * (size_t)n, hipMemcpyDeviceToHost), what);
}

static int download_i32(std::vector<int32_t> &dst, const int32_t *src, int64_t n, const char *what) {
    dst.resize((size_t)n);
    if (n == 0) return KGE_OK;
    return hip_check(hipMemcpy(dst.data(), src, sizeof(int32_t) * (size_t)n, hipMemcpyDeviceToHost), what);
}

static bool eval_build_on_device(int64_t n_all) {
    Engine &e = engine();
    const int64_t min = e.eval_index_device_min;
    return min >= 0 && n_all >= min && device_ok() && device_eval_build_supported(e.index.ent_total, e.index.rel_total, n_all);
}

int kge_import_eval_arrays(INT n_valid, const INT *valid_h, const INT *valid_t, const INT *valid_r, INT n_test, const INT *test_h,
                           const INT *test_t, const INT *test_r) {
    Engine &e = engine();
    if (!e.index.loaded) return fail(KGE_ERR_NO_DATASET, "kge_import_eval_arrays: no training set imported (importTrainFiles / kge_import_train_arrays)");
    const int64_t E = e.index.ent_total, R = e.index.rel_total, n_train = e.index.train_dup;
    int rc;
    if ((rc = bad_id("valid", n_valid, valid_h, valid_t, valid_r, E, R))) return rc;
    if ((rc = bad_id("test", n_test, test_h, test_t, test_r, E, R))) return rc;
    const int64_t n_all = n_test + n_train + n_valid;
    if (n_all >= (int64_t(1) << 31)) return fail(KGE_ERR_BAD_ARG, "kge_import_eval_arrays: train + valid + test must stay below 2^31 triples");
    std::vector<Int4> all, test, valid;
    if (eval_build_on_device(n_all)) {
        test.resize((size_t)n_test); valid.resize((size_t)n_valid);   // file order (h,t,r,0), the build's only uploads
        for (INT i = 0; i < n_test; i++) test[(size_t)i] = Int4{(int32_t)test_h[i], (int32_t)test_t[i], (int32_t)test_r[i], 0};
        for (INT i = 0; i < n_valid; i++) valid[(size_t)i] = Int4{(int32_t)valid_h[i], (int32_t)valid_t[i], (int32_t)valid_r[i], 0};
        ScopedDevBuf<int4> train_up;   // the training triples: the device index's `pos` where it is resident
        const int4 *d_train = e.dev.pos;
        if (!e.dev.uploaded) {
            if ((rc = train_up.upload(e.index.pos, "eval build: training triples"))) return rc;
            d_train = train_up;
        }
        EvalTriplesBuilt b;
        if ((rc = build_eval_lists_device(E, R, d_train, n_train, valid, test, b))) return rc;
        // host copies for the legacy host routines (getHeadBatch, getValidBatch, find_host, eval_tc_lists), by download
        if ((rc = download_int4(all, b.all, n_all, "download triples"))) return rc;
        if ((rc = download_int4(test, b.test, n_test, "download test list"))) return rc;
        if ((rc = download_int4(valid, b.valid, n_valid, "download valid list"))) return rc;
        reset_eval_state();
        g_ed.all.adopt(b.all.release(), n_all); g_ed.all_t.adopt(b.all_t.release(), n_all); g_ed.all_ht.adopt(b.all_ht.release(), n_all);
        g_ed.test.adopt(b.test.release(), n_test > 0 ? n_test : 1); g_ed.valid.adopt(b.valid.release(), n_valid > 0 ? n_valid : 1);
        g_eh.dev_triples = true;
    } else {
        build_eval_lists(e.index.pos, n_valid, (const int64_t *)valid_h, (const int64_t *)valid_t, (const int64_t *)valid_r, n_test,
                         (const int64_t *)test_h, (const int64_t *)test_t, (const int64_t *)test_r, all, test, valid);
        reset_eval_state();
    }
    g_eh.all = std::move(all); g_eh.test = std::move(test); g_valid = std::move(valid);
    g_eh.test_total = n_test; g_eh.valid_total = n_valid; g_eh.triple_total = n_all;
    g_eh.loaded = true;
    return KGE_OK;
}

int kge_set_type_lists(const INT *head_off, const INT *head_ids, const INT *tail_off, const INT *tail_ids) {
    Engine &e = engine();
    if (!e.index.loaded) return fail(KGE_ERR_NO_DATASET, "kge_set_type_lists: no training set imported");
    const int64_t E = e.index.ent_total, R = e.index.rel_total;
    if (!head_off || !tail_off) return fail(KGE_ERR_BAD_ARG, "kge_set_type_lists: null offsets");
    const INT *offs[2] = {head_off, tail_off}, *ids[2] = {head_ids, tail_ids};
    const char *side[2] = {"head", "tail"};
    for (int s = 0; s < 2; s++) {
        if (offs[s][0] != 0) return fail(KGE_ERR_BAD_ARG, std::string("kge_set_type_lists: ") + side[s] + " offsets must start at 0");
        for (int64_t r = 0; r < R; r++)
            if (offs[s][r + 1] < offs[s][r])
                return fail(KGE_ERR_BAD_ARG, std::string("kge_set_type_lists: ") + side[s] + " offsets decrease at relation " + std::to_string((long long)r));
        const INT n = offs[s][R];
        if (n >= (INT(1) << 31) || (n > 0 && !ids[s])) return fail(KGE_ERR_BAD_ARG, std::string("kge_set_type_lists: ") + side[s] + " ids: null or too many");
        for (INT i = 0; i < n; i++)
            if (ids[s][i] < 0 || ids[s][i] >= E)
                return fail(KGE_ERR_BAD_ARG, std::string("kge_set_type_lists: ") + side[s] + " id out of range at index " + std::to_string((long long)i));
    }
    std::vector<int32_t> *lef[2] = {&g_eh.head_lef, &g_eh.tail_lef}, *rig[2] = {&g_eh.head_rig, &g_eh.tail_rig}, *typ[2] = {&g_eh.head_type, &g_eh.tail_type};
    for (int s = 0; s < 2; s++) {
        lef[s]->resize((size_t)R); rig[s]->resize((size_t)R);
        typ[s]->resize((size_t)offs[s][R]);
        for (INT i = 0; i < offs[s][R]; i++) (*typ[s])[(size_t)i] = (int32_t)ids[s][i];
        for (int64_t r = 0; r < R; r++) {   // each list sorted, duplicates kept, as importTypeFiles leaves them
            (*lef[s])[(size_t)r] = (int32_t)offs[s][r]; (*rig[s])[(size_t)r] = (int32_t)offs[s][r + 1];
            std::sort(typ[s]->begin() + offs[s][r], typ[s]->begin() + offs[s][r + 1]);
        }
    }
    g_eh.types = true;
    g_eh.dev_types = false;
    g_ed.uploaded = false;
    e.index.typed_built = false;
    return KGE_OK;
}

int kge_derive_type_lists(void) {
    Engine &e = engine();
    if (!g_eh.loaded) return fail(KGE_ERR_NO_DATASET, "kge_derive_type_lists: no evaluation import (importTestFiles / kge_import_eval_arrays)");
    const int64_t E = e.index.ent_total, R = e.index.rel_total, n_all = (int64_t)g_eh.all.size();
    if (eval_build_on_device(n_all)) {
        int rc = ensure_eval_device();   // `all` on the device: built there, or uploaded by the file path
        if (rc) return rc;
        TypeListsBuilt b;
        if ((rc = derive_type_lists_device(E, R, g_ed.all, n_all, b))) return rc;
        std::vector<int32_t> hl, hr, ht, tl, tr, tt;   // host copies for the typed sampling index and the host classification routines
        if ((rc = download_i32(hl, b.head_lef, R, "download type lists")) || (rc = download_i32(hr, b.head_rig, R, "download type lists")) ||
            (rc = download_i32(ht, b.head_type, b.n_head, "download type lists")) || (rc = download_i32(tl, b.tail_lef, R, "download type lists")) ||
            (rc = download_i32(tr, b.tail_rig, R, "download type lists")) || (rc = download_i32(tt, b.tail_type, b.n_tail, "download type lists")))
            return rc;
        g_eh.head_lef.swap(hl); g_eh.head_rig.swap(hr); g_eh.head_type.swap(ht);
        g_eh.tail_lef.swap(tl); g_eh.tail_rig.swap(tr); g_eh.tail_type.swap(tt);
        g_ed.head_lef.adopt(b.head_lef.release(), R); g_ed.head_rig.adopt(b.head_rig.release(), R);
        g_ed.tail_lef.adopt(b.tail_lef.release(), R); g_ed.tail_rig.adopt(b.tail_rig.release(), R);
        g_ed.head_type.adopt(b.head_type.release(), b.n_head); g_ed.tail_type.adopt(b.tail_type.release(), b.n_tail);
        g_eh.dev_types = true;   // g_ed.uploaded stays: the views hand out the adopted arrays
    } else {
        derive_type_lists(g_eh.all, R, g_eh.head_lef, g_eh.head_rig, g_eh.head_type, g_eh.tail_lef, g_eh.tail_rig, g_eh.tail_type);
        g_eh.dev_types = false;
        g_ed.uploaded = false;
    }
    g_eh.types = true;
    e.index.typed_built = false;
    return KGE_OK;
}

int kge_have_type_lists(void) { return g_eh.types ? 1 : 0; }

int kge_get_type_lists(INT *head_off, INT *head_ids, INT *tail_off, INT *tail_ids) {
    if (!g_eh.types) return fail(KGE_ERR_NO_DATASET, "kge_get_type_lists: no type lists (importTypeFiles / kge_set_type_lists / kge_derive_type_lists)");
    const int64_t R = engine().index.rel_total;
    auto side = [&](const std::vector<int32_t> &lef, const std::vector<int32_t> &rig, const std::vector<int32_t> &typ, INT *off, INT *ids) {
        INT k = 0;
        for (int64_t r = 0; r < R; r++) {
            if (off) off[r] = k;
            const int32_t lo = r < (int64_t)lef.size() ? lef[(size_t)r] : 0, hi = r < (int64_t)rig.size() ? rig[(size_t)r] : 0;
            if (ids) for (int32_t q = lo; q < hi; q++) ids[k + (q - lo)] = typ[(size_t)q];
            k += hi - lo;
        }
        if (off) off[R] = k;
    };
    side(g_eh.head_lef, g_eh.head_rig, g_eh.head_type, head_off, head_ids);
    side(g_eh.tail_lef, g_eh.tail_rig, g_eh.tail_type, tail_off, tail_ids);
    return KGE_OK;
}

int kge_write_type_constraints(const char *path) {
    if (!g_eh.types) return fail(KGE_ERR_NO_DATASET, "kge_write_type_constraints: no type lists (importTypeFiles / kge_set_type_lists / kge_derive_type_lists)");
    if (!path) return fail(KGE_ERR_BAD_ARG, "kge_write_type_constraints: null path");
    const std::string tmp = std::string(path) + ".tmp";   // renamed into place: a reader never sees half a file
    FILE *f = std::fopen(tmp.c_str(), "w");
    if (!f) return fail(KGE_ERR_BAD_ARG, "kge_write_type_constraints: cannot write `" + tmp + "`");
    const int64_t R = engine().index.rel_total;
    std::fprintf(f, "%lld\n", (long long)R);
    auto line = [&](int64_t r, const std::vector<int32_t> &lef, const std::vector<int32_t> &rig, const std::vector<int32_t> &typ) {
        const int32_t lo = lef[(size_t)r], hi = rig[(size_t)r];
        std::fprintf(f, "%lld\t%d", (long long)r, (int)(hi - lo));
        for (int32_t q = lo; q < hi; q++) std::fprintf(f, "\t%d", (int)typ[(size_t)q]);
        std::fputc('\n', f);
    };
    for (int64_t r = 0; r < R; r++) {
        line(r, g_eh.head_lef, g_eh.head_rig, g_eh.head_type);
        line(r, g_eh.tail_lef, g_eh.tail_rig, g_eh.tail_type);
    }
    const bool bad = std::ferror(f) != 0;
    if (std::fclose(f) != 0 || bad || std::rename(tmp.c_str(), path) != 0) return fail(KGE_ERR_BAD_ARG, std::string("kge_write_type_constraints: writing `") + path + "` failed");
    return KGE_OK;
}

int64_t kge_eval_copy(const char *what, void *dst, int64_t bytes) {
    if (!g_eh.loaded) return fail(KGE_ERR_NO_DATASET, "kge_eval_copy: no evaluation import (importTestFiles / kge_import_eval_arrays)");
    const std::string w = what ? what : "";
    const int64_t R = engine().index.rel_total, n_all = (int64_t)g_eh.all.size();
    const bool on_device = device_ok();
    if (on_device) { int rc = ensure_eval_device(); if (rc) return rc; }
    if (w == "valid" && !ensure_classification_lists()) return KGE_ERR_NO_DATASET;   // (the file path reads valid2id.txt on first use)
    if (g_eh.head_lef.empty()) { g_eh.head_lef.assign((size_t)R, 0); g_eh.head_rig.assign((size_t)R, 0); g_eh.tail_lef.assign((size_t)R, 0); g_eh.tail_rig.assign((size_t)R, 0); }
    std::vector<Int4> order;   // all_t / all_ht without a device: the host sort of ensure_eval_device
    const void *host = nullptr, *dev = nullptr;
    int64_t have = -1;
#define KGE_EVAL_ARR(name, hvec, dbuf, count, elem) if (w == name) { host = (hvec); dev = (dbuf); have = (int64_t)(count) * (int64_t)(elem); }
    KGE_EVAL_ARR("all", g_eh.all.data(), g_ed.all.ptr(), n_all, 16)
    KGE_EVAL_ARR("all_t", nullptr, g_ed.all_t.ptr(), n_all, 16)
    KGE_EVAL_ARR("all_ht", nullptr, g_ed.all_ht.ptr(), n_all, 16)
    KGE_EVAL_ARR("test", g_eh.test.data(), g_ed.test.ptr(), g_eh.test_total, 16)
    KGE_EVAL_ARR("valid", g_valid.data(), g_eh.dev_triples ? g_ed.valid.ptr() : nullptr, g_eh.valid_total, 16)
    KGE_EVAL_ARR("head_lef", g_eh.head_lef.data(), g_ed.head_lef.ptr(), R, 4)
    KGE_EVAL_ARR("head_rig", g_eh.head_rig.data(), g_ed.head_rig.ptr(), R, 4)
    KGE_EVAL_ARR("tail_lef", g_eh.tail_lef.data(), g_ed.tail_lef.ptr(), R, 4)
    KGE_EVAL_ARR("tail_rig", g_eh.tail_rig.data(), g_ed.tail_rig.ptr(), R, 4)
    KGE_EVAL_ARR("head_type", g_eh.head_type.data(), g_ed.head_type.ptr(), g_eh.head_type.size(), 4)
    KGE_EVAL_ARR("tail_type", g_eh.tail_type.data(), g_ed.tail_type.ptr(), g_eh.tail_type.size(), 4)
#undef KGE_EVAL_ARR
    if (have < 0) return fail(KGE_ERR_BAD_ARG, "kge_eval_copy: unknown array " + w);
    if (!dst || bytes <= 0 || have == 0) return have;
    const size_t n = (size_t)(bytes < have ? bytes : have);
    if (on_device && dev) {
        int rc = hip_check(hipMemcpy(dst, dev, n, hipMemcpyDeviceToHost), "kge_eval_copy");
        return rc ? rc : have;
    }
    if (!host) {
        const bool by_tail = w == "all_t";
        order.resize(g_eh.all.size());
        for (size_t i = 0; i < order.size(); i++) {
            const Int4 &a = g_eh.all[i];
            order[i] = by_tail ? Int4{a.z, a.y, a.x, 0} : Int4{a.x, a.z, a.y, 0};
        }
        std::sort(order.begin(), order.end(), [](const Int4 &a, const Int4 &b) {
            if (a.x != b.x) return a.x < b.x; if (a.y != b.y) return a.y < b.y; return a.z < b.z; });
        host = order.data();
    }
    std::memcpy(dst, host, n);
    return have;
}

INT kge_eval_test_total(void) { return g_eh.test_total; }
INT kge_eval_valid_total(void) { return g_eh.valid_total; }
INT kge_eval_triple_total(void) { return g_eh.triple_total; }

void getHeadBatch(INT index, INT *ph, INT *pt, INT *pr) {   // Test.h:11-17
    if (!g_eh.loaded || index < 0 || index >= g_eh.test_total) { set_error("getHeadBatch: bad index / importTestFiles missing"); return; }
    const Int4 &tt = g_eh.test[(size_t)index];
    for (INT i = 0; i < engine().index.ent_total; i++) { ph[i] = i; pt[i] = tt.y; pr[i] = tt.z; }
}

void getTailBatch(INT index, INT *ph, INT *pt, INT *pr) {   // Test.h:20-26
    if (!g_eh.loaded || index < 0 || index >= g_eh.test_total) { set_error("getTailBatch: bad index / importTestFiles missing"); return; }
    const Int4 &tt = g_eh.test[(size_t)index];
    for (INT i = 0; i < engine().index.ent_total; i++) { ph[i] = tt.x; pt[i] = i; pr[i] = tt.z; }
}

static INT *rank_one_host_scores(INT index, REAL *con, int head) {
    // the reference returns `new INT[8]` that its callers never free (Test.h:37, Config.py:36-39);
    // here a small ring of result slots is reused instead
    static long long ring[64][8];
    static int slot = 0;
    long long *out = ring[slot];
    slot = (slot + 1) % 64;
    std::memset(out, 0, sizeof(long long) * 8);
    if (ensure_eval_device()) return (INT *)out;
    if (index < 0 || index >= g_eh.test_total) { set_error("testHead/testTail: index out of range"); return (INT *)out; }
    const int64_t E = engine().index.ent_total;
    if (g_ed.scores.reserve(E, "alloc scores")) return (INT *)out;
    if (g_ed.req_one.reserve(2, "alloc req")) return (INT *)out;
    int32_t *d_req = g_ed.req_one;
    int32_t req[2] = {(int32_t)index, head};
    if (hip_check(hipMemcpy(g_ed.scores, con, sizeof(float) * (size_t)E, hipMemcpyHostToDevice), "upload scores")) return (INT *)out;
    if (hip_check(hipMemcpy(d_req, req, sizeof(req), hipMemcpyHostToDevice), "upload req")) return (INT *)out;
    std::vector<int32_t> idx{(int32_t)index}, hd{head};
    rank_requests(g_ed.scores, idx, hd, out, nullptr, d_req, d_req + 1);
    return (INT *)out;
}

INT *testHead(INT index, REAL *con) { return rank_one_host_scores(index, con, 1); }   // Test.h:31-136
INT *testTail(INT index, REAL *con) { return rank_one_host_scores(index, con, 0); }   // Test.h:141-249

/* ------------------------------------------------------------------------------------------------
 * Triple classification (Test.h:262-444).  These are the reference's HOST
 * routines over validTotal / testTotal-long score arrays (run once per early-stop check, not a hot
 * path): negatives drawn with libc rand() from the relation's tail type list until unknown
 * (Corrupt.h:118-137), a per-relation threshold grid search with step `interval` = 0.01f
 * (Setting.h:118), accuracy / TP-FP counts.  Restated in float exactly as written there.
 * ---------------------------------------------------------------------------------------------- */
static const float kInterval = 0.01f;   // Setting.h:118
// min_score + i * interval (Test.h:326).  The reference is built with -O3 -march=native (make.sh:1), where
// GCC contracts this expression into ONE fused multiply-add; a separate multiply and add rounds twice and
// lands on different thresholds.  The fused form is what an FMA-capable host produces, so it is pinned here.
static inline float grid_point(float mn, INT i) { return fmaf((float)i, kInterval, mn); }

static bool find_host(int h, int t, int r) {   // Corrupt.h:104-115 on the host copy
    const std::vector<Int4> &all = g_eh.all;
    long long lef = 0, rig = (long long)all.size() - 1;
    while (lef + 1 < rig) {
        const long long mid = (lef + rig) >> 1;
        const Int4 &m = all[(size_t)mid];
        if (m.x < h || (m.x == h && m.y < r) || (m.x == h && m.y == r && m.z < t)) lef = mid; else rig = mid;
    }
    const Int4 &a = all[(size_t)lef], &b = all[(size_t)rig];
    return (a.x == h && a.y == r && a.z == t) || (b.x == h && b.y == r && b.z == t);
}

// corrupt_head(0, h, r) on the host index (Corrupt.h:7-37), consuming rng stream 0; used only after 1000
// failed type-constrained draws (Corrupt.h:131-133)
static int corrupt_head_stream0(int h, int r) {
    Engine &e = engine();
    if (e.dev.streams_sync == 2 && e.dev.streams)
        (void)hipMemcpy(e.streams.data(), e.dev.streams, sizeof(uint64_t) * e.streams.size(), hipMemcpyDeviceToHost);
    if (e.streams.empty()) e.streams.assign(1, 0);
    e.streams[0] = e.streams[0] * kLcgMul + kLcgAdd;
    e.dev.streams_sync = 0;
    // known tails of (h, r): any file-order triple of the group carries its [offset, length]
    const KgIndex &ix = e.index;
    int off = 0, len = 0;
    for (size_t i = 0; i < ix.pos.size(); i++)
        if (ix.pos[i].x == h && ix.pos[i].z == r) { off = ix.grp[i].x; len = ix.grp[i].y; break; }
    const long long tmp = (long long)(e.streams[0] % (uint64_t)(ix.ent_total - len));
    int lo = 0, hi = len;
    while (lo < hi) { const int mid = (lo + hi) >> 1; if ((long long)ix.tails_hr[(size_t)off + mid] - mid <= tmp) lo = mid + 1; else hi = mid; }
    return (int)(tmp + lo);
}

static int corrupt_typed(int h, int r) {   // Corrupt.h:118-137
    Engine &e = engine();
    const int ll = g_eh.tail_lef.empty() ? 0 : g_eh.tail_lef[(size_t)r], rr = g_eh.tail_rig.empty() ? 0 : g_eh.tail_rig[(size_t)r];
    if (rr <= ll) { set_error("getValidBatch/getTestBatch: relation without tail type list (importTypeFiles)"); return 0; }
    for (int loop = 0;;) {
        const int t = g_eh.tail_type[(size_t)(ll + e.libc.next() % (rr - ll))];   // Random.h:38-40 rand(a,b)
        if (!find_host(h, t, r)) return t;
        if (++loop >= 1000) return corrupt_head_stream0(h, r);
    }
}


static void build_rel_ranges(const std::vector<Int4> &list, std::vector<int32_t> &lef, std::vector<int32_t> &rig) {
    const int64_t R = engine().index.rel_total;
    lef.assign((size_t)R, -1); rig.assign((size_t)R, -1);
    for (size_t i = 0; i < list.size(); i++) {
        const int r = list[i].z;
        if (lef[(size_t)r] < 0) lef[(size_t)r] = (int32_t)i;
        rig[(size_t)r] = (int32_t)i;
    }
}

static bool ensure_classification_lists() {
    if (!g_eh.loaded) { set_error("triple classification: importTestFiles has not been called"); return false; }
    if (g_valid.size() != (size_t)g_eh.valid_total) {
        // the valid triples are part of `all`; re-read them in file order is not needed: only the sorted list is used
        std::vector<int64_t> va;
        if (!read_all_longs(engine().in_path + "valid2id.txt", va)) { set_error("valid2id.txt does not exist"); return false; }
        g_valid.clear();
        for (int64_t i = 0; i < g_eh.valid_total; i++)
            g_valid.push_back(Int4{(int32_t)va[1 + 3 * i], (int32_t)va[2 + 3 * i], (int32_t)va[3 + 3 * i], 0});
        std::sort(g_valid.begin(), g_valid.end(), [](const Int4 &a, const Int4 &b) {
            if (a.z != b.z) return a.z < b.z; if (a.x != b.x) return a.x < b.x; return a.y < b.y; });
    }
    build_rel_ranges(g_valid, g_valid_lef, g_valid_rig);
    build_rel_ranges(g_eh.test, g_test_lef, g_test_rig);
    return true;
}

static void fill_batch(const std::vector<Int4> &list, INT *ph, INT *pt, INT *pr, INT *nh, INT *nt, INT *nr) {
    for (size_t i = 0; i < list.size(); i++) {   // Test.h:252-300: negative = positive with a new tail
        ph[i] = list[i].x; pt[i] = list[i].y; pr[i] = list[i].z;
        nh[i] = list[i].x; nr[i] = list[i].z;
        nt[i] = corrupt_typed(list[i].x, list[i].z);
    }
}

void getTestBatch(INT *ph, INT *pt, INT *pr, INT *nh, INT *nt, INT *nr) {
    if (!ensure_classification_lists()) return;
    fill_batch(g_eh.test, ph, pt, pr, nh, nt, nr);
}

void getValidBatch(INT *ph, INT *pt, INT *pr, INT *nh, INT *nt, INT *nr) {
    if (!ensure_classification_lists()) return;
    fill_batch(g_valid, ph, pt, pr, nh, nt, nr);
}

// min / max of the relation's validation scores and the grid size (Test.h:310-322, :394-410)
static bool score_range(INT r, const REAL *sp, const REAL *sn, float &mn, float &mx, INT &n_interval) {
    if (r < 0 || r >= (INT)g_valid_lef.size() || g_valid_lef[(size_t)r] == -1) return false;
    const int lo = g_valid_lef[(size_t)r], hi = g_valid_rig[(size_t)r];
    mn = sp[lo]; if (sn[lo] < mn) mn = sn[lo];
    mx = sp[lo]; if (sn[lo] > mx) mx = sn[lo];
    for (int i = lo + 1; i <= hi; i++) {
        if (sp[i] < mn) mn = sp[i];
        if (sp[i] > mx) mx = sp[i];
        if (sn[i] < mn) mn = sn[i];
        if (sn[i] > mx) mx = sn[i];
    }
    n_interval = (INT)((mx - mn) / kInterval);
    return true;
}

void getBestThreshold(REAL *relThresh, REAL *score_pos, REAL *score_neg) {   // Test.h:304-341
    if (!ensure_classification_lists()) return;
    for (INT r = 0; r < engine().index.rel_total; r++) {
        float mn, mx; INT n_interval;
        if (!score_range(r, score_pos, score_neg, mn, mx, n_interval)) continue;
        const int lo = g_valid_lef[(size_t)r], hi = g_valid_rig[(size_t)r];
        const INT total = (INT)(hi - lo + 1) * 2;
        float bestThresh = 0.f, bestAcc = 0.f;
        for (INT i = 0; i <= n_interval; i++) {
            const float tmpThresh = grid_point(mn, i);
            INT correct = 0;
            for (int j = lo; j <= hi; j++) {
                if (score_pos[j] <= tmpThresh) correct++;
                if (score_neg[j] > tmpThresh) correct++;
            }
            const float tmpAcc = (float)(1.0 * correct / total);
            if (i == 0 || tmpAcc > bestAcc) { bestAcc = tmpAcc; bestThresh = tmpThresh; }
        }
        relThresh[r] = bestThresh;
    }
}

void test_triple_classification(REAL *relThresh, REAL *score_pos, REAL *score_neg, REAL *acc_addr) {   // Test.h:347-387
    if (!ensure_classification_lists()) return;
    INT TP = 0, TN = 0, FP = 0, FN = 0;
    for (INT r = 0; r < engine().index.rel_total; r++) {
        if (g_valid_lef[(size_t)r] == -1 || g_test_lef[(size_t)r] == -1) continue;
        for (int i = g_test_lef[(size_t)r]; i <= g_test_rig[(size_t)r]; i++) {
            if (score_pos[i] <= relThresh[r]) TP++; else FN++;
            if (score_neg[i] > relThresh[r]) TN++; else FP++;
        }
    }
    const double accuracy = 1.0 * (TP + TN) / (TP + TN + FP + FN);
    const double precision = 1.0 * TP / (TP + FP);
    const double recall = 1.0 * TP / (TP + FN);
    const double fmeasure = (2 * precision * recall) / (precision + recall);
    std::printf("triple classification accuracy is %lf\n", accuracy);
    std::printf("triple classification precision is %lf\n", precision);
    std::printf("triple classification recall is %lf\n", recall);
    std::printf("triple classification f-measure is %lf\n", fmeasure);
    if (acc_addr) acc_addr[0] = (float)(1.0 * (TP + TN) / (TP + TN + FP + FN));
}

INT get_n_interval(INT r, REAL *score_pos, REAL *score_neg) {   // Test.h:390-407
    if (!ensure_classification_lists()) return 0;
    float mn, mx; INT n;
    return score_range(r, score_pos, score_neg, mn, mx, n) ? n : 0;
}

INT *get_TPFP(INT r, REAL *score_pos, REAL *score_neg, REAL *score_pos_test, REAL *score_neg_test) {   // Test.h:410-444
    static std::vector<INT> buf;   // the reference leaks a new INT[] per call
    if (!ensure_classification_lists()) return nullptr;
    float mn, mx; INT n_interval;
    if (!score_range(r, score_pos, score_neg, mn, mx, n_interval)) return nullptr;
    buf.assign((size_t)(n_interval + 1) * 2, 0);
    for (INT i = 0; i <= n_interval; i++) {
        const float tmpThresh = grid_point(mn, i);
        INT TP = 0, FP = 0;
        if (g_test_lef[(size_t)r] != -1)
            for (int j = g_test_lef[(size_t)r]; j <= g_test_rig[(size_t)r]; j++) {
                if (score_pos_test[j] <= tmpThresh) TP++;
                if (score_neg_test[j] <= tmpThresh) FP++;
            }
        buf[(size_t)i] = TP;
        buf[(size_t)(i + n_interval + 1)] = FP;
    }
    return buf.data();
}

/* Device-native evaluation of test triples [first, first+count): for each, the model's predict op over
 * ALL entities as tail (and, if test_head != 0, as head) candidates, then the ranker.  out receives
 * count x 2 x 8 int64: [i][0] = testTail result, [i][1] = testHead result (zeros when test_head == 0),
 * each as the reference's 8-vector (distribute_training.py:465-590 consumes exactly these). */
static int link_prediction_v1(const kge_model_desc *m, const float *const tables[KGE_MAX_TABLES], INT first, INT count,
                              INT test_head, int64_t *out, void *stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    int rc = ensure_eval_device();
    if (rc) return rc;
    if (!m || !tables || !out || first < 0 || count < 0 || first + count > g_eh.test_total) return fail(KGE_ERR_BAD_ARG, "kge_link_prediction: bad range");
    const int64_t E = m->ent_total;
    const int sides = test_head ? 2 : 1;
    const int max_req = m->model == KGE_TRANSR ? 1 : 32;   // TransR's predict uses ONE matrix per call (TransR.py:83)
    if ((rc = g_ed.scores.reserve(max_req * E, "alloc scores"))) return rc;
    if ((rc = g_ed.cand.reserve(3 * max_req * E, "alloc candidates"))) return rc;
    if ((rc = g_ed.req_v1.reserve(2 * 64, "alloc req"))) return rc;
    int32_t *d_req = g_ed.req_v1;
    std::memset(out, 0, sizeof(int64_t) * 16 * (size_t)count);
    std::vector<int32_t> idx, hd;
    std::vector<long long> res;
    for (INT base = 0; base < count * sides; base += max_req) {
        idx.clear(); hd.clear();
        for (INT q = base; q < base + max_req && q < count * sides; q++) { idx.push_back((int32_t)(first + q / sides)); hd.push_back((int32_t)(q % sides)); }
        const int n = (int)idx.size();
        if ((rc = hip_check(hipMemcpyAsync(d_req, idx.data(), sizeof(int32_t) * n, hipMemcpyHostToDevice, stream), "upload req"))) return rc;
        if ((rc = hip_check(hipMemcpyAsync(d_req + 64, hd.data(), sizeof(int32_t) * n, hipMemcpyHostToDevice, stream), "upload req"))) return rc;
        int32_t *ch = g_ed.cand, *ct = g_ed.cand + (size_t)max_req * E, *cr = g_ed.cand + 2 * (size_t)max_req * E;
        long long tot = (long long)n * E;
        int blocks = (int)std::min<long long>((tot + 255) / 256, 4096);
        hipLaunchKernelGGL(candidates_kernel, dim3(blocks), dim3(256), 0, stream, g_ed.test, d_req, d_req + 64, n, (int)E, ch, ct, cr);
        if ((rc = launch_predict(*m, tables, ch, ct, cr, tot, g_ed.scores, stream))) return rc;
        res.assign((size_t)n * 8, 0);
        if ((rc = rank_requests(g_ed.scores, idx, hd, res.data(), stream, d_req, d_req + 64))) return rc;
        for (int q = 0; q < n; q++) {
            const INT i = idx[q] - first;
            std::memcpy(out + (i * 2 + hd[q]) * 8, res.data() + (size_t)q * 8, sizeof(int64_t) * 8);
        }
    }
    return KGE_OK;
}


// Relation-grouped ranker (models.hip lp_table_kernel / lp_score_kernel): importTestFiles keeps the test triples sorted
// by (r, h, t) (Triple.h:30-32), so the requests of a range are already grouped by relation.  Per relation: one table
// of all candidates' projected + normalised vectors, one scoring pass per chunk of requests, the rank kernel; the 8-vectors
// of all requests come back in ONE copy at the end.
int kge_link_prediction(const kge_model_desc *m, const float *const tables[KGE_MAX_TABLES], INT first, INT count,
                        INT test_head, int64_t *out, void *stream_) {
    if (engine().lp_v1) return link_prediction_v1(m, tables, first, count, test_head, out, stream_);
    hipStream_t stream = (hipStream_t)stream_;
    int rc = ensure_eval_device();
    if (rc) return rc;
    if (!m || !tables || !out || first < 0 || count < 0 || first + count > g_eh.test_total) return fail(KGE_ERR_BAD_ARG, "kge_link_prediction: bad range");
    std::memset(out, 0, sizeof(int64_t) * 16 * (size_t)count);
    if (count == 0) return KGE_OK;
    const int64_t E = m->ent_total;
    const int sides = test_head ? 2 : 1;
    const int64_t n_req = count * sides;
    const int D = m->model == KGE_TRANSR ? m->rel_dim : m->ent_dim;
    // requests in the order (test triple, tail then head)
    std::vector<int32_t> idx((size_t)n_req), hd((size_t)n_req), fixed((size_t)n_req), rel((size_t)n_req);
    for (int64_t q = 0; q < n_req; q++) {
        const int64_t i = first + q / sides;
        const Int4 &tt = g_eh.test[(size_t)i];   // (h, t, r)
        idx[(size_t)q] = (int32_t)i;
        hd[(size_t)q] = (int32_t)(q % sides);
        fixed[(size_t)q] = hd[(size_t)q] ? tt.y : tt.x;   // head request: the tail stays; tail request: the head stays
        rel[(size_t)q] = tt.z;
    }
    if ((rc = g_ed.req.reserve(3 * n_req, "alloc lp requests"))) return rc;
    if ((rc = g_ed.T.reserve(E * D, "alloc lp table"))) return rc;
    if (m->model == KGE_TRANSR && (rc = g_ed.P.reserve((E + 1) * D, "alloc lp projections"))) return rc;
    float *d_T = g_ed.T, *d_P = g_ed.P;
    // scores for a chunk of requests: at most 1 GiB
    int64_t qmax = (int64_t(1) << 28) / (E > 0 ? E : 1);
    if (qmax < 1) qmax = 1;
    if (qmax > 4096) qmax = 4096;
    if (qmax > n_req) qmax = n_req;
    if ((rc = g_ed.scores.reserve(qmax * E, "alloc scores"))) return rc;
    if ((rc = g_ed.out.reserve(8 * n_req, "alloc rank out"))) return rc;
    int32_t *d_idx = g_ed.req, *d_hd = d_idx + n_req, *d_fixed = d_idx + 2 * n_req;
    if ((rc = hip_check(hipMemcpyAsync(d_idx, idx.data(), sizeof(int32_t) * (size_t)n_req, hipMemcpyHostToDevice, stream), "upload req"))) return rc;
    if ((rc = hip_check(hipMemcpyAsync(d_hd, hd.data(), sizeof(int32_t) * (size_t)n_req, hipMemcpyHostToDevice, stream), "upload req"))) return rc;
    if ((rc = hip_check(hipMemcpyAsync(d_fixed, fixed.data(), sizeof(int32_t) * (size_t)n_req, hipMemcpyHostToDevice, stream), "upload req"))) return rc;
    RankArgs a;
    a.test = g_ed.test; a.all = g_ed.all; a.all_t = g_ed.all_t; a.n_all = (long long)g_eh.all.size();
    a.head_lef = g_ed.head_lef; a.head_rig = g_ed.head_rig; a.tail_lef = g_ed.tail_lef; a.tail_rig = g_ed.tail_rig;
    a.head_type = g_ed.head_type; a.tail_type = g_ed.tail_type;
    a.sup_lef = g_ed.sup_lef; a.sup_rig = g_ed.sup_rig; a.sub_lef = g_ed.sub_lef; a.sub_rig = g_ed.sub_rig;
    a.sup_type = g_ed.sup_type; a.sub_type = g_ed.sub_type; a.E = (int)E;
    bool have_table = false;
    for (int64_t q0 = 0; q0 < n_req;) {
        const int32_t r = rel[(size_t)q0];
        int64_t q1 = q0;
        while (q1 < n_req && rel[(size_t)q1] == r) q1++;
        if (m->model != KGE_TRANSE || !have_table) {   // TransE's candidates do not depend on the relation
            if (m->model == KGE_TRANSR && (rc = transr_project_all(*m, tables, r, d_P, stream))) return rc;
            if ((rc = launch_lp_table(*m, tables, d_P, r, d_T, stream))) return rc;
            have_table = true;
        }
        for (int64_t c0 = q0; c0 < q1; c0 += qmax) {
            const int64_t n = std::min<int64_t>(qmax, q1 - c0);
            if ((rc = launch_lp_scores(*m, tables, d_T, r, d_fixed + c0, d_hd + c0, n, g_ed.scores, stream))) return rc;
            a.scores = g_ed.scores; a.req_index = d_idx + c0; a.req_head = d_hd + c0; a.out = g_ed.out + c0 * 8;
            hipLaunchKernelGGL(rank_kernel, dim3((unsigned)n), dim3(256), 0, stream, a);
        }
        q0 = q1;
    }
    std::vector<long long> res((size_t)n_req * 8);
    if ((rc = hip_check(hipMemcpyAsync(res.data(), g_ed.out, sizeof(long long) * 8 * (size_t)n_req, hipMemcpyDeviceToHost, stream), "copy ranks"))) return rc;
    if ((rc = hip_check(hipStreamSynchronize(stream), "rank sync"))) return rc;
    for (int64_t q = 0; q < n_req; q++) {
        const int64_t i = q / sides;
        std::memcpy(out + (i * 2 + hd[(size_t)q]) * 8, res.data() + (size_t)q * 8, sizeof(int64_t) * 8);
    }
    return KGE_OK;
}

}  // extern "C"

namespace kge {

uint64_t eval_tc_generation() { return g_tc_generation; }

int eval_tc_lists(TcLists &v) {
    if (!ensure_classification_lists()) return KGE_ERR_NO_DATASET;
    v.lef[0] = &g_valid_lef; v.rig[0] = &g_valid_rig; v.lef[1] = &g_test_lef; v.rig[1] = &g_test_rig;
    v.total[0] = g_eh.valid_total; v.total[1] = g_eh.test_total;
    return KGE_OK;
}

}  // namespace kge
