// extern "C" surface of libkge_mi355.so (declared in include/kge_mi355.h) and the process-global
// engine state behind it.
#include <cstdio>
#include <cstring>
#include <iostream>

#include "engine.hpp"

namespace kge {

Engine &engine() {
    static Engine e;
    return e;
}

void set_error(const std::string &msg) {
    engine().last_error = msg;
    std::fprintf(stderr, "[kge_mi355] error: %s\n", msg.c_str());
}

int fail(int code, const std::string &msg) {
    set_error(msg);
    return code;
}

int hip_check(hipError_t e, const char *what) {
    if (e == hipSuccess) return KGE_OK;
    return fail(KGE_ERR_NO_DEVICE, std::string(what) + ": " + hipGetErrorString(e));
}

bool device_ok() {
    Engine &e = engine();
    if (e.device_state == 0) {
        int n = 0;
        hipError_t rc = hipGetDeviceCount(&n);
        e.device_state = (rc == hipSuccess && n > 0) ? 1 : -1;
        if (e.device_state < 0) (void)hipGetLastError();
    }
    return e.device_state > 0;
}

int ensure_device_index() {
    Engine &e = engine();
    if (!e.index.loaded) return fail(KGE_ERR_NO_DATASET, "no training set imported (importTrainFiles / kge_import_train_arrays)");
    if (!device_ok()) return fail(KGE_ERR_NO_DEVICE, "no usable HIP device: the sampler has no CPU fallback");
    int rc = KGE_OK;
    if (!e.dev.uploaded) {
        const KgIndex &ix = e.index;
        if ((rc = e.dev.pos.upload(ix.pos, "upload pos"))) return rc;
        if ((rc = e.dev.grp.upload(ix.grp, "upload grp"))) return rc;
        if ((rc = e.dev.ht.upload(ix.ht, "upload ht"))) return rc;
        if ((rc = e.dev.tails_hr.upload(ix.tails_hr, "upload tails"))) return rc;
        if ((rc = e.dev.heads_tr.upload(ix.heads_tr, "upload heads"))) return rc;
        if ((rc = e.dev.rels_ht.upload(ix.rels_ht, "upload rels"))) return rc;
        if ((rc = e.dev.bern_prob.upload(ix.bern_prob, "upload bern"))) return rc;
        e.dev.uploaded = true;
    }
    if (!e.dev.tables_uploaded) {
        const KgIndex &ix = e.index;
        if ((rc = e.dev.jump_digits.upload(e.jump_digits, "upload jump digits"))) return rc;
        if ((rc = e.dev.ent_magic.upload(ix.ent_magic, "upload entity moduli"))) return rc;
        if ((rc = e.dev.rel_magic.upload(ix.rel_magic, "upload relation moduli"))) return rc;
        e.dev.tables_uploaded = true;
    }
    if ((int64_t)e.streams.size() != e.work_threads) {
        // setWorkThreads without randReset: the reference would read unallocated memory; give zeros
        e.streams.assign((size_t)e.work_threads, 0);
        e.dev.streams_sync = 0;
    }
    if (e.dev.streams_sync == 0) {
        bool grew;
        rc = e.dev.streams_buf.reserve(2 * e.work_threads, "alloc streams", &grew);
        if (grew) { e.dev.streams = e.dev.streams_buf; e.dev.streams_next = rc ? nullptr : e.dev.streams + e.work_threads; }   // (both null after a failure)
        if (rc) return rc;
        if ((rc = hip_check(hipMemcpy(e.dev.streams, e.streams.data(), sizeof(uint64_t) * (size_t)e.work_threads,
                                      hipMemcpyHostToDevice), "upload streams"))) return rc;
        e.dev.streams_sync = 1;
    }
    return KGE_OK;
}

int ensure_typed_host_index() {
    Engine &e = engine();
    if (!e.index.loaded) return fail(KGE_ERR_NO_DATASET, "type-constrained sampling: no training set imported");
    if (e.index.typed_built) return KGE_OK;
    TypeListsHost v;
    if (!eval_type_lists_host(v))
        return fail(KGE_ERR_NO_DATASET, "type-constrained sampling: no type file imported (importTypeFiles reads type_constrain.txt) and no lists set or derived "
                                        "(kge_set_type_lists / kge_derive_type_lists)");
    const std::string err = build_typed_index(e.index, *v.head_lef, *v.head_rig, *v.head_type, *v.tail_lef, *v.tail_rig, *v.tail_type);
    e.dev.typed_uploaded = false;
    if (!err.empty()) return fail(KGE_ERR_BAD_ARG, "type-constrained sampling: " + err);
    return KGE_OK;
}

int ensure_typed_index(bool always) {
    Engine &e = engine();
    if (!e.typed_sampling && !always) return KGE_OK;
    int rc = ensure_typed_host_index();
    if (rc) return rc;
    if (e.dev.typed_uploaded) return KGE_OK;
    if (!device_ok()) return fail(KGE_ERR_NO_DEVICE, "no usable HIP device: the sampler has no CPU fallback");
    const KgIndex &ix = e.index;
    if ((rc = e.dev.typed_len.upload(ix.typed_len, "upload typed lengths"))) return rc;
    if ((rc = e.dev.type_bounds.upload(ix.type_bounds, "upload type bounds"))) return rc;
    if ((rc = e.dev.type_tails.upload(ix.type_tails, "upload tail type lists"))) return rc;
    if ((rc = e.dev.type_heads.upload(ix.type_heads, "upload head type lists"))) return rc;
    if ((rc = e.dev.typed_pos_hr.upload(ix.typed_pos_hr, "upload typed positions"))) return rc;
    if ((rc = e.dev.typed_pos_tr.upload(ix.typed_pos_tr, "upload typed positions"))) return rc;
    e.dev.typed_uploaded = true;
    return KGE_OK;
}

static int pull_streams() {
    Engine &e = engine();
    { int rc = flush_attached_sampler(nullptr); if (rc) return rc; }   // an armed sampler has yet to write the states being read
    if (e.dev.streams_sync == 2) {
        int rc = hip_check(hipMemcpy(e.streams.data(), e.dev.streams, sizeof(uint64_t) * e.streams.size(),
                                     hipMemcpyDeviceToHost), "download streams");
        if (rc) return rc;
        e.dev.streams_sync = 1;
    }
    return KGE_OK;
}

static void adopt_index(KgIndex &&ix) {
    Engine &e = engine();
    e.index = std::move(ix);
    e.dev.uploaded = false;
}

// Reader.h:102-177 on the host (kg_index.cpp) or, for large training sets, on the device (index_build.hip);
// both produce the same arrays bit for bit
static std::string build_and_adopt(int64_t E, int64_t R, int64_t nb, int64_t n, const int64_t *h, const int64_t *t, const int64_t *r) {
    Engine &e = engine();
    // an armed sampler (kge_sampling_attach) points into the index arrays that are about to be replaced: run it first
    if (device_ok()) { (void)flush_attached_sampler(nullptr); (void)hipDeviceSynchronize(); }
    if (e.index_device_min >= 0 && n >= e.index_device_min && device_ok() && device_index_build_supported(E, R, n)) {
        KgIndex ix;
        std::string err = build_index_device(ix, e.dev, E, R, nb, n, h, t, r);
        if (!err.empty()) { e.dev.uploaded = false; return err; }
        e.index = std::move(ix);   // e.dev already holds the arrays (uploaded = true)
    } else {
        KgIndex ix;
        std::string err = build_index(ix, E, R, nb, n, h, t, r);
        if (!err.empty()) return err;
        adopt_index(std::move(ix));
    }
    build_magic_tables(e.index, e.sampler_magic_len);
    e.dev.tables_uploaded = false;
    e.index_generation++;
    return "";
}

void transe_team_shape(int D, int &L, int &C);   // models.hip
}  // namespace kge

using namespace kge;

extern "C" {

void setInPath(char *path) {
    engine().in_path = path ? path : "";
    std::printf("Input Files Path : %s\n", engine().in_path.c_str());
}

void setOutPath(char *path) {
    engine().out_path = path ? path : "";
    std::printf("Output Files Path : %s\n", engine().out_path.c_str());
}

void setWorkThreads(INT threads) { engine().work_threads = threads < 1 ? 1 : threads; }
INT getWorkThreads(void) { return engine().work_threads; }
void setBern(INT con) { engine().bern = con; }

void randReset(void) {
    Engine &e = engine();
    e.streams.resize((size_t)e.work_threads);
    for (auto &s : e.streams) s = (uint64_t)(int64_t)e.libc.next();
    e.dev.streams_sync = 0;
}

void importTrainFiles(void) {
    Engine &e = engine();
    std::printf("The toolkit is importing datasets.\n");
    int64_t E = 0, R = 0, nb = 0;
    std::vector<int64_t> h, t, r;
    std::string err = load_openke_dir(e.in_path, E, R, nb, h, t, r);
    if (!err.empty()) {
        std::cout << err << std::endl;  // the reference prints and returns (Reader.h:36-39)
        set_error(err);
        return;
    }
    std::printf("The total of relations is %ld.\n", (long)R);
    std::printf("The total of entities is %ld.\n", (long)E);
    if (nb > 0) std::printf("The total number of new batch triples is: %ld\n", (long)nb);
    std::printf("The total of train triples is %ld.\n", (long)h.size());
    err = build_and_adopt(E, R, nb, (int64_t)h.size(), h.data(), t.data(), r.data());
    if (!err.empty()) { set_error(err); return; }
    std::fflush(stdout);
}

INT getEntityTotal(void) { return engine().index.ent_total; }
INT getRelationTotal(void) { return engine().index.rel_total; }
INT kge_eval_test_total(void); INT kge_eval_valid_total(void); INT kge_eval_triple_total(void);
INT getTripleTotal(void) { return kge_eval_triple_total(); }  // set by importTestFiles (Reader.h:231)
INT getTrainTotal(void) { return engine().index.train_uniq; }
INT getTrainTotal_(void) { return engine().index.train_dup; }
INT getBatchTotal(void) { return engine().index.new_batch; }
INT getTestTotal(void) { return kge_eval_test_total(); }
INT getValidTotal(void) { return kge_eval_valid_total(); }

void sampling(INT *batch_h, INT *batch_t, INT *batch_r, REAL *batch_y, INT batchSize, INT negRate, INT negRelRate) {
    Engine &e = engine();
    if (ensure_device_index()) return;
    if (batchSize <= 0 || negRate < 0 || negRelRate < 0) { set_error("sampling: bad sizes"); return; }
    const int64_t total = batchSize * (1 + negRate + negRelRate);
    if (e.dev.stage_i32.reserve(3 * total, "alloc stage")) return;
    if (e.dev.stage_i64.reserve((int64_t)(sizeof(int64_t) * 3 + sizeof(float)) * total, "alloc stage")) return;
    int32_t *s = e.dev.stage_i32;
    // stage arrays are packed at `total` so the widen kernel can address them as [3][total]
    if (launch_sampler(s, s + total, s + 2 * total, batchSize, negRate, negRelRate, 0, e.work_threads, batchSize, nullptr, nullptr)) return;
    int64_t *w = reinterpret_cast<int64_t *>(e.dev.stage_i64.ptr());
    if (launch_widen(s, w, batchSize, total, nullptr)) return;
    if (hip_check(hipMemcpy(batch_h, w, sizeof(int64_t) * total, hipMemcpyDeviceToHost), "copy batch_h")) return;
    if (hip_check(hipMemcpy(batch_t, w + total, sizeof(int64_t) * total, hipMemcpyDeviceToHost), "copy batch_t")) return;
    if (hip_check(hipMemcpy(batch_r, w + 2 * total, sizeof(int64_t) * total, hipMemcpyDeviceToHost), "copy batch_r")) return;
    hip_check(hipMemcpy(batch_y, w + 3 * total, sizeof(float) * total, hipMemcpyDeviceToHost), "copy batch_y");
}

size_t kge_last_error(char *buf, size_t n) {
    const std::string &s = engine().last_error;
    if (buf && n) {
        size_t k = s.size() < n - 1 ? s.size() : n - 1;
        std::memcpy(buf, s.data(), k);
        buf[k] = 0;
    }
    return s.size();
}

void kge_clear_error(void) { engine().last_error.clear(); }
int kge_workspace_bytes(int64_t *live, int64_t *peak, int reset_peak) {
    if (live) *live = g_dev_buf_bytes.live;
    if (peak) *peak = g_dev_buf_bytes.peak;
    if (reset_peak) g_dev_buf_bytes.peak = g_dev_buf_bytes.live;
    return KGE_OK;
}
int kge_device_available(void) { return device_ok() ? 1 : 0; }
const char *kge_version(void) { return "kge_mi355 0.1 (gfx950)"; }

int kge_set_option(const char *name, INT value) {
    std::string n = name ? name : "";
    if (n == "counts_force_sort") { engine().counts_force_sort = value != 0; return KGE_OK; }
    if (n == "sampler_magic_len") {   // an armed sampler points into the tables that are about to be replaced: run it first
        Engine &e = engine();
        if (device_ok()) { (void)flush_attached_sampler(nullptr); (void)hipDeviceSynchronize(); }
        e.sampler_magic_len = value > 0 ? value : 0;
        if (e.index.loaded) build_magic_tables(e.index, e.sampler_magic_len);
        e.dev.tables_uploaded = false;
        return KGE_OK;
    }
    if (n == "counts_sort_tiles") { engine().counts_sort_tiles = value > 0 ? (int)value : 0; return KGE_OK; }
    if (n == "counts_sort_blocked") { engine().counts_sort_blocked = value > 0 ? (int)value : 0; return KGE_OK; }
    if (n == "ride_shares") { engine().ride_shares = (int)value; return KGE_OK; }
    if (n == "transr_bf16x3") { engine().transr_bf16x3 = value != 0; return KGE_OK; }
    if (n == "transr_groups") { engine().transr_groups = (int)value; return KGE_OK; }
    if (n == "transr_fuse_vec") { engine().transr_fuse_vec = value != 0; return KGE_OK; }
    if (n == "shared_transr_stages") { engine().shared_transr_stages = value >= 1 && value <= 5 ? (int)value : 5; return KGE_OK; }
    if (n == "counts_fused") { engine().counts_fused = value != 0; return KGE_OK; }
    if (n == "counts_fused_diag") { engine().counts_fused_diag = (int)value; return KGE_OK; }
    if (n == "counts_fused_cap") { engine().counts_fused_cap = value > 0 ? (int)value : 0; return KGE_OK; }
    if (n == "counts_fused_tail") { engine().counts_fused_tail = value != 0; return KGE_OK; }
    if (n == "inv_table_max_bytes") { engine().inv_table_max_bytes = value; return KGE_OK; }
    if (n == "tables_changed") { tables_written(); return KGE_OK; }     // the caller wrote device tables itself (value ignored)
    if (n == "counts_krel") { int k = 1; while (k * 2 <= value && k < 64) k *= 2; engine().counts_krel = k; return KGE_OK; }
    if (n == "inv_carry") { engine().inv_carry = value != 0; tables_written(); return KGE_OK; }
    if (n == "emit_rounds") { engine().emit_rounds = value != 0; return KGE_OK; }
    if (n == "emit_pack") { engine().emit_pack = value != 0; return KGE_OK; }
    if (n == "emit_keys_grouped") { engine().emit_keys_grouped = value != 0; return KGE_OK; }
    if (n == "counts_sort_test_group") { engine().counts_sort_test_group = value > 0 ? (int)value : 0; return KGE_OK; }
    if (n == "float_records") { engine().float_records = value != 0; return KGE_OK; }
    if (n == "float_records_min") { engine().float_records_min = value; return KGE_OK; }
    if (n == "index_device_min") { engine().index_device_min = value; return KGE_OK; }
    if (n == "eval_index_device_min") { engine().eval_index_device_min = value; return KGE_OK; }
    if (n == "hub_copies") { engine().hub_copies = value != 0; return KGE_OK; }
    if (n == "pair_counts") { engine().pair_counts = value != 0; return KGE_OK; }
    if (n == "record_emit_event") { engine().record_emit_event = value != 0; return KGE_OK; }
    if (n == "transr_dgrad_records") { engine().transr_dgrad_records = value != 0; return KGE_OK; }
    if (n == "transr_dgrad_records_min") { engine().transr_dgrad_records_min = value; return KGE_OK; }
    if (n == "transr_lean") { engine().transr_lean = value != 0; return KGE_OK; }
    if (n == "pair_counts_min_neg") { engine().pair_counts_min_neg = (int)value; return KGE_OK; }
    if (n == "topk_table_max_bytes") { engine().topk_table_max_bytes = value; return KGE_OK; }
    if (n == "relpred_chunk_bytes") { engine().relpred_chunk_bytes = value; return KGE_OK; }
    if (n == "lp_v1") { engine().lp_v1 = value != 0; return KGE_OK; }
    if (n == "rank_slices") { engine().rank_slices = value > 0 ? (int)value : 0; return KGE_OK; }
    if (n == "rankc_slices") { engine().rankc_slices = value > 0 ? (int)value : 0; return KGE_OK; }
    if (n == "rankc_fused") { engine().rankc_fused = value != 0; return KGE_OK; }
    if (n == "transr_v1") { engine().transr_v1 = (int)value; return KGE_OK; }
    if (n == "time_emit") { engine().time_emit = value > 0 ? (int)value : 0; if (value > 0) { engine().emit_launches = 0; engine().emit_seen = 0; } return KGE_OK; }
    if (n == "time_sampler") { engine().time_sampler = value > 0 ? (int)value : 0; if (value > 0) { engine().samp_launches = 0; engine().samp_seen = 0; } return KGE_OK; }
    if (n == "fb_occ4") { engine().fb_occ4 = value != 0; return KGE_OK; }
    if (n == "persist_ahead") { engine().persist_ahead = value != 0; return KGE_OK; }
    if (n == "persist_touch") { engine().persist_touch = value != 0; return KGE_OK; }
    if (n == "persist_trace") { engine().persist_trace = value != 0; return KGE_OK; }
    if (n == "persist_threads") { engine().persist_threads = value == 1024 ? 1024 : 512; return KGE_OK; }
    if (n == "libc_rand_restart") { engine().libc = LibcRand(); return KGE_OK; }  // as in a fresh process
    return fail(KGE_ERR_BAD_ARG, "kge_set_option: unknown option " + n);
}

int kge_last_kernel_ms(const char *name, float *ms) {
    Engine &e = engine();
    std::string n = name ? name : "";
    if ((n != "transe_emit" && n != "sampler") || !ms) return fail(KGE_ERR_BAD_ARG, "kge_last_kernel_ms: unknown kernel " + n);
    const bool samp = n == "sampler";
    const long long done = samp ? e.samp_launches : e.emit_launches;
    hipEvent_t *ev0 = samp ? e.ev_samp0 : e.ev_emit0, *ev1 = samp ? e.ev_samp1 : e.ev_emit1;
    if (done <= 0) return fail(KGE_ERR_BAD_ARG, "kge_last_kernel_ms: enable option time_emit / time_sampler and run a step first");
    const int slot = (int)((done - 1) % Engine::kEmitRing);
    if (hip_check(hipEventSynchronize(ev1[slot]), "event sync")) return KGE_ERR_NO_DEVICE;
    return hip_check(hipEventElapsedTime(ms, ev0[slot], ev1[slot]), "event elapsed");
}

int kge_kernel_ms_mean(const char *name, float *mean_ms, INT *launches) {
    Engine &e = engine();
    std::string n = name ? name : "";
    if ((n != "transe_emit" && n != "sampler") || !mean_ms) return fail(KGE_ERR_BAD_ARG, "kge_kernel_ms_mean: unknown kernel " + n);
    const bool samp = n == "sampler";
    const long long done = samp ? e.samp_launches : e.emit_launches;
    hipEvent_t *ev0 = samp ? e.ev_samp0 : e.ev_emit0, *ev1 = samp ? e.ev_samp1 : e.ev_emit1;
    const long long have = done < Engine::kEmitRing ? done : (long long)Engine::kEmitRing;
    if (have <= 0) return fail(KGE_ERR_BAD_ARG, "kge_kernel_ms_mean: enable option time_emit / time_sampler and run steps first");
    double sum = 0.0;
    for (long long i = 0; i < have; i++) {
        const int slot = (int)((done - 1 - i) % Engine::kEmitRing);
        float ms = 0.f;
        if (hip_check(hipEventSynchronize(ev1[slot]), "event sync")) return KGE_ERR_NO_DEVICE;
        if (hip_check(hipEventElapsedTime(&ms, ev0[slot], ev1[slot]), "event elapsed")) return KGE_ERR_NO_DEVICE;
        sum += ms;
    }
    *mean_ms = (float)(sum / (double)have);
    if (launches) *launches = have;
    return KGE_OK;
}

int kge_import_train_arrays(INT ent_total, INT rel_total, INT n, const INT *h, const INT *t, const INT *r,
                            INT new_batch_total) {
    std::string err = build_and_adopt(ent_total, rel_total, new_batch_total, n, (const int64_t *)h, (const int64_t *)t,
                                      (const int64_t *)r);
    if (!err.empty()) return fail(KGE_ERR_BAD_ARG, err);
    return KGE_OK;
}

int64_t kge_index_copy(const char *what, void *dst, int64_t bytes) {
    const KgIndex &ix = engine().index;
    if (!ix.loaded) return fail(KGE_ERR_NO_DATASET, "kge_index_copy: no dataset");
    const void *src = nullptr;
    int64_t have = 0;
    std::string w = what ? what : "";
    const bool typed = w == "type_tails" || w == "type_heads" || w == "type_bounds" || w == "typed_pos_hr" || w == "typed_pos_tr" ||
                       w == "typed_len";
    if (typed) { int rc = ensure_typed_host_index(); if (rc) return rc; }
#define KGE_ARR(name, vec) if (w == name) { src = (vec).data(); have = (int64_t)((vec).size() * sizeof((vec)[0])); }
    KGE_ARR("tails_hr", ix.tails_hr) KGE_ARR("heads_tr", ix.heads_tr) KGE_ARR("rels_ht", ix.rels_ht)
    KGE_ARR("pos", ix.pos) KGE_ARR("grp", ix.grp) KGE_ARR("ht", ix.ht)
    KGE_ARR("left_mean", ix.left_mean) KGE_ARR("right_mean", ix.right_mean) KGE_ARR("bern_prob", ix.bern_prob)
    KGE_ARR("type_tails", ix.type_tails) KGE_ARR("type_heads", ix.type_heads) KGE_ARR("type_bounds", ix.type_bounds)
    KGE_ARR("typed_pos_hr", ix.typed_pos_hr) KGE_ARR("typed_pos_tr", ix.typed_pos_tr) KGE_ARR("typed_len", ix.typed_len)
    KGE_ARR("jump_digits", engine().jump_digits) KGE_ARR("ent_magic", ix.ent_magic) KGE_ARR("rel_magic", ix.rel_magic)
#undef KGE_ARR
    if (!src && have == 0 && !typed && w != "jump_digits" && w != "ent_magic" && w != "rel_magic" && w != "tails_hr" && w != "heads_tr" && w != "rels_ht" && w != "pos" && w != "grp" && w != "ht" &&
        w != "left_mean" && w != "right_mean" && w != "bern_prob")
        return fail(KGE_ERR_BAD_ARG, "kge_index_copy: unknown array " + w);
    if (dst && bytes > 0 && have > 0) std::memcpy(dst, src, (size_t)(bytes < have ? bytes : have));
    return have;
}

int kge_set_typed_sampling(INT on) {
    Engine &e = engine();
    int rc = flush_attached_sampler(nullptr);   // an armed sampler draws its batch in the mode it was armed in
    if (rc) return rc;
    if (on && (rc = ensure_typed_host_index())) return rc;   // (the device copy follows with the first batch drawn)
    e.typed_sampling = on ? 1 : 0;
    return KGE_OK;
}

int kge_typed_sampling(void) { return engine().typed_sampling; }

int kge_get_stream_states(uint64_t *dst, INT n) {
    Engine &e = engine();
    int rc = pull_streams();
    if (rc) return rc;
    for (INT i = 0; i < n && i < (INT)e.streams.size(); i++) dst[i] = e.streams[(size_t)i];
    return KGE_OK;
}

int kge_set_stream_states(const uint64_t *src, INT n) {
    Engine &e = engine();
    if (n != e.work_threads) return fail(KGE_ERR_BAD_ARG, "kge_set_stream_states: n must equal workThreads");
    // a sampler launched on another (non-blocking) stream may still be writing the other half of the device state buffer, which
    // the next upload reuses; nothing orders a blocking copy on the null stream behind it, so drain the device first (rare,
    // control-path call: restore / tests)
    if (e.dev.streams && device_ok()) { (void)flush_attached_sampler(nullptr); (void)hipDeviceSynchronize(); }
    e.streams.assign(src, src + n);
    e.dev.streams_sync = 0;
    return KGE_OK;
}

INT kge_slice_positions(INT batchSize, INT thread_lo, INT thread_hi, INT *first_position) {
    const int64_t W = engine().work_threads;
    if (batchSize <= 0 || thread_lo < 0 || thread_hi > W || thread_lo >= thread_hi) {
        if (first_position) *first_position = 0;
        return 0;
    }
    int64_t lo, hi, tmp;
    thread_slice(batchSize, W, thread_lo, lo, tmp);
    thread_slice(batchSize, W, thread_hi - 1, tmp, hi);
    if (first_position) *first_position = lo;
    return hi - lo;
}

int kge_sampling_attach(int32_t *d_h, int32_t *d_t, int32_t *d_r, INT batchSize, INT negRate, INT negRelRate,
                        INT thread_lo, INT thread_hi, INT out_stride, INT *n_local, void *stream) {
    return kge_sampling_attach_packed(d_h, d_t, d_r, nullptr, batchSize, negRate, negRelRate, thread_lo, thread_hi, out_stride, n_local, stream);
}

int kge_sampling_attach_packed(int32_t *d_h, int32_t *d_t, int32_t *d_r, int32_t *d_pack, INT batchSize, INT negRate, INT negRelRate,
                               INT thread_lo, INT thread_hi, INT out_stride, INT *n_local, void *stream) {
    int64_t nl = 0;
    int rc = attach_sampler(d_h, d_t, d_r, batchSize, negRate, negRelRate, thread_lo, thread_hi, out_stride, &nl, (hipStream_t)stream, d_pack);
    if (n_local) *n_local = nl;
    return rc;
}

INT kge_emit_pack_words(INT n_positions, INT negRate, INT negRelRate, INT dim) {
    const KgIndex &ix = engine().index;
    if (n_positions <= 0 || negRate < 0 || negRelRate < 0 || !emit_pack_shape(ix.ent_total, ix.rel_total, negRate, negRelRate)) return 0;
    if (dim > 0) {   // only the round body reads a pack: the widths whose team is one wave with four elements per lane
        int L = 0, C = 0;
        transe_team_shape((int)dim, L, C);
        if (dim % 4 != 0 || L != 64 || C > 4) return 0;
    }
    return n_positions << sampler_kshift(negRate, negRelRate);
}

int kge_sampling_flush(void *stream) { return flush_attached_sampler((hipStream_t)stream); }

int kge_sampling_device(int32_t *d_h, int32_t *d_t, int32_t *d_r, INT batchSize, INT negRate, INT negRelRate,
                        INT thread_lo, INT thread_hi, INT out_stride, INT *n_local, void *stream) {
    return kge_sampling_device_packed(d_h, d_t, d_r, nullptr, batchSize, negRate, negRelRate, thread_lo, thread_hi, out_stride, n_local, stream);
}

int kge_sampling_device_packed(int32_t *d_h, int32_t *d_t, int32_t *d_r, int32_t *d_pack, INT batchSize, INT negRate, INT negRelRate,
                               INT thread_lo, INT thread_hi, INT out_stride, INT *n_local, void *stream) {
    int64_t nl = 0;
    int rc = launch_sampler(d_h, d_t, d_r, batchSize, negRate, negRelRate, thread_lo, thread_hi, out_stride, &nl,
                            (hipStream_t)stream, d_pack);
    if (n_local) *n_local = nl;
    return rc;
}

int kge_table_shape(const kge_model_desc *m, int table, int64_t *rows, int64_t *cols) {
    if (!m || !rows || !cols) return KGE_ERR_BAD_ARG;
    *rows = 0; *cols = 0;
    switch (table) {
        case 0: *rows = m->ent_total; *cols = m->ent_dim; break;
        case 1: *rows = m->rel_total; *cols = m->rel_dim; break;
        case 2:
            if (m->model == KGE_TRANSH || m->model == KGE_TRANSD) { *rows = m->rel_total; *cols = m->rel_dim; }
            if (m->model == KGE_TRANSR) { *rows = m->rel_total; *cols = (int64_t)m->ent_dim * m->rel_dim; }
            break;
        case 3:
            if (m->model == KGE_TRANSD) { *rows = m->ent_total; *cols = m->ent_dim; }
            break;
        default: return KGE_ERR_BAD_ARG;
    }
    return KGE_OK;
}

int kge_forward_backward(const kge_model_desc *m, const float *const tables[KGE_MAX_TABLES], const int32_t *d_h,
                         const int32_t *d_t, const int32_t *d_r, INT n_pos, INT n_neg, INT stride, INT denom,
                         float *const grads[KGE_MAX_TABLES], float *d_loss, void *stream) {
    if (!m || !tables || !grads || !d_loss) return fail(KGE_ERR_BAD_ARG, "kge_forward_backward: null argument");
    return launch_forward_backward(*m, tables, d_h, d_t, d_r, n_pos, n_neg, stride, denom, grads, d_loss, (hipStream_t)stream, false);
}

int kge_forward_backward_sgd_rows(const kge_model_desc *m, float *const tables[KGE_MAX_TABLES], const int32_t *d_h, const int32_t *d_t,
                                  const int32_t *d_r, INT n_pos, INT n_neg, INT stride, INT denom, float lr, float *d_loss, void *stream) {
    if (!m || !tables || !d_loss) return fail(KGE_ERR_BAD_ARG, "kge_forward_backward_sgd_rows: null argument");
    if (!(lr > 0.f)) return fail(KGE_ERR_BAD_ARG, "kge_forward_backward_sgd_rows: learning rate must be positive");
    return launch_forward_backward(*m, tables, d_h, d_t, d_r, n_pos, n_neg, stride, denom, tables, d_loss, (hipStream_t)stream, false, lr);
}

int kge_forward_backward_records(const kge_model_desc *m, const float *const tables[KGE_MAX_TABLES], const int32_t *d_h, const int32_t *d_t,
                                 const int32_t *d_r, INT n_pos, INT n_neg, INT stride, INT denom, INT n_pos_total, float *d_rec,
                                 int32_t *d_dst, INT rec_offset, INT rec_slice, float *d_loss, void *stream) {
    if (!m || !tables || !d_loss) return fail(KGE_ERR_BAD_ARG, "kge_forward_backward_records: null argument");
    return launch_forward_backward_records(*m, tables, d_h, d_t, d_r, n_pos, n_neg, stride, denom, n_pos_total, d_rec, d_dst, rec_offset,
                                           rec_slice, d_loss, (hipStream_t)stream);
}

int kge_float_records_apply(const kge_model_desc *m, float *const tables[KGE_MAX_TABLES], const float *d_rec, int32_t *d_dst, INT n_records,
                            INT n_pos_total, INT n_neg, float lr, void *stream) {
    if (!m || !tables) return fail(KGE_ERR_BAD_ARG, "kge_float_records_apply: null argument");
    return launch_float_records_apply(*m, tables, d_rec, d_dst, n_records, n_pos_total, n_neg, lr, (hipStream_t)stream);
}

// the moments of the model's tables (a table the model does not have: ignored), or false if one is missing
static bool adam_rows_of(const kge_model_desc &m, float *const tables[KGE_MAX_TABLES], float *const adam_m[KGE_MAX_TABLES],
                         float *const adam_v[KGE_MAX_TABLES], float lr_t, float beta1, float beta2, float eps, RowRule &ad) {
    ad = {};
    for (int t = 0; t < 4; t++) {
        if (!tables[t]) continue;
        if (!adam_m[t] || !adam_v[t]) return false;
        ad.m[t] = adam_m[t]; ad.v[t] = adam_v[t];
    }
    ad.lr_t = lr_t; ad.b1 = beta1; ad.b2 = beta2; ad.eps = eps; ad.rule = kRuleAdam;
    return true;
}

int kge_forward_backward_adam_rows(const kge_model_desc *m, float *const tables[KGE_MAX_TABLES], float *const adam_m[KGE_MAX_TABLES],
                                   float *const adam_v[KGE_MAX_TABLES], const int32_t *d_h, const int32_t *d_t, const int32_t *d_r, INT n_pos,
                                   INT n_neg, INT stride, INT denom, float lr_t, float beta1, float beta2, float eps, float *d_loss, void *stream) {
    if (!m || !tables || !adam_m || !adam_v || !d_loss) return fail(KGE_ERR_BAD_ARG, "kge_forward_backward_adam_rows: null argument");
    if (m->model == KGE_TRANSR) return fail(KGE_ERR_UNSUPPORTED, "lazy Adam on the touched rows: TransE / TransH / TransD only");
    RowRule ad;
    if (!adam_rows_of(*m, tables, adam_m, adam_v, lr_t, beta1, beta2, eps, ad))
        return fail(KGE_ERR_BAD_ARG, "kge_forward_backward_adam_rows: every table needs its two moment tables");
    return launch_forward_backward(*m, tables, d_h, d_t, d_r, n_pos, n_neg, stride, denom, tables, d_loss, (hipStream_t)stream, false, 0.f, &ad);
}

int kge_float_records_apply_adam(const kge_model_desc *m, float *const tables[KGE_MAX_TABLES], float *const adam_m[KGE_MAX_TABLES],
                                 float *const adam_v[KGE_MAX_TABLES], const float *d_rec, int32_t *d_dst, INT n_records, INT n_pos_total,
                                 INT n_neg, float lr_t, float beta1, float beta2, float eps, void *stream) {
    if (!m || !tables || !adam_m || !adam_v) return fail(KGE_ERR_BAD_ARG, "kge_float_records_apply_adam: null argument");
    RowRule ad;
    if (!adam_rows_of(*m, tables, adam_m, adam_v, lr_t, beta1, beta2, eps, ad))
        return fail(KGE_ERR_BAD_ARG, "kge_float_records_apply_adam: every table needs its two moment tables");
    return launch_float_records_apply_adam(*m, tables, ad, d_rec, d_dst, n_records, n_pos_total, n_neg, (hipStream_t)stream);
}

// the accumulators of the model's tables as the row rule's one slot table each, or false if one is missing
static bool adagrad_rows_of(float *const tables[KGE_MAX_TABLES], float *const acc[KGE_MAX_TABLES], float lr, RowRule &ad) {
    ad = {};
    for (int t = 0; t < 4; t++) {
        if (!tables[t]) continue;
        if (!acc[t]) return false;
        ad.m[t] = acc[t];
    }
    ad.lr_t = lr; ad.rule = kRuleAdagrad;
    return true;
}

int kge_forward_backward_adagrad_rows(const kge_model_desc *m, float *const tables[KGE_MAX_TABLES], float *const acc[KGE_MAX_TABLES],
                                      const int32_t *d_h, const int32_t *d_t, const int32_t *d_r, INT n_pos, INT n_neg, INT stride, INT denom,
                                      float lr, float *d_loss, void *stream) {
    if (!m || !tables || !acc || !d_loss) return fail(KGE_ERR_BAD_ARG, "kge_forward_backward_adagrad_rows: null argument");
    if (m->model == KGE_TRANSR) return fail(KGE_ERR_UNSUPPORTED, "Adagrad on the touched rows: TransE / TransH / TransD only");
    RowRule ad;
    if (!adagrad_rows_of(tables, acc, lr, ad))
        return fail(KGE_ERR_BAD_ARG, "kge_forward_backward_adagrad_rows: every table needs its accumulator table");
    return launch_forward_backward(*m, tables, d_h, d_t, d_r, n_pos, n_neg, stride, denom, tables, d_loss, (hipStream_t)stream, false, 0.f, &ad);
}

int kge_float_records_apply_adagrad(const kge_model_desc *m, float *const tables[KGE_MAX_TABLES], float *const acc[KGE_MAX_TABLES],
                                    const float *d_rec, int32_t *d_dst, INT n_records, INT n_pos_total, INT n_neg, float lr, void *stream) {
    if (!m || !tables || !acc) return fail(KGE_ERR_BAD_ARG, "kge_float_records_apply_adagrad: null argument");
    if (m->model == KGE_TRANSR) return fail(KGE_ERR_UNSUPPORTED, "Adagrad on the touched rows: TransE / TransH / TransD only");
    RowRule ad;
    if (!adagrad_rows_of(tables, acc, lr, ad))
        return fail(KGE_ERR_BAD_ARG, "kge_float_records_apply_adagrad: every table needs its accumulator table");
    return launch_float_records_apply_adam(*m, tables, ad, d_rec, d_dst, n_records, n_pos_total, n_neg, (hipStream_t)stream);
}

// the per-row accumulators of the model's tables ([rows] floats each) as the row rule's one slot each, or false if one is missing
static bool rowadagrad_rows_of(float *const tables[KGE_MAX_TABLES], float *const acc[KGE_MAX_TABLES], float lr, RowRule &ad) {
    ad = {};
    for (int t = 0; t < 4; t++) {
        if (!tables[t]) continue;
        if (!acc[t]) return false;
        ad.m[t] = acc[t];
    }
    ad.lr_t = lr; ad.rule = kRuleRowAdagrad;
    return true;
}

int kge_forward_backward_rowadagrad_rows(const kge_model_desc *m, float *const tables[KGE_MAX_TABLES], float *const acc[KGE_MAX_TABLES],
                                         const int32_t *d_h, const int32_t *d_t, const int32_t *d_r, INT n_pos, INT n_neg, INT stride, INT denom,
                                         float lr, float *d_loss, void *stream) {
    if (!m || !tables || !acc || !d_loss) return fail(KGE_ERR_BAD_ARG, "kge_forward_backward_rowadagrad_rows: null argument");
    if (m->model == KGE_TRANSR) return fail(KGE_ERR_UNSUPPORTED, "row-wise Adagrad on the touched rows: TransE / TransH / TransD only");
    RowRule ad;
    if (!rowadagrad_rows_of(tables, acc, lr, ad))
        return fail(KGE_ERR_BAD_ARG, "kge_forward_backward_rowadagrad_rows: every table needs its row accumulators");
    return launch_forward_backward(*m, tables, d_h, d_t, d_r, n_pos, n_neg, stride, denom, tables, d_loss, (hipStream_t)stream, false, 0.f, &ad);
}

int kge_float_records_apply_rowadagrad(const kge_model_desc *m, float *const tables[KGE_MAX_TABLES], float *const acc[KGE_MAX_TABLES],
                                       const float *d_rec, int32_t *d_dst, INT n_records, INT n_pos_total, INT n_neg, float lr, void *stream) {
    if (!m || !tables || !acc) return fail(KGE_ERR_BAD_ARG, "kge_float_records_apply_rowadagrad: null argument");
    if (m->model == KGE_TRANSR) return fail(KGE_ERR_UNSUPPORTED, "row-wise Adagrad on the touched rows: TransE / TransH / TransD only");
    RowRule ad;
    if (!rowadagrad_rows_of(tables, acc, lr, ad))
        return fail(KGE_ERR_BAD_ARG, "kge_float_records_apply_rowadagrad: every table needs its row accumulators");
    return launch_float_records_apply_adam(*m, tables, ad, d_rec, d_dst, n_records, n_pos_total, n_neg, (hipStream_t)stream);
}

int kge_loss_limbs_target(int32_t *d_limbs4) {
    engine().loss_limbs = d_limbs4;
    return KGE_OK;
}

int kge_sgd_rows_skipped(int32_t *n_negatives) {
    if (!n_negatives) return fail(KGE_ERR_BAD_ARG, "kge_sgd_rows_skipped: null argument");
    return sgd_rows_skipped(n_negatives);
}

int kge_pair_path_active(const kge_model_desc *m, INT n_pos, INT n_neg) { return m && pair_path_active(*m, n_pos, n_neg) ? 1 : 0; }

int kge_transr_group_layout_active(const kge_model_desc *m, INT n_pos, INT n_neg) {
    return m && transr_group_layout_active(*m, n_pos, n_neg) ? 1 : 0;
}

INT kge_transe_relation_copies(const kge_model_desc *m, INT n_pos) { return m ? transe_relation_copies(*m, n_pos) : 1; }

INT kge_float_records_chunk_len(INT n_records) { return float_records_chunk_len(n_records); }

int kge_stream_wait_emit(void *stream) {
    Engine &e = engine();
    // nothing recorded since the last wait (recording off, or this step's path has no emit kernel): the caller must order the
    // side stream some other way -- returning OK here would leave it with no dependency on the step at all
    if (!e.emit_done || e.emit_seq == e.emit_waited) return KGE_NO_EVENT;
    e.emit_waited = e.emit_seq;
    return hip_check(hipStreamWaitEvent((hipStream_t)stream, e.emit_done, 0), "wait for the emit kernel");
}

int kge_forward_backward_sampled(const kge_model_desc *m, const float *const tables[KGE_MAX_TABLES], const int32_t *d_h,
                                 const int32_t *d_t, const int32_t *d_r, INT n_pos, INT n_neg, INT stride, INT denom,
                                 float *const grads[KGE_MAX_TABLES], float *d_loss, void *stream) {
    if (!m || !tables || !grads || !d_loss) return fail(KGE_ERR_BAD_ARG, "kge_forward_backward_sampled: null argument");
    return launch_forward_backward(*m, tables, d_h, d_t, d_r, n_pos, n_neg, stride, denom, grads, d_loss, (hipStream_t)stream, true);
}

int kge_sgd_update(float *d_p, float *d_g, int64_t n, float lr, void *stream) {
    tables_written();
    return launch_sgd(d_p, d_g, n, lr, (hipStream_t)stream);
}

int kge_adam_update(float *d_p, float *d_m, float *d_v, float *d_g, int64_t n, float lr_t, float beta1, float beta2,
                    float eps, void *stream) {
    tables_written();
    return launch_adam(d_p, d_m, d_v, d_g, n, lr_t, beta1, beta2, eps, (hipStream_t)stream);
}

int kge_sgd_update_tables(int32_t n_tables, float *const d_p[KGE_MAX_TABLES], float *const d_g[KGE_MAX_TABLES],
                          const INT numel[KGE_MAX_TABLES], float lr, void *stream) {
    tables_written();
    return launch_sgd_tables(n_tables, d_p, d_g, (const int64_t *)numel, lr, (hipStream_t)stream);
}

int kge_adam_update_tables(int32_t n_tables, float *const d_p[KGE_MAX_TABLES], float *const d_m[KGE_MAX_TABLES],
                           float *const d_v[KGE_MAX_TABLES], float *const d_g[KGE_MAX_TABLES], const INT numel[KGE_MAX_TABLES],
                           float lr_t, float beta1, float beta2, float eps, void *stream) {
    tables_written();
    return launch_adam_tables(n_tables, d_p, d_m, d_v, d_g, (const int64_t *)numel, lr_t, beta1, beta2, eps, (hipStream_t)stream);
}

int kge_adagrad_update(float *d_p, float *d_acc, float *d_g, int64_t n, float lr, void *stream) {
    if (!d_p || !d_acc || !d_g) return fail(KGE_ERR_BAD_ARG, "kge_adagrad_update: null argument");
    tables_written();
    return launch_adagrad(d_p, d_acc, d_g, n, lr, (hipStream_t)stream);
}

int kge_adagrad_update_tables(int32_t n_tables, float *const d_p[KGE_MAX_TABLES], float *const d_acc[KGE_MAX_TABLES],
                              float *const d_g[KGE_MAX_TABLES], const INT numel[KGE_MAX_TABLES], float lr, void *stream) {
    tables_written();
    return launch_adagrad_tables(n_tables, d_p, d_acc, d_g, (const int64_t *)numel, lr, (hipStream_t)stream);
}

int kge_rowadagrad_update_tables(int32_t n_tables, float *const d_p[KGE_MAX_TABLES], float *const d_acc[KGE_MAX_TABLES],
                                 float *const d_g[KGE_MAX_TABLES], const INT rows[KGE_MAX_TABLES], const INT row_len[KGE_MAX_TABLES], float lr,
                                 void *stream) {
    tables_written();
    return launch_rowadagrad_tables(n_tables, d_p, d_acc, d_g, (const int64_t *)rows, (const int64_t *)row_len, lr, (hipStream_t)stream);
}

int kge_predict(const kge_model_desc *m, const float *const tables[KGE_MAX_TABLES], const int32_t *d_h,
                const int32_t *d_t, const int32_t *d_r, INT n, float *d_out, void *stream) {
    if (!m || !tables || !d_out) return fail(KGE_ERR_BAD_ARG, "kge_predict: null argument");
    return launch_predict(*m, tables, d_h, d_t, d_r, n, d_out, (hipStream_t)stream);
}

}  // extern "C"
