/*
 * kge_mi355.h -- C ABI of libkge_mi355.so, the MI355X (gfx950) engine for the OpenKEonSpark hot path.
 *
 * Two groups of entry points:
 *
 *  (1) The hot-path subset of the reference's `Base.so` ABI, with the reference's exact unmangled
 *      names and signatures, so that /root/reference/Config.py:30-31,160-170,347 binds to this
 *      library unchanged (ctypes.cdll.LoadLibrary + the same calls).  INT = long (int64 on LP64),
 *      REAL = float (base/Setting.h:3-4).  `sampling` runs the HIP sampler and copies the batch
 *      into the caller's host buffers.
 *
 *  (2) `kge_*` entry points that replace what the reference does inside TensorFlow
 *      (`sess.run([train_op, loss, global_step], feed_dict)`, distribute_training.py:282) with
 *      device-resident operators: on-device sampling, fused gather/score/hinge/backward for
 *      TransE/H/D/R, SGD / TF-parity Adam updates, scoring for prediction.  Plain pointers and
 *      sizes only; device pointers are raw HIP device addresses (e.g. torch.Tensor.data_ptr()),
 *      `stream` is a hipStream_t passed as void* (NULL = default stream).
 *
 * Error convention: the reference has none (void functions, missing files only print;
 * Reader.h:36-39).  Here every kge_* function returns 0 on success or a negative code, the
 * Base-compatible void functions record a message, and `kge_last_error` returns the most recent
 * message (empty string if none).  There is NO CPU fallback: device entry points fail with
 * KGE_ERR_NO_DEVICE when no gfx950 device is usable.
 */
#ifndef KGE_MI355_H
#define KGE_MI355_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#ifndef INT
#define INT long
#endif
#ifndef REAL
#define REAL float
#endif

/* ------------------------------------------------------------------------------------------
 * (1) Base.so-compatible entry points
 * ---------------------------------------------------------------------------------------- */
void setInPath(char *path);       /* replaces base/Setting.h:12-19  */
void setOutPath(char *path);      /* replaces base/Setting.h:21-28  */
void setWorkThreads(INT threads); /* replaces base/Setting.h:36-39: number of VIRTUAL sampler threads (rng streams + batch slices) */
INT getWorkThreads(void);         /* replaces base/Setting.h:41-44  */
void setBern(INT con);            /* replaces base/Setting.h:110-113 */
void randReset(void);             /* replaces base/Random.h:8-13: seeds one 64-bit LCG stream per virtual thread from the (continuing) unseeded glibc rand() sequence */
void importTrainFiles(void);      /* replaces base/Reader.h:26-179: parse, dedup, build the device-resident filter index */
INT getEntityTotal(void);         /* replaces base/Setting.h:63-66  */
INT getRelationTotal(void);       /* replaces base/Setting.h:68-71  */
INT getTripleTotal(void);         /* replaces base/Setting.h:73-76  */
INT getTrainTotal(void);          /* replaces base/Setting.h:78-81  (after dedup) */
INT getTrainTotal_(void);         /* replaces base/Setting.h:84-87  (file count, duplicates kept) */
INT getBatchTotal(void);          /* replaces base/Setting.h:90-93  (newBatchTotal, incremental mode) */
INT getTestTotal(void);           /* replaces base/Setting.h:95-98  */
INT getValidTotal(void);          /* replaces base/Setting.h:100-103 */
/* replaces base/Base.cpp:149-172.  Caller-owned HOST buffers of length batchSize*(1+negRate+negRelRate),
 * layout [B positives | B negatives round 0 | ... | relation negatives] (Base.cpp:109-139).
 * Bit-identical to the reference for the same workThreads / bern / call history. */
void sampling(INT *batch_h, INT *batch_t, INT *batch_r, REAL *batch_y, INT batchSize, INT negRate, INT negRelRate);

/* Evaluation subset of Base.so (link prediction) */
void importTestFiles(void);      /* replaces base/Reader.h:185-292: test2id / valid2id + the sorted union used by the filter */
void importTypeFiles(void);      /* replaces base/Reader.h:301-365: type_constrain.txt */
void importOntologyFiles(void);  /* replaces base/Reader.h:375-449: ontology_constrain.txt */
void getHeadBatch(INT index, INT *ph, INT *pt, INT *pr);  /* replaces base/Test.h:10-17 */
void getTailBatch(INT index, INT *ph, INT *pt, INT *pr);  /* replaces base/Test.h:19-26 */
/* replace base/Test.h:30-136 and :140-249.  `con` = HOST score vector of all entities; returns 8 INT:
 * [0..3] candidates scoring strictly lower (raw, filtered, type-constrained, both), [4..7] ontology
 * class of the four arg-mins.  The pointer addresses a library-owned slot reused after 64 calls (the
 * reference leaks a `new INT[8]` per call). */
INT *testHead(INT index, REAL *con);
INT *testTail(INT index, REAL *con);
/* Triple classification (replace base/Test.h:252-444).  Host routines over
 * validTotal / testTotal-long score arrays, as in the reference: negatives are the positives with a
 * type-constrained new tail drawn with the (continuing) libc rand() sequence (Corrupt.h:118-137);
 * thresholds by grid search with step 0.01f per relation; get_TPFP returns (n_interval+1)*2 INT in a
 * library-owned buffer valid until the next call (the reference leaks a new[] per call). */
void getTestBatch(INT *ph, INT *pt, INT *pr, INT *nh, INT *nt, INT *nr);
void getValidBatch(INT *ph, INT *pt, INT *pr, INT *nh, INT *nt, INT *nr);
void getBestThreshold(REAL *relThresh, REAL *score_pos, REAL *score_neg);
void test_triple_classification(REAL *relThresh, REAL *score_pos, REAL *score_neg, REAL *acc);
INT get_n_interval(INT r, REAL *score_pos, REAL *score_neg);
INT *get_TPFP(INT r, REAL *score_pos, REAL *score_neg, REAL *threshold, REAL *unused);

/* ------------------------------------------------------------------------------------------
 * (2) Engine entry points
 * ---------------------------------------------------------------------------------------- */
enum {
    KGE_OK = 0,
    KGE_NO_EVENT = 1,         /* kge_stream_wait_emit: no emit launch was recorded since the previous wait */
    KGE_ERR_NO_DEVICE = -1,   /* no usable gfx950 device / HIP runtime error */
    KGE_ERR_NO_DATASET = -2,  /* importTrainFiles / kge_import_train_arrays not done */
    KGE_ERR_BAD_ARG = -3,
    KGE_ERR_UNSUPPORTED = -4
};

enum { KGE_TRANSE = 0, KGE_TRANSH = 1, KGE_TRANSR = 2, KGE_TRANSD = 3 };

/* copies the last error message (NUL terminated, truncated to n) and returns its length */
size_t kge_last_error(char *buf, size_t n);
void kge_clear_error(void);
/* 1 when a HIP device is visible and usable, else 0 (never throws, never falls back) */
int kge_device_available(void);
const char *kge_version(void);

/* engine options (testing / measurement).
 *   "counts_force_sort": 1 = order the sign-count records with rocPRIM's radix sort instead of the
 *                        hand-written two-level counting sort (default 0)
 *   "counts_fused":      1 (default) = kge_transe_train_step_counts sums the records of a row and applies the optimizer to it in one
 *                        kernel (rows whose int8 and 2-bit record lists hold up to 64 records each; longer rows and relation rows go through the count image);
 *                        0 = the two-kernel form (segmented sum into the image, then kge_transe_apply_counts_tables).  Same bits.
 *   "counts_sort_tiles": how the hand-written record sort runs: 1 (default) = two launches -- every tile of 2048 keys sorts its
 *                        live pairs by bucket and publishes its bucket offsets, then one workgroup per bucket collects its segments
 *                        and orders them by key -- with no sizing pass and no global atomics; 0 = the three-launch form (bucket
 *                        histogram, scatter through global cursors, bucket sort), which inputs of more than 2048 tiles (4 194 304
 *                        keys) take as well.  Same sorted keys and row spans; the order inside a key is unspecified in both.
 *                        1024 / 4096 = the two-launch form at that tile size (measurements)
 *   "counts_sort_blocked": layout of the two-launch sort's per-tile bucket offsets and order of its bucket pass: 1 (default) = one
 *                        packed word (start | length << 16) per (tile, bucket), stored block-major in blocks of 8 buckets, and
 *                        the bucket pass's workgroups take the buckets in an order that keeps neighbouring buckets on one XCD
 *                        (speed only); 0 = a row of 513 exclusive offsets per tile and bucket = workgroup index.  Same results.
 *                        4 / 16 = blocks of that many buckets (measurements; tile size 2048 only, other tile sizes take 8)
 *   "ride_shares":       where an armed sampler (kge_sampling_attach) rides: percent of its workgroups for the bucket histogram /
 *                        bucket scatter / bucket sort / the launch that ends the step, one byte each; parts that no launch took
 *                        are launched by kge_sampling_flush.  The two-launch sort has no histogram launch: byte 0 is ignored
 *                        there, byte 1 is its tile pass and byte 2 its bucket pass.  Default -1 = automatic: 100 << 8 (all of it in
 *                        the scatter launch) with the three-launch sort, 50 << 8 | 50 << 16 (half in each launch) with the
 *                        two-launch sort
 *   "sampler_magic_len": T (default 2048): filter groups of fewer than T known ids take the modulus of their filtered pick from the
 *                        tables "ent_magic" / "rel_magic" (kge_index_copy), longer ones from two fp64 divisions.  Same draws; the
 *                        tables of an imported training set are rebuilt at once (tests lower it so that both ways run)
 *   "counts_fused_diag": measurement hook of the fused kernel (1: no record loops, 2: no row update);
 *                        any value but 0 gives WRONG results.  With "counts_fused_tail" on, the teams of the image path still
 *                        take their tickets at 2 and the last one resets the row's counters: the next step starts clean
 *   "counts_fused_cap":  test hook: rows of more than this many records take the image path (0 = the default, 64)
 *   "counts_fused_tail": 1 (default) = in the fused step the rows that go through the count image (entity rows with a list
 *                        longer than the cap, and every relation row) are updated inside the fused kernel, by the last of
 *                        the teams that add into the row's image, and no closing apply launch is made; byte 3 of
 *                        "ride_shares" then rides in the fused kernel.  0 = the fused kernel, then the apply kernel over
 *                        those rows.  Same bits.
 *   "inv_table_max_bytes": the TransE emit kernel reads 1/|row| from a per-row table rebuilt every step while
 *                        the two tables are at most this many bytes (default 256 MiB); larger tables (or 0)
 *                        compute the norms from the gathered rows
 *   "float_records":     1 (default) = kge_forward_backward stores TransE/H/D gradient rows as records and sums
 *                        them by destination after a sort; 0 = fp32 atomic adds straight into the accumulators
 *   "float_records_min": smallest number of gradient rows per step that takes the record path (default 65536: measured cross-over, tools/sweep_paths.py)
 *   "tables_changed": the caller has written device parameter tables itself (a copy into them, an all-gather, a restored
 *                     checkpoint).  The TransE emit kernel keeps a table of 1/|row| that the full-table apply kernel
 *                     (kge_transe_apply_counts_tables) refreshes row by row, so that no pre-pass over the tables is needed between
 *                     steps; every kge_* entry point that writes tables marks it stale itself, this option is for writes the
 *                     library cannot see.  Value ignored.
 *   "counts_krel": dense TransE sign-count path: group b sends its relation-side records to virtual copy b % counts_krel of the
 *                     relation rows while they are ordered, the segmented sum folds the copies back (hub rows otherwise
 *                     serialise the LDS atomics of the bucketing kernels); a power of two, default 4 (measured best of 1..64), 1 = off
 *   "transr_dgrad_records" / "transr_dgrad_records_min": TransR backward w.r.t. the entity rows: 1 (default) = the rows of
 *                     G . M_r^T are stored as float records and summed per entity by the record sort + segmented sum from
 *                     `_min` (default 32768) projected rows per step on; 0 = fp32 atomics always
 *   "inv_carry": 0 = recompute that table in front of every emit launch (test hook; default 1)
 *   "emit_rounds": 1 (default) = the TransE emit kernel at widths 132..256 (multiples of 4) walks a group's negatives in rounds
 *                     of one corruption kind with raw buffer gathers and one merged reduction per round; 0 = its earlier body
 *                     (kernel transe_emit_vec_v1_kernel), which computes the same bits: A/B measurements and the tests' reference
 *   "emit_pack": 1 (default) = the _packed sampler entry points also write one packed word per negative, a group's words side by
 *                     side (kge_sampling_device_packed), and that round body reads a group's negatives from them -- one line per
 *                     group instead of a line per negative and id array; 0 = no pack is written or read and kge_emit_pack_words
 *                     returns 0, which is the step without it, bit for bit: A/B measurements and the tests' reference
 *   "emit_keys_grouped": 1 (default) = in kge_transe_train_step_counts at the round body's widths the emit kernel writes the record
 *                     keys of a group side by side (key of slot s of group b at word b * (3 + n_neg) + s: one store instruction
 *                     per group, one run of lines per workgroup) and the two-launch record sort turns a key's position into its
 *                     record id; records, record ids and kge_transe_step_scratch_read's view of the keys stay slot-major.
 *                     0 = slot-major keys (word s * n_pos + b), the step as it was, bit for bit.  Steps whose sort takes the
 *                     three-launch form, and every other producer of records, write slot-major keys whatever the value
 *   "counts_sort_test_group": test hook: S > 0 = kge_counts_sort_test takes its keys as group-major, n_keys / S groups of S (the
 *                     pair at position p gets the id (p % S) * (n_keys / S) + p / S); two-launch form only.  Default 0
 *   "record_emit_event": 1 = record an event behind every TransE emit launch (kge_stream_wait_emit); default 0
 *   "pair_counts":       1 (default) = TransH / TransD steps of at least float_records_min entity-side rows (widths that are
 *                        multiples of 4 up to 256, at most 63 negatives, ent_total*rel_total below 2^31) take the
 *                        pair-count path: int8 sign records keyed by (entity, relation), the backward applied once per pair
 *                        (csrc/pairs.hip); 0 = float records / atomics as for the other shapes
 *   "pair_counts_min_neg": fewest negatives per positive for that path; default 0 = the measured cross-over (TransH 5, TransD 3)
 *   "index_device_min":  training sets with at least this many lines are indexed on the device (rocPRIM sorts,
 *                        same arrays bit for bit); default 4194304, 0 = always, negative = never
 *   "eval_index_device_min": the same for kge_import_eval_arrays and kge_derive_type_lists, counted in triples of the union
 *                        train + valid + test (csrc/eval_build.hip); default 4194304 (not measured for that build)
 *   "hub_copies":        1 (default) = on the fp32-atomic TransH/TransD path, relation-side gradient rows that would
 *                        take >= 128 adds per step are accumulated in up to 64 copies and folded (same-address
 *                        atomics serialise); 0 = straight into the accumulators
 *   "transr_bf16x3":     1 (default) = TransR's row GEMMs and wgrad (dims <= 208, multiples of 4) form the fp32 products as six
 *                        bf16 x bf16 term products of an exact three-term split on the bf16 matrix pipe (error vs fp64 equal to the
 *                        fp32 MFMA's); 0 = the fp32 MFMA kernels
 *   "transr_groups":     TransR, device-sampled batches, 2 + negatives <= 16: 1 (default) = steps with well-filled relation buckets
 *                        sort GROUPS by relation and keep a group's rows inside one 16-row sub-tile; 2 = at any size; 0 = never
 *   "transr_fuse_vec":   1 (default) = with that layout the vector stage runs inside the projection's epilogue; 0 = as its own launch
 *   "transr_v1":         test hooks for the TransR MFMA tilings (default 0 = automatic): 1 = always the 32x32x2 tiles; 2 = 16x16x4
 *                        tiles with the all-output-tiles wgrad and its 512-row spans forced; 3 = 16x16x4 tiles with the 32x32x2 wgrad
 *   "time_emit":         N > 0 = bracket every N-th launch of the TransE emit kernel with HIP events on its launch stream
 *   "time_sampler":      N > 0 = the same around every N-th launch of the sampler's own kernels (kernel name "sampler"; a sampler
 *                        that rides in another kernel's launch is not timed)
 *   "fb_occ4":           1 (default) = TransH / TransD / TransR's vector stage at <= 4 elements per lane run the forward/backward body
 *                        compiled for four waves per SIMD (128 VGPRs); 0 = the uncapped build
 *   "persist_touch":     1 = the persistent launch requests all rows of a group together before its dependent gathers (default 0:
 *                        measured, no gain -- the phase is bound by same-address atomics, not by cold gathers)
 *   "persist_ahead":     1 (default) = teams without a group draw the next batch during the forward/backward phase
 *   "persist_trace":     1 = kge_train_steps_persistent stamps its phase boundaries (read with kge_persistent_trace)
 *   "persist_threads":   threads per workgroup of the persistent launch, 512 (default) or 1024
 *   "topk_table_max_bytes": kge_topk_entities (TransE / TransH / TransD / TransR) and kge_topk_entities_range (rows x dim x 4)
 *                     score the candidates from a table of their
 *                     projected, normalised vectors while it is at most this many bytes (E x dim x 4; default 1 GiB); larger
 *                     tables, or 0, compute the candidate side on the fly from the parameter rows (same functions, same bits)
 *   "relpred_chunk_bytes": kge_topk_relations / kge_relation_prediction / kge_relation_prediction_rows score their queries in
 *                     chunks whose [chunk x R] fp32 score block is at most this many bytes (default 256 MiB; at least one query
 *                     per chunk); TransR's buffer of projected distinct entities is held to the same size (at least one relation
 *                     per block).  Results do not depend on it, bit for bit
 *   "libc_rand_restart": restart the glibc-compatible seed generator, as in a fresh process (the next
 *                        randReset then yields 1804289383, 846930886, ... again) */
int kge_set_option(const char *name, INT value);
/* elapsed time of the most recent launch of a timed kernel; name = "transe_emit" (needs time_emit) or "sampler" (time_sampler) */
int kge_last_kernel_ms(const char *name, float *ms);
/* mean over the launches since "time_emit" / "time_sampler" was switched on (the most recent 512 of them); one event pair per launch, read
 * back here, so nothing synchronises inside the timed region */
int kge_kernel_ms_mean(const char *name, float *mean_ms, INT *launches);

/* Same as importTrainFiles but from arrays already in memory (h,t,r in FILE ORDER, duplicates
 * kept; new_batch_total as batch2id.txt's first line, 0 = not incremental).  Restates
 * Reader.h:82-177 without the text parse. */
int kge_import_train_arrays(INT ent_total, INT rel_total, INT n, const INT *h, const INT *t, const INT *r,
                            INT new_batch_total);

/* Host-side copies of the index, for inspection and CPU tests.  `what` is one of
 *   "tails_hr"  int32[trainTotal]  tails in (h,r,t) order         (= trainHead[].t, Reader.h:125)
 *   "heads_tr"  int32[trainTotal]  heads in (t,r,h) order         (= trainTail[].h, Reader.h:126)
 *   "rels_ht"   int32[trainTotal]  relations in (h,t,r) order     (= trainRel[].r,  Reader.h:127)
 *   "pos"       int32[trainTotal_][4]  file-order triples (h,t,r,0)             (= trainList_no)
 *   "grp"       int32[trainTotal_][4]  (hr_off,hr_len,tr_off,tr_len) per file-order triple
 *   "ht"        int32[trainTotal_][2]  (ht_off,ht_len) per file-order triple
 *   "left_mean" / "right_mean" float[relationTotal]               (Reader.h:160-177)
 *   "bern_prob" float[relationTotal]  1000*right/(right+left)      (Base.cpp:117)
 * and, built on first request from the imported type lists (kge_set_typed_sampling; an error without type lists),
 *   "type_tails" / "type_heads"  int32[]  every relation's tail / head type list, sorted, duplicates removed, back to back
 *   "type_bounds"  int32[relationTotal][4]  (tail_off,tail_len,head_off,head_len) into those two
 *   "typed_pos_hr" / "typed_pos_tr"  int32[trainTotal]  at a group's offset in tails_hr / heads_tr: the increasing positions
 *               inside the relation's list of the group's known ids that occur in it, then -1 up to the group's length
 *   "typed_len"  int32[trainTotal_][2]  per file-order triple: how many positions its (h,r) group and its (t,r) group have
 * and the device sampler's tables,
 *   "jump_digits"  uint64[4 * 512][2]  entry [k * 512 + d]: (mul, add) of x -> mul * x + add after d * 512^k steps of the 64-bit LCG
 *   "ent_magic" / "rel_magic"  uint64[sampler_magic_len]  entry len: (2^64 - 1) / (entityTotal - len) resp. (relationTotal - len),
 *               0 where that divisor is not positive
 * Returns the number of BYTES the array holds (copying at most `bytes` of them), <0 on error. */
int64_t kge_index_copy(const char *what, void *dst, int64_t bytes);

/* Same as importTestFiles but from arrays already in memory: the validation and test triples in any order, duplicates kept; the
 * training triples are the ones the engine holds (file order, duplicates kept -- the list importTestFiles re-reads from
 * train2id.txt).  Produces the state importTestFiles and the first device use produce for the same triples: `all` (h,r,t,0)
 * sorted by (h,r,t), `all_t` (t,r,h,0) by (t,r,h), `all_ht` (h,t,r,0) by (h,t,r), `test` and the validation list (h,t,r,0) by
 * (r,h,t), and the totals behind getTestTotal / getValidTotal / getTripleTotal.  Like importTestFiles it drops the type and
 * ontology lists, marks the typed sampling index stale and starts a new triple-classification generation.  Ontology lists
 * cannot be supplied as arrays: the four arg-min classes of a rank stay 0 / 3 as without ontology_constrain.txt.
 * KGE_ERR_NO_DATASET before a training set; KGE_ERR_BAD_ARG for an id outside [0, entityTotal) / [0, relationTotal) -- the
 * message names the split ("valid" / "test") and the first offending index -- with the previous evaluation state untouched.
 * n_valid == 0 and n_test == 0 are legal.  Option "eval_index_device_min" (default 4194304 triples in the union, the value of
 * "index_device_min" and not measured for this build; 0 = always, negative = never): from that size on, with a device and
 * 2 bits(entityTotal) + bits(relationTotal) <= 64, the lists are built on the device (csrc/eval_build.hip: packed 64-bit keys,
 * radix sorts limited to the bits in use, unpacked into the arrays the kernels read; the training triples come from the device
 * index where it is resident) and the host copies the legacy host routines need are downloaded; below it on the host.  Same
 * arrays bit for bit either way. */
int kge_import_eval_arrays(INT n_valid, const INT *valid_h, const INT *valid_t, const INT *valid_r,
                           INT n_test, const INT *test_h, const INT *test_t, const INT *test_r);

/* The per-relation type lists (importTypeFiles' state) without type_constrain.txt.
 * kge_set_type_lists: the lists as CSR -- head_off / tail_off hold relationTotal + 1 offsets from 0, relation r's list is
 *   ids[off[r] .. off[r+1]).  Copied in, every list sorted, duplicates kept, as importTypeFiles leaves them; the typed sampling
 *   index is stale afterwards.  Offsets that do not start at 0 or decrease, or an id outside [0, entityTotal):
 *   KGE_ERR_BAD_ARG and nothing changes.
 * kge_derive_type_lists: what the reference's n_n() writes on every launch (main_spark.py:209-290): for every relation the
 *   distinct heads and the distinct tails over train + valid + test (the current `all`), each list increasing; a relation
 *   without triples gets two empty lists.  Needs importTestFiles or kge_import_eval_arrays (KGE_ERR_NO_DATASET otherwise).  On
 *   the device from "eval_index_device_min" triples on (keys relation << bits(entityTotal) | entity per side: sort, first of
 *   each equal run, scan, compact, one bound search per relation, written straight into the arrays the rankers read), on the
 *   host below; same arrays bit for bit.
 * kge_have_type_lists: 1 when lists are present (file, arrays or derived), else 0.
 * kge_get_type_lists: the current lists as CSR in increasing relation order (offsets relationTotal + 1 each).  A NULL ids
 *   pointer skips that copy: offsets alone, for sizing.  KGE_ERR_NO_DATASET without lists.
 * kge_write_type_constraints: the current lists in the format Reader.h:317-362 reads: a first line relationTotal, then for
 *   EVERY relation in increasing id a head line and a tail line "rel<TAB>count<TAB>id...", count 0 for a relation without
 *   triples.  This departs from n_n() on purpose: it writes only the relations that occur (in dictionary order), after a first
 *   line that counts them, and the reference's reader then loops relationTotal times over a shorter file.  Written under a
 *   temporary name and renamed into place. */
int kge_set_type_lists(const INT *head_off, const INT *head_ids, const INT *tail_off, const INT *tail_ids);
int kge_derive_type_lists(void);
int kge_have_type_lists(void);
int kge_get_type_lists(INT *head_off, INT *head_ids, INT *tail_off, INT *tail_ids);
int kge_write_type_constraints(const char *path);

/* Copies of the evaluation arrays, for inspection and tests; read from the device copies where a device is usable (uploaded on
 * first use), so a test sees what the kernels see.  `what` is one of
 *   "all" / "all_t" / "all_ht"  int32[tripleTotal][4]  the union as (h,r,t,0) / (t,r,h,0) / (h,t,r,0), each sorted by its fields
 *   "test" / "valid"            int32[testTotal][4] / int32[validTotal][4]  (h,t,r,0) sorted by (r,h,t)
 *   "head_lef" / "head_rig" / "tail_lef" / "tail_rig"  int32[relationTotal]  relation r's list is [lef[r], rig[r]) of
 *   "head_type" / "tail_type"   int32[]  (all zero / empty without type lists)
 * Returns the number of BYTES the array holds (copying at most `bytes` of them), <0 on error. */
int64_t kge_eval_copy(const char *what, void *dst, int64_t bytes);

/* Type-constrained negative sampling for TRAINING (NON-PARITY, off by default; the reference trains on untyped negatives,
 * Corrupt.h:7-69): an entity negative is drawn from the corrupted side's type list of its relation (type_constrain.txt) instead
 * of from all entities.  Nothing about the random stream changes: a positive still consumes 1 + 2*negRate + negRelRate draws,
 * draw 0 picks the training triple, entity negative k uses draw 1 + 2(k-1) as the head-or-tail coin (compared in float with the
 * Bernoulli probability or 500) and the next draw s for the corruption; relation negatives are untouched.  Only how s becomes
 * an id changes.  Coin says "new tail":
 *     L  = the tail type list of r, sorted, duplicates removed
 *     K' = the increasing positions in L of the known tails of (h, r) (training set) that occur in L
 *     c  = |L| - |K'|
 *     c > 0:  tmp = s mod c,  pos = tmp + #{ j : K'[j] - j <= tmp },  new tail = L[pos]
 *     c = 0:  the reference's untyped draw from the same s (no list, an empty list, or a list the known tails exhaust)
 * Coin says "new head": the same with the head type list of r and the known heads of (t, r).  Known ids outside L do not count.
 * So positives, coins, relation negatives and all stream states are bit-identical to the untyped batch, and a typed negative
 * with c > 0 lies in the list and is not a training triple.
 * kge_set_typed_sampling(1) needs type lists -- importTypeFiles, kge_set_type_lists or kge_derive_type_lists -- (error otherwise), runs an armed sampler first (kge_sampling_flush), builds the
 * typed index on the host at once and uploads it with the first batch drawn; importing the training set or the type file again
 * marks it stale (rebuilt on next use).  `sampling`, kge_sampling_device(_packed) and kge_sampling_attach(_packed) honour it; an
 * armed typed sampler rides in no other launch (kge_sampling_flush launches it), and kge_train_steps_persistent refuses while it
 * is on.  kge_typed_sampling: the current setting. */
int kge_set_typed_sampling(INT on);
int kge_typed_sampling(void);

/* rng stream states of the virtual threads (host view; Random.h:6) */
int kge_get_stream_states(uint64_t *dst, INT n);
int kge_set_stream_states(const uint64_t *src, INT n);

/* On-device sampling of the slice of the batch owned by virtual threads [thread_lo, thread_hi)
 * (Base.cpp:85-92 partitions the batch by thread id; a data-parallel rank owns a range of them).
 * d_h/d_t/d_r: DEVICE int32 arrays of length out_stride*(1+negRate+negRelRate); the positive at
 * global batch position p goes to index p - first_position(thread_lo), negative k to that +
 * (k+1)*out_stride.  All workThreads rng streams advance exactly as one reference `sampling`
 * call would advance them, whatever the owned range, so replicas stay in step.
 * *n_local receives the number of positives written (may be NULL). */
int kge_sampling_device(int32_t *d_h, int32_t *d_t, int32_t *d_r, INT batchSize, INT negRate, INT negRelRate,
                        INT thread_lo, INT thread_hi, INT out_stride, INT *n_local, void *stream);

/* The same batch, ARMED instead of launched: the sampler depends on the rng streams and the dataset only, never on the
 * parameters, so the batch of step i+1 can be drawn while step i is being reduced.  The armed sampler rides in the launch of
 * the next kernel of the sign-count / pair-count pipeline that leaves most wave slots idle -- the bucket scatter, one
 * workgroup per CU -- as extra workgroups of that launch: no side stream, no events, no second queue for the command
 * processor to arbitrate (the step is one in-order stream of launches).  kge_sampling_flush launches an armed sampler on its
 * own when the step's path had no such kernel (and is a no-op otherwise); every other sampler entry point, the stream-state
 * accessors and the persistent launch flush it first, so batches are always drawn in order.  The rng streams are accounted
 * as advanced from the moment of the call (Base.cpp:149-172 semantics unchanged: same batches, same order, same bits). */
int kge_sampling_attach(int32_t *d_h, int32_t *d_t, int32_t *d_r, INT batchSize, INT negRate, INT negRelRate,
                        INT thread_lo, INT thread_hi, INT out_stride, INT *n_local, void *stream);
int kge_sampling_flush(void *stream);
/* The same two calls, which ALSO write the batch's packed negatives for the TransE emit kernel: d_pack[(b << kshift) + k], one
 * int32 per slot k of local positive b, kshift = ceil(log2(1 + negRate + negRelRate)) -- bits 0..27 the row the kernel gathers for
 * negative k (the new head, tail or relation id), bits 28..29 which one (0 new head, 1 new tail, 2 new relation), bit 31 set
 * when not exactly one slot differs from the positive; slot 0 and the slots past the last negative are 0.  The word is derived
 * from the very ids written to d_h / d_t / d_r, by the classification the emit kernel itself applies to them.  d_pack holds
 * kge_emit_pack_words(n_local, negRate, negRelRate) words; it is not written when that is 0, or when d_pack is NULL (= the
 * calls above).  Hand the pointer to the _packed step entry point that consumes THIS batch and to no other: the library never
 * guesses a pack from a batch pointer. */
int kge_sampling_device_packed(int32_t *d_h, int32_t *d_t, int32_t *d_r, int32_t *d_pack, INT batchSize, INT negRate, INT negRelRate,
                               INT thread_lo, INT thread_hi, INT out_stride, INT *n_local, void *stream);
int kge_sampling_attach_packed(int32_t *d_h, int32_t *d_t, int32_t *d_r, int32_t *d_pack, INT batchSize, INT negRate, INT negRelRate,
                               INT thread_lo, INT thread_hi, INT out_stride, INT *n_local, void *stream);
/* words of the pack of n_positions positives; 0 = batches of this shape have none (option emit_pack = 0, more than 63 negatives,
 * 2^28 or more entities or relations) or, with dim > 0, a TransE step of that width would not read it (dim = 0: any width) */
INT kge_emit_pack_words(INT n_positions, INT negRate, INT negRelRate, INT dim);
/* number of batch positions owned by virtual threads [thread_lo, thread_hi) for this batchSize */
INT kge_slice_positions(INT batchSize, INT thread_lo, INT thread_hi, INT *first_position);

typedef struct kge_model_desc {
    int32_t model;        /* KGE_TRANSE .. KGE_TRANSD  (distribute_training.py:62-69) */
    int32_t negative_rel; /* Config.negative_rel; TransR reuses the positive's matrix when 0 (TransR.py:57) */
    int64_t ent_total, rel_total;
    int32_t ent_dim, rel_dim; /* TransE/H/D: both = hidden_size (TransD.py:37-40 ignores ent/rel_size) */
    float margin;
    int32_t reserved;
} kge_model_desc;

/* Parameter tables, by the reference's variable names (the checkpoint contract):
 *   [0] ent_embeddings [E,De]  [1] rel_embeddings [R,Dr]
 *   [2] normal_vectors [R,Dr] (TransH) | transfer_matrix [R,De*Dr] (TransR) | rel_transfer [R,Dr] (TransD)
 *   [3] ent_transfer [E,De] (TransD)
 * Dense row-major fp32, no padding. */
#define KGE_MAX_TABLES 4
int kge_table_shape(const kge_model_desc *m, int table, int64_t *rows, int64_t *cols);

/* Fused gather -> score -> margin-ranking loss -> backward for one batch already on the device.
 * Replaces the forward/backward half of sess.run(train_op) for TransE.py:26-51, TransH.py:33-69,
 * TransD.py:46-84, TransR.py:36-75.
 *   d_h,d_t,d_r : DEVICE int32[stride*(1+n_neg)], the Base.cpp:109-139 layout
 *   n_pos       : positives in this (local) batch; n_neg = negative_ent + negative_rel
 *   denom       : the reduce_mean denominator, GLOBAL batch_size*n_neg (TransE.py:51)
 *   grads[i]    : DEVICE fp32 dense accumulators shaped like tables[i]; the summed (deduplicated)
 *                 IndexedSlices gradient is ADDED into them (zero them first; the update ops
 *                 re-zero them)
 *   d_loss      : DEVICE float[1], receives sum(hinge)/denom of this local batch
 */
int kge_forward_backward(const kge_model_desc *m, const float *const tables[KGE_MAX_TABLES],
                         const int32_t *d_h, const int32_t *d_t, const int32_t *d_r,
                         INT n_pos, INT n_neg, INT stride, INT denom,
                         float *const grads[KGE_MAX_TABLES], float *d_loss, void *stream);

/* Makes `stream` wait for the most recent launch of the TransE emit kernel (or of the pair-count path's emit kernel) (option "record_emit_event" = 1 records an event
 * behind every such launch).  Config.prefetch_sampling uses it to start the next batch's sampler on a side stream as soon as the
 * emit kernel -- the one bandwidth-bound kernel of the step -- has finished, so that it runs beside the small latency-bound
 * kernels that follow (bucketing, segmented sum, apply).  Returns KGE_NO_EVENT (and makes `stream` wait for nothing) when no
 * emit launch was recorded since the previous call: the caller then orders `stream` behind the step by an event of its own. */
int kge_stream_wait_emit(void *stream);
/* Forward / backward AND plain SGD on the touched rows only, in place (TransE / TransH / TransD): the step's gradient rows are
 * stored as float records, ordered by destination row, summed by segments and added to their PARAMETER rows as -lr * sum.
 * No gradient tables and no sweep over the tables: for tables whose size, not the batch, would set the step time (the dense
 * form is kge_forward_backward + kge_sgd_update_tables; same update up to fp32 summation order -- GradientDescentOptimizer
 * leaves rows without gradient alone, distribute_training.py:99-101).  Not for Adam: TF1's Adam moves every row.
 * Negatives that are not single-slot corruptions of their positive (the reference's sampler draws no others; a hand-fed batch
 * may hold them) are SKIPPED -- their exact path adds rows atomically, which in place would race with the forward reads -- and
 * counted: kge_sgd_rows_skipped (synchronises); the caller must treat a non-zero count as an error of that step. */
int kge_forward_backward_sgd_rows(const kge_model_desc *m, float *const tables[KGE_MAX_TABLES], const int32_t *d_h, const int32_t *d_t,
                                  const int32_t *d_r, INT n_pos, INT n_neg, INT stride, INT denom, float lr, float *d_loss, void *stream);
int kge_sgd_rows_skipped(int32_t *n_negatives);
/* The same update across N ranks (replaces the per-variable scatter_sub the reference's workers send to the parameter servers,
 * distribute_training.py:99-101,193-196): kge_forward_backward_records stores the gradient rows of THIS rank's slice of the batch
 * as float records (d_rec [*, dim], destination keys d_dst) into its slice [rec_offset, rec_offset + rec_slice) of two buffers the
 * caller owns (unused positions of the slice get key -1), the caller all-gathers the slices, and kge_float_records_apply sums ALL
 * n_records records by destination row and adds -lr * sum to the rows of every replica -- the sparse touched-row exchange; the
 * replicas stay identical because every rank reduces the same records in the same order.  n_pos_total = positives of the GLOBAL
 * batch (it fixes the virtual row space of the keys, which must be the same on all ranks); `denom` the global denominator;
 * d_loss receives this rank's share of the loss.  kge_sgd_rows_skipped applies as above. */
int kge_forward_backward_records(const kge_model_desc *m, const float *const tables[KGE_MAX_TABLES], const int32_t *d_h, const int32_t *d_t,
                                 const int32_t *d_r, INT n_pos, INT n_neg, INT stride, INT denom, INT n_pos_total, float *d_rec,
                                 int32_t *d_dst, INT rec_offset, INT rec_slice, float *d_loss, void *stream);
int kge_float_records_apply(const kge_model_desc *m, float *const tables[KGE_MAX_TABLES], const float *d_rec, int32_t *d_dst, INT n_records,
                            INT n_pos_total, INT n_neg, float lr, void *stream);
/* NON-PARITY, opt-in: the two entry points above ending in LAZY ADAM instead of the add -- the reference trains with TF1's
 * AdamOptimizer, which moves every row of every table each step (distribute_training.py:95-101; kge_adam_update_tables is the
 * parity path).  Here the records are ordered by a stable sort and every destination row's COMPLETE sum (one team per run, record
 * order; the copies of a relation-side row folded in copy order; no atomics) goes through the Adam element rule on that row's
 * value and its moments adam_m / adam_v (one per table of the model, shaped like it), in place: EVERY element of a row that has a
 * record -- elements whose summed gradient is exactly zero decay m and v and move too, as kge_transe_apply_rows_adam_lazy
 * documents -- and no element of a row without one (keys < 0 or beyond the row space carry no record).  No buffer shaped like a
 * table and no pass over one.  The order of every sum is fixed: a step is reproducible bit for bit, and ranks that apply the same
 * records keep bit-identical replicas.  lr_t = lr sqrt(1 - beta2^t) / (1 - beta1^t) from the caller.  TransE / TransH / TransD;
 * TransR: KGE_ERR_UNSUPPORTED.  kge_sgd_rows_skipped applies as above. */
int kge_forward_backward_adam_rows(const kge_model_desc *m, float *const tables[KGE_MAX_TABLES], float *const adam_m[KGE_MAX_TABLES],
                                   float *const adam_v[KGE_MAX_TABLES], const int32_t *d_h, const int32_t *d_t, const int32_t *d_r, INT n_pos,
                                   INT n_neg, INT stride, INT denom, float lr_t, float beta1, float beta2, float eps, float *d_loss, void *stream);
int kge_float_records_apply_adam(const kge_model_desc *m, float *const tables[KGE_MAX_TABLES], float *const adam_m[KGE_MAX_TABLES],
                                 float *const adam_v[KGE_MAX_TABLES], const float *d_rec, int32_t *d_dst, INT n_records, INT n_pos_total,
                                 INT n_neg, float lr_t, float beta1, float beta2, float eps, void *stream);
/* Opt-in ("Adagrad"): the same two entry points ending in TF1's AdagradOptimizer on the touched rows -- per element, in fp32,
 *     if (g != 0) { a += g*g;  p -= lr * g / sqrt(a); }
 * with no epsilon (the caller fills the accumulators `acc` -- one per table of the model, shaped like it -- with a positive
 * value before the first step; TF's default is 0.1) and no step-dependent factor.  Unlike lazy Adam this IS the dense rule: an
 * element with zero gradient keeps its value and its accumulator bit for bit, so updating only the rows that have a record
 * gives the tables kge_adagrad_update_tables gives from the same summed gradient.  g is a row's complete sum (record order,
 * hub copies in copy order), as for lazy Adam; the step is reproducible bit for bit.  A missing accumulator: KGE_ERR_BAD_ARG
 * before anything is launched.  TransE / TransH / TransD; TransR: KGE_ERR_UNSUPPORTED.  kge_sgd_rows_skipped applies as above.
 * `lr` is used as given, here and on kge_transe_apply_rows_adagrad / kge_adagrad_update(_tables): none of the four checks its
 * sign or size, as none of the Adam or SGD entry points does. */
int kge_forward_backward_adagrad_rows(const kge_model_desc *m, float *const tables[KGE_MAX_TABLES], float *const acc[KGE_MAX_TABLES],
                                      const int32_t *d_h, const int32_t *d_t, const int32_t *d_r, INT n_pos, INT n_neg, INT stride, INT denom,
                                      float lr, float *d_loss, void *stream);
int kge_float_records_apply_adagrad(const kge_model_desc *m, float *const tables[KGE_MAX_TABLES], float *const acc[KGE_MAX_TABLES],
                                    const float *d_rec, int32_t *d_dst, INT n_records, INT n_pos_total, INT n_neg, float lr, void *stream);
/* Opt-in ("RowAdagrad"): the same two entry points ending in row-wise Adagrad (PyTorch-BigGraph's RowAdagrad) on the touched rows.
 * ONE fp32 accumulator per table row: `acc` holds, for each table of the model, [rows] floats (not a table-shaped array).  With
 * g[0..D) the row's complete gradient sum (record order, hub copies folded in copy order -- as for lazy Adam and Adagrad), in
 * fp32 with contraction off:
 *     q = sum_j g[j]*g[j];  a += q / D;  s = sqrt(a);  p[j] -= (lr * g[j]) / s  for every j with g[j] != 0
 * q is summed in one fixed order per width (a lane's elements in index order, then the team's butterfly), the same in every run.
 * No epsilon, nothing advances between steps: the caller fills the accumulators with a positive value before the first step
 * (PBG's own form starts at 0 and adds 1e-10 to the root; this keeps the Adagrad entry points' convention).  Like Adagrad it IS
 * the dense rule: a row whose gradient is all zero -- no record, or records of zeros -- keeps its value and its accumulator bit
 * for bit, and so does an element with g = 0 in a row that moves.  A missing accumulator: KGE_ERR_BAD_ARG before anything is
 * launched.  TransE / TransH / TransD; TransR: KGE_ERR_UNSUPPORTED (its form is kge_rowadagrad_update_tables). */
int kge_forward_backward_rowadagrad_rows(const kge_model_desc *m, float *const tables[KGE_MAX_TABLES], float *const acc[KGE_MAX_TABLES],
                                         const int32_t *d_h, const int32_t *d_t, const int32_t *d_r, INT n_pos, INT n_neg, INT stride, INT denom,
                                         float lr, float *d_loss, void *stream);
int kge_float_records_apply_rowadagrad(const kge_model_desc *m, float *const tables[KGE_MAX_TABLES], float *const acc[KGE_MAX_TABLES],
                                       const float *d_rec, int32_t *d_dst, INT n_records, INT n_pos_total, INT n_neg, float lr, void *stream);
/* 1 when kge_forward_backward on a step of this shape takes the TransH / TransD pair-count path (whose emit kernel also records
 * the event above), else 0 */
int kge_pair_path_active(const kge_model_desc *m, INT n_pos, INT n_neg);
/* 1 when kge_forward_backward_sampled on a TransR step of this shape takes the group layout (groups sorted by relation, the
 * vector stage in the projection's epilogue: option "transr_groups"), else 0 -- what the tests of that layout assert */
int kge_transr_group_layout_active(const kge_model_desc *m, INT n_pos, INT n_neg);
/* Host-only, as the two above.  The number of virtual copies of the relation rows that kge_transe_forward_counts /
 * kge_transe_train_step_counts sort a step of n_pos groups over: 1 below 4096 groups, else option "counts_krel" (a power of
 * two, default 4), halved while copies * rel_total > 2 * (ent_total + rel_total). */
INT kge_transe_relation_copies(const kge_model_desc *m, INT n_pos);
/* Records per team of the float-record segmented sum of a step with n_records records: 16, 32 from 2^18, 64 from 2^20 on. */
INT kge_float_records_chunk_len(INT n_records);

/* The same call for a batch the caller KNOWS to be sampler-shaped -- what kge_sampling_device / `sampling` produce
 * (Base.cpp:109-139): every negative differs from its positive in exactly one entity slot, or (negative_rel) in the relation.
 * Paths that route other groups to a separate exact pass (the TransH / TransD pair-count path) then skip that pass and
 * its two bookkeeping launches.  A group that breaks the promise contributes nothing on those paths. */
int kge_forward_backward_sampled(const kge_model_desc *m, const float *const tables[KGE_MAX_TABLES],
                                 const int32_t *d_h, const int32_t *d_t, const int32_t *d_r,
                                 INT n_pos, INT n_neg, INT stride, INT denom,
                                 float *const grads[KGE_MAX_TABLES], float *d_loss, void *stream);

/* The loss of a data-parallel TransE step, carried inside the int32 count image that the step reduce-scatters anyway (one
 * collective less per step): d_limbs4 receives the four 16-bit limbs of llrint(loss * 2^32); after the SUM exchange
 * kge_limbs_to_loss turns the summed limbs back into the summed loss.  Exact integer arithmetic: the result does not depend on
 * the number of ranks or on the reduction order. */
int kge_loss_to_limbs(const float *d_loss, int32_t *d_limbs4, void *stream);
int kge_limbs_to_loss(const int32_t *d_limbs4, float *d_out, void *stream);
/* From now on kge_transe_forward_counts on a device-sampled batch ALSO writes its loss as those four limbs to d_limbs4 (the emit
 * kernel's last workgroup does it: no conversion launch); NULL switches it off.  The pointer must stay valid until then. */
int kge_loss_limbs_target(int32_t *d_limbs4);

/* GradientDescentOptimizer on the summed gradient: p -= lr*g; g = 0   (distribute_training.py:98) */
int kge_sgd_update(float *d_p, float *d_g, int64_t n, float lr, void *stream);
/* TF1 AdamOptimizer._apply_sparse_shared on the summed gradient (distribute_training.py:96): every
 * row decays and moves.  lr_t = lr*sqrt(1-beta2^t)/(1-beta1^t) computed by the caller; g = 0 after. */
int kge_adam_update(float *d_p, float *d_m, float *d_v, float *d_g, int64_t n, float lr_t, float beta1,
                    float beta2, float eps, void *stream);
/* TF1 AdagradOptimizer on the summed gradient: where g != 0, a += g*g; p -= lr * g / sqrt(a); g = 0 after.  Elements (and whole
 * 16-byte groups) with zero gradient are left alone, accumulator included.  Null pointers: KGE_ERR_BAD_ARG, nothing launched. */
int kge_adagrad_update(float *d_p, float *d_acc, float *d_g, int64_t n, float lr, void *stream);

/* The same updates for all tables of a model in ONE launch (n_tables <= KGE_MAX_TABLES; numel[i] elements each) */
int kge_sgd_update_tables(int32_t n_tables, float *const d_p[KGE_MAX_TABLES], float *const d_g[KGE_MAX_TABLES],
                          const INT numel[KGE_MAX_TABLES], float lr, void *stream);
int kge_adam_update_tables(int32_t n_tables, float *const d_p[KGE_MAX_TABLES], float *const d_m[KGE_MAX_TABLES],
                           float *const d_v[KGE_MAX_TABLES], float *const d_g[KGE_MAX_TABLES], const INT numel[KGE_MAX_TABLES],
                           float lr_t, float beta1, float beta2, float eps, void *stream);
int kge_adagrad_update_tables(int32_t n_tables, float *const d_p[KGE_MAX_TABLES], float *const d_acc[KGE_MAX_TABLES],
                              float *const d_g[KGE_MAX_TABLES], const INT numel[KGE_MAX_TABLES], float lr, void *stream);
/* Row-wise Adagrad (the rule above) on dense summed gradients, for TransR: table i has rows[i] rows of row_len[i] elements (a
 * relation's whole De x Dr matrix is ONE row; row_len up to 2^24), d_acc[i] holds rows[i] floats.  One wave per row up to 1024
 * elements, one workgroup per row beyond; the sum of squares loops over the row in a fixed order.  The gradient consumed is
 * zeroed; a row whose gradient is all zero is read once (g) and nothing of it -- p, accumulator, g -- is written.  One launch per
 * table.  Null pointers, a negative row count or a row length outside [1, 2^24]: KGE_ERR_BAD_ARG, nothing launched. */
int kge_rowadagrad_update_tables(int32_t n_tables, float *const d_p[KGE_MAX_TABLES], float *const d_acc[KGE_MAX_TABLES],
                                 float *const d_g[KGE_MAX_TABLES], const INT rows[KGE_MAX_TABLES], const INT row_len[KGE_MAX_TABLES], float lr,
                                 void *stream);

/* ---- TransE sign-count path (exact integer gradients, no fp32 atomics) ----------------------
 * For the L1 score of TransE.py:11-15 the gradient w.r.t. every l2-normalised vector is (1/denom) x an
 * integer vector of signs, so the backward can be carried as exact int32 COUNTS per table row:
 *   counts[(E+R), D]  rows [0,E) = ent_embeddings, rows [E,E+R) = rel_embeddings.
 * kge_transe_forward_counts = gather/score/hinge (as kge_forward_backward) + int8 gradient records +
 * sort-and-sum into `d_counts` (must be zero on entry; kge_transe_apply_counts re-zeroes it).  The
 * counts are order-independent, so a data-parallel all-reduce of them is exact and every replica
 * stays bit-identical.  Negatives that are not sampler-shaped (more than one slot differs from the
 * positive) are differentiated exactly in fp32 into the residual accumulators d_resid_ent [E,D] /
 * d_resid_rel [R,D] (zero on entry, all-zero afterwards for sampler batches).  d_resid_ent = d_resid_rel = NULL
 * is the caller's guarantee that the batch IS sampler-shaped (it came from kge_sampling_device): no deferral
 * bookkeeping, no fp32 pass, and the loss is written by the emit kernel itself.
 * kge_transe_apply_counts: per row g = (1/denom)*inv*(S - x^<x^,S>) + resid (the normalise-backward
 * applied once to the summed counts), then SGD (adam=0, lr) or TF1 Adam (adam=1, lr = lr_t) in place. */
int kge_transe_counts_supported(const kge_model_desc *m, INT n_neg);
int kge_transe_forward_counts(const kge_model_desc *m, const float *d_ent, const float *d_rel, const int32_t *d_h,
                              const int32_t *d_t, const int32_t *d_r, INT n_pos, INT n_neg, INT stride, INT denom,
                              int32_t *d_counts, float *d_resid_ent, float *d_resid_rel, float *d_loss, void *stream);
/* kge_transe_forward_counts on a sampler-shaped batch (no residual tables) with the pack kge_sampling_device_packed /
 * kge_sampling_attach_packed wrote for it (NULL = none): at widths 132..256 (multiples of 4) the emit kernel reads the negatives
 * from it.  Same results, bit for bit. */
int kge_transe_forward_counts_packed(const kge_model_desc *m, const float *d_ent, const float *d_rel, const int32_t *d_h,
                                     const int32_t *d_t, const int32_t *d_r, const int32_t *d_pack, INT n_pos, INT n_neg, INT stride,
                                     INT denom, int32_t *d_counts, float *d_loss, void *stream);
int kge_transe_apply_counts(float *d_p, float *d_m, float *d_v, int32_t *d_counts, float *d_resid, int64_t rows, int32_t dim,
                            INT denom, int32_t adam, float lr, float beta1, float beta2, float eps, void *stream);
/* The whole single-process step of the sign-count path in one call -- what sess.run([train_op, loss, global_step]) does for TransE
 * (distribute_training.py:95-101,282): kge_transe_forward_counts followed by kge_transe_apply_counts_tables, with the middle fused
 * where the shape allows (widths that are multiples of 4, tables that take the bucket sort): the negatives' records shrink to two
 * bits per element, and the rows whose records fit one team are summed in registers and updated right there -- no count image, no
 * second pass -- by the same per-row arithmetic as the apply kernel (bit-identical results; tests/test_gpu_models.py).  Longer
 * rows, relation rows and rows without records go through `d_counts` (zero on entry, zero on return) and one apply launch.
 * sampler_shaped = 1: the batch came from kge_sampling_device (no deferral bookkeeping, no fp32 pass, d_resid tables not read);
 * 0: any batch, d_resid [E,D] / [R,D] (zero on entry and return) take the exact fp32 gradients of groups that are not
 * sampler-shaped.  d_m / d_v may be NULL for SGD (adam = 0, lr); Adam (adam = any other value): lr = lr_t.  `adam` is a yes / no
 * flag on this and on the kge_transe_apply_counts* entry points: the dense forms have these two rules only (Adagrad's is the
 * row-list form, kge_transe_apply_rows_adagrad). */
int kge_transe_train_step_counts(const kge_model_desc *m, float *const d_p[2], float *const d_m[2], float *const d_v[2], const int32_t *d_h,
                                 const int32_t *d_t, const int32_t *d_r, INT n_pos, INT n_neg, INT stride, INT denom, int32_t *d_counts,
                                 float *const d_resid[2], int32_t sampler_shaped, int32_t adam, float lr, float beta1, float beta2, float eps,
                                 float *d_loss, void *stream);
/* the same with the batch's pack (see kge_sampling_device_packed; NULL = none, and ignored unless sampler_shaped = 1) */
int kge_transe_train_step_counts_packed(const kge_model_desc *m, float *const d_p[2], float *const d_m[2], float *const d_v[2],
                                        const int32_t *d_h, const int32_t *d_t, const int32_t *d_r, const int32_t *d_pack, INT n_pos,
                                        INT n_neg, INT stride, INT denom, int32_t *d_counts, float *const d_resid[2],
                                        int32_t sampler_shaped, int32_t adam, float lr, float beta1, float beta2, float eps, float *d_loss,
                                        void *stream);
/* both tables ([0] = ent_embeddings, [1] = rel_embeddings; d_counts = the whole [(E+R), D] image) in one launch */
int kge_transe_apply_counts_tables(const kge_model_desc *m, float *const d_p[2], float *const d_m[2], float *const d_v[2],
                                   int32_t *d_counts, float *const d_resid[2], INT denom, int32_t adam, float lr, float beta1,
                                   float beta2, float eps, void *stream);

/* the same on the row range [row_lo, row_hi) of the [(E+R), D] row space only; d_counts_chunk = the count image OF THAT RANGE
 * (a data-parallel rank's reduce-scattered chunk): owner-computes update, replaces the replicated optimizer sweep */
int kge_transe_apply_counts_range(const kge_model_desc *m, float *const d_p[2], float *const d_m[2], float *const d_v[2],
                                  int32_t *d_counts_chunk, float *const d_resid[2], INT row_lo, INT row_hi, INT denom, int32_t adam,
                                  float lr, float beta1, float beta2, float eps, void *stream);

/* ---- TransE sign-count path, stage level: for tables too large for a dense count image and for the
 * multi-GPU exchange, where the int8 records (8x smaller than fp32 gradient rows) are the wire format ----
 *   kge_transe_record_dwords : dwords per record for this embedding width
 *   kge_transe_emit_records  : stage 1 into CALLER buffers d_rec [n_pos*(3+n_neg), dwords], d_dst [n_pos*(3+n_neg)]
 *                              (destination row in the [0,E)+[E,E+R) row space, -1 = no record)
 *   kge_transe_reduce_records: order any number of records (e.g. all ranks' records after an all-gather) by
 *                              destination and sum them into a COMPACT image: d_rows[i] = touched row,
 *                              d_row_counts[i, D] = its int32 count vector, *d_n_rows = how many (device scalar);
 *                              buffers sized for n_records rows; d_dst is overwritten
 *   kge_transe_apply_rows_sgd: SGD on the touched rows only (same arithmetic as kge_transe_apply_counts)
 *   kge_transe_deferred_groups: groups of the last emit whose negatives were not sampler-shaped (each negative
 *                              differing from its positive in exactly one slot).  With residual accumulators they
 *                              were handled by the fp32 path; with d_resid_* == NULL they were SKIPPED and the
 *                              caller must treat a non-zero count as an error.  Synchronises.
 *   kge_transe_step_scratch_read: test hook.  Copies `count` 32-bit words from word `offset` of the engine-owned buffers the
 *                              last kge_transe_forward_counts / kge_transe_train_step_counts call wrote to the host:
 *                              which = 0 the records (3 * n_pos int8 records of kge_transe_record_dwords words each, then --
 *                              the fused step at widths that are multiples of 4 -- the 2-bit record of negative k of group b
 *                              as record k * n_pos + b of a quarter of that size), which = 1 the destination keys as the
 *                              call left them (inactive slots hold its sentinel, the largest key), always in slot-major order
 *                              (word s * n_pos + b) whichever layout the step kept them in, which = 2 the emit kernel's table of
 *                              1/|row| (entity rows, then relation rows; fp32 words).  Synchronises.
 *   kge_counts_sort_test:      test hook.  Runs the hand-written record sort (option "counts_sort_tiles") on `stream` over the n_keys
 *                              HOST keys `keys` (a key < 0 = no record, else < rows), buckets of rpb rows (rows <= 512 * rpb,
 *                              rpb <= 8192), and copies back: sorted_keys / sorted_ids [n_keys] (the first *n_live entries are
 *                              meaningful), n_live [1], bucket_start [514] (start of each of the 512 buckets, [512] = *n_live,
 *                              [513] = n_keys).  plan_cap > 0 (rpb even: key = 2 * row + kind) also builds the fused step's plan with
 *                              lists cut at plan_cap records: row_span [rows][2] = (first position, records) of every key, pieces
 *                              [max_pieces][4] = (key, first position, records, 0), n_pieces [1] (an error when it exceeds
 *                              max_pieces).  Synchronises. */
INT kge_transe_record_dwords(const kge_model_desc *m);
int kge_transe_deferred_groups(int32_t *n_groups);
int kge_transe_step_scratch_read(int which, INT offset, INT count, void *host_out);
int kge_counts_sort_test(const int32_t *keys, INT n_keys, INT rows, INT rpb, INT plan_cap, int32_t *sorted_keys, int32_t *sorted_ids,
                         int32_t *n_live, int32_t *bucket_start, int32_t *row_span, int32_t *pieces, INT max_pieces, int32_t *n_pieces,
                         void *stream);
int kge_transe_emit_records(const kge_model_desc *m, const float *d_ent, const float *d_rel, const int32_t *d_h, const int32_t *d_t,
                            const int32_t *d_r, INT n_pos, INT n_neg, INT stride, INT denom, uint32_t *d_rec, int32_t *d_dst,
                            float *d_resid_ent, float *d_resid_rel, float *d_loss, void *stream);
int kge_transe_reduce_records(const kge_model_desc *m, const uint32_t *d_rec, int32_t *d_dst, INT n_records, int32_t *d_rows,
                              int32_t *d_row_counts, int32_t *d_n_rows, void *stream);
int kge_transe_apply_rows_sgd(const kge_model_desc *m, float *d_ent, float *d_rel, const int32_t *d_rows, const int32_t *d_row_counts,
                              const int32_t *d_n_rows, INT max_rows, INT denom, float lr, void *stream);
/* NON-PARITY, opt-in ("LazyAdam"): Adam on the touched rows only -- m = b1 m + (1-b1) g, v = b2 v + (1-b2) g^2,
 * p -= lr_t m / (sqrt(v) + eps) for the rows listed in d_rows (every element of a listed row, zero gradients included), all
 * other rows and their moments left alone: tf.contrib.opt.LazyAdamOptimizer's rule, NOT what the reference trains with (TF1's
 * AdamOptimizer moves every row of the table every step, distribute_training.py:96 -- kge_transe_apply_counts / kge_adam_dense
 * are the parity path).  For tables whose dense sweep (32 bytes per element per step) would dominate the step.  lr_t =
 * lr sqrt(1 - b2^t) / (1 - b1^t) with the global step t, computed by the caller.
 * d_row_live: null = every listed row; else int32[max_rows], listed row i is processed only where d_row_live[i] != 0.  For the
 * table-sharded data-parallel step: the replicated relation rows are listed in full with their all-reduced counts, and a
 * relation for which NO rank had a record must keep its row and moments (the lazy rule). */
int kge_transe_apply_rows_adam_lazy(const kge_model_desc *m, float *d_ent, float *d_rel, float *d_m_ent, float *d_m_rel, float *d_v_ent,
                                    float *d_v_rel, const int32_t *d_rows, const int32_t *d_row_counts, const int32_t *d_n_rows,
                                    INT max_rows, INT denom, float lr_t, float beta1, float beta2, float eps,
                                    const int32_t *d_row_live, void *stream);
/* Opt-in ("Adagrad"): TF1's AdagradOptimizer on the rows listed in d_rows, from their counts -- the row's gradient g is formed as
 * the lazy-Adam call forms it, then per element: if (g != 0) { a += g*g; p -= lr * g / sqrt(a); }.  d_acc_ent / d_acc_rel are the
 * accumulator tables, shaped like the parameter tables.  Rows that are not listed, listed rows whose counts are all zero and
 * elements whose gradient is zero keep value and accumulator bit for bit -- so no live mask is needed where all rows of a table
 * are listed with all-reduced counts, and the touched rows are all the dense rule would move. */
int kge_transe_apply_rows_adagrad(const kge_model_desc *m, float *d_ent, float *d_rel, float *d_acc_ent, float *d_acc_rel, const int32_t *d_rows,
                                  const int32_t *d_row_counts, const int32_t *d_n_rows, INT max_rows, INT denom, float lr, void *stream);
/* Opt-in ("RowAdagrad"): row-wise Adagrad (see kge_forward_backward_rowadagrad_rows) on the rows listed in d_rows, from their
 * counts -- the row's gradient g is formed as kge_transe_apply_rows_adagrad forms it (same team shape, same bits), then
 * q = sum g^2; a += q / D; p[j] -= (lr * g[j]) / sqrt(a) where g[j] != 0.  d_acc_ent / d_acc_rel hold ONE float per row ([E] and
 * [R]).  Rows that are not listed and listed rows whose counts are all zero keep value and accumulator bit for bit, so no live
 * mask is needed where all rows of a table are listed with all-reduced counts.  A kernel of its own: the SGD / lazy-Adam /
 * Adagrad row-list launch is untouched. */
int kge_transe_apply_rows_rowadagrad(const kge_model_desc *m, float *d_ent, float *d_rel, float *d_acc_ent, float *d_acc_rel, const int32_t *d_rows,
                                     const int32_t *d_row_counts, const int32_t *d_n_rows, INT max_rows, INT denom, float lr, void *stream);
/* reduce + apply in one pass (embedding width a multiple of 4): rows whose records all fall inside one 64-record chunk
 * of the sorted list are updated straight from the registers that hold their sum; only chunk-boundary rows go through
 * d_row_counts and a second, small pass.  Same bits as kge_transe_reduce_records + kge_transe_apply_rows_sgd.
 * d_rows / *d_n_rows as there; d_row_counts is only meaningful for the boundary rows afterwards. */
int kge_transe_reduce_apply_records_sgd(const kge_model_desc *m, const uint32_t *d_rec, int32_t *d_dst, INT n_records, float *d_ent,
                                        float *d_rel, int32_t *d_rows, int32_t *d_row_counts, int32_t *d_n_rows, INT denom, float lr,
                                        void *stream);

/* ---- bf16 table storage (NON-PARITY, opt-in: Config.set_table_dtype("bf16"); csrc/bf16_tables.hip) ----
 * TransE's two tables are STORED as bf16 -- there is no fp32 copy beside them -- and trained by the one-rank int8-record
 * touched-rows step (emit -> kge_transe_reduce_records -> apply) with SGD or row-wise Adagrad.  Every gather and every
 * touched-row update moves half the bytes, and a table takes half the memory.  With the mode off nothing changes.
 *
 * Storage.  [E, D] and [R, D], dense row-major, one uint16 per element: the top 16 bits of the fp32 pattern.  D % 8 == 0 and
 *   D <= 1024, so rows are 16-byte aligned; other widths are refused with the reason (KGE_ERR_UNSUPPORTED).
 * Forward / backward.  A stored value is widened exactly (bits << 16).  From there the arithmetic is kge_transe_emit_records'
 *   without the inverse-norm table: the norms come from the gathered rows in fp32, 1 / sqrt(max(sum x^2, 1e-12)) (eps inside the
 *   max), e = fma(f, x, B) against the group's constants, sign(0) = 0, a hinge tie is active.  Records, keys, loss and the deferral
 *   of groups that are not sampler-shaped have that call's format: byte e of a record is element e, records are
 *   kge_transe_record_dwords words apart (bytes from D on are not written), key -1 = no record, entity e -> e, relation r -> E + r.
 *   kge_transe_reduce_records therefore serves unchanged and kge_transe_deferred_groups reports the deferred groups.  The order
 *   of the fp32 sums differs from kge_transe_emit_records' (another team shape): scores agree to rounding, the loss to 1e-5.
 *   1 to 127 negatives; a positive's int8 sums hold 2 x 63 signs, so a group with MORE than 63 ACTIVE negatives is deferred as well
 *   (keys -1, counted, nothing added to the loss) rather than written wrapped.
 * Update.  A listed row's gradient g is formed from its int32 counts exactly as kge_transe_apply_rows_rowadagrad forms it (same
 *   team shape, same operations: normalise, then unit * inv * (s - d * x^) with every operation rounded on its own), with the
 *   widened row as x.  SGD: y = x - lr * g.  RowAdagrad: q = sum g^2; a += q / D; y = x - (lr * g) / sqrt(a), the accumulators
 *   fp32, one per row, as in kge_transe_apply_rows_rowadagrad.  y is an fp32 value and is stored by stochastic rounding.
 * Stochastic rounding.  All arithmetic mod 2^64, mix = splitmix64's finaliser and G = 0x9E3779B97F4A7C15 (csrc/mix_dev.hpp):
 *     k      = mix(seed + G * (step + 1))                      step: global step of the update, 0 for the first
 *     z      = mix(k + G * (key * (D / 4) + (j >> 2) + 1))     key: the row in the record row space; j: the column
 *     rnd    = (z >> (16 * (j & 3))) & 0xFFFF
 *     stored = exponent(y) all ones ? bits(y) >> 16 : (bits(y) + rnd) >> 16
 *   One mix serves four columns.  The expected stored value is y (a plain down-cast would drop almost every update: one step
 *   moves an element by far less than a bf16 ulp).  A value that is already a bf16 value is stored unchanged whatever rnd is, so
 *   elements with zero gradient, rows that are not listed, and listed rows whose counts are all zero (their accumulators too)
 *   keep their bits.  inf stays inf and a NaN whose top mantissa bits are set stays a NaN.  The stored bits depend on (seed,
 *   step, key, column, y) only: a run is reproducible bit for bit and a resumed run equals the uninterrupted one.
 *
 * kge_bf16_tables_supported: 1 when the descriptor and negative count can take the mode, else 0.
 * kge_transe_emit_records_bf16: kge_transe_emit_records' arguments with bf16 tables and no residual pointers.
 * kge_transe_apply_rows_sgd_bf16 / kge_transe_apply_rows_rowadagrad_bf16: their fp32 namesakes' arguments plus seed and step.
 * kge_bf16_round_stochastic: test hook -- the rounding rule alone on d_y [rows, D] fp32 -> d_out [rows, D] uint16, row i under
 *   the key first_key + i (D % 8 == 0, D <= 1024). */
int kge_bf16_tables_supported(const kge_model_desc *m, INT n_neg);
int kge_transe_emit_records_bf16(const kge_model_desc *m, const uint16_t *d_ent, const uint16_t *d_rel, const int32_t *d_h, const int32_t *d_t,
                                 const int32_t *d_r, INT n_pos, INT n_neg, INT stride, INT denom, uint32_t *d_rec, int32_t *d_dst,
                                 float *d_loss, void *stream);
int kge_transe_apply_rows_sgd_bf16(const kge_model_desc *m, uint16_t *d_ent, uint16_t *d_rel, const int32_t *d_rows, const int32_t *d_row_counts,
                                   const int32_t *d_n_rows, INT max_rows, INT denom, float lr, uint64_t seed, uint64_t step, void *stream);
int kge_transe_apply_rows_rowadagrad_bf16(const kge_model_desc *m, uint16_t *d_ent, uint16_t *d_rel, float *d_acc_ent, float *d_acc_rel,
                                          const int32_t *d_rows, const int32_t *d_row_counts, const int32_t *d_n_rows, INT max_rows, INT denom,
                                          float lr, uint64_t seed, uint64_t step, void *stream);
int kge_bf16_round_stochastic(const float *d_y, INT rows, INT D, INT first_key, uint64_t seed, uint64_t step, uint16_t *d_out, void *stream);

/* ---- TransE on negatives SHARED by a chunk of positives (NON-PARITY, opt-in; csrc/shared_neg.hip) ----
 * The reference draws every negative for one positive (Base.cpp:109-139).  Here a chunk of P consecutive positives scores the
 * same N candidate entities, as large-scale trainers do (PyTorch-BigGraph, DGL-KE): a chunk gathers 3 P + N table rows instead
 * of P (3 + N), and the P x N distances are formed on chip.  The records are kge_transe_emit_records' records, so the reduce and
 * apply stages above serve unchanged.
 *   Chunks.     The positives at batch positions [j P, min((j + 1) P, n_pos)) form chunk j; n_chunks = ceil(n_pos / P), the last
 *               may be short.  1 <= P <= 127: a candidate's count lies within +-P.  1 <= N <= 63: a positive's h-side or t-side
 *               count lies within +-2N.  Both make the counts fit the int8 record.
 *   Candidates. All arithmetic mod 2^64; mix(z) is the finaliser of KGE_RANKC_DRAWN below (csrc/mix_dev.hpp): z = (z ^ z >> 30) *
 *               0xBF58476D1CE4E5B9; z = (z ^ z >> 27) * 0x94D049BB133111EB; z ^= z >> 31.  G = 0x9E3779B97F4A7C15.
 *                   step key          S  = mix(seed + (step + 1) * G)
 *                   candidate k of chunk j:  z = mix(S + (((j << 8) | k) + 1) * G),   id = ((z >> 32) * ent_total) >> 32
 *               Drawn with replacement: a repeated id counts every time.
 *   Side.       Of the pair (batch position p, candidate k): z = mix(S + (((p << 8) | 128 | k) + 1) * G), v = ((z >> 32) * 1000) >> 32.
 *               v takes the place of the draw `rand % 1000` in the head-or-tail comparison of Base.cpp:118: (float)v < 500.0f, or
 *               < the relation's Bernoulli value with setBern(1), means a new TAIL (side 0), else a new HEAD (side 1).
 *   Mask.       A pair is masked exactly when its corrupted triple -- (h, r, c) for a new tail, (c, r, t) for a new head -- is a
 *               training triple; that includes c equal to the entity it replaces.
 *   Loss.       loss = (1 / denom) * sum over the unmasked pairs of max(p_score - n_score + margin, 0), scores sum |h^ + r^ - t^| over
 *               l2-normalised rows (TransE.py:11-15), denom = batch_size * N.  Masked pairs contribute zero and stay in the
 *               denominator.  A hinge tie is active and sign(0) = 0, as in kge_transe_emit_records.
 * kge_shared_negatives_draw: one launch.  d_h / d_t / d_r: the n_pos positives (DEVICE int32); first_position: the batch position
 *   of the first of them, a multiple of P (chunk j of the call is chunk first_position / P + j of the batch).  Writes d_cand
 *   (int32 [n_chunks][N]) and d_pair (uint8 [n_pos][N]: bit 0 = side, bit 1 = masked).  The mask is looked up in the sampler's
 *   sorted lists -- the known tails of (h, r), the known heads of (t, r) -- by the sampler's bisection; the lists of a positive
 *   are found by the same bisection in a directory of the groups' keys taken from the index's group records (the sampler finds
 *   them through the training triple it picked, which the ids alone do not name).  A positive whose (h, r) / (t, r) has no
 *   training triple masks nothing on that side.  ent_total, the Bernoulli values and setBern are the imported training set's.
 * kge_transe_emit_records_shared: gather / score / hinge of the chunks against the lists in d_cand / d_pair (inputs: any lists,
 *   not only drawn ones) and 3 n_pos + n_chunks N records in kge_transe_emit_records' format (kge_transe_record_dwords words
 *   each, keys in the [0, E) + [E, E + R) row space, -1 = no record): record s * n_pos + b for slot s = 0 / 1 / 2 (h / t / r) of
 *   positive b, then record 3 n_pos + j N + k for candidate k of chunk j.  A candidate without an active pair has key -1; so has an
 *   h, t or r slot whose count vector is all zero.  An id outside [0, ent_total) in d_cand is masked for every pair; a positive
 *   with an id outside its table takes no part.  d_h / d_t / d_r hold n_pos positives (`stride` >= n_pos is the arrays' length
 *   and otherwise unused); d_loss receives the loss of this call's positives.  The norms are computed from the gathered rows.
 *   KGE_ERR_UNSUPPORTED, with a message: another model, negative_rel != 0, P or N outside their ranges, a shape outside
 *   kge_transe_counts_supported, an embedding width above 512 (the kernel's LDS tiles).
 * A SLICE of the batch (a rank's share on more than one rank: a range of the sampler's virtual threads, not of chunks).  Chunk
 *   membership is a property of the GLOBAL batch position: position p belongs to chunk p / P.  A call that covers the positions
 *   [first, first + n_pos) meets the chunks c0 = first / P .. c1 = (first + n_pos - 1) / P, n_chunks = c1 - c0 + 1 of them; the
 *   first and the last may be partial.  The two `_at` entry points take any first_position >= 0 and otherwise the arguments, the
 *   checks and the refusals of the two above:
 * kge_shared_negatives_draw_at: d_cand[j][k] = candidate k of global chunk c0 + j (int32 [n_chunks][N]); d_pair[b][k] = side and mask
 *   of global position first_position + b.  Every value is what ONE draw of the whole batch writes for that chunk or position.
 * kge_transe_emit_records_shared_at: workgroup j handles the call's positions that lie in global chunk c0 + j, against row j of
 *   d_cand.  Records as above with the call's own counts: s * n_pos + b for slot s of the call's positive b, then 3 n_pos + j N + k
 *   for candidate k of the call's j-th chunk -- 3 n_pos + n_chunks N records.  A partial chunk's candidate records hold the signs
 *   of the call's own pairs only (counts within +-P as ever); summed per destination key over the calls that cover a batch they
 *   are the whole-batch call's sums.  With first_position a multiple of P the records, keys and loss are those of
 *   kge_transe_emit_records_shared bit for bit.  d_loss: this call's hinge sum / denom (denom: the whole batch's). */
int kge_shared_negatives_draw(const int32_t *d_h, const int32_t *d_t, const int32_t *d_r, INT n_pos, INT first_position, INT P, INT N,
                              uint64_t seed, INT step, int32_t *d_cand, uint8_t *d_pair, void *stream);
int kge_transe_emit_records_shared(const kge_model_desc *m, const float *d_ent, const float *d_rel, const int32_t *d_h, const int32_t *d_t,
                                   const int32_t *d_r, INT n_pos, INT stride, INT P, const int32_t *d_cand, INT N, const uint8_t *d_pair,
                                   INT denom, uint32_t *d_rec, int32_t *d_dst, float *d_loss, void *stream);
int kge_shared_negatives_draw_at(const int32_t *d_h, const int32_t *d_t, const int32_t *d_r, INT n_pos, INT first_position, INT P, INT N,
                                 uint64_t seed, INT step, int32_t *d_cand, uint8_t *d_pair, void *stream);
int kge_transe_emit_records_shared_at(const kge_model_desc *m, const float *d_ent, const float *d_rel, const int32_t *d_h, const int32_t *d_t,
                                      const int32_t *d_r, INT n_pos, INT stride, INT first_position, INT P, const int32_t *d_cand, INT N,
                                      const uint8_t *d_pair, INT denom, uint32_t *d_rec, int32_t *d_dst, float *d_loss, void *stream);

/* ---- Shared negatives on RELATION-GROUPED chunks, with typed candidates (NON-PARITY, opt-in; csrc/shared_neg.hip) ----
 * A chunk of consecutive batch positions mixes relations, so its candidates cannot come from one relation's type list.  Here the
 * step's positives are ordered by relation and a chunk never crosses a relation boundary (PyTorch-BigGraph's way).  mix, G and the
 * step key S = mix(seed + (step + 1) G) are those of the definition above.
 *   Order.      The n_pos positives are drawn as ever (the sampler at negRate = 0).  perm is the STABLE order of the batch positions
 *               by relation id; an id outside [0, rel_total) sorts as rel_total -- one trailing run, whose positives take no part.
 *               Sorted position b holds batch position perm[b].
 *   Chunks.     The run of relation rho is cut from its start into pieces of P positions, the last piece of a run may be short;
 *               chunk j counts the pieces in sorted order.  n_chunks = sum over rho of ceil(len_rho / P) <= cap = ceil(n_pos / P) +
 *               min(rel_total + 1, n_pos).  The chunk table is int2 [cap] = (first sorted position, length); the slots from
 *               n_chunks on have length 0 (and first position n_pos).  n_chunks stays on the device: every launch and buffer is
 *               sized by cap, and the step gains no host synchronisation.
 *   Side.       Per CANDIDATE, not per pair (a typed candidate is drawn from one side's list): of candidate k of chunk j,
 *               v = ((mix(S + (((j << 8) | 128 | k) + 1) G) >> 32) * 1000) >> 32; a new TAIL iff (float)v < bern_prob[rho_j] with
 *               setBern(1) and rho_j valid, else iff (float)v < 500.0f.  Every positive of the chunk meets candidate k on that side.
 *   Id.         u = mix(S + (((j << 8) | k) + 1) G) >> 32.  Typed, rho_j valid: L = the side's type list of rho_j in the typed index
 *               (type_tails / type_heads / type_bounds: sorted, duplicates removed); |L| > 0: id = L[(u |L|) >> 32].  Otherwise --
 *               untyped, a relation without a list, an empty list -- id = (u ent_total) >> 32.  Drawn with replacement.
 *   Mask, loss, records.  As above: a pair is masked exactly when its corrupted triple is a training triple (that includes the
 *               candidate equal to the entity it replaces); loss = (1 / (batch_size N)) sum over the unmasked pairs, masked pairs
 *               stay in the denominator; a hinge tie is active, sign(0) = 0.  pair[b][k] = side_k | (masked ? 2 : 0), b the SORTED
 *               position.  Records in kge_transe_emit_records' format: record s * n_pos + b is slot s (h / t / r) of sorted
 *               position b, record 3 n_pos + j N + k candidate k of chunk j -- 3 n_pos + cap N records; the candidate keys of an
 *               unused chunk slot are -1.  1 <= P <= 127, 1 <= N <= 63.
 * kge_shared_chunk_cap: the bound `cap` above (host only).
 * kge_shared_order_by_relation: d_perm (int32 [n_pos]), the ids in sorted order d_h2 / d_t2 / d_r2 (d_r2 keeps the ids as given),
 *   d_chunks (int2 [cap] as int32 pairs, cap = kge_shared_chunk_cap(n_pos, P, rel_total of the imported training set)) and
 *   d_n_chunks (int32 [1]).  A stable radix sort of the clamped relation ids (rocPRIM), a max-scan of the run starts, a plus-scan of
 *   the chunk starts; the engine itself has no size branch here.  Needs an imported training set (its rel_total).
 * kge_shared_negatives_draw_grouped: d_cand (int32 [cap][N]; -1 in unused slots) and d_pair (uint8 [n_pos][N]) of a table -- the
 *   ordering stage's, or any table whose used slots come first and in position order.  A thread per pair and per candidate; a pair
 *   finds its chunk by bisection in the table, its mask by the bisection of kge_shared_negatives_draw.  typed != 0 draws from the
 *   type lists and fails with type-constrained sampling's own error when none are imported, set or derived.
 * kge_transe_emit_records_shared_chunks: kge_transe_emit_records_shared with workgroup j reading (first position, length) from
 *   d_chunks[j] instead of computing them from j and P; cap workgroups, 3 n_pos + cap N records.  A slot of length 0 (or one that
 *   points outside [0, n_pos)) writes its N candidate keys as -1 and a zero loss partial.  The loss partials are summed over all
 *   cap slots in index order.  A table that states fixed chunks of P gives kge_transe_emit_records_shared's records, keys and loss
 *   bit for bit.  Same refusals (there is no P to refuse; a chunk longer than 127 is the caller's error). */
INT kge_shared_chunk_cap(INT n_pos, INT P, INT rel_total);
int kge_shared_order_by_relation(const int32_t *d_h, const int32_t *d_t, const int32_t *d_r, INT n_pos, INT P, int32_t *d_perm, int32_t *d_h2,
                                 int32_t *d_t2, int32_t *d_r2, int32_t *d_chunks, int32_t *d_n_chunks, void *stream);
int kge_shared_negatives_draw_grouped(const int32_t *d_h2, const int32_t *d_t2, const int32_t *d_r2, INT n_pos, const int32_t *d_chunks, INT cap,
                                      INT N, INT typed, uint64_t seed, INT step, int32_t *d_cand, uint8_t *d_pair, void *stream);
int kge_transe_emit_records_shared_chunks(const kge_model_desc *m, const float *d_ent, const float *d_rel, const int32_t *d_h2, const int32_t *d_t2,
                                          const int32_t *d_r2, INT n_pos, INT stride, const int32_t *d_chunks, INT cap, const int32_t *d_cand, INT N,
                                          const uint8_t *d_pair, INT denom, uint32_t *d_rec, int32_t *d_dst, float *d_loss, void *stream);

/* ---- In-chunk candidates (NON-PARITY, opt-in; csrc/shared_neg.hip) ----
 * Batch negatives (PyTorch-BigGraph's num_batch_negs, DGL-KE's neg_deg_sample): beside the N DRAWN candidates of a relation-grouped
 * chunk, K more are the entities of the chunk's own positives.  They are sampled by the data distribution and, on chunks of one
 * relation, type-consistent by construction.  The order, the chunk table, cap, S, mix, G, the drawn candidates, their sides and
 * their masks are those of "Shared negatives on RELATION-GROUPED chunks"; none of them changes.
 * N = the drawn candidates per chunk, K >= 0 the in-chunk ones, Nt = N + K.  A used chunk slot j = (first_j, len_j) of relation
 * rho_j has Nt candidate columns:
 *   Columns k < N.       The section above's candidate and side: the same hash keys, the same bits for every K.
 *   Columns k = N + i, 0 <= i < K.
 *     Side.       The per-candidate formula above with this k: v = ((mix(S + (((j << 8) | 128 | k) + 1) G) >> 32) * 1000) >> 32,
 *                 the same Bernoulli / 500 comparison (k <= 62: the key space reserved for sides).
 *     Rotation.   o_j = ((mix(S + (((j << 8) | 64) + 1) G) >> 32) * len_j) >> 32.  No candidate key (k <= 62) and no side key
 *                 (>= 128) has the low byte 64.
 *     Id.         i < len_j: q = first_j + ((o_j + i) mod len_j); the id is t2[q] for a new tail, h2[q] for a new head.
 *                 i >= len_j: the id is -1 and every pair of the column is masked.  The type lists are not consulted.
 *     Trailing run.  A slot whose relation lies outside [0, rel_total) has its K in-chunk ids at -1 and their pairs masked; its
 *                 drawn columns stay what the section above makes them, and its positives take no part, as ever.
 *   Mask of an in-chunk pair (b, k): the lookup above (the corrupted triple is a training triple), OR the candidate id equals
 *                 the entity it replaces -- t2[b] for a new tail, h2[b] for a new head.  The second rule is for in-chunk columns
 *                 alone: a hand-fed positive that is not a training triple does not score against itself.
 *   Unused slots have all Nt ids at -1.
 *   Loss, records.  The section above's with Nt for N: the denominator is batch_size Nt, masked pairs and -1 columns stay in it.
 *                 TransE 3 n_pos + cap Nt records, TransH 2 n_pos + cap (Nt + 2), TransD 4 n_pos + cap (2 Nt + 2), TransR
 *                 2 n_pos + cap Nt rows through the GEMMs.  Every emit entry point is called with Nt where it took N and with the
 *                 wider lists; a candidate id outside the table is masked for every pair in all of them (TransR projects row 0 in
 *                 its place and gives it no gradient).  The K rows are gathered again, not re-used from the positives on chip.
 *   Limit.      1 <= N, 0 <= K, N + K <= 63: a positive's sign count lies within +-2 Nt <= 126; a candidate's within +-P as before
 *                 (an in-chunk candidate meets at most P positives), so the LDS byte fields still see at most 2 P.
 * kge_shared_negatives_draw_grouped_mixed: d_cand (int32 [cap][N + K]) and d_pair (uint8 [n_pos][N + K]) of a table, by a sibling of
 *   the grouped draw kernel (a thread per pair and per candidate, no LDS, no scratch): a pair thread of an in-chunk column has its
 *   slot from the bisection, hashes o_j and gathers one more id.  K = 0 IS kge_shared_negatives_draw_grouped, bit for bit. */
int kge_shared_negatives_draw_grouped_mixed(const int32_t *d_h2, const int32_t *d_t2, const int32_t *d_r2, INT n_pos, const int32_t *d_chunks,
                                            INT cap, INT N, INT K, INT typed, uint64_t seed, INT step, int32_t *d_cand, uint8_t *d_pair,
                                            void *stream);

/* ---- Shared negatives on bf16 tables (NON-PARITY, opt-in; csrc/shared_neg.hip, the shared emit kernel under BF16) ----
 * The two sections "bf16 table storage" and "TransE on negatives SHARED by a chunk of positives" together: the tables are stored
 * as bf16 and a chunk gathers 3 P + N rows of them, each half as long.
 *   Definition. `kge_transe_emit_records_shared[_chunks]` on the exactly widened tables, bit for bit -- records, keys and loss.
 *   (A lane reads its four elements 4 (l + 64 q) .. + 3 in one 8-byte load and widens them, bits << 16; from there the kernel is
 *   the fp32 one: same lane-to-element map, same order of every fp32 sum.)  The draw, order and in-chunk kernels work on ids and
 *   serve unchanged, kge_transe_reduce_records takes the records, and kge_transe_apply_rows_sgd_bf16 /
 *   kge_transe_apply_rows_rowadagrad_bf16 the row lists it makes.
 *   Refused (KGE_ERR_UNSUPPORTED, with the reason): a model other than TransE, negative_rel != 0, N outside 1..63, a width that is
 *   not a multiple of 8 (rows are 16-byte aligned, a lane's load 8-byte aligned), a width above 512 (the kernel's LDS tiles), a
 *   shape outside kge_transe_counts_supported.  There is no `_at` form: more than one rank stays refused.
 *   Seeds.  The rounding hash and the shared-negatives hashes start from the same step key, mix(seed + (step + 1) G): with one seed
 *   for both, the word that rounds columns 4 g .. 4 g + 3 of row `key` is the word that drew the candidate (or the side) whose
 *   counter is key (D / 4) + g.  The library takes the seeds in different calls and cannot see the pair; Config refuses equal seeds.
 * kge_bf16_shared_supported: 1 exactly where the two calls accept the model and N (TransE, ent_dim == rel_dim, negative_rel == 0,
 *   width % 8 == 0, width <= 512, 1 <= N <= 63, fewer than 2^30 rows), else 0.  Host only.
 * kge_transe_emit_records_shared_bf16 / kge_transe_emit_records_shared_chunks_bf16: the arguments of their fp32 namesakes with
 *   tables of stored bf16. */
int kge_bf16_shared_supported(const kge_model_desc *m, INT N);
int kge_transe_emit_records_shared_bf16(const kge_model_desc *m, const uint16_t *d_ent, const uint16_t *d_rel, const int32_t *d_h, const int32_t *d_t,
                                        const int32_t *d_r, INT n_pos, INT stride, INT P, const int32_t *d_cand, INT N, const uint8_t *d_pair,
                                        INT denom, uint32_t *d_rec, int32_t *d_dst, float *d_loss, void *stream);
int kge_transe_emit_records_shared_chunks_bf16(const kge_model_desc *m, const uint16_t *d_ent, const uint16_t *d_rel, const int32_t *d_h2,
                                               const int32_t *d_t2, const int32_t *d_r2, INT n_pos, INT stride, const int32_t *d_chunks, INT cap,
                                               const int32_t *d_cand, INT N, const uint8_t *d_pair, INT denom, uint32_t *d_rec, int32_t *d_dst,
                                               float *d_loss, void *stream);

/* ---- TransH on relation-grouped chunks (NON-PARITY, opt-in; csrc/shared_proj.hip) ----
 * Every positive of a relation-grouped chunk has the chunk's relation, so a chunk has ONE normalised normal vector and ONE r^,
 * and a candidate is projected and normalised once per chunk: a chunk gathers 2 P + N + 2 table rows where the unshared step
 * gathers P (2 + N) + 2 P.
 *   Order, draw, mask.  Exactly those of the section above: kge_shared_order_by_relation and kge_shared_negatives_draw_grouped are
 *               called unchanged (the draw handles ids only), and cap, the candidates, their sides, the masks and the typed lists
 *               are theirs.  b is the SORTED position throughout.
 *   Forward.    Chunk j has the relation rho of its first position (the ordering stage gives every position of a chunk the same
 *               one; rho outside [0, rel_total): the chunk takes no part).  l2n(x) = x / sqrt(max(sum x^2, 1e-12)).
 *               w^ = l2n(normal_vectors[rho]), r^ = l2n(rel_embeddings[rho]).  For an entity row x: a = x . w^, x_perp = x - a w^,
 *               x^ = l2n(x_perp) (side_project<KGE_TRANSH>, csrc/models_dev.hpp).  p_b = sum |h^_b + r^ - t^_b|.  For the pair
 *               (b, k): e = c^_k + r^ - t^_b for a new head, h^_b + r^ - c^_k for a new tail; v = p_b - sum |e| + margin.  The pair
 *               is ACTIVE when it is unmasked, h_b, t_b and the candidate id lie in [0, ent_total), and v >= 0 (a tie is active;
 *               sign(0) = 0).  loss = (1 / denom) sum over the active pairs of v; masked pairs stay in the denominator.
 *   Backward.   The gradients with respect to the NORMALISED PROJECTED vectors are integer sign counts, those of the TransE
 *               definition (tests/shared_neg_ref.py forward, `recs`): with s = sign(e) of an active pair, G(c^_k) takes -s for a
 *               new head and +s for a new tail, G(t^_b) +s of every new head, G(h^_b) -s of every new tail, G_r of the positive
 *               -s of every active pair; a positive with cnt active pairs adds cnt sign(h^ + r^ - t^) to G(h^_b) and its G_r and
 *               subtracts it from G(t^_b).  The chunk's G_r is the sum of its positives' (within +-2 N P: an int32, not an int8).
 *               With unit = 1 / denom, every entity row goes through side_backward<KGE_TRANSH> of unit G:
 *                 gxp = normalize_bwd(x^, unit G) = inv (unit G - [the norm was not clipped] (x^ . unit G) x^), inv = 1 / |x_perp|
 *                 d = gxp . w^;  the row's gradient = gxp - d w^;  acw -= d x + a gxp
 *               The chunk's rel_embeddings gradient is normalize_bwd(r^, unit G_r), its normal_vectors gradient
 *               normalize_bwd(w^, acw), acw summed over the 2 len + N entity rows of the chunk in a fixed order (the rows with a
 *               zero count vector add nothing).  A normal vector whose norm is clipped (an all-zero row) gives w^ = 0: the
 *               projection is the identity and acw is zero.
 *   Records.    M = 2 n_pos + cap (N + 2) FLOAT records of D floats: record b is h of position b, n_pos + b its t, 2 n_pos + j
 *               the rel_embeddings row of chunk j, 2 n_pos + cap + j its normal_vectors row, 2 n_pos + 2 cap + j N + k candidate
 *               k of chunk j.
 *   Keys.       In the virtual row space kge_float_records_apply / _adam / _adagrad give a TransH step of n_pos_total positives and
 *               N negatives: an entity id; hub_base + (j % hub_k) 2 R + rho for rel_embeddings and ... + R + rho for
 *               normal_vectors, with R = rel_total, hub_base = ent_total and hub_k = min(max(n_pos_total / (64 R), 1), 4096).
 *               A record whose count vector is all zero has key -1 (and unspecified contents); the relation record carries a key
 *               iff G_r != 0, the normal-vector record iff any entity record of the chunk does; every key of an empty slot, and of
 *               a position no slot covers, is -1.
 * kge_transh_emit_records_shared_chunks: one workgroup of four waves per chunk slot; no global atomics; a wave's shares of acw are
 *   added in the order it meets its rows, the four waves are folded in index order and the loss partials are summed over all cap
 *   slots in index order: a step is reproducible bit for bit.  tables: ent_embeddings, rel_embeddings, normal_vectors.  denom:
 *   batch_size * N of the whole step; n_pos_total: the step's positives (what the apply call is given).  d_rec: float [M][D], 16-byte
 *   aligned; d_dst: int32 [M].  KGE_ERR_UNSUPPORTED, naming the limit: another model, negative_rel > 0, N outside 1..63,
 *   ent_dim != rel_dim, a width above 512.  A chunk longer than 127 is the caller's error.
 * kge_shared_float_supported: 1 where that entry point takes the model and N (TransH, ent_dim == rel_dim <= 512,
 *   negative_rel == 0, 1 <= N <= 63), else 0.  Host only. */
int kge_transh_emit_records_shared_chunks(const kge_model_desc *m, const float *const tables[KGE_MAX_TABLES], const int32_t *d_h2,
                                          const int32_t *d_t2, const int32_t *d_r2, INT n_pos, INT stride, const int32_t *d_chunks, INT cap,
                                          const int32_t *d_cand, INT N, const uint8_t *d_pair, INT denom, INT n_pos_total, float *d_rec,
                                          int32_t *d_dst, float *d_loss, void *stream);
int kge_shared_float_supported(const kge_model_desc *m, INT N);

/* ---- TransD on relation-grouped chunks (NON-PARITY, opt-in; csrc/shared_proj.hip, the TransH kernel under MODEL = KGE_TRANSD) ----
 * A chunk of one relation shares r^ and the relation's transfer vector r_p, and a candidate's two rows (ent_embeddings and
 * ent_transfer) are gathered, projected and normalised once per chunk: a chunk gathers 2 (2 P + N) + 2 table rows where the
 * unshared step gathers P (4 + 2 N) + 2 P.
 *   Order, draw, mask.  Exactly those of the two sections above: kge_shared_order_by_relation and
 *               kge_shared_negatives_draw_grouped are called unchanged, and cap, the candidates, their sides, the masks and the
 *               typed lists are theirs.  b is the SORTED position throughout.
 *   Forward.    Chunk j has the relation rho of its first position (rho outside [0, rel_total): the chunk takes no part).
 *               l2n(x) = x / sqrt(max(sum x^2, 1e-12)).  r^ = l2n(rel_embeddings[rho]); r_p = rel_transfer[rho], RAW, not
 *               normalised (ctx_forward<KGE_TRANSD>).  For an entity id with ent_embeddings row x and ent_transfer row x_p:
 *               a = x . x_p, x_perp = x + a r_p, x^ = l2n(x_perp) (side_project<KGE_TRANSD>, csrc/models_dev.hpp).  p_b, e, v,
 *               ACTIVE, loss and denominator are TransH's on these x^: a tie v >= 0 is active, sign(0) = 0, masked pairs stay
 *               in the denominator.
 *   Backward.   The gradients with respect to the NORMALISED PROJECTED vectors are the integer sign counts of the TransE / TransH
 *               definition: G(c^_k), G(h^_b), G(t^_b), and the chunk's G_r as an int32.  With unit = 1 / denom, every entity goes
 *               through side_backward<KGE_TRANSD> of unit G:
 *                 gxp = normalize_bwd(x^, unit G) = inv (unit G - [the norm was not clipped] (x^ . unit G) x^), inv = 1 / |x_perp|
 *                 d = gxp . r_p;  gradient of the ent_embeddings row = gxp + d x_p;  of the ent_transfer row = d x;  acw += a gxp
 *               The chunk's rel_embeddings gradient is normalize_bwd(r^, unit G_r); its rel_transfer gradient is acw ITSELF (r_p
 *               is used raw: no normalise-backward), summed over the chunk's 2 len + N entities in a fixed order: each wave in
 *               the order it meets its rows, then the four waves in index order.  An all-zero rel_transfer row makes the
 *               projection the identity and d = 0: the transfer records are then zero, and still carry their keys.
 *   Records.    M = 4 n_pos + cap (2 N + 2) FLOAT records of D floats: record b is h's ent_embeddings row, n_pos + b h's
 *               ent_transfer row, 2 n_pos + b t's ent_embeddings row, 3 n_pos + b t's ent_transfer row, 4 n_pos + j the
 *               rel_embeddings row of chunk j, 4 n_pos + cap + j its rel_transfer row, 4 n_pos + 2 cap + j N + k candidate k's
 *               ent_embeddings row, 4 n_pos + 2 cap + cap N + j N + k its ent_transfer row.
 *   Keys.       In the virtual row space kge_float_records_apply / _adam / _adagrad give a TransD step of n_pos_total positives and
 *               N negatives: ent [0, E) | ent_transfer [E, 2 E) | hub_k copies of { rel [R] | rel_transfer [R] } from
 *               hub_base = 2 E, with hub_k = min(max(n_pos_total / (64 R), 1), 4096).  An entity row has key id, its transfer
 *               row E + id; rel_embeddings hub_base + (j % hub_k) 2 R + rho, rel_transfer ... + R + rho.  A row whose count vector
 *               is all zero has key -1 for BOTH of its records (contents unspecified), and an entity's transfer record carries a
 *               key exactly when its embedding record does, even where d = 0.  The rel_embeddings record carries a key iff
 *               G_r != 0, the rel_transfer record iff any entity record of the chunk does; every key of an empty slot, and of a
 *               position no slot covers, is -1.
 * kge_transd_emit_records_shared_chunks: the arguments of kge_transh_emit_records_shared_chunks; one workgroup of four waves per
 *   chunk slot, no global atomics, fixed summation orders: a step is reproducible bit for bit.  tables: ent_embeddings,
 *   rel_embeddings, rel_transfer, ent_transfer (all four are read).  With more than one candidate tile a positive's two count
 *   vectors wait as int32 in record slots b and 2 n_pos + b.  d_rec: float [M][D], 16-byte aligned; d_dst: int32 [M], all blanked
 *   first.  KGE_ERR_UNSUPPORTED, naming the limit: another model, negative_rel > 0, N outside 1..63, ent_dim != rel_dim, a width
 *   above 512.  A chunk longer than 127 is the caller's error.
 * kge_shared_transd_supported: 1 where that entry point takes the model and N (TransD, ent_dim == rel_dim <= 512,
 *   negative_rel == 0, 1 <= N <= 63), else 0.  Host only.  (kge_shared_float_supported keeps answering 0 for TransD.) */
int kge_transd_emit_records_shared_chunks(const kge_model_desc *m, const float *const tables[KGE_MAX_TABLES], const int32_t *d_h2,
                                          const int32_t *d_t2, const int32_t *d_r2, INT n_pos, INT stride, const int32_t *d_chunks, INT cap,
                                          const int32_t *d_cand, INT N, const uint8_t *d_pair, INT denom, INT n_pos_total, float *d_rec,
                                          int32_t *d_dst, float *d_loss, void *stream);
int kge_shared_transd_supported(const kge_model_desc *m, INT N);

/* ---- TransR on relation-grouped chunks (NON-PARITY, opt-in; csrc/shared_transr.hip, the row GEMMs of csrc/transr.hip) ----
 * A chunk of one relation has ONE matrix M_rho, so its 2 len positive rows and its N candidates are projected once each: a chunk
 * of P positives puts 2 P + N rows through the three row GEMMs (12 De Dr FLOPs a row) where the unshared step puts P (2 + N).
 *   Order, draw, mask.  Exactly those of "TransH on relation-grouped chunks": kge_shared_order_by_relation and
 *               kge_shared_negatives_draw_grouped are called unchanged, and cap, the candidates, their sides, the masks, the typed
 *               lists and the loss denominator are theirs.  b is the SORTED position throughout.
 *   Forward.    Chunk j has the relation rho of its first position (rho outside [0, rel_total): the chunk takes no part).
 *               l2n(x) = x / sqrt(max(sum x^2, 1e-12)).  r^ = l2n(rel_embeddings[rho]); for an entity row x: x^ = l2n(x . M_rho),
 *               M_rho = transfer_matrix[rho] as [ent_dim][rel_dim] (TransR.py:16-23; with negative_rel == 0 every negative takes
 *               the positive's matrix, TransR.py:57-60).  p_b = sum |h^_b + r^ - t^_b|.  For the pair (b, k): e = c^_k + r^ - t^_b
 *               for a new head, h^_b + r^ - c^_k for a new tail; v = p_b - sum |e| + margin.  The pair is ACTIVE when it is
 *               unmasked, h_b, t_b and the candidate id lie in [0, ent_total), and v >= 0 (a tie is active; sign(0) = 0: the
 *               rules of transr_vec_kernel).  loss = (1 / denom) sum over the active pairs of v; masked pairs stay in the
 *               denominator.
 *   Backward.   The gradients with respect to the NORMALISED PROJECTED vectors are the integer sign counts of the TransE / TransH
 *               definition: G(c^_k), G(h^_b), G(t^_b), and the chunk's G_r as an int32.  With unit = 1 / denom a row's GP row
 *               (width rel_dim) is normalize_bwd(x^, unit G) = inv (unit G - [the norm was not clipped] (x^ . unit G) x^),
 *               inv = 1 / |x . M_rho|; a row with a zero count vector, an invalid id or an inactive chunk has a zero GP row.
 *               ent_embeddings[id] += GP . M_rho^T per row, transfer_matrix[rho] += sum over the chunk's rows of x^T GP,
 *               rel_embeddings[rho] += normalize_bwd(r^, unit G_r).
 *   Rows.       J = 2 n_pos + cap N rows, chunk-major: slot c begins at row 2 first_c + c N and holds its len head rows, its len
 *               tail rows, then its N candidates (the used slots come first, in position order, and cover the positions without a
 *               gap, so no scan is needed; the slots are in relation order, so the rows are).  A slot of length 0, of a length above
 *               127, one that points outside [0, n_pos) or one whose relation lies outside the table owns no row; a row no slot
 *               owns has the key rel_total, the bucket the GEMMs skip, and a zero GP row.
 * kge_transr_forward_backward_shared_chunks: job list -> projection -> pair walk -> dgrad -> wgrad, ADDING into the dense gradient
 *   tables grads[0..2] (ent_embeddings, rel_embeddings, transfer_matrix) exactly as kge_forward_backward does for TransR; the
 *   chunk count stays on the device and the call has no host synchronisation.  The GEMM kernels are the unshared plain layout's,
 *   chosen by the same dimension rules and sized by J; dgrad takes its float-record mode by the existing size rule.  The pair walk
 *   is one workgroup of four waves per chunk slot; the loss partials are summed over all cap slots in index order (the loss is
 *   reproducible bit for bit), the relation row's gradient, dgrad below its record size and wgrad are fp32 atomics (the gradient
 *   tables are reproducible to rounding, not bit for bit).  d_h2 / d_t2 / d_r2: the sorted positives; stride >= n_pos; denom:
 *   batch_size * N of the whole step.  n_pos == 0 zeroes the loss and touches no gradient.  KGE_ERR_UNSUPPORTED, naming the limit:
 *   another model, negative_rel > 0, N outside 1..63, rel_dim above 512, more than 2^31 - 1 rows.
 * kge_shared_transr_supported: 1 where that entry point takes the model and N (TransR, negative_rel == 0, 1 <= N <= 63,
 *   1 <= rel_dim <= 512, ent_dim >= 1), else 0; 0 for a null descriptor.  Host only.  (The TransH and TransD answers stay 0 for
 *   TransR.) */
int kge_transr_forward_backward_shared_chunks(const kge_model_desc *m, const float *const tables[KGE_MAX_TABLES], const int32_t *d_h2,
                                              const int32_t *d_t2, const int32_t *d_r2, INT n_pos, INT stride, const int32_t *d_chunks, INT cap,
                                              const int32_t *d_cand, INT N, const uint8_t *d_pair, INT denom, float *const grads[KGE_MAX_TABLES],
                                              float *d_loss, void *stream);
int kge_shared_transr_supported(const kge_model_desc *m, INT N);

/* ---- Table-sharded sparse path (N GPUs, BASELINE config #5): rank g OWNS the entity rows [g*chunk, (g+1)*chunk); what the
 * reference does with ps tasks holding the variables and workers pulling rows / pushing IndexedSlices over gRPC
 * (distribute_training.py:193-196) becomes: request ids -> all-to-all -> owners gather rows -> all-to-all -> emit records
 * against the fetched rows -> all-to-all (row id, record) -> owners reduce + apply their rows.  These are the device stages
 * between the collectives (csrc/shard.hip); the collectives themselves are torch.distributed all_to_all_single (RCCL).
 *   kge_shard_requests      : d_req[slot*n_pos + b] = entity touched by record slot (slot, b) of the emit kernel, -1 if none
 *                             (slot 0/1 = the positive's head/tail, 2 = relation, 3+k = the new entity of negative k)
 *   kge_shard_count         : d_counts[o] = how many of d_ids (ids < 0 skipped) rank o = id / chunk owns   (n_owners <= 64)
 *   kge_shard_scatter       : d_sorted = the live ids grouped by owner (h_counts = HOST copy of d_counts), d_slot_of[i] = position of
 *                             d_ids[i] in d_sorted or -1; d_cursor = n_owners ints of scratch.  Only the first sum(h_counts)
 *                             entries of d_sorted are written, in any order inside an owner's group; h_counts summing to more
 *                             than n, or more than 64 owners, is KGE_ERR_BAD_ARG and nothing is written
 *   kge_shard_remap_batch   : the batch with entity ids replaced by positions in the fetched-row list (d_slot_of from the
 *                             requests), so the unchanged emit kernel runs against the fetched rows as its "entity table"
 *   kge_shard_requests_shared: the request list of a SHARED-negatives slice (above): d_req = [h of the n_pos positives | t of them
 *                             | the n_cand = n_chunks N candidate ids of d_cand], 2 n_pos + n_cand entries; an id outside
 *                             [0, ent_total) becomes -1, so nothing is requested for it.  A chunk of P positives asks for 2 P + N
 *                             rows where kge_shard_requests asks for P (2 + N)
 *   kge_shard_remap_shared  : the same ids as positions in the fetched-row list: d_h2[b] = d_slot_of[b], d_t2[b] =
 *                             d_slot_of[n_pos + b], d_cand2[i] = d_slot_of[2 n_pos + i] (d_slot_of from kge_shard_scatter of that
 *                             request list, where a -1 request has position -1); a negative id gives -1 whatever d_slot_of holds.
 *                             -1 is "outside the table" to kge_transe_emit_records_shared_at, which runs against the fetched rows
 *                             with ent_total = their number
 *   kge_shard_gather_rows   : d_out[i,:] = d_table[d_ids[i] - row_lo, :]  (the owner's reply; dim % 4 == 0); the ids come from a
 *                             peer, so the row index is clamped into [0, rows - 1]: nothing outside the shard is read
 *   kge_shard_record_ids    : d_ids[m] = global entity id of record m when its destination is a fetched-row slot, else -1
 *   kge_shard_pack_records  : d_out[d_slot_of[m], :] = d_rec[m, :] for the records that travel
 *   kge_shard_relation_counts: relation records (destination >= cache_rows) summed into the dense int32 image [R, dim]
 *                             (zero it first; all-reduced across ranks, the small relation table stays replicated) */
int kge_shard_requests(const int32_t *d_h, const int32_t *d_t, const int32_t *d_r, INT n_pos, INT n_neg, INT stride, int32_t *d_req,
                       void *stream);
int kge_shard_count(const int32_t *d_ids, INT n, INT chunk, INT n_owners, int32_t *d_counts, void *stream);
int kge_shard_scatter(const int32_t *d_ids, INT n, INT chunk, INT n_owners, const INT *h_counts, int32_t *d_cursor, int32_t *d_sorted,
                      int32_t *d_slot_of, void *stream);
int kge_shard_remap_batch(const int32_t *d_h, const int32_t *d_t, INT n_pos, INT n_neg, INT stride, const int32_t *d_slot_of, int32_t *d_h2,
                          int32_t *d_t2, void *stream);
int kge_shard_requests_shared(const int32_t *d_h, const int32_t *d_t, INT n_pos, const int32_t *d_cand, INT n_cand, INT ent_total, int32_t *d_req,
                              void *stream);
int kge_shard_remap_shared(const int32_t *d_h, const int32_t *d_t, INT n_pos, const int32_t *d_cand, INT n_cand, const int32_t *d_slot_of,
                           int32_t *d_h2, int32_t *d_t2, int32_t *d_cand2, void *stream);
int kge_shard_gather_rows(const float *d_table, const int32_t *d_ids, INT n, INT row_lo, INT rows, INT dim, float *d_out, void *stream);
int kge_shard_record_ids(const int32_t *d_dst, INT n_records, INT cache_rows, const int32_t *d_cache_ids, int32_t *d_ids, void *stream);
int kge_shard_pack_records(const uint32_t *d_rec, const int32_t *d_slot_of, INT n_records, INT dwords, uint32_t *d_out, void *stream);
/* The same image from a COMPACT (rows, counts) pair as kge_transe_reduce_records leaves it (dim % 4 == 0): image[row - base] =
 * counts of that row for rows in [base, base + rel_total); the image is zeroed by the caller.  Config._sharded_step reduces the
 * relation-slot records (a contiguous third of the record buffer) by sort + segmented sum and scatters the <= R rows with this --
 * the per-element int32 atomics of kge_shard_relation_counts were 0.40 ms of a 3.0 ms step at 133 k positives x dim 512. */
int kge_shard_scatter_count_rows(const int32_t *d_rows, const int32_t *d_row_counts, const int32_t *d_n_rows, INT max_rows, INT base,
                                 INT rel_total, INT dim, int32_t *d_image, void *stream);
int kge_shard_relation_counts(const uint32_t *d_rec, const int32_t *d_dst, INT n_records, INT cache_rows, INT rel_total, INT dwords, INT dim,
                              int32_t *d_counts, void *stream);

/* ---- Many training steps in ONE persistent launch (csrc/persist.hip): the loop body of distribute_training.py:267-283 --
 * sampling, forward / backward, optimizer -- at the reference's own (launch-latency bound) batch sizes.  One workgroup per CU
 * stays resident and walks n_steps steps with two XCD-hierarchical grid barriers per step; batches are bit-identical to n_steps
 * calls of `sampling` (all workThreads streams are advanced accordingly), gradients go through fp32 atomics as in
 * kge_forward_backward's small-step path.  TransE / TransH / TransD, embedding width <= 256, the whole batch on this GPU.
 *   h_lr[n_steps] : HOST array, the learning rate of each step (SGD: alpha; Adam: lr_t = alpha*sqrt(1-b2^t)/(1-b1^t))
 *   d_losses[n_steps] : DEVICE array, receives every step's loss
 * kge_persistent_aborted: 1 if a grid barrier of the last launch gave up (a bounded spin expired); the tables are then in an
 * unspecified intermediate state and the caller must treat the run as failed.  Synchronises. */
int kge_train_steps_persistent(const kge_model_desc *m, float *const tables[KGE_MAX_TABLES], float *const grads[KGE_MAX_TABLES],
                               float *const adam_m[KGE_MAX_TABLES], float *const adam_v[KGE_MAX_TABLES], INT batchSize, INT negRate,
                               INT negRelRate, INT n_steps, int32_t adam, const float *h_lr, float beta1, float beta2, float eps,
                               float *d_losses, void *stream);
int kge_persistent_aborted(int32_t *flag);
/* measurement hook (option "persist_trace"): workgroup 0's 100 MHz clock at the six phase boundaries of each of the first
 * n_steps (<= 256) steps of the last launch: [sweep start, sampling start, barrier-1 arrive, barrier-1 leave, barrier-2 arrive, leave] */
int kge_persistent_trace(uint64_t *h_out, INT n_steps);

/* Device-native link prediction for test triples [first, first+count) (replaces the loop
 * distribute_training.py:465-590: getTailBatch -> sess.run(predict) -> testTail, and the head side when
 * test_head != 0).  h_out (HOST) receives count x 2 x 8 int64: [i][0] testTail's 8-vector, [i][1]
 * testHead's (zeros if test_head == 0).  Needs importTestFiles (+ Type / Ontology files if present). */
int kge_link_prediction(const kge_model_desc *m, const float *const tables[KGE_MAX_TABLES], INT first, INT count,
                        INT test_head, int64_t *h_out, void *stream);

/* Link prediction against a ROW RANGE of the entity table (a table sharded by rows across ranks; csrc/lp_shard.hip).
 * Rank test triples [first, first+count) (kge_link_prediction's order) against the candidate entities [row_lo, row_lo+rows)
 * only.  tables[0] holds exactly those rows (row i = entity row_lo+i); tables[1] is the whole relation table.  d_query_rows
 * (DEVICE fp32 [count][2][ent_dim]) holds the raw h and t rows of each test triple.
 * d_counts (DEVICE int64 [count][2][4], written): side 0 tail / side 1 head; raw, filtered, typed, filtered+typed counts of the
 *   candidates in the range (the target excluded) scoring strictly below the true triple; NaN never counts.
 * d_keys (DEVICE int64 [count][2][4], written): the four arg-mins as pack_key(score, id) (select_dev.hpp), INT64_MAX if no
 *   candidate in the range scores below.  Counted scores are >= +0, so the keys order as int64 the way they order unsigned.
 * The score is the L1 distance |hn + rn - tn| summed in one fixed order (TransE's predict op divides it by the dimension), the
 * true triple's score by the same function from d_query_rows: an entity whose row equals the target's ties with it and is not
 * counted, in whichever range it lies.  Merging ranges: SUM of d_counts, MIN of d_keys -- exactly, bit for bit, for any cut.
 * TransE only (KGE_ERR_UNSUPPORTED otherwise; ent_dim <= 1024).  Needs importTestFiles.  No host synchronisation. */
int kge_link_prediction_range(const kge_model_desc *m, const float *const tables[KGE_MAX_TABLES], INT row_lo, INT rows,
                              const float *d_query_rows, INT first, INT count, INT test_head, int64_t *d_counts, int64_t *d_keys,
                              void *stream);
/* Merged counts + keys -> kge_link_prediction's host layout [count][2][8] (side 1 zero when test_head == 0), ontology classes
 * resolved as rank_kernel does (Test.h:113-135: shared, never-rewinding cursors).  One host synchronisation. */
int kge_link_prediction_finish(INT first, INT count, INT test_head, const int64_t *d_counts, const int64_t *d_keys, int64_t *h_out,
                               void *stream);
/* d_ids (DEVICE int32 [count][2]) = the head and tail ids of test triples [first, first+count), kge_link_prediction's order. */
int kge_test_entity_ids(INT first, INT count, int32_t *d_ids, void *stream);
/* kge_rank_triples against a ROW RANGE of the entity table (csrc/lp_shard.hip: kge_link_prediction_range's scan for any triples,
 * counts only).  Triple i = (d_h[i], d_t[i], d_r[i]) (DEVICE int32; any order, any mix of relations, duplicates); tables[0]
 * holds rows [row_lo, row_lo+rows) of the entity table (row j = entity row_lo+j), tables[1] the whole relation table, and
 * d_query_rows (DEVICE fp32 [n][2][ent_dim]) the raw h and t row of each triple, which may lie outside the range.
 * d_counts (DEVICE int64 [n][2][4], zeroed and then accumulated into): side 0 tail / side 1 head (zeros when test_head == 0);
 *   raw, filtered (train + valid + test), typed, filtered + typed counts of the candidates in the range, other than the target,
 *   that score strictly below the true triple; NaN never counts.
 * The score bits are kge_link_prediction_range's (one definition for candidates and targets: a row equal to the target's row
 * ties and is not counted, whichever range holds it), so for the triples of the test split d_counts equals its d_counts bit for
 * bit, and the SUM over any cut of the table into ranges equals the whole table as one range.  Against kge_rank_triples a
 * candidate within an ulp or so of the true triple may fall on the other side of it.
 * A triple with an id outside [0, ent_total) / [0, rel_total) is disabled -- all its counts stay zero and nothing is indexed
 * with its ids -- and the call still returns KGE_OK.  n == 0 checks the arguments and the files and launches nothing; rows == 0
 * only zeroes d_counts.  No host synchronisation and no copy of the triples to the host.  TransE only (KGE_ERR_UNSUPPORTED
 * otherwise; ent_dim in [1, 1024]); 0 <= n < 2^30, the range inside the table and non-null arrays when n > 0 (KGE_ERR_BAD_ARG);
 * needs importTestFiles (KGE_ERR_NO_DATASET).  Nothing is written to d_counts when an error is returned. */
int kge_rank_triples_range(const kge_model_desc *m, const float *const tables[KGE_MAX_TABLES], INT row_lo, INT rows,
                           const float *d_query_rows, const int32_t *d_h, const int32_t *d_t, const int32_t *d_r, INT n, INT test_head,
                           int64_t *d_counts, void *stream);

/* Filtered ranks of caller-supplied triples on the device (csrc/rank.hip): triple i = (d_h[i], d_t[i], d_r[i]) (DEVICE int32),
 * in any order, with any mix of relations and with duplicates -- the validation split, or any triples of the caller's.
 * d_counts (DEVICE int64 [n][2][4], every element written): side 0 ranks all entities as the tail of (h, r, ?), side 1 as the
 * head of (?, r, t) (all zeros when test_head == 0); the four columns are the numbers of candidates other than the target that
 * score strictly below the true triple -- raw, filtered, typed, filtered + typed -- exactly as columns 0..3 of
 * kge_link_prediction's 8-vectors: NaN never counts, the filter is the train + valid + test union of importTestFiles (the triple
 * itself need not be in it), typed means membership in the relation's head / tail type list (0 without importTypeFiles).  No
 * arg-mins and no ontology classes.  The scores are kge_predict's bits, the ones kge_link_prediction ranks (TransR: each
 * relation's own matrix).  All four models; embedding dimension (TransR: relation dimension) <= 1024, KGE_ERR_UNSUPPORTED above.
 * Needs importTestFiles (KGE_ERR_NO_DATASET).  Ids are the caller's precondition.  No [n x E] score matrix is formed; one host
 * synchronisation (the triples are grouped by relation).  With n == 0 only the arguments (null pointers included) and the files are checked.  Nothing is
 * written to d_counts when an error is returned.  Option "rank_slices" (test hook): N > 0 cuts the candidates into N slices,
 * 0 chooses; the counts do not depend on it. */
int kge_rank_triples(const kge_model_desc *m, const float *const tables[KGE_MAX_TABLES], const int32_t *d_h, const int32_t *d_t,
                     const int32_t *d_r, INT n, INT test_head, int64_t *d_counts, void *stream);

/* Ranks of triples against CANDIDATE LISTS instead of every entity (csrc/rank_cand.hip): triple i = (d_h[i], d_t[i], d_r[i])
 * (DEVICE int32), each side ranked against n_cand candidates that the caller supplies or that the kernel draws.  Cost is
 * n x n_cand x dim; no candidate table, no score matrix, no host synchronisation.
 * d_counts (DEVICE int64 [n][2][2], every element written): side 0 ranks the list as the tail of (h, r, ?), side 1 as the head
 *   of (?, r, t).  Column 0: the listed candidates, other than the target id, whose score is strictly below the true triple's
 *   (NaN never counts); column 1: the same without the candidates that form a known triple with the fixed entity and the
 *   relation (the train + valid + test union of importTestFiles).  Without KGE_RANKC_FILTERED column 1 is not computed and
 *   equals column 0, and importTestFiles is not needed.
 * Lists: a side's list is read at d_*_cand[i * stride + k], k < n_cand (DEVICE int32): stride >= n_cand is one list per triple,
 *   stride == 0 one list shared by all triples.  A NULL list: that side is not ranked and its counts are zero.  An id outside
 *   [0, ent_total) is skipped, so -1 pads ragged lists; a repeated id counts every time it is listed.
 * KGE_RANKC_DRAWN: both list pointers are NULL and candidate k of (triple i, side s) is drawn inside the kernel (no list exists
 *   in memory), all arithmetic mod 2^64:
 *       c = ((2 i + s) << 32) | k;   z = seed + (c + 1) * 0x9E3779B97F4A7C15;
 *       z = (z ^ z >> 30) * 0xBF58476D1CE4E5B9;   z = (z ^ z >> 27) * 0x94D049BB133111EB;   z ^= z >> 31;
 *       id = ((z >> 32) * ent_total) >> 32
 *   With KGE_RANKC_TYPED the same ((z >> 32) * len) >> 32 indexes the relation's tail (side 0) / head (side 1) type list of
 *   importTypeFiles (len its length); a relation with an empty list takes the untyped draw.  With KGE_RANKC_NO_HEAD only the
 *   tail side is drawn and ranked.  TYPED and NO_HEAD need DRAWN.
 * The scores are kge_predict's bits (TransR: each relation's own matrix).  TransE / TransH / TransD take one fused kernel
 * (a team per (triple, side), candidate rows gathered straight into registers); TransR, and every model with option
 * "rankc_fused" = 0, takes the two-stage form: chunks of at most 2^22 (triple, candidate) pairs are spelled out in a bounded
 * workspace, scored by kge_predict's own kernels and counted; both forms give the same counts.  Option "rankc_slices" (test
 * hook): N > 0 cuts every list into N slices over the grid, 0 chooses; the counts do not depend on it.
 * A triple with an id outside [0, ent_total) / [0, rel_total) is disabled: its counts stay zero, nothing is indexed with its
 * ids and the call still returns KGE_OK.  n == 0 or n_cand == 0 checks the arguments, zeroes d_counts and launches nothing.
 * KGE_ERR_BAD_ARG: a null model, table, triple or output array, n outside [0, 2^30), n_cand outside [0, 2^31), unknown flags,
 * a list pointer together with DRAWN, no list at all without it, TYPED / NO_HEAD without DRAWN, a stride that is neither 0 nor
 * >= n_cand; KGE_ERR_UNSUPPORTED: embedding (TransR: relation) dimension above 1024; KGE_ERR_NO_DATASET: FILTERED before
 * importTestFiles, TYPED before importTypeFiles.  Nothing is written to d_counts when an error is returned. */
#define KGE_RANKC_FILTERED 1
#define KGE_RANKC_DRAWN 2
#define KGE_RANKC_TYPED 4
#define KGE_RANKC_NO_HEAD 8
int kge_rank_candidates(const kge_model_desc *m, const float *const tables[KGE_MAX_TABLES], const int32_t *d_h, const int32_t *d_t,
                        const int32_t *d_r, INT n, const int32_t *d_tail_cand, INT tail_stride, const int32_t *d_head_cand,
                        INT head_stride, INT n_cand, INT flags, uint64_t seed, int64_t *d_counts, void *stream);
/* kge_rank_candidates against a ROW RANGE of the entity table (a table sharded by rows across ranks; the RANGE form of the fused
 * kernel in csrc/rank_cand.hip).  tables[0] holds rows [row_lo, row_lo+rows) of the entity table (row j = entity row_lo+j),
 * tables[1] the whole relation table, and d_query_rows (DEVICE fp32 [n][2][ent_dim], kge_rank_triples_range's layout) the raw h
 * and t row of each triple, which may lie outside the range.  Triples, lists, strides, flags, seed and the drawn ids are
 * kge_rank_candidates'; ent_total stays the GLOBAL entity count (it bounds the listed ids and scales the drawn ones).
 * d_counts (DEVICE int64 [n][2][2], every element written): kge_rank_candidates' two columns over the candidates whose global id
 * lies in the range.  A candidate outside it is neither gathered nor counted; the target is excluded by its global id.  The true
 * triple's score is formed from d_query_rows by the very operations kge_rank_candidates applies to the table's rows, so every
 * range compares against the same score bits, and the SUM of d_counts over any cut of [0, ent_total) into ranges equals
 * kge_rank_candidates on the whole table, bit for bit.  Work follows the candidates the range owns: a team compacts the owned
 * ids of each batch into a pending queue and gathers rows U at a time from it, at most owned + U - 1 rows per (request, slice).
 * A triple with an id out of range is disabled as in kge_rank_candidates (zero counts; its query rows are not read).
 * rows == 0 only zeroes d_counts; n == 0 or n_cand == 0 checks the arguments and the files, zeroes d_counts and launches
 * nothing.  No host synchronisation; option "rankc_slices" applies; there is no two-stage form.
 * KGE_ERR_UNSUPPORTED: a model other than TransE, ent_dim above 1024; KGE_ERR_BAD_ARG: what kge_rank_candidates refuses, a range
 * outside the table, null d_query_rows with n > 0; KGE_ERR_NO_DATASET as kge_rank_candidates.  Nothing is written to d_counts
 * when an error is returned. */
int kge_rank_candidates_range(const kge_model_desc *m, const float *const tables[KGE_MAX_TABLES], INT row_lo, INT rows,
                              const float *d_query_rows, const int32_t *d_h, const int32_t *d_t, const int32_t *d_r, INT n,
                              const int32_t *d_tail_cand, INT tail_stride, const int32_t *d_head_cand, INT head_stride,
                              INT n_cand, INT flags, uint64_t seed, int64_t *d_counts, void *stream);

/* ---- Evaluation on bf16 tables (csrc/bf16_eval.hip; csrc/rank_cand.hip, the fused kernel under BF16) ----
 * The evaluators whose cost is the rows they gather -- kge_predict and kge_rank_candidates -- on tables STORED as bf16 ("bf16
 * table storage"): d_ent [ent_total, D] and d_rel [rel_total, D], one uint16 per element, in place of tables[].  No float32 copy
 * of a table is made or needed, and a gathered row is half the bytes.
 * Definition.  A stored row is read in the team layout of the fp32 kernels (lane l of a team of L holds elements l, l + L, ...;
 *   (L, C) is for_team_shape's rung for D), each element widened exactly (bits << 16), elements from D on are 0.  Every operation
 *   after the load is the fp32 kernel's, in its order.  So:
 *     kge_predict_bf16          returns, bit for bit, the scores kge_predict returns on the widened tables;
 *     kge_rank_candidates_bf16  returns the counts kge_rank_candidates returns on the widened tables, in every candidate mode
 *                               (lists, DRAWN, DRAWN | TYPED), both sides, NO_HEAD, FILTERED, any "rankc_slices", and in the
 *                               two-stage form of option "rankc_fused" = 0 (pairs spelled out, scored by kge_predict_bf16's kernel,
 *                               counted), which gives the fused form's counts.
 *   The rows are deliberately not read as packed pairs: that would change the order of the sums, and with it the bits.
 * kge_bf16_eval_supported (host only, no device needed): 1 exactly when the model is TransE, ent_dim == rel_dim, D % 8 == 0 and
 *   8 <= D <= 1024 -- the storage rule of "bf16 table storage" -- else 0.  The two calls refuse every other descriptor with
 *   KGE_ERR_UNSUPPORTED and the limit's name.
 * Arguments, the n == 0 and n_cand == 0 cases, disabled triples, the files FILTERED / TYPED need and every other error are those of
 * the fp32 namesakes, with "a null table" meaning d_ent or d_rel; nothing is written when an error is returned. */
int kge_bf16_eval_supported(const kge_model_desc *m);
int kge_predict_bf16(const kge_model_desc *m, const uint16_t *d_ent, const uint16_t *d_rel, const int32_t *d_h, const int32_t *d_t,
                     const int32_t *d_r, INT n, float *d_out, void *stream);
int kge_rank_candidates_bf16(const kge_model_desc *m, const uint16_t *d_ent, const uint16_t *d_rel, const int32_t *d_h, const int32_t *d_t,
                             const int32_t *d_r, INT n, const int32_t *d_tail_cand, INT tail_stride, const int32_t *d_head_cand,
                             INT head_stride, INT n_cand, INT flags, uint64_t seed, int64_t *d_counts, void *stream);
/* The FULL-ENTITY evaluators on stored bf16 tables (csrc/rank.hip and csrc/topk.hip, their kernels under BF16): every entity is a
 * candidate, and the candidate rows are streamed from the stored table once per request block -- no float32 view of a table and no
 * [E, D] candidate table is made.  Same descriptors as above (kge_bf16_eval_supported), refused the same way, before the device
 * check.
 *     kge_rank_triples_bf16    returns all [n][2][4] counts kge_rank_triples returns on the widened tables, for every "rank_slices".
 *                              kge_rank_triples scores rows of a table of NORMALISED rows; here each candidate, fixed and target
 *                              row is normalised as it is read, by the same function (each lane's own 1 / |x|, a rounded product),
 *                              which costs one more team reduction per row.  Allocates its request and block arrays only.
 *     kge_topk_entities_bf16   returns every id and every score bit kge_topk_entities returns on the widened tables (padding and NaN
 *                              order included), for both settings of "topk_table_max_bytes" (the budget is compared with
 *                              E * D * 4, as there).  d_rel_tab is the relation TABLE, d_rel the queries' relation ids.  Allocates
 *                              the [E] float32 inverse norms (within the budget) and the partial key lists, nothing of E * D.
 * Arguments, n == 0, and every other error are those of the fp32 namesakes, with "a null table" meaning d_ent or the relation
 * table; nothing is written when an error is returned. */
int kge_rank_triples_bf16(const kge_model_desc *m, const uint16_t *d_ent, const uint16_t *d_rel, const int32_t *d_h, const int32_t *d_t,
                          const int32_t *d_r, INT n, INT test_head, int64_t *d_counts, void *stream);
int kge_topk_entities_bf16(const kge_model_desc *m, const uint16_t *d_ent, const uint16_t *d_rel_tab, const int32_t *d_fixed,
                           const int32_t *d_rel, const int32_t *d_head, INT n, INT k, INT flags, int32_t *d_ids, float *d_scores,
                           void *stream);

/* The engine's own device memory.  Its workspaces are allocated with hipMalloc (csrc/dev_buf.hpp), which a caller's allocator
 * statistics (torch's, for one) do not see.  *live: bytes held now by all of them; *peak: the largest *live since the last reset
 * (or since the process began).  reset_peak != 0 sets the peak to the current live bytes after reporting it.  Either pointer may
 * be null.  Host only: no device needed, and 0 / 0 in a process that has allocated nothing.  Always KGE_OK. */
int kge_workspace_bytes(int64_t *live, int64_t *peak, int reset_peak);

/* Batched top-k entity prediction on the device.  Query i: d_head[i] == 0 asks for the k best tails of (d_fixed[i], d_rel[i], ?),
 * d_head[i] != 0 for the k best heads of (?, d_rel[i], d_fixed[i]); sides and relations may be mixed in any order.  d_ids /
 * d_scores (DEVICE, row-major [n][k]) receive the candidates in ascending (score, id) order -- NaN after every number -- with
 * kge_predict's score for that triple up to the contraction of its products (ulp level; TransR: each query with its own
 * relation's matrix), identical on the table and on-the-fly paths; rows with fewer
 * than k eligible candidates are padded with id -1 / score +inf.  flags: KGE_TOPK_FILTERED drops candidates forming a known
 * triple (train + valid + test, needs importTestFiles), KGE_TOPK_TYPED keeps only the relation's head / tail type list (needs
 * importTypeFiles) -- what kge_link_prediction's filtered / type-constrained ranks count.  1 <= k <= 1024.  Ids are the
 * caller's precondition.  No [n x E] score matrix is formed; TransE needs no host synchronisation, the other models one
 * (queries are grouped by relation).  Option "topk_table_max_bytes" chooses between a candidate table and on-the-fly sides. */
#define KGE_TOPK_FILTERED 1
#define KGE_TOPK_TYPED 2
int kge_topk_entities(const kge_model_desc *m, const float *const tables[KGE_MAX_TABLES], const int32_t *d_fixed, const int32_t *d_rel,
                      const int32_t *d_head, INT n, INT k, INT flags, int32_t *d_ids, float *d_scores, void *stream);
/* Top-k entities against a ROW RANGE of the entity table (a table sharded by rows across ranks; csrc/topk.hip).  The queries
 * of kge_topk_entities, scored against the candidates with global ids [row_lo, row_lo+rows) only: tables[0] holds exactly
 * those rows (row i = entity row_lo+i), tables[1] is the whole relation table, and d_query_rows (DEVICE fp32 [n][ent_dim])
 * holds the raw row of each query's fixed entity d_fixed[i] (which may lie outside the range).  The filter and the type lists
 * test the global id.  d_keys (DEVICE uint64 [n][k], written) receives each query's k smallest keys in ascending order,
 * padded with KGE_TOPK_NO_KEY.  Key layout (select_dev.hpp pack_key): bits 63..32 the score's bits made orderable as an
 * unsigned integer (sign bit set for a positive float, all bits flipped for a negative one; every NaN 0xFFFFFFFF), bits 31..0
 * the global entity id -- keys order as (score, id), NaN after every number, and are unique per query.  rows == 0 is legal
 * (all padding).  The score bits are kge_topk_entities' (same functions, same per-dimension bucket), so merging the ranges of
 * any cut with kge_topk_merge_keys gives kge_topk_entities on the whole table, ids and score bits alike.  TransE only
 * (KGE_ERR_UNSUPPORTED otherwise; ent_dim <= 1024).  Option "topk_table_max_bytes" as for kge_topk_entities (rows x dim x 4).
 * No host synchronisation.  With n == 0 only the arguments (and the files the flags need) are checked. */
#define KGE_TOPK_NO_KEY 0xFFFFFFFFFFFFFFFFull
int kge_topk_entities_range(const kge_model_desc *m, const float *const tables[KGE_MAX_TABLES], INT row_lo, INT rows,
                            const float *d_query_rows, const int32_t *d_fixed, const int32_t *d_rel, const int32_t *d_head, INT n,
                            INT k, INT flags, uint64_t *d_keys, void *stream);
/* The k smallest keys of `parts` key lists per query -- d_keys (DEVICE uint64 [parts][n][k], e.g. the ranges' kge_topk_entities_range
 * outputs grouped by source) -- unpacked into d_ids / d_scores (DEVICE [n][k]) as kge_topk_entities writes them: ascending, padded
 * with id -1 / score +inf.  1 <= k <= 1024.  No host synchronisation. */
int kge_topk_merge_keys(const uint64_t *d_keys, INT n, INT parts, INT k, int32_t *d_ids, float *d_scores, void *stream);

/* Batched top-k relation prediction on the device: the k best relations of (d_h[i], ?, d_t[i]) for n queries (DEVICE int32 ids).
 * d_ids / d_scores (DEVICE, row-major [n][k]) receive the relations in ascending (score, id) order -- NaN after every number --
 * with kge_predict's score of (h, t, r) up to the contraction of its products (ulp level); TransR scores every relation with
 * that relation's own matrix (kge_predict called on all relations at once would not).  Rows with fewer than k eligible
 * relations are padded with id -1 / score +inf.  flags as for kge_topk_entities: KGE_TOPK_FILTERED drops relations forming a
 * known triple (train + valid + test, needs importTestFiles), KGE_TOPK_TYPED keeps relations whose head type list holds h
 * and whose tail type list holds t (needs importTypeFiles).  1 <= k <= 1024.  Ids out of range score NaN (callers check them).
 * KGE_ERR_UNSUPPORTED for an embedding (TransR: relation) dimension above 1024.  No host synchronisation. */
int kge_topk_relations(const kge_model_desc *m, const float *const tables[KGE_MAX_TABLES], const int32_t *d_h,
                       const int32_t *d_t, INT n, INT k, INT flags, int32_t *d_ids, float *d_scores, void *stream);
/* Relation prediction for test triples [first, first+count) in kge_link_prediction's order (importTestFiles' (r, h, t) sort):
 * h_out (HOST) receives count x 4 int64, the number of relations r' != r scoring strictly below the true relation r (scores
 * as kge_topk_relations; NaN never counts): [0] raw, [1] filtered (r' with (h, r', t) in train + valid + test left out),
 * [2] typed (only r' whose head type list holds h and tail type list holds t), [3] filtered and typed.  Without
 * importTypeFiles no relation is typed and columns 2 / 3 are 0, as kge_link_prediction's constrained columns count nothing
 * then.  KGE_ERR_NO_DATASET before importTestFiles.  One host synchronisation, at the end. */
int kge_relation_prediction(const kge_model_desc *m, const float *const tables[KGE_MAX_TABLES], INT first, INT count,
                            int64_t *h_out, void *stream);
/* Relation prediction with the entity rows supplied by the caller (an entity table sharded by rows across ranks;
 * csrc/relpred.hip).  Test triples [first, first+count) in kge_relation_prediction's order; d_query_rows (DEVICE fp32
 * [count][2][ent_dim]) holds the raw h and t rows of each triple, the layout kge_link_prediction_range takes.  d_counts (DEVICE
 * int64 [count][4], written) receives kge_relation_prediction's four columns: raw, filtered, typed, filtered + typed.  tables[0]
 * is never read (on a sharded rank it is the shard); tables[1] is the whole relation table.  The scores come from the same
 * kernel instantiation on the same row values, so the counts equal kge_relation_prediction's exactly.  TransE only
 * (KGE_ERR_UNSUPPORTED otherwise; ent_dim <= 1024).  KGE_ERR_NO_DATASET before importTestFiles, KGE_ERR_BAD_ARG for a range
 * outside the test set.  With count == 0 only the arguments and the files are checked.  No host synchronisation. */
int kge_relation_prediction_rows(const kge_model_desc *m, const float *const tables[KGE_MAX_TABLES], const float *d_query_rows,
                                 INT first, INT count, int64_t *d_counts, void *stream);

/* ---- Triple classification on the device (csrc/tclass.hip): getBestThreshold / test_triple_classification over DEVICE score
 * arrays, with the host routines' bits.  Scores are fp32 in the order of the validation / test list (sorted by relation, the
 * order getValidBatch / getTestBatch fill).  Need importTestFiles: before it, KGE_ERR_NO_DATASET with the host routines' message.
 * KGE_ERR_NO_DEVICE without a GPU, KGE_ERR_BAD_ARG for a null array or a size that is not the split's total.
 *
 * kge_tc_fit: d_thresh[r] (DEVICE fp32 [rel_total]) = getBestThreshold's threshold of every relation with validation triples
 *   -- the lowest grid point fmaf(i, 0.01f, min), i = 0..n_interval, of the best float accuracy -- and is left untouched for the
 *   others.  d_n_interval (DEVICE int32 [rel_total], or NULL) receives get_n_interval's value of every relation (0 without
 *   validation triples).  n_valid must be getValidTotal().  A non-finite score (the host's INT conversion is undefined there) is
 *   KGE_ERR_BAD_ARG, a relation whose n_interval is 2^24 or more, or grids needing more than 2^28 histogram bins together,
 *   KGE_ERR_UNSUPPORTED; in these cases NO threshold is written and d_n_interval is left untouched too.  Those return codes come from the scores, so the call waits
 *   ONCE on `stream`, behind its min / max pass, for a 16-byte status; the binning, prefix sums and arg-max that follow are
 *   enqueued and not waited for, and no other stream is touched.  The fit's working state (per-relation ranges, the global
 *   histogram, the status word) is one per process: ONE kge_tc_fit at a time -- do not call it from two threads or enqueue
 *   fits on two streams that may run concurrently.
 * kge_tc_apply: split 0 = validation scores, 1 = test scores (n = that list's total).  d_counts (DEVICE int64 [4], written) =
 *   TP, TN, FP, FN over the relations that have both validation and split triples (Test.h:353), a positive counted right when
 *   score <= d_thresh[r], a negative when score > d_thresh[r]; d_rel (DEVICE int64 [rel_total][2] or NULL, written) = each
 *   relation's right answers and answers (0, 0 for a relation left out).  Integer sums: the same for any order.  No host
 *   synchronisation. */
int kge_tc_fit(const float *d_pos, const float *d_neg, INT n_valid, float *d_thresh, int32_t *d_n_interval, void *stream);
int kge_tc_apply(INT split, const float *d_thresh, const float *d_pos, const float *d_neg, INT n, int64_t *d_counts, int64_t *d_rel,
                 void *stream);

/* kge_tc_roc: get_TPFP's counts for EVERY relation at once, and the exact area under each relation's ROC polyline.  d_vpos /
 *   d_vneg = the validation scores (n_valid = getValidTotal()): they give each relation's grid g(i) = fmaf(i, 0.01f, min),
 *   i = 0..n_interval, kge_tc_fit's grid bit for bit.  split 0 = validation list, 1 = test list; d_pos / d_neg = that list's
 *   scores, n = its total (split 0 may pass the validation arrays again).
 *   h_offsets (HOST int64 [rel_total + 1], written before the call returns) = prefix sums of 2 * (n_interval + 1) over the
 *   relations with validation triples; a relation without them has an empty slice.
 *   d_tpfp (DEVICE int64, or NULL for the areas alone): d_tpfp[h_offsets[r] .. h_offsets[r + 1]) = get_TPFP(r)'s layout,
 *   TP(0..n_interval) then FP(0..n_interval), TP(i) / FP(i) = the relation's split positives / negatives with score <= g(i);
 *   zeros for a relation with validation but no split triples (as the host get_TPFP of this library gives).  tpfp_capacity =
 *   the int64 elements d_tpfp holds: below h_offsets[rel_total] is KGE_ERR_BAD_ARG, with h_offsets filled so that the caller
 *   can size the buffer.
 *   d_auc2 (DEVICE int64 [rel_total][2], every element written) = (area2, n_r) for a relation with validation AND split
 *   triples, (0, 0) otherwise: n_r = its triples in the split, area2 = twice the trapezoid area, in counts, under the polyline
 *   (0,0), (FP(0),TP(0)), ..., (FP(n_interval),TP(n_interval)), (n_r,n_r), so AUC = area2 / (2 n_r^2).  An integer sum: the
 *   same for any order of arrival.
 *   Errors as kge_tc_fit's (KGE_ERR_NO_DATASET, KGE_ERR_NO_DEVICE, KGE_ERR_BAD_ARG for a null array, a wrong size, a split
 *   outside {0, 1} or a non-finite validation score, KGE_ERR_UNSUPPORTED for a grid of 2^24 points or more or more than 2^28
 *   int32 histogram bins, hpos and hneg counted, over the relations on the global path); a non-finite score in the split is
 *   KGE_ERR_BAD_ARG too.  On every error NO device output is written.  The call waits ONCE on `stream`, where the fit
 *   waits: behind the min / max pass over the validation scores and a finiteness pass over the split's, for the status and
 *   every relation's n_interval; the binning, the prefix sums and the writes that follow are enqueued and not waited for.
 *   It works in the fit's per-process state (ranges, global histogram, status word), so the fit's rule covers it: ONE
 *   kge_tc_fit or kge_tc_roc at a time -- not from two threads, not enqueued on two streams that may run concurrently. */
int kge_tc_roc(const float *d_vpos, const float *d_vneg, INT n_valid, INT split, const float *d_pos, const float *d_neg, INT n,
               int64_t *d_auc2, int64_t *d_tpfp, INT tpfp_capacity, int64_t *h_offsets, void *stream);

/* predict op: score n triples.  TransE: mean over the dimension (TransE.py:58); others: sum
 * (TransH.py:82, TransR.py:87 with predict_r[0]'s matrix for all, TransD.py:98). */
int kge_predict(const kge_model_desc *m, const float *const tables[KGE_MAX_TABLES], const int32_t *d_h,
                const int32_t *d_t, const int32_t *d_r, INT n, float *d_out, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* KGE_MI355_H */
