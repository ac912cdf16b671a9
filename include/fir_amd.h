/*
 * fir_amd.h -- C ABI of the MI355X (gfx950) gallery matcher.
 *
 * Drop-in boundary for the brute-force / probabilistic match path of
 * av-savchenko/fast-image-recognition (qt_cpp). The reference has no FFI of its own -- the path
 * is plain C++ called in-process -- so each entry point below names the reference function it
 * replaces (path:line under the reference checkout); the C++ host shim in
 * fast-image-recognition_amd/host/ re-creates the reference's classes on top of these calls.
 *
 * Conventions
 *   - plain C types only; `fir_gallery` is an opaque handle; no exceptions cross the boundary;
 *   - every function returns FIR_OK (0) or a negative FIR_ERR_* code; fir_last_error() gives
 *     the message of the calling thread's last failure;
 *   - "not found" is reported the reference's way: index -1 and distance 100000
 *     (qt_cpp/db_features.cpp:322-323, qt_cpp/ann.cpp:115-116);
 *   - the gallery rows are COPIED at create time (the reference only borrows them,
 *     qt_cpp/ImageTesting.cpp:40, qt_cpp/ann.h:28): the caller may free its rows afterwards;
 *   - one handle is used by one host thread at a time (the reference is single threaded);
 *   - `*_dev` variants take DEVICE pointers and a HIP stream (void* = hipStream_t, NULL = the
 *     handle's own stream) and are asynchronous; the others take host pointers and return
 *     when the results are in the caller's buffers;
 *   - there is no CPU fallback: without a usable gfx950 device every call fails.
 */
#ifndef FIR_AMD_H
#define FIR_AMD_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct fir_gallery fir_gallery;

/* The reference's compile-time metric switch (qt_cpp/db_features.h:12,
 * qt_cpp/db_features.cpp:25-39) as a runtime value. */
enum {
    FIR_METRIC_L2 = 0,   /* sum (a-b)^2 / n                          db_features.cpp:26,40  */
    FIR_METRIC_CHI2 = 1, /* sum_{a+b>0} (a-b)^2/(a+b) / n            db_features.cpp:29-31  */
    FIR_METRIC_KL = 2    /* sum a ln(2a/(a+b)) + b ln(2b/(a+b)) / n  db_features.cpp:33-36  */
};

enum {
    FIR_OK = 0,
    FIR_ERR_ARG = -1,      /* bad argument                                   */
    FIR_ERR_HIP = -2,      /* a HIP runtime call failed                      */
    FIR_ERR_NOMEM = -3,    /* host or device allocation failed               */
    FIR_ERR_NODEVICE = -4, /* no gfx950 device / device index out of range   */
    FIR_ERR_STATE = -5,    /* call not valid for this handle (e.g. no labels) */
    FIR_ERR_COMM = -6      /* an RCCL call failed                             */
};

#define FIR_NOT_FOUND_DIST 100000.0f
#define FIR_KEY_NONE 0xFFFFFFFFFFFFFFFFull

const char* fir_last_error(void);
int fir_version(void);

/* Number of visible HIP devices (does not initialise a device context). */
int fir_device_count(void);
/* name[cap] <- gcnArchName; *cus, *hbm_bytes as reported by the runtime. */
int fir_device_info(int32_t device, char* name, int32_t cap, int32_t* cus, int64_t* hbm_bytes);
/* Spec peak HBM bandwidth in GB/s (the denominator of the roofline report): 8000 on gfx950 (MI350X / MI355X). */
int fir_device_peak_hbm_gbs(int32_t device, double* gbs);

/* ---- gallery ------------------------------------------------------------------------------
 * Replaces the `std::vector<ImageInfo>` gallery that Classifier::train (ImageTesting.cpp:40)
 * and ClassificationMethod's constructor (ann.h:11) borrow. rows[n][d] float32 row-major,
 * class_no[n] (may be NULL: then class lookups fail with FIR_ERR_STATE). */
int fir_gallery_create(const float* rows, int64_t n, int32_t d, const int32_t* class_no, int32_t metric,
                       int32_t device, fir_gallery** out);
/* Same, rows/class_no already in this device's memory (row-major); async on `stream`. */
int fir_gallery_create_dev(const float* d_rows, int64_t n, int32_t d, const int32_t* d_class_no, int32_t metric,
                           int32_t device, void* stream, fir_gallery** out);
int fir_gallery_destroy(fir_gallery* g);
int fir_gallery_info(const fir_gallery* g, int64_t* n, int32_t* d, int32_t* metric, int32_t* device);
int fir_gallery_set_metric(fir_gallery* g, int32_t metric);
/* Row-sharded galleries: global index of this shard's row 0 (added to every reported index). */
int fir_gallery_set_row_offset(fir_gallery* g, int64_t first_global_row);

/* ---- in-place updates: append, overwrite and remove rows ---------------------------------------
 * Enrolment, re-enrolment with a better template and removal without a new upload of the gallery. After any sequence of the
 * calls below the handle answers every call as a handle fresh from fir_gallery_create over the array the sequence describes
 * would: the same indices, distance bits, keys, counts, classes and thresholds, for every metric and feature range, in the scan
 * forms and in the routed matrix-core forms. The handle's settings (metric, row offset, tuning, large_batch_mfma, int8 mode,
 * shadow mode, profiling) survive. Two things may read differently from a fresh handle, neither changes an answer:
 * fir_gallery_value_range's gallery_plain is sticky (a value outside the plain range that was overwritten or removed since
 * keeps the full division sequence: the same bits), and the warm-up / learnt-dispatch counters of the automatic matrix-core
 * dispatch start again with every mutation.
 *   Indices are LOCAL rows (as in fir_rows_distances: without the row offset); n + m + row offset must stay below 2^31 - 64.
 *   Labels: a handle with labels requires class_no on append, a handle without refuses it (FIR_ERR_ARG either way); an empty
 * handle (n == 0) takes its labelled-ness from its first append; any int32 is a label.
 *   Checks: NULL, m < 0, m == 0 (nothing to do), labels, index range and duplicates, the 32-bit limit -- before anything is
 * allocated or queued. A call that returns FIR_ERR_ARG, FIR_ERR_STATE or FIR_ERR_NOMEM leaves rows, labels, n, capacity and
 * every answer as they were. A shard lent by fir_sharded_shard refuses every mutation with FIR_ERR_STATE.
 *   Order: a mutation is a call on the handle in the sense of "Streams" below: it takes effect in call order whatever stream each
 * call was given. The host-pointer calls return when the change is in place.
 *   Derived state: what the handle caches about its rows (matrix-core states with their fp16 / int8 / row-major copies, row sums,
 * the label range) is dropped and rebuilt by the next call that wants it: the first routed call after a mutation pays for the
 * copies again (1M x 512, 1 024 queries: 4.2 ms against 1.0 ms in steady state, the cost of a fresh handle's first call). States the CALLER made over the handle (fir_gemm_create*, fir_dem_create) are not rebuilt: every
 * search / recognize / likelihood call on them returns FIR_ERR_STATE ("the gallery changed after this ... state was built")
 * without queueing anything; destroy them and create them again.
 *   Cost: with room reserved an append moves O(m d) bytes and allocates nothing proportional to n; set_rows and remove_rows move
 * O(m d) bytes. When n + m exceeds the capacity the buffers grow to n + m plus a quarter of headroom in whole 64-row tiles
 * (the exact size when the headroom cannot be had, then FIR_ERR_NOMEM): the call first waits for the handle's queued calls,
 * allocates the new buffers, copies on the device and frees the old ones -- old and new buffers exist side by side for that
 * moment. fir_gallery_memory_bytes' `tiled` reports the allocated capacity. Measured (profiles/gallery_update.txt; whole
 * host-pointer calls, 512 features, labelled): appending 64 / 4 096 / 65 536 rows with room reserved 0.09 / 0.23 / 2.6 ms at 100 000
 * and at 1M rows (destroy + create of n + m rows: 39 - 42 ms at 1M, 4.6 - 7.1 ms at 100 000), 1.6 / 1.8 / 4.1 ms when the 1M-row
 * buffers have to grow; set_rows 0.12 / 0.38 ms and remove_rows 0.05 / 0.21 ms for 64 / 4 096 rows at 1M.
 *
 * fir_gallery_reserve: room for at least `rows` rows (and their labels on a labelled handle) without another allocation; never
 * shrinks; rows <= n is a no-op. fir_gallery_capacity: *rows <- the rows the handle holds room for. */
int fir_gallery_reserve(fir_gallery* g, int64_t rows);
int fir_gallery_capacity(const fir_gallery* g, int64_t* rows);
/* rows[m][d] (class_no[m]) become gallery rows n .. n + m - 1, n grows by m. The _dev form reads d_rows / d_class_no on `stream`
 * and is asynchronous; once the capacity is there and the handle's labelled-ness is settled it never synchronises. */
int fir_gallery_append(fir_gallery* g, const float* rows, int64_t m, const int32_t* class_no);
int fir_gallery_append_dev(fir_gallery* g, const float* d_rows, int64_t m, const int32_t* d_class_no, void* stream);
/* Rows row_idx[i] (distinct, < n) take the values new_rows[i][d]; class_no NULL keeps their labels (a handle without labels
 * refuses class_no). */
int fir_gallery_set_rows(fir_gallery* g, const int32_t* row_idx, int32_t m, const float* new_rows, const int32_t* class_no);
/* Swap-remove of the m distinct rows row_idx, deterministic: n' = n - m; the holes are the removed rows below n', ascending; the
 * survivors are the rows of [n', n) that are not removed, ascending (as many as holes); the j-th hole receives the j-th survivor,
 * features and label; every other row keeps its index. moved_from[m] (may be NULL): the former row now at row_idx[i], -1 when
 * row_idx[i] >= n'. fir_gallery_remove_plan is the rule alone -- pure integer work on the host, no device (like
 * fir_keys_unpack) -- with the argument checks: an index outside [0, n), a duplicate, m < 0 give FIR_ERR_ARG. */
int fir_gallery_remove_rows(fir_gallery* g, const int32_t* row_idx, int32_t m, int32_t* moved_from);
int fir_gallery_remove_plan(int64_t n, const int32_t* row_idx, int32_t m, int32_t* moved_from);
/* Rows row0 .. row0 + m - 1 back in row-major form, rows_out[m][d], and their labels (class_out[m], may be NULL; FIR_ERR_STATE when
 * asked for labels the handle does not have). */
int fir_gallery_read_rows(fir_gallery* g, int64_t row0, int64_t m, float* rows_out, int32_t* class_out);

/* ---- single pair ----------------------------------------------------------------------------
 * feature_distance(lhs, rhs, start_pos, end_pos), db_features.cpp:22-42 (ImageInfo::distance,
 * db_features.h:24). len = number of floats in each vector. Computed on the device. */
int fir_feature_distance(const float* lhs, const float* rhs, int32_t len, int32_t start_pos, int32_t end_pos,
                         int32_t metric, int32_t device, float* out);

/* ---- nearest row ---------------------------------------------------------------------------
 * Batched recognize_image_bf (db_features.cpp:319-335) / BruteForce::recognize
 * (ann.cpp:113-126): for each of qb queries, the row with the smallest distance over features
 * [start_pos, end_pos) -- first minimum in row order, strict `<` from 100000. end_pos = 0 means d
 * (the reference's max_features == 0 rule, db_features.cpp:320-321).
 * idx[qb] <- row index (+ row offset) or -1, dist[qb] <- its distance (either may be NULL). */
int fir_search_top1(fir_gallery* g, const float* queries, int32_t qb, int32_t start_pos, int32_t end_pos,
                    int32_t* idx, float* dist);

/* Streams. The *_dev calls (and the fir_gemm_search_*_keys_dev calls below) queue their work on `stream` (NULL: the handle's own
 * stream) and, but for the forms noted below that synchronise `stream` once, return without waiting for it. Calls on ONE gallery handle -- and on the fir_gemm states over it, which share its
 * scratch -- take effect in call order whatever stream each is given: a call on another stream than the handle's previous call
 * first makes its stream wait for that call's end (a device-side wait: the host does not block), and host-pointer calls count as
 * calls on the handle's own stream. Calls on the same stream pay nothing for this but one event record each. Calls on different
 * handles are independent. What a call reads and writes through the caller's pointers is ordered on `stream` only: the caller
 * makes `stream` wait for whatever produced the queries, and waits for `stream` (or fir_gallery_sync) before reading the keys.
 * fir_gallery_sync, fir_gallery_destroy, fir_gemm_destroy, and the settings that free a matrix-core state
 * (fir_gallery_set_large_batch_mfma(g, 0), fir_gallery_set_shadow_copies, fir_gallery_set_row_offset) first wait on the host
 * for the handle's most recent call; so do the in-place updates above that take host pointers, and any of them that has to grow
 * the handle's buffers (fir_gallery_append_dev with room reserved does not wait). After fir_gallery_append_dev the NEXT chi-square
 * / KL search on the handle, its *_keys_dev forms included, synchronises its `stream` once: it has to read whether an appended value
 * left the plain range before it picks its form (the host-pointer updates read that themselves; a growth alone changes no value
 * and causes no such wait).
 *
 * Device-resident form. d_keys[qb] receives one packed key per query:
 *   (orderable(float bits of distance) << 32) | uint32(row index + row offset),
 * FIR_KEY_NONE when no row qualifies. Keys order exactly like (distance, index), so the minimum
 * of the keys of several row shards is the reference's answer on the whole gallery: reduce them
 * with an integer MIN (RCCL all-reduce on uint64/int64), then unpack. */
int fir_search_top1_keys_dev(fir_gallery* g, const float* d_queries, int32_t qb, int32_t start_pos, int32_t end_pos,
                             uint64_t* d_keys, void* stream);
/* Two batch forms synchronise `stream` once before returning (they have to know that their certificate / candidate lists
 * held, and re-run the exact scan for what did not): L2 whole-range batches that take the matrix-core path (see
 * fir_gallery_set_large_batch_mfma) and chi-square batches of >= 8 queries over >= 65536 rows, which take a nomination scan
 * (1-ulp reciprocal, threshold widened by its error bound) + exact re-rank of the appended rows. The keys are the exact
 * scan's either way; fir_gallery_set_tuning(g, 8, 0) pins the exact scan. */
/* Host-side unpack of packed keys (pure integer work, no device). */
int fir_keys_unpack(const uint64_t* keys, int32_t n, int32_t* idx, float* dist);
uint64_t fir_key_pack(float dist, int32_t idx);
/* classNo of each index (BruteForceClassifier::recognize, ImageTesting.cpp:61-67): -1 stays -1.
 * idx are LOCAL+offset indices as returned above. */
int fir_gallery_classes_of(fir_gallery* g, const int32_t* idx, int32_t n, int32_t* class_out);

/* ---- K nearest rows -------------------------------------------------------------------------
 * The K smallest entries of the distance vector of db_features.cpp:325-333, ascending, equal
 * distances by ascending row index; unused slots idx -1 / dist 100000. idx[qb*k], dist[qb*k]. */
int fir_search_topk(fir_gallery* g, const float* queries, int32_t qb, int32_t start_pos, int32_t end_pos, int32_t k,
                    int32_t* idx, float* dist);
/* Batches of >= 8 queries over >= 65536 rows (L2, whole-chunk ranges) take a candidate-list form: a threshold from a
 * row sample, an append scan at the speed of the top-1 scan, the K smallest of each list -- the same keys; that form
 * synchronises `stream` once before returning (it has to know that no list overflowed; if one did, the register-list
 * scan answers instead). */
int fir_search_topk_keys_dev(fir_gallery* g, const float* d_queries, int32_t qb, int32_t start_pos, int32_t end_pos,
                             int32_t k, uint64_t* d_keys /* [qb*k] ascending */, void* stream);

/* ---- K nearest distinct classes ---------------------------------------------------------------
 * The k nearest DISTINCT classes of each query: for every class c in [0, num_classes) its nearest row
 * (first minimum in row order, the rule of db_features.cpp:329-332) over features [start_pos, end_pos)
 * (end_pos = 0: d), then the k classes whose nearest rows are nearest, ascending by (distance, row index):
 * the best row of every class and then the best classes of ConventionalTWDClassifier::recognize
 * (ImageTesting.cpp:118-122, 141-149) for any metric, range and k -- rank-k candidates, not k rows of one class.
 * 1 <= k <= 32, 1 <= num_classes <= 16777216 (else FIR_ERR_ARG). class_out / idx / dist are [qb*k], any may be NULL; unused slots: class -1, idx -1, dist 100000.
 * The gallery needs class labels (else FIR_ERR_STATE). Rows labelled outside [0, num_classes) take no part
 * (as in fir_twd_conventional). A row qualifies only if `dist < 100000.0f` is true (so NaN distances never do).
 * One exact gallery scan per 8 queries (the arithmetic and distance bits of fir_search_top1's scan). fir_search_top_classes (the
 * host-pointer call) sends an L2 batch over features [0, end_pos) -- whole rows, or a prefix with end_pos % 16 == 0, end_pos >= 64 --
 * of a labelled gallery through fir_gemm_search_top_classes_keys_dev instead, same classes, rows and distance bits: by default
 * from 128 queries against 65536 rows on (3.9 - 6.5 x the scan's rate at 1M x 512, 100 000 classes, 128 .. 32 768 queries per call: profiles/class_rank_matrix_cores.txt),
 * with fir_gallery_set_large_batch_mfma(g, min_queries > 0) from the caller's threshold on at any gallery size, never after
 * fir_gallery_set_large_batch_mfma(g, 0) or with FIR_SHADOW_NONE; fir_search_top_classes_keys_dev always takes the scan.
 * Device scratch of the scan: 64 bytes per class and 8 queries, and the select step reads a query's 8 bytes per class twice with one
 * workgroup: with num_classes in the millions that read, not the scan, sets the time of a call of few queries. */
int fir_search_top_classes(fir_gallery* g, const float* queries, int32_t qb, int32_t start_pos, int32_t end_pos,
                           int32_t num_classes, int32_t k, int32_t* class_out, int32_t* idx, float* dist);
/* Device-resident, asynchronous on `stream`, never synchronises once its scratch is large enough.
 * d_keys[qb*k]: packed keys of the winning rows (index + row offset), ascending, FIR_KEY_NONE for unused slots;
 * d_classes[qb*k]: their classes, -1 for unused slots. One of the two may be NULL. */
int fir_search_top_classes_keys_dev(fir_gallery* g, const float* d_queries, int32_t qb, int32_t start_pos, int32_t end_pos,
                                    int32_t num_classes, int32_t k, uint64_t* d_keys, int32_t* d_classes, void* stream);
/* Host-side merge of `parts` such lists (keys[parts][qb][k], classes likewise: row shards made with
 * fir_gallery_set_row_offset, or ranks): per class the smallest key, then the k smallest. Pure integer work, no device.
 * Exact: a class among the global k best is among the k best of the shard that holds its nearest row -- every class
 * ahead of it in that shard is ahead of it globally too. */
int fir_class_keys_merge(const uint64_t* keys, const int32_t* classes, int32_t parts, int32_t qb, int32_t k,
                         uint64_t* keys_out, int32_t* classes_out);

/* ---- the K nearest rows, K up to 1024 ---------------------------------------------------------
 * fir_search_topk's result for 1 <= k <= FIR_KNN_MAX (else FIR_ERR_ARG, "k=%d outside [1,1024]"): per query the k smallest
 * packed keys (orderable(distance bits) << 32) | uint32(row + row offset), ascending -- equal distances by ascending row --
 * over features [start_pos, end_pos) (end_pos = 0: d), any metric. A row qualifies only if `dist < 100000.0f` is true (so NaN
 * distances never do); unused slots -- k > n, an empty gallery, fewer than k qualifying rows -- hold FIR_KEY_NONE (idx -1,
 * dist 100000). For k <= 8 the keys are fir_search_topk_keys_dev's bit for bit, and for any k the first k' keys are those of the
 * k' call. idx and dist are [qb*k], both required. Arguments are checked in the order of the other searches (NULL, qb < 0, k,
 * qb == 0: nothing to do, the range) before anything is allocated or queued.
 * Form: per tile of up to 8 queries ONE exact gallery scan stores the tile's distances (fir_range_distances' pass and bits) in
 * the handle's scratch, then a radix select over the 64-bit keys finds each query's k-th smallest key, and the keys up to it are
 * sorted. Keys are unique (the row is part of them), so the k-th key names one row however many rows share its distance: the
 * result is exact under ties and two calls return the same bytes. Device scratch: 4 bytes per row and query of ONE tile plus
 * 130 KiB, whatever qb is (counted under `scratch` in fir_gallery_memory_bytes); when a tile of 8 cannot be had the tile is
 * halved down to one query before the call fails with FIR_ERR_NOMEM. The select re-reads the stored distances, not the gallery:
 * timed by its own event pair it is 14-20 % of store + select at 1M x 512 for k <= 256 and 32 % at k = 1024; at 100 000 x 512, where
 * the scan of a tile takes 0.065 ms, it is 45-70 % (profiles/knn_select.txt). Every call in this form pays one exact scan per 8
 * queries whatever the batch size.
 * Matrix-core form: an L2 batch with k <= FIR_GEMM_KNN_MAX over features [0, end_pos) -- whole rows, or a prefix with end_pos % 16 == 0
 * and end_pos >= 64 -- goes through fir_gemm_search_knn_keys_dev (same keys, see there) as fir_search_top_classes routes its batches:
 * with fir_gallery_set_large_batch_mfma(g, min_queries > 0) from the caller's threshold on, at any gallery size; never with threshold
 * 0 or FIR_SHADOW_NONE; by itself for 8 < k <= 256 from 128 queries over >= 65536 rows on, as for classes -- every measured k
 * (9 .. 256) was at least 1.15 x store + select at 1 024 queries and not slower at 128, at 1M x 512 (128 / 1 024 / 8 192 queries:
 * k = 9 9.2 / 21 / 23 x, k = 64 4.7 / 10 / 11 x, k = 256 1.6 / 2.1 / 2.2 x) and at 100 000 x 512 (k = 9 3.7 / 8.6 / 8.4 x, k = 256
 * 1.6 / 5.8 / 5.6 x; profiles/knn_matrix_cores.txt). Such a call synchronises the handle's stream once more than store + select
 * does and costs the fp16 gallery copy (n*d*2 bytes, created on first use). fir_search_knn_keys_dev and fir_sharded_search_knn
 * always keep the store + select form.
 * fir_gallery_last_dispatch does not describe a store + select call; a routed call it describes as it does a routed class call
 * (path mfma, the f16x<1, ...> append pass). With fir_profile_enable on, fir_profile_read returns two durations per tile of queries,
 * in call order -- the tile's store pass (query transposition + scan), then its select -- for the store + select form only; a
 * routed call leaves the append pass's launches (and the two-per-tile pairs of whatever queries it could not certify). */
#define FIR_KNN_MAX 1024
int fir_search_knn(fir_gallery* g, const float* queries, int32_t qb, int32_t start_pos, int32_t end_pos, int32_t k,
                   int32_t* idx, float* dist);
/* Device-resident, asynchronous on `stream` (NULL: the handle's own), in the handle's call order like every *_dev call; never
 * synchronises once its scratch is large enough. d_keys[qb*k] ascending per query, FIR_KEY_NONE for unused slots. */
int fir_search_knn_keys_dev(fir_gallery* g, const float* d_queries, int32_t qb, int32_t start_pos, int32_t end_pos, int32_t k,
                            uint64_t* d_keys, void* stream);

/* ---- every row within a per-query radius --------------------------------------------------------
 * The exhaustive answer behind the reference's acceptance rules, which are distance thresholds: DirectedEnumeration stops at the
 * first row with bestDistance < threshold (ann.cpp:390-400), getThreshold places that threshold at a false-accept rate over
 * other-class distances (ann.cpp:84-93), ProposedTWDClassifier keeps the rows within best / threshold (ImageTesting.cpp:256-266).
 * Per query q, over features [start_pos, end_pos) (end_pos = 0: d), any metric: a row qualifies iff `dist < radius[q]` and
 * `dist < 100000.0f` are both true as float compares -- the strict < of ann.cpp:396 and the cut-off of every other search. NaN
 * distances never qualify; a NaN, zero or negative radius qualifies nothing; a radius >= 100000 (+inf included) qualifies every
 * row fir_search_knn would consider. count[q] <- the number of qualifying rows, exact however large, never capped by max_results.
 * idx / dist [qb*max_results] <- the min(count[q], max_results) smallest packed keys (orderable(distance bits) << 32) |
 * uint32(row + row offset) of the qualifying rows, ascending -- equal distances by ascending row --, FIR_KEY_NONE (idx -1,
 * dist 100000) behind them: with radius = +inf they are fir_search_knn's for k = max_results bit for bit, and two calls return
 * the same bytes. 0 <= max_results <= FIR_KNN_MAX (else FIR_ERR_ARG, "max_results=%d outside [0,1024]"); 0 is the count-only
 * call, where idx and dist must be NULL; otherwise both are required. count and radius [qb] are always required. Arguments are
 * checked in the order of the other searches (NULL, qb < 0, max_results, qb == 0: nothing to do, the range) before anything is
 * allocated or queued. An empty gallery: counts 0, every slot FIR_KEY_NONE.
 * Form: fir_search_knn's store + select with a count in between. Per tile of up to 8 queries ONE exact gallery scan stores the
 * tile's distances (fir_range_distances' pass and bits); a count kernel reads them once (4 bytes per row and query) and leaves each
 * query's number of qualifying rows; the radix select then runs with each query's own rank min(count, max_results), read on the
 * device: a query whose qualifying rows all fit needs no digit passes (its threshold is "everything that qualifies"), max_results
 * = 0 stops after the count. Scratch and its halving as for fir_search_knn. With fir_profile_enable on, fir_profile_read returns
 * two durations per tile of queries: the store pass, then count + select + sort. fir_gallery_last_dispatch does not describe it.
 * Matrix-core form: an L2 batch with max_results <= FIR_GEMM_KNN_MAX over features [0, end_pos) -- whole rows, or a prefix with
 * end_pos % 16 == 0 and end_pos >= 64 -- goes through fir_gemm_search_radius_keys_dev (same counts and keys, see there) ONLY with
 * fir_gallery_set_large_batch_mfma(g, min_queries > 0), from the caller's threshold on, as fir_search_knn routes under a
 * threshold; never with threshold 0 or FIR_SHADOW_NONE, and never by itself. fir_gallery_last_dispatch describes a routed call as
 * it does a routed fir_search_knn call. Why the default is "never" (profiles/radius_search.txt: whole host-pointer calls at 100 000 x
 * 512 and 1M x 512, 128 / 1 024 / 8 192 queries, radii at the K-th distance, K in {1, 9, 64, 256}, max_results = K): the matrix-core
 * form is 1.75 - 74 x the store + count + select form at every such point, but a default needs 1.15 x at every point of a class the
 * code can observe (queries, rows, max_results) AND an overflow case that loses no more than the spread -- and with 1 000 rows
 * inside the radius (max_results 256) it is 0.78 x at 100 000 rows and 128 queries, and with a radius that overflows every list
 * (4 096 entries; every query is then answered twice) 0.12 / 0.64 / 0.78 x at 100 000 rows and 0.09 / 0.48 / 0.64 x at 1M. How many
 * rows lie near a radius is not visible beforehand. A later default would rest on a cheap count estimate and the same measurements
 * (tools/radius_search_probe.py). The store + count + select form itself takes 0.83 - 0.96 x the time of fir_search_knn(k =
 * max_results)'s store + select while the count fits max_results and 1.03 - 1.10 x when it does not.
 * fir_search_radius_keys_dev and fir_sharded_search_radius always keep the store + count + select form. */
int fir_search_radius(fir_gallery* g, const float* queries, int32_t qb, int32_t start_pos, int32_t end_pos,
                      const float* radius, int32_t max_results, int32_t* count, int32_t* idx, float* dist);
/* Device-resident, asynchronous on `stream` (NULL: the handle's own), in the handle's call order like every *_dev call; never
 * synchronises once its scratch is large enough. d_radius[qb], d_count[qb]; d_keys[qb*max_results] ascending per query,
 * FIR_KEY_NONE for unused slots (NULL with max_results = 0). */
int fir_search_radius_keys_dev(fir_gallery* g, const float* d_queries, int32_t qb, int32_t start_pos, int32_t end_pos,
                               const float* d_radius, int32_t max_results, int32_t* d_count, uint64_t* d_keys, void* stream);

/* ---- the nearest row of another class -------------------------------------------------------------
 * The primitive behind the reference's false-accept threshold (otherClassesDists, ann.cpp:286-298: for every gallery row the
 * distance to the nearest row of another class), leave-own-class-out evaluation, impostor mining and the "best row of another
 * class" ConventionalTWDClassifier keeps next to its best row (ImageTesting.cpp:123-131).
 * Per query q, over features [start_pos, end_pos) (end_pos = 0: d), any metric: a row qualifies iff `class_no[row] !=
 * exclude_class[q]` (a plain int32 compare: any value is a legal label or exclusion, negatives, INT32_MIN and INT32_MAX included)
 * and `dist < 100000.0f` is true (so NaN distances never qualify). The answer is the smallest packed key (orderable(distance
 * bits) << 32) | uint32(row + row offset) among the qualifying rows -- the first-minimum rule of db_features.cpp:329-332 over those
 * rows --, FIR_KEY_NONE (idx -1, dist 100000) when there is none. An exclude_class[q] no row carries gives fir_search_top1_keys_dev's
 * key bit for bit; the distance bits are the exact scan's (fir_range_distances'). The gallery needs class labels (else
 * FIR_ERR_STATE). idx, dist and exclude_class are [qb], all required. Arguments are checked in fir_search_top_classes' order (NULL,
 * qb < 0, the labels, the range, qb == 0: nothing to do) before anything is allocated or queued.
 * Form: one exact gallery scan per tile of up to 8 queries -- the generic top-1 scan with one more compare per (row, query): the
 * tile's 64 labels come in one coalesced load ahead of the features, the tile's excluded classes through the scalar cache from a
 * copy padded to whole tiles in the handle's scratch. fir_gallery_last_dispatch describes it (k_scan<..., 6, ...>).
 * Matrix-core form (no pass of its own): the nearest row of a class other than c is the best row of the best class other than c,
 * which is rank 1 or 2 among all classes -- the first of fir_gemm_search_top_classes_keys_dev(k = 2)'s two entries whose class
 * differs from c, the same key bit for bit. fir_search_top1_other_class (the host-pointer call) and the host calls of the
 * self-join below send a batch that way where fir_search_top_classes would route a batch of that size and range, when every label
 * of the gallery lies in [0, 16777216) (found once by a reduction over the labels; num_classes = largest label + 1): by default
 * from 128 queries against 65536 rows on, with fir_gallery_set_large_batch_mfma(g, min_queries > 0) from the caller's threshold on
 * at any gallery size, never after fir_gallery_set_large_batch_mfma(g, 0) or with FIR_SHADOW_NONE. The default rests on whole
 * host-pointer calls of 128 / 1 024 / 8 192 queries, 10 rows per class (profiles/other_class.txt, tools/other_class_probe.py): at
 * 100 000 x 512 the routed form is 3.8 / 7.7 / 8.7 x the scan form on class-major labels and 3.1 / 4.9 / 5.3 x on permuted ones, at
 * 1M x 512 5.5 / 7.7 / 7.9 x and 4.8 / 6.6 / 6.7 x, the same answers, no query left to the exact class scan -- every point beyond the
 * 1.15 x an automatic route needs. Such a call synchronises the handle's stream and costs the fp16 gallery copy (n*d*2 bytes,
 * created on first use). fir_gallery_last_dispatch describes a routed call as it does a routed class call. The *_dev call always
 * takes the scan form; against the exact top-1 scan of the same batch (8 queries per pass) that form takes 1.00 - 1.02 x the time
 * at 1M x 512, where both wait for HBM, and 1.15 - 1.41 x at 100 000 x 512, where the rows sit in the caches and the top-1 call
 * runs the hand-scheduled packed kernel, which has no form with this epilogue; over features [1, 512), where the top-1 call runs
 * the generic scan too, 0.98 - 1.06 x (same file). */
int fir_search_top1_other_class(fir_gallery* g, const float* queries, int32_t qb, int32_t start_pos, int32_t end_pos,
                                const int32_t* exclude_class /* [qb] */, int32_t* idx, float* dist);
/* Device-resident, asynchronous on `stream` (NULL: the handle's own), in the handle's call order like every *_dev call; never
 * synchronises once its scratch is large enough. d_exclude_class[qb], d_keys[qb]. */
int fir_search_top1_other_class_keys_dev(fir_gallery* g, const float* d_queries, int32_t qb, int32_t start_pos, int32_t end_pos,
                                         const int32_t* d_exclude_class, uint64_t* d_keys, void* stream);
/* The gallery against itself: d_keys[i] = the key of row row0 + i searched with ITSELF as the query and its own class excluded,
 * i < m (so the row itself never answers); rows are taken in blocks of up to 8 192 from the tiled copy, no other copy of the
 * gallery is needed. Argument order: this is feature_distance(row i, row j) -- row i is the query --, the reference's table entry
 * is distance(dbImages[j], i) = feature_distance(row j, row i): the same bits for L2 and chi-square ((a-b)^2 = (b-a)^2, a+b
 * commutes); for KL the two terms of a feature are added in the other order, and the contract here is "row i is the query".
 * FIR_ERR_ARG unless 0 <= row0, 0 <= m, row0 + m <= n; FIR_ERR_STATE without labels. Asynchronous on `stream`, scan form. */
int fir_gallery_other_class_keys_dev(fir_gallery* g, int64_t row0, int64_t m, int32_t start_pos, int32_t end_pos,
                                     uint64_t* d_keys /* [m] */, void* stream);
/* ... of every row, unpacked: idx / dist [n], both required (-1 / 100000 for a row with no row of another class). */
int fir_gallery_other_class(fir_gallery* g, int32_t start_pos, int32_t end_pos, int32_t* idx /* [n] */, float* dist /* [n] */);
/* getThreshold (ann.cpp:84-93) over that statistic (ann.cpp:286-298), on the device: rows_counted = the rows that have a row of
 * another class (the reference's build pushes nothing for the others); ind = (int)((float)rows_counted * false_accept_rate), a
 * float product as the reference's size_t * float; threshold = the (ind + 1)-th smallest of the rows_counted distances; min_dist /
 * max_dist = the two other numbers the reference prints. min_dist, max_dist and rows_counted may be NULL. FIR_ERR_ARG: a NaN or
 * negative rate, or ind >= rows_counted (a rate of 1.0 indexes past the end in the reference); FIR_ERR_STATE: rows_counted == 0, or
 * no labels. One host synchronisation, at the end (scan form; a routed block synchronises by itself). Whole calls at rate 0.01
 * (profiles/other_class.txt): 100 000 x 512 0.81 s in the scan form and 0.09 s routed; 1M x 512 5.0 s routed -- the scan form is one
 * exact scan per 8 rows of the gallery, about n / 26 000 s there, and was not run. */
int fir_gallery_far_threshold(fir_gallery* g, int32_t start_pos, int32_t end_pos, float false_accept_rate,
                              float* threshold, float* min_dist, float* max_dist, int64_t* rows_counted);

/* ---- searches over a subset of the rows ---------------------------------------------------------
 * "This handle, these rows only": the random train / test splits of the reference's experiments (getTrainingAndTestImages,
 * db_features.cpp:117-162, called TESTS times by testRecognitionMethod, ImageTesting.cpp:445-466), watch-lists, consent or expiry
 * flags, soft delete without fir_gallery_remove_rows' renumbering, leave-several-classes-out evaluation -- over ONE upload of the
 * whole set, a subset being n / 8 bytes.
 * The mask: FIR_MASK_WORDS(n) 64-bit words, n = the handle's row count at the time of the call (after in-place updates: the current
 * n, whatever the capacity). LOCAL row r (without the row offset, as in fir_rows_distances and the update calls; on a shard lent by
 * fir_sharded_shard: the shard's local row) takes part iff bit r & 63 of word r >> 6 is set. Bits at or past n in the last word are
 * ignored, whatever they hold. The mask must be 8-byte aligned. Keys still carry row + row offset.
 * A row qualifies iff its bit is set AND it qualifies in the unmasked call of the same name; everything else is the unmasked
 * call's contract word for word: ordering, the first-minimum rule, padding with FIR_KEY_NONE (idx -1, dist 100000; class -1), exact
 * counts never capped by max_results, `dist < 100000.0f`, NaN never qualifying, which outputs may be NULL. Equivalently: the answer
 * of a handle freshly created over the selected rows in their order, every returned row mapped back to its index in the full
 * gallery (the map is monotone, so ties keep their order; the distance bits are fir_range_distances'). A class with no masked-in
 * row does not appear in a class answer. An all-ones mask gives the unmasked call's bytes.
 * Each call has its unmasked sibling's arguments with the mask directly after end_pos. A NULL mask is FIR_ERR_ARG unless n == 0:
 * the mask is then not read and the unmasked empty-gallery results apply. Arguments are checked in the sibling's order, the mask
 * among the NULL checks, before anything is allocated or queued. fir_search_knn_masked: 1 <= k <= FIR_KNN_MAX; for k <= 8 it is also
 * the masked fir_search_topk (the same keys), there is no separate call. fir_search_radius_masked: the counts count masked-in rows
 * only; max_results = 0 stays the count-only call.
 * Form: a masked call ALWAYS takes the exact scan form of its kind -- the generic scan (k_scan<..., MASKED = 1>) with the top-1
 * epilogue, the store pass of store + select (+ count), or the class-minimum scan + select. It never takes the matrix-core routes,
 * the int8 or fp16 nomination, the chi-square / KL nomination lists of the top-1 call or the hand-scheduled L2 kernels, whatever
 * fir_gallery_set_large_batch_mfma and the batch size say (as fir_search_top1_other_class_keys_dev always takes the scan): none of
 * those has a masked form. A 64-row tile is one mask word: the scan reads it once per tile through the scalar cache; a tile none
 * of whose rows below n has its bit set is not read at all (the store pass writes 100000 for its rows, which count and select
 * reject), every other tile is read whole. A mask much sparser than one row per tile therefore still reads every tile it touches;
 * there is no gather form. fir_gallery_last_dispatch describes a masked top-1 and class call by the kernel instantiation that ran
 * (path 0, "fir::k_scan<..., 0, 1>": the last template argument is MASKED); a masked kNN / radius call it does not describe, like
 * the unmasked one. fir_profile_read's bytes_per_launch is the unmasked figure plus the mask words: the host cannot know how many
 * tiles a device mask skips without a synchronisation, so skipped tiles are still counted.
 * Measured (profiles/masked_search.txt, tools/masked_search_probe.py: whole host-pointer calls, L2, 512 features, 100 000 and 1M rows,
 * 8 / 128 / 1 024 queries): the all-ones mask takes 0.98 - 1.05 x the time of the unmasked generic scan (top-1 and kNN); a clustered mask
 * (runs of 16 whole tiles) of density 1/64 takes 0.06 - 0.13 of the all-ones top-1 time from 128 queries on, one of density 1/8 0.12 - 0.19 at
 * 100 000 rows but 0.61 at 1M rows, where the probe's 128-tile period divides the 3 072 waves of a pass and an eighth of the waves read
 * everything (a wave strides over the tiles); scattered masks read nearly every tile (0.97 - 1.10 at 1/2 and 1/8); masked kNN at k = 64 stays
 * within 0.70 - 1.02 of all-ones, its select reading 4 bytes per row and query whatever the mask. A second handle over the compacted rows
 * answers a large L2 batch far faster once it is uploaded (it may take the matrix cores); the mask saves the copy and the upload.
 * Left out: masked calls on fir_sharded handles (shards are whole 64-row tiles, so the words can be sliced by shard
 * later); masked matrix-core forms; a gather form for very sparse masks; masked other-class search (fir_gallery_mask_of_classes
 * with invert = 1 composes it); masks for fir_cls / TWD / DEM. */
#define FIR_MASK_WORDS(n) (((n) + 63) / 64)
int fir_search_top1_masked(fir_gallery* g, const float* queries, int32_t qb, int32_t start_pos, int32_t end_pos,
                           const uint64_t* mask, int32_t* idx, float* dist);
int fir_search_knn_masked(fir_gallery* g, const float* queries, int32_t qb, int32_t start_pos, int32_t end_pos,
                          const uint64_t* mask, int32_t k, int32_t* idx, float* dist);
int fir_search_radius_masked(fir_gallery* g, const float* queries, int32_t qb, int32_t start_pos, int32_t end_pos,
                             const uint64_t* mask, const float* radius, int32_t max_results, int32_t* count, int32_t* idx, float* dist);
int fir_search_top_classes_masked(fir_gallery* g, const float* queries, int32_t qb, int32_t start_pos, int32_t end_pos,
                                  const uint64_t* mask, int32_t num_classes, int32_t k, int32_t* class_out, int32_t* idx, float* dist);
/* The host forms above copy the mask into the handle's scratch. The device forms read d_mask on `stream` (NULL: the handle's own),
 * are asynchronous, take effect in the handle's call order ("Streams") and never synchronise once the scratch is large enough; a
 * mask written on the same stream just before -- by fir_gallery_mask_of_classes_dev, say -- needs no synchronisation in between. */
int fir_search_top1_masked_keys_dev(fir_gallery* g, const float* d_queries, int32_t qb, int32_t start_pos, int32_t end_pos,
                                    const uint64_t* d_mask, uint64_t* d_keys, void* stream);
int fir_search_knn_masked_keys_dev(fir_gallery* g, const float* d_queries, int32_t qb, int32_t start_pos, int32_t end_pos,
                                   const uint64_t* d_mask, int32_t k, uint64_t* d_keys, void* stream);
int fir_search_radius_masked_keys_dev(fir_gallery* g, const float* d_queries, int32_t qb, int32_t start_pos, int32_t end_pos,
                                      const uint64_t* d_mask, const float* d_radius, int32_t max_results, int32_t* d_count,
                                      uint64_t* d_keys, void* stream);
int fir_search_top_classes_masked_keys_dev(fir_gallery* g, const float* d_queries, int32_t qb, int32_t start_pos, int32_t end_pos,
                                           const uint64_t* d_mask, int32_t num_classes, int32_t k, uint64_t* d_keys,
                                           int32_t* d_classes, void* stream);
/* The mask of a class filter: bit r = (class_no[r] is one of classes[0, m)) XOR (invert != 0), bits past n in the last word zero.
 * Any int32 is a class; m = 0 is legal and gives all zeros, or all ones with invert. FIR_ERR_STATE without labels; an empty gallery
 * has no word to write. The host form has everything in host memory (mask_out [FIR_MASK_WORDS(n)]) and sorts a copy of `classes`
 * itself; one synchronisation. The device form is asynchronous on `stream`; d_classes must be ascending, duplicates allowed -- this
 * is not checked. One wave per tile, a binary search per row. */
int fir_gallery_mask_of_classes(fir_gallery* g, const int32_t* classes, int32_t m, int32_t invert, uint64_t* mask_out);
int fir_gallery_mask_of_classes_dev(fir_gallery* g, const int32_t* d_classes, int32_t m, int32_t invert, uint64_t* d_mask_out,
                                    void* stream);

/* ---- device-side subsets of a gallery: compact by mask or row list, map back ------------------------
 * A masked call always takes the exact generic scan. A NEW handle over the selected rows takes every routed form there is (the
 * hand-scheduled kernels, the fp16 / int8 matrix-core top-1, top-K, kNN, classes, radius, other-class, the conventional TWD), and
 * building it here costs one gather inside HBM instead of a host-side compaction and an upload: the random train / test splits of
 * the reference's experiments (a dense mask, a large L2 batch per split), bootstrap samples and medoid-only galleries (row lists
 * with repeats, which no mask expresses). Rows are LOCAL rows of the source throughout, as in the masked searches.
 *
 * fir_gallery_rows_of_mask: *count = the exact number of set bits below n (bits at or past n are ignored), rows_out[0 ..
 * min(count, cap)) = those rows ascending; rows_out == NULL with cap == 0 is the count-only call. A NULL mask is FIR_ERR_ARG
 * unless n == 0 (count 0). The _dev form has everything in device memory (d_count one int64), is asynchronous on `stream`, runs in
 * the handle's call order ("Streams") and never synchronises once the handle's scratch is large enough. Three small launches over
 * the FIR_MASK_WORDS(n) words -- popcounts per 64 words, an exclusive scan of those sums in one workgroup, then every wave scans
 * its 64 popcounts with shuffles and every lane writes the set bits of its word at its prefix -- with plain stores and no
 * atomics: two calls return the same bytes.
 *
 * fir_gallery_gather_rows_dev: d_rows_out[m][d] row-major = rows d_row_idx[0 .. m) of the handle (any order, repeats allowed),
 * d_class_out[m] (may be NULL; FIR_ERR_STATE on a non-empty handle without labels) their labels: queries taken from the upload
 * itself, no host round trip. Asynchronous. An index outside [0, n) gives a row of zeros and label -1 -- a device call cannot
 * fail late.
 *
 * fir_gallery_create_from_rows[_dev] / fir_gallery_create_subset[_dev]: *out = a new, independent handle on the source's device
 * holding rows row_idx[0 .. m) of src in that order -- the mask forms: the rows the mask selects, ascending, the list never leaving
 * the device -- with their labels iff src has labels. It answers every call with the bytes of a handle made by fir_gallery_create
 * over rows[row_idx] and class_no[row_idx] with the source's metric: every metric, range, scan form and routed form. It starts with
 * default settings and row offset 0 and owns its memory: the source may be changed or destroyed afterwards; source and subset exist
 * side by side, which is the only extra memory. The chi-square / KL plain-range flag is recomputed from the gathered values (a
 * subset that leaves the offending rows out is plain again), and the layout invariant holds (rows at or beyond m and features beyond
 * d are zero: the gather writes every float4 of tiles [0, ceil(m / 64))). m == 0 or a mask without a set bit gives an empty handle,
 * like fir_gallery_create with n = 0; m must stay below 2^31 - 64. The host list form checks every index before anything is allocated
 * (FIR_ERR_ARG, the message names it); the device list form writes a row of zeros with label -1 for an index outside [0, n), and
 * keys that name such a row map to FIR_KEY_NONE below. A NULL mask is FIR_ERR_ARG unless n == 0. Creation is a call on src in the
 * sense of "Streams": it sees an earlier fir_gallery_append_dev on any stream; like fir_gallery_create_dev it synchronises before
 * it returns (the mask forms twice: they read the count first). A shard lent by fir_sharded_shard may be the source -- creation
 * only reads it. Not offered: fir_sharded sources as a whole, subsets of fir_cls handles.
 *
 * Where the rows came from. The new handle keeps its row list on the device (4 bytes per row, under `scratch` in
 * fir_gallery_memory_bytes) and the source's row offset at creation time. fir_gallery_origin_rows: rows_out[0 .. m) = the source's
 * LOCAL rows of the handle's rows [row0, row0 + m). fir_keys_to_origin_dev rewrites d_keys[0 .. count) in place, asynchronously, as
 * a call on the subset handle: a key's low word r + the subset's own row offset becomes origin[r] + the source's offset, the
 * distance bits stay, FIR_KEY_NONE stays; a low word outside the handle's rows becomes FIR_KEY_NONE. fir_keys_map_rows is the same
 * map as pure host code (no device, like fir_keys_unpack) over a caller's table: low word r -> uint32(row_map[r] + row_add); a low
 * word at or beyond m is FIR_ERR_ARG and nothing is written.
 * A mask subset's map is strictly increasing, so mapped keys stay ascending and ties keep their order: they are the bytes of the
 * _masked call of the same name on the source. That equality is the contract. An arbitrary list keeps each query's order by
 * distance only (equal distances may come out in another row order than a masked call's), and repeated rows give equal keys.
 * A handle not made by these calls: FIR_ERR_STATE. So is a subset handle after an in-place update of its own (fir_gallery_append /
 * _set_rows / _remove_rows): its rows are no longer the list's. The origin is the immediate source's: subsets of subsets do not
 * compose (map twice). The library's _masked calls never compact by themselves -- that would double the memory silently.
 * Measured: profiles/gallery_subset.txt (tools/subset_probe.py). */
int fir_gallery_rows_of_mask(fir_gallery* g, const uint64_t* mask, int32_t* rows_out, int64_t cap, int64_t* count);
int fir_gallery_rows_of_mask_dev(fir_gallery* g, const uint64_t* d_mask, int32_t* d_rows_out, int64_t cap, int64_t* d_count,
                                 void* stream);
int fir_gallery_gather_rows_dev(fir_gallery* g, const int32_t* d_row_idx, int64_t m, float* d_rows_out, int32_t* d_class_out,
                                void* stream);
int fir_gallery_create_from_rows(fir_gallery* src, const int32_t* row_idx, int64_t m, fir_gallery** out);
int fir_gallery_create_from_rows_dev(fir_gallery* src, const int32_t* d_row_idx, int64_t m, void* stream, fir_gallery** out);
int fir_gallery_create_subset(fir_gallery* src, const uint64_t* mask, fir_gallery** out);
int fir_gallery_create_subset_dev(fir_gallery* src, const uint64_t* d_mask, void* stream, fir_gallery** out);
int fir_gallery_origin_rows(fir_gallery* sub, int64_t row0, int64_t m, int32_t* rows_out);
int fir_keys_to_origin_dev(fir_gallery* sub, uint64_t* d_keys, int64_t count, void* stream);
int fir_keys_map_rows(uint64_t* keys, int64_t count, const int32_t* row_map, int64_t m, int64_t row_add);

/* ---- linear projection / PCA ------------------------------------------------------------------
 * The device side of extract_pca_features (classification.cpp:864-940) and extractPCA (db_features.cpp:218-315): the feature
 * statistics and the scatter matrix of the rows a mask selects, and a linear map (an eigenvector basis, or any p x d matrix)
 * applied to every row of a handle into a new handle. The eigen-decomposition of the d x d matrix is the caller's (host/fir_eigen.h
 * has one). Masks are host words as in "searches over a subset of the rows": FIR_MASK_WORDS(n) of them, bits at or past n ignored,
 * NULL = every row. Every call takes part in the handle's call order ("Streams"); the host-pointer calls synchronise before
 * they return. An empty gallery is FIR_ERR_ARG for all of them.
 *
 * All sums are float64 over exactly widened f32 values. The rows are cut into fixed segments of whole tiles (a function of n and d
 * alone), every segment's partial result is written to scratch and a second small kernel folds the partials in ascending segment
 * order: no floating-point atomics, two calls return the same bytes.
 *
 * fir_gallery_feature_stats -- split_train_test's statistics (classification.cpp:969-989) over the selected rows, per feature:
 *   *count = the selected rows; min / max exact, starting from FLT_MAX / -FLT_MAX as the reference does; avg = sum(x) / count;
 *   std = sqrt((sum(x^2) - avg * avg * count) / (count - 1)), evaluated literally, un-fused, in IEEE double on the host from the
 *   device's two sums -- whatever that yields for count 0 or 1. Each output array holds d doubles and may be NULL.
 *
 * fir_gallery_scatter -- S[a][b] = sum_j (x_ja - c_a)(x_jb - c_b) over the selected rows, the numerator of the covariance (the caller
 *   divides by count or count - 1). center NULL: c = the mean of the selected rows (the column sums above / count; zeros when no row
 *   is selected), returned in mean_out. The products run on the float64 matrix cores; only the 64 x 64 feature blocks a <= b are
 *   computed and the other triangle is mirrored: S is symmetric bit for bit. d <= 4096. Scratch (owned by the handle, reported by
 *   fir_gallery_memory_bytes): segments x computed blocks x 32 KiB of partials, held at or below 256 MiB by the choice of the segment
 *   count (at least one segment; d = 4096 has 2080 blocks, 65 MiB a segment), plus d x d x 8 bytes for S itself. It is reserved
 *   before anything is queued: FIR_ERR_NOMEM leaves the handle as it was.
 *
 * fir_projection -- y[k] = f32(sum_f x_f W[k][f] - b[k]), b[k] = sum_f c_f W[k][f] (float64, computed once at creation): inputs
 *   widened exactly, products and sums in float64 on the matrix cores, ONE rounding to f32 at the end. basis is [p][d] row-major
 *   (rows = OpenCV's eigenvectors layout), 1 <= p <= 4096, p may exceed d; center NULL = zeros. The handle keeps the basis on
 *   `device` in the order the kernel's operand reads it.
 *   fir_projection_apply[_dev]: rows[m][d] row-major -> out[m][p] row-major; the _dev form is asynchronous on `stream` (NULL = the
 *   projection's own) and calls on one projection are ordered among themselves whatever their streams.
 *   fir_gallery_create_projected: a new independent handle on the source's device holding the source's n rows mapped to p features,
 *   with the source's labels, metric and row offset, default settings and no origin list; written straight into the new handle's
 *   tiles (the only extra memory is the new handle). It answers every call with the bytes of a handle made by fir_gallery_create
 *   over its own rows. The source may be changed or destroyed afterwards; a shard lent by fir_sharded_shard may be the source.
 *   FIR_ERR_ARG when the projection's d is not the source's or the two are on different devices.
 *   The same row gives the same bits through either path (one kernel, one order of summation: the row-major form re-tiles its
 *   input), so a gallery row projected as a query finds itself at distance 0 in the projected handle.
 *
 * Not offered: sharded handles as a whole (scatter matrices and column sums of shards add; the caller adds them), fir_cls handles,
 * device-resident masks, any normalisation after the projection. */
int fir_gallery_feature_stats(fir_gallery* g, const uint64_t* mask, int64_t* count, double* min, double* max, double* avg, double* std);
int fir_gallery_scatter(fir_gallery* g, const uint64_t* mask, const double* center /* [d] or NULL */, double* scatter /* [d][d] */,
                        double* mean_out /* [d], may be NULL */, int64_t* count);
typedef struct fir_projection fir_projection;
int fir_projection_create(const double* basis /* [p][d] */, int32_t p, int32_t d, const double* center /* [d] or NULL */, int32_t device,
                          fir_projection** out);
int fir_projection_destroy(fir_projection* pr);
int fir_projection_info(const fir_projection* pr, int32_t* p, int32_t* d, int32_t* device);
int fir_projection_apply(fir_projection* pr, const float* rows /* [m][d] */, int64_t m, float* out /* [m][p] */);
int fir_projection_apply_dev(fir_projection* pr, const float* d_rows, int64_t m, float* d_out, void* stream);
int fir_gallery_create_projected(fir_gallery* src, fir_projection* pr, fir_gallery** out);

/* ---- all distances of a feature sub-range ---------------------------------------------------
 * out[qb][n] <- distance(query, row j) over [start_pos,end_pos): the per-row loops of
 * ConventionalTWDClassifier / ProposedTWDClassifier (ImageTesting.cpp:117,174,243). */
int fir_range_distances(fir_gallery* g, const float* queries, int32_t qb, int32_t start_pos, int32_t end_pos,
                        float* out);
int fir_range_distances_dev(fir_gallery* g, const float* d_queries, int32_t qb, int32_t start_pos, int32_t end_pos,
                            float* d_out, void* stream);

/* ---- three-way-decision classifiers -----------------------------------------------------------
 * ConventionalTWDClassifier::recognize, ImageTesting.cpp:108-186. type 0 = Posteriors
 * (exp(-100 d) per class, best / sum of the 5 largest class posteriors > threshold, :118-122,141-149),
 * 1 = DistDiff (:157-159), 2 = DistRatio (:160-162). First stage over features
 * [0, reduced_features_count); unreliable queries get the second stage over [.., 256) (:165-180).
 * The gallery needs class labels and d >= 256. class_out[qb] <- class id or -1,
 * unreliable_out[qb] (may be NULL) <- 1 when the second stage ran (num_of_unreliable, :167). */
int fir_twd_conventional(fir_gallery* g, const float* queries, int32_t qb, int32_t num_classes, int32_t type,
                         double threshold, int32_t reduced_features_count, int32_t* class_out, int32_t* unreliable_out);
/* ProposedTWDClassifier::recognize, ImageTesting.cpp:207-288 (CHECK_ALL_INSTANCES build):
 * chunks of reduced_features_count features up to 256, running per-row sums, rows further than
 * best * (1 / threshold) dropped, stop when one class is left. chunks_out (may be NULL) <- chunks used. */
int fir_twd_proposed(fir_gallery* g, const float* queries, int32_t qb, int32_t reduced_features_count, double threshold,
                     int32_t* class_out, int32_t* unreliable_out, int32_t* chunks_out);
/* Which form answered the most recent fir_twd_* call on this handle. Small calls are answered by ONE launch
 * (k_twd_conv_fused / k_twd_prop_fused), the others -- and a one-launch call whose workgroups did not meet in
 * time -- by the launch-per-stage / launch-per-chunk kernels; the verdicts are the same either way, so only this
 * record tells a test or a benchmark which kernels it ran. Every fir_twd_* call that passes its argument checks
 * overwrites the record; the counts add up over the internal batches of that one call (8 queries per one-launch
 * batch). Reading it copies a few words kept in the handle on the host: it does not touch the device, launches
 * and synchronises nothing. FIR_ERR_ARG for a NULL argument or a struct_bytes outside [8, sizeof]. */
typedef struct fir_twd_dispatch_info {
    int32_t struct_bytes;          /* in: sizeof(fir_twd_dispatch_info) */
    int32_t classifier;            /* 0 = fir_twd_conventional, 1 = fir_twd_proposed; -1 = no TWD call on this handle yet */
    int32_t planned_fused;         /* 1 = the call's plan chose the one-launch form (shape, FIR_TWD_FUSED and the occupancy query allowed it) */
    int32_t tiles_per_wave;        /* of that plan: 64-row tiles each wave owns (the kernel's T: 1, 2, 4, 8 or 16); 0 when not fused */
    int32_t workgroups_per_query;  /* grid.x of a one-launch kernel (its workgroups meet each other); 0 when not fused */
    int32_t queries_per_launch;    /* grid.y of a full one-launch batch: min(qb, 8); 0 when not fused */
    int32_t fused_launches;        /* one-launch kernels the call queued (its internal batches) */
    int32_t fused_gave_up;         /* of them: launches whose workgroups did not meet in time (re-answered by the staged form) */
    int32_t staged_batches;        /* internal batches the launch-per-stage / launch-per-chunk form answered */
    int32_t reserved;
    char kernel[160];              /* the one-launch kernel as instantiated, e.g. "fir::k_twd_conv_fused<0, 4>"
                                    * (<metric: 0 L2, 1 chi-square; tiles per wave>); "" when not fused */
} fir_twd_dispatch_info;
int fir_twd_last_dispatch(fir_gallery* g, fir_twd_dispatch_info* out);
/* Batches through the matrix cores. A fir_twd_conventional call with type 0 on an L2 gallery, reduced_features_count a multiple of
 * 16 in [64, 256) and every label of the gallery in [0, num_classes) takes another form when fir_search_top_classes would send a batch
 * of qb queries over [0, reduced_features_count) through the matrix cores (see there and fir_gallery_set_large_batch_mfma: the
 * caller's threshold at any gallery size, never with threshold 0 or FIR_SHADOW_NONE; by default from 128 queries over 65536 rows on:
 * 1.6 - 24 x the launch-per-stage form's speed at 230 400 and 1M rows x 256, 7 680 classes, 128 .. 32 768 queries per call,
 * profiles/twd_conventional_batch.txt; smaller galleries were not measured). Same class_out and unreliable_out for every query:
 *   first stage   the 5 nearest distinct classes over [0, reduced_features_count) (fir_gemm_search_top_classes_keys_dev: the exact
 *                 scan's keys) give the nearest row and the 5 largest class posteriors; max_probab is formed from them in the
 *                 arithmetic of :130,141-148. A query whose max_probab lies within 2^-40 (relative) of the threshold, or is a NaN,
 *                 is answered by the launch-per-stage form instead;
 *   second stage  the 8 nearest rows over [0, 256) of the unreliable queries (fir_gemm_search_topk_keys_dev) are re-evaluated in the
 *                 arithmetic of :173-174, first minimum by (value, row); the answer stands when the 8th row's distance, lowered by
 *                 2^-14 (relative), is still above the winner's value -- no row outside the 8 can then win or tie. A query without
 *                 that certificate (duplicated rows, fewer than 8 rows) is answered by the launch-per-stage form.
 * The call costs the fp16 copies of the two feature prefixes (0.5 x their bytes each; with d == 256 the second is the whole-row
 * state) and synchronises the handle's stream a few times per 32768 queries. fir_twd_last_dispatch then reports classifier 0,
 * planned_fused 0, fused_launches 0, kernel "" and staged_batches = the batches of queries handed to the launch-per-stage form.
 * Types 1 and 2 keep the forms above: their secondBestDist depends on the scan order (:123-126).
 *
 * What the most recent fir_twd_conventional call on this handle did with the matrix cores (host memory, no device access):
 * out[0] queries the matrix-core form took (0: the call was not routed), out[1] of them reliable after stage 1,
 * out[2] unreliable ones answered by the matrix-core second stage, out[3] queries inside the threshold band,
 * out[4] second-stage queries not certified, out[5] stage-1 queries the class call's own exact scan answered.
 * out[3] and out[4] are the queries that went to the launch-per-stage form. FIR_ERR_ARG for a NULL argument. */
int fir_twd_last_mfma(fir_gallery* g, int64_t out[6]);

/* ---- double-precision classifiers (qt_cpp/classification.cpp) ---------------------------------
 * The training set of KNNClassifier / PNNClassifier (classification.cpp:116-226): train_rows[nt][d]
 * float64 in the reference's scan order -- class 0's training rows, then class 1's, ...
 * (classification.cpp:121-122,195-198), train_class[nt] non-decreasing in [0, num_classes),
 * avg[d] = avgValues (classification.cpp:984; Classifier::normalize subtracts it, :103-105).
 * Rows are copied. */
typedef struct fir_cls fir_cls;
int fir_cls_create(const double* train_rows, int64_t nt, int32_t d, const int32_t* train_class, int32_t num_classes,
                   const double* avg, int32_t device, fir_cls** out);
/* Same, train_rows already in `device`'s memory (row-major float64); train_class and avg are host arrays. */
int fir_cls_create_dev(const double* d_train_rows, int64_t nt, int32_t d, const int32_t* train_class, int32_t num_classes,
                       const double* avg, int32_t device, fir_cls** out);
int fir_cls_destroy(fir_cls* c);
/* HIP event pairs around the launches of the float64 distance scan (on the handle's stream); fir_cls_profile_read waits for
 * them and returns their durations (ms) since the previous read, the algorithmic bytes of the last one (training rows once per
 * tile of eight queries + the query tiles + the sums written) and the kernel's name. */
int fir_cls_profile_enable(fir_cls* c, int32_t on);
int fir_cls_profile_read(fir_cls* c, float* ms, int32_t cap, int32_t* count, double* bytes_per_launch, char* kernel, int32_t kernel_cap);
/* PNNwithClusteringClassifier::predict (classification.cpp:389-428) runs the PNN over the medoid rows
 * only but still divides by the FULL training size: set it here (0 = the number of rows held). */
int fir_cls_set_total_training_size(fir_cls* c, int64_t total);
/* PNNwithClusteringClassifier::train, classification.cpp:320-388: k-medoids inside every class of the handle, on the device.
 * Classes: class i holds the rows [class_off[i], class_off[i+1]) of train_rows (the handle's own classes; a class may be
 *   empty). A class with n <= num_clusters rows keeps every row in order (:381-385): medoid_count = n, steps_run = 0.
 * Distance table of a class: T[t][t1] = S / d, S = what fir_cls_distance_sums returns for query = training row t and row t1
 *   (((g - avg) - (q - avg))^2 summed in feature order, un-fused), the division the IEEE double division. With avg all zeros
 *   these are the reference's bits (:337-343, :358-364). T is symmetric bit for bit: the difference only changes sign.
 * One step. Assign: every t goes to the first cluster c (ascending) whose medoid is alive and whose T[medoid_c][t] is the
 *   strict minimum starting from DBL_MAX; when no cluster qualifies (NaN) t belongs to none. Update: the new medoid of a
 *   cluster is its first member t (ascending) whose sum over the members t1 of T[t][t1] -- a plain double sum in ascending t1
 *   -- is the strict minimum starting from DBL_MAX. A cluster with no such member is dead (-1) and stays dead (the reference
 *   indexes [-1] there; it is skipped).
 * Start: medoid c = member c. steps = 0 means the reference's 100 steps, otherwise steps is the upper bound. A step that
 *   leaves the medoid vector unchanged ends the iteration: every later step would repeat it, so the result is that of all
 *   `steps` steps. steps_run[i] (may be NULL) <- the steps computed, the one that confirmed the fixed point included.
 * medoid_rows[i * num_clusters + j] <- position in train_rows of the j-th live medoid of class i, in cluster order; unused
 *   slots hold -1. medoid_count[i] <- how many.
 * scratch_bytes bounds the bytes of distance tables (n^2 * 8 per clustered class) held at once: classes are processed in
 *   groups of consecutive classes whose tables fit. 0 = automatic: half of the device memory free at the time of the call.
 *   Only what the largest group needs is allocated (plus that group's rows in scan order and nt doubles); the handle keeps it.
 * FIR_ERR_ARG: NULL c / medoid_rows / medoid_count, num_clusters outside [1, 256], steps < 0, scratch_bytes < 0, a class of
 *   more than 32768 rows that needs clustering. FIR_ERR_NOMEM: one class's table exceeds the bound, or an allocation failed.
 *   Arguments are checked before anything is allocated or launched. The call synchronises the handle's stream before it
 *   returns and leaves every other call on the handle unaffected. One class runs on one compute unit. */
int fir_cls_kmedoids(fir_cls* c, int32_t num_clusters, int32_t steps, int64_t scratch_bytes, int32_t* medoid_rows /* [num_classes * num_clusters] */,
                     int32_t* medoid_count /* [num_classes] */, int32_t* steps_run /* [num_classes], may be NULL */);
/* sums[qb][nt] <- sum_f ((g_f - avg_f) - (q_f - avg_f))^2 per training row, accumulated in feature
 * order in double (classification.cpp:123-141 before the division, :199-211). */
int fir_cls_distance_sums(fir_cls* c, const double* queries, int32_t qb, double* sums);
/* PNNClassifier::predict_bf, classification.cpp:188-226. var <= 0 selects the reference's value
 * (2e-5, divided by 10 when d > 2000, :190-193). scores[qb][num_classes] (may be NULL) <-
 * sum_t exp(-dist / (2 d var)) / nt per class; best_class[qb] <- first maximum.
 * Batches the caller routes with fir_cls_set_pnn_mfma (never by default) take the float64 matrix cores: the distance table is computed as
 *   |q-avg|^2 + |g-avg|^2 - 2 (q-avg).(g-avg), the dot products by v_mfma_f64_16x16x4_f64, and exp, class sums and arg-max run on it as
 * before (no atomics: the same bits from run to run). Contract of a routed call:
 *   Scores. Every class score lies within a relative E(q) + 2^-40 of the scan's,
 *     E(q) = 2 * 2^-53 * (d + 2) * (|q-avg|^2 + max_t |g_t-avg|^2) / (2 d var)
 *   (first order, |dS| <= 2u(d+2)(|q|^2+|g|^2) for the three-term form in any summation order, divided by the PNN denominator; 2^-40
 *   covers the device exp and the summation order of the class sums).
 *   E(q) is a first-order bound of the form against exact arithmetic; the scan's own sum carries rounding of the same kind (about
 *   (d+2) u S), so the worst case against the scan's score approaches 2 E(q) -- which the class rule below allows for -- while the
 *   differences measured are a thousandth of E(q).
 *   Classes. best_class is the scan's class for every query: a query whose two largest scores s1 >= s2 do not satisfy
 *   s2 (1 + B) < s1 (1 - B), B = 2 (E(q) + 2^-40), or with a NaN score, or with all scores 0 (underflow), is answered by the scan form,
 *   class and scores, written into its slots; fir_cls_pnn_stats counts such queries.
 *   Costs. One double per training row (|g-avg|^2, made on first use, freed by fir_cls_set_pnn_mfma(c, 0) and by destroy) and the centred
 *   queries in the order the instruction's A operand reads them (the tiled training rows are its B operand as they are).
 *   Shapes. 32 queries share one read of the rows while their operands fit the 160 KiB of LDS (d <= 640), 16 up to d <= 1280; a longer
 *   row is answered by the scan and not counted as routed -- never an error. A one-query call with scores == NULL is never routed.
 *   With fir_cls_profile_enable on, the launches of the kernel are bracketed like the scan's and fir_cls_last_dispatch reports its name
 *   (it contains k_cls_pnn_mfma), its bytes and flops_per_launch = 2 * rows * d * queries.
 *   fir_cls_profile_read then holds three times per internal batch, in this order: that kernel, the class sums (k_cls_pnn), the band test.
 *   The scan of the queries sent back is not bracketed: three times per batch whatever the band decides.
 * The row-sharded PNN (fir_cls_create_sharded), fir_cls_pnn_predict_seq and fir_cls_distance_sums keep the scan whatever is set. */
int fir_cls_pnn_predict(fir_cls* c, const double* queries, int32_t qb, double var, double* scores, int32_t* best_class);
/* min_queries > 0: PNN batches of at least that many queries take the f64 matrix cores; 0: never (frees what the form keeps);
 * < 0: the automatic choice -- in this version: never (profiles/pnn_matrix_cores.txt holds the measurements a later default would
 * rest on). A fresh handle is at 0. */
int fir_cls_set_pnn_mfma(fir_cls* c, int32_t min_queries);
/* queries that took the matrix-core form so far, and how many of them the exact scan answered after all */
int fir_cls_pnn_stats(fir_cls* c, int64_t* matrix_core_queries, int64_t* exact_scan_queries_of_them);
/* PNNClassifier::predict_sequentional, classification.cpp:228-295: 32-feature chunks, running per-row
 * sums, class outputs with 2*var*max_fi, classes below max/1e9 dropped, stop when one class is left.
 * chunks_out[qb] (may be NULL) <- chunks used. */
int fir_cls_pnn_predict_seq(fir_cls* c, const double* queries, int32_t qb, double var, int32_t* best_class, int32_t* chunks_out);
/* KNNClassifier::predict, classification.cpp:116-170: rows sorted by mean distance vote for their
 * class until one class has k votes. 1 <= k <= 8. best_class[qb].
 * Batches of >= 128 queries against a training set that streams from HBM (> 256 MiB of rows) go through the matrix cores: an fp16
 * copy of the centred rows nominates the nearest rows (one for k = 1, eight for k > 1), the reference's float64 arithmetic re-ranks
 * them and a rounding-error certificate proves that no other row can be among them; the vote is taken over those rows. A query that
 * is not certified, whose eight rows do not settle the vote, or with equal distances among them goes through the exact scan of every
 * row as before: the classes are the exact scan's either way. Costs the fp16 copy (nt * d * 2 bytes), made on first use. */
int fir_cls_knn_predict(fir_cls* c, const double* queries, int32_t qb, int32_t k, int32_t* best_class);
/* min_queries > 0: kNN batches of at least that many queries take the matrix cores whatever the training set's size; 0: never (frees
 * the fp16 copy); < 0: back to the automatic choice above. */
int fir_cls_set_knn_mfma(fir_cls* c, int32_t min_queries);
/* queries that took the matrix-core path so far, and how many of them the exact scan answered after all */
int fir_cls_knn_stats(fir_cls* c, int64_t* matrix_core_queries, int64_t* exact_scan_queries_of_them);
/* the dominant kernel of the most recent PROFILED launch (fir_cls_profile_enable): name, algorithmic bytes (scans), dot-product flops
 * (matrix-core passes: 2 * rows * d * queries of the launch) */
int fir_cls_last_dispatch(fir_cls* c, char* kernel, int32_t kernel_cap, double* bytes_per_launch, double* flops_per_launch);
/* The part of that vote a row shard can do alone: nearest[qb][num_classes][k] <- the k smallest mean distances of every
 * class among the rows held, ascending, DBL_MAX where the class has fewer. The class that first collects k votes in the
 * globally sorted order is the one whose k-th nearest member is nearest, so ranks exchange these lists, keep the k
 * smallest per class and take the first minimum of the k-th values (sharding.py: merge_knn_class_nearest). */
int fir_cls_knn_class_nearest(fir_cls* c, const double* queries, int32_t qb, int32_t k, double* nearest);

/* ---- FPNNClassifier: orthogonal-series (trigonometric) PNN, classification.cpp:618-791 ----------
 * train() (:661-696): train_rows[nt][d] float64, class-major like fir_cls_create (train_class non-decreasing), avg[d] /
 * sd[d] = avgValues / stdValues of split_train_test (:969-989), scale = features_scale. J = max(3, ceil(cbrt(nt /
 * num_classes))) harmonics; the model has d * num_classes * (2J+1) doubles. */
typedef struct fir_fpnn fir_fpnn;
int fir_fpnn_train(const double* train_rows, int64_t nt, int32_t d, const int32_t* train_class, int32_t num_classes,
                   const double* avg, const double* sd, double scale, int32_t device, fir_fpnn** out);
int fir_fpnn_destroy(fir_fpnn* h);
int fir_fpnn_info(const fir_fpnn* h, int32_t* J, int32_t* d, int32_t* num_classes);
/* a_out[(f * num_classes + c) * (2J+1) + k]: the reference's `a` (:676-690). */
int fir_fpnn_get_model(fir_fpnn* h, double* a_out);
/* predict_bf (:698-735): best_class[qb]; outputs[qb][num_classes] (may be NULL) = the float log-scores. */
int fir_fpnn_predict(fir_fpnn* h, const double* queries, int32_t qb, int32_t* best_class, float* outputs);
/* predict_sequentional (:736-791): 32-feature chunks, classes below max + fastlog(output_ratio) * features_seen are
 * dropped, stop when one is left. chunks_out[qb] (may be NULL) = chunks evaluated. */
int fir_fpnn_predict_seq(fir_fpnn* h, const double* queries, int32_t qb, float output_ratio, int32_t* best_class,
                         int32_t* chunks_out);

/* ---- DirectedEnumeration (maximum-likelihood directed enumeration, ann.h:64-100) -------------------
 * The PIVOT build of the constructor, ann.cpp:302-331: for ii = 0..n_pivots-1, table row ii = distance(gallery row j,
 * pivot ii) over all d features (ann.h:33-38), min_other[ii] = smallest distance from pivot ii to a row of another class
 * (:309-311,325 -> otherClassesDists, the input of getThreshold :341-343), and pivot ii+1 = the first row whose summed
 * distance to the pivots so far (-1000000 restart at a pivot, :313-318) is largest and > 0 (:319-322).
 * pivots[0] = first_pivot (the reference draws it with random_shuffle, :366-376). The gallery needs class labels.
 * pivots_out[n_pivots], table_out[n_pivots][n] (may be NULL), min_other_out[n_pivots] (may be NULL).
 * *n_built_out (may be NULL) < n_pivots when no row had a positive sum (identical rows): the reference would index
 * dbImages[-1] there; the remaining pivots are -1 and their table rows unspecified. */
int fir_dem_pivot_table(fir_gallery* g, int32_t first_pivot, int32_t n_pivots, int32_t* pivots_out, float* table_out,
                        float* min_other_out, int32_t* n_built_out);

/* The same build kept on the device for query time: the table rows of the first min(n_built, 32) pivots
 * (ann.cpp:333-334 keeps 32) and those pivots as a small gallery of their own. The gallery handle must outlive it, and stay
 * as it is: after fir_gallery_append / _set_rows / _remove_rows / a growth, fir_dem_likelihoods and fir_dem_recognize(_dev) return
 * FIR_ERR_STATE (destroy, info and get keep working). */
typedef struct fir_dem fir_dem;
int fir_dem_create(fir_gallery* g, int32_t first_pivot, int32_t n_pivots, fir_dem** out);
int fir_dem_destroy(fir_dem* h);
int fir_dem_info(const fir_dem* h, int32_t* n_pivots, int32_t* n_built, int32_t* n_used, int64_t* n);
/* pivots_out[n_pivots], min_other_out[n_pivots], table_out[n_used][n], order_out[n] = the state of
 * `likelihood_indices` after the pivot loop of recognize (ann.cpp:427-432; identity except near the front). Any may be NULL. */
int fir_dem_get(fir_dem* h, int32_t* pivots_out, float* min_other_out, float* table_out, int32_t* order_out);
/* The data-parallel part of DirectedEnumeration::recognize (ann.cpp:427-447) for qb queries:
 * pivot_dist_out[qb][n_used] = distance(query, pivot i) (CHECK_FOR_BEST_DIST's tmpDist), and
 * lik_out[qb][n] = `likelihoods` after all n_used pivots: sum over i, in order, of (tmpDist_i - table[i][nu])^2 in
 * float, each row visited as often as the reference's index bookkeeping visits it. Either may be NULL. */
int fir_dem_likelihoods(fir_dem* h, const float* queries, int32_t qb, float* pivot_dist_out, float* lik_out);

/* DirectedEnumeration::recognize, ann.cpp:416-507 (PIVOT build), for qb queries in one call. threshold = the
 * object's `threshold`; image_count_to_check as setImageCountToCheck takes it (<= 0 or >= n: n).
 * row[qb] (bestIndex or -1), dist[qb] (bestDistance; FLT_MAX when no row was ever best), found[qb]
 * (isFoundLessThreshold), calc[qb] (distanceCalcCount), tie[qb]; any may be NULL.
 * Per query, with `used` kept pivots, M the count to check, order[] and the likelihoods as fir_dem_get /
 * fir_dem_likelihoods report them:
 *  1. the pivots in order, bestDistance from FLT_MAX with a strict <; a pivot that becomes the best below the
 *     threshold is the answer (found = 1, calc = its number + 1, tie = 0);
 *  2. Mc = M - used; Mc <= 0: the pivots' best, found = 0, calc = used, tie = 0;
 *  3. the candidates are the POSITIONS p in [used, n) of order[] (it may hold a row twice), with the key
 *     (orderable bits of likelihood[order[p]], p): equal likelihoods are walked in position order;
 *  4. the Mc smallest keys are selected, and distance(query, order[p]) over all features is taken for them;
 *  5. if a selected candidate is below the threshold, the one with the smallest key is the answer: found = 1,
 *     calc = used + the number of selected keys up to its own;
 *  6. otherwise found = 0, calc = used + Mc, and the selected candidate with the smallest (distance, key) is the
 *     answer if its distance is strictly below the pivots' best, which stands otherwise.
 * The reference's std::partial_sort leaves the order of equal likelihoods open. tie = 1 says that another order
 * could give another answer: an unselected position shares its likelihood with a selected one; in 5, another
 * selected position has the answer's likelihood; in 6, when a candidate wins, another selected position has both
 * its likelihood and its distance; or a pivot distance is NaN. With tie = 0 every such order gives this answer. */
int fir_dem_recognize(fir_dem* h, const float* queries, int32_t qb, float threshold, int32_t image_count_to_check,
                      int32_t* row, float* dist, int32_t* found, int32_t* calc, int32_t* tie);
/* Device pointers, asynchronous on `stream` (NULL: the gallery handle's), never synchronises once its scratch is
 * large enough; ordered with the other calls on the gallery handle like every *_dev call. */
int fir_dem_recognize_dev(fir_dem* h, const float* d_queries, int32_t qb, float threshold, int32_t image_count_to_check,
                          int32_t* d_row, float* d_dist, int32_t* d_found, int32_t* d_calc, int32_t* d_tie, void* stream);

/* out[qb][m] = distance(query q, gallery row rows[q][m]) over [start_pos, end_pos) (end_pos 0 = d): the candidate
 * checks of an enumeration (CHECK_FOR_BEST_DIST, ann.cpp:389-399) as one gather. Rows are LOCAL indices; a row
 * outside the gallery yields 100000. */
int fir_rows_distances(fir_gallery* g, const float* queries, int32_t qb, const int32_t* rows, int32_t m, int32_t start_pos,
                       int32_t end_pos, float* out);

/* ---- large query batches through the matrix cores (L2, whole feature range) ------------------------
 * Same answers as fir_search_top1 -- bit-identical index and distance: an MFMA GEMM only nominates
 * candidate rows, the reference's arithmetic re-ranks them, a rounding-error certificate proves no other
 * row can win, and uncertified queries are re-run through the exact streaming scan (fir_gemm.hip).
 * Costs one extra copy of the gallery in MFMA fragment order. The gallery handle must outlive it. */
typedef struct fir_gemm fir_gemm;
enum {
    FIR_GEMM_F32 = 0,        /* v_mfma_f32_32x32x2_f32: exact products (157 TF peak)                                */
    FIR_GEMM_BF16_SPLIT = 1, /* x = hi + lo in bf16, hi.hi + hi.lo + lo.hi on v_mfma_f32_32x32x16_bf16           */
    FIR_GEMM_F16 = 2         /* (default) one v_mfma_f32_16x16x32_f16 term on power-of-two-scaled fp16 copies: half the gallery
                              * bytes and a third of the MFMAs per 128 queries; the proxy is good to 2^-10 |q||g|, which the
                              * certificate carries: more rows fall inside the rounding window and are re-ranked exactly */
};
/* Limits, every precision: rows of at most 4608 features (the exact fallback scan keeps eight queries in LDS); longer rows
 * return FIR_ERR_ARG. FIR_GEMM_F16 also wants a device whose compute-unit count is a multiple of 8 and at least 8 (its kernels
 * place the readers of one row range on one XCD): anything else returns FIR_ERR_ARG -- no gfx950 partition mode has such a count,
 * and gfx950 is the only device fir_gallery_create accepts. In both cases the search entry points that create this state by
 * themselves keep the exact streaming scan for the gallery (automatic mode; an explicit fir_gallery_set_large_batch_mfma threshold gets the error).
 * A state is built over the gallery's rows as they are: after an in-place update of the gallery (fir_gallery_append ...) every
 * fir_gemm_search_* call on it returns FIR_ERR_STATE before queueing anything; fir_gemm_destroy and fir_gemm_stats* keep working. */
int fir_gemm_create(fir_gallery* g, fir_gemm** out);   /* = fir_gemm_create_ex(g, FIR_GEMM_F16, out) */
int fir_gemm_create_ex(fir_gallery* g, int32_t precision, fir_gemm** out);
/* ... over a feature prefix [0, end_pos) of every row (0 or d: the whole row): end_pos a multiple of 16, FIR_GEMM_F16 only.
 * The reference's "BF, 64" / "BF, 256" classifiers (ImageTesting.cpp:526-529) compare prefixes; the search entry points
 * route such batches here by themselves (start_pos == 0, end_pos % 16 == 0, end_pos >= 64, same thresholds). */
int fir_gemm_create_range(fir_gallery* g, int32_t precision, int32_t end_pos, fir_gemm** out);
int fir_gemm_destroy(fir_gemm* m);
int fir_gemm_search_top1_keys_dev(fir_gemm* m, const float* d_queries, int32_t qb, uint64_t* d_keys, void* stream);
/* 1..8 queries: one pass over the fp16 copy with v_dot2 (no matrix cores), the rows within one rounding window of the smallest proxy of
 * ALL rows re-ranked exactly, same certificate, same keys. Half the bytes of the exact scan's pass: the search entry points route
 * ONE-query L2 calls here when the compared rows are >= 1.5 GB, from the gallery's 17th such call on (332 -> 253 us for one query against 1M x 512; with two queries the
 * forms tie, beyond that the f32 scan is faster). */
int fir_gemm_search_few_keys_dev(fir_gemm* m, const float* d_queries, int32_t qb, uint64_t* d_keys, void* stream);
/* The k nearest rows (2 <= k <= 8; k = 1 is the call above): d_keys[q * k + r], ascending, the keys fir_search_topk_keys_dev
 * gives. The bound of the append pass is an order statistic of a row sample plus one rounding window; the re-rank window hangs
 * on the k-th smallest proxy and the certificate is taken against the k-th exact distance. fir_search_topk[_keys_dev] route
 * whole-range L2 batches here under the same rule as the top-1 calls (fir_gallery_set_large_batch_mfma). */
int fir_gemm_search_topk_keys_dev(fir_gemm* m, const float* d_queries, int32_t qb, int32_t k, uint64_t* d_keys, void* stream);
/* The keys and classes of fir_search_top_classes_keys_dev, bit for bit, for the feature range the state covers (whole rows or
 * its prefix), through the matrix cores: 1 <= k <= 32, 1 <= num_classes <= 16777216 (else FIR_ERR_ARG), one of d_keys / d_classes
 * may be NULL, a gallery without labels gives FIR_ERR_STATE, a state that is not FIR_GEMM_F16 FIR_ERR_ARG. An exact class-minimum
 * scan over a row sample (the leading max(16384, n k / 64) rows) bounds the k-th class distance from above; the fp16 pass appends
 * every row below that bound (plus one rounding window); the re-rank drops duplicate classes, re-computes every row that can still
 * matter in the reference's arithmetic and certifies against the k-th exact class distance. Unlike the calls above this one
 * SYNCHRONISES `stream` once before returning: it has to learn which queries were not certified (list overflow, window reaching
 * the bound, NaN) and runs the exact scan form for them, straight into their slots (fir_gemm_stats_ex counts them in out[1] and
 * out[2]). fir_search_top_classes routes batches here under fir_gallery_set_large_batch_mfma's rule (see there). */
int fir_gemm_search_top_classes_keys_dev(fir_gemm* m, const float* d_queries, int32_t qb, int32_t num_classes, int32_t k,
                                         uint64_t* d_keys, int32_t* d_classes, void* stream);
/* The keys of fir_search_knn_keys_dev, bit for bit, for the feature range the state covers (whole rows or its prefix), through the
 * matrix cores: 1 <= k <= FIR_GEMM_KNN_MAX (else FIR_ERR_ARG, "k=%d outside [1,256]"); d_keys[q * k + r] ascending, FIR_KEY_NONE for
 * unused slots (an empty gallery: every slot). k <= 8 is the top-1 / top-K call above as it is: it does not synchronise. k > 8 needs
 * a FIR_GEMM_F16 state (else FIR_ERR_ARG) and SYNCHRONISES `stream` once, like the class call: the exact k-th smallest distance over
 * a row sample -- min(n, max(32768, n k / 1024)) rows in 16 runs spread over the gallery (FIR_GEMM_KNN_SAMPLE_DIV replaces the 1024 for
 * experiments; any sample is sound) -- bounds the k-th distance from above; the fp16 pass appends every row below that bound (plus one
 * rounding window); the re-rank re-computes every entry within a window of the k-th smallest proxy in the reference's arithmetic,
 * returns the k smallest exact keys and certifies against the k-th exact distance. Queries that were not certified (more than 4096
 * rows below the bound, NaN, a tie at the certificate's bound) are answered by the store + select form, straight into their slots
 * (fir_gemm_stats_ex counts them in out[1] and out[2]). Argument checks in the order of the other fir_gemm_search_* calls. */
#define FIR_GEMM_KNN_MAX 256
int fir_gemm_search_knn_keys_dev(fir_gemm* m, const float* d_queries, int32_t qb, int32_t k, uint64_t* d_keys, void* stream);
/* The counts and keys of fir_search_radius_keys_dev, bit for bit, for the feature range the state covers (whole rows or its prefix),
 * through the matrix cores: the rows inside DirectedEnumeration's threshold (ann.cpp:390-400). A FIR_GEMM_F16 state, L2,
 * 0 <= max_results <= FIR_GEMM_KNN_MAX (else FIR_ERR_ARG, "max_results=%d outside [0,256]"); d_keys NULL exactly when max_results = 0.
 * The flow of fir_gemm_search_knn_keys_dev without its row sample -- the query brings its bound: the radius, in proxy units plus one
 * rounding window, is the bound the fp16 append pass lists rows below (every row whose reference distance is <= the radius has a
 * proxy below it, whatever the radius is; a radius >= 100000 lists everything); then one wave per query re-computes EVERY listed
 * row in the reference's arithmetic, keeps those with dist < radius and dist < 100000, counts them and sorts the max_results
 * smallest keys. A query is certified when its list did not overflow (4096 entries) and the bound's distance less the rounding
 * window lies above the radius -- rows never listed are then outside it. What is not certified (an overflowed list: more than
 * 4096 rows near the radius, a radius of +inf over more than 4096 rows; NaN operands) gets keys and count from the store + count
 * + select form after the call's one synchronisation of `stream`; fir_gemm_stats_ex counts those queries. */
int fir_gemm_search_radius_keys_dev(fir_gemm* m, const float* d_queries, int32_t qb, const float* d_radius, int32_t max_results,
                                    int32_t* d_count, uint64_t* d_keys, void* stream);
/* fir_search_top1 and fir_search_top1_keys_dev send L2 whole-range batches through this path BY DEFAULT when the batch
 * has >= 128 queries and the gallery >= 65536 rows (smaller, cache-resident galleries: where a cost model of the two forms gives the
 * matrix cores 15 % or more -- e.g. 128 queries against 40 000 x 512, 1 024 against 8 192 x 512 --, from the gallery's fourth such
 * call on; fewer queries on larger galleries: 32 from 128 MB of compared rows on; from 300 MB on wherever a cost model of the two forms says so -- 3, 5, 6, 7 queries are two or three scan passes -- down to 3 queries) (created on first use; costs the extra fp16 gallery copy, n*d*2
 * bytes; identical keys). min_queries > 0: the caller's threshold instead (any gallery size); 0: never, frees the copy
 * (the exact streaming scan answers everything); < 0: back to the default. */
int fir_gallery_set_large_batch_mfma(fir_gallery* g, int32_t min_queries);
/* The int8 nomination pass of large L2 top-1 batches: the batch's rows and queries minus the gallery's column means, quantised to
 * int8 (one scale for the gallery, one per query), nominated on v_mfma_i32_16x16x64_i8 at half the fp16 pass's instructions and
 * gallery bytes; the certificate carries the MEASURED quantisation residuals, the re-rank is the reference's arithmetic on the
 * f32 rows: identical keys. Eligible: top-1 over the whole row of at most 1024 features, more than 32 queries, a call the matrix
 * cores take anyway; top-K, classes, feature prefixes and longer rows keep the fp16 pass. mode 1: every eligible call; 0: never;
 * -1 (default): the library's rule -- automatic matrix-core dispatch over >= 65536 rows only, never under a caller's
 * fir_gallery_set_large_batch_mfma threshold, and back to fp16 for good on a gallery the window does not suit (more than one
 * query in sixteen of a call needing a second pass; learnt without synchronising). The first int8 call builds the int8 copy
 * (n*d bytes next to the fp16 one, reported with the fragments by fir_gallery_memory_bytes) and synchronises its stream once.
 * If there is no memory for the copy, that call and every later one on the gallery are answered by the fp16 pass instead, in
 * every mode (the same keys, no error; fir_gallery_last_dispatch then reads "... (int8 nomination off for this gallery: no
 * memory)"), and what the attempt allocated is freed. A query whose own scale, or its product with the gallery's, leaves
 * (1e-30, 1e30) is left to the exact device scan like a non-finite one. */
int fir_gallery_set_int8_nomination(fir_gallery* g, int32_t mode);
/* passes = 64-query GEMM passes queued so far, fallback_queries = queries answered by the exact device scan instead (results
 * identical either way). Uncertified queries are dealt with on the device, in stream order (a second matrix-core pass with the
 * tightest bound the first one justifies, then the exact scan): the search calls never synchronise; this call waits for the
 * device and reads the counters. */
int fir_gemm_stats(const fir_gemm* m, int64_t* passes, int64_t* fallback_queries);
/* out[0] = passes, out[1] = queries whose FIRST certificate did not hold (list overflow, window reaching the bound, NaN),
 * out[2] = queries the exact device scan answered (= fallback_queries above). */
int fir_gemm_stats_ex(const fir_gemm* m, int64_t out[3]);
/* Diagnostics: the first (up to 8) queries of this state's life whose first certificate did not hold -- per query four floats:
 * entries its candidate list was asked to take (4096 fit), the bound the pass appended below, the smallest stored proxy (K-th
 * smallest for the K nearest), |q|^2. *count = filled slots. Waits for the device. */
int fir_gemm_uncertified_notes(const fir_gemm* m, float out[32], int32_t* count);
int fir_gallery_mfma_uncertified_notes(fir_gallery* g, float out[32], int32_t* count);   /* ... of the automatic dispatch's whole-row state */
/* The same counters for the matrix-core states a gallery's AUTOMATIC dispatch has built (whole rows and feature prefixes),
 * summed: fallback_queries = queries it could not certify and sent through the exact scan (results identical either way). */
int fir_gallery_mfma_stats(fir_gallery* g, int64_t* passes, int64_t* fallback_queries);
int fir_gallery_mfma_stats_ex(fir_gallery* g, int64_t out[3]);
/* HBM held by a gallery handle, in bytes: the tiled f32 rows (+ labels), the fp16 fragment copies the automatic dispatch has
 * made (0.5 x the rows each; one per feature prefix in use), the row-major f32 shadow copies the exact re-rank gathers from
 * (1 x the rows; made only when four times their size was free), and all other scratch. Any pointer may be NULL. */
int fir_gallery_memory_bytes(fir_gallery* g, int64_t* tiled, int64_t* fp16_fragments, int64_t* rowmajor_shadow, int64_t* scratch);
/* Which copies of the gallery the automatic dispatch may keep next to the tiled rows: FIR_SHADOW_ALL (default), FIR_SHADOW_FP16
 * (fragments only: the re-rank gathers from the tiled rows), FIR_SHADOW_NONE (none: every call takes the exact scan, like
 * fir_gallery_set_large_batch_mfma(g, 0)). Takes effect for states built afterwards; existing ones are dropped. */
enum { FIR_SHADOW_NONE = 0, FIR_SHADOW_FP16 = 1, FIR_SHADOW_ALL = 2 };
int fir_gallery_set_shadow_copies(fir_gallery* g, int32_t mode);

/* ---- one gallery sharded by rows over several GPUs (BASELINE.json configs[3]) -----------------
 * The reference is single threaded and single device; this is how BruteForce::recognize (ann.cpp:113-126) and
 * BruteForceClassifier::recognize (ImageTesting.cpp:58-71) use a whole node. Rows are split into contiguous blocks
 * of whole 64-row tiles, one block (or shards_per_device blocks) per listed device; every shard scans the batch and
 * the ranks exchange
 *   top-1: ncclAllReduce(ncclMin, ncclUint64) over the packed keys -- the low word is the GLOBAL row index, so the
 *          integer minimum is the first-minimum rule of db_features.cpp:329-332 over the whole gallery;
 *   top-K: ncclAllGather of K keys per query per rank + an integer K-way merge;
 *   class: ncclAllReduce(ncclMin, ncclInt32) of classNo-if-I-hold-the-winning-row.
 * RCCL over xGMI; the handle owns the per-device streams and communicators. Results are identical to the
 * one-device calls on the unsplit gallery (index, distance bits, tie-break). */
typedef struct fir_sharded fir_sharded;
#define FIR_COMM_ID_BYTES 128
typedef struct fir_shard_opts {
    int32_t struct_bytes;       /* sizeof(fir_shard_opts) */
    int32_t shards_per_device;  /* logical shards per listed device (0 or 1: one); > 1 exercises the split on few GPUs   */
    int64_t first_global_row;   /* global index of rows[0]: this process's row block in a multi-process gallery          */
    const void* comm_id;        /* NULL: this process holds the whole gallery. Else FIR_COMM_ID_BYTES bytes that process 0
                                 * got from fir_comm_unique_id and handed to every process (any out-of-band channel)     */
    int32_t proc_rank, nprocs;  /* with comm_id: this process among nprocs; each lists the same NUMBER of devices        */
    int32_t rows_on_device;     /* 1: rows / class_no are device pointers on devices[0] (one-entry device list only)     */
    int32_t reserved;
    int64_t total_rows;         /* fir_cls_create_sharded with comm_id: training rows over ALL processes (PNN divisor); 0 = n */
    int32_t timeout_ms;         /* bound of every wait behind a collective (0: 120 000). When it passes, or RCCL reports an
                                 * asynchronous error, the communicator is aborted and the call returns FIR_ERR_COMM          */
    int32_t fail_shard;         /* AUDIT BUILD ONLY (libfir_amd_audit.so, -DFIR_AUDIT; the shipped library returns FIR_ERR_ARG for a
                                 * non-zero value): 1-based index of the local shard whose step fails with FIR_ERR_NOMEM (0: none)   */
    int32_t fail_step;          /* ... 1: its scan, after the buffers were agreed on; 2: the buffer growth of its device; 3: from the
                                 * handle's second exchange on the status element comes back poisoned, as if a PEER's scan had failed */
    int32_t reserved2;
} fir_shard_opts;
/* Failure semantics of every sharded handle (the reference's convention is "-1, never block", ann.cpp:113-126): a call in which
 * ANY rank fails -- an allocation, a scan, an RCCL call, a peer that never shows up within timeout_ms -- returns a negative
 * FIR_ERR_* on EVERY rank and never blocks for longer than the time-out: buffers grow in a step the ranks agree on (one-int
 * ncclAllReduce), a rank whose scans fail still enters the exchange with neutral keys and a poisoned status element, waits are
 * bounded and poll ncclCommGetAsyncError, a broken communicator is aborted. The handle is then closed: further calls return
 * FIR_ERR_STATE at once; fir_sharded_destroy / fir_cls_sharded_destroy free it and a fresh handle works. For the asynchronous
 * device-pointer call the failing rank gets its error from the call itself, the others from fir_sharded_sync. */
int fir_comm_unique_id(void* id_out /* [FIR_COMM_ID_BYTES] */);
/* Single process, all rows, one shard per listed device. devices[ndev]: HIP device indices, no repeats. */
int fir_gallery_create_sharded(const float* rows, int64_t n, int32_t d, const int32_t* class_no, int32_t metric,
                               const int32_t* devices, int32_t ndev, fir_sharded** out);
/* General form. Collective over all processes of the communicator (like every search call below). */
int fir_gallery_create_sharded_ex(const float* rows, int64_t n, int32_t d, const int32_t* class_no, int32_t metric,
                                  const int32_t* devices, int32_t ndev, const fir_shard_opts* opts, fir_sharded** out);
int fir_sharded_destroy(fir_sharded* h);
int fir_sharded_info(const fir_sharded* h, int64_t* n_local, int32_t* d, int32_t* ndev, int32_t* nshards, int32_t* nranks,
                     int32_t* first_rank);
/* Shard i of this process (borrowed: tuning, profiling; NULL when the shard holds no rows), its first global row, its rows. */
int fir_sharded_shard(fir_sharded* h, int32_t i, fir_gallery** g, int64_t* first_global_row, int64_t* rows);
int fir_sharded_set_metric(fir_sharded* h, int32_t metric);
/* fir_search_top1 / fir_search_topk over the whole sharded gallery; indices are global rows. */
int fir_sharded_search_top1(fir_sharded* h, const float* queries, int32_t qb, int32_t start_pos, int32_t end_pos,
                            int32_t* idx, float* dist);
int fir_sharded_search_topk(fir_sharded* h, const float* queries, int32_t qb, int32_t start_pos, int32_t end_pos,
                            int32_t k, int32_t* idx, float* dist);
/* fir_search_knn over the shards, 1 <= k <= FIR_KNN_MAX, idx and dist required: every shard produces its k keys with global rows
 * (fir_search_knn_keys_dev), ncclAllGather, and for k > 8 the k smallest of each query's k x ranks gathered keys are taken by the
 * same radix select the shards ran (the keys are orderable and unique); k <= 8 merges as fir_sharded_search_topk does. The keys
 * are the unsharded handle's. Failure semantics, agreed buffer growth and the status element as for the other searches. */
int fir_sharded_search_knn(fir_sharded* h, const float* queries, int32_t qb, int32_t start_pos, int32_t end_pos, int32_t k,
                           int32_t* idx, float* dist);
/* fir_search_top1_other_class over the shards, idx, dist and exclude_class required: every shard runs
 * fir_search_top1_other_class_keys_dev with global rows (the excluded classes ride behind the queries), and the exchange is top-1's
 * ncclMin over the packed keys. The keys are the unsharded handle's. FIR_ERR_STATE without labels. Failure semantics, agreed buffer
 * growth and the status element as for the other searches. The self-join over the shards is not provided. */
int fir_sharded_search_top1_other_class(fir_sharded* h, const float* queries, int32_t qb, int32_t start_pos, int32_t end_pos,
                                        const int32_t* exclude_class /* [qb] */, int32_t* idx, float* dist);
/* fir_search_radius over the shards (the rows inside DirectedEnumeration's threshold, ann.cpp:390-400, of the whole gallery),
 * 0 <= max_results <= FIR_KNN_MAX, arguments as there: every shard runs fir_search_radius_keys_dev with global rows; its counts
 * travel behind its keys in the same ncclAllGather, in front of the status element, and are summed on the device; the keys merge
 * as fir_sharded_search_knn's do -- the max_results smallest of the union are among every shard's max_results smallest.
 * max_results = 0 exchanges counts only. Counts and keys are the unsharded handle's. Failure semantics, agreed buffer growth and
 * the status element as for the other searches. */
int fir_sharded_search_radius(fir_sharded* h, const float* queries, int32_t qb, int32_t start_pos, int32_t end_pos,
                              const float* radius, int32_t max_results, int32_t* count, int32_t* idx, float* dist);
/* Batched BruteForceClassifier::recognize (ImageTesting.cpp:58-71): class_out[qb] <- classNo of the nearest row or -1;
 * idx / dist may be NULL. Needs class labels. */
int fir_sharded_classify_top1(fir_sharded* h, const float* queries, int32_t qb, int32_t start_pos, int32_t end_pos,
                              int32_t* class_out, int32_t* idx, float* dist);
/* One process per GPU (one-entry device list): device pointers on that GPU, asynchronous on `stream`
 * (NULL = the handle's); d_keys[qb] <- the reduced keys, identical on every rank.
 * A rank whose own scans fail gets its error from the call; its peers learn of it from the status element that travels
 * behind the keys: it lands in a sticky word that (a) the NEXT call on the handle looks at on entry, if the previous call's
 * work is through by then, and (b) fir_sharded_sync waits for -- on the stream the call actually ran on, with the handle's
 * time-out -- and reports. A peer that failed skips every later collective, so a caller that must never outrun a failure
 * calls fir_sharded_sync between asynchronous calls (or at least before it relies on the keys); without it the second of two
 * back-to-back calls can enqueue a collective the failed peer never enters, which then ends at the time-out of the next sync. */
int fir_sharded_search_top1_keys_dev(fir_sharded* h, const float* d_queries, int32_t qb, int32_t start_pos,
                                     int32_t end_pos, uint64_t* d_keys, void* stream);
/* Waits (bounded by timeout_ms) for everything the handle has queued, the asynchronous calls on their callers' streams included,
 * and returns the worst status any of their exchanges came back with (FIR_OK, or the peer's error: the handle is then closed). */
int fir_sharded_sync(fir_sharded* h);

/* PNNClassifier::predict_bf (classification.cpp:188-226) over training rows split across GPUs: every shard sums
 * exp(-dist / (2 d var)) over ITS rows per class with the GLOBAL training-set size as divisor, the partial class scores
 * are added on the device and across ranks with ncclAllReduce(ncclSum, ncclDouble), then the first maximum is the class.
 * Only the order of the additions differs from the one-device call (scores within 1e-12 relative, same arg-max unless
 * two classes tie to that precision). train_rows / train_class as in fir_cls_create (class-major); shards are
 * contiguous row blocks. opts may be NULL (one process, one shard per device). */
typedef struct fir_cls_sharded fir_cls_sharded;
int fir_cls_create_sharded(const double* train_rows, int64_t nt, int32_t d, const int32_t* train_class, int32_t num_classes,
                           const double* avg, const int32_t* devices, int32_t ndev, const fir_shard_opts* opts,
                           fir_cls_sharded** out);
int fir_cls_sharded_destroy(fir_cls_sharded* h);
int fir_cls_sharded_pnn_predict(fir_cls_sharded* h, const double* queries, int32_t qb, double var, double* scores,
                                int32_t* best_class);
/* KNNClassifier::predict (classification.cpp:116-170) over the same shards: every shard's k smallest mean distances per class
 * (fir_cls_knn_class_nearest) are merged on the device and across ranks (ncclAllGather); the class whose k-th nearest member is
 * nearest is the one that first collects k votes in the globally sorted order. Exact: the same class as the one-device call. */
int fir_cls_sharded_knn_predict(fir_cls_sharded* h, const double* queries, int32_t qb, int32_t k, int32_t* best_class);
/* HIP events around the exchange step on this process's first device: durations (ms) since the previous read. */
int fir_sharded_profile_enable(fir_sharded* h, int32_t on);
int fir_sharded_profile_read(fir_sharded* h, float* exchange_ms, int32_t cap, int32_t* count);

/* ---- profiling ------------------------------------------------------------------------------
 * When enabled, every gallery-scan kernel launch is bracketed by HIP events on the stream it
 * is launched on. fir_profile_read waits for them and returns the launch durations (ms) in
 * launch order since the previous read; *bytes_per_launch is the algorithmic byte count of the
 * LAST launch (gallery range + query tile + keys). */
int fir_profile_enable(fir_gallery* g, int32_t on);
int fir_profile_read(fir_gallery* g, float* ms, int32_t cap, int32_t* count, double* bytes_per_launch);
/* What the most recent top-1 search on this handle dispatched: its dominant kernel (the gallery-streaming one) as the
 * library launched it, with the code object's resource numbers -- so that a benchmark reports the kernel that ran,
 * not the one it expects. With profiling on, fir_profile_read's durations are the launches of exactly this kernel. */
typedef struct fir_dispatch_info {
    int32_t struct_bytes;     /* in: sizeof(fir_dispatch_info) */
    int32_t path;             /* 0 = exact streaming scan; 1 = matrix-core nomination + exact re-rank + certificate */
    char kernel[160];         /* e.g. "fir::k_scan_l2_lds<1, 8, 4, false>" */
    int32_t launches;         /* launches of it in that call */
    int32_t grid_x, grid_y, block;
    int32_t lds_bytes;        /* static + dynamic LDS of one workgroup */
    int32_t vgprs;            /* registers per lane (hipFuncGetAttributes) */
    int32_t queries_per_pass; /* queries that share one read of the gallery */
    double bytes_per_launch;  /* algorithmic HBM bytes of one launch */
    double flops_per_launch;  /* matrix-core path: 2 * rows * d * queries of one launch; 0 for the scan */
    int32_t warmup_calls_left; /* automatic dispatch, small-saving cases (cache-resident galleries, one-query calls): the matrix-core
                               * state is built only for a gallery that keeps getting such calls; > 0 = this call was one of the
                               * first few and took the scan, this many more will; 0 = steady state */
    int32_t reserved;
    char knobs[160];          /* the FIR_* environment knobs this PROCESS has honoured so far, space separated ("" = none; a trailing
                               * "..." = more than fit). Experiment switches only: none of them changes an answer in the shipped library
                               * (the audit knobs that can are compiled into libfir_amd_audit.so alone, which also lists them here) */
} fir_dispatch_info;
int fir_gallery_last_dispatch(fir_gallery* g, fir_dispatch_info* out);

/* Chi-square / KL galleries: which division sequence the scans use. The IEEE f32 division the compiler emits carries
 * scaling and fix-up steps for operands near the ends of the exponent range; when every gallery value and every query
 * value of a call is +0 or within [2^-26, 2^16] (any L1- or L2-normalised non-negative feature vector is) those steps
 * are the identity, and the scans run the same arithmetic without them -- the same bits, about half the VALU work for
 * chi-square and a third for KL. The check is made on the device while rows are uploaded and queries transposed; one
 * value outside the range (a negative, a NaN, a denormal) and the whole call takes the full sequence.
 * *gallery_plain: every uploaded value was in range; *last_queries_plain: so was every query value of the most recent
 * search on this handle. Synchronises the handle's stream. */
int fir_gallery_value_range(fir_gallery* g, int32_t* gallery_plain, int32_t* last_queries_plain);

/* Block until all work queued by this handle is done: its most recent call, on whatever stream it was given, and with it every
 * earlier call (see "Streams" above fir_search_top1_keys_dev). */
int fir_gallery_sync(fir_gallery* g);

/* Tunables (for experiments). queries_per_pass: 1, 2, 4, 8 or 16; 0 keeps the current setting, < 0 returns to the
 * automatic choice: at most 8 for galleries streamed from HBM and 16 for galleries that stay resident in the 256 MiB
 * Infinity Cache (8 when a 16-query tile would not fit 64 KiB of LDS, d > 1020), halved per call until
 * tiles x passes gives every SIMD a wave (small galleries, small batches). waves: waves per gallery pass, 0 = automatic. */
int fir_gallery_set_tuning(fir_gallery* g, int32_t queries_per_pass, int32_t waves);
int fir_gallery_get_tuning(const fir_gallery* g, int32_t* queries_per_pass, int32_t* waves, int32_t* max_waves);

#ifdef __cplusplus
}
#endif
#endif /* FIR_AMD_H */
