// fir_internal.h -- what the library's translation units share (not part of the public ABI).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/fir_amd.h"

struct fir_gallery;

// The library's one error path: formats the message straight into the (thread-local) buffer fir_last_error() reads and returns `code`.
extern "C" int fir_fail_(int code, const char* fmt, ...) __attribute__((format(printf, 2, 3)));
#define FIR_HIP(expr)                                                                                                  \
    do {                                                                                                               \
        hipError_t e_ = (expr);                                                                                        \
        if (e_ != hipSuccess) return fir_fail_(e_ == hipErrorOutOfMemory ? FIR_ERR_NOMEM : FIR_ERR_HIP,               \
                                               "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), __FILE__, __LINE__); \
    } while (0)

// Read-only view of a gallery handle for the other translation units (fir_twd.hip).
struct fir_gallery_view {
    int device;
    int cus;
    int64_t n;
    int d;
    int metric;             // FIR_METRIC_*
    int64_t row_offset;
    const int32_t* cls;     // device, may be NULL
    hipStream_t stream;     // the handle's own stream
    uint64_t generation;    // bumped by every successful fir_gallery_append / _set_rows / _remove_rows / growth (fir_gallery_generation_)
};
extern "C" int fir_gallery_view_(fir_gallery* g, fir_gallery_view* out);
// In-place updates (include/fir_amd.h: fir_gallery_append ...). A view, or anything built from one (fir_gemm, fir_dem), is good while its
// generation is the handle's: after a mutation n, the labels and -- after a growth -- the buffers behind cls / fir_gallery_tiled_ are
// other ones. fir_gallery_stale_: FIR_OK, or FIR_ERR_STATE ("the gallery changed after this state was built") for the entry points
// of such states to return before they queue anything. g NULL (a float64 state has no gallery): FIR_OK.
extern "C" uint64_t fir_gallery_generation_(const fir_gallery* g);
extern "C" int fir_gallery_stale_(const fir_gallery* g, uint64_t built_at, const char* what);
// fir_shard.hip marks the shards it owns: every mutation of a marked handle fails with FIR_ERR_STATE (their row ranges are the
// sharded handle's bookkeeping).
extern "C" void fir_gallery_set_borrowed_(fir_gallery* g, int borrowed);
// tests only: the number of non-zero 32-bit words among what the layout invariant says is zero -- the rows at or beyond n of every
// allocated tile and the features beyond d. Waits for the handle's calls; one small kernel on its own stream.
extern "C" int fir_gallery_padding_words_(fir_gallery* g, int64_t* words);
// tests only: the two device sums behind fir_gallery_feature_stats' avg and std -- sum[d] and sum_sq[d] over the rows of the host
// mask (NULL: every row), as the fold kernel left them.
extern "C" int fir_gallery_feature_sums_(fir_gallery* g, const uint64_t* mask, double* sum, double* sum_sq);

// Call order of one gallery handle (include/fir_amd.h: calls on one handle take effect in call order, whatever stream they are
// given). Every entry point that queues work on the handle -- or on a fir_gemm state over it: they share its scratch -- holds a
// FirCallOrder for the call, on the stream the call queues on (host-pointer calls: the handle's own). The outermost one makes that
// stream wait for the end of the handle's previous call when that call ran on another stream, and records the end of this call
// on the way out, error returns included; nested ones (entry points other entry points call) do nothing. g may be NULL (no-op).
// A call that has seen all of its work finish on the device before returning (host-pointer calls) says so with done(): it
// records nothing, and the next call, whatever its stream, has nothing to wait for.
extern "C" int fir_gallery_call_begin_(fir_gallery* g, hipStream_t st);
extern "C" void fir_gallery_call_end_(fir_gallery* g, hipStream_t st, int finished);
// Host side: block until the handle's most recent call (and so every call before it) has finished on the device. Before anything
// that frees what calls may still be using, and before reporting.
extern "C" int fir_gallery_wait_calls_(fir_gallery* g);
struct FirCallOrder {
    fir_gallery* g;
    hipStream_t st;
    int rc;
    bool finished = false;
    FirCallOrder(fir_gallery* g_, hipStream_t st_) : g(g_), st(st_) { rc = fir_gallery_call_begin_(g, st); }
    ~FirCallOrder() { fir_gallery_call_end_(g, st, finished); }
    void done() { finished = true; }
    FirCallOrder(const FirCallOrder&) = delete;
    FirCallOrder& operator=(const FirCallOrder&) = delete;
};
// Runs f when the scope is left, however it is left.
template <typename F>
struct FirOnExit {
    F f;
    ~FirOnExit() { f(); }
};
template <typename F>
FirOnExit<F> fir_on_exit(F f) { return FirOnExit<F>{f}; }
// Device memory owned by a handle or a scope: pointer + capacity, freed on destruction. reserve() is a no-op when the bytes
// fit; otherwise it frees and allocates afresh (nothing is carried over, and nobody may still be using the old block).
struct FirBuf {
    void* p = nullptr;
    size_t cap = 0;
    FirBuf() = default;
    FirBuf(const FirBuf&) = delete;
    FirBuf& operator=(const FirBuf&) = delete;
    ~FirBuf() { release(); }
    void release() { if (p) (void)hipFree(p); p = nullptr; cap = 0; }
    hipError_t reserve(size_t bytes) {
        if (p && bytes <= cap) return hipSuccess;
        release();
        const hipError_t e = hipMalloc(&p, bytes < 16 ? 16 : bytes);
        if (e == hipSuccess) cap = bytes < 16 ? 16 : bytes; else p = nullptr;
        return e;
    }
    template <typename T> T* as() const { return (T*)p; }
};
// The same for pinned host memory (hipHostMalloc with the flags the buffer was made with): the staging areas and status
// blocks of fir_shard.hip.
struct FirPinBuf {
    void* p = nullptr;
    size_t cap = 0;
    unsigned flags = hipHostMallocPortable;
    FirPinBuf() = default;
    explicit FirPinBuf(unsigned flags_) : flags(flags_) {}
    FirPinBuf(const FirPinBuf&) = delete;
    FirPinBuf& operator=(const FirPinBuf&) = delete;
    ~FirPinBuf() { release(); }
    void release() { if (p) (void)hipHostFree(p); p = nullptr; cap = 0; }
    hipError_t reserve(size_t bytes) {
        if (p && bytes <= cap) return hipSuccess;
        release();
        const hipError_t e = hipHostMalloc(&p, bytes, flags);
        if (e == hipSuccess) cap = bytes; else p = nullptr;
        return e;
    }
    template <typename T> T* as() const { return (T*)p; }
};
// FIR_RESERVE(buffer, bytes): buffer.reserve(bytes) as a return code on the library's error path -- FIR_ERR_NOMEM when the device
// has no memory left, FIR_ERR_HIP otherwise --, the message naming the buffer and the place of the call as FIR_HIP's does.
template <typename Buf>
int fir_reserve_(Buf& b, size_t bytes, const char* what, const char* file, int line) {
    const hipError_t e = b.reserve(bytes);
    if (e == hipSuccess) return FIR_OK;
    return fir_fail_(e == hipErrorOutOfMemory ? FIR_ERR_NOMEM : FIR_ERR_HIP, "%s.reserve(%zu) failed: %s (%s:%d)", what, bytes, hipGetErrorString(e), file, line);
}
#define FIR_RESERVE(buf, bytes) fir_reserve_(buf, bytes, #buf, __FILE__, __LINE__)
extern "C" void fir_set_last_error_(const char* msg);    // a message kept aside earlier (fir_shard.hip: another rank's or worker's error)
// Every environment knob the library honours goes through here: getenv(name), and a set one is remembered (once) in the list
// fir_gallery_last_dispatch reports in fir_dispatch_info::knobs -- a stray variable in a production environment is visible.
// The knobs that can change ANSWERS (FIR_GEMM_EREL_SCALE, FIR_GEMM_DBG_SKIP, FIR_GEMM_ADAPT_DBG, fir_shard_opts.fail_*) exist
// only in the audit build (-DFIR_AUDIT, libfir_amd_audit.so: what the tests that need them load); the shipped library ignores them.
extern "C" const char* fir_knob_(const char* name);
extern "C" int fir_gallery_tiled_(fir_gallery* g, const void** gal4, int* dp4);   // the tiled f32 gallery (fir_kernels.h layout)

// Device scratch owned by the gallery handle: `slot` in [0, 25), grown on demand, kept until the gallery is destroyed
// (the per-call hipMalloc / hipFree pairs of the classifier entry points cost more than their kernels on small galleries).
// Slots 0-7 and 16: fir_twd.hip (0 queries, 1 conventional distance tables, 2 k_twd_prop_fused state, 3 verdicts, 4-6 proposed chunk
// distances / sums / alive flags, 7 segment records of either staged form, 16 k_twd_conv_fused state), 8-11: fir_dem.hip, 12-15, 17, 18, 23 and 24: fir_capi.hip (17, 18: top_classes_dev; 23: label range; 24: knn_sample_bound_dev);
// 19-22: fir_twd.hip's matrix-core batch form (fir_twd_batch.h: 19 the chunk's queries, 20 the unreliable queries' vectors, 21 keys and classes, 22 flags and lists).
extern "C" int fir_gallery_scratch_(fir_gallery* g, int slot, size_t bytes, void** out);
// Per-handle call counters of the other translation units (slot 0: fir_twd.hip's fused classifier): returns the value before the increment.
extern "C" uint64_t fir_gallery_next_counter_(fir_gallery* g, int slot);
// The handle's record of its most recent fir_twd_* call (fir_twd_last_dispatch): host memory, written by fir_twd.hip's drivers.
extern "C" fir_twd_dispatch_info* fir_gallery_twd_record_(fir_gallery* g);

// d_out[(ci * qb + q) * n + row] = distance(query q, row) over sub-range ci = [start + ci*step, start + (ci+1)*step), for
// every sub-range of [start, end): ONE gallery pass (k_scan_subranges) when step is a multiple of 32 features, one
// range-distance pass per sub-range otherwise. Device pointers; asynchronous on `stream`.
extern "C" int fir_subrange_distances_dev_(fir_gallery* g, const float* d_queries, int32_t qb, int32_t start, int32_t end, int32_t step,
                                           float* d_out, void* stream);

// d_out[q * n + row] = distance over [0, split), d_out[(qb + q) * n + row] = distance over [split, end): ONE gallery pass when
// both widths are multiples of 32 features (the two stages of the conventional TWD: 64 and 192), two otherwise.
extern "C" int fir_split_distances_dev_(fir_gallery* g, const float* d_queries, int32_t qb, int32_t split, int32_t end, float* d_out, void* stream);

// Tests only: the kScanTable name of the kernel of the most recent one-pass launch of the two entries above on this handle, "" when
// their most recent call went range by range (or none was made). A host-side pointer; reading it does not touch the device.
extern "C" const char* fir_gallery_last_subrange_kernel_(fir_gallery* g);

// First touch of a device by this library. The HIP runtime's start-up draws from libc's rand(); the reference's harnesses
// lean on that stream (std::random_shuffle in getTrainingAndTestImages and DirectedEnumeration::init, srand(13) in
// testRecognitionMethod), so the start-up runs on a private random state and the caller's is handed back untouched.
extern "C" int fir_runtime_init_(int device);

// Small host-pointer calls, without copy engine and without stream synchronisation: the kernels read the queries from pinned,
// device-visible host memory and the call's last kernel writes the results there, then a ticket number the host is waiting for.
// fir_wait_ticket_ is that wait for every translation unit (galleries, fir_cls, fir_dem, fir_fpnn, the TWD drivers): it spins on
// the pinned word for 2 ms at most (the clock is read every 1024 spins), then synchronises `st`, which lets the runtime report a
// failed launch, and looks once more. A gallery handle lends its pinned buffer to the other translation units: queries go in at
// `base`, up to *query_bytes; results come back at *results, 4096 eight-byte words; tickets come from fir_gallery_next_ticket_.
extern "C" int fir_wait_ticket_(hipStream_t st, volatile uint64_t* flag, uint64_t ticket);
extern "C" int fir_gallery_pin_(fir_gallery* g, void** base, size_t* query_bytes, uint64_t** results);
extern "C" uint64_t fir_gallery_next_ticket_(fir_gallery* g);

// The exact streaming scan whatever the batch size (fir_search_top1_keys_dev may route large L2 batches through fir_gemm_*,
// whose uncertified queries must not come back to it).
extern "C" int fir_search_top1_exact_keys_dev_(fir_gallery* g, const float* d_queries, int32_t qb, int32_t start_pos, int32_t end_pos,
                                               uint64_t* d_keys, void* stream);

// ... and the exact K-nearest-rows form over features [0, end_pos), never through fir_gemm_*.
extern "C" int fir_search_topk_exact_keys_dev_(fir_gallery* g, const float* d_queries, int32_t qb, int32_t end_pos, int32_t k, uint64_t* d_keys, void* stream);

// The exact class-minimum scan of fir_search_top_classes_keys_dev over features [0, end_pos), on behalf of
// fir_gemm_search_top_classes_keys_dev: not recorded as the handle's dispatch, not timed. sample_rows == 0: the whole gallery,
// keys and classes as the public call writes them (its uncertified queries). sample_rows > 0: only the leading sample_rows rows
// (whole tiles of 64) are scanned and d_bound[q] = the exact K-th smallest class minimum among them, 100000 when fewer than K
// classes qualify there: a minimum over a subset of the rows, so an upper bound of the gallery's K-th class distance.
extern "C" int fir_class_scan_dev_(fir_gallery* g, const float* d_queries, int32_t qb, int32_t end_pos, int32_t num_classes, int32_t k,
                                   int64_t sample_rows, uint64_t* d_keys, int32_t* d_classes, float* d_bound, void* stream);

// The sample bound of fir_gemm_search_knn_keys_dev (fir_gemm_knn.h) over features [0, end_pos), L2 galleries: d_bound[q] = the exact
// K-th smallest reference distance of query q -- the store pass's arithmetic, the bits fir_range_distances returns -- over the row
// sample of knn_sample_plan(n, k, sample_div) (fir_knn_select.h), 100000 when fewer than K rows qualify there: an order statistic of
// a subset of the rows, so an upper bound of the gallery's K-th distance whatever the sample is. Not recorded as the handle's
// dispatch, not timed; asynchronous on `stream` once scratch slot 24 is large enough.
extern "C" int fir_knn_sample_bound_dev_(fir_gallery* g, const float* d_queries, int32_t qb, int32_t end_pos, int32_t k, int32_t sample_div,
                                         float* d_bound, void* stream);

// The matrix-core steps of fir_twd_conventional's batch form (fir_twd.hip), on a prefix [0, end_pos) of the rows (end_pos == d: the
// whole-row state; the handle's two prefix slots hold the others).
// fir_twd_wants_mfma_: 1 when wants_mfma(g, qb, 0, end_pos, classes) holds -- the caller's fir_gallery_set_large_batch_mfma threshold or the
// automatic rule, the pinned-tuning exclusions, gemm_failed -- and the shadow mode is not FIR_SHADOW_NONE; 0 otherwise. Host only.
extern "C" int fir_twd_wants_mfma_(fir_gallery* g, int32_t qb, int32_t end_pos);
// try_mfma_search (kSearchClasses) / run_mfma (rows) of fir_capi.hip: 0 = the keys (and classes) of fir_search_top_classes_keys_dev / fir_search_topk_keys_dev over
// [0, end_pos) are queued or written, 1 = this call stays with the scan (nothing was queued), < 0 = error. The class form synchronises
// `stream`; *exact_answered <- the queries of this call its own exact class scan answered (fir_gemm_stats_ex out[2], this call's share).
// The row form is asked for a part of a batch (the unreliable queries of qb_call): it takes the matrix cores when the rule holds for
// its own qb queries or, under a caller's threshold, for the qb_call queries of the batch that was admitted.
extern "C" int fir_twd_mfma_classes_(fir_gallery* g, const float* d_queries, int32_t qb, int32_t end_pos, int32_t num_classes, int32_t k,
                                     uint64_t* d_keys, int32_t* d_classes, void* stream, int64_t* exact_answered);
extern "C" int fir_twd_mfma_topk_(fir_gallery* g, const float* d_queries, int32_t qb, int32_t qb_call, int32_t end_pos, int32_t k, uint64_t* d_keys,
                                  void* stream);
// The smallest and the largest label of the gallery: one small reduction kernel on the handle's stream the first time (it
// synchronises that stream), the cached words afterwards. FIR_ERR_STATE without labels; an empty gallery gives lo > hi.
extern "C" int fir_gallery_label_range_(fir_gallery* g, int32_t* lo, int32_t* hi);
// The handle's six counters of its most recent fir_twd_conventional call (fir_twd_last_mfma): host memory, written by fir_twd.hip.
extern "C" int64_t* fir_gallery_twd_mfma_record_(fir_gallery* g);

// fir_profile_enable / fir_profile_read / fir_gallery_last_dispatch for kernels launched by the other translation units:
// an event pair around ONE launch on `st` (no-ops unless profiling is on), and the record of the call's dominant kernel.
extern "C" int fir_gallery_profile_begin_(fir_gallery* g, void* st);
extern "C" int fir_gallery_profile_end_(fir_gallery* g, void* st, double bytes_alg);
extern "C" void fir_gallery_note_dispatch_(fir_gallery* g, const void* fn, const char* name, int first, int gx, int gy, int block, size_t dyn_lds,
                                           int qpp, double bytes, double flops);

// tests only: the candidate-list path of the scan (fir_capi.hip: list_nominate, the steps of topk_lists_dev before the re-rank) for
// qb <= 1024 host queries, whatever the gallery's size -- the metric the append scan ran, counts, widened thresholds, per-query and
// per-row constants, sample keys and lists, copied out; all_rows = 1 (n <= 4096): thresholds at +inf, every row listed. See its definition.
extern "C" int fir_gallery_list_nominations_(fir_gallery* g, const float* queries, int32_t qb, int32_t start_pos, int32_t end_pos, int32_t k, int32_t all_rows,
                                             int32_t* info, int32_t* counts, float* tau, float* sq, float* rowsum, uint64_t* skeys, uint64_t* lists,
                                             int32_t* flag);

struct fir_gemm;
// fir_gemm_search_top1 / _topk_keys_dev for queries still in host memory: uploaded into d_stage one super-batch at a time, each
// upload under the previous super-batch's full passes.
extern "C" int fir_gemm_search_staged_(fir_gemm* m, const float* h_queries, float* d_stage, int32_t qb, int32_t k, uint64_t* d_keys, void* stream);

// fir_gemm_create_range with the re-rank's row-major shadow copy decided by the caller: -1 = when HBM has room for it (or as
// FIR_GEMM_ROWMAJOR says), 0 = never, 1 = whenever it can be allocated.
extern "C" int fir_gemm_create_range_ex_(fir_gallery* g, int32_t precision, int32_t end_pos, int32_t rowmajor_mode, fir_gemm** out);
// device bytes one matrix-core state holds: the fp16 (bf16 / f32) fragment copy, the row-major shadow, everything else (scratch)
// tests only: what the most recent call's last super-batch handed its re-rank (fir_gemm.hip); reads, computes and allocates nothing
extern "C" int fir_gemm_nominations_(fir_gemm* m, int32_t which, int32_t q0, int32_t nq, int32_t max_entries, int32_t* counts, float* tau, float* qnorm,
                                     uint64_t* lists, float* proxies, float* gmax, int32_t* qmap, int32_t* live);
// what the gallery handle allows the state's next top-1 call (fir_gallery_set_int8_nomination): 0 = fp16, 1 = the int8 pass for every
// eligible call, -1 = the automatic rule (fir_gemm.hip: gemm_wants_i8_)
extern "C" void fir_gemm_set_int8_(fir_gemm* m, int32_t mode);
// the int8 pass's 256-query tile (two pairs per workgroup, every gallery fragment against both; 257-512 features, launches of two
// pairs or more): -1 = the rule (fir_gemm.hip: gemm_pass_f16_), 0 = never, 1 = whenever the shape allows
extern "C" void fir_gemm_set_int8_tile_(fir_gemm* m, int32_t mode);
extern "C" void fir_gemm_memory_bytes_(const fir_gemm* m, int64_t* fragments, int64_t* rowmajor, int64_t* scratch);
// the gallery generation the state was built at (the handle's own states are rebuilt when it is no longer the handle's)
extern "C" uint64_t fir_gemm_generation_(const fir_gemm* m);

struct fir_cls;
extern "C" int fir_cls_pnn_scores_dev_(fir_cls* c, const double* queries, int32_t qb, double var, double** d_scores, void** stream, int32_t* max_batch);
extern "C" int fir_cls_knn_nearest_dev_(fir_cls* c, const double* queries, int32_t qb, int32_t k, double** d_lists, void** stream, int32_t* max_batch);

// fir_gemm_f64.h: the matrix-core nomination over a float64 training set (tiled layout of fir_cls.hip), for large kNN batches
extern "C" int fir_gemm_create_f64_(int device, int cus, void* stream, const void* gal2, int64_t nt, int d, int dp2, fir_gemm** out);
extern "C" int fir_gemm_knn_f64_(fir_gemm* m, const double* d_qc, int32_t qb, int32_t kp, int32_t* d_rows, double* d_dist, int32_t* d_ok, void* stream,
                                 const char** kernel_name, double* flops_per_launch, hipEvent_t* ev_pair);
extern "C" int fir_gemm_destroy(fir_gemm* m);
// tests only: the nominate + re-rank step of fir_cls_knn_predict's matrix-core path for qb <= 8192 host queries (one super-batch), kp = 1
// or 8 -- rows[qb][kp] (-1 padded), dist[qb][kp] (+inf padded), ok[qb], host memory; the kNN counters are not touched -- and the
// handle's float64 nomination state (NULL: none yet), which fir_gemm_nominations_ reads with which = 0
extern "C" int fir_cls_knn_rows_(fir_cls* c, const double* queries, int32_t qb, int32_t kp, int32_t* rows, double* dist, int32_t* ok);
extern "C" fir_gemm* fir_cls_knn_state_(fir_cls* c);
