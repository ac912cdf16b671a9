// fir_shard.hip -- one gallery sharded by rows over several GPUs, behind the C ABI.
//
// Every shard is an ordinary fir_gallery on its device with row_offset = the global index of its first row; a query
// batch is scanned by all shards at once and the only exchange is
//   top-1:  ncclAllReduce(ncclMin, ncclUint64) of qb packed keys (the low word is the GLOBAL row index, so the integer
//           minimum is the reference's first-minimum rule over the whole gallery, db_features.cpp:329-332);
//   top-K:  ncclAllGather of every rank's K keys per query + an integer K-way merge;
//   class:  ncclAllReduce(ncclMin, ncclInt32) of "classNo of the winning row if I hold it, else INT32_MAX".
// All payloads are KB-sized: the collectives are latency-bound and run on the stream that produced the keys.
//
// Two ways to span GPUs, freely combined (ranks = processes x devices per process):
//   * one process, a device list: one worker thread per device issues that device's launches and its RCCL call;
//   * one process per GPU (torch.distributed.run style): process 0 makes an id with fir_comm_unique_id, hands it
//     to the others out of band, and every process passes it in fir_shard_opts.
// Several logical shards per device (shards_per_device) exist so that the whole path -- split, per-shard scan,
// on-device minimum, RCCL call -- can be exercised on a one-GPU box.
//
// Failure semantics: the reference's convention is "-1, never block" (ann.cpp:113-126, ImageTesting.cpp:63). A collective
// in which one rank does not take part blocks every other rank for good, so no rank ever leaves a call between two
// collectives of it:
//   * buffers grow in an AGREED step: the rank tries its allocations, then a one-int ncclAllReduce(ncclMin) of the local
//     status (on a word allocated when the communicator was made) tells every rank whether all of them have their
//     buffers; the step runs only in calls that have to grow something, which are the same calls on every rank (the
//     capacities depend on the sequence of batch shapes only);
//   * a rank whose scans fail afterwards still enters the exchange, with neutral keys (FIR_KEY_NONE / +0 sums) and a
//     poisoned status element that travels behind the payload (min / gather / sum like the payload itself): every rank
//     returns the same FIR_ERR_* from that call;
//   * every wait on a stream that carries a collective is bounded (fir_shard_opts.timeout_ms, default 120 s) and polls
//     ncclCommGetAsyncError; an error or the time-out aborts the communicator (ncclCommAbort);
//   * after any such failure the handle is dead: later calls return FIR_ERR_STATE at once on every rank (they have all
//     seen the failure), fir_sharded_destroy still frees it, and a fresh handle works.
// fir_shard_opts.fail_shard / fail_step inject a failure for the tests.
#include <hip/hip_runtime.h>
#include <rccl/rccl.h>
#include <stdint.h>
#include <unistd.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cstdio>
#include <cstring>
#include <functional>
#include <mutex>
#include <new>
#include <string>
#include <thread>
#include <vector>

#include "../../include/fir_amd.h"
#include "fir_common.h"
#include "fir_internal.h"
#include "fir_knn_select.h"
#include "fir_search_request.h"
#include "fir_shard_workers.h"

namespace {

using fir::FirSearch;
using fir::kKeyNone;
using fir::KnnArgs;
using fir::KnnCtl;
using fir::kKnnTile;
constexpr int kMergeListMax = 8;     // k up to which k_shard_merge_topk merges (fir_sharded_search_topk's range); beyond it merge_knn

#define SH_NCCL(expr)                                                                                                  \
    do {                                                                                                               \
        ncclResult_t r_ = (expr);                                                                                      \
        if (r_ != ncclSuccess) return fir_fail_(FIR_ERR_COMM, "%s failed: %s (%s:%d)", #expr, ncclGetErrorString(r_), __FILE__, __LINE__); \
    } while (0)

// keys[q] = min over parts p of parts[p][q]   (the shards of one device, before the RCCL call)
__global__ void __launch_bounds__(256) k_shard_min_keys(const uint64_t* __restrict__ parts, int nparts, int n, uint64_t* __restrict__ keys) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    uint64_t m = kKeyNone;
    for (int p = 0; p < nparts; ++p) {
        const uint64_t v = parts[(size_t)p * n + i];
        m = v < m ? v : m;
    }
    keys[i] = m;
}

// *out = min over parts p of first[p * stride]   (the status elements behind gathered parts)
__global__ void __launch_bounds__(64) k_shard_min_status(const uint64_t* __restrict__ first, int nparts, size_t stride, uint64_t* __restrict__ out) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    uint64_t m = kKeyNone;
    for (int p = 0; p < nparts; ++p) {
        const uint64_t v = first[(size_t)p * stride];
        m = v < m ? v : m;
    }
    *out = m;
}

// out[q][0..k) = the k smallest of parts[p][q][0..k), p < nparts, ascending. Every part is ascending and keys are unique
// (global row index in the low word), FIR_KEY_NONE sorts last: exactly fir_search_topk over the union of the parts.
// stride: elements from one part to the next (qb * k, or qb * k + 1 when a status element rides behind every part: then
// status_out <- the minimum of those elements).
__global__ void __launch_bounds__(64) k_shard_merge_topk(const uint64_t* __restrict__ parts, int nparts, int qb, int k, uint64_t* __restrict__ out,
                                                          size_t stride, uint64_t* __restrict__ status_out) {
    const int q = blockIdx.x * 64 + threadIdx.x;
    if (status_out && q == 0) {
        uint64_t m = kKeyNone;
        for (int p = 0; p < nparts; ++p) {
            const uint64_t v = parts[(size_t)p * stride + (size_t)qb * k];
            m = v < m ? v : m;
        }
        *status_out = m;
    }
    if (q >= qb) return;
    uint64_t prev = 0;
    bool first = true;
    for (int j = 0; j < k; ++j) {           // j-th smallest = the smallest key greater than the previous pick
        uint64_t m = kKeyNone;
        for (int p = 0; p < nparts; ++p) {
            const uint64_t* L = parts + (size_t)p * stride + (size_t)q * k;
            for (int i = 0; i < k; ++i) {
                const uint64_t v = L[i];
                if ((first || v > prev) && v < m) m = v;
            }
        }
        out[(size_t)q * k + j] = m;
        if (m == kKeyNone) { for (int r = j + 1; r < k; ++r) out[(size_t)q * k + r] = kKeyNone; break; }
        prev = m;
        first = false;
    }
}

// cls_out[q] = classNo of the row keys[q] names when rows [lo, hi) are held here (cls = their labels), left alone otherwise
__global__ void __launch_bounds__(256) k_shard_class_owned(const uint64_t* __restrict__ keys, int n, const int32_t* __restrict__ cls, int64_t lo,
                                                            int64_t hi, int32_t* __restrict__ cls_out) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const uint64_t v = keys[i];
    if (v == kKeyNone) return;
    const int64_t row = (int64_t)(uint32_t)(v & 0xFFFFFFFFull);
    if (row >= lo && row < hi) cls_out[i] = cls[row - lo];
}
__global__ void __launch_bounds__(256) k_shard_fill_i32(int32_t* p, int n, int32_t v) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < n) p[i] = v;
}
__global__ void __launch_bounds__(256) k_shard_fill_u64(uint64_t* p, int n, uint64_t v) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < n) p[i] = v;
}

// out[q] = sum over parts p of parts[p * stride + q], q < qb: the rows inside each query's radius (fir_sharded_search_radius), over the
// shards of one device and then over the ranks. The counts ride behind the keys in whole 64-bit words: with an odd qb the last
// half word is kept 0.
__global__ void __launch_bounds__(256) k_shard_sum_counts(const int32_t* __restrict__ parts, int nparts, size_t stride, int qb, int32_t* __restrict__ out) {
    const int q = blockIdx.x * 256 + threadIdx.x;
    if (q >= qb + (qb & 1)) return;
    int32_t sum = 0;
    if (q < qb)
        for (int p = 0; p < nparts; ++p) sum += parts[(size_t)p * stride + q];
    out[q] = sum;
}

using fir::KeptError;

struct Shard {
    int slot = 0;              // index into devs
    fir_gallery* g = nullptr;  // nullptr: no rows (more shards than 64-row tiles)
    int64_t lo = 0, hi = 0;    // global rows
    const int32_t* cls = nullptr;
};

struct DevCtx {
    int device = 0;
    hipStream_t stream = nullptr;
    ncclComm_t comm = nullptr;
    FirBuf dq;                                            // float: the queries of a host-pointer call
    FirBuf parts;                                         // uint64_t [shards here][qb * k]
    FirBuf keys;                                          // uint64_t [qb * k] reduced
    FirBuf gath;                                          // uint64_t [nranks][qb * k]
    FirBuf cls;                                           // int32_t: the winners' classes
    FirBuf sel;                                           // the control block of the K > 8 merge (fir_knn_select.h: KnnCtl)
    std::vector<int> shards;
    std::vector<hipEvent_t> evs;                          // pairs around the RCCL calls (profiling, device slot 0)
    size_t ev_used = 0;
    FirBuf status;                                        // int32_t: [0] the agreed-growth word, [1] sticky status of the asynchronous calls
    FirPinBuf h_status{hipHostMallocPortable | hipHostMallocMapped};   // int32_t: [0] what this rank contributes, [1] what came back, [2] sticky read-back,
                                                          // [3] the sticky status as the device mirrors it (k_shard_note_status), [4..5] a double (fir_cls_sharded)
    int32_t* d_hsticky = nullptr;                         // device address of h_status[3]
    hipEvent_t async_done = nullptr;                      // behind the last asynchronous device-pointer call, on the stream it ran on
    bool async_pending = false;                           // ... whose status nobody has looked at yet
    int32_t* dstat() const { return status.as<int32_t>(); }
    int32_t* hstat() const { return h_status.as<int32_t>(); }
};

// The devices of a handle and, when it lists several, their worker threads. setup_devices makes what is in here and
// teardown_devices is the one place that releases it: stream, communicator, status words, events, buffers, workers.
struct Devices {
    std::vector<DevCtx> ctx;
    fir::Workers workers;
    DevCtx& operator[](int slot) { return ctx[(size_t)slot]; }
    int run_all(const std::function<int(int)>& fn) { return workers.run_all(fn); }
};

// What the ranks of a handle have to agree on to stay out of each other's way (see "Failure semantics" above).
struct Health {
    std::atomic<bool> dead{false};   // a collective failed or a peer reported an error: no further collective is attempted
    std::atomic<int> dead_code{0};
    int timeout_ms = 120000;         // bound of every wait behind a collective
    int fail_shard = 0;              // test hook: 1-based local shard whose step fails, 0 = none
    int fail_step = 0;               // 1 = its scan (after the agreed growth), 2 = its device's buffer growth
    int exchanges_done = 0;          // (audit build's fail_step = 3)
    void apply(const fir_shard_opts& o) {
        if (o.timeout_ms > 0) timeout_ms = o.timeout_ms;
        fail_shard = o.fail_shard;
        fail_step = o.fail_step;
    }
    // The handle is dead from here on. The first code stays: every call starts on a live handle, so a later close() of the same
    // call (another device's, or the caller's after run_all) speaks of the same failure.
    int close(int code) {
        int none = 0;
        dead_code.compare_exchange_strong(none, code);
        dead = true;
        return code;
    }
};

// buffer.reserve with the size rule of its call site: nothing when `bytes` fit (no bytes always fit), else a fresh block of
// max(bytes, floor) -- asked for by what the call needs, never by what a block happens to hold beyond it.
template <typename Buf>
int grow_buf(Buf& b, size_t bytes, size_t floor, const char* what, int line) {
    if (bytes <= b.cap) return FIR_OK;
    return fir_reserve_(b, std::max(bytes, floor), what, __FILE__, line);
}
#define SH_GROW(buf, bytes, floor) grow_buf(buf, bytes, floor, #buf, __LINE__)

int peer_failed(int code) {
    const char* what = code == FIR_ERR_NOMEM ? "allocation failed" : code == FIR_ERR_HIP ? "a HIP call failed" : code == FIR_ERR_COMM ? "an RCCL call failed"
                                                                                                                                    : "its step failed";
    return fir_fail_(code < 0 ? code : FIR_ERR_COMM, "a rank of the sharded handle reported an error (%s): the call fails on every rank and the handle is closed for further calls", what);
}

// Abort this device's communicator (a blocked collective returns) and mark the handle dead.
int comm_dead(DevCtx& dc, Health& hl, int code, const char* why) {
    hl.close(code);
    if (dc.comm) { (void)ncclCommAbort(dc.comm); dc.comm = nullptr; }
    return fir_fail_(code, "sharded handle: %s; the communicator was aborted and the handle is closed for further calls", why);
}

// A synchronisation with a bound: polls `query` (hipSuccess = done) and the communicator's asynchronous error state; an error
// or hl.timeout_ms without completion abort the communicator.
template <typename Query>
int wait_bounded(DevCtx& dc, Health& hl, Query query, const char* timed_out) {
    const auto t0 = std::chrono::steady_clock::now();
    for (int spins = 0;; ++spins) {
        const hipError_t q = query();
        if (q == hipSuccess) return FIR_OK;
        if (q != hipErrorNotReady) { (void)hipGetLastError(); return comm_dead(dc, hl, FIR_ERR_HIP, hipGetErrorString(q)); }
        if (dc.comm && (spins & 63) == 63) {
            ncclResult_t ar = ncclSuccess;
            if (ncclCommGetAsyncError(dc.comm, &ar) == ncclSuccess && ar != ncclSuccess && ar != ncclInProgress)
                return comm_dead(dc, hl, FIR_ERR_COMM, ncclGetErrorString(ar));
        }
        if (spins > 2000) {
            if (std::chrono::duration_cast<std::chrono::milliseconds>(std::chrono::steady_clock::now() - t0).count() > hl.timeout_ms)
                return comm_dead(dc, hl, FIR_ERR_COMM, timed_out);
            std::this_thread::sleep_for(std::chrono::microseconds(20));
        }
    }
}
// hipStreamSynchronize with that bound ...
int wait_stream(DevCtx& dc, hipStream_t st, Health& hl) {
    return wait_bounded(dc, hl, [st] { return hipStreamQuery(st); }, "a collective did not complete within the time-out (a peer is gone or never entered it)");
}
// ... and the same for an event (the asynchronous device-pointer call runs on the CALLER's stream: its completion is an event
// recorded there, not the state of the handle's own stream)
int wait_event(DevCtx& dc, hipEvent_t ev, Health& hl) {
    return wait_bounded(dc, hl, [ev] { return hipEventQuery(ev); },
                        "an asynchronous call's exchange did not complete within the time-out (a peer is gone or never entered it)");
}

// Every rank contributes its local status (FIR_OK or a negative FIR_ERR_*); all of them get the minimum.
int agree(DevCtx& dc, hipStream_t st, Health& hl, int local_rc, int* agreed) {
    if (!dc.comm) return fir_fail_(FIR_ERR_STATE, "sharded handle: no communicator");
    dc.hstat()[0] = local_rc;
    hipError_t e = hipMemcpyAsync(dc.dstat(), dc.hstat(), sizeof(int32_t), hipMemcpyHostToDevice, st);
    ncclResult_t nr = e == hipSuccess ? ncclAllReduce(dc.dstat(), dc.dstat(), 1, ncclInt32, ncclMin, dc.comm, st) : ncclSuccess;
    if (e == hipSuccess && nr == ncclSuccess) e = hipMemcpyAsync(dc.hstat() + 1, dc.dstat(), sizeof(int32_t), hipMemcpyDeviceToHost, st);
    if (e != hipSuccess) return comm_dead(dc, hl, FIR_ERR_HIP, hipGetErrorString(e));
    if (nr != ncclSuccess) return comm_dead(dc, hl, FIR_ERR_COMM, ncclGetErrorString(nr));
    const int rc = wait_stream(dc, st, hl);
    if (rc) return rc;
    *agreed = dc.hstat()[1];
    return FIR_OK;
}

// One call of an entry point on one device, in the steps the entry points share: the agreed growth (grow_agreed), this rank's own
// work with its error kept aside (keep_local) -- the rank enters the exchange whatever happened to it --, and after the wait the
// verdict: my error, a peer's, or fine. The payload between these steps is the entry point's own.
struct Call {
    DevCtx& dc;
    Health& hl;
    hipStream_t st;
    int local = FIR_OK;        // what this rank's own step returned ...
    KeptError mine;            // ... and said
};

// The agreed growth step of a call: `need` says whether this call grows anything on this rank (the same answer on every
// rank), `alloc` tries the allocations. Everyone leaves with the same verdict.
int grow_agreed(Call& c, bool need, bool inject, const std::function<int()>& alloc) {
    if (!need) return FIR_OK;
    const int r = inject ? fir_fail_(FIR_ERR_NOMEM, "injected allocation failure (fir_shard_opts.fail_step = 2)") : alloc();
    if (r) c.mine.capture();
    int all = FIR_OK;
    const int ra = agree(c.dc, c.st, c.hl, r, &all);
    if (ra) return ra;
    if (all == FIR_OK) return FIR_OK;
    c.hl.close(all);
    if (r) { c.mine.restore(); return r; }                // this rank's own error text
    return peer_failed(all);
}
void keep_local(Call& c, int rc) {
    c.local = rc;
    if (rc) { c.mine.capture(); (void)hipGetLastError(); }
}
int peer_verdict(Health& hl, int code) {                  // what came back from the other ranks: a FIR_ERR_* of one of them, or FIR_OK
    if (code == FIR_OK) return FIR_OK;
    hl.close(code);
    return peer_failed(code);
}
int verdict(Call& c, int peers) {
    if (c.local) { c.hl.close(c.local); c.mine.restore(); return c.local; }
    return peer_verdict(c.hl, peers);
}
// ... and of the whole call, after the fan-out over the devices
int call_done(Health& hl, int rc) { return rc ? hl.close(rc) : FIR_OK; }

constexpr uint64_t kStatusOk = kKeyNone;                  // the element behind a key payload: all ones = every rank was fine
__host__ __device__ inline uint64_t status_key(int rc) { return rc == FIR_OK ? kStatusOk : (uint64_t)(uint32_t)(1000 + rc); }   // smaller = worse under ncclMin
inline int status_code(uint64_t v) { return v == kStatusOk ? FIR_OK : (int)(int64_t)v - 1000; }

__global__ void k_shard_set_u64(uint64_t* p, uint64_t v) { *p = v; }
__global__ void k_shard_set_i32(int32_t* p, int32_t v) { *p = v; }
__global__ void k_shard_set_f64(double* p, double v) { *p = v; }
// sticky[0] = min(sticky[0], status of the exchange just finished) -- the asynchronous device-pointer call's record
// ... mirrored into pinned host memory, where the next call (or fir_sharded_sync) reads it without a copy of its own
__global__ void k_shard_note_status(const uint64_t* __restrict__ st, int32_t* __restrict__ sticky, int32_t* __restrict__ host_sticky) {
    const uint64_t v = *st;
    const int32_t c = v == kKeyNone ? 0 : (int32_t)(int64_t)v - 1000;
    if (c < *sticky) { *sticky = c; *host_sticky = c; }
}

}  // namespace

struct fir_sharded {
    int d = 0, metric = 0;
    int64_t n_local = 0, first_row = 0;
    int ndev = 0, spd = 1, nranks = 1, rank0 = 0;
    bool has_labels = false;
    Devices devs;
    std::vector<Shard> shards;
    FirPinBuf pin;                   // pinned host staging: queries in, keys / classes out
    bool profiling = false;
    Health health;
};

namespace {

int check_range(const fir_sharded* h, int32_t& start, int32_t& end) {
    if (end == 0) end = h->d;
    if (start < 0 || end > h->d || start >= end) return fir_fail_(FIR_ERR_ARG, "feature range [%d,%d) not inside [0,%d)", start, end, h->d);
    return FIR_OK;
}

// The buffers of one call on one device, grown in the call's agreed step, in bytes: queries (host-pointer form), the shards'
// partial keys, the reduced keys + status element, the gathered keys of all ranks (top-K), the winners' classes + status
// element and the control block of the K > 8 merge. Every device holds h->spd shards, so the sizes are every device's.
// A radius call (fir_sharded_search_radius, k = max_results, 0 included) carries qb counts as well: the radii behind the queries,
// every shard's counts behind all the shards' keys, and the device's counts in FirSearch::count_words(qb) 64-bit words between its keys
// and the status element (FirSearch::status_index) -- one payload, one ncclAllGather.
struct CallBuffers { size_t dq, parts, keys, gath, cls, sel; };
CallBuffers call_buffers(const fir_sharded* h, int32_t qb, const FirSearch& s, bool host_queries, bool winners_classes) {
    const size_t u64 = sizeof(uint64_t), payload = s.status_index(qb);
    return {host_queries ? (size_t)qb * h->d * sizeof(float) + s.radii_bytes(qb) + s.exclude_bytes(qb) : 0, payload * (size_t)h->spd * u64, (payload + 1) * u64,
            s.k != 1 || s.is_radius() ? (payload + 1) * (size_t)h->nranks * u64 : 0, winners_classes ? ((size_t)qb + 1) * sizeof(int32_t) : 0,
            s.k > kMergeListMax ? (sizeof(KnnCtl) + 7) / 8 * u64 : 0};
}
// Does this call grow anything? Asked ONCE per call, before the fan-out over the devices, of device slot 0's capacities (and
// the staging area's): a one-int collective hangs on the answer, so it has to be the same on every slot and every rank. It is,
// because it depends on the history of call shapes only: every device of every rank holds the same number of shards, every
// growth so far ran in an agreed step that either gave every buffer of every rank its size or closed the handle, and SH_GROW
// sizes a block by what was asked for. It must never become "is MY buffer too small".
bool call_grows(const DevCtx& dc, const CallBuffers& b) {
    return b.dq > dc.dq.cap || b.parts > dc.parts.cap || b.keys > dc.keys.cap || b.gath > dc.gath.cap || b.cls > dc.cls.cap || b.sel > dc.sel.cap;
}
int call_alloc(DevCtx& dc, const CallBuffers& b) {
    constexpr size_t f4 = 1024 * sizeof(float), f8 = 1024 * sizeof(uint64_t);     // no block below 1 024 elements
    int rc;
    if ((rc = SH_GROW(dc.dq, b.dq, f4))) return rc;
    if ((rc = SH_GROW(dc.parts, b.parts, f8))) return rc;
    if ((rc = SH_GROW(dc.keys, b.keys, f8))) return rc;
    if ((rc = SH_GROW(dc.gath, b.gath, f8))) return rc;
    if ((rc = SH_GROW(dc.sel, b.sel, f8))) return rc;
    return SH_GROW(dc.cls, b.cls, f4);
}
bool inject_here(const fir_sharded* h, const DevCtx& dc, int step) {
    if (h->health.fail_step != step || h->health.fail_shard <= 0) return false;
    for (int si : dc.shards)
        if (si == h->health.fail_shard - 1) return true;
    return false;
}

// out[q][0..k) = the k smallest of parts[p][q][0..k), p < nparts, ascending, for k > kMergeListMax (fir_sharded_search_knn): the
// keys are orderable and unique, so the radix select of fir_knn_select.h over each query's nparts * k keys finds exactly them
// -- k_shard_merge_topk reads every list k times with one lane per query, which holds for 8 keys and not for 1024 x ranks.
// kKnnTile queries per select; status_out (may be NULL) <- the minimum of the status elements behind the parts.
int merge_knn(DevCtx& dc, const uint64_t* parts, int nparts, int32_t qb, int32_t k, uint64_t* out, size_t stride, uint64_t* status_out, hipStream_t st) {
    if (status_out) hipLaunchKernelGGL(k_shard_min_status, dim3(1), dim3(64), 0, st, parts + (size_t)qb * k, nparts, stride, status_out);
    for (int q0 = 0; q0 < qb; q0 += kKnnTile) {
        KnnArgs a{};
        a.keys = parts + (size_t)q0 * k;
        a.n = (int64_t)nparts * k;
        a.stride = (int64_t)stride;
        a.k_in = k;
        a.k = k;
        a.ctl = dc.sel.as<KnnCtl>();
        a.out = out + (size_t)q0 * k;
        FIR_HIP(fir::knn_select_launch<false>(a, std::min<int>(kKnnTile, qb - q0), fir::kKnnMaxBlocks, st));
    }
    return FIR_OK;
}

// The merge of nparts lists of k keys per query, `stride` words apart, into out[qb * k]: none for k = 0, the minimum for one key in back-to-back lists, the list merge up to 8, else the select
int merge_keys(DevCtx& dc, const uint64_t* parts, int nparts, int32_t qb, int32_t k, uint64_t* out, size_t stride, uint64_t* status_out, hipStream_t st) {
    if (k > kMergeListMax) return merge_knn(dc, parts, nparts, qb, k, out, stride, status_out, st);
    if (k == 1 && stride == (size_t)qb) hipLaunchKernelGGL(k_shard_min_keys, dim3((unsigned)((qb + 255) / 256)), dim3(256), 0, st, parts, nparts, qb, out);
    else if (k > 0) hipLaunchKernelGGL(k_shard_merge_topk, dim3((qb + 63) / 64), dim3(64), 0, st, parts, nparts, qb, k, out, stride, status_out);
    return FIR_OK;
}

// The keys of one device: every shard it holds scans the batch (s.k keys per query, each kind through its gallery call; K = 1:
// top-1), then the merge over those shards lands in dc.keys[0, qb * k). Buffers exist (call_alloc). s.radius (device memory): the
// radius call -- every shard's fir_search_radius_keys_dev with global rows, the sum of their counts in the words behind the keys.
// s.exclude (device memory): the other-class call -- every shard's fir_search_top1_other_class_keys_dev, one key per query like top-1.
int device_keys(fir_sharded* h, int slot, const float* d_queries, int32_t qb, int32_t start, int32_t end, const FirSearch& s, hipStream_t st) {
    DevCtx& dc = h->devs[slot];
    uint64_t *parts = dc.parts.as<uint64_t>(), *keys = dc.keys.as<uint64_t>();
    const size_t per = s.key_words(qb);
    int32_t* cparts = (int32_t*)(parts + per * (size_t)h->spd);              // [shard here][qb]
    int rc;
    int live = 0;
    for (size_t i = 0; i < dc.shards.size(); ++i) {
        Shard& sh = h->shards[dc.shards[i]];
        if (h->health.fail_step == 1 && h->health.fail_shard - 1 == dc.shards[i])
            return fir_fail_(FIR_ERR_NOMEM, "injected scan failure on shard %d (fir_shard_opts.fail_step = 1)", dc.shards[i]);
        if (!sh.g) continue;
        uint64_t* out = parts + (size_t)live * per;
        rc = s.is_radius() ? fir_search_radius_keys_dev(sh.g, d_queries, qb, start, end, s.radius, s.k, cparts + (size_t)live * qb, s.k ? out : nullptr, st)
             : s.kind == fir::kSearchOtherClass ? fir_search_top1_other_class_keys_dev(sh.g, d_queries, qb, start, end, s.exclude, out, st)
             : s.k == 1 ? fir_search_top1_keys_dev(sh.g, d_queries, qb, start, end, out, st)
             : s.kind == fir::kSearchSelect ? fir_search_knn_keys_dev(sh.g, d_queries, qb, start, end, s.k, out, st)
                                            : fir_search_topk_keys_dev(sh.g, d_queries, qb, start, end, s.k, out, st);
        if (rc) return rc;
        ++live;
    }
    if (s.is_radius()) hipLaunchKernelGGL(k_shard_sum_counts, dim3((qb + 256) / 256), dim3(256), 0, st, cparts, live, (size_t)qb, qb, (int32_t*)(keys + per));
    if (live == 0 && per) hipLaunchKernelGGL(k_shard_fill_u64, dim3((unsigned)((per + 255) / 256)), dim3(256), 0, st, keys, (int)per, kKeyNone);
    else if ((rc = merge_keys(dc, parts, live, qb, s.k, keys, per, nullptr, st))) return rc;
    FIR_HIP(hipGetLastError());
    return FIR_OK;
}

// The exchange step over all ranks, on `st`, result in dc.keys (in place); dc.keys[qb * k] carries local_rc in and the worst
// status of all ranks out. A rank whose scans failed contributes FIR_KEY_NONE keys. Errors here kill the communicator.
// radius: the counts travel between the keys and the status element (which is then dc.keys[FirSearch::status_index(qb)]) in the same
// ncclAllGather -- for every k, 0 and 1 included --, and the ranks' counts are summed in place.
int exchange_keys(fir_sharded* h, int slot, int32_t qb, const FirSearch& s, hipStream_t st, int local_rc) {
    DevCtx& dc = h->devs[slot];
    uint64_t *keys = dc.keys.as<uint64_t>(), *gath = dc.gath.as<uint64_t>();
    const size_t per = s.key_words(qb), payload = s.status_index(qb);
    const bool prof = h->profiling && slot == 0;
    if (local_rc && per) hipLaunchKernelGGL(k_shard_fill_u64, dim3((unsigned)((per + 255) / 256)), dim3(256), 0, st, keys, (int)per, kKeyNone);
    if (local_rc && s.is_radius()) hipLaunchKernelGGL(k_shard_sum_counts, dim3((qb + 256) / 256), dim3(256), 0, st, (const int32_t*)nullptr, 0, (size_t)0, qb, (int32_t*)(keys + per));
    hipLaunchKernelGGL(k_shard_set_u64, dim3(1), dim3(1), 0, st, keys + payload, status_key(local_rc));
    if (prof) {
        if (dc.ev_used + 2 > dc.evs.size())
            for (int i = 0; i < 64; ++i) {
                hipEvent_t e;
                if (hipEventCreate(&e) != hipSuccess) break;
                dc.evs.push_back(e);
            }
        if (dc.ev_used + 2 <= dc.evs.size()) (void)hipEventRecord(dc.evs[dc.ev_used], st);
    }
    ncclResult_t nr;
    if (s.k == 1 && !s.is_radius()) {                   // one key per query and no counts: the minimum is the collective's
        nr = ncclAllReduce(keys, keys, per + 1, ncclUint64, ncclMin, dc.comm, st);
    } else {
        nr = ncclAllGather(keys, gath, payload + 1, ncclUint64, dc.comm, st);
        // (the merges find the status element right behind the keys; behind the counts it is taken by itself)
        uint64_t* status_out = s.is_radius() ? nullptr : keys + per;
        if (nr == ncclSuccess && s.is_radius()) {
            hipLaunchKernelGGL(k_shard_min_status, dim3(1), dim3(64), 0, st, gath + payload, h->nranks, payload + 1, keys + payload);
            hipLaunchKernelGGL(k_shard_sum_counts, dim3((qb + 256) / 256), dim3(256), 0, st, (const int32_t*)(gath + per), h->nranks, 2 * (payload + 1), qb,
                               (int32_t*)(keys + per));
        }
        if (nr == ncclSuccess && merge_keys(dc, gath, h->nranks, qb, s.k, keys, payload + 1, status_out, st)) {
            const std::string why = fir_last_error();
            return comm_dead(dc, h->health, FIR_ERR_HIP, why.c_str());
        }
    }
    if (nr != ncclSuccess) return comm_dead(dc, h->health, FIR_ERR_COMM, ncclGetErrorString(nr));
#ifdef FIR_AUDIT
    // fail_step = 3 (audit build): from the handle's SECOND exchange on the status element comes BACK poisoned, as if a peer's scan had
    // failed -- this rank's own work is fine (the first call of a handle grows its buffers in the agreed, blocking step: a test of the
    // asynchronous path needs one clean call in front)
    if (inject_here(h, dc, 3) && h->health.exchanges_done++ >= 1) hipLaunchKernelGGL(k_shard_set_u64, dim3(1), dim3(1), 0, st, keys + payload, status_key(FIR_ERR_NOMEM));
#endif
    if (prof && dc.ev_used + 2 <= dc.evs.size()) {
        (void)hipEventRecord(dc.evs[dc.ev_used + 1], st);
        dc.ev_used += 2;
    }
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return comm_dead(dc, h->health, FIR_ERR_HIP, hipGetErrorString(e));
    return FIR_OK;
}

// class of every winning row: the rank that holds the row knows it, everyone else contributes INT32_MAX; dc.cls[qb] is the
// status element (INT32_MAX = fine, a negative FIR_ERR_* otherwise: the minimum finds it)
int device_classes(fir_sharded* h, int slot, const uint64_t* keys, int32_t qb, hipStream_t st, int local_rc) {
    DevCtx& dc = h->devs[slot];
    int32_t* cls = dc.cls.as<int32_t>();
    hipLaunchKernelGGL(k_shard_fill_i32, dim3((qb + 255) / 256), dim3(256), 0, st, cls, qb, 0x7FFFFFFF);
    hipLaunchKernelGGL(k_shard_set_i32, dim3(1), dim3(1), 0, st, cls + qb, local_rc ? local_rc : 0x7FFFFFFF);
    if (!local_rc)
        for (int si : dc.shards) {
            const Shard& s = h->shards[si];
            if (!s.g || !s.cls) continue;
            hipLaunchKernelGGL(k_shard_class_owned, dim3((qb + 255) / 256), dim3(256), 0, st, keys, qb, s.cls, s.lo, s.hi, cls);
        }
    const ncclResult_t nr = ncclAllReduce(cls, cls, (size_t)qb + 1, ncclInt32, ncclMin, dc.comm, st);
    if (nr != ncclSuccess) return comm_dead(dc, h->health, FIR_ERR_COMM, ncclGetErrorString(nr));
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return comm_dead(dc, h->health, FIR_ERR_HIP, hipGetErrorString(e));
    return FIR_OK;
}

int dead_handle(const Health& hl) {
    return fir_fail_(FIR_ERR_STATE, "this sharded handle is closed: an earlier call failed on some rank (code %d); destroy it and create a fresh one", hl.dead_code.load());
}

// Host-pointer search: queries go to every device from pinned memory, keys (and classes: class_out, fir_sharded_classify_top1) come back from device slot 0. hs: the
// host-side twin of the request -- kind, K, radius[qb] in and count[qb] out in HOST memory, no keys: they come back unpacked into idx / dist; each device gets its own `dev`.
int search_host(fir_sharded* h, const float* queries, int32_t qb, int32_t start, int32_t end, const FirSearch& hs, int32_t* idx, float* dist, int32_t* class_out) {
    const bool rad = hs.is_radius(), knn = hs.kind == fir::kSearchSelect, other = hs.kind == fir::kSearchOtherClass;
    const int32_t k = hs.k;
    if (!h || (qb > 0 && !queries) || ((knn || other) && (!idx || !dist)) || (other && qb > 0 && !hs.exclude)) return fir_fail_(FIR_ERR_ARG, "NULL argument");
    if (rad && (!hs.count || (qb > 0 && !hs.radius) || (k >= 1 && k <= FIR_KNN_MAX && (!idx || !dist)) || (k == 0 && (idx || dist)))) return fir_fail_(FIR_ERR_ARG, "NULL argument");
    if (qb < 0) return fir_fail_(FIR_ERR_ARG, "qb < 0");
    const int kmax = knn || rad ? FIR_KNN_MAX : 8;
    if (rad && (k < 0 || k > kmax)) return fir_fail_(FIR_ERR_ARG, "max_results=%d outside [0,%d]", k, kmax);
    if (!rad && (k < 1 || k > kmax)) return fir_fail_(FIR_ERR_ARG, "k=%d outside [1,%d]", k, kmax);
    if ((int64_t)qb * k >= ((int64_t)1 << 31)) return fir_fail_(FIR_ERR_ARG, "qb * k = %lld keys do not fit 32-bit counts", (long long)qb * k);
    if ((class_out || other) && !h->has_labels) return fir_fail_(FIR_ERR_STATE, "the sharded gallery was created without class labels");
    if (h->health.dead) return dead_handle(h->health);
    if (qb == 0) return FIR_OK;
    int rc = check_range(h, start, end);
    if (rc) return rc;
    // (argument errors above are the same on every rank: nobody has entered a collective yet)
    const size_t per = hs.key_words(qb), payload = hs.status_index(qb);
    const size_t rbytes = hs.radii_bytes(qb) + hs.exclude_bytes(qb);                   // the radii (the excluded classes) ride behind the queries, in whole 8 bytes
    const size_t qbytes = (size_t)qb * h->d * sizeof(float) + rbytes, kbytes = (payload + 1) * sizeof(uint64_t), cbytes = ((size_t)qb + 1) * sizeof(int32_t);
    // the pinned staging area is part of the agreed growth as well: slot 0 tries it inside the step
    float* hq = nullptr;
    uint64_t* hk = nullptr;
    int32_t* hc = nullptr;
    fir::Published staged;                                                   // slot 0: the staging area is there (or is not)
    const CallBuffers nb = call_buffers(h, qb, hs, true, class_out != nullptr);
    const bool grows = call_grows(h->devs[0], nb) || qbytes + kbytes + cbytes > h->pin.cap;   // once, before the fan-out (see call_grows)
    rc = h->devs.run_all([&](int slot) -> int {
        DevCtx& dc = h->devs[slot];
        FIR_HIP(hipSetDevice(dc.device));
        Call c{dc, h->health, dc.stream};
        int r = grow_agreed(c, grows, inject_here(h, dc, 2), [&]() -> int {
            int ra = call_alloc(dc, nb);
            if (slot == 0 && !ra) ra = SH_GROW(h->pin, qbytes + kbytes + cbytes, (size_t)1 << 20);
            return ra;
        });
        if (slot == 0) {
            // the other devices of this process read the queries from the staging area slot 0 has just made sure of
            if (!r) {
                hq = h->pin.as<float>();
                hk = (uint64_t*)(h->pin.as<char>() + qbytes);
                hc = (int32_t*)(h->pin.as<char>() + qbytes + kbytes);
                std::memcpy(hq, queries, qbytes - rbytes);
                if (rad) {
                    std::memset(hq + (size_t)qb * h->d, 0, rbytes);
                    std::memcpy(hq + (size_t)qb * h->d, hs.radius, (size_t)qb * sizeof(float));
                }
                if (other) {
                    std::memset(hq + (size_t)qb * h->d, 0, rbytes);
                    std::memcpy(hq + (size_t)qb * h->d, hs.exclude, (size_t)qb * sizeof(int32_t));
                }
            }
            staged.publish(r);
        } else {
            const int r0 = staged.wait();
            if (!r) r = r0;                        // (an agreed failure has r != 0 everywhere already)
        }
        if (r) return r;
        const FirSearch dev{hs.kind, k, 0, nullptr, nullptr, rad ? dc.dq.as<float>() + (size_t)qb * h->d : nullptr, nullptr,
                            other ? (const int32_t*)(dc.dq.as<float>() + (size_t)qb * h->d) : nullptr};   // no host pointer; its radii (excluded classes) lie behind its queries
        // from here on every rank takes part in every collective of the call, whatever happens to it
        keep_local(c, hipMemcpyAsync(dc.dq.p, hq, qbytes, hipMemcpyHostToDevice, dc.stream) != hipSuccess
                          ? fir_fail_(FIR_ERR_HIP, "query upload failed")
                          : device_keys(h, slot, dc.dq.as<float>(), qb, start, end, dev, dc.stream));
        uint64_t* keys = dc.keys.as<uint64_t>();
        if ((r = exchange_keys(h, slot, qb, dev, dc.stream, c.local))) return r;
        if (class_out && (r = device_classes(h, slot, keys, qb, dc.stream, c.local))) return r;
        if (slot == 0) {
            (void)hipMemcpyAsync(hk, keys, kbytes, hipMemcpyDeviceToHost, dc.stream);
            if (class_out) (void)hipMemcpyAsync(hc, dc.cls.p, cbytes, hipMemcpyDeviceToHost, dc.stream);
        } else {
            (void)hipMemcpyAsync(dc.hstat() + 1, keys + payload, sizeof(int32_t), hipMemcpyDeviceToHost, dc.stream);   // low word of the status element
        }
        if ((r = wait_stream(dc, dc.stream, h->health))) return r;
        return verdict(c, FIR_OK);                 // (the peers' status is slot 0's to read, below)
    });
    if (rc) return call_done(h->health, rc);
    int all = status_code(hk[payload]);
    if (!all && class_out && hc[qb] != 0x7FFFFFFF) all = hc[qb];
    if ((rc = peer_verdict(h->health, all))) return rc;
    if (class_out)
        for (int i = 0; i < qb; ++i) class_out[i] = hc[i] == 0x7FFFFFFF ? -1 : hc[i];     // ImageTesting.cpp:63: no row found -> -1
    if (rad) std::memcpy(hs.count, hk + per, (size_t)qb * sizeof(int32_t));
    if ((idx || dist) && per) return fir_keys_unpack(hk, qb * k, idx, dist);
    return FIR_OK;
}

// per-device stream, communicator (rank = first_rank + slot) and, for several devices, worker threads
int setup_devices(Devices& devs, const int32_t* devices, int ndev, int nranks, int first_rank, const void* comm_id) {
    ncclUniqueId id;
    if (comm_id) std::memcpy(&id, comm_id, sizeof id);
    else SH_NCCL(ncclGetUniqueId(&id));
    for (int s = 0; s < ndev; ++s) {
        DevCtx& dc = devs[s];
        dc.device = devices[s];
        FIR_HIP(hipSetDevice(dc.device));
        FIR_HIP(hipStreamCreateWithFlags(&dc.stream, hipStreamNonBlocking));
    }
    for (int s = 0; s < ndev; ++s) {
        DevCtx& dc = devs[s];
        FIR_HIP(hipSetDevice(dc.device));
        int rc;
        if ((rc = FIR_RESERVE(dc.status, 4 * sizeof(int32_t)))) return rc;
        FIR_HIP(hipMemset(dc.status.p, 0, 4 * sizeof(int32_t)));
        if ((rc = FIR_RESERVE(dc.h_status, 8 * sizeof(int32_t)))) return rc;
        std::memset(dc.h_status.p, 0, 8 * sizeof(int32_t));
        void* dp = nullptr;
        FIR_HIP(hipHostGetDevicePointer(&dp, dc.h_status.p, 0));
        dc.d_hsticky = (int32_t*)dp + 3;
        FIR_HIP(hipEventCreateWithFlags(&dc.async_done, hipEventDisableTiming));
    }
    // RCCL writes its version banner to STDOUT when a process's FIRST communicator comes up. The callers of this library print
    // results there (the reference's harnesses, whose output must stay diffable): for that one creation -- serialised by a
    // process-wide mutex -- file descriptor 1 points at stderr. Later communicators print nothing and touch no descriptor.
    static std::mutex banner_mu;
    static bool banner_done = false;
    ncclResult_t nr;
    {
        std::unique_lock<std::mutex> lk(banner_mu);
        const bool first = !banner_done;
        int saved_stdout = -1;
        if (first) {
            std::fflush(stdout);
            saved_stdout = dup(1);
            if (saved_stdout >= 0) (void)dup2(2, 1);
        } else {
            lk.unlock();
        }
        nr = ncclGroupStart();
        for (int s = 0; s < ndev && nr == ncclSuccess; ++s) {
            (void)hipSetDevice(devs[s].device);
            nr = ncclCommInitRank(&devs[s].comm, nranks, id, first_rank + s);
        }
        if (nr == ncclSuccess) nr = ncclGroupEnd(); else (void)ncclGroupEnd();
        if (first) {
            std::fflush(stdout);
            if (saved_stdout >= 0) { (void)dup2(saved_stdout, 1); (void)close(saved_stdout); }
            banner_done = true;
        }
    }
    if (nr != ncclSuccess) return fir_fail_(FIR_ERR_COMM, "RCCL communicator of %d ranks: %s", nranks, ncclGetErrorString(nr));
    if (!devs.workers.start(ndev)) return fir_fail_(FIR_ERR_NOMEM, "host allocation failed");
    return FIR_OK;
}

// The one release of everything setup_devices and the calls made: a handle's destroy and every failing create end here.
// dead: the communicators are aborted, not drained (a collective of theirs may never complete).
void teardown_devices(Devices& devs, bool dead) {
    devs.workers.stop();
    for (DevCtx& dc : devs.ctx) {
        (void)hipSetDevice(dc.device);
        if (dc.stream && !dead) (void)hipStreamSynchronize(dc.stream);
        if (dc.comm) { if (dead) (void)ncclCommAbort(dc.comm); else (void)ncclCommDestroy(dc.comm); }
        dc.status.release();
        dc.h_status.release();
        if (dc.async_done) (void)hipEventDestroy(dc.async_done);
        for (FirBuf* b : {&dc.dq, &dc.parts, &dc.keys, &dc.gath, &dc.cls, &dc.sel}) b->release();
        for (hipEvent_t e : dc.evs) (void)hipEventDestroy(e);
        if (dc.stream) (void)hipStreamDestroy(dc.stream);
    }
    devs.ctx.clear();
}

int check_devices(const int32_t* devices, int32_t ndev) {
    if (!devices || ndev < 1 || ndev > 64) return fir_fail_(FIR_ERR_ARG, "device list of %d entries", ndev);
    for (int i = 0; i < ndev; ++i)
        for (int j = 0; j < i; ++j)
            if (devices[i] == devices[j]) return fir_fail_(FIR_ERR_ARG, "device %d listed twice (use shards_per_device for logical shards)", devices[i]);
    const int cnt = fir_device_count();
    for (int i = 0; i < ndev; ++i)
        if (devices[i] < 0 || devices[i] >= cnt) return fir_fail_(FIR_ERR_NODEVICE, "device %d out of range (%d visible)", devices[i], cnt);
    return FIR_OK;
}

int read_opts(const fir_shard_opts* opts, fir_shard_opts* o) {
    std::memset(o, 0, sizeof *o);
    if (opts) {
        if (opts->struct_bytes < 8 || opts->struct_bytes > (int32_t)sizeof *o) return fir_fail_(FIR_ERR_ARG, "fir_shard_opts.struct_bytes = %d", opts->struct_bytes);
        std::memcpy(o, opts, (size_t)opts->struct_bytes);
    }
    if (o->shards_per_device <= 0) o->shards_per_device = 1;
    if (!o->comm_id) { o->nprocs = 1; o->proc_rank = 0; }
    if (o->shards_per_device > 64) return fir_fail_(FIR_ERR_ARG, "shards_per_device = %d", o->shards_per_device);
    if (o->nprocs < 1 || o->proc_rank < 0 || o->proc_rank >= o->nprocs) return fir_fail_(FIR_ERR_ARG, "process %d of %d", o->proc_rank, o->nprocs);
#ifndef FIR_AUDIT
    // the failure-injection hooks exist in the audit build only (libfir_amd_audit.so): the shipped library refuses them loudly
    if (o->fail_shard != 0 || o->fail_step != 0)
        return fir_fail_(FIR_ERR_ARG, "fir_shard_opts.fail_shard / fail_step are test hooks of the audit build (libfir_amd_audit.so); this library has none");
#endif
    return FIR_OK;
}

// acc[i] += part[i]
__global__ void __launch_bounds__(256) k_shard_add_f64(double* __restrict__ acc, const double* __restrict__ part, int64_t n, int first) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) acc[i] = first ? part[i] : acc[i] + part[i];
}
// best[q] = first maximum of scores[q][0..C) from -DBL_MAX (classification.cpp:217-224); one wave per query
__global__ void __launch_bounds__(64) k_shard_argmax_first(const double* __restrict__ scores, int num_classes, int32_t* __restrict__ best) {
    const int q = blockIdx.x, lane = threadIdx.x;
    const double* s = scores + (size_t)q * num_classes;
    double mx = -1.7976931348623157e308;
    int bi = 0x7FFFFFFF;
    for (int i = lane; i < num_classes; i += 64)
        if (mx < s[i]) { mx = s[i]; bi = i; }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
        const double om = __shfl_xor(mx, o, 64);
        const int oi = __shfl_xor(bi, o, 64);
        if (om > mx || (om == mx && oi < bi)) { mx = om; bi = oi; }
    }
    if (lane == 0) best[q] = bi == 0x7FFFFFFF ? -1 : bi;
}

// merged[q][c][0..k) = the k smallest of parts[p][q][c][0..k), p < nparts (every part ascending, DBL_MAX = no such row)
// stride: doubles from one part to the next (qc * k, or qc * k + 1 with a status element behind every part: then
// status_out <- the largest of those elements; 0 = every rank was fine)
__global__ void __launch_bounds__(256) k_shard_merge_knn(const double* __restrict__ parts, int nparts, int64_t qc /* qb * C */, int k, double* __restrict__ merged,
                                                          size_t stride, double* __restrict__ status_out) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (status_out && i == 0) {
        double m = 0.0;
        for (int p = 0; p < nparts; ++p) m = fmax(m, parts[(size_t)p * stride + (size_t)qc * k]);
        *status_out = m;
    }
    if (i >= qc) return;
    double best[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) best[j] = 1.7976931348623157e308;
    for (int p = 0; p < nparts; ++p)
        for (int j = 0; j < k; ++j) {
            double v = parts[(size_t)p * stride + (size_t)i * k + j];
#pragma unroll
            for (int t = 0; t < 8; ++t) {
                const bool sw = v < best[t];
                const double tmp = best[t];
                best[t] = sw ? v : tmp;
                v = sw ? tmp : v;
            }
        }
    for (int j = 0; j < k; ++j) merged[(size_t)i * k + j] = best[j];
}
// KNNClassifier::predict's vote (classification.cpp:151-168) from the merged lists: the class that first collects k votes in the
// globally sorted order is the one whose k-th nearest member is nearest (first minimum); when no class has k rows the
// reference's loop ends without a break and the largest class (first on ties) wins. One thread per query.
__global__ void __launch_bounds__(64) k_shard_knn_vote(const double* __restrict__ merged, int qb, int num_classes, int k,
                                                       const int32_t* __restrict__ class_count, int32_t* __restrict__ best) {
    const int q = blockIdx.x * 64 + threadIdx.x;
    if (q >= qb) return;
    double mn = 1.7976931348623157e308;
    int b = -1;
    for (int c = 0; c < num_classes; ++c) {
        const double v = class_count[c] >= k ? merged[((size_t)q * num_classes + c) * k + (k - 1)] : 1.7976931348623157e308;
        if (v < mn) { mn = v; b = c; }
    }
    if (b < 0) {
        int mc = -1;
        for (int c = 0; c < num_classes; ++c)
            if (class_count[c] > mc) { mc = class_count[c]; b = c; }
    }
    best[q] = b;
}

}  // namespace

struct fir_cls_sharded {
    int d = 0, num_classes = 0, ndev = 0, nranks = 1;
    int64_t nt_local = 0;
    Devices devs;
    std::vector<fir_cls*> parts;       // the training-set shards, device-major; nullptr: no rows
    struct Dev {                       // per device
        std::vector<int> parts;        // the shards it holds (indices into parts)
        FirBuf acc;                    // double: summed class scores [qb][C] + the status element
        FirBuf best;                   // int32_t [qb]
        FirBuf class_count;            // int32_t: training rows per class over ALL shards and ranks
        FirBuf knn;                    // double: [shards here + nranks][qb][C][k] lists being merged
    };
    std::vector<Dev> cdev;
    FirPinBuf pin;
    Health health;
};

namespace {

// the test hook: is this the part whose step is made to fail (by its index among all parts of the handle)? does the device hold it?
bool cls_inject(const fir_cls_sharded* h, int part_index, int step) { return h->health.fail_step == step && h->health.fail_shard - 1 == part_index; }
bool cls_inject_dev(const fir_cls_sharded* h, int slot, int step) {
    for (int pi : h->cdev[(size_t)slot].parts)
        if (cls_inject(h, pi, step)) return true;
    return false;
}
// scan(shard) for every shard of this device that has rows, until one fails
template <typename Scan>
int cls_scan_parts(const fir_cls_sharded* h, const fir_cls_sharded::Dev& cd, Scan scan) {
    int rc;
    for (int pi : cd.parts) {
        if (cls_inject(h, pi, 1)) return fir_fail_(FIR_ERR_NOMEM, "injected scan failure on training-set shard %d (fir_shard_opts.fail_step = 1)", pi);
        if (h->parts[(size_t)pi] && (rc = scan(h->parts[(size_t)pi]))) return rc;
    }
    return FIR_OK;
}

// The allocations of a classifier call on one device, in its agreed step: the call's table (knn or acc, its exact size), best
// (no fewer than 4 096 ints) and, on slot 0, the staging area (no smaller than pin_floor).
struct ClsBuffers { size_t table, best, pin, pin_floor; };
// ... and whether the call grows anything: once per call, before the fan-out, of slot 0's capacities -- see call_grows
bool cls_grows(const fir_cls_sharded* h, const FirBuf& table0, const ClsBuffers& b) {
    return b.table > table0.cap || b.best > h->cdev[0].best.cap || b.pin > h->pin.cap;
}
int cls_alloc(fir_cls_sharded* h, int slot, FirBuf& table, const ClsBuffers& b) {
    int rc;
    if ((rc = SH_GROW(table, b.table, 0))) return rc;
    if ((rc = SH_GROW(h->cdev[(size_t)slot].best, b.best, 4096 * sizeof(int32_t)))) return rc;
    return slot == 0 ? SH_GROW(h->pin, b.pin, b.pin_floor) : FIR_OK;
}

}  // namespace

extern "C" {

int fir_cls_sharded_destroy(fir_cls_sharded* h) {
    if (!h) return FIR_OK;
    for (fir_cls* c : h->parts)
        if (c) fir_cls_destroy(c);
    for (size_t s = 0; s < h->devs.ctx.size(); ++s) {      // (a device's buffers go while it is the current one)
        (void)hipSetDevice(h->devs[(int)s].device);
        for (FirBuf* b : {&h->cdev[s].acc, &h->cdev[s].best, &h->cdev[s].class_count, &h->cdev[s].knn}) b->release();
    }
    teardown_devices(h->devs, h->health.dead);
    delete h;
    return FIR_OK;
}

int fir_cls_create_sharded(const double* train_rows, int64_t nt, int32_t d, const int32_t* train_class, int32_t num_classes, const double* avg,
                           const int32_t* devices, int32_t ndev, const fir_shard_opts* opts, fir_cls_sharded** out) {
    if (!out) return fir_fail_(FIR_ERR_ARG, "out is NULL");
    *out = nullptr;
    if (nt < 0 || d <= 0 || num_classes <= 0 || !avg || (nt > 0 && (!train_rows || !train_class))) return fir_fail_(FIR_ERR_ARG, "bad training set (nt=%lld d=%d classes=%d)", (long long)nt, d, num_classes);
    int rc = check_devices(devices, ndev);
    if (rc) return rc;
    fir_shard_opts o;
    if ((rc = read_opts(opts, &o))) return rc;
    if (o.rows_on_device) return fir_fail_(FIR_ERR_ARG, "fir_cls_create_sharded takes host rows");
    fir_cls_sharded* h = new (std::nothrow) fir_cls_sharded();
    if (!h) return fir_fail_(FIR_ERR_NOMEM, "host allocation failed");
    h->d = d; h->num_classes = num_classes; h->ndev = ndev; h->nranks = o.nprocs * ndev; h->nt_local = nt;
    h->health.apply(o);
    h->devs.ctx = std::vector<DevCtx>((size_t)ndev);
    h->cdev = std::vector<fir_cls_sharded::Dev>((size_t)ndev);
    const int spd = o.shards_per_device, nsh = ndev * spd;
    const int64_t total = o.total_rows > 0 ? o.total_rows : nt;
    const int64_t per = (((nt + 63) / 64 + nsh - 1) / nsh) * 64;
    for (int s = 0; s < nsh && rc == FIR_OK; ++s) {
        const int64_t lo = std::min<int64_t>((int64_t)s * per, nt), hi = std::min<int64_t>((int64_t)(s + 1) * per, nt);
        fir_cls* c = nullptr;
        if (hi > lo) {
            rc = fir_cls_create(train_rows + lo * d, hi - lo, d, train_class + lo, num_classes, avg, devices[s / spd], &c);
            if (rc == FIR_OK) rc = fir_cls_set_total_training_size(c, total);     // classification.cpp:215: every partial sum over the global N
        }
        h->cdev[(size_t)(s / spd)].parts.push_back(s);
        h->parts.push_back(c);
    }
    if (rc == FIR_OK) rc = setup_devices(h->devs, devices, ndev, h->nranks, o.proc_rank * ndev, o.comm_id);
    // rows per class over all shards and ranks (the kNN vote's "class has k rows" and its largest-class rule)
    if (rc == FIR_OK) {
        std::vector<int32_t> cnt((size_t)num_classes, 0);
        for (int64_t t = 0; t < nt; ++t)
            if (train_class[t] >= 0 && train_class[t] < num_classes) cnt[(size_t)train_class[t]]++;
        rc = h->devs.run_all([&](int slot) -> int {
            DevCtx& dc = h->devs[slot];
            FIR_HIP(hipSetDevice(dc.device));
            FirBuf& count = h->cdev[(size_t)slot].class_count;
            const int ra = FIR_RESERVE(count, (size_t)num_classes * sizeof(int32_t));
            if (ra) return ra;
            int32_t* cc = count.as<int32_t>();
            if (slot == 0) FIR_HIP(hipMemcpyAsync(cc, cnt.data(), (size_t)num_classes * sizeof(int32_t), hipMemcpyHostToDevice, dc.stream));
            else FIR_HIP(hipMemsetAsync(cc, 0, (size_t)num_classes * sizeof(int32_t), dc.stream));      // this process's rows are counted once
            SH_NCCL(ncclAllReduce(cc, cc, (size_t)num_classes, ncclInt32, ncclSum, dc.comm, dc.stream));
            return wait_stream(dc, dc.stream, h->health);
        });
    }
    if (rc) { fir_cls_sharded_destroy(h); return rc; }
    *out = h;
    return FIR_OK;
}

int fir_cls_sharded_knn_predict(fir_cls_sharded* h, const double* queries, int32_t qb, int32_t k, int32_t* best_class) {
    if (!h || !best_class || (qb > 0 && !queries)) return fir_fail_(FIR_ERR_ARG, "NULL argument");
    if (qb < 0) return fir_fail_(FIR_ERR_ARG, "qb < 0");
    if (k < 1 || k > 8) return fir_fail_(FIR_ERR_ARG, "k=%d outside [1,8]", k);
    if (h->health.dead) return dead_handle(h->health);
    if (qb == 0) return FIR_OK;
    int32_t maxb = 1 << 30;
    for (fir_cls* c : h->parts)
        if (c) { int32_t mb = 0; double* ds; void* st; fir_cls_knn_nearest_dev_(c, nullptr, 0, k, &ds, &st, &mb); maxb = std::min(maxb, mb); }
    maxb = std::min(maxb, 1024);
    if (qb > maxb) {
        for (int32_t q0 = 0; q0 < qb; q0 += maxb) {
            const int rc0 = fir_cls_sharded_knn_predict(h, queries + (size_t)q0 * h->d, std::min(maxb, qb - q0), k, best_class + q0);
            if (rc0) return rc0;
        }
        return FIR_OK;
    }
    const size_t per = (size_t)qb * h->num_classes * k;                       // doubles in one [qb][C][k] table
    size_t max_parts = 1;
    for (const auto& cd : h->cdev) {
        size_t np = 0;
        for (int pi : cd.parts) np += h->parts[(size_t)pi] ? 1 : 0;
        max_parts = std::max(max_parts, np);
    }
    // [max_parts] shard tables | their merge + status element | [nranks] gathered tables + status elements | the merge over the ranks + status
    const size_t need = per * max_parts + (per + 1) + (per + 1) * (size_t)h->nranks + (per + 1);
    const ClsBuffers nb{need * sizeof(double), (size_t)qb * sizeof(int32_t), ((size_t)qb + 2) * sizeof(int32_t) + sizeof(double), 4096 * sizeof(int32_t) + 64};
    const bool grows = cls_grows(h, h->cdev[0].knn, nb);
    const int64_t qc = (int64_t)qb * h->num_classes;
    const int rc = h->devs.run_all([&](int slot) -> int {
        DevCtx& dc = h->devs[slot];
        fir_cls_sharded::Dev& cd = h->cdev[(size_t)slot];
        FIR_HIP(hipSetDevice(dc.device));
        Call c{dc, h->health, dc.stream};
        int r = grow_agreed(c, grows, cls_inject_dev(h, slot, 2), [&]() -> int { return cls_alloc(h, slot, cd.knn, nb); });
        if (r) return r;
        double* parts = cd.knn.as<double>();                                  // [max_parts] tables of the shards held here
        double* mine = parts + per * max_parts;                               // their merge (+ status element)
        double* gath = mine + per + 1;                                        // [nranks] tables (+ status elements)
        double* all = gath + (per + 1) * (size_t)h->nranks;                   // the merge over the ranks (+ the worst status)
        int np = 0;
        keep_local(c, cls_scan_parts(h, cd, [&](fir_cls* shard) -> int {
            double* dl = nullptr;
            void* st = nullptr;
            const int rs = fir_cls_knn_nearest_dev_(shard, queries, qb, k, &dl, &st, nullptr);
            if (rs) return rs;
            if (hipStreamSynchronize((hipStream_t)st) != hipSuccess ||
                hipMemcpyAsync(parts + per * (size_t)np++, dl, per * sizeof(double), hipMemcpyDeviceToDevice, dc.stream) != hipSuccess)
                return fir_fail_(FIR_ERR_HIP, "copying a shard's k-nearest table failed");
            return FIR_OK;
        }));
        const int local = c.local;
        if (local) np = 0;
        hipLaunchKernelGGL(k_shard_merge_knn, dim3((unsigned)((qc + 255) / 256)), dim3(256), 0, dc.stream, parts, np, qc, k, mine, per, (double*)nullptr);   // np == 0: all DBL_MAX
        hipLaunchKernelGGL(k_shard_set_f64, dim3(1), dim3(1), 0, dc.stream, mine + per, local ? (double)(-local) : 0.0);
        const ncclResult_t nr = ncclAllGather(mine, gath, per + 1, ncclDouble, dc.comm, dc.stream);
        if (nr != ncclSuccess) return comm_dead(dc, h->health, FIR_ERR_COMM, ncclGetErrorString(nr));
        hipLaunchKernelGGL(k_shard_merge_knn, dim3((unsigned)((qc + 255) / 256)), dim3(256), 0, dc.stream, gath, h->nranks, qc, k, all, per + 1, all + per);
        hipLaunchKernelGGL(k_shard_knn_vote, dim3((qb + 63) / 64), dim3(64), 0, dc.stream, all, qb, h->num_classes, k, cd.class_count.as<int32_t>(),
                           cd.best.as<int32_t>());
        double* hst = slot == 0 ? (double*)(h->pin.as<char>() + (((size_t)qb * sizeof(int32_t) + 7) & ~(size_t)7)) : (double*)(dc.hstat() + 4);
        (void)hipMemcpyAsync(hst, all + per, sizeof(double), hipMemcpyDeviceToHost, dc.stream);
        if (slot == 0) (void)hipMemcpyAsync(h->pin.p, cd.best.p, (size_t)qb * sizeof(int32_t), hipMemcpyDeviceToHost, dc.stream);
        if ((r = wait_stream(dc, dc.stream, h->health))) return r;
        return verdict(c, -(int)*hst);                                        // the status element: the largest -FIR_ERR_* of any rank
    });
    if (rc) return call_done(h->health, rc);
    std::memcpy(best_class, h->pin.p, (size_t)qb * sizeof(int32_t));
    return FIR_OK;
}

int fir_cls_sharded_pnn_predict(fir_cls_sharded* h, const double* queries, int32_t qb, double var, double* scores, int32_t* best_class) {
    if (!h || (qb > 0 && !queries)) return fir_fail_(FIR_ERR_ARG, "NULL argument");
    if (qb < 0) return fir_fail_(FIR_ERR_ARG, "qb < 0");
    if (h->health.dead) return dead_handle(h->health);
    if (qb == 0) return FIR_OK;
    // internal batches: what every shard's distance table allows (fir_cls_pnn_scores_dev_)
    int32_t maxb = 1 << 30;
    for (fir_cls* c : h->parts)
        if (c) { int32_t mb = 0; double* ds; void* st; fir_cls_pnn_scores_dev_(c, nullptr, 0, var, &ds, &st, &mb); maxb = std::min(maxb, mb); }
    maxb = std::min(maxb, 4096);
    if (qb > maxb) {
        for (int32_t q0 = 0; q0 < qb; q0 += maxb) {
            const int rc0 = fir_cls_sharded_pnn_predict(h, queries + (size_t)q0 * h->d, std::min(maxb, qb - q0), var,
                                                        scores ? scores + (size_t)q0 * h->num_classes : nullptr, best_class ? best_class + q0 : nullptr);
            if (rc0) return rc0;
        }
        return FIR_OK;
    }
    const size_t nsc = (size_t)qb * h->num_classes;
    const size_t pin_need = (nsc + 1) * sizeof(double) + (size_t)qb * sizeof(int32_t);
    const ClsBuffers nb{(nsc + 1) * sizeof(double), (size_t)qb * sizeof(int32_t), pin_need, 0};
    const bool grows = cls_grows(h, h->cdev[0].acc, nb);
    const int rc = h->devs.run_all([&](int slot) -> int {
        DevCtx& dc = h->devs[slot];
        fir_cls_sharded::Dev& cd = h->cdev[(size_t)slot];
        FIR_HIP(hipSetDevice(dc.device));
        Call c{dc, h->health, dc.stream};
        int r = grow_agreed(c, grows, cls_inject_dev(h, slot, 2), [&]() -> int { return cls_alloc(h, slot, cd.acc, nb); });
        if (r) return r;
        double* acc = cd.acc.as<double>();
        int first = 1;
        keep_local(c, cls_scan_parts(h, cd, [&](fir_cls* shard) -> int {
            double* ds = nullptr;
            void* st = nullptr;
            const int rs = fir_cls_pnn_scores_dev_(shard, queries, qb, var, &ds, &st, nullptr);
            if (rs) return rs;
            if (hipStreamSynchronize((hipStream_t)st) != hipSuccess) return fir_fail_(FIR_ERR_HIP, "a shard's class scores did not complete");   // the shard's own stream
            hipLaunchKernelGGL(k_shard_add_f64, dim3((unsigned)((nsc + 255) / 256)), dim3(256), 0, dc.stream, acc, ds, (int64_t)nsc, first);
            first = 0;
            return FIR_OK;
        }));
        const int local = c.local;
        if (first || local) (void)hipMemsetAsync(acc, 0, nsc * sizeof(double), dc.stream);     // a device without rows (or whose step failed) adds nothing
        hipLaunchKernelGGL(k_shard_set_f64, dim3(1), dim3(1), 0, dc.stream, acc + nsc, local ? 1.0 : 0.0);   // the status element: the sum counts the ranks that failed
        const ncclResult_t nr = ncclAllReduce(acc, acc, nsc + 1, ncclDouble, ncclSum, dc.comm, dc.stream);
        if (nr != ncclSuccess) return comm_dead(dc, h->health, FIR_ERR_COMM, ncclGetErrorString(nr));
        hipLaunchKernelGGL(k_shard_argmax_first, dim3(qb), dim3(64), 0, dc.stream, acc, h->num_classes, cd.best.as<int32_t>());
        double* hst = slot == 0 ? h->pin.as<double>() + nsc : (double*)(dc.hstat() + 4);
        if (slot == 0) {
            (void)hipMemcpyAsync(h->pin.p, acc, (nsc + 1) * sizeof(double), hipMemcpyDeviceToHost, dc.stream);
            (void)hipMemcpyAsync(h->pin.as<char>() + (nsc + 1) * sizeof(double), cd.best.p, (size_t)qb * sizeof(int32_t), hipMemcpyDeviceToHost, dc.stream);
        } else {
            (void)hipMemcpyAsync(hst, acc + nsc, sizeof(double), hipMemcpyDeviceToHost, dc.stream);
        }
        if ((r = wait_stream(dc, dc.stream, h->health))) return r;
        return verdict(c, *hst != 0.0 ? FIR_ERR_COMM : FIR_OK);               // a count of failed ranks: it cannot say which error
    });
    if (rc) return call_done(h->health, rc);
    if (scores) std::memcpy(scores, h->pin.p, nsc * sizeof(double));
    if (best_class) std::memcpy(best_class, h->pin.as<char>() + (nsc + 1) * sizeof(double), (size_t)qb * sizeof(int32_t));
    return FIR_OK;
}

int fir_comm_unique_id(void* id_out) {
    if (!id_out) return fir_fail_(FIR_ERR_ARG, "id_out is NULL");
    static_assert(sizeof(ncclUniqueId) <= FIR_COMM_ID_BYTES, "FIR_COMM_ID_BYTES too small");
    ncclUniqueId id;
    SH_NCCL(ncclGetUniqueId(&id));
    std::memset(id_out, 0, FIR_COMM_ID_BYTES);
    std::memcpy(id_out, &id, sizeof id);
    return FIR_OK;
}

int fir_sharded_destroy(fir_sharded* h) {
    if (!h) return FIR_OK;
    for (Shard& s : h->shards)
        if (s.g) fir_gallery_destroy(s.g);
    teardown_devices(h->devs, h->health.dead);
    delete h;
    return FIR_OK;
}

int fir_gallery_create_sharded_ex(const float* rows, int64_t n, int32_t d, const int32_t* class_no, int32_t metric, const int32_t* devices,
                                  int32_t ndev, const fir_shard_opts* opts, fir_sharded** out) {
    if (!out) return fir_fail_(FIR_ERR_ARG, "out is NULL");
    *out = nullptr;
    int rc = check_devices(devices, ndev);
    if (rc) return rc;
    if (n < 0 || d <= 0 || (n > 0 && !rows)) return fir_fail_(FIR_ERR_ARG, "bad gallery shape n=%lld d=%d", (long long)n, d);
    fir_shard_opts o;
    if ((rc = read_opts(opts, &o))) return rc;
    const int spd = o.shards_per_device;
    if (o.rows_on_device && ndev != 1) return fir_fail_(FIR_ERR_ARG, "device-resident rows need a one-entry device list (they live on one device)");
    if (o.first_global_row < 0 || o.first_global_row + n >= ((int64_t)1 << 31)) return fir_fail_(FIR_ERR_ARG, "rows [%lld, +%lld) do not fit 32-bit indices", (long long)o.first_global_row, (long long)n);
    if (o.fail_shard < 0 || o.fail_shard > ndev * spd) return fir_fail_(FIR_ERR_ARG, "fail_shard = %d of %d shards", o.fail_shard, ndev * spd);

    fir_sharded* h = new (std::nothrow) fir_sharded();
    if (!h) return fir_fail_(FIR_ERR_NOMEM, "host allocation failed");
    h->d = d; h->metric = metric; h->n_local = n; h->first_row = o.first_global_row;
    h->ndev = ndev; h->spd = spd; h->nranks = o.nprocs * ndev; h->rank0 = o.proc_rank * ndev;
    h->has_labels = class_no != nullptr;
    h->health.apply(o);
    h->devs.ctx = std::vector<DevCtx>((size_t)ndev);

    // shards: whole 64-row tiles, contiguous, device-major (device i holds shards i*spd .. i*spd+spd-1)
    const int nsh = ndev * spd;
    const int64_t tiles = (n + fir::kTileRows - 1) / fir::kTileRows;
    const int64_t per = ((tiles + nsh - 1) / nsh) * fir::kTileRows;
    h->shards.resize((size_t)nsh);
    for (int s = 0; s < nsh && rc == FIR_OK; ++s) {
        Shard& sh = h->shards[(size_t)s];
        sh.slot = s / spd;
        const int64_t lo = std::min<int64_t>((int64_t)s * per, n), hi = std::min<int64_t>((int64_t)(s + 1) * per, n);
        sh.lo = o.first_global_row + lo;
        sh.hi = o.first_global_row + hi;
        h->devs[sh.slot].shards.push_back(s);
        if (hi <= lo) continue;
        const int dev = devices[sh.slot];
        if (o.rows_on_device) rc = fir_gallery_create_dev(rows + lo * d, hi - lo, d, class_no ? class_no + lo : nullptr, metric, dev, nullptr, &sh.g);
        else rc = fir_gallery_create(rows + lo * d, hi - lo, d, class_no ? class_no + lo : nullptr, metric, dev, &sh.g);
        if (rc == FIR_OK) rc = fir_gallery_set_row_offset(sh.g, sh.lo);
        if (rc == FIR_OK) fir_gallery_set_borrowed_(sh.g, 1);      // (fir_sharded_shard lends it: its rows are this handle's bookkeeping)
        if (rc == FIR_OK) {
            fir_gallery_view v;
            fir_gallery_view_(sh.g, &v);
            sh.cls = v.cls;
        }
    }
    // per-device stream, communicator (rank = proc * ndev + slot), worker threads
    if (rc == FIR_OK) rc = setup_devices(h->devs, devices, ndev, h->nranks, h->rank0, o.comm_id);
    if (rc) { fir_sharded_destroy(h); return rc; }
    *out = h;
    return FIR_OK;
}

int fir_gallery_create_sharded(const float* rows, int64_t n, int32_t d, const int32_t* class_no, int32_t metric, const int32_t* devices,
                               int32_t ndev, fir_sharded** out) {
    return fir_gallery_create_sharded_ex(rows, n, d, class_no, metric, devices, ndev, nullptr, out);
}

int fir_sharded_info(const fir_sharded* h, int64_t* n_local, int32_t* d, int32_t* ndev, int32_t* nshards, int32_t* nranks, int32_t* first_rank) {
    if (!h) return fir_fail_(FIR_ERR_ARG, "handle is NULL");
    if (n_local) *n_local = h->n_local;
    if (d) *d = h->d;
    if (ndev) *ndev = h->ndev;
    if (nshards) *nshards = (int32_t)h->shards.size();
    if (nranks) *nranks = h->nranks;
    if (first_rank) *first_rank = h->rank0;
    return FIR_OK;
}

int fir_sharded_shard(fir_sharded* h, int32_t i, fir_gallery** g, int64_t* first_global_row, int64_t* rows) {
    if (!h || i < 0 || i >= (int32_t)h->shards.size()) return fir_fail_(FIR_ERR_ARG, "shard %d of %d", i, h ? (int)h->shards.size() : 0);
    if (g) *g = h->shards[(size_t)i].g;
    if (first_global_row) *first_global_row = h->shards[(size_t)i].lo;
    if (rows) *rows = h->shards[(size_t)i].hi - h->shards[(size_t)i].lo;
    return FIR_OK;
}

int fir_sharded_set_metric(fir_sharded* h, int32_t metric) {
    if (!h) return fir_fail_(FIR_ERR_ARG, "handle is NULL");
    for (Shard& s : h->shards)
        if (s.g) { const int rc = fir_gallery_set_metric(s.g, metric); if (rc) return rc; }
    h->metric = metric;
    return FIR_OK;
}

int fir_sharded_search_top1(fir_sharded* h, const float* queries, int32_t qb, int32_t start_pos, int32_t end_pos, int32_t* idx, float* dist) {
    return search_host(h, queries, qb, start_pos, end_pos, FirSearch::rows(1, nullptr), idx, dist, nullptr);
}

int fir_sharded_search_topk(fir_sharded* h, const float* queries, int32_t qb, int32_t start_pos, int32_t end_pos, int32_t k, int32_t* idx,
                            float* dist) {
    return search_host(h, queries, qb, start_pos, end_pos, FirSearch::rows(k, nullptr), idx, dist, nullptr);
}

int fir_sharded_search_knn(fir_sharded* h, const float* queries, int32_t qb, int32_t start_pos, int32_t end_pos, int32_t k, int32_t* idx,
                           float* dist) {
    return search_host(h, queries, qb, start_pos, end_pos, FirSearch::select(k, nullptr), idx, dist, nullptr);
}

int fir_sharded_search_top1_other_class(fir_sharded* h, const float* queries, int32_t qb, int32_t start_pos, int32_t end_pos, const int32_t* exclude_class,
                                        int32_t* idx, float* dist) {
    return search_host(h, queries, qb, start_pos, end_pos, FirSearch::other_class(exclude_class, nullptr), idx, dist, nullptr);
}

int fir_sharded_search_radius(fir_sharded* h, const float* queries, int32_t qb, int32_t start_pos, int32_t end_pos, const float* radius,
                              int32_t max_results, int32_t* count, int32_t* idx, float* dist) {
    return search_host(h, queries, qb, start_pos, end_pos, FirSearch::within(radius, max_results, count, nullptr), idx, dist, nullptr);
}

int fir_sharded_classify_top1(fir_sharded* h, const float* queries, int32_t qb, int32_t start_pos, int32_t end_pos, int32_t* class_out,
                              int32_t* idx, float* dist) {
    if (!class_out) return fir_fail_(FIR_ERR_ARG, "class_out is NULL");
    return search_host(h, queries, qb, start_pos, end_pos, FirSearch::rows(1, nullptr), idx, dist, class_out);
}

int fir_sharded_search_top1_keys_dev(fir_sharded* h, const float* d_queries, int32_t qb, int32_t start_pos, int32_t end_pos, uint64_t* d_keys,
                                     void* stream) {
    if (!h || !d_keys || (qb > 0 && !d_queries)) return fir_fail_(FIR_ERR_ARG, "NULL argument");
    if (h->ndev != 1) return fir_fail_(FIR_ERR_STATE, "device-pointer calls need a one-device handle (one process per GPU); this one lists %d", h->ndev);
    if (qb < 0) return fir_fail_(FIR_ERR_ARG, "qb < 0");
    if (h->health.dead) return dead_handle(h->health);
    if (qb == 0) return FIR_OK;
    int rc = check_range(h, start_pos, end_pos);
    if (rc) return rc;
    DevCtx& dc = h->devs[0];
    FIR_HIP(hipSetDevice(dc.device));
    Call c{dc, h->health, stream ? (hipStream_t)stream : dc.stream};
    // What the previous asynchronous call found, if it is through (no waiting here): a peer's failure closes the handle BEFORE this rank
    // enqueues another collective that the failed peer -- dead since that call -- will never enter. A previous call that is still in
    // flight is the caller's to order (fir_amd.h: fir_sharded_sync between asynchronous calls whose failure must not be outrun).
    if (dc.async_pending && hipEventQuery(dc.async_done) == hipSuccess) {
        dc.async_pending = false;
        if (dc.hstat()[3] < 0) return peer_verdict(h->health, dc.hstat()[3]);
    }
    (void)hipGetLastError();
    const FirSearch top1 = FirSearch::rows(1, d_keys);
    const CallBuffers nb = call_buffers(h, qb, top1, false, false);
    if ((rc = grow_agreed(c, call_grows(dc, nb), inject_here(h, dc, 2), [&]() -> int { return call_alloc(dc, nb); }))) return rc;
    // every rank enters the exchange; one whose scans failed sends FIR_KEY_NONE keys and a poisoned status element, returns its
    // error here, and the others find it in fir_sharded_sync (the call is asynchronous: nobody waits for the exchange here)
    keep_local(c, device_keys(h, 0, d_queries, qb, start_pos, end_pos, top1, c.st));
    if ((rc = exchange_keys(h, 0, qb, top1, c.st, c.local))) return rc;
    uint64_t* keys = dc.keys.as<uint64_t>();
    hipLaunchKernelGGL(k_shard_note_status, dim3(1), dim3(1), 0, c.st, keys + qb, dc.dstat() + 1, dc.d_hsticky);
    (void)hipMemcpyAsync(d_keys, keys, (size_t)qb * sizeof(uint64_t), hipMemcpyDeviceToDevice, c.st);
    (void)hipEventRecord(dc.async_done, c.st);         // what fir_sharded_sync (and the next call's look at the status) waits for: the stream may be the caller's
    dc.async_pending = true;
    if ((rc = verdict(c, FIR_OK))) return rc;          // (a peer's error is the next call's, or fir_sharded_sync's, to find)
    FIR_HIP(hipGetLastError());
    return FIR_OK;
}

int fir_sharded_sync(fir_sharded* h) {
    if (!h) return fir_fail_(FIR_ERR_ARG, "handle is NULL");
    if (h->health.dead) return dead_handle(h->health);
    for (DevCtx& dc : h->devs.ctx) {
        FIR_HIP(hipSetDevice(dc.device));
        int rc;
        // the last asynchronous call ran on whatever stream its caller named: its completion is the event recorded behind it, waited for
        // with the same bound as every other wait behind a collective (the handle's own stream says nothing about it)
        if (dc.async_pending && (rc = wait_event(dc, dc.async_done, h->health))) return rc;
        dc.async_pending = false;
        if ((rc = wait_stream(dc, dc.stream, h->health))) return rc;
        // the asynchronous calls' record: the worst status any exchange since the last sync came back with (device word and its host mirror)
        FIR_HIP(hipMemcpyAsync(dc.hstat() + 2, dc.dstat() + 1, sizeof(int32_t), hipMemcpyDeviceToHost, dc.stream));
        if ((rc = wait_stream(dc, dc.stream, h->health))) return rc;
        const int32_t worst = std::min(dc.hstat()[2], dc.hstat()[3]);
        if (worst < 0) return peer_verdict(h->health, worst);
    }
    return FIR_OK;
}

int fir_sharded_profile_enable(fir_sharded* h, int32_t on) {
    if (!h) return fir_fail_(FIR_ERR_ARG, "handle is NULL");
    h->profiling = on != 0;
    h->devs[0].ev_used = 0;
    return FIR_OK;
}

int fir_sharded_profile_read(fir_sharded* h, float* exchange_ms, int32_t cap, int32_t* count) {
    if (!h) return fir_fail_(FIR_ERR_ARG, "handle is NULL");
    DevCtx& dc = h->devs[0];
    FIR_HIP(hipSetDevice(dc.device));
    const int32_t have = (int32_t)(dc.ev_used / 2);
    for (int32_t i = 0; i < have; ++i) {
        FIR_HIP(hipEventSynchronize(dc.evs[2 * (size_t)i + 1]));
        float ms = 0.f;
        FIR_HIP(hipEventElapsedTime(&ms, dc.evs[2 * (size_t)i], dc.evs[2 * (size_t)i + 1]));
        if (exchange_ms && i < cap) exchange_ms[i] = ms;
    }
    if (count) *count = have;
    dc.ev_used = 0;
    return FIR_OK;
}

}  // extern "C"
