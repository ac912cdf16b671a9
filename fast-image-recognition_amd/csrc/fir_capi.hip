// fir_capi.hip -- the C ABI (include/fir_amd.h) over the gfx950 kernels in fir_kernels.h.
//
// Host side of the drop-in boundary: owns device buffers, streams and launch geometry.
// Nothing here computes a distance on the host; without a HIP device every entry point fails.
#include "fir_kernels.h"

#include <algorithm>
#include <cfloat>
#include <chrono>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <new>
#include <string>
#include <vector>

#include "../../include/fir_amd.h"
#include "fir_internal.h"
#include "fir_knn_select.h"
#include "fir_search_request.h"

using namespace fir;

namespace {

thread_local char g_err[512] = "";     // what fir_last_error() returns; written by fir_fail_ and fir_set_last_error_

constexpr int kU = 8;        // float4 chunks per lane per load group (8 KiB per wave in flight per group)
constexpr int kUDeep = 16;   // ... of the few-tiles form of a one-query tile
constexpr int kUSub = 8;     // ... of k_scan_subranges: sub-ranges are multiples of 32 features
constexpr int kWps = 4;      // waves per SIMD the scan kernels are register-budgeted for (<= 128 VGPRs)
// The plain-range chi-square / KL kernels and the nomination metrics pair their operands for v_pk_fma_f32 and want more registers
// (with 128 the chi-square loop spills, and every reload waits for the gallery loads in flight); pick_waves never asks for more than 3.
constexpr int kWpsPlain = 3;
constexpr int kKMax = 8;     // per-lane candidate list length of the top-K scan

}  // namespace

// A FirBuf that reads as the T* it holds (fir_gemm.hip's GemmBuf). need(): the handle's workspaces -- `elems` elements are
// max(elems, 4096) of them when the buffer has to be (re)allocated; one that is large enough is not touched.
template <typename T>
struct GalleryBuf : FirBuf {
    operator T*() const { return (T*)p; }
    int need(size_t elems, const char* what, const char* file, int line) {
        if (elems * sizeof(T) <= cap) return FIR_OK;
        return fir_reserve_(*this, std::max(elems, (size_t)4096) * sizeof(T), what, file, line);
    }
};
#define FIR_NEED(buf, elems) (buf).need(elems, #buf, __FILE__, __LINE__)

// Everything the handle holds releases itself: the buffers below are FirBufs, and the destructor takes care of what is not
// memory. Nothing in this file frees by hand.
struct fir_gallery {
    int device = 0;
    int cus = 0;
    int64_t n = 0;
    int d = 0, dp4 = 0;
    int64_t tiles = 0;
    int metric = FIR_METRIC_L2;
    int64_t row_offset = 0;
    GalleryBuf<float4> gal4;      // the tiled rows (fir_kernels.h layout) ...
    GalleryBuf<int32_t> cls;      // ... and their labels (empty: created without): fir_gallery_memory_bytes' `tiled`
    // in-place updates (fir_gallery_append ...): gal4 has room for cap_tiles tiles (every one beyond `tiles` zero), cls for cls_rows labels;
    // generation counts the successful mutations (views and the states built from them carry the number they were made at)
    int64_t cap_tiles = 0, cls_rows = 0;
    uint64_t generation = 0;
    bool borrowed = false;        // a shard of a fir_sharded handle (fir_gallery_set_borrowed_): every mutation is refused
    bool plain_stale = false;     // gallery_plain has to be read again: a mutation ran since (refresh_plain)
    hipStream_t stream = nullptr;
    // chi-square / KL: range[0] = a gallery value outside in_plain_range() was uploaded, range[1] = serial of the last query
    // transposition that met one (fir_common.h); the scans read both and pick their division sequence on the device
    GalleryBuf<int32_t> range;
    int q_serial = 0;
    bool gallery_plain = false;   // host copy of range[0] == 0, read once after the upload (chi-square nomination, topk_lists_dev)
    GalleryBuf<uint64_t> one_keys;  // one-query calls on small galleries (top1_one_query): device key + completion counter, armed once
    int32_t* one_done = nullptr;    // (a word of one_keys) and re-armed by the kernel itself
    uint64_t one_ticket = 0;        // number of such calls so far: the word the host waits for

    // workspaces (grown on demand with FIR_NEED, never inside a *_dev call once large enough) and the scratch slots of
    // fir_gallery_scratch_ (classifier entry points in the other translation units): fir_gallery_memory_bytes' `scratch`
    GalleryBuf<float> qt;         // transposed query tiles
    GalleryBuf<float> dq;         // staged host queries
    GalleryBuf<uint64_t> dkeys;   // keys for the host-pointer API
    GalleryBuf<uint64_t> part;    // top-K per-wave partials
    GalleryBuf<float> dout;       // range distances for the host-pointer API
    GalleryBuf<int32_t> didx;
    GalleryBuf<float> rowsum;     // chi-square nomination (kChi2Harm): per-row sums over [rs_start, rs_end) + their maximum (rowsum[n])
    FirBuf knn;                   // fir_search_knn: one query tile's stored distances + the select's control block (knn_plan)
    // fir_search_top1_other_class and the self-join over it: the excluded classes padded to whole tiles; the two nearest classes of a routed
    // batch (keys, classes); one block of gallery rows back in row-major form, its keys; the statistic's float row + FarStats + the threshold
    GalleryBuf<int32_t> excl;
    GalleryBuf<uint64_t> okeys;
    GalleryBuf<int32_t> ocls;
    GalleryBuf<float> selfq;
    GalleryBuf<uint64_t> selfkeys;
    GalleryBuf<float> fardist;
    // the masked searches: a host call's mask words; fir_gallery_mask_of_classes' sorted class list, and behind it room for the words it returns
    GalleryBuf<uint64_t> dmask;
    GalleryBuf<uint64_t> mclasses;
    // subsets. On a source: the mask -> row list scan's total (one int64) and, behind it, the segment sums (rows_of_mask_launch).
    // On a handle made by fir_gallery_create_subset / _from_rows (is_subset): origin[origin_n] = the source's LOCAL row of each row and
    // the source's row offset at creation; origin_ok ends with the handle's first in-place update (gallery_changed), the buffer stays --
    // queued key maps may still read it
    GalleryBuf<int32_t> mseg;
    GalleryBuf<int32_t> origin;
    int64_t origin_n = 0, origin_offset = 0;
    bool is_subset = false, origin_ok = false;
    // linear projection / PCA (fir_projection.h): the column statistics' partials and folded sums; the scatter's centre, partials and result
    GalleryBuf<double> pjstat, pjcen, pjpart, pjout;
    FirBuf scratch[25];
    size_t scratch_bytes() const {
        size_t sum = qt.cap + dq.cap + dkeys.cap + part.cap + dout.cap + didx.cap + rowsum.cap + knn.cap + excl.cap + okeys.cap + ocls.cap + selfq.cap +
                     selfkeys.cap + fardist.cap + dmask.cap + mclasses.cap + mseg.cap + origin.cap + pjstat.cap + pjcen.cap + pjpart.cap + pjout.cap;
        for (const FirBuf& s : scratch) sum += s.cap;
        return sum;
    }
    // pinned, device-visible host staging of the small host-pointer calls: queries go in, packed keys come out, with
    // no copy engine in between (the kernels read / write it over PCIe) and one stream synchronisation per call
    void* pin = nullptr;
    uint64_t counters[4] = {};  // fir_gallery_next_counter_

    int qpp = 0;              // queries per gallery pass; 0 = automatic (effective_qpp)
    int waves_req = 0;        // 0 = automatic
    int max_waves = 0;        // upper bound over all scan kernels (8 blocks per CU)
    int last_waves = 0;       // waves of the most recent scan launch
    // L2 whole-range batches of at least this many queries go through fir_gemm_* (same keys): -1 = automatic
    // (kAutoMfmaQueries queries against at least kAutoMfmaRows rows), 0 = never, > 0 = the caller's threshold
    int large_batch_min = -1;
    int int8_mode = -1;       // fir_gallery_set_int8_nomination: -1 = automatic, 0 = never, 1 = every eligible call
    // the matrix-core states of the last TWO feature prefixes [0, end) asked for: the reference's harness alternates "BF, 64" and
    // "BF, 256" (ImageTesting.cpp:526-529); one slot would rebuild fragments and scratch on every call
    struct PrefixSlot { fir_gemm* m = nullptr; int end = 0; uint64_t used = 0; } gemm_prefix[2];
    uint64_t prefix_clock = 0;
    int rs_start = -1, rs_end = -1, rs_metric = -1;   // (what g->rowsum holds: row sums for chi-square, row entropies for KL)
    int warm_left = 0;                  // fir_dispatch_info::warmup_calls_left of the most recent call
    int shadow_mode = FIR_SHADOW_ALL;   // which copies of the gallery the automatic dispatch may keep next to the tiled f32 rows (fir_gallery_set_shadow_copies)
    int small_hits = 0, few_hits = 0;   // automatic mode: calls so far that would have profited from a matrix-core state not built yet (see ensure_gemm)
    bool gemm_failed = false; // automatic mode: the matrix-core path could not be set up for this shape (rows too long): scan
    fir_gemm* gemm = nullptr; // created on first use
    fir_dispatch_info last{}; // dominant kernel of the most recent search
    fir_twd_dispatch_info twd_last{0, -1};   // fir_twd_last_dispatch (fir_twd.hip writes it through fir_gallery_twd_record_); classifier -1: no call yet
    int64_t twd_mfma[6] = {};                // fir_twd_last_mfma (fir_twd.hip writes it through fir_gallery_twd_mfma_record_)
    const char* last_subrange_kernel = "";   // fir_gallery_last_subrange_kernel_: subranges_dev's most recent one-pass kernel, "" after the per-range branch
    bool label_known = false;                // fir_gallery_label_range_: smallest and largest label, found once per generation
    int32_t label_lo = 0, label_hi = -1;
    int call_launches = 0;    // scan launches of the current call (note_dispatch)
    int max_tiles_per_launch = 64;   // query tiles (gallery passes) folded into one launch of the hand-scheduled kernels

    struct Occ { const void* fn; size_t lds; int waves; };
    std::vector<Occ> occ;     // resident-wave capacity per scan kernel

    bool profiling = false;
    std::vector<hipEvent_t> ev;   // pairs
    size_t ev_used = 0;
    double last_bytes = 0.0;

    // call order (FirCallOrder, fir_internal.h): the end of the most recent call on this handle or a fir_gemm state over it
    hipEvent_t last_done = nullptr;
    hipStream_t last_stream = nullptr;   // the stream last_done was recorded on (nullptr: no call yet)
    int call_depth = 0;                  // > 0 inside a call

    void drop_gemm_states() {            // the whole-row state and both prefix slots (they cache the offset, the shadow mode, ...)
        if (gemm) { fir_gemm_destroy(gemm); gemm = nullptr; }
        for (auto& ps : gemm_prefix) if (ps.m) { fir_gemm_destroy(ps.m); ps.m = nullptr; ps.end = 0; }
    }
    // The matrix-core states first (they queue on this stream and hang off these buffers), the stream last; then the members.
    ~fir_gallery() {
        drop_gemm_states();
        for (hipEvent_t e : ev) (void)hipEventDestroy(e);
        if (last_done) (void)hipEventDestroy(last_done);
        if (pin) (void)hipHostFree(pin);
        if (stream) (void)hipStreamDestroy(stream);
    }
};

namespace {

// What one scan covers, and on whose behalf: tiles [tile_begin, tile_begin + tiles) of the gallery (tiles == 0: all of it), the
// groups a row sample's tiles form (ScanArgs::groups / group_stride, chi-square / KL top-1 scans only), and quiet: a scan on
// behalf of another path -- the matrix-core path's uncertified queries, a threshold's row samples -- is not recorded in g->last,
// gets no event pair and takes no candidate-list path of its own.
struct ScanScope {
    int64_t tile_begin = 0, tiles = 0;
    int groups = 0;
    int64_t group_stride = 0;
    bool quiet = false;
    // the store scan over a row sample (knn_sample_bound_dev): `tiles` sample tiles in run_count runs of run_len, spread over run_slack more
    // gallery tiles (ScanArgs::run_len, fir_kernels.h), run_rows rows of the gallery among them; tile_begin 0
    int32_t run_len = 0, run_count = 0;
    int64_t run_slack = 0, run_rows = 0;
};
const ScanScope kOnBehalf{0, 0, 0, 0, true};      // the whole gallery, quietly

typedef void (*scan_fn)(const ScanArgs);

// ---- the scan kernels: one table, one selector -------------------------------------------------------------------------------
// Every kernel launched through a scan_fn is a row of kScanTable. FIR_ROW writes the pointer and the name that fir_dispatch_info
// reports from the SAME template arguments, so the record cannot name a kernel that did not run. The arguments are spelled as
// the numbers those names have always carried:
//   metric     0 L2, 1 chi-square, 2 KL, 3 / 4 their plain-range forms, 5-7 the nomination metrics (fir_common.h)
//   U          kU chunks per load group, kUDeep in the few-tiles form, kUSub in k_scan_subranges
//   epilogue   0 top-1, 1 top-K, 2 store, 3 append, 5 class minimum, 6 top-1 over the other classes
//   KMAX       kKMax
//   waves per SIMD   kWps; kWpsPlain for the metrics from 3 on
//   LDSQ, MASKED     1 = the query tile staged in LDS (the few-tiles form); 1 = only the rows of a mask take part (kMasked rows)
enum ScanKind { kGeneric, kDeep, kL2Lds, kL2Scalar, kNominate, kSubranges, kMasked };
constexpr int kEpiSubranges = 4;   // selector only: k_scan_subranges (one stored distance per sub-range)
static_assert(kEpiTop1 == 0 && kEpiTopK == 1 && kEpiStore == 2 && kEpiAppend == 3 && kEpiClassMin == 5 && kEpiTop1Other == 6 && kL2 == 0 && kChi2 == 1 && kKL == 2 && kChi2InRange == 3 &&
                  kKLInRange == 4 && kChi2Approx == 5 && kChi2Harm == 6 && kKLEnt == 7 && kU == 8 && kUDeep == 16 && kUSub == 8 && kKMax == 8 && kWps == 4 && kWpsPlain == 3,
              "kScanTable spells these as numbers");
struct ScanRow { int kind, epi, qb, metric; scan_fn fn; const char* name; };
#define FIR_ROW(KIND, EPI, QB, M, KERNEL, ...) {KIND, EPI, QB, M, (scan_fn)KERNEL<__VA_ARGS__>, "fir::" #KERNEL "<" #__VA_ARGS__ ">"},
#define FIR_SCAN(EPI, QB, M, WPS) FIR_ROW(kGeneric, EPI, QB, M, k_scan, QB, M, 8, EPI, 8, WPS, 0)
#define FIR_SCAN_M(EPI, QB) FIR_SCAN(EPI, QB, 0, 4) FIR_SCAN(EPI, QB, 1, 4) FIR_SCAN(EPI, QB, 2, 4) FIR_SCAN(EPI, QB, 3, 3) FIR_SCAN(EPI, QB, 4, 3)
#define FIR_MASKED(EPI, QB, M, WPS) FIR_ROW(kMasked, EPI, QB, M, k_scan, QB, M, 8, EPI, 8, WPS, 0, 1)
#define FIR_MASKED_M(EPI, QB) FIR_MASKED(EPI, QB, 0, 4) FIR_MASKED(EPI, QB, 1, 4) FIR_MASKED(EPI, QB, 2, 4) FIR_MASKED(EPI, QB, 3, 3) FIR_MASKED(EPI, QB, 4, 3)
#define FIR_DEEP(EPI, M, WPS) FIR_ROW(kDeep, EPI, 1, M, k_scan, 1, M, 16, EPI, 8, WPS, 1)
#define FIR_APPEND(M, WPS) FIR_ROW(kGeneric, 3, 8, M, k_scan, 8, M, 8, 3, 8, WPS)
#define FIR_SUB(QB) FIR_ROW(kSubranges, 4, QB, 0, k_scan_subranges, QB, 0, 8, 4) FIR_ROW(kSubranges, 4, QB, 1, k_scan_subranges, QB, 1, 8, 4) \
                    FIR_ROW(kSubranges, 4, QB, 2, k_scan_subranges, QB, 2, 8, 4)
static const ScanRow kScanTable[] = {
    // the hand-scheduled L2 top-1 kernels (whole-chunk feature ranges): the query tile staged in LDS -- 8 queries, 16 queries (two
    // rows per lane: fir_kernels.h, l2_chunk_lds), the append form of the top-K lists -- or, for a tile beyond LDS (rows longer
    // than ~4600 features), read through the scalar cache
    FIR_ROW(kL2Lds, 0, 8, 0, k_scan_l2_lds, 1, 8, 4, false) FIR_ROW(kL2Lds, 0, 16, 0, k_scan_l2_lds, 2, 4, 3, false, 2)
    FIR_ROW(kL2Lds, 3, 8, 0, k_scan_l2_lds, 1, 8, 4, true) FIR_ROW(kL2Scalar, 0, 8, 0, k_scan_l2_fast, 1, 8, 4)
    // few tiles (a gallery of a few thousand rows): every wave owns a whole tile and streams it alone, so what limits a one-query
    // call is how many gallery loads the wave keeps in flight; a one-query tile has the registers for 16 chunks per load group
    FIR_DEEP(0, 0, 4) FIR_DEEP(0, 1, 4) FIR_DEEP(0, 2, 4) FIR_DEEP(0, 3, 3) FIR_DEEP(0, 4, 3)
    FIR_DEEP(2, 0, 4) FIR_DEEP(2, 1, 4) FIR_DEEP(2, 2, 4) FIR_DEEP(2, 3, 3) FIR_DEEP(2, 4, 3)
    // the generic scan, any feature range (the top-K scan keeps 2 * KMAX registers per query: 4 queries at most)
    FIR_SCAN_M(0, 1) FIR_SCAN_M(0, 2) FIR_SCAN_M(0, 4) FIR_SCAN_M(0, 8)
    FIR_SCAN_M(1, 1) FIR_SCAN_M(1, 2) FIR_SCAN_M(1, 4)
    FIR_SCAN_M(2, 1) FIR_SCAN_M(2, 2) FIR_SCAN_M(2, 4) FIR_SCAN_M(2, 8)
    // topk_lists_dev: the row samples in a nomination metric, the append scan, and its two-tiles-per-read form, the only
    // append scan of metrics 6 and 7
    FIR_ROW(kGeneric, 0, 8, 6, k_scan, 8, 6, 8, 0, 8, 3) FIR_ROW(kGeneric, 0, 8, 7, k_scan, 8, 7, 8, 0, 8, 3)
    FIR_APPEND(0, 4) FIR_APPEND(1, 4) FIR_APPEND(2, 4) FIR_APPEND(3, 3) FIR_APPEND(4, 3) FIR_APPEND(5, 3)
    FIR_ROW(kNominate, 3, 16, 6, k_nominate, 6, 2, 8, 3) FIR_ROW(kNominate, 3, 16, 7, k_nominate, 7, 2, 8, 3)
    FIR_SUB(1) FIR_SUB(2) FIR_SUB(4) FIR_SUB(8)
    // top_classes_dev: the smallest key of every class, tiles of 8 queries
    FIR_SCAN_M(5, 8)
    // other_class_dev: top-1 over the rows of another class, the tile sizes and the few-tiles form of the generic top-1 scan
    FIR_DEEP(6, 0, 4) FIR_DEEP(6, 1, 4) FIR_DEEP(6, 2, 4) FIR_DEEP(6, 3, 3) FIR_DEEP(6, 4, 3)
    FIR_SCAN_M(6, 1) FIR_SCAN_M(6, 2) FIR_SCAN_M(6, 4) FIR_SCAN_M(6, 8)
    // the masked searches (masked_top1_dev, knn_dev, top_classes_dev with a mask): the generic scan's top-1, store and class-minimum
    // forms over the rows of a mask; no few-tiles form -- a one-query masked call on a small gallery takes these
    FIR_MASKED_M(0, 1) FIR_MASKED_M(0, 2) FIR_MASKED_M(0, 4) FIR_MASKED_M(0, 8)
    FIR_MASKED_M(2, 1) FIR_MASKED_M(2, 2) FIR_MASKED_M(2, 4) FIR_MASKED_M(2, 8)
    FIR_MASKED_M(5, 8)
};
#undef FIR_ROW
#undef FIR_SCAN
#undef FIR_SCAN_M
#undef FIR_DEEP
#undef FIR_MASKED
#undef FIR_MASKED_M
#undef FIR_APPEND
#undef FIR_SUB

const ScanRow* scan_row(int kind, int epi, int qb, int metric) {
    for (const ScanRow& r : kScanTable)
        if (r.kind == kind && r.epi == epi && r.qb == qb && r.metric == metric) return &r;
    return nullptr;
}

// What one scan launches: fn, for chi-square / KL its plain-range twin (launched next to it with the same grid -- which of the
// two does the pass is decided on the device from the range flags, the other returns at once), the name of fn for the dispatch
// record, and the dynamic LDS both are launched with. fn == nullptr: no kernel takes this shape.
struct ScanKernel { scan_fn fn = nullptr, fn_plain = nullptr; const char* name = ""; size_t lds_bytes = 0; };
constexpr size_t kMaxQueryTileLds = 144 * 1024;   // of the CU's 160 KiB; one workgroup per CU above 80 KiB (above 64 KiB the launch opts in: run_pass)
// whole_chunks: start and end are multiples of 4 features; few_tiles: no more tiles than SIMDs (one-query tiles then take the
// 16-chunk form when the query fits 64 KiB of LDS). The append epilogue with 16 queries is the two-tiles-per-read nomination scan.
// masked: the kMasked row of the shape and nothing else -- neither the hand-scheduled L2 kernels nor the few-tiles form has one.
ScanKernel select_scan(int epi, int qb, int metric, bool whole_chunks, int dp4, bool few_tiles, bool masked = false) {
    const bool l2_hand = !masked && metric == kL2 && whole_chunks && (epi == kEpiTop1 || epi == kEpiAppend);
    const size_t tile = (size_t)(dp4 + 1) * qb * 16;                       // query tile + one zero chunk of slack
    const size_t tile_max = epi == kEpiAppend ? 64 * 1024 : kMaxQueryTileLds;
    const size_t deep_tile = (size_t)dp4 * 4 * qb * sizeof(float);
    const size_t deep_extra = epi == kEpiTop1Other ? 16 : 0;               // the excluded classes behind the staged tile
    ScanKernel k;
    const ScanRow* r = nullptr;
    if (masked) r = scan_row(kMasked, epi, qb, metric);
    else if (epi == kEpiSubranges) r = scan_row(kSubranges, epi, qb, metric);
    else if (l2_hand && tile <= tile_max && (r = scan_row(kL2Lds, epi, qb, metric))) k.lds_bytes = tile;
    else if (l2_hand && (r = scan_row(kL2Scalar, epi, qb, metric))) k.lds_bytes = 0;
    else if (few_tiles && deep_tile + deep_extra <= 64 * 1024 && (r = scan_row(kDeep, epi, qb, metric))) k.lds_bytes = deep_tile + deep_extra;
    else if (epi == kEpiAppend && qb == 16) r = scan_row(kNominate, epi, qb, metric);
    else r = scan_row(kGeneric, epi, qb, metric);
    if (!r) return k;
    k.fn = r->fn;
    k.name = r->name;
    if (metric == kChi2 || metric == kKL)
        if (const ScanRow* p = scan_row(r->kind, epi, qb, metric + 2)) k.fn_plain = p->fn;
    return k;
}

// Number of waves for `tiles` tiles. All waves are resident at once (waves <= capacity) and each
// gets ceil(tiles / waves) or one fewer tile. Large galleries use a whole number of waves per
// SIMD -- 3 measured best on MI355X for the HBM-bound L2 scan (profiles/r01_sweep_notes.md):
// with a fractional count the SIMDs that hold one wave more finish late.
int pick_waves(int64_t tiles, int max_waves, int simds) {
    if (tiles <= 0) return 4;
    const int per_simd = std::max(1, std::min(3, max_waves / std::max(simds, 1)));
    const int w = per_simd * simds;
    if (tiles <= w) return (int)((tiles + 3) / 4 * 4);
    return w;
}

// Queries per gallery pass. Galleries larger than the 256 MiB Infinity Cache are streamed from HBM and the
// L2 scan stays HBM-bound up to 8 queries per pass (profiles/r01_sweep_notes.md); a gallery (shard) that stays
// cache-resident is VALU-bound either way, and 16 queries per pass halve its cache traffic
// (profiles/r01_qb_table_100kx512.txt: 295k vs 175k queries/s at 100k x 512).
double gallery_bytes(const fir_gallery* g) { return (double)g->tiles * 64.0 * g->dp4 * 16.0; }
int effective_qpp(const fir_gallery* g) {
    if (g->qpp > 0) return g->qpp;
    return gallery_bytes(g) <= 384.0 * 1024 * 1024 ? 16 : 8;
}

// Queries per pass of one top-1 call of qb queries. A wave owns whole 64-row tiles, so a gallery of few tiles gives
// few waves per pass: the automatic choice halves the query tile until the launch (tiles x passes) has a wave for
// every SIMD (profiles/r01_small_gallery_sweep.txt).
int top1_qpp(const fir_gallery* g, const ScanScope& scope, int qb, int cap) {
    if (g->qpp > 0) return cap;
    const int64_t simds = (int64_t)g->cus * 4;
    int q = cap;
    const int64_t tiles = scope.tiles > 0 ? std::min<int64_t>(scope.tiles, g->tiles) : g->tiles;
    while (q > 1 && tiles * ((qb + q - 1) / q) < simds) q /= 2;
    return q;
}

// Automatic matrix-core dispatch (fir_gallery_set_large_batch_mfma): measured on MI355X, 1M x 512: 256 queries 444k/s
// against 26k/s through the exact scan, identical keys (profiles/); below ~64k rows the gallery is cache-resident and the
// scan's 16-queries-per-pass form is within reach of it for small batches: a cost model of the two forms decides there.
constexpr int kAutoMfmaQueries = 128;
constexpr int64_t kAutoMfmaRows = 65536;
// The K nearest distinct classes (fir_gemm_search_top_classes_keys_dev) from kAutoMfmaQueries queries over kAutoMfmaRows rows on:
// 1M x 512, 100 000 classes, K = 5, 128 .. 32 768 queries per call: 4.1-6.5 x the scan form's rate on class-major labels, 3.9-5.2 x
// on permuted ones, every case far beyond the 15 % the cost model above asks for (profiles/class_rank_matrix_cores.txt). Smaller
// galleries were not measured: they stay with the scan unless the caller sets a threshold.
constexpr bool kAutoMfmaClasses = true;
// classes (fir_search_top_classes): the same ranges and the same caller's threshold; the automatic rule is kAutoMfmaClasses
bool wants_mfma(const fir_gallery* g, int32_t qb, int32_t start, int32_t end, bool classes = false) {
    // the whole row, or a prefix of whole 16-feature k-blocks (>= 64 features: below that the scan's prefix pass is cheap)
    if (g->metric != FIR_METRIC_L2 || start != 0 || g->n <= 0) return false;
    if (end != g->d && (end < 64 || end % 16 != 0)) return false;
    if (g->large_batch_min == 0 || g->gemm_failed) return false;
    if (g->large_batch_min > 0) return qb >= g->large_batch_min;
    if (g->qpp != 0) return false;                                              // a pinned queries-per-pass asks for the scan
    if (classes) return kAutoMfmaClasses && qb >= kAutoMfmaQueries && g->n >= kAutoMfmaRows;
    if (g->n < kAutoMfmaRows) {
        // Cache-resident galleries: the scan folds its 16-query passes into one launch, ~40 us + (2 us + 0.25 us per MB) per pass;
        // the matrix-core call ~125 us (225 us with rows longer than 512 features: streamed query slabs) + 0.06 (0.12) us per MB and
        // 128 queries. Measured (us, scan / matrix cores): 40 000 x 512: 128 queries 329 / 140, 1 024: 1 568 / 178; 16 384 x 512:
        // 128: 121 / 135, 256: 234 / 138, 1 024: 788 / 155; 8 192 x 512: 256: 105 / 133, 1 024: 303 / 145; 30 000 x 1536: 128:
        // 589 / 387, 1 024: 4 036 / 496; 3 030 x 1536 (the reference's gallery): 256: 136 / 270, 1 024: 377 / 346. The matrix cores
        // are taken where the model gives them 15 % or more.
        if (g->n < 2048 || qb < 64) return false;
        // (the constants were measured on a 256-CU MI355X; the per-MB terms -- bandwidth and matrix-core time -- scale with the CU count
        // of the device the gallery lives on, the fixed terms -- launches, synchronisation -- do not)
        const double mbs = (double)g->n * (double)end * 4.0 / 1.0e6 * (256.0 / std::max(g->cus, 1));
        const bool streamed = end > 512;
        // (round 4: every super-batch finds its threshold on the way and small calls stay on one stream -- the matrix-core call's fixed part
        // fell from ~125 / 225 us to ~100 / 170 us: 8 192 x 512, 128 / 256 / 1 024 queries 103 / 100 / 115 us, 65 536 x 512 98 / 99 / 162,
        // 8 192 x 1280 148 / 200 / 231, 65 536 x 1280 172 / 234 / 446: profiles/r04_adaptive_cutoff.txt)
        const double mfma_us = (streamed ? 170.0 : 100.0) + (double)((qb + 127) / 128) * (streamed ? 0.12 : 0.06) * mbs;
        const double scan_us = 40.0 + (double)((qb + 15) / 16) * (2.0 + 0.25 * mbs);
        return mfma_us * 1.15 < scan_us;
    }
    // Smaller batches on larger galleries: a matrix-core call costs ~125 us + 0.1 us per MB of compared rows whatever the batch
    // (up to 128 queries), the scan 0.15 us per MB for every 8 queries. Measured at d = 512 (one MI355X, device pointers):
    // 1M rows 8 / 16 / 64 queries: scan 397 / 750 / 2583 us, matrix cores 347 / 336 / 343; 100 000 rows 16 / 32 / 64: 108 / 283 /
    // 445 against 146 / 148 / 159; 65 536 rows 32 / 64: 134 / 429 against 133 / 148; 1M rows 2 / 4 / 7 queries: 349 / 353 / 1016 against ~345.
    const double mb = (double)g->n * (double)end * 4.0 / 1.0e6 * (256.0 / std::max(g->cus, 1));     // (scaled as above)
    if (qb >= kAutoMfmaQueries || (qb >= 32 && mb >= 128.0)) return true;
    if (qb < 2 || mb < 300.0) return false;
    // 2..31 queries over rows streamed from HBM: the scan takes one pass per power-of-two group of up to 8 queries (3 queries: 2 + 1,
    // 7: 4 + 2 + 1), ~15 us + 0.16 us per MB each (1M x 512, 2 048 MB: 340 us for 1, 2, 4 or 8 queries, three times that for 7); the
    // matrix-core call, since round 4 (live query blocks only, one stream, the first row block summed once: profiles/r04_small_calls.txt),
    // ~75 us + 0.095 us per MB for anything up to 32 queries (1M x 512: 265 us; 1M x 1280: 575 us), ~125 us + 0.105 us per MB up to 128
    const int passes = qb / 8 + __builtin_popcount((unsigned)qb & 7u);
    return (qb <= 32 ? 75.0 + 0.095 * mb : 125.0 + 0.105 * mb) < passes * (15.0 + 0.16 * mb);
}

// ONE query against rows far beyond the caches (automatic mode only): the nomination scan over the fp16 copy
// (fir_gemm_search_few_keys_dev) reads half the bytes of the exact scan's pass and costs ~65 us more around it: 1M x 512 (2 GB)
// 332 -> 253 us, 1M x 1280 790 -> 550 us, 300 000 x 512 116 -> 173 us (not taken). With 2 queries the two forms tie, from 3 on
// the dot products (v_dot2 + one LDS read per query and fragment) cost more than the bytes saved: those stay with the f32 scan.
bool wants_few(const fir_gallery* g, int32_t qb, int32_t start, int32_t end) {
    if (g->metric != FIR_METRIC_L2 || start != 0 || g->n < kAutoMfmaRows || g->qpp != 0 || g->few_hits < 0) return false;
    if (end != g->d && (end < 64 || end % 16 != 0)) return false;
    if (g->large_batch_min >= 0 || g->gemm_failed) return false;
    return qb == 1 && (double)g->n * (double)end * 4.0 >= 1500.0e6;
}

void note_dispatch(fir_gallery* g, const void* fn, const char* name, int launches_add, int gx, int gy, int block, size_t dyn_lds, int qpp,
                   double bytes, double flops, int path) {
    fir_dispatch_info& L = g->last;
    if (launches_add == 0 || std::strncmp(L.kernel, name, sizeof(L.kernel)) != 0) {
        std::memset(&L, 0, sizeof L);
        std::snprintf(L.kernel, sizeof(L.kernel), "%s", name);
        hipFuncAttributes at;
        if (fn && hipFuncGetAttributes(&at, fn) == hipSuccess) {
            L.vgprs = at.numRegs;
            L.lds_bytes = (int32_t)(at.sharedSizeBytes + dyn_lds);
        } else {
            L.lds_bytes = (int32_t)dyn_lds;
        }
    }
    L.struct_bytes = (int32_t)sizeof L;
    L.path = path;
    L.launches += 1;
    L.grid_x = gx; L.grid_y = gy; L.block = block;
    L.queries_per_pass = qpp;
    L.bytes_per_launch = bytes;
    L.flops_per_launch = flops;
}

// g->gallery_plain after a mutation: the update kernels have set range[0] where a written value asked for it (it is never cleared: an
// out-of-range value that was overwritten or removed since keeps the full division sequence, the same bits). `st` is the stream of
// the call that asks, which the call order has made wait for the mutation; it is synchronised once.
int refresh_plain(fir_gallery* g, hipStream_t st) {
    if (!g->plain_stale) return FIR_OK;
    int32_t r0 = 1;
    FIR_HIP(hipMemcpyAsync(&r0, g->range, sizeof r0, hipMemcpyDeviceToHost, st));
    FIR_HIP(hipStreamSynchronize(st));
    g->gallery_plain = r0 == 0;
    g->plain_stale = false;
    return FIR_OK;
}

int check_range(const fir_gallery* g, int32_t& start, int32_t& end) {
    if (end == 0) end = g->d;   // db_features.cpp:320-321
    if (start < 0 || end > g->d || start >= end)
        return fir_fail_(FIR_ERR_ARG, "feature range [%d,%d) not inside [0,%d)", start, end, g->d);
    return FIR_OK;
}

// Serial number of a query transposition (fir_gallery::range): wraps without overflow; a collision after 2^32 calls only
// sends one chi-square / KL call through the full division sequence.
int next_serial(fir_gallery* g) {
    g->q_serial = (int)((unsigned)g->q_serial + 1u);
    return g->q_serial;
}

// Resident-wave capacity of one scan kernel on this device (cached per kernel / LDS size).
int max_waves_for(fir_gallery* g, scan_fn fn, size_t lds_bytes) {
    for (const auto& e : g->occ)
        if (e.fn == (const void*)fn && e.lds == lds_bytes) return e.waves;
    int nb = 0;
    hipError_t e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, (const void*)fn, kBlock, lds_bytes);
    if (e != hipSuccess || nb <= 0) nb = 2;
    nb = std::min(nb, 8);
    const int waves = g->cus * nb * (kBlock / 64);
    g->occ.push_back({(const void*)fn, lds_bytes, waves});
    return waves;
}

// The ScanArgs fields every scan shares: the tiled gallery -- the scope's window of it --, the scope's sample groups, the feature
// range and the grid's wave count. Every gallery is read with the non-temporal hint: plain loads gained nothing even for an 18 MB
// gallery that fits the L2s (one-query calls unchanged, multi-pass calls slower -- profiles/r01_small_gallery_sweep.txt).
ScanArgs scan_args(const fir_gallery* g, const ScanScope& scope, int32_t start, int32_t end, int waves) {
    ScanArgs a{};
    const int64_t tile0 = scope.tiles > 0 ? std::min<int64_t>(scope.tile_begin, g->tiles) : 0;
    const int64_t tiles = scope.tiles > 0 ? std::min<int64_t>(scope.tiles, g->tiles - tile0) : g->tiles;
    a.groups = scope.groups;
    a.group_stride = scope.group_stride;
    a.gal4 = g->gal4 + (size_t)tile0 * g->dp4 * 64;
    a.row_offset = g->row_offset + tile0 * kTileRows;
    a.n = std::min<int64_t>(g->n - tile0 * kTileRows, tiles * kTileRows);
    a.tiles = (int32_t)tiles;
    a.dp4 = g->dp4;
    a.start = start;
    a.end = end;
    a.waves = waves;
    a.nt = 1;
    a.cls = g->cls ? g->cls + tile0 * kTileRows : nullptr;
    if (scope.run_len > 0) {
        a.n = scope.run_rows;
        a.run_len = scope.run_len;
        a.run_count = scope.run_count;
        a.run_slack = scope.run_slack;
    }
    return a;
}

bool whole_chunks(int32_t start, int32_t end) { return ((start | end) & 3) == 0; }
bool few_tiles(const fir_gallery* g) { return g->tiles <= (int64_t)g->cus * 4; }

// What the class-minimum epilogue needs beyond a pass's other arguments (`keys` is then the table cmin[query][class]).
// nq: live queries of the launch, the last tile may be part full; tiles_ready: the pass before this one left the same tiles in g->qt
struct ClassPass { const float* tau; int32_t num_classes; int32_t nq; bool tiles_ready; };

// Queue: transpose (+ key init) of one query tile, then one gallery pass.
int run_pass(fir_gallery* g, hipStream_t st, const ScanScope& scope, int epi, const float* d_queries, int q0, int qb_tile, int32_t start,
             int32_t end, uint64_t* keys, float* out, int64_t out_stride, int k, int* waves_used = nullptr, int ny = 1,
             int init_keys = 0, const ClassPass* cp = nullptr, int live = 0, const int32_t* excl = nullptr, const uint64_t* mask = nullptr) {
    // mask != NULL (top-1, store and class-minimum epilogues): the masked form of the scan over the rows whose bit is set (word 0 = local tile 0)
    // ny > 1 (top-1 kernels, the class-minimum scan and the store scan only): ny consecutive query tiles of qb_tile queries in ONE launch;
    // live > 0 (the store scan): the launch's live queries, the last tile may be part full -- query y * qb_tile + q goes to out + that * out_stride
    const int kk = g->dp4 * 4;
    float* qt = g->qt + (size_t)q0 * kk;
    if (!(cp && cp->tiles_ready)) {
        const int64_t total = std::max<int64_t>((int64_t)kk * qb_tile * ny, init_keys);
        const int blocks = (int)((total + kBlock - 1) / kBlock);
        hipLaunchKernelGGL(k_transpose_queries, dim3(blocks), dim3(kBlock), 0, st, d_queries + (size_t)q0 * g->d, cp ? cp->nq : live > 0 ? live : qb_tile * ny,
                           g->d, g->dp4, qb_tile, qt, init_keys > 0 ? keys : nullptr, init_keys, g->range, next_serial(g));
    }
    const ScanKernel sk = select_scan(epi, qb_tile, g->metric, whole_chunks(start, end), g->dp4, few_tiles(g), mask != nullptr);
    if (!sk.fn) return fir_fail_(FIR_ERR_ARG, "no kernel for qb=%d metric=%d", qb_tile, g->metric);
    if (sk.lds_bytes > 64 * 1024) {   // more than the default dynamic LDS limit: opt in once per kernel
        bool known = false;
        for (const auto& e : g->occ) known = known || (e.fn == (const void*)sk.fn && e.lds == sk.lds_bytes);
        if (!known) FIR_HIP(hipFuncSetAttribute((const void*)sk.fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kMaxQueryTileLds));
    }
    int max_waves = max_waves_for(g, sk.fn, sk.lds_bytes);
    if (sk.fn_plain) max_waves = std::min(max_waves, max_waves_for(g, sk.fn_plain, sk.lds_bytes));
    int waves = g->waves_req > 0 ? std::min(g->waves_req, max_waves) : pick_waves(scope.run_len > 0 ? scope.tiles : g->tiles, max_waves, g->cus * 4);
    const int groups = epi == kEpiTop1 && scope.groups > 1 && g->metric != kL2 ? scope.groups : 0;
    if (groups) waves = std::max(4 * groups, waves / (4 * groups) * (4 * groups));      // a wave's tiles all belong to one group
    g->last_waves = waves;
    if (waves_used) *waves_used = waves;
    ScanArgs a = scan_args(g, scope, start, end, waves);
    a.groups = groups;
    a.qt = qt;
    a.keys = keys;
    a.out = out;
    a.out_stride = out_stride;
    a.nq = live > 0 ? live : qb_tile;
    a.k = k;
    a.qt_stride = (int64_t)kk * qb_tile;
    a.range = g->range;
    a.serial = g->q_serial;
    a.excl = excl;                  // kEpiTop1Other: the tile-padded excluded classes of this launch's first query
    a.mask = mask ? mask + (scope.tiles > 0 ? std::min<int64_t>(scope.tile_begin, g->tiles) : 0) : nullptr;      // the scope's window of the words, as scan_args takes the tiles'
    if (cp) {
        a.tau = cp->tau;
        a.num_classes = cp->num_classes;
        a.nq = cp->nq;
    }
    // algorithmic bytes of one launch: per pass the gallery range once (the class-minimum scan: and a label per row), the query tile, the keys
    // (a masked pass: the unmasked figure plus the mask words -- how many tiles a device mask lets the scan skip is not known here)
    const double bytes_alg = ny * ((double)a.n * ((end - start) * 4.0 + (cp || excl ? 4.0 : 0.0)) + (double)qb_tile * (end - start) * 4.0 + qb_tile * 8.0 + (mask ? a.tiles * 8.0 : 0.0));
    int rc;
    if (!scope.quiet && (rc = fir_gallery_profile_begin_(g, st))) return rc;
    hipLaunchKernelGGL(sk.fn, dim3(waves / 4, ny), dim3(kBlock), sk.lds_bytes, st, a);
    if (sk.fn_plain) hipLaunchKernelGGL(sk.fn_plain, dim3(waves / 4, ny), dim3(kBlock), sk.lds_bytes, st, a);
    if (!scope.quiet && (rc = fir_gallery_profile_end_(g, st, bytes_alg))) return rc;
    if (!scope.quiet) note_dispatch(g, (const void*)sk.fn, sk.name, g->call_launches++, waves / 4, ny, kBlock, sk.lds_bytes, qb_tile, bytes_alg, 0.0, 0);
    FIR_HIP(hipGetLastError());
    return FIR_OK;
}

int topk_lists_dev(fir_gallery* g, const float* d_queries, int32_t qb, int32_t start, int32_t end, int32_t k, uint64_t* d_keys,
                   hipStream_t st);

int top1_dev(fir_gallery* g, const float* d_queries, int32_t qb, int32_t start, int32_t end, uint64_t* d_keys,
             hipStream_t st, const ScanScope& scope = {}) {
    // chi-square batches over a large plain-range gallery: nomination scan + exact re-rank (topk_lists_dev with K = 1), the same
    // keys at about twice the rate; it synchronises `st` once (it has to know that no list overflowed) and leaves the call to the
    // exact scan below when it cannot answer (operands outside the plain range, list overflow)
    if (g->metric == kChi2 || g->metric == kKL)
        if (const int rcp = refresh_plain(g, st)) return rcp;
    if ((g->metric == kChi2 || g->metric == kKL) && g->gallery_plain && scope.tiles == 0 && !scope.quiet && qb >= 8 && g->n >= 65536 &&
        g->qpp == 0) {
        int rc0 = FIR_OK;
        for (int q0 = 0; q0 < qb && rc0 == FIR_OK; q0 += 1024)       // candidate lists are 32 KiB per query: bounded scratch for any qb
            rc0 = topk_lists_dev(g, d_queries + (size_t)q0 * g->d, std::min(1024, qb - q0), start, end, 1, d_keys + q0, st);
        if (rc0 != FIR_ERR_STATE) return rc0;
    }
    int rc = FIR_NEED(g->qt, (size_t)qb * g->dp4 * 4 + 64);   // +64: the fast kernel prefetches one unit past the tile
    if (rc) return rc;
    // 16 queries per pass exist only in the hand-scheduled kernel (whole-chunk L2 ranges)
    int cap = g->metric == kL2 && whole_chunks(start, end) ? effective_qpp(g) : std::min(effective_qpp(g), 8);
    // 16 queries per pass only while their tile fits the default 64 KiB of LDS (d <= 1020): a larger tile leaves one
    // workgroup per CU, and the 8-query tile then does better
    if (cap > 8 && (size_t)(g->dp4 + 1) * 16 * 16 > 64 * 1024) cap = 8;
    cap = top1_qpp(g, scope, qb, cap);
    int q0 = 0;
    while (q0 < qb) {
        const int t = largest_pow2_le(qb - q0, cap);
        // all the whole tiles of t queries go into one launch (blockIdx.y)
        const int ny = std::min((qb - q0) / t, g->max_tiles_per_launch);
        rc = run_pass(g, st, scope, kEpiTop1, d_queries, q0, t, start, end, d_keys + q0, nullptr, 0, 0, nullptr, ny, /*init_keys=*/t * ny);
        if (rc) return rc;
        q0 += t * ny;
    }
    return FIR_OK;
}

int try_mfma_search(fir_gallery* g, const float* d_queries, int32_t qb, int32_t start, int32_t end, const FirSearch& s, hipStream_t st);

int topk_dev(fir_gallery* g, const float* d_queries, int32_t qb, int32_t start, int32_t end, int32_t k, uint64_t* d_keys,
             hipStream_t st, bool allow_lists = true, bool allow_mfma = true) {
    // large whole-range L2 batches over a large gallery: the matrix-core nomination pass + exact re-rank (fir_gemm.hip), the
    // same keys; what it cannot certify comes back through this function with allow_mfma = false
    if (allow_mfma) {
        const int rcm = try_mfma_search(g, d_queries, qb, start, end, FirSearch::rows(k, d_keys), st);
        if (rcm <= 0) return rcm;
    }
    // batches over a large gallery: threshold from a row sample, append scan at the speed of the top-1 scan, K smallest
    // of each candidate list (exact distances throughout); anything it cannot certify falls back to the scan below
    if (allow_lists && qb >= 8 && g->n >= 65536) {
        constexpr int kListBatch = 1024;           // candidate lists are 32 KiB per query: bounded scratch for any qb
        if (qb > kListBatch) {
            for (int q0 = 0; q0 < qb; q0 += kListBatch) {
                const int rc3 = topk_dev(g, d_queries + (size_t)q0 * g->d, std::min(kListBatch, qb - q0), start, end, k, d_keys + (size_t)q0 * k, st, true, false);
                if (rc3) return rc3;
            }
            return FIR_OK;
        }
        const int rc2 = topk_lists_dev(g, d_queries, qb, start, end, k, d_keys, st);
        if (rc2 != FIR_ERR_STATE) return rc2;      // FIR_ERR_STATE: not certified -> the register-list scan answers
    }
    int rc = FIR_NEED(g->qt, (size_t)qb * g->dp4 * 4);
    if (rc) return rc;
    const int qcap = std::min(effective_qpp(g), 4);   // 2*kKMax registers per query per lane
    rc = FIR_NEED(g->part, (size_t)g->max_waves * qcap * k);
    if (rc) return rc;
    int q0 = 0;
    while (q0 < qb) {
        const int t = largest_pow2_le(qb - q0, qcap);
        int waves = 0;
        rc = run_pass(g, st, {}, kEpiTopK, d_queries, q0, t, start, end, g->part, nullptr, 0, k, &waves);
        if (rc) return rc;
        hipLaunchKernelGGL(k_topk_merge, dim3(t), dim3(kBlock), 0, st, g->part, waves, t, q0, t, k, d_keys);
        q0 += t;
    }
    FIR_HIP(hipGetLastError());
    return FIR_OK;
}

// ---- the K nearest rows of a batch through candidate lists (see k_scan_l2_lds<..., APPEND>) ---------------------------------------
// A threshold per query from a row sample, an append scan at the speed of the top-1 scan, the K smallest of each list.
constexpr int kListCap = 4096;
constexpr float kUlp = 5.9604645e-8f;   // u = 2^-24

// chi-square over a plain-range gallery: the append scan runs a NOMINATION metric against a threshold widened by its error bound,
// and the few hundred appended rows per query are re-ranked with the reference's arithmetic before the K smallest are taken: the
// same keys as the exact scan, about twice as fast. Every row whose reference distance is <= the unwidened threshold is appended,
// and the K-th smallest reference distance is <= that threshold (K sample rows are), so the K best are all in the list.
// Two nomination metrics. kChi2Approx: (l - r)^2 * rcp(l + r), within (2 nf + 8) 2^-24 RELATIVE of the reference's value (all
// terms >= 0), 5.5-6.6 issue slots per element instead of 11: the threshold is scaled by 1 + 1.5 (2 nf + 16) u (approx_tau_scale).
// kChi2Harm (default): chi2 = sum(l) + sum(r) - 4 sum_k 1/(1/l_k + 1/r_k), two terms per reciprocal, 1/A + 1/B = (A + B) / (A B)
// with A = 1/l_k + 1/r_k: 2.25 issue slots per element, 1/r computed once per gallery value and pass. Its error is relative to
// sum(l) + sum(r), not to chi2, u = 2^-24: 1/l (IEEE division) u, 1/r (v_rcp_f32, 1 ulp) 2 u, so A and B within 3 u, A + B 4 u, A B 7 u,
// its reciprocal 9 u, the pair of terms (4 + 9 + 1) u = 14 u of its value; harmonic terms <= (l + r)/4, so 4 * their sum <= sum(l) +
// sum(r): 14 u (sum(l) + sum(r)); the fma chain of nf / 2 non-negative terms adds nf u / 2, the two plain sums nf u each, the
// reference's own chain (nf + 3) u of chi2 <= sum(l) + sum(r):
//   |harmonic form - reference| <= B = (3 nf + 19) 2^-24 (sum(l) + max_rows sum(r)) / nf.
// scale * B's coefficient of sum(l) + max_rows sum(r); k_query_sums_widen widens the threshold by 1.5 times what it is given.
float harm_bound_coef(float nf, float scale) { return scale * (3.0f * nf + 19.0f) * kUlp / nf; }
float approx_tau_scale(float nf) { return 1.0f + 1.5f * (2.0f * nf + 16.0f) * kUlp; }

// KL over a plain-range gallery, the entropy form: KL = ln2 (Lq + Lg - E), Lq = sum(l log2 l + l), Lg the same over the row (both
// added up in double once per query / per row), E = sum_k s_k log2 s_k with s_k = l_k + r_k the only sum the scan runs: a packed
// add, a v_log_f32 and a packed fma per (value, query) = 3 issue slots instead of the ~35 of two quotients and two logarithms.
// Error against the reference's float value, u = 2^-24, S = sum(l) + sum(r), |log2 s_k| <= 26 in the plain range:
//   rounding of s_k: (26 + log2 e) u s_k;  v_log_f32, 1 ulp of a value below 32: 32 u s_k;  the fmas of a 4 U-term group and
//   the tail / edge terms: <= 64 * 26.1 u S;  the nf / (4 U) group sums: (nf / 32) 26.1 u S;  Lq, Lg to float and the two
//   combining operations: <= 85 u S;  the reference's own chain (two products and two adds per feature, |terms| <= S): (2 nf + 8) u S
//   |entropy form - reference| <= B = [ln2 (26.1 (64 + nf / 32) + 150) + 2 nf + 8] 2^-24 (sum(l) + max_rows sum(r)) / nf
// (U = 8 chunks per load group, as the kernels are instantiated). k_query_entropy_widen widens by 1.5 times what it is given.
// The 2^-100 the query tile adds to l changes s_k only where l_k = r_k = 0 (anything else is >= 2^-26 and absorbs it): the term is then
// -100 * 2^-100 where the reference skips the pair, at most ln2 * 100 * 2^-100 < 2^-93 of the value whatever nf. Where sum(l) + max_rows
// sum(r) > 0 that vanishes in B's slack (B >= 2^-50 then); where it is 0 -- the query and every row 0 over the whole range -- B is 0
// and the value ln2 * 100 * 2^-100, not the reference's 0: the bound is B + 2^-93, and k_query_entropy_widen adds 2^-92 to what it multiplies
// by 1.5 (>= 2.5 * 2^-93, the widening owed over a sample in the nomination metric).
float entropy_bound_coef(float nf, float scale) { return scale * (0.6932f * (26.1f * (64.0f + nf / 32.0f) + 150.0f) + 2.0f * nf + 8.0f) * kUlp / nf; }

// One call of topk_lists_dev: its arguments, the form it takes (list_form) and its workspace (list_workspace).
struct ListCall {
    fir_gallery* g; const float* d_queries; int32_t qb, start, end, k; hipStream_t st;
    bool nominate, harm, klent;   // chi-square nomination (kChi2Approx, or kChi2Harm when harm is set too); KL nomination (kKLEnt)
    bool approx_samples;          // the row samples run the nomination metric too
    int nh, qpad;                 // tiles of eight queries per gallery read of the append scan; qb padded to whole reads
    int sample_stride;            // keys of sample group i: skeys[i * sample_stride + q]
    bool tiles_ready;             // the query tiles are already in g->qt, in the nomination form (list_row_samples)
    int64_t group_tiles;          // tiles per sample group (list_row_samples)
    uint64_t *skeys, *lists; float *tau, *sq; int32_t *counts, *flag;
    float nf() const { return (float)(end - start); }
    float bound_coef(float scale) const { return harm ? harm_bound_coef(nf(), scale) : entropy_bound_coef(nf(), scale); }
    int nomination_metric() const { return klent ? (int)kKLEnt : harm ? (int)kChi2Harm : nominate ? (int)kChi2Approx : g->metric; }
    int transpose_form() const { return harm ? 1 : klent ? 2 : 0; }    // k_transpose_queries: 1 = 1/l, 2 = l + 2^-100
};

void list_form(ListCall& c) {
    const fir_gallery* g = c.g;
    const bool no_nominate = fir_knob_("FIR_NO_CHI2_NOMINATION") != nullptr;                   // experiments / tests
    const bool allowed = g->gallery_plain && !no_nominate && (size_t)g->d * sizeof(float) <= 48 * 1024;   // (k_list_rerank stages the query in LDS)
    const char* form_env = fir_knob_("FIR_CHI2_NOMINATION");                                   // experiments / tests: 1 = kChi2Approx
    c.nominate = g->metric == kChi2 && allowed;
    c.harm = c.nominate && (form_env ? std::atoi(form_env) : 2) == 2;
    c.klent = g->metric == kKL && allowed;
    // the two cheap nomination forms take two tiles of 8 queries per gallery read (k_nominate): whole pairs of tiles
    c.nh = c.harm || c.klent ? 2 : 1;
    c.qpad = (c.qb + 8 * c.nh - 1) / (8 * c.nh) * (8 * c.nh);
    // chi-square / KL nomination: the row samples run the NOMINATION metric too (2.25 / 3 issue slots per element instead of the
    // exact metric's 11 / ~35: the samples were 0.9 of a 256-query call's 12.3 ms). A sampled minimum is then within B of the
    // reference's value of that row, so at least K rows have a reference distance <= max_i(sample_i) + B, and the append scan
    // (the same metric) has to take everything <= max_i(sample_i) + 2 B: the thresholds are widened by 2.5 B instead of 1.5 B.
    c.approx_samples = (c.harm || c.klent) && !fir_knob_("FIR_EXACT_SAMPLES");
    c.sample_stride = c.approx_samples ? c.qpad : c.qb;
    c.tiles_ready = false;
}

int list_workspace(ListCall& c) {
    fir_gallery* g = c.g;
    void *p_skeys = nullptr, *p_small = nullptr, *p_lists = nullptr, *p_sq = nullptr;
    int rc;
    if ((rc = fir_gallery_scratch_(g, 12, (size_t)c.qpad * c.k * 8, &p_skeys))) return rc;
    if ((rc = fir_gallery_scratch_(g, 13, (size_t)c.qpad * 8 + 16, &p_small))) return rc;
    if ((rc = fir_gallery_scratch_(g, 14, (size_t)c.qpad * kListCap * 8, &p_lists))) return rc;
    c.skeys = (uint64_t*)p_skeys;
    c.tau = (float*)p_small;
    c.counts = (int32_t*)(c.tau + c.qpad);
    c.flag = c.counts + c.qpad;
    c.lists = (uint64_t*)p_lists;
    if ((rc = FIR_NEED(g->qt, (size_t)c.qpad * g->dp4 * 4 + 64))) return rc;      // before anything is queued on it
    if ((c.harm || c.klent) && (rc = fir_gallery_scratch_(g, 15, (size_t)c.qpad * sizeof(float), &p_sq))) return rc;
    c.sq = (float*)p_sq;
    return FIR_OK;
}

// kChi2Harm / kKLEnt: the per-row sums (entropies) over [start, end) and their maximum, kept until the range or the metric changes.
int list_row_sums(ListCall& c) {
    fir_gallery* g = c.g;
    if (!(c.harm || c.klent) || (g->rs_start == c.start && g->rs_end == c.end && g->rs_metric == g->metric && g->rowsum)) return FIR_OK;
    int rc;
    if ((rc = FIR_NEED(g->rowsum, (size_t)g->n + 4))) return rc;
    FIR_HIP(hipMemsetAsync(g->rowsum + g->n, 0, 4 * sizeof(float), c.st));
    hipLaunchKernelGGL(c.klent ? k_row_entropy : k_row_sums, dim3((unsigned)((g->n + kBlock - 1) / kBlock)), dim3(kBlock), 0, c.st, g->gal4, g->n, g->dp4,
                       c.start, c.end, g->rowsum, (unsigned int*)(g->rowsum + g->n));
    g->rs_start = c.start;
    g->rs_end = c.end;
    g->rs_metric = g->metric;
    return FIR_OK;
}

// The per-query sums (entropies) of the nomination metrics, and tau widened by 1.5 * coef * (sum(l) + max_rows sum(r)).
void list_widen(const ListCall& c, float coef) {
    hipLaunchKernelGGL(c.harm ? k_query_sums_widen : k_query_entropy_widen, dim3(c.qpad), dim3(64), 0, c.st, c.d_queries, c.qb, c.g->d, c.start, c.end, c.sq,
                       c.tau, (const unsigned int*)(c.g->rowsum + c.g->n), coef);
}

// The nearest row inside each of k disjoint groups of sample tiles (k top-1 scans, each over all the queries): the largest of the
// k distances is a threshold at least k rows pass; about 2.3 * n * k / rows_sampled rows will.
int list_row_samples(ListCall& c) {
    fir_gallery* g = c.g;
    const int32_t k = c.k, qb = c.qb;
    const hipStream_t st = c.st;
    const int64_t want_rows = std::max<int64_t>(16384, (int64_t)g->n * k / 256);
    const int64_t group_tiles = std::max<int64_t>(1, std::min<int64_t>(g->tiles / k, (want_rows / k + kTileRows - 1) / kTileRows));
    c.group_tiles = group_tiles;
    // (the row samples are not what a profile of this call is about: the events and the dispatch record belong to the append scan)
    ScanScope sample = kOnBehalf;
    FIR_HIP(hipMemsetAsync(c.flag, 0, 4, st));
    int rc = FIR_OK;
    if (c.approx_samples) {
        const int kk = g->dp4 * 4;
        // the per-query sums first (thresholds at -inf: nothing to widen yet)
        FIR_HIP(hipMemsetD32Async((hipDeviceptr_t)c.tau, (int)0xFF800000u, (size_t)c.qpad, st));
        list_widen(c, c.bound_coef(1.0f));
        // every query tile of the call, once, in the form both scans read
        hipLaunchKernelGGL(k_transpose_queries, dim3((unsigned)(((int64_t)kk * c.qpad + kBlock - 1) / kBlock)), dim3(kBlock), 0, st, c.d_queries, qb, g->d,
                           g->dp4, 8, g->qt, (uint64_t*)nullptr, 0, g->range, next_serial(g), c.transpose_form());
        c.tiles_ready = true;
        FIR_HIP(hipMemsetAsync(c.skeys, 0xFF, (size_t)c.qpad * k * 8, st));
        const ScanKernel sk = select_scan(kEpiTop1, 8, c.nomination_metric(), whole_chunks(c.start, c.end), g->dp4, false);
        sample.tiles = std::min<int64_t>(group_tiles * k, g->tiles);
        sample.groups = k > 1 ? k : 0;
        sample.group_stride = c.sample_stride;
        int waves = pick_waves(sample.tiles, max_waves_for(g, sk.fn, 0), g->cus * 4);
        if (k > 1) waves = std::max(4 * k, waves / (4 * k) * (4 * k));                  // a wave's tiles all belong to one group
        ScanArgs a = scan_args(g, sample, c.start, c.end, waves);
        a.nq = 8;
        a.qt_stride = (int64_t)kk * 8;
        a.nt = 0;                                     // the sample is a small part of the gallery: plain loads
        a.range = g->range;
        a.serial = g->q_serial;
        a.flag = c.flag;
        a.sg = g->rowsum;
        for (int y0 = 0; y0 < c.qpad / 8; y0 += g->max_tiles_per_launch) {
            const int ny = std::min(g->max_tiles_per_launch, c.qpad / 8 - y0);
            a.qt = g->qt + (size_t)y0 * 8 * kk;
            a.keys = c.skeys + (size_t)y0 * 8;
            a.sq = c.sq + (size_t)y0 * 8;
            hipLaunchKernelGGL(sk.fn, dim3(waves / 4, ny), dim3(kBlock), 0, st, a);
        }
    } else if (k > 1 && g->metric != kL2) {
        // chi-square / KL: the K samples in ONE launch -- sample tile t belongs to group t mod K, a wave reports into its group's keys
        // (K launches of group_tiles tiles each leave most of the chip idle: a tile is one wave's serial work)
        FIR_HIP(hipMemsetAsync(c.skeys, 0xFF, (size_t)qb * k * 8, st));
        sample.tiles = group_tiles * k;
        sample.groups = k;
        sample.group_stride = qb;
        rc = top1_dev(g, c.d_queries, qb, c.start, c.end, c.skeys, st, sample);
    } else {
        sample.tiles = group_tiles;
        for (int i = 0; i < k && !rc; ++i) {
            sample.tile_begin = i * group_tiles;
            rc = top1_dev(g, c.d_queries, qb, c.start, c.end, c.skeys + (size_t)i * qb, st, sample);
        }
    }
    return rc;
}

// tau[q] = the largest of query q's k sampled minima, widened by the nomination metric's error bound.
void list_threshold(const ListCall& c) {
    const float tau_scale = c.nominate && !c.harm ? approx_tau_scale(c.nf()) : 1.0f;
    hipLaunchKernelGGL(k_topk_tau, dim3((c.qpad + 63) / 64), dim3(64), 0, c.st, c.skeys, c.qb, c.qpad, c.k, c.tau, c.counts, c.flag, tau_scale, c.sample_stride);
    // (1.5 B over an exact sample; 2.5 B over a sample in the nomination metric -- the kernels multiply by 1.5)
    if (c.harm || c.klent) list_widen(c, c.bound_coef(c.approx_samples ? 1.67f : 1.0f));
}

// The append scan over the whole gallery: 8 queries per tile, every tile of the call in one launch (blockIdx.y) -- the hand-scheduled
// LDS-tile kernel where it applies (L2, whole-chunk ranges, tile within 64 KiB), k_nominate for the two cheap forms, else the generic one.
int list_append_scan(const ListCall& c) {
    fir_gallery* g = c.g;
    const hipStream_t st = c.st;
    const int nh = c.nh, kk = g->dp4 * 4;
    const ScanKernel sk = select_scan(kEpiAppend, 8 * nh, c.nomination_metric(), whole_chunks(c.start, c.end), g->dp4, false);
    int launches_noted = 0, rc;
    int max_waves = max_waves_for(g, sk.fn, sk.lds_bytes);
    if (sk.fn_plain) max_waves = std::min(max_waves, max_waves_for(g, sk.fn_plain, sk.lds_bytes));
    const int waves = g->waves_req > 0 ? std::min(g->waves_req, max_waves) : pick_waves(g->tiles, max_waves, g->cus * 4);
    const int tiles_per_launch = nh == 2 ? std::max(2, g->max_tiles_per_launch & ~1) : g->max_tiles_per_launch;
    for (int q0 = 0; q0 < c.qpad; q0 += 8 * tiles_per_launch) {
        const int ny = std::min(tiles_per_launch, (c.qpad - q0) / 8);
        const int live = std::max(0, std::min(c.qb - q0, ny * 8));
        float* qt = g->qt + (size_t)q0 * kk;
        if (!c.tiles_ready)
            hipLaunchKernelGGL(k_transpose_queries, dim3((unsigned)(((int64_t)kk * 8 * ny + kBlock - 1) / kBlock)), dim3(kBlock), 0, st,
                               c.d_queries + (size_t)q0 * g->d, live, g->d, g->dp4, 8, qt, (uint64_t*)nullptr, 0, g->range, next_serial(g), c.transpose_form());
        ScanArgs a = scan_args(g, {}, c.start, c.end, waves);
        a.range = g->range;
        a.serial = g->q_serial;
        a.qt = qt;
        a.keys = c.lists + (size_t)q0 * kListCap;
        a.k = kListCap;
        a.tau = c.tau + q0;
        a.counts = c.counts + q0;
        a.qt_stride = (int64_t)kk * 8;
        a.flag = c.flag;
        a.sg = g->rowsum;
        a.sq = c.sq ? c.sq + q0 : nullptr;
        // algorithmic bytes of the launch: one read of the compared features per nh tiles of eight queries, the query tiles, the appended keys aside
        const double launch_bytes = (double)(ny / nh) * ((double)g->n * (c.end - c.start) * 4.0) + (double)ny * ((double)(c.end - c.start) * 32.0 + 64.0);
        if ((rc = fir_gallery_profile_begin_(g, st))) return rc;             // (never on behalf of another path: top1_dev)
        hipLaunchKernelGGL(sk.fn, dim3(waves / 4, ny / nh), dim3(kBlock), sk.lds_bytes, st, a);
        if (sk.fn_plain) hipLaunchKernelGGL(sk.fn_plain, dim3(waves / 4, ny), dim3(kBlock), sk.lds_bytes, st, a);
        if ((rc = fir_gallery_profile_end_(g, st, launch_bytes))) return rc;
        note_dispatch(g, (const void*)sk.fn, sk.name, launches_noted++, waves / 4, ny / nh, kBlock, sk.lds_bytes, 8 * nh, launch_bytes, 0.0, 0);
    }
    return FIR_OK;
}

// (nomination) the reference's distance of every appended row, keys rewritten in place; then the K smallest keys of every list.
// FIR_ERR_STATE when a list overflowed or a sample fell short (the flag the kernels raise).
int list_rerank_select(const ListCall& c, uint64_t* d_keys) {
    const fir_gallery* g = c.g;
    if (c.klent)
        hipLaunchKernelGGL(k_list_rerank<kKLInRange>, dim3(c.qb), dim3(kBlock), (size_t)g->d * sizeof(float), c.st, c.lists, c.counts, kListCap, g->gal4, g->dp4, g->n,
                           g->row_offset, c.d_queries, g->d, c.start, c.end);
    if (c.nominate)
        hipLaunchKernelGGL(k_list_rerank<kChi2>, dim3(c.qb), dim3(kBlock), (size_t)g->d * sizeof(float), c.st, c.lists, c.counts, kListCap, g->gal4, g->dp4, g->n,
                           g->row_offset, c.d_queries, g->d, c.start, c.end);
    hipLaunchKernelGGL(k_topk_select, dim3(c.qb), dim3(kBlock), 0, c.st, c.lists, c.counts, kListCap, c.k, d_keys, c.flag);
    FIR_HIP(hipGetLastError());
    int32_t h_flag = 0;
    FIR_HIP(hipMemcpyAsync(&h_flag, c.flag, 4, hipMemcpyDeviceToHost, c.st));
    FIR_HIP(hipStreamSynchronize(c.st));
    return h_flag ? FIR_ERR_STATE : FIR_OK;
}

// Every step of a call up to the candidate lists, queued on c.st: what list_rerank_select is handed, and what
// fir_gallery_list_nominations_ (tests) reads out instead. all_rows (tests only): every live query's threshold becomes +inf once it
// has been formed, so the append scan lists every row with its nomination value.
int list_nominate(ListCall& c, bool all_rows = false) {
    int rc;
    if ((rc = refresh_plain(c.g, c.st))) return rc;
    list_form(c);
    if ((rc = list_workspace(c))) return rc;
    if ((rc = list_row_sums(c))) return rc;
    if ((rc = list_row_samples(c))) return rc;
    list_threshold(c);
    if (all_rows) FIR_HIP(hipMemsetD32Async((hipDeviceptr_t)c.tau, (int)0x7F800000u, (size_t)c.qb, c.st));
    return list_append_scan(c);
}

// Returns FIR_ERR_STATE (without setting the error text) when a query could not be certified: fewer than K sample rows below
// 100000, or a list overflow.
int topk_lists_dev(fir_gallery* g, const float* d_queries, int32_t qb, int32_t start, int32_t end, int32_t k, uint64_t* d_keys,
                   hipStream_t st) {
    ListCall c{g, d_queries, qb, start, end, k, st};
    const int rc = list_nominate(c);
    return rc ? rc : list_rerank_select(c, d_keys);
}

// ---- the K nearest distinct classes (fir_search_top_classes) -----------------------------------------------------------------
// ConventionalTWDClassifier::recognize keeps the best row of every class (ImageTesting.cpp:118-122) and then the best classes
// (:141-149); here that is one gallery scan whose epilogue lowers cmin[query][class] (k_scan, kEpiClassMin) and a select kernel.
// kClassTableBytes: as many tiles of 8 queries share a launch (blockIdx.y) as keep the table within this budget -- 8 queries x
// 100 000 classes are 6.4 MB, ten tiles of them 64 MB: scattered 8-byte minima land in the 256 MiB Infinity Cache rather than
// in HBM -- but never fewer than one tile: num_classes may be as large as n, and the table is then 64 bytes per row.
constexpr size_t kClassTableBytes = (size_t)64 << 20;
constexpr int32_t kClassMax = 1 << 24;      // 1 GiB of table per tile of 8 queries: beyond it the call is refused, not attempted
// Galleries of at least this many tiles take a bound from a row sample first: the scan over the first eighth of the tiles
// leaves the minima of the classes met there; the K-th smallest of them is an upper bound
// tau of the final K-th class minimum (a minimum over a subset of the rows), so in the remaining tiles a row above tau -- almost
// every row -- cannot belong to an answer and never reaches the shuffles or the table. Fewer than K classes in the sample: tau
// stays 100000 and nothing is filtered.
constexpr int64_t kClassSampleFromTiles = 128;

// bound_tiles > 0 (fir_class_scan_dev_): only the scan over the leading bound_tiles tiles runs, and d_bound[q] gets its bound.
// Of `scope` only quiet is the caller's: the windows of the sample and of the remainder are made here.
int top_classes_dev(fir_gallery* g, const float* d_queries, int32_t qb, int32_t start, int32_t end, int32_t num_classes, int32_t k,
                    uint64_t* d_keys, int32_t* d_classes, hipStream_t st, const ScanScope& scope = {}, int64_t bound_tiles = 0,
                    float* d_bound = nullptr, const uint64_t* mask = nullptr) {
    // mask: both scans take their masked form -- the sample's bound is then the K-th smallest minimum over masked-in rows of the sample,
    // an upper bound of the masked answer's K-th class minimum for the same reason
    if (g->n == 0) {                                             // no row: every slot unused (kKeyNone, class -1)
        if (d_keys) FIR_HIP(hipMemsetAsync(d_keys, 0xFF, (size_t)qb * k * sizeof(uint64_t), st));
        if (d_classes) FIR_HIP(hipMemsetAsync(d_classes, 0xFF, (size_t)qb * k * sizeof(int32_t), st));
        return FIR_OK;
    }
    const int tiles_q = (qb + 7) / 8;
    const size_t tile_bytes = (size_t)8 * (size_t)num_classes * sizeof(uint64_t);
    const int per_launch = (int)std::min<size_t>(std::min(tiles_q, g->max_tiles_per_launch), std::max<size_t>(1, kClassTableBytes / tile_bytes));
    void *p_table = nullptr, *p_tau = nullptr;
    int rc;
    if ((rc = fir_gallery_scratch_(g, 17, tile_bytes * per_launch, &p_table))) return rc;
    if ((rc = fir_gallery_scratch_(g, 18, (size_t)per_launch * 8 * sizeof(float), &p_tau))) return rc;
    if ((rc = FIR_NEED(g->qt, (size_t)tiles_q * 8 * g->dp4 * 4 + 64))) return rc;
    uint64_t* table = (uint64_t*)p_table;
    float* tau = (float*)p_tau;
    const int64_t sample_tiles = bound_tiles > 0 ? std::min(bound_tiles, g->tiles) : g->tiles >= kClassSampleFromTiles ? g->tiles / 8 : 0;
    ScanScope sample = scope, rest = scope;      // (no sample: the remainder is the whole gallery)
    sample.tile_begin = 0;
    sample.tiles = sample_tiles;
    rest.tile_begin = sample_tiles;
    rest.tiles = sample_tiles > 0 ? g->tiles - sample_tiles : 0;
    for (int q0 = 0; q0 < qb; q0 += 8 * per_launch) {
        const int nq = std::min(qb - q0, 8 * per_launch), ny = (nq + 7) / 8;
        // a fresh table for every launch group: nothing of an earlier group, call, num_classes or k is left to see
        FIR_HIP(hipMemsetAsync(table, 0xFF, tile_bytes * ny, st));
        ClassPass cp{nullptr, num_classes, nq, false};
        if (sample_tiles > 0) {
            if ((rc = run_pass(g, st, sample, kEpiClassMin, d_queries, q0, 8, start, end, table, nullptr, 0, k, nullptr, ny, 0, &cp, 0, nullptr, mask))) return rc;
            hipLaunchKernelGGL(k_class_select, dim3(nq), dim3(kBlock), 0, st, table, num_classes, k, (uint64_t*)nullptr, (int32_t*)nullptr,
                               bound_tiles > 0 ? d_bound + q0 : tau);
            if (bound_tiles > 0) { FIR_HIP(hipGetLastError()); continue; }
            cp.tau = tau;
            cp.tiles_ready = true;
        }
        if ((rc = run_pass(g, st, rest, kEpiClassMin, d_queries, q0, 8, start, end, table, nullptr, 0, k, nullptr, ny, 0, &cp, 0, nullptr, mask))) return rc;
        hipLaunchKernelGGL(k_class_select, dim3(nq), dim3(kBlock), 0, st, table, num_classes, k, d_keys ? d_keys + (size_t)q0 * k : nullptr,
                           d_classes ? d_classes + (size_t)q0 * k : nullptr, (float*)nullptr);
        FIR_HIP(hipGetLastError());
    }
    return FIR_OK;
}

int range_dev(fir_gallery* g, const float* d_queries, int32_t qb, int32_t start, int32_t end, float* d_out, hipStream_t st) {
    int rc = FIR_NEED(g->qt, (size_t)qb * g->dp4 * 4);
    if (rc) return rc;
    int q0 = 0;
    while (q0 < qb) {
        const int t = largest_pow2_le(qb - q0, std::min(effective_qpp(g), 8));
        rc = run_pass(g, st, {}, kEpiStore, d_queries, q0, t, start, end, nullptr, d_out + (size_t)q0 * g->n, g->n, 0);
        if (rc) return rc;
        q0 += t;
    }
    return FIR_OK;
}

// ---- the K nearest rows for K up to FIR_KNN_MAX: store + select ---------------------------------------------------------------------
// Per tile of t queries (range_dev's choice of t) ONE gallery read: the store pass of range_dev writes the tile's exact distances
// into g->knn -- the reference's arithmetic, the bits fir_range_distances returns -- and the radix select of fir_knn_select.h
// takes the K smallest (distance, row) keys of each row of them. The slot holds one tile whatever qb is; when it cannot be had
// for t queries the tile is halved, down to one query. Nothing synchronises once the slot is large enough. Not recorded as the
// handle's dispatch (kOnBehalf): fir_gallery_last_dispatch describes searches that have a dominant scan kernel of their own.
// With fir_profile_enable on, every tile leaves two event pairs: around the store pass (transposition + scan), then around the select.
// FIR_KNN_SELECT_BLOCKS: workgroups per query of the select at most, for measurements (1 = one workgroup per query, the form
// profiles/knn_select.txt refutes: never the default).
int knn_select_blocks() {
    const char* e = fir_knob_("FIR_KNN_SELECT_BLOCKS");
    const int v = e ? atoi(e) : 0;
    return v >= 1 ? std::min(v, kKnnMaxBlocks) : kKnnMaxBlocks;
}
// The radius form (s.kind == kSearchRadius: fir_search_radius, k = max_results, 0 included): the same store pass, then per tile
// the count of the rows inside each query's radius (k_knn_count, into s.count) and the select with each query's own rank
// min(count, k) -- no digit passes for a query whose rows inside all fit. The second event pair is around count + select + sort.
int knn_dev(fir_gallery* g, const float* d_queries, int32_t qb, int32_t start, int32_t end, const FirSearch& s, hipStream_t st) {
    if (g->n == 0) {                                         // every slot FIR_KEY_NONE (all bytes 0xFF), every count 0
        if (s.k > 0) FIR_HIP(hipMemsetAsync(s.keys, 0xFF, s.key_words(qb) * sizeof(uint64_t), st));
        if (s.count) FIR_HIP(hipMemsetAsync(s.count, 0, (size_t)qb * sizeof(int32_t), st));
        return FIR_OK;
    }
    int t = largest_pow2_le(qb, std::min(effective_qpp(g), 8));
    KnnPlan plan = knn_plan(g->n, t, sizeof(KnnCtl));
    while (plan.bytes > g->knn.cap) {
        const hipError_t e = g->knn.reserve(plan.bytes);
        if (e == hipSuccess) break;
        (void)hipGetLastError();
        if (e != hipErrorOutOfMemory || t == 1)
            return fir_fail_(e == hipErrorOutOfMemory ? FIR_ERR_NOMEM : FIR_ERR_HIP, "no room for the distances of one query over %lld rows (%zu bytes): %s",
                             (long long)g->n, plan.bytes, hipGetErrorString(e));
        t /= 2;
        plan = knn_plan(g->n, t, sizeof(KnnCtl));
    }
    int rc = FIR_NEED(g->qt, (size_t)t * g->dp4 * 4);
    if (rc) return rc;
    const int blocks = knn_select_blocks();
    float* dist = g->knn.as<float>();
    for (int q0 = 0; q0 < qb;) {
        const int tt = largest_pow2_le(qb - q0, t);
        if ((rc = fir_gallery_profile_begin_(g, st))) return rc;
        // s.mask: the masked store pass -- masked-out rows are stored as 100000, which count and select reject like any row that far
        rc = run_pass(g, st, kOnBehalf, kEpiStore, d_queries + (size_t)q0 * g->d, 0, tt, start, end, nullptr, dist, plan.row_stride, 0, nullptr, 1, 0, nullptr, 0, nullptr, s.mask);
        if (rc) return rc;
        if ((rc = fir_gallery_profile_end_(g, st, (double)g->n * (end - start) * 4.0 + (s.mask ? g->tiles * 8.0 : 0.0)))) return rc;
        KnnArgs a{};
        a.dist = dist;
        a.n = g->n;
        a.stride = plan.row_stride;
        a.row_offset = g->row_offset;
        a.k = s.k;
        a.ctl = (KnnCtl*)((char*)g->knn.p + plan.dist_bytes);
        const FirSearch o = s.at(q0);
        a.out = o.keys; a.radius = o.radius; a.inside = o.count;
        if ((rc = fir_gallery_profile_begin_(g, st))) return rc;
        FIR_HIP(s.is_radius() ? (knn_select_launch<true, true>(a, tt, blocks, st)) : (knn_select_launch<true>(a, tt, blocks, st)));
        if ((rc = fir_gallery_profile_end_(g, st, (double)tt * g->n * 4.0))) return rc;
        q0 += tt;
    }
    return FIR_OK;
}

// ---- the sample bound of the matrix-core form for 8 < K <= FIR_GEMM_KNN_MAX (fir_gemm_knn.h) ----
// d_bound[q] = the exact K-th smallest reference distance of query q over the row sample of knn_sample_plan (fir_knn_select.h):
// 100000 with fewer than K qualifying rows there. The arithmetic is the store pass's, over features [0, end): the bits
// fir_range_distances returns. Queries go in groups whose stored distances fit kKnnSampleBytes of scratch slot 24 (and one launch's
// query tiles); per group one transposition, ONE store pass over the sample -- every tile of 8 queries of the group a blockIdx.y, the
// runs of the sample found by the kernel (ScanScope::run_len) -- and one select launch (k_knn_sample_kth, a workgroup per query).
// Nothing grows with qb, nothing synchronises once the slot is large enough.
int knn_sample_bound_dev(fir_gallery* g, const float* d_queries, int32_t qb, int32_t end, int32_t k, int div, float* d_bound, hipStream_t st) {
    const KnnSamplePlan plan = knn_sample_plan(g->n, k, div, kKnnSampleBytes);
    if (plan.rows < k) {                                     // (an empty gallery included) no bound
        FIR_HIP(hipMemsetD32Async((hipDeviceptr_t)d_bound, 0x47C35000, (size_t)qb, st));      // 100000.0f
        return FIR_OK;
    }
    const int group = std::min(std::min(plan.group, 8 * g->max_tiles_per_launch), (qb + 7) / 8 * 8);
    void* p_dist = nullptr;
    int rc;
    if ((rc = fir_gallery_scratch_(g, 24, (size_t)group * plan.row_stride * sizeof(float), &p_dist))) return rc;
    if ((rc = FIR_NEED(g->qt, (size_t)((group + 7) / 8 * 8) * g->dp4 * 4))) return rc;
    float* dist = (float*)p_dist;
    ScanScope sample = kOnBehalf;
    sample.tiles = plan.tiles;
    sample.run_len = (int32_t)plan.run_len;
    sample.run_count = plan.nruns;
    sample.run_slack = plan.slack;
    sample.run_rows = plan.rows;
    for (int g0 = 0; g0 < qb; g0 += group) {
        const int ng = std::min(group, qb - g0);
        // (a group of fewer than 8 queries -- a sample of more than 2M rows -- goes tile by tile, as range_dev sizes them)
        for (int q0 = 0; q0 < ng;) {
            const int tile = group >= 8 ? 8 : largest_pow2_le(ng - q0, 8), live = group >= 8 ? ng : tile;
            if ((rc = run_pass(g, st, sample, kEpiStore, d_queries + (size_t)(g0 + q0) * g->d, 0, tile, 0, end, nullptr, dist + (size_t)q0 * plan.row_stride,
                               plan.row_stride, 0, nullptr, (live + tile - 1) / tile, 0, nullptr, live)))
                return rc;
            q0 += live;
        }
        hipLaunchKernelGGL(k_knn_sample_kth, dim3(ng), dim3(kBlock), 0, st, (const float*)dist, plan.row_stride, plan.rows, k, d_bound + g0);
        FIR_HIP(hipGetLastError());
    }
    return FIR_OK;
}

int subranges_dev(fir_gallery* g, const float* d_queries, int32_t qb, int32_t start, int32_t end, int32_t step, float* d_out, hipStream_t st,
                  int32_t step2 = 0) {
    // step2 != 0: two sub-ranges, [start, start + step) and [start + step, end) with end - start - step == step2 (whole load groups both)
    const int nsub = step2 ? 2 : (end - start) / step;
    if (!step2 && (step % (4 * kUSub) != 0 || start % 4 != 0)) {   // one pass per sub-range (any step)
        g->last_subrange_kernel = "";
        for (int ci = 0; ci < nsub; ++ci) {
            const int rc = range_dev(g, d_queries, qb, start + ci * step, start + (ci + 1) * step, d_out + (size_t)ci * qb * g->n, st);
            if (rc) return rc;
        }
        return FIR_OK;
    }
    int rc = FIR_NEED(g->qt, (size_t)8 * g->dp4 * 4);
    if (rc) return rc;
    const int kk = g->dp4 * 4;
    for (int q0 = 0; q0 < qb; q0 += 8) {
        const int live = std::min(8, qb - q0);
        const int qbt = live <= 1 ? 1 : live <= 2 ? 2 : live <= 4 ? 4 : 8;   // kernel tile: the next power of two (extra queries are zero padding)
        const ScanKernel sk = select_scan(kEpiSubranges, qbt, g->metric, whole_chunks(start, end), g->dp4, false);
        const scan_fn fn = sk.fn;
        if (!fn) return fir_fail_(FIR_ERR_ARG, "no sub-range kernel for qb=%d metric=%d", qbt, g->metric);
        g->last_subrange_kernel = sk.name;
        hipLaunchKernelGGL(k_transpose_queries, dim3((unsigned)(((int64_t)kk * qbt + kBlock - 1) / kBlock)), dim3(kBlock), 0, st,
                           d_queries + (size_t)q0 * g->d, live, g->d, g->dp4, qbt, g->qt, (uint64_t*)nullptr, 0);
        const int max_waves = max_waves_for(g, fn, 0);
        ScanArgs a = scan_args(g, {}, start, end, pick_waves(g->tiles, max_waves, g->cus * 4));
        a.qt = g->qt;
        a.step = step;
        a.step2 = step2;
        a.out = d_out + (size_t)q0 * g->n;
        a.out_stride = g->n;
        a.nq = live;
        a.k = qb;
        hipLaunchKernelGGL(fn, dim3(a.waves / 4), dim3(kBlock), 0, st, a);
        FIR_HIP(hipGetLastError());
    }
    return FIR_OK;
}

// hipGetDeviceCount, the first time on the private random state of fir_runtime_init_ (it starts the runtime).
hipError_t device_count(int* cnt) {
    static bool started = false;
    if (started) return hipGetDeviceCount(cnt);
    char state[256];
    char* caller = initstate(1u, state, sizeof state);
    const hipError_t e = hipGetDeviceCount(cnt);
    setstate(caller);
    started = true;
    return e;
}

int set_device(int device) {
    int cnt = 0;
    if (device_count(&cnt) != hipSuccess || cnt <= 0) return fir_fail_(FIR_ERR_NODEVICE, "no HIP device visible");
    if (device < 0 || device >= cnt) return fir_fail_(FIR_ERR_NODEVICE, "device %d out of range (%d visible)", device, cnt);
    return fir_runtime_init_(device);
}

int gallery_alloc(int64_t n, int32_t d, int32_t metric, int32_t device, fir_gallery** out) {
    if (!out) return fir_fail_(FIR_ERR_ARG, "out is NULL");
    *out = nullptr;
    if (n < 0 || d <= 0) return fir_fail_(FIR_ERR_ARG, "bad gallery shape n=%lld d=%d", (long long)n, d);
    if (n >= ((int64_t)1 << 31) - 64) return fir_fail_(FIR_ERR_ARG, "n=%lld does not fit 32-bit row indices", (long long)n);
    if (metric < 0 || metric > 2) return fir_fail_(FIR_ERR_ARG, "bad metric %d", metric);
    int rc = set_device(device);
    if (rc) return rc;
    hipDeviceProp_t prop;
    FIR_HIP(hipGetDeviceProperties(&prop, device));
    if (strncmp(prop.gcnArchName, "gfx950", 6) != 0)
        return fir_fail_(FIR_ERR_NODEVICE, "device %d is %s; this library is built for gfx950 only", device, prop.gcnArchName);
    fir_gallery* g = new (std::nothrow) fir_gallery();
    if (!g) return fir_fail_(FIR_ERR_NOMEM, "host allocation failed");
    g->device = device;
    g->cus = prop.multiProcessorCount;
    g->n = n;
    g->d = d;
    g->dp4 = (d + 3) / 4;
    g->tiles = (n + kTileRows - 1) / kTileRows;
    g->cap_tiles = g->tiles;      // (an empty gallery's one tile is never written: its first append allocates)
    g->metric = metric;
    g->max_waves = g->cus * 8 * (kBlock / 64);
    const auto fail = [g](int code) { delete g; return code; };      // (the destructor releases whatever exists by then)
    hipError_t e = hipStreamCreateWithFlags(&g->stream, hipStreamNonBlocking);
    if (e != hipSuccess) return fail(fir_fail_(FIR_ERR_HIP, "hipStreamCreate: %s", hipGetErrorString(e)));
    e = hipEventCreateWithFlags(&g->last_done, hipEventDisableTiming);
    if (e != hipSuccess) return fail(fir_fail_(FIR_ERR_HIP, "hipEventCreate: %s", hipGetErrorString(e)));
    const size_t f4 = (size_t)std::max<int64_t>(g->tiles, 1) * g->dp4 * 64;
    e = g->gal4.reserve(f4 * sizeof(float4));
    if (e != hipSuccess) return fail(fir_fail_(FIR_ERR_NOMEM, "hipMalloc of %zu gallery bytes: %s", f4 * sizeof(float4), hipGetErrorString(e)));
    e = g->range.reserve(2 * sizeof(int32_t));
    if (e == hipSuccess) e = hipMemsetAsync(g->range, 0, 2 * sizeof(int32_t), g->stream);      // (not hipMemset: see fir_gallery_scratch_)
    if (e == hipSuccess) e = hipStreamSynchronize(g->stream);                                  // the retile may run on a caller's stream
    if (e != hipSuccess) return fail(fir_fail_(FIR_ERR_NOMEM, "hipMalloc of the range flags: %s", hipGetErrorString(e)));
    *out = g;
    return FIR_OK;
}

int retile_slab(fir_gallery* g, const float* d_rows, int64_t slab_rows, int64_t row0, hipStream_t st) {
    const int64_t slab_tiles = (slab_rows + kTileRows - 1) / kTileRows;
    const int64_t total = slab_tiles * g->dp4 * 64;
    if (total == 0) return FIR_OK;
    const int64_t blocks = (total + kBlock - 1) / kBlock;
    if (blocks > 0x7FFFFFFF) return fir_fail_(FIR_ERR_ARG, "slab too large");
    hipLaunchKernelGGL(k_retile, dim3((unsigned)blocks), dim3(kBlock), 0, st, d_rows, slab_rows, row0, g->n, g->d, g->dp4, g->gal4,
                       g->range);
    FIR_HIP(hipGetLastError());
    return FIR_OK;
}

// What the device-side constructors (fir_gallery_create_dev, fir_gallery_create_subset / _from_rows) share after gallery_alloc.
// labels_alloc: room for the labels of the handle's n > 0 rows; what fills them follows on the constructor's stream.
hipError_t labels_alloc(fir_gallery* g) {
    const hipError_t e = g->cls.reserve((size_t)g->n * sizeof(int32_t));
    g->cls_rows = g->n;
    return e;
}
// created_dev: the end of such a constructor -- rc is what queueing the rows and labels on `st` returned. One synchronisation, the
// plain-range flag read once, the handle handed out; on an error it is destroyed.
int created_dev(fir_gallery* g, int rc, hipStream_t st, fir_gallery** out) {
    if (rc == FIR_OK) {
        const hipError_t e = hipStreamSynchronize(st);
        if (e != hipSuccess) rc = fir_fail_(FIR_ERR_HIP, "gallery retile: %s", hipGetErrorString(e));
    }
    if (rc) { delete g; return rc; }
    { int32_t r0 = 1; if (hipMemcpy(&r0, g->range, sizeof r0, hipMemcpyDeviceToHost) == hipSuccess) g->gallery_plain = r0 == 0; }
    *out = g;
    return FIR_OK;
}

// ---- what every entry point that queues work on a handle starts with ------------------------------------------------------------
// The (queries, qb, range) arguments of a search: 0 = go on (end == 0 has become d), kNothingToDo = a call that succeeds without
// doing anything (qb == 0; or what `extra` says), < 0 = the error. pointers_ok: the entry point's other required pointers.
// extra(): its own checks, made where they have always been made -- after qb < 0, before qb == 0 and the range -- so that the
// first error a bad call reports stays the same; it returns as this function does.
constexpr int kNothingToDo = 1;
template <typename Extra>
int check_search(const fir_gallery* g, const void* queries, int32_t qb, int32_t& start, int32_t& end, bool pointers_ok, Extra extra) {
    if (!g || !pointers_ok || (qb > 0 && !queries)) return fir_fail_(FIR_ERR_ARG, "NULL argument");
    if (qb < 0) return fir_fail_(FIR_ERR_ARG, "qb < 0");
    if (const int rc = extra()) return rc;
    if (qb == 0) return kNothingToDo;
    return check_range(g, start, end);
}
int check_search(const fir_gallery* g, const void* queries, int32_t qb, int32_t& start, int32_t& end, bool pointers_ok = true) {
    return check_search(g, queries, qb, start, end, pointers_ok, [] { return FIR_OK; });
}
int check_k(int32_t k) { return k < 1 || k > kKMax ? fir_fail_(FIR_ERR_ARG, "k=%d outside [1,%d]", k, kKMax) : FIR_OK; }
int check_knn_k(int32_t k) { return knn_k_ok(k) ? FIR_OK : fir_fail_(FIR_ERR_ARG, "k=%d outside [1,%d]", k, kKnnMax); }
int check_max_results(int32_t m) { return m >= 0 && m <= kKnnMax ? FIR_OK : fir_fail_(FIR_ERR_ARG, "max_results=%d outside [0,%d]", m, kKnnMax); }

// One call on a handle: its device made current, the stream it queues on (the caller's, else the handle's own: a host-pointer
// call is a call on the handle's own stream) and its place in the handle's call order (FirCallOrder, which cannot be copied:
// this object lives in the entry point's scope). rc != 0: return it, nothing was queued.
struct GalleryCall {
    int rc;
    hipStream_t st;
    FirCallOrder order;
    static int make_current(const fir_gallery* g) { FIR_HIP(hipSetDevice(g->device)); return FIR_OK; }
    explicit GalleryCall(fir_gallery* g, void* stream = nullptr)
        : rc(make_current(g)), st(stream ? (hipStream_t)stream : g->stream), order(rc ? nullptr : g, st) { if (!rc) rc = order.rc; }
    void done() { order.done(); }       // all of the call's work has been seen to finish on the device
};

}  // namespace

extern "C" {

const char* fir_last_error(void) { return g_err; }
int fir_fail_(int code, const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
    return code;
}
int fir_gallery_view_(fir_gallery* g, fir_gallery_view* out) {
    if (!g || !out) return FIR_ERR_ARG;
    out->device = g->device; out->cus = g->cus; out->n = g->n; out->d = g->d; out->metric = g->metric; out->row_offset = g->row_offset;
    out->cls = g->cls; out->stream = g->stream; out->generation = g->generation;
    return FIR_OK;
}
int fir_gallery_call_begin_(fir_gallery* g, hipStream_t st) {
    if (!g || g->call_depth++ > 0) return FIR_OK;
    if (g->last_stream && g->last_stream != st) {          // (same stream: stream order already does it)
        const hipError_t e = hipStreamWaitEvent(st, g->last_done, 0);
        if (e != hipSuccess) return fir_fail_(FIR_ERR_HIP, "hipStreamWaitEvent (call order): %s", hipGetErrorString(e));
    }
    return FIR_OK;
}
void fir_gallery_call_end_(fir_gallery* g, hipStream_t st, int finished) {
    if (!g || --g->call_depth > 0) return;
    if (finished) g->last_stream = nullptr;                 // (its stream had passed the wait for every earlier call, too)
    else if (hipEventRecord(g->last_done, st) == hipSuccess) g->last_stream = st;
}
int fir_gallery_wait_calls_(fir_gallery* g) {
    if (!g || !g->last_stream) return FIR_OK;
    FIR_HIP(hipEventSynchronize(g->last_done));
    return FIR_OK;
}
__global__ void k_runtime_warmup(int* p) {
    if (p && threadIdx.x == 0 && blockIdx.x == 0) *p = 1;
}
int fir_runtime_init_(int device) {
    static bool touched[64] = {};
    if (device >= 0 && device < 64 && !touched[device]) {
        char state[256];
        char* caller = initstate(1u, state, sizeof state);      // the runtime's start-up draws from here ...
        hipError_t e = hipSetDevice(device);
        void* p = nullptr;
        hipStream_t st = nullptr;
        hipDeviceProp_t prop;
        if (e == hipSuccess) e = hipGetDeviceProperties(&prop, device);
        if (e == hipSuccess) e = hipMalloc(&p, 256);             // forces the context ...
        if (e == hipSuccess) e = hipStreamCreateWithFlags(&st, hipStreamNonBlocking);
        if (e == hipSuccess) {                                   // ... the code object load, a queue, a copy in each direction
            int h = 0;
            hipLaunchKernelGGL(k_runtime_warmup, dim3(1), dim3(64), 0, st, (int*)p);
            e = hipMemcpyAsync(&h, p, sizeof h, hipMemcpyDeviceToHost, st);
            if (e == hipSuccess) e = hipMemcpyAsync(p, &h, sizeof h, hipMemcpyHostToDevice, st);
            if (e == hipSuccess) e = hipStreamSynchronize(st);
        }
        if (st) (void)hipStreamDestroy(st);
        if (p) (void)hipFree(p);
        setstate(caller);                                        // ... and the caller's rand() stream continues where it was
        if (e != hipSuccess) return fir_fail_(FIR_ERR_HIP, "device %d start-up failed: %s", device, hipGetErrorString(e));
        touched[device] = true;
        return FIR_OK;
    }
    FIR_HIP(hipSetDevice(device));
    return FIR_OK;
}
int fir_gallery_scratch_(fir_gallery* g, int slot, size_t bytes, void** out) {
    if (!g || !out || slot < 0 || slot >= 25) return fir_fail_(FIR_ERR_ARG, "bad scratch request");
    FirBuf& s = g->scratch[slot];
    if (bytes > s.cap) {                                      // a quarter of headroom, a page at least
        const int rc = FIR_RESERVE(s, std::max<size_t>(bytes + bytes / 4, 4096));
        if (rc) return rc;
        // a fresh slot reads as zeros (fir_rows_distances' arrival counter, the fused TWD kernels' state) -- to whoever is handed
        // it, on whatever stream: hipMemset may return before the fill has run, and it runs on the null stream, which no
        // non-blocking stream waits for
        FIR_HIP(hipMemsetAsync(s.p, 0, s.cap, g->stream));
        FIR_HIP(hipStreamSynchronize(g->stream));
    }
    *out = s.p;
    return FIR_OK;
}
int fir_subrange_distances_dev_(fir_gallery* g, const float* d_queries, int32_t qb, int32_t start, int32_t end, int32_t step, float* d_out,
                                void* stream) {
    if (!g || !d_queries || !d_out) return fir_fail_(FIR_ERR_ARG, "NULL argument");
    if (qb <= 0) return fir_fail_(FIR_ERR_ARG, "qb=%d must be positive", qb);
    if (step <= 0 || start < 0 || end > g->d || start >= end || (end - start) % step != 0)
        return fir_fail_(FIR_ERR_ARG, "sub-ranges of %d features do not tile [%d,%d) inside [0,%d)", step, start, end, g->d);
    if (g->n == 0) return FIR_OK;
    GalleryCall call(g, stream);
    if (call.rc) return call.rc;
    return subranges_dev(g, d_queries, qb, start, end, step, d_out, call.st);
}
int fir_split_distances_dev_(fir_gallery* g, const float* d_queries, int32_t qb, int32_t split, int32_t end, float* d_out, void* stream) {
    if (!g || !d_queries || !d_out) return fir_fail_(FIR_ERR_ARG, "NULL argument");
    if (qb <= 0) return fir_fail_(FIR_ERR_ARG, "qb=%d must be positive", qb);
    if (split <= 0 || split >= end || end > g->d) return fir_fail_(FIR_ERR_ARG, "split %d / end %d outside (0,%d]", split, end, g->d);
    if (g->n == 0) return FIR_OK;
    GalleryCall call(g, stream);
    if (call.rc) return call.rc;
    const hipStream_t st = call.st;
    if (split % (4 * kUSub) == 0 && (end - split) % (4 * kUSub) == 0) return subranges_dev(g, d_queries, qb, 0, end, split, d_out, st, end - split);
    g->last_subrange_kernel = "";
    const int rc = range_dev(g, d_queries, qb, 0, split, d_out, st);
    if (rc) return rc;
    return range_dev(g, d_queries, qb, split, end, d_out + (size_t)qb * g->n, st);
}
const char* fir_gallery_last_subrange_kernel_(fir_gallery* g) { return g ? g->last_subrange_kernel : ""; }
int fir_gallery_tiled_(fir_gallery* g, const void** gal4, int* dp4) {
    if (!g || !gal4 || !dp4) return FIR_ERR_ARG;
    *gal4 = g->gal4;
    *dp4 = g->dp4;
    return FIR_OK;
}
void fir_set_last_error_(const char* msg) {
    strncpy(g_err, msg ? msg : "", sizeof(g_err) - 1);
    g_err[sizeof(g_err) - 1] = 0;
}
int fir_version(void) { return 100; }

int fir_device_count(void) {
    int cnt = 0;
    if (device_count(&cnt) != hipSuccess) return 0;
    return cnt;
}

int fir_device_info(int32_t device, char* name, int32_t cap, int32_t* cus, int64_t* hbm_bytes) {
    int cnt = 0;
    if (device_count(&cnt) != hipSuccess || device < 0 || device >= cnt)
        return fir_fail_(FIR_ERR_NODEVICE, "device %d not available", device);
    hipDeviceProp_t prop;
    FIR_HIP(hipGetDeviceProperties(&prop, device));
    if (name && cap > 0) { strncpy(name, prop.gcnArchName, (size_t)cap - 1); name[cap - 1] = 0; }
    if (cus) *cus = prop.multiProcessorCount;
    if (hbm_bytes) *hbm_bytes = (int64_t)prop.totalGlobalMem;
    return FIR_OK;
}

int fir_device_peak_hbm_gbs(int32_t device, double* gbs) {
    int cnt = 0;
    if (!gbs) return fir_fail_(FIR_ERR_ARG, "gbs is NULL");
    if (device_count(&cnt) != hipSuccess || device < 0 || device >= cnt)
        return fir_fail_(FIR_ERR_NODEVICE, "device %d not available", device);
    hipDeviceProp_t prop;
    FIR_HIP(hipGetDeviceProperties(&prop, device));
    if (strncmp(prop.gcnArchName, "gfx950", 6) != 0) return fir_fail_(FIR_ERR_NODEVICE, "device %d is %s, not gfx950", device, prop.gcnArchName);
    *gbs = 8000.0;   // MI350X / MI355X: 8 stacks of HBM3E, 8 TB/s (the runtime's clock x bus-width fields do not give this)
    return FIR_OK;
}

int fir_gallery_create(const float* rows, int64_t n, int32_t d, const int32_t* class_no, int32_t metric, int32_t device,
                       fir_gallery** out) {
    if (n > 0 && !rows) return fir_fail_(FIR_ERR_ARG, "rows is NULL");
    fir_gallery* g = nullptr;
    int rc = gallery_alloc(n, d, metric, device, &g);
    if (rc) return rc;
    // upload in slabs of whole tiles (<= 256 MiB of rows each) and re-tile on the device
    int64_t slab = std::max<int64_t>(kTileRows, ((int64_t)(256u << 20) / ((int64_t)d * 4)) / kTileRows * kTileRows);
    slab = std::min<int64_t>(slab, std::max<int64_t>(g->tiles, 1) * kTileRows);
    GalleryBuf<float> stage;                               // (gone when this function returns)
    hipError_t e = stage.reserve((size_t)slab * d * sizeof(float));
    if (e != hipSuccess) { delete g; return fir_fail_(FIR_ERR_NOMEM, "staging hipMalloc: %s", hipGetErrorString(e)); }
    for (int64_t r0 = 0; r0 < std::max<int64_t>(g->tiles, 1) * kTileRows && rc == FIR_OK; r0 += slab) {
        const int64_t have = std::max<int64_t>(0, std::min<int64_t>(slab, n - r0));
        if (have > 0) {
            e = hipMemcpyAsync(stage, rows + r0 * d, (size_t)have * d * sizeof(float), hipMemcpyHostToDevice, g->stream);
            if (e != hipSuccess) { rc = fir_fail_(FIR_ERR_HIP, "gallery upload: %s", hipGetErrorString(e)); break; }
        }
        if (have > 0) rc = retile_slab(g, stage, have, r0, g->stream);
        e = hipStreamSynchronize(g->stream);   // the staging buffer is reused by the next slab
        if (e != hipSuccess && rc == FIR_OK) rc = fir_fail_(FIR_ERR_HIP, "gallery retile: %s", hipGetErrorString(e));
    }
    stage.release();                                       // before the labels are allocated, as ever
    if (rc == FIR_OK && class_no && n > 0) {
        e = g->cls.reserve((size_t)n * sizeof(int32_t));
        g->cls_rows = n;
        if (e == hipSuccess) e = hipMemcpy(g->cls, class_no, (size_t)n * sizeof(int32_t), hipMemcpyHostToDevice);
        if (e != hipSuccess) rc = fir_fail_(FIR_ERR_HIP, "class upload: %s", hipGetErrorString(e));
    }
    if (rc) { delete g; return rc; }
    { int32_t r0 = 1; if (hipMemcpy(&r0, g->range, sizeof r0, hipMemcpyDeviceToHost) == hipSuccess) g->gallery_plain = r0 == 0; }
    *out = g;
    return FIR_OK;
}

int fir_gallery_create_dev(const float* d_rows, int64_t n, int32_t d, const int32_t* d_class_no, int32_t metric,
                           int32_t device, void* stream, fir_gallery** out) {
    if (n > 0 && !d_rows) return fir_fail_(FIR_ERR_ARG, "d_rows is NULL");
    fir_gallery* g = nullptr;
    int rc = gallery_alloc(n, d, metric, device, &g);
    if (rc) return rc;
    hipStream_t st = stream ? (hipStream_t)stream : g->stream;
    // slabs keep the launch grid inside 2^31 blocks
    const int64_t slab = std::max<int64_t>(kTileRows, ((int64_t)1 << 30) / ((int64_t)g->dp4 * 4) / kTileRows * kTileRows);
    for (int64_t r0 = 0; r0 < g->tiles * kTileRows && rc == FIR_OK; r0 += slab) {
        const int64_t span = std::min<int64_t>(slab, g->tiles * kTileRows - r0);
        rc = retile_slab(g, d_rows + r0 * d, span, r0, st);
    }
    if (rc == FIR_OK && d_class_no && n > 0) {
        hipError_t e = labels_alloc(g);
        if (e == hipSuccess) e = hipMemcpyAsync(g->cls, d_class_no, (size_t)n * sizeof(int32_t), hipMemcpyDeviceToDevice, st);
        if (e != hipSuccess) rc = fir_fail_(FIR_ERR_HIP, "class copy: %s", hipGetErrorString(e));
    }
    return created_dev(g, rc, st, out);
}

int fir_gallery_destroy(fir_gallery* g) {
    if (!g) return FIR_OK;
    (void)hipSetDevice(g->device);
    (void)fir_gallery_wait_calls_(g);         // calls queued on the callers' streams may still use what is freed below
    if (g->stream) (void)hipStreamSynchronize(g->stream);
    delete g;
    return FIR_OK;
}

int fir_gallery_info(const fir_gallery* g, int64_t* n, int32_t* d, int32_t* metric, int32_t* device) {
    if (!g) return fir_fail_(FIR_ERR_ARG, "gallery is NULL");
    if (n) *n = g->n;
    if (d) *d = g->d;
    if (metric) *metric = g->metric;
    if (device) *device = g->device;
    return FIR_OK;
}

int fir_gallery_set_metric(fir_gallery* g, int32_t metric) {
    if (!g) return fir_fail_(FIR_ERR_ARG, "gallery is NULL");
    if (metric < 0 || metric > 2) return fir_fail_(FIR_ERR_ARG, "bad metric %d", metric);
    g->metric = metric;
    return FIR_OK;
}

int fir_gallery_set_large_batch_mfma(fir_gallery* g, int32_t min_queries) {
    if (!g) return fir_fail_(FIR_ERR_ARG, "gallery is NULL");
    g->large_batch_min = min_queries < 0 ? -1 : min_queries;
    g->gemm_failed = false;
    if (min_queries == 0) g->drop_gemm_states();
    return FIR_OK;
}

int fir_gallery_set_int8_nomination(fir_gallery* g, int32_t mode) {
    if (!g) return fir_fail_(FIR_ERR_ARG, "gallery is NULL");
    if (mode < -1 || mode > 1) return fir_fail_(FIR_ERR_ARG, "int8 nomination mode %d outside [-1,1]", mode);
    g->int8_mode = mode;
    return FIR_OK;
}

int fir_gallery_mfma_stats_ex(fir_gallery* g, int64_t out[3]) {
    if (!g || !out) return fir_fail_(FIR_ERR_ARG, "NULL argument");
    int64_t o[3];
    out[0] = out[1] = out[2] = 0;
    if (g->gemm && fir_gemm_stats_ex(g->gemm, o) == FIR_OK) { out[0] += o[0]; out[1] += o[1]; out[2] += o[2]; }
    for (auto& ps : g->gemm_prefix)
        if (ps.m && fir_gemm_stats_ex(ps.m, o) == FIR_OK) { out[0] += o[0]; out[1] += o[1]; out[2] += o[2]; }
    // (states dropped since -- fir_gallery_set_large_batch_mfma(g, 0) frees them -- took their counters along)
    return FIR_OK;
}

int fir_gallery_mfma_uncertified_notes(fir_gallery* g, float out[32], int32_t* count) {
    if (!g || !out || !count) return fir_fail_(FIR_ERR_ARG, "NULL argument");
    *count = 0;
    if (!g->gemm) return FIR_OK;
    return fir_gemm_uncertified_notes(g->gemm, out, count);
}

int fir_gallery_mfma_stats(fir_gallery* g, int64_t* passes, int64_t* fallback_queries) {
    int64_t o[3];
    const int rc = fir_gallery_mfma_stats_ex(g, o);
    if (rc) return rc;
    if (passes) *passes = o[0];
    if (fallback_queries) *fallback_queries = o[2];
    return FIR_OK;
}

int fir_gallery_memory_bytes(fir_gallery* g, int64_t* tiled, int64_t* fp16_fragments, int64_t* rowmajor_shadow, int64_t* scratch) {
    if (!g) return fir_fail_(FIR_ERR_ARG, "gallery is NULL");
    int64_t fr = 0, rm = 0, sc = 0, a = 0, b = 0, c = 0;
    if (g->gemm) { fir_gemm_memory_bytes_(g->gemm, &a, &b, &c); fr += a; rm += b; sc += c; }
    for (auto& ps : g->gemm_prefix)
        if (ps.m) { fir_gemm_memory_bytes_(ps.m, &a, &b, &c); fr += a; rm += b; sc += c; }
    // the capacities of the workspaces and the scratch slots; the range flags and the one-query key block (16 and 64 bytes) are
    // reported nowhere, as ever
    sc += (int64_t)g->scratch_bytes();
    // (the allocated capacity: on a handle that was never updated the tiles and labels of its n rows)
    if (tiled) *tiled = (int64_t)g->cap_tiles * fir::kTileRows * (int64_t)((g->d + 3) / 4) * 16 + (g->cls ? (int64_t)g->cls_rows * 4 : 0);
    if (fp16_fragments) *fp16_fragments = fr;
    if (rowmajor_shadow) *rowmajor_shadow = rm;
    if (scratch) *scratch = sc;
    return FIR_OK;
}

int fir_gallery_set_shadow_copies(fir_gallery* g, int32_t mode) {
    if (!g) return fir_fail_(FIR_ERR_ARG, "gallery is NULL");
    if (mode != FIR_SHADOW_NONE && mode != FIR_SHADOW_FP16 && mode != FIR_SHADOW_ALL) return fir_fail_(FIR_ERR_ARG, "shadow mode %d", mode);
    if (mode != g->shadow_mode) {
        g->drop_gemm_states();
        g->gemm_failed = false;
    }
    g->shadow_mode = mode;
    return FIR_OK;
}

int fir_gallery_set_row_offset(fir_gallery* g, int64_t first_global_row) {
    if (!g) return fir_fail_(FIR_ERR_ARG, "gallery is NULL");
    if (first_global_row < 0 || first_global_row + g->n >= ((int64_t)1 << 31))
        return fir_fail_(FIR_ERR_ARG, "row offset %lld + n does not fit 32-bit indices", (long long)first_global_row);
    g->row_offset = first_global_row;
    g->drop_gemm_states();                                           // they cache the offset; rebuilt on next use
    return FIR_OK;
}

// ---- in-place updates: append, overwrite and remove rows (include/fir_amd.h has the contract) -------------------------------------
// Every successful mutation ends in gallery_changed(): whatever the handle caches about rows, labels or n starts again, and the
// generation moves on, which the states other code built over the handle compare with theirs (fir_gallery_stale_).
namespace {
constexpr int64_t kRowLimit = ((int64_t)1 << 31) - 64;        // gallery_alloc's limit, for n + row offset
constexpr int64_t kUpdateSlabBytes = (int64_t)64 << 20;       // host rows pass through g->dq in slabs of this size

void gallery_changed(fir_gallery* g) {
    ++g->generation;
    g->tiles = (g->n + kTileRows - 1) / kTileRows;
    g->rs_start = g->rs_end = g->rs_metric = -1;              // row sums / entropies (list_row_sums)
    g->label_known = false;
    g->small_hits = g->few_hits = 0;                          // the warm-up and learnt-dispatch counters start again
    g->gemm_failed = false;
    g->warm_left = 0;
    g->plain_stale = true;
    g->origin_ok = false;                                     // a subset handle's rows are no longer its row list's (the buffer stays: queued key maps read it)
    // (the handle's matrix-core states carry their generation: drop_stale_gemm_states)
}

int check_mutable(const fir_gallery* g) {
    if (!g) return fir_fail_(FIR_ERR_ARG, "gallery is NULL");
    if (g->borrowed) return fir_fail_(FIR_ERR_STATE, "the gallery is a shard of a sharded handle: its rows cannot be changed");
    return FIR_OK;
}

int64_t capacity_rows(const fir_gallery* g) {
    const int64_t rows = g->cap_tiles * kTileRows;
    return g->cls ? std::min(rows, g->cls_rows) : rows;
}

// Room for need_rows rows, and for their labels when `labels`. Nothing to do when both are there. Otherwise: wait for the handle's
// queued calls (they read the old buffers), allocate -- with a quarter of headroom when `headroom`, the exact size when that cannot
// be had --, copy on the device, clear the new tiles, free the old buffers. Old and new buffers exist side by side until the copy
// is done. On failure the handle is as it was.
int gallery_room(fir_gallery* g, int64_t need_rows, bool headroom, bool labels) {
    const bool grow_tiles = need_rows > g->cap_tiles * kTileRows;
    const bool grow_cls = labels && need_rows > g->cls_rows;
    if (!grow_tiles && !grow_cls) return FIR_OK;
    int rc = fir_gallery_wait_calls_(g);
    if (rc) return rc;
    FIR_HIP(hipStreamSynchronize(g->stream));
    const size_t tile_bytes = (size_t)g->dp4 * 64 * sizeof(float4);
    for (int attempt = headroom ? 0 : 1; attempt < 2; ++attempt) {
        const int64_t rows = attempt == 0 ? need_rows + need_rows / 4 : need_rows;
        const int64_t new_tiles = grow_tiles ? (rows + kTileRows - 1) / kTileRows : g->cap_tiles;
        const int64_t new_cls_rows = new_tiles * kTileRows;
        GalleryBuf<float4> ngal;
        GalleryBuf<int32_t> ncls;
        hipError_t e = hipSuccess;
        if (grow_tiles) e = ngal.reserve((size_t)new_tiles * tile_bytes);
        if (e == hipSuccess && (grow_cls || (grow_tiles && g->cls))) e = ncls.reserve((size_t)new_cls_rows * sizeof(int32_t));
        if (e == hipErrorOutOfMemory) { (void)hipGetLastError(); continue; }        // (what was allocated goes with this scope)
        if (e != hipSuccess) return fir_fail_(FIR_ERR_HIP, "hipMalloc of the grown gallery: %s", hipGetErrorString(e));
        if (grow_tiles) {
            const size_t used = (size_t)g->tiles * tile_bytes;
            if (used) FIR_HIP(hipMemcpyAsync(ngal.p, g->gal4.p, used, hipMemcpyDeviceToDevice, g->stream));
            FIR_HIP(hipMemsetAsync((char*)ngal.p + used, 0, (size_t)new_tiles * tile_bytes - used, g->stream));
        }
        if (ncls.p && g->cls && g->n > 0) FIR_HIP(hipMemcpyAsync(ncls.p, g->cls.p, (size_t)g->n * sizeof(int32_t), hipMemcpyDeviceToDevice, g->stream));
        FIR_HIP(hipStreamSynchronize(g->stream));
        if (grow_tiles) { std::swap(g->gal4.p, ngal.p); std::swap(g->gal4.cap, ngal.cap); g->cap_tiles = new_tiles; }
        if (ncls.p) { std::swap(g->cls.p, ncls.p); std::swap(g->cls.cap, ncls.cap); g->cls_rows = new_cls_rows; }
        g->drop_gemm_states();                  // they hold the old buffer's address
        const bool plain_stale = g->plain_stale, origin_ok = g->origin_ok;
        gallery_changed(g);
        g->plain_stale = plain_stale;           // (the rows were copied, not changed: range[0] still says what gallery_plain says)
        g->origin_ok = origin_ok;               // (... and a subset handle's rows are still its row list's)
        return FIR_OK;                         // (ngal / ncls now own the old buffers: freed here)
    }
    return fir_fail_(FIR_ERR_NOMEM, "no device memory for a gallery of %lld rows", (long long)need_rows);
}

// The checks of both appends, in the order of the other calls. 0 = go on, kNothingToDo, < 0 = the error.
int check_append(const fir_gallery* g, const void* rows, int64_t m, const void* class_no) {
    const int rc = check_mutable(g);
    if (rc) return rc;
    if (m > 0 && !rows) return fir_fail_(FIR_ERR_ARG, "NULL argument");
    if (m < 0) return fir_fail_(FIR_ERR_ARG, "m < 0");
    if (m == 0) return kNothingToDo;
    if (g->n > 0 && g->cls && !class_no) return fir_fail_(FIR_ERR_ARG, "the gallery has class labels: appended rows need class_no");
    if (g->n > 0 && !g->cls && class_no) return fir_fail_(FIR_ERR_ARG, "the gallery has no class labels: class_no must be NULL");
    if (g->n + m + g->row_offset >= kRowLimit)
        return fir_fail_(FIR_ERR_ARG, "n + m + row offset = %lld does not fit 32-bit row indices", (long long)(g->n + m + g->row_offset));
    return FIR_OK;
}

// The room for n + m rows. An empty handle takes its labelled-ness from its first append: it holds no labels (one created empty keeps
// none, one emptied by fir_gallery_remove_rows gives them up there), so `labels` alone decides whether a label buffer is made.
int append_room(fir_gallery* g, int64_t m, bool labels) { return gallery_room(g, g->n + m, true, labels); }

int launch_append(fir_gallery* g, const float* d_rows, int64_t m, int64_t first, hipStream_t st) {
    const int64_t ntiles = (first + m + kTileRows - 1) / kTileRows - first / kTileRows;
    const int64_t blocks = (ntiles * g->dp4 * 64 + kBlock - 1) / kBlock;
    hipLaunchKernelGGL(k_append_rows, dim3((unsigned)blocks), dim3(kBlock), 0, st, d_rows, m, first, g->d, g->dp4, (float4*)g->gal4, (int32_t*)g->range);
    FIR_HIP(hipGetLastError());
    return FIR_OK;
}
// rows per slab of a host-pointer update: the launch grid stays inside 2^31 blocks, the staging buffer inside kUpdateSlabBytes
int64_t update_slab_rows(const fir_gallery* g) { return std::max<int64_t>(kTileRows, kUpdateSlabBytes / ((int64_t)g->dp4 * 16) / kTileRows * kTileRows); }

// row_idx[m]: inside [0, n) and distinct. sorted <- the indices ascending.
int check_row_list(int64_t n, const int32_t* row_idx, int32_t m, std::vector<int32_t>& sorted) {
    sorted.assign(row_idx, row_idx + m);
    std::sort(sorted.begin(), sorted.end());
    if (sorted.front() < 0 || sorted.back() >= n) return fir_fail_(FIR_ERR_ARG, "row index %d outside [0,%lld)", sorted.front() < 0 ? sorted.front() : sorted.back(), (long long)n);
    for (int32_t i = 1; i < m; ++i)
        if (sorted[i] == sorted[i - 1]) return fir_fail_(FIR_ERR_ARG, "row index %d is listed twice", sorted[i]);
    return FIR_OK;
}

// The removal rule. dst_of (may be NULL) <- for each tail row n' + i its hole, -1 when the row is removed itself.
int remove_plan(int64_t n, const int32_t* row_idx, int32_t m, int32_t* moved_from, std::vector<int32_t>* dst_of) {
    if (n < 0 || (m > 0 && !row_idx)) return fir_fail_(FIR_ERR_ARG, n < 0 ? "n < 0" : "NULL argument");
    if (m < 0) return fir_fail_(FIR_ERR_ARG, "m < 0");
    if (dst_of) dst_of->clear();
    if (m == 0) return FIR_OK;
    std::vector<int32_t> sorted;
    const int rc = check_row_list(n, row_idx, m, sorted);
    if (rc) return rc;
    const int64_t n_new = n - m;
    const size_t holes = (size_t)(std::lower_bound(sorted.begin(), sorted.end(), n_new) - sorted.begin());     // sorted[0, holes): the holes, ascending
    std::vector<int32_t> survivors;                                  // the rows of [n', n) that stay, ascending: as many as holes
    survivors.reserve(holes);
    if (dst_of) dst_of->assign((size_t)m, -1);
    size_t t = holes;
    for (int64_t r = n_new; r < n; ++r) {
        if (t < sorted.size() && sorted[t] == r) { ++t; continue; }
        if (dst_of) (*dst_of)[(size_t)(r - n_new)] = sorted[survivors.size()];
        survivors.push_back((int32_t)r);
    }
    if (moved_from)
        for (int32_t i = 0; i < m; ++i)
            moved_from[i] = row_idx[i] >= n_new ? -1 : survivors[(size_t)(std::lower_bound(sorted.begin(), sorted.begin() + (long)holes, row_idx[i]) - sorted.begin())];
    return FIR_OK;
}
}  // namespace

void fir_gallery_set_borrowed_(fir_gallery* g, int borrowed) { if (g) g->borrowed = borrowed != 0; }
uint64_t fir_gallery_generation_(const fir_gallery* g) { return g ? g->generation : 0; }
int fir_gallery_stale_(const fir_gallery* g, uint64_t built_at, const char* what) {
    if (!g || g->generation == built_at) return FIR_OK;
    return fir_fail_(FIR_ERR_STATE, "the gallery changed after this %s state was built (rows were appended, overwritten or removed): destroy it and create it again", what);
}

int fir_gallery_reserve(fir_gallery* g, int64_t rows) {
    const int rc = check_mutable(g);
    if (rc) return rc;
    if (rows <= g->n) return FIR_OK;
    if (rows + g->row_offset >= kRowLimit) return fir_fail_(FIR_ERR_ARG, "rows + row offset = %lld does not fit 32-bit row indices", (long long)(rows + g->row_offset));
    FIR_HIP(hipSetDevice(g->device));
    return gallery_room(g, rows, false, g->cls != nullptr);
}

int fir_gallery_capacity(const fir_gallery* g, int64_t* rows) {
    if (!g || !rows) return fir_fail_(FIR_ERR_ARG, "NULL argument");
    *rows = std::max(capacity_rows(g), g->n);
    return FIR_OK;
}

int fir_gallery_append_dev(fir_gallery* g, const float* d_rows, int64_t m, const int32_t* d_class_no, void* stream) {
    int rc = check_append(g, d_rows, m, d_class_no);
    if (rc) return rc < 0 ? rc : FIR_OK;
    FIR_HIP(hipSetDevice(g->device));
    if ((rc = append_room(g, m, d_class_no != nullptr))) return rc;
    GalleryCall call(g, stream);
    if (call.rc) return call.rc;
    const int64_t slab = update_slab_rows(g);
    for (int64_t r0 = 0; r0 < m; r0 += slab)
        if ((rc = launch_append(g, d_rows + r0 * g->d, std::min(slab, m - r0), g->n + r0, call.st))) return rc;
    if (d_class_no) FIR_HIP(hipMemcpyAsync(g->cls + g->n, d_class_no, (size_t)m * sizeof(int32_t), hipMemcpyDeviceToDevice, call.st));
    g->n += m;
    gallery_changed(g);
    return FIR_OK;
}

int fir_gallery_append(fir_gallery* g, const float* rows, int64_t m, const int32_t* class_no) {
    int rc = check_append(g, rows, m, class_no);
    if (rc) return rc < 0 ? rc : FIR_OK;
    FIR_HIP(hipSetDevice(g->device));
    // the staging buffer first (only host-pointer calls use it, and those have finished): if it cannot be had, nothing has grown yet
    const int64_t slab = std::min(update_slab_rows(g), m);
    if ((rc = FIR_NEED(g->dq, (size_t)slab * g->d))) return rc;
    if ((rc = append_room(g, m, class_no != nullptr))) return rc;
    g->drop_gemm_states();                                 // (this call waits anyway: their memory goes now, not with the next routed call)
    GalleryCall call(g);
    if (call.rc) return call.rc;
    for (int64_t r0 = 0; r0 < m; r0 += slab) {
        const int64_t have = std::min(slab, m - r0);
        FIR_HIP(hipMemcpyAsync(g->dq, rows + r0 * g->d, (size_t)have * g->d * sizeof(float), hipMemcpyHostToDevice, g->stream));
        if ((rc = launch_append(g, g->dq, have, g->n + r0, g->stream))) return rc;
        FIR_HIP(hipStreamSynchronize(g->stream));           // the staging buffer is reused by the next slab
    }
    if (class_no) FIR_HIP(hipMemcpyAsync(g->cls + g->n, class_no, (size_t)m * sizeof(int32_t), hipMemcpyHostToDevice, g->stream));
    FIR_HIP(hipStreamSynchronize(g->stream));
    g->n += m;
    gallery_changed(g);
    call.done();
    return refresh_plain(g, g->stream);
}

int fir_gallery_set_rows(fir_gallery* g, const int32_t* row_idx, int32_t m, const float* new_rows, const int32_t* class_no) {
    int rc = check_mutable(g);
    if (rc) return rc;
    if (m > 0 && (!row_idx || !new_rows)) return fir_fail_(FIR_ERR_ARG, "NULL argument");
    if (m < 0) return fir_fail_(FIR_ERR_ARG, "m < 0");
    if (m == 0) return FIR_OK;
    if (class_no && !g->cls) return fir_fail_(FIR_ERR_ARG, "the gallery has no class labels: class_no must be NULL");
    std::vector<int32_t> sorted;
    if ((rc = check_row_list(g->n, row_idx, m, sorted))) return rc;
    FIR_HIP(hipSetDevice(g->device));
    const int64_t slab = std::min<int64_t>(update_slab_rows(g), m);
    if ((rc = FIR_NEED(g->dq, (size_t)slab * g->d)) || (rc = FIR_NEED(g->didx, (size_t)2 * m))) return rc;
    g->drop_gemm_states();
    GalleryCall call(g);
    if (call.rc) return call.rc;
    FIR_HIP(hipMemcpyAsync(g->didx, row_idx, (size_t)m * sizeof(int32_t), hipMemcpyHostToDevice, g->stream));
    if (class_no) FIR_HIP(hipMemcpyAsync(g->didx + m, class_no, (size_t)m * sizeof(int32_t), hipMemcpyHostToDevice, g->stream));
    for (int64_t r0 = 0; r0 < m; r0 += slab) {
        const int64_t have = std::min<int64_t>(slab, m - r0);
        FIR_HIP(hipMemcpyAsync(g->dq, new_rows + r0 * g->d, (size_t)have * g->d * sizeof(float), hipMemcpyHostToDevice, g->stream));
        hipLaunchKernelGGL(k_scatter_rows, dim3((unsigned)((have * g->dp4 + kBlock - 1) / kBlock)), dim3(kBlock), 0, g->stream, (const float*)g->dq,
                           (const int32_t*)(g->didx + r0), have, g->d, g->dp4, (float4*)g->gal4, (int32_t*)g->range,
                           class_no ? (const int32_t*)(g->didx + m + r0) : (const int32_t*)nullptr, (int32_t*)g->cls);
        FIR_HIP(hipGetLastError());
        FIR_HIP(hipStreamSynchronize(g->stream));
    }
    gallery_changed(g);
    call.done();
    return refresh_plain(g, g->stream);
}

int fir_gallery_remove_plan(int64_t n, const int32_t* row_idx, int32_t m, int32_t* moved_from) { return remove_plan(n, row_idx, m, moved_from, nullptr); }

int fir_gallery_remove_rows(fir_gallery* g, const int32_t* row_idx, int32_t m, int32_t* moved_from) {
    int rc = check_mutable(g);
    if (rc) return rc;
    std::vector<int32_t> dst_of, moved((size_t)std::max(m, 0));       // (moved_from is the caller's: written only after the checks and the allocation have passed)
    if ((rc = remove_plan(g->n, row_idx, m, moved_from ? moved.data() : nullptr, &dst_of))) return rc;
    if (m == 0) return FIR_OK;
    FIR_HIP(hipSetDevice(g->device));
    if ((rc = FIR_NEED(g->didx, (size_t)m))) return rc;
    g->drop_gemm_states();
    GalleryCall call(g);
    if (call.rc) return call.rc;
    if (moved_from) std::copy(moved.begin(), moved.end(), moved_from);
    const int64_t n_new = g->n - m;
    FIR_HIP(hipMemcpyAsync(g->didx, dst_of.data(), (size_t)m * sizeof(int32_t), hipMemcpyHostToDevice, g->stream));
    hipLaunchKernelGGL(k_move_rows, dim3((unsigned)(((int64_t)m * g->dp4 + kBlock - 1) / kBlock)), dim3(kBlock), 0, g->stream, (float4*)g->gal4, g->dp4, n_new,
                       (int64_t)m, (const int32_t*)g->didx, (int32_t*)g->cls);
    FIR_HIP(hipGetLastError());
    FIR_HIP(hipStreamSynchronize(g->stream));
    g->n = n_new;
    if (n_new == 0 && g->cls) {                             // as fir_gallery_create with n == 0: an empty handle keeps no labels
        g->cls.release();
        g->cls_rows = 0;
    }
    const bool plain_stale = g->plain_stale;
    gallery_changed(g);
    g->plain_stale = plain_stale;                           // (rows moved and cleared: no value a row did not hold before)
    call.done();
    return FIR_OK;
}

int fir_gallery_read_rows(fir_gallery* g, int64_t row0, int64_t m, float* rows_out, int32_t* class_out) {
    if (!g || (m > 0 && !rows_out)) return fir_fail_(FIR_ERR_ARG, "NULL argument");
    if (m < 0) return fir_fail_(FIR_ERR_ARG, "m < 0");
    if (m == 0) return FIR_OK;
    if (class_out && !g->cls) return fir_fail_(FIR_ERR_STATE, "gallery was created without class labels");
    if (row0 < 0 || row0 > g->n || m > g->n - row0) return fir_fail_(FIR_ERR_ARG, "rows [%lld,+%lld) outside [0,%lld)", (long long)row0, (long long)m, (long long)g->n);
    FIR_HIP(hipSetDevice(g->device));
    const int64_t slab = std::min(update_slab_rows(g), m);
    int rc = FIR_NEED(g->dq, (size_t)slab * g->d);
    if (rc) return rc;
    GalleryCall call(g);
    if (call.rc) return call.rc;
    for (int64_t r0 = 0; r0 < m; r0 += slab) {
        const int64_t have = std::min(slab, m - r0);
        hipLaunchKernelGGL(k_untile_rows, dim3((unsigned)((have * g->dp4 + kBlock - 1) / kBlock)), dim3(kBlock), 0, g->stream, (const float4*)g->gal4, g->dp4, g->d,
                           row0 + r0, have, (float*)g->dq);
        FIR_HIP(hipGetLastError());
        FIR_HIP(hipMemcpyAsync(rows_out + r0 * g->d, g->dq, (size_t)have * g->d * sizeof(float), hipMemcpyDeviceToHost, g->stream));
        FIR_HIP(hipStreamSynchronize(g->stream));
    }
    if (class_out) FIR_HIP(hipMemcpyAsync(class_out, g->cls + row0, (size_t)m * sizeof(int32_t), hipMemcpyDeviceToHost, g->stream));
    FIR_HIP(hipStreamSynchronize(g->stream));
    call.done();
    return FIR_OK;
}

int fir_gallery_padding_words_(fir_gallery* g, int64_t* words) {
    if (!g || !words) return fir_fail_(FIR_ERR_ARG, "NULL argument");
    *words = 0;
    if (g->cap_tiles == 0) return FIR_OK;
    FIR_HIP(hipSetDevice(g->device));
    void* p = nullptr;
    int rc = fir_gallery_scratch_(g, 23, 16, &p);            // (the label range's two words are entered afresh by every use; words 2 and 3 are this counter)
    if (rc) return rc;
    GalleryCall call(g);
    if (call.rc) return call.rc;
    unsigned long long* cnt = (unsigned long long*)p + 1;
    unsigned long long h = 0;
    FIR_HIP(hipMemsetAsync(cnt, 0, sizeof h, g->stream));
    hipLaunchKernelGGL(k_count_padding, dim3((unsigned)((g->cap_tiles * g->dp4 * 64 + kBlock - 1) / kBlock)), dim3(kBlock), 0, g->stream, (const float4*)g->gal4,
                       g->n, g->cap_tiles, g->d, g->dp4, cnt);
    FIR_HIP(hipGetLastError());
    FIR_HIP(hipMemcpyAsync(&h, cnt, sizeof h, hipMemcpyDeviceToHost, g->stream));
    FIR_HIP(hipStreamSynchronize(g->stream));
    call.done();
    *words = (int64_t)h;
    return FIR_OK;
}

int fir_feature_distance(const float* lhs, const float* rhs, int32_t len, int32_t start_pos, int32_t end_pos,
                         int32_t metric, int32_t device, float* out) {
    if (!lhs || !rhs || !out) return fir_fail_(FIR_ERR_ARG, "NULL argument");
    if (start_pos < 0 || end_pos > len || start_pos >= end_pos) return fir_fail_(FIR_ERR_ARG, "bad range [%d,%d) of %d", start_pos, end_pos, len);
    if (metric < 0 || metric > 2) return fir_fail_(FIR_ERR_ARG, "bad metric %d", metric);
    int rc = set_device(device);
    if (rc) return rc;
    GalleryBuf<float> buf;                                 // both vectors and the result; gone when this function returns
    if ((rc = FIR_RESERVE(buf, (size_t)(2 * len + 1) * sizeof(float)))) return rc;
    hipError_t e = hipMemcpy(buf, lhs, (size_t)len * sizeof(float), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(buf + len, rhs, (size_t)len * sizeof(float), hipMemcpyHostToDevice);
    if (e == hipSuccess) {
        if (metric == 0) hipLaunchKernelGGL(k_pair_distance<0>, dim3(1), dim3(64), 0, 0, buf, buf + len, start_pos, end_pos, buf + 2 * len);
        else if (metric == 1) hipLaunchKernelGGL(k_pair_distance<1>, dim3(1), dim3(64), 0, 0, buf, buf + len, start_pos, end_pos, buf + 2 * len);
        else hipLaunchKernelGGL(k_pair_distance<2>, dim3(1), dim3(64), 0, 0, buf, buf + len, start_pos, end_pos, buf + 2 * len);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpy(out, buf + 2 * len, sizeof(float), hipMemcpyDeviceToHost);
    if (e != hipSuccess) return fir_fail_(FIR_ERR_HIP, "pair distance: %s", hipGetErrorString(e));
    return FIR_OK;
}

namespace {
// The handle's own states that were built before its most recent mutation (fir_gallery_append_dev does not wait, so it leaves them
// to the next call that wants one): freed here, which waits for the handle's calls, and rebuilt by that call.
void drop_stale_gemm_states(fir_gallery* g) {
    if (g->gemm && fir_gemm_generation_(g->gemm) != g->generation) { fir_gemm_destroy(g->gemm); g->gemm = nullptr; }
    for (auto& ps : g->gemm_prefix)
        if (ps.m && fir_gemm_generation_(ps.m) != g->generation) { fir_gemm_destroy(ps.m); ps.m = nullptr; ps.end = 0; }
}
// 0 = *m is the handle's fir_gemm for features [0, end), 1 = this shape stays with the scan, < 0 = error
int ensure_gemm(fir_gallery* g, int32_t end, fir_gemm** m, int* warm = nullptr, int warm_calls = 0) {
    // warm / warm_calls (automatic dispatch of cases that save tens to hundreds of microseconds per call: cache-resident galleries,
    // one-query calls): the state -- an fp16 copy, scratch, and the first time in a process ~12 ms of kernel loading -- is only built for
    // a gallery that keeps getting such calls; the first warm_calls of them take the scan (a test harness that makes ONE batched call
    // against a 3 030-row gallery would pay 16 ms to save 2)
    const bool whole = end == g->d;
    drop_stale_gemm_states(g);
    if (g->shadow_mode == FIR_SHADOW_NONE && g->large_batch_min <= 0) return 1;     // the caller forbade every copy: the scan
    fir_gallery::PrefixSlot* ps = nullptr;
    if (!whole) {
        for (auto& c : g->gemm_prefix) if (c.m && c.end == end) ps = &c;
        if (!ps) {                                                  // the free slot, else the one used longest ago
            ps = &g->gemm_prefix[0];
            for (auto& c : g->gemm_prefix) if (!c.m) { ps = &c; break; } else if (c.used < ps->used) ps = &c;
        }
    }
    fir_gemm*& slot = whole ? g->gemm : ps->m;
    const bool have = slot && (whole || ps->end == end);
    if (warm && !have && g->large_batch_min < 0) {
        ++*warm;
        g->warm_left = *warm <= warm_calls ? warm_calls - *warm + 1 : 0;
        if (*warm <= warm_calls) return 1;
    }
    if (!whole && slot && ps->end != end) {                         // a third prefix: its fragments replace the least recently used ones
        fir_gemm_destroy(slot);
        slot = nullptr;
        ps->end = 0;
    }
    if (!slot) {
        const int rc = fir_gemm_create_range_ex_(g, FIR_GEMM_F16, whole ? 0 : end, g->shadow_mode == FIR_SHADOW_FP16 ? 0 : -1, &slot);
        if (rc) {
            slot = nullptr;
            if (g->large_batch_min > 0 || (rc != FIR_ERR_ARG && rc != FIR_ERR_NOMEM)) return rc;    // asked for explicitly, or a real failure
            g->gemm_failed = true;                                           // automatic: this shape (or this much HBM) stays with the scan
            return 1;
        }
        if (!whole) ps->end = end;
    }
    if (!whole) ps->used = ++g->prefix_clock;
    *m = slot;
    return 0;
}
// ... with the warm-up rule by gallery size: a cache-resident gallery (fewer than kAutoMfmaRows rows) gets its state with the
// fourth call that would have profited from it
int ensure_gemm_warm(fir_gallery* g, int32_t end, fir_gemm** m) {
    return g->n < kAutoMfmaRows ? ensure_gemm(g, end, m, &g->small_hits, 3) : ensure_gemm(g, end, m);
}
// The state for [0, end) (warm: by the rule above), then run(state). As ensure_gemm: 0 = done, 1 = take the scan, < 0 = error;
// in automatic mode a call that finds no room for its candidate lists (FIR_ERR_NOMEM) is left to the scan as well.
extern "C++" template <typename Run>
int run_mfma(fir_gallery* g, int32_t end, bool warm, Run run) {
    fir_gemm* m = nullptr;
    const int rc = warm ? ensure_gemm_warm(g, end, &m) : ensure_gemm(g, end, &m);
    if (rc) return rc;
    const int rcs = run(m);
    if (rcs == FIR_ERR_NOMEM && g->large_batch_min < 0) {
        (void)hipGetLastError();
        return 1;
    }
    return rcs;
}
// The matrix-core path for this call, if it applies: 0 = done, 1 = take the scan, < 0 = error.
int try_mfma(fir_gallery* g, const float* d_queries, int32_t qb, int32_t start, int32_t end, uint64_t* d_keys, hipStream_t st,
             const float* h_queries = nullptr) {
    // h_queries: the queries are still on the host and d_queries is the (writable) device buffer they are staged through
    if (!h_queries && wants_few(g, qb, start, end)) {
        fir_gemm* mf = nullptr;
        const int rcf = ensure_gemm(g, end, &mf, &g->few_hits, 16);
        if (rcf) return rcf;
        const int rcs = fir_gemm_search_few_keys_dev(mf, d_queries, qb, d_keys, st);
        if (rcs != FIR_ERR_NOMEM) return rcs;
        g->few_hits = -(1 << 30);          // no room for the proxy table: this gallery's one-query calls stay with the exact scan
        return 1;
    }
    if (!wants_mfma(g, qb, start, end)) return 1;
    return run_mfma(g, end, true, [&](fir_gemm* m) {
        // the int8 nomination (fir_gemm.hip: gemm_wants_i8_): the caller's switch; by itself only where the matrix cores were chosen
        // automatically, for the whole row, over at least kAutoMfmaRows rows
        fir_gemm_set_int8_(m, g->int8_mode > 0 ? 1 : (g->int8_mode < 0 && g->large_batch_min < 0 && end == g->d && g->n >= kAutoMfmaRows) ? -1 : 0);
        return h_queries ? fir_gemm_search_staged_(m, h_queries, (float*)d_queries, qb, 1, d_keys, st)
                         : fir_gemm_search_top1_keys_dev(m, d_queries, qb, d_keys, st);
    });
}
// ... and for every kind but top-1 (fir_search_request.h): the kind's own gate, the ranges wants_mfma admits, the state, the kind's fir_gemm entry point
constexpr int kAutoMfmaKnnMaxK = 256;
int try_mfma_search(fir_gallery* g, const float* d_queries, int32_t qb, int32_t start, int32_t end, const FirSearch& s, hipStream_t st) {
    const bool rows = s.kind == kSearchRows;                         // (the top-1 ranges, and the one kind with a warm-up)
    if (rows && s.k < 2) return 1;                                   // K = 1 callers use the top-1 entry points
    // the K nearest distinct classes of a host-pointer batch (fir_search_top_classes): the gallery needs its labels
    // (never a warm-up: the automatic rule takes galleries of kAutoMfmaRows rows or more, below that only a caller's threshold does)
    if (s.kind == kSearchClasses && !g->cls) return 1;
    // the K <= FIR_GEMM_KNN_MAX nearest rows of a host-pointer batch (fir_search_knn): the ranges and the caller's threshold of the
    // class form; by itself (kAutoMfmaQueries queries over kAutoMfmaRows rows) for 8 < K <= kAutoMfmaKnnMaxK: the largest measured K that was
    // at least 1.15 x store + select at 1 024 queries and not slower at 128, at 1M x 512 and at 100 000 x 512, together with every smaller
    // measured K (9, 16, 32, 64, 128, 256; profiles/knn_matrix_cores.txt: K = 256 is 1.56 x / 2.12 x at 128 / 1 024 queries over 1M rows and
    // 1.62 x / 5.76 x over 100 000; K = 9 9.2 x / 21 x and 3.7 x / 8.6 x). K <= 8 was not measured through this call: a caller's threshold only
    // (fir_search_topk is that call). Smaller galleries were not measured either: they stay with store + select unless the caller sets a threshold.
    if (s.kind == kSearchSelect && (s.k > FIR_GEMM_KNN_MAX || (g->large_batch_min < 0 && (s.k <= kKMax || s.k > kAutoMfmaKnnMaxK)))) return 1;
    // the rows within a radius (fir_search_radius): the ranges of the class form, max_results <= FIR_GEMM_KNN_MAX, and ONLY from a
    // caller's threshold on -- never by itself (profiles/radius_search.txt): 1.75 - 74 x store + count + select while the count fits max_results,
    // but a radius that overflows every list costs 0.09 - 0.78 x (every query answered twice) and 1 000 rows inside at 100 000 rows, 128 queries
    // 0.78 x -- far beyond the spread, and (queries, rows, max_results) do not show how many rows lie near a radius.
    if (s.is_radius() && (s.k > FIR_GEMM_KNN_MAX || g->large_batch_min <= 0)) return 1;
    if (!wants_mfma(g, qb, start, end, !rows)) return 1;
    return run_mfma(g, end, rows, [&](fir_gemm* m) {
        return rows                      ? fir_gemm_search_topk_keys_dev(m, d_queries, qb, s.k, s.keys, st)
               : s.kind == kSearchSelect ? fir_gemm_search_knn_keys_dev(m, d_queries, qb, s.k, s.keys, st)
               : s.is_radius()           ? fir_gemm_search_radius_keys_dev(m, d_queries, qb, s.radius, s.k, s.count, s.keys, st)
                                         : fir_gemm_search_top_classes_keys_dev(m, d_queries, qb, s.num_classes, s.k, s.keys, s.classes, st);
    });
}
}  // namespace

// ---- the matrix-core steps of fir_twd_conventional's batch form (fir_twd.hip; fir_internal.h has the contracts) ----
// The automatic rule (kAutoMfmaQueries queries over kAutoMfmaRows rows) for fir_twd_conventional's batch form: on. Measured against the
// launch-per-stage form of the commit before it, 7 680 classes, reduced 64, 128 .. 32 768 queries per call (profiles/twd_conventional_batch.txt):
// 230 400 x 256 1.7-24 x faster class-major and 2.5-13 x permuted; 1M x 256 1.6-3.9 x class-major (a fifth of the class lists overflow
// into the exact class scan there) and 4.5-11 x permuted, with every query reliable and with every query unreliable -- every case
// beyond the 15 % the other automatic routes ask for. Smaller galleries were not measured: a caller's threshold only.
constexpr bool kAutoMfmaTwd = true;
int fir_twd_wants_mfma_(fir_gallery* g, int32_t qb, int32_t end_pos) {
    if (!g || !g->cls) return 0;
    if (g->large_batch_min < 0 && !kAutoMfmaTwd) return 0;
    if (g->shadow_mode == FIR_SHADOW_NONE) return 0;       // the caller forbade every copy; this form needs two fp16 copies, whatever the threshold
    return wants_mfma(g, qb, 0, end_pos, true) ? 1 : 0;
}
int fir_twd_mfma_classes_(fir_gallery* g, const float* d_queries, int32_t qb, int32_t end_pos, int32_t num_classes, int32_t k, uint64_t* d_keys,
                          int32_t* d_classes, void* stream, int64_t* exact_answered) {
    if (!g || !d_queries || !exact_answered) return fir_fail_(FIR_ERR_ARG, "NULL argument");
    const hipStream_t st = stream ? (hipStream_t)stream : g->stream;
    drop_stale_gemm_states(g);      // (a state the call below would replace must not lend its total to `before`)
    // the exact-scan total of the state for [0, end_pos), before and after: the difference is this call's share (a state built by
    // this call starts from zero)
    auto state_of = [&]() -> fir_gemm* {
        if (end_pos == g->d) return g->gemm;
        for (auto& c : g->gemm_prefix) if (c.m && c.end == end_pos) return c.m;
        return nullptr;
    };
    int64_t before[3] = {0, 0, 0}, after[3] = {0, 0, 0};
    if (fir_gemm* m0 = state_of()) { const int rs = fir_gemm_stats_ex(m0, before); if (rs) return rs; }
    const int rc = try_mfma_search(g, d_queries, qb, 0, end_pos, FirSearch::distinct(num_classes, k, d_keys, d_classes), st);
    if (rc) return rc;
    if (fir_gemm* m1 = state_of()) { const int rs = fir_gemm_stats_ex(m1, after); if (rs) return rs; }
    *exact_answered = after[2] - before[2];
    return FIR_OK;
}
int fir_twd_mfma_topk_(fir_gallery* g, const float* d_queries, int32_t qb, int32_t qb_call, int32_t end_pos, int32_t k, uint64_t* d_keys, void* stream) {
    if (!g || !d_queries || !d_keys) return fir_fail_(FIR_ERR_ARG, "NULL argument");
    // the rule for these qb queries; under a caller's threshold the batch that was admitted (qb_call queries) decides for its parts too
    const bool by_call = g->large_batch_min > 0 && wants_mfma(g, qb_call, 0, end_pos);
    if (k < 2 || g->shadow_mode == FIR_SHADOW_NONE || !(by_call || wants_mfma(g, qb, 0, end_pos))) return 1;
    // (no warm-up: the batch form has made up its mind; no room for this call's candidate lists in automatic mode: the staged form answers)
    return run_mfma(g, end_pos, false, [&](fir_gemm* m) { return fir_gemm_search_topk_keys_dev(m, d_queries, qb, k, d_keys, stream ? (hipStream_t)stream : g->stream); });
}
int64_t* fir_gallery_twd_mfma_record_(fir_gallery* g) { return g->twd_mfma; }

namespace {
// out[0] = smallest label, out[1] = largest (entered with INT32_MAX, INT32_MIN)
__global__ void __launch_bounds__(kBlock) k_label_range(const int32_t* __restrict__ cls, int64_t n, int32_t* __restrict__ out) {
    int32_t lo = INT32_MAX, hi = INT32_MIN;
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += (int64_t)gridDim.x * kBlock) {
        const int32_t c = cls[i];
        lo = c < lo ? c : lo;
        hi = c > hi ? c : hi;
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        const int32_t l2 = __shfl_xor(lo, off, 64), h2 = __shfl_xor(hi, off, 64);
        lo = l2 < lo ? l2 : lo;
        hi = h2 > hi ? h2 : hi;
    }
    if ((threadIdx.x & 63) == 0) { atomicMin(&out[0], lo); atomicMax(&out[1], hi); }
}
}  // namespace

int fir_gallery_label_range_(fir_gallery* g, int32_t* lo, int32_t* hi) {
    if (!g || !lo || !hi) return fir_fail_(FIR_ERR_ARG, "NULL argument");
    if (!g->cls) return fir_fail_(FIR_ERR_STATE, "gallery was created without class labels");
    if (!g->label_known) {
        FIR_HIP(hipSetDevice(g->device));
        void* p = nullptr;
        const int rc = fir_gallery_scratch_(g, 23, 16, &p);
        if (rc) return rc;
        int32_t h[2] = {INT32_MAX, INT32_MIN};
        // (the labels may have been appended by a call on another stream: the handle's own waits for the handle's last call)
        if (g->last_stream && g->last_stream != g->stream) FIR_HIP(hipStreamWaitEvent(g->stream, g->last_done, 0));
        FIR_HIP(hipMemcpyAsync(p, h, sizeof h, hipMemcpyHostToDevice, g->stream));
        const int grid = (int)std::min<int64_t>(std::max<int64_t>((g->n + kBlock - 1) / kBlock, 1), 4 * std::max(g->cus, 1));
        hipLaunchKernelGGL(k_label_range, dim3(grid), dim3(kBlock), 0, g->stream, g->cls, g->n, (int32_t*)p);
        FIR_HIP(hipGetLastError());
        FIR_HIP(hipMemcpyAsync(h, p, sizeof h, hipMemcpyDeviceToHost, g->stream));
        FIR_HIP(hipStreamSynchronize(g->stream));
        g->label_lo = h[0];
        g->label_hi = h[1];
        g->label_known = true;
    }
    *lo = g->label_lo;
    *hi = g->label_hi;
    return FIR_OK;
}

int fir_search_topk_exact_keys_dev_(fir_gallery* g, const float* d_queries, int32_t qb, int32_t end_pos, int32_t k, uint64_t* d_keys, void* stream) {
    int32_t start_pos = 0;
    const int rc = check_search(g, d_queries, qb, start_pos, end_pos, d_keys != nullptr, [&] { return qb == 0 ? kNothingToDo : check_k(k); });
    if (rc) return rc < 0 ? rc : FIR_OK;
    GalleryCall call(g, stream);
    if (call.rc) return call.rc;
    // timed like any scan of the call, but the caller's dispatch record stays the matrix-core pass's, not this fallback's
    const fir_dispatch_info saved = g->last;
    const int rc2 = topk_dev(g, d_queries, qb, 0, end_pos, k, d_keys, call.st, true, false);
    g->last = saved;
    return rc2;
}

int fir_search_top1_keys_dev(fir_gallery* g, const float* d_queries, int32_t qb, int32_t start_pos, int32_t end_pos,
                             uint64_t* d_keys, void* stream) {
    int rc = check_search(g, d_queries, qb, start_pos, end_pos, d_keys != nullptr);
    if (rc) return rc < 0 ? rc : FIR_OK;
    GalleryCall call(g, stream);
    if (call.rc) return call.rc;
    g->call_launches = 0;
    g->warm_left = 0;
    rc = try_mfma(g, d_queries, qb, start_pos, end_pos, d_keys, call.st);
    if (rc <= 0) return rc;
    return top1_dev(g, d_queries, qb, start_pos, end_pos, d_keys, call.st);
}

// The exact streaming scan, whatever the batch size (fir_gemm.hip sends its uncertified queries here).
int fir_search_top1_exact_keys_dev_(fir_gallery* g, const float* d_queries, int32_t qb, int32_t start_pos, int32_t end_pos, uint64_t* d_keys,
                                    void* stream) {
    const int rc = check_search(g, d_queries, qb, start_pos, end_pos, d_keys != nullptr);
    if (rc) return rc < 0 ? rc : FIR_OK;
    GalleryCall call(g, stream);
    if (call.rc) return call.rc;
    return top1_dev(g, d_queries, qb, start_pos, end_pos, d_keys, call.st, kOnBehalf);
}

// Profiling hooks for the library's other translation units: an event pair around one launch on `st`.
int fir_gallery_profile_begin_(fir_gallery* g, void* st) {
    if (!g->profiling) return FIR_OK;
    if (g->ev_used + 2 > g->ev.size())
        for (int i = 0; i < 64; ++i) {
            hipEvent_t e;
            FIR_HIP(hipEventCreate(&e));
            g->ev.push_back(e);
        }
    FIR_HIP(hipEventRecord(g->ev[g->ev_used], (hipStream_t)st));
    return FIR_OK;
}
int fir_gallery_profile_end_(fir_gallery* g, void* st, double bytes_alg) {
    if (!g->profiling) return FIR_OK;
    FIR_HIP(hipEventRecord(g->ev[g->ev_used + 1], (hipStream_t)st));
    g->ev_used += 2;
    g->last_bytes = bytes_alg;
    return FIR_OK;
}
void fir_gallery_note_dispatch_(fir_gallery* g, const void* fn, const char* name, int first, int gx, int gy, int block, size_t dyn_lds, int qpp,
                                double bytes, double flops) {
    note_dispatch(g, fn, name, first ? 0 : 1, gx, gy, block, dyn_lds, qpp, bytes, flops, 1);
}

namespace {
std::mutex g_knob_mu;
std::vector<std::string> g_knobs;        // names of the set FIR_* variables the library has looked at, in order of first use
void knobs_list_(char* out, size_t cap) {
    std::lock_guard<std::mutex> lk(g_knob_mu);
    size_t used = 0;
    out[0] = 0;
    for (const std::string& k : g_knobs) {
        if (used + k.size() + 6 >= cap) { std::snprintf(out + used, cap - used, "..."); return; }
        used += (size_t)std::snprintf(out + used, cap - used, "%s%s", used ? " " : "", k.c_str());
    }
}
}  // namespace

extern "C" const char* fir_knob_(const char* name) {
    const char* v = std::getenv(name);
    if (v) {
        std::lock_guard<std::mutex> lk(g_knob_mu);
        if (std::find(g_knobs.begin(), g_knobs.end(), name) == g_knobs.end()) g_knobs.emplace_back(name);
    }
    return v;
}

int fir_gallery_last_dispatch(fir_gallery* g, fir_dispatch_info* out) {
    if (!g || !out) return fir_fail_(FIR_ERR_ARG, "NULL argument");
    if (out->struct_bytes < 8 || out->struct_bytes > (int32_t)sizeof(fir_dispatch_info)) return fir_fail_(FIR_ERR_ARG, "fir_dispatch_info.struct_bytes = %d", out->struct_bytes);
    const int32_t nb = out->struct_bytes;
    fir_dispatch_info tmp = g->last;
    tmp.warmup_calls_left = g->warm_left;
    knobs_list_(tmp.knobs, sizeof tmp.knobs);
    tmp.struct_bytes = nb;
    std::memcpy(out, &tmp, (size_t)nb);
    return FIR_OK;
}

namespace {
constexpr size_t kPinQueryBytes = 512 * 1024;    // host-pointer calls up to this many query bytes take the pinned path (a 64 x 1536 TWD batch fits)
constexpr size_t kPinKeys = 4096;                // and up to this many result keys
// ticket != 0 (single-block launches only): after the keys, host_keys[n] <- ticket -- the host spins on that word instead of
// synchronising the stream (fir_wait_ticket_)
__global__ void __launch_bounds__(kBlock) k_publish_keys(const uint64_t* __restrict__ keys, int n, uint64_t* __restrict__ host_keys,
                                                         uint64_t ticket) {
    const int i = blockIdx.x * kBlock + threadIdx.x;
    if (i < n) host_keys[i] = keys[i];
    if (ticket) {
        __threadfence_system();
        __syncthreads();
        if (threadIdx.x == 0) __hip_atomic_store(host_keys + n, ticket, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
    }
}
// One L2 query against a gallery of few tiles -- the reference's own call pattern, recognize() per test image against
// ~3 000 rows. Such a call is mostly fixed cost (three launches and a stream synchronisation next to ~20 us of kernels),
// so here it is ONE launch and no synchronisation: the scan stages the query in LDS straight from the pinned buffer (a
// one-query tile needs no transposition), its last workgroup writes the key and then a ticket to pinned host memory and
// re-arms the device key, and the host spins on the ticket (falling back to hipStreamSynchronize after 2 ms).
// 3 030 x 1536: 34 instead of 40 us per call (profiles/r01_sweep_notes.md). Returns 1 when the shape does not qualify.
int top1_one_query(fir_gallery* g, const float* pinned_query, int32_t start, int32_t end, uint64_t* pinned_key) {
    // up to 256 tiles (16 384 rows): every workgroup of this form ends on a device-wide fence before it is counted, and beyond
    // ~90 workgroups those fences cost more than the two extra launches of the general path (12 000 x 512: 25.5 against
    // 28.1 us; 24 000: 32.8 / 32.2; 50 000: 44.4 / 35.4)
    if (g->metric != kL2 || g->n <= 0 || g->tiles > 256 || g->profiling) return 1;
    const ScanKernel sk = select_scan(kEpiTop1, 1, g->metric, whole_chunks(start, end), g->dp4, /*few_tiles=*/true);
    if (!sk.fn || sk.lds_bytes == 0) return 1;       // (only the form that stages the query in LDS publishes)
    const scan_fn fn = sk.fn;
    const size_t lds_bytes = sk.lds_bytes;
    if (!g->one_keys) {
        const int rc = FIR_RESERVE(g->one_keys, 64);
        if (rc) return rc;
        g->one_done = (int32_t*)(g->one_keys + 4);
        const uint64_t init[8] = {kKeyNone, kKeyNone, kKeyNone, kKeyNone, 0, 0, 0, 0};
        FIR_HIP(hipMemcpy(g->one_keys, init, sizeof init, hipMemcpyHostToDevice));
    }
    const int max_waves = max_waves_for(g, fn, lds_bytes);
    const int waves = g->waves_req > 0 ? std::min(g->waves_req, max_waves) : pick_waves(g->tiles, max_waves, g->cus * 4);
    g->last_waves = waves;
    ScanArgs a = scan_args(g, {}, start, end, waves);
    a.qt = pinned_query;
    a.keys = g->one_keys;
    a.nq = 1;
    a.qt_stride = (int64_t)g->dp4 * 4;
    a.publish = pinned_key;
    a.done = g->one_done;
    a.ticket = ++g->one_ticket;
    hipLaunchKernelGGL(fn, dim3(waves / 4, 1), dim3(kBlock), lds_bytes, g->stream, a);
    const hipError_t le = hipGetLastError();
    if (le == hipSuccess && fir_wait_ticket_(g->stream, pinned_key + 1, a.ticket) == FIR_OK) return FIR_OK;
    // The launch failed or its last workgroup never published: only that workgroup re-arms the device key and the arrival
    // counter, so they are re-armed here (else every later one-query call would wait 2 ms and fail), and this call goes
    // through the general path. If the device itself is gone that path reports it.
    (void)hipStreamSynchronize(g->stream);
    const uint64_t init[8] = {kKeyNone, kKeyNone, kKeyNone, kKeyNone, 0, 0, 0, 0};
    (void)hipMemcpy(g->one_keys, init, sizeof init, hipMemcpyHostToDevice);
    return 1;
}

int ensure_pin(fir_gallery* g) {
    if (g->pin) return FIR_OK;
    FIR_HIP(hipHostMalloc(&g->pin, kPinQueryBytes + kPinKeys * sizeof(uint64_t), hipHostMallocDefault));
    return FIR_OK;
}
uint64_t* pin_keys(const fir_gallery* g) { return (uint64_t*)((char*)g->pin + kPinQueryBytes); }

// ---- how a host-pointer call gets its keys home: both end the call (call.done()) and unpack into idx / dist -----------------------
// Small calls: g->dkeys[0, count) published through the pinned block by a kernel; the host waits for the ticket that kernel writes
// after them when one block publishes and nobody is profiling, else for the stream.
int deliver_pinned(fir_gallery* g, GalleryCall& call, int count, int32_t* idx, float* dist) {
    uint64_t* hk = pin_keys(g);
    const uint64_t ticket = count <= kBlock && !g->profiling ? ++g->one_ticket : 0;
    hipLaunchKernelGGL(k_publish_keys, dim3((count + kBlock - 1) / kBlock), dim3(kBlock), 0, g->stream, g->dkeys, count, hk, ticket);
    FIR_HIP(hipGetLastError());
    if (ticket) {
        const int rc = fir_wait_ticket_(g->stream, hk + count, ticket);
        if (rc) return rc;
    } else FIR_HIP(hipStreamSynchronize(g->stream));
    call.done();
    return fir_keys_unpack(hk, count, idx, dist);
}
// Any call: g->dkeys[0, count) -- and g->didx[0, count) into class_out, when asked for -- copied back, one synchronisation.
int deliver_copied(fir_gallery* g, GalleryCall& call, size_t count, int32_t* class_out, int32_t* idx, float* dist) {
    std::vector<uint64_t> keys(count);
    if (count) FIR_HIP(hipMemcpyAsync(keys.data(), g->dkeys, count * sizeof(uint64_t), hipMemcpyDeviceToHost, g->stream));    // (0: a count-only radius call)
    if (class_out) FIR_HIP(hipMemcpyAsync(class_out, g->didx, count * sizeof(int32_t), hipMemcpyDeviceToHost, g->stream));
    FIR_HIP(hipStreamSynchronize(g->stream));
    call.done();
    return fir_keys_unpack(keys.data(), (int32_t)count, idx, dist);
}
}  // namespace

int fir_gallery_pin_(fir_gallery* g, void** base, size_t* query_bytes, uint64_t** results) {
    if (!g) return FIR_ERR_ARG;
    const int rc = ensure_pin(g);
    if (rc) return rc;
    *base = g->pin;
    *query_bytes = kPinQueryBytes;
    *results = pin_keys(g);
    return FIR_OK;
}
uint64_t fir_gallery_next_ticket_(fir_gallery* g) { return ++g->one_ticket; }
uint64_t fir_gallery_next_counter_(fir_gallery* g, int slot) { return g->counters[slot & 3]++; }
fir_twd_dispatch_info* fir_gallery_twd_record_(fir_gallery* g) { return &g->twd_last; }
// The one ticket wait (fir_internal.h): cheaper than hipStreamSynchronize for calls that take tens of microseconds.
int fir_wait_ticket_(hipStream_t st, volatile uint64_t* flag, uint64_t ticket) {
    const auto t0 = std::chrono::steady_clock::now();
    for (int spins = 0; __atomic_load_n(flag, __ATOMIC_ACQUIRE) != ticket; ++spins) {
        if ((spins & 1023) == 1023 && std::chrono::steady_clock::now() - t0 > std::chrono::milliseconds(2)) {
            FIR_HIP(hipStreamSynchronize(st));       // a long or failed launch: let the runtime report it
            if (__atomic_load_n(flag, __ATOMIC_ACQUIRE) != ticket) return fir_fail_(FIR_ERR_HIP, "the result ticket was not published");
            break;
        }
    }
    return FIR_OK;
}

int fir_search_top1(fir_gallery* g, const float* queries, int32_t qb, int32_t start_pos, int32_t end_pos, int32_t* idx,
                    float* dist) {
    int rc = check_search(g, queries, qb, start_pos, end_pos);
    if (rc) return rc < 0 ? rc : FIR_OK;
    GalleryCall call(g);
    if (call.rc) return call.rc;
    const bool mfma = wants_mfma(g, qb, start_pos, end_pos);
    g->call_launches = 0;
    if (!mfma && (size_t)qb * g->d * sizeof(float) <= kPinQueryBytes && (size_t)qb <= kPinKeys) {
        // small call: queries are read from, and keys written to, pinned host memory by the kernels themselves
        if ((rc = ensure_pin(g))) return rc;
        if ((rc = FIR_NEED(g->dkeys, (size_t)qb))) return rc;
        float* hq = (float*)g->pin;
        std::memcpy(hq, queries, (size_t)qb * g->d * sizeof(float));
        if (qb == 1) {
            for (int k = g->d; k < g->dp4 * 4; ++k) hq[k] = 0.0f;        // the one-query tile, zero padded
            rc = top1_one_query(g, hq, start_pos, end_pos, pin_keys(g));
            if (rc < 0) return rc;
            if (rc == FIR_OK) { call.done(); return fir_keys_unpack(pin_keys(g), 1, idx, dist); }
        }
        rc = try_mfma(g, hq, qb, start_pos, end_pos, g->dkeys, g->stream);              // (the few-query form on large galleries; else 1)
        if (rc < 0) return rc;
        if (rc > 0 && (rc = top1_dev(g, hq, qb, start_pos, end_pos, g->dkeys, g->stream))) return rc;
        return deliver_pinned(g, call, qb, idx, dist);
    }
    if ((rc = FIR_NEED(g->dq, (size_t)qb * g->d))) return rc;
    if ((rc = FIR_NEED(g->dkeys, (size_t)qb))) return rc;
    // large L2 batches go through the matrix cores (same keys, fir_gemm.hip) unless switched off; their queries are uploaded
    // super-batch by super-batch under the passes of the one before
    rc = try_mfma(g, g->dq, qb, start_pos, end_pos, g->dkeys, g->stream, queries);
    if (rc > 0) {
        FIR_HIP(hipMemcpyAsync(g->dq, queries, (size_t)qb * g->d * sizeof(float), hipMemcpyHostToDevice, g->stream));
        rc = top1_dev(g, g->dq, qb, start_pos, end_pos, g->dkeys, g->stream);
    }
    if (rc) return rc;
    return deliver_copied(g, call, (size_t)qb, nullptr, idx, dist);
}

uint64_t fir_key_pack(float dist, int32_t idx) {
    if (idx < 0) return kKeyNone;
    return key_pack(dist, (uint32_t)idx);
}

int fir_keys_unpack(const uint64_t* keys, int32_t n, int32_t* idx, float* dist) {
    if (!keys && n > 0) return fir_fail_(FIR_ERR_ARG, "keys is NULL");
    for (int32_t i = 0; i < n; ++i) {
        if (keys[i] == kKeyNone) {
            if (idx) idx[i] = -1;
            if (dist) dist[i] = kNotFound;
        } else {
            if (idx) idx[i] = (int32_t)(uint32_t)(keys[i] & 0xFFFFFFFFull);
            if (dist) dist[i] = f32_from_orderable((uint32_t)(keys[i] >> 32));
        }
    }
    return FIR_OK;
}

int fir_gallery_classes_of(fir_gallery* g, const int32_t* idx, int32_t n, int32_t* class_out) {
    if (!g || !idx || !class_out) return fir_fail_(FIR_ERR_ARG, "NULL argument");
    if (!g->cls) return fir_fail_(FIR_ERR_STATE, "gallery was created without class labels");
    if (n <= 0) return FIR_OK;
    GalleryCall call(g);
    if (call.rc) return call.rc;
    const int rc = FIR_NEED(g->didx, (size_t)2 * n);
    if (rc) return rc;
    FIR_HIP(hipMemcpyAsync(g->didx, idx, (size_t)n * sizeof(int32_t), hipMemcpyHostToDevice, g->stream));
    hipLaunchKernelGGL(k_classes_of, dim3((n + kBlock - 1) / kBlock), dim3(kBlock), 0, g->stream, g->cls, g->n, g->row_offset,
                       g->didx, n, g->didx + n);
    FIR_HIP(hipGetLastError());
    FIR_HIP(hipMemcpyAsync(class_out, g->didx + n, (size_t)n * sizeof(int32_t), hipMemcpyDeviceToHost, g->stream));
    FIR_HIP(hipStreamSynchronize(g->stream));
    return FIR_OK;
}

int fir_search_topk_keys_dev(fir_gallery* g, const float* d_queries, int32_t qb, int32_t start_pos, int32_t end_pos,
                             int32_t k, uint64_t* d_keys, void* stream) {
    const int rc = check_search(g, d_queries, qb, start_pos, end_pos, d_keys != nullptr, [&] { return check_k(k); });
    if (rc) return rc < 0 ? rc : FIR_OK;
    GalleryCall call(g, stream);
    if (call.rc) return call.rc;
    return topk_dev(g, d_queries, qb, start_pos, end_pos, k, d_keys, call.st);
}

int fir_search_topk(fir_gallery* g, const float* queries, int32_t qb, int32_t start_pos, int32_t end_pos, int32_t k,
                    int32_t* idx, float* dist) {
    int rc = check_search(g, queries, qb, start_pos, end_pos, true, [&] { return check_k(k); });
    if (rc) return rc < 0 ? rc : FIR_OK;
    GalleryCall call(g);
    if (call.rc) return call.rc;
    if ((rc = FIR_NEED(g->dkeys, (size_t)qb * k))) return rc;
    if ((size_t)qb * g->d * sizeof(float) <= kPinQueryBytes && qb * k <= kBlock && qb < 8 && !g->profiling) {
        // small call (below the candidate-list form, which synchronises by itself): pinned queries in, keys + ticket out, as in fir_search_top1
        if ((rc = ensure_pin(g))) return rc;
        float* hq = (float*)g->pin;
        std::memcpy(hq, queries, (size_t)qb * g->d * sizeof(float));
        if ((rc = topk_dev(g, hq, qb, start_pos, end_pos, k, g->dkeys, g->stream))) return rc;
        return deliver_pinned(g, call, qb * k, idx, dist);
    }
    if ((rc = FIR_NEED(g->dq, (size_t)qb * g->d))) return rc;
    // large L2 batches: the matrix cores, the queries uploaded super-batch by super-batch under the passes (as fir_search_top1;
    // here a call that finds no room for its lists fails, as it always has)
    rc = 1;
    if (k >= 2 && wants_mfma(g, qb, start_pos, end_pos)) {
        fir_gemm* m = nullptr;
        rc = ensure_gemm_warm(g, end_pos, &m);
        if (rc == 0) rc = fir_gemm_search_staged_(m, queries, g->dq, qb, k, g->dkeys, g->stream);
        if (rc < 0) return rc;
    }
    if (rc > 0) {
        FIR_HIP(hipMemcpyAsync(g->dq, queries, (size_t)qb * g->d * sizeof(float), hipMemcpyHostToDevice, g->stream));
        if ((rc = topk_dev(g, g->dq, qb, start_pos, end_pos, k, g->dkeys, g->stream, true, false))) return rc;   // (the matrix cores were consulted above)
    }
    return deliver_copied(g, call, (size_t)qb * k, nullptr, idx, dist);
}

namespace {
// The host-pointer body of fir_search_knn, fir_search_radius and fir_search_top_classes, arguments checked. `s` names the kind, K and num_classes; its device
// pointers are made here, in the handle's buffers (behind the keys' slots the counts out, then the radii in). Matrix cores, else the kind's exact form.
struct HostOut {
    int32_t* idx; float* dist; int32_t* class_out = nullptr; const float* radius = nullptr; int32_t* count = nullptr; const int32_t* exclude = nullptr;
    bool masked = false;      // a masked call: the request's mask is a HOST pointer (NULL only over an empty gallery) and the exact scan form answers
};

// ---- the nearest row of another class (fir_search_top1_other_class): the scan form -------------------------------------------
// top1_dev's passes with the kEpiTop1Other epilogue: tiles of 8, 4, 2, 1 queries (the generic scan's; a 16-query tile exists only in
// the hand-scheduled L2 kernel), all the whole tiles of one size in one launch. d_exclude[qb] is copied into the handle's scratch,
// padded to whole tiles, once per call. Nothing synchronises once the scratch is large enough.
int other_class_dev(fir_gallery* g, const float* d_queries, int32_t qb, int32_t start, int32_t end, const int32_t* d_exclude, uint64_t* d_keys,
                    hipStream_t st) {
    if (g->n == 0) {                                             // no row: FIR_KEY_NONE (all bytes 0xFF)
        FIR_HIP(hipMemsetAsync(d_keys, 0xFF, (size_t)qb * sizeof(uint64_t), st));
        return FIR_OK;
    }
    const int qpad = (qb + 15) / 16 * 16;
    int rc;
    if ((rc = FIR_NEED(g->qt, (size_t)qb * g->dp4 * 4 + 64)) || (rc = FIR_NEED(g->excl, (size_t)qpad))) return rc;
    hipLaunchKernelGGL(k_pad_exclude, dim3((qpad + kBlock - 1) / kBlock), dim3(kBlock), 0, st, d_exclude, qb, (int32_t*)g->excl, qpad);
    // chi-square / KL, automatic tuning: tiles of 4 -- the 8-query plain-range forms with this epilogue keep 249-328 vector registers in
    // scratch inside the feature loop (the 4-query forms none), and those scans are bound by the vector pipes, not by gallery reads
    const int cap = top1_qpp(g, {}, qb, std::min(effective_qpp(g), g->metric != kL2 && g->qpp == 0 ? 4 : 8));
    int q0 = 0;
    while (q0 < qb) {
        const int t = largest_pow2_le(qb - q0, cap);
        const int ny = std::min((qb - q0) / t, g->max_tiles_per_launch);
        rc = run_pass(g, st, {}, kEpiTop1Other, d_queries, q0, t, start, end, d_keys + q0, nullptr, 0, 0, nullptr, ny, /*init_keys=*/t * ny, nullptr, 0,
                      g->excl + q0);
        if (rc) return rc;
        q0 += t * ny;
    }
    return FIR_OK;
}

// The routed form of a host call's batch (and of the self-join's host calls): the nearest row of a class other than c is the best row
// of the best class other than c, and that class is rank 1 or rank 2 among all classes -- the first of
// fir_gemm_search_top_classes_keys_dev(k = 2)'s two entries whose class differs from c, FIR_KEY_NONE when neither does; the same key
// bit for bit, keys being unique and ordered by (distance, row). Routed exactly where fir_search_top_classes would route a batch of
// this size and range, and only when every label lies in [0, 16777216) (the class form's limit; num_classes = largest label + 1).
// kAutoMfmaOtherClass: it routes by itself from kAutoMfmaQueries queries over kAutoMfmaRows rows on, as the class form does: whole
// host-pointer calls of 128 / 1 024 / 8 192 queries at 100 000 x 512 and 1M x 512, 10 rows per class (profiles/other_class.txt): 3.8 / 7.7 /
// 8.7 x and 5.5 / 7.7 / 7.9 x the scan form on class-major labels, 3.1 / 4.9 / 5.3 x and 4.8 / 6.6 / 6.7 x on permuted ones, the same
// answers and no query left to the exact class scan -- every point far beyond the 15 % the automatic routes ask for. Smaller galleries
// were not measured: they stay with the scan unless the caller sets a threshold.
// 0 = queued, 1 = the scan form answers (nothing was queued), < 0 = error.
constexpr bool kAutoMfmaOtherClass = true;
int other_class_routed(fir_gallery* g, const float* d_queries, int32_t qb, int32_t start, int32_t end, const int32_t* d_exclude, uint64_t* d_keys,
                       hipStream_t st) {
    if (!g->cls || (g->large_batch_min < 0 && !kAutoMfmaOtherClass) || !wants_mfma(g, qb, start, end, true)) return 1;
    int32_t lo = 0, hi = -1;
    int rc = fir_gallery_label_range_(g, &lo, &hi);
    if (rc) return rc;
    if (lo < 0 || hi >= kClassMax) return 1;
    if ((rc = FIR_NEED(g->okeys, (size_t)2 * qb)) || (rc = FIR_NEED(g->ocls, (size_t)2 * qb))) return rc;
    rc = try_mfma_search(g, d_queries, qb, start, end, FirSearch::distinct(hi + 1, 2, g->okeys, g->ocls), st);
    if (rc) return rc;
    hipLaunchKernelGGL(k_pick_other, dim3((qb + kBlock - 1) / kBlock), dim3(kBlock), 0, st, (const uint64_t*)g->okeys, (const int32_t*)g->ocls, d_exclude, qb, d_keys);
    FIR_HIP(hipGetLastError());
    return FIR_OK;
}
// ---- the nearest row among the rows of a mask (fir_search_top1_masked): the scan form, the only one --------------------------------
// top1_dev's passes with the masked form of the generic top-1 scan: tiles of 8, 4, 2, 1 queries, all the whole tiles of one size in
// one launch. No nomination lists, no matrix cores, no hand-scheduled kernel: none of them has a masked form, and this function asks
// for none (as other_class_dev does not). Nothing synchronises once the scratch is large enough.
int masked_top1_dev(fir_gallery* g, const float* d_queries, int32_t qb, int32_t start, int32_t end, const uint64_t* d_mask, uint64_t* d_keys,
                    hipStream_t st) {
    if (g->n == 0) {                                             // no row: FIR_KEY_NONE (all bytes 0xFF); the mask is not read
        FIR_HIP(hipMemsetAsync(d_keys, 0xFF, (size_t)qb * sizeof(uint64_t), st));
        return FIR_OK;
    }
    int rc;
    if ((rc = FIR_NEED(g->qt, (size_t)qb * g->dp4 * 4 + 64))) return rc;
    // chi-square / KL, automatic tuning: tiles of 4, as other_class_dev -- the 8-query plain-range forms keep 232-318 vector registers in
    // scratch with this epilogue (their unmasked siblings 8-78, the 4-query forms none), and those scans wait for the vector pipes
    const int cap = top1_qpp(g, {}, qb, std::min(effective_qpp(g), g->metric != kL2 && g->qpp == 0 ? 4 : 8));
    int q0 = 0;
    while (q0 < qb) {
        const int t = largest_pow2_le(qb - q0, cap);
        const int ny = std::min((qb - q0) / t, g->max_tiles_per_launch);
        rc = run_pass(g, st, {}, kEpiTop1, d_queries, q0, t, start, end, d_keys + q0, nullptr, 0, 0, nullptr, ny, /*init_keys=*/t * ny, nullptr, 0, nullptr, d_mask);
        if (rc) return rc;
        q0 += t * ny;
    }
    return FIR_OK;
}
// A masked entry point's mask among its NULL checks: required unless the gallery is empty (it is then not read)
bool mask_ok(const fir_gallery* g, const void* mask) { return !g || mask != nullptr || g->n == 0; }

int search_host(fir_gallery* g, const float* queries, int32_t qb, int32_t start, int32_t end, FirSearch s, const HostOut& out) {
    GalleryCall call(g);
    if (call.rc) return call.rc;
    const size_t slots = s.key_words(qb);
    const bool classes = s.kind == kSearchClasses;
    int rc;
    const bool other = s.kind == kSearchOtherClass;
    if ((rc = FIR_NEED(g->dkeys, s.status_index(qb) + (s.radii_bytes(qb) + s.exclude_bytes(qb)) / sizeof(uint64_t))) || (rc = FIR_NEED(g->dq, (size_t)qb * g->d))) return rc;
    if (classes && (rc = FIR_NEED(g->didx, slots))) return rc;
    uint64_t* base = g->dkeys;
    s.keys = slots ? base : nullptr;
    if (classes) s.classes = g->didx;
    FIR_HIP(hipMemcpyAsync(g->dq, queries, (size_t)qb * g->d * sizeof(float), hipMemcpyHostToDevice, g->stream));
    if (s.is_radius()) {
        s.count = (int32_t*)(base + slots);
        s.radius = (const float*)(base + s.status_index(qb));
        FIR_HIP(hipMemcpyAsync((void*)s.radius, out.radius, (size_t)qb * sizeof(float), hipMemcpyHostToDevice, g->stream));
    }
    if (other) {                                                 // the excluded classes ride behind the keys as the radii do
        s.exclude = (const int32_t*)(base + s.status_index(qb));
        FIR_HIP(hipMemcpyAsync((void*)s.exclude, out.exclude, (size_t)qb * sizeof(int32_t), hipMemcpyHostToDevice, g->stream));
    }
    if (out.masked) {                                            // the mask words into the handle's scratch (an empty gallery has none)
        const uint64_t* host_mask = s.mask;
        s.mask = nullptr;
        if (g->n > 0) {
            if ((rc = FIR_NEED(g->dmask, (size_t)g->tiles))) return rc;
            FIR_HIP(hipMemcpyAsync(g->dmask, host_mask, (size_t)g->tiles * sizeof(uint64_t), hipMemcpyHostToDevice, g->stream));
            s.mask = g->dmask;
        }
    }
    g->call_launches = 0;
    g->warm_left = 0;
    // (a masked call is never routed: no matrix-core pass reads a mask)
    rc = out.masked ? 1 : other ? other_class_routed(g, g->dq, qb, start, end, s.exclude, s.keys, g->stream) : try_mfma_search(g, g->dq, qb, start, end, s, g->stream);
    if (rc > 0)
        rc = classes ? top_classes_dev(g, g->dq, qb, start, end, s.num_classes, s.k, s.keys, s.classes, g->stream, {}, 0, nullptr, s.mask)
             : other ? other_class_dev(g, g->dq, qb, start, end, s.exclude, s.keys, g->stream)
             : s.kind == kSearchRows ? masked_top1_dev(g, g->dq, qb, start, end, s.mask, s.keys, g->stream)      // (only the masked top-1 call comes here as kSearchRows)
                                     : knn_dev(g, g->dq, qb, start, end, s, g->stream);
    if (rc) return rc;
    if (s.is_radius()) FIR_HIP(hipMemcpyAsync(out.count, s.count, (size_t)qb * sizeof(int32_t), hipMemcpyDeviceToHost, g->stream));
    return deliver_copied(g, call, slots, out.class_out, out.idx, out.dist);
}
// The radius calls' pointers_ok: a bad max_results is reported as such, not as a NULL argument -- the key pointer(s) are judged once it is known to be in range
bool radius_pointers_ok(int32_t qb, const float* radius, int32_t max_results, const int32_t* count, bool any_out, bool all_out) {
    return count != nullptr && (qb <= 0 || radius != nullptr) && (max_results < 0 || max_results > kKnnMax || (max_results == 0 ? !any_out : all_out));
}
}  // namespace

int fir_search_knn_keys_dev(fir_gallery* g, const float* d_queries, int32_t qb, int32_t start_pos, int32_t end_pos, int32_t k, uint64_t* d_keys,
                            void* stream) {
    const int rc = check_search(g, d_queries, qb, start_pos, end_pos, d_keys != nullptr, [&] { return check_knn_k(k); });
    if (rc) return rc < 0 ? rc : FIR_OK;
    GalleryCall call(g, stream);
    if (call.rc) return call.rc;
    return knn_dev(g, d_queries, qb, start_pos, end_pos, FirSearch::select(k, d_keys), call.st);
}

int fir_search_knn(fir_gallery* g, const float* queries, int32_t qb, int32_t start_pos, int32_t end_pos, int32_t k, int32_t* idx, float* dist) {
    const int rc = check_search(g, queries, qb, start_pos, end_pos, idx != nullptr && dist != nullptr, [&] { return check_knn_k(k); });
    if (rc) return rc < 0 ? rc : FIR_OK;
    return search_host(g, queries, qb, start_pos, end_pos, FirSearch::select(k, nullptr), {idx, dist});
}

// ---- every row within a per-query radius (fir_amd.h) ----
int fir_search_radius_keys_dev(fir_gallery* g, const float* d_queries, int32_t qb, int32_t start_pos, int32_t end_pos, const float* d_radius,
                               int32_t max_results, int32_t* d_count, uint64_t* d_keys, void* stream) {
    const bool pointers_ok = radius_pointers_ok(qb, d_radius, max_results, d_count, d_keys != nullptr, d_keys != nullptr);
    const int rc = check_search(g, d_queries, qb, start_pos, end_pos, pointers_ok, [&] { return check_max_results(max_results); });
    if (rc) return rc < 0 ? rc : FIR_OK;
    GalleryCall call(g, stream);
    if (call.rc) return call.rc;
    return knn_dev(g, d_queries, qb, start_pos, end_pos, FirSearch::within(d_radius, max_results, d_count, d_keys), call.st);
}

int fir_search_radius(fir_gallery* g, const float* queries, int32_t qb, int32_t start_pos, int32_t end_pos, const float* radius, int32_t max_results,
                      int32_t* count, int32_t* idx, float* dist) {
    const bool pointers_ok = radius_pointers_ok(qb, radius, max_results, count, idx || dist, idx && dist);
    const int rc = check_search(g, queries, qb, start_pos, end_pos, pointers_ok, [&] { return check_max_results(max_results); });
    if (rc) return rc < 0 ? rc : FIR_OK;
    return search_host(g, queries, qb, start_pos, end_pos, FirSearch::within(nullptr, max_results, nullptr, nullptr), {idx, dist, nullptr, radius, count});
}

namespace {
// check_search for the class searches: k, num_classes and the labels in its `extra` place -- and the range too, which these entry
// points have always checked before they look at qb == 0.
int check_top_classes(const fir_gallery* g, const float* queries, int32_t qb, int32_t& start_pos, int32_t& end_pos, int32_t num_classes, int32_t k,
                      bool pointers_ok = true) {
    return check_search(g, queries, qb, start_pos, end_pos, pointers_ok, [&] {
        if (k < 1 || k > 32) return fir_fail_(FIR_ERR_ARG, "k=%d outside [1,32]", k);
        if (num_classes < 1 || num_classes > kClassMax) return fir_fail_(FIR_ERR_ARG, "num_classes=%d outside [1,%d]", num_classes, kClassMax);
        if (!g->cls && g->n > 0) return fir_fail_(FIR_ERR_STATE, "gallery was created without class labels");      // (an empty gallery keeps none)
        return check_range(g, start_pos, end_pos);
    });
}
}  // namespace

int fir_search_top_classes_keys_dev(fir_gallery* g, const float* d_queries, int32_t qb, int32_t start_pos, int32_t end_pos, int32_t num_classes,
                                    int32_t k, uint64_t* d_keys, int32_t* d_classes, void* stream) {
    const int rc = check_top_classes(g, d_queries, qb, start_pos, end_pos, num_classes, k);
    if (rc < 0) return rc;
    if (qb > 0 && !d_keys && !d_classes) return fir_fail_(FIR_ERR_ARG, "d_keys and d_classes are both NULL");
    if (rc) return FIR_OK;
    GalleryCall call(g, stream);
    if (call.rc) return call.rc;
    g->call_launches = 0;
    g->warm_left = 0;
    return top_classes_dev(g, d_queries, qb, start_pos, end_pos, num_classes, k, d_keys, d_classes, call.st);
}

// The class-minimum scan on behalf of fir_gemm_search_top_classes_keys_dev, neither recorded nor timed (fir_internal.h).
int fir_class_scan_dev_(fir_gallery* g, const float* d_queries, int32_t qb, int32_t end_pos, int32_t num_classes, int32_t k, int64_t sample_rows,
                        uint64_t* d_keys, int32_t* d_classes, float* d_bound, void* stream) {
    int32_t start_pos = 0;
    const int rc = check_top_classes(g, d_queries, qb, start_pos, end_pos, num_classes, k);
    if (rc < 0) return rc;
    if (sample_rows > 0 ? !d_bound : (!d_keys && !d_classes)) return fir_fail_(FIR_ERR_ARG, "NULL argument");
    if (rc) return FIR_OK;
    GalleryCall call(g, stream);
    if (call.rc) return call.rc;
    return top_classes_dev(g, d_queries, qb, 0, end_pos, num_classes, k, d_keys, d_classes, call.st, kOnBehalf, (sample_rows + kTileRows - 1) / kTileRows, d_bound);
}

// The sample bound of fir_gemm_search_knn_keys_dev (fir_internal.h), neither recorded nor timed.
int fir_knn_sample_bound_dev_(fir_gallery* g, const float* d_queries, int32_t qb, int32_t end_pos, int32_t k, int32_t sample_div, float* d_bound,
                              void* stream) {
    int32_t start_pos = 0;
    const int rc = check_search(g, d_queries, qb, start_pos, end_pos, d_bound != nullptr, [&] { return check_knn_k(k); });
    if (rc) return rc < 0 ? rc : FIR_OK;
    if (g->metric != FIR_METRIC_L2) return fir_fail_(FIR_ERR_ARG, "the sample bound is an L2 distance");
    GalleryCall call(g, stream);
    if (call.rc) return call.rc;
    return knn_sample_bound_dev(g, d_queries, qb, end_pos, k, sample_div, d_bound, call.st);
}

int fir_search_top_classes(fir_gallery* g, const float* queries, int32_t qb, int32_t start_pos, int32_t end_pos, int32_t num_classes, int32_t k,
                           int32_t* class_out, int32_t* idx, float* dist) {
    int rc = check_top_classes(g, queries, qb, start_pos, end_pos, num_classes, k);
    if (rc) return rc < 0 ? rc : FIR_OK;
    return search_host(g, queries, qb, start_pos, end_pos, FirSearch::distinct(num_classes, k, nullptr, nullptr), {idx, dist, class_out});
}

// ---- the nearest row of another class, the gallery's self-join over it, the false-accept threshold (fir_amd.h) ----
namespace {
// check_search in fir_search_top_classes' order: NULL, qb < 0, the labels, the range, then qb == 0
int check_other_class(const fir_gallery* g, const void* queries, int32_t qb, int32_t& start_pos, int32_t& end_pos, bool pointers_ok) {
    return check_search(g, queries, qb, start_pos, end_pos, pointers_ok, [&] {
        if (!g->cls) return fir_fail_(FIR_ERR_STATE, "gallery was created without class labels");
        return check_range(g, start_pos, end_pos);
    });
}
constexpr int64_t kSelfJoinBlock = 8192;      // gallery rows per self-join block: one call of the search with that many queries
// Rows [row0, row0 + m) (m <= kSelfJoinBlock) as queries with their own classes excluded: un-tiled into g->selfq (the tiled f32 rows
// are the one copy every gallery has), then the search -- routed where a host call's batch would be, when the caller is a host call.
int self_join_block(fir_gallery* g, int64_t row0, int32_t m, int32_t start, int32_t end, uint64_t* d_keys, hipStream_t st, bool may_route) {
    int rc = FIR_NEED(g->selfq, (size_t)m * g->d);
    if (rc) return rc;
    const int64_t chunks = (int64_t)m * g->dp4;
    hipLaunchKernelGGL(k_untile_rows, dim3((unsigned)((chunks + kBlock - 1) / kBlock)), dim3(kBlock), 0, st, (const float4*)g->gal4, g->dp4, g->d, row0, (int64_t)m,
                       (float*)g->selfq);
    FIR_HIP(hipGetLastError());
    if (may_route) {
        rc = other_class_routed(g, g->selfq, m, start, end, g->cls + row0, d_keys, st);
        if (rc <= 0) return rc;
    }
    return other_class_dev(g, g->selfq, m, start, end, g->cls + row0, d_keys, st);
}
int check_self_join(const fir_gallery* g, int32_t& start_pos, int32_t& end_pos, bool pointers_ok) {
    if (!g || !pointers_ok) return fir_fail_(FIR_ERR_ARG, "NULL argument");
    if (!g->cls) return fir_fail_(FIR_ERR_STATE, "gallery was created without class labels");
    return check_range(g, start_pos, end_pos);
}
}  // namespace

int fir_search_top1_other_class_keys_dev(fir_gallery* g, const float* d_queries, int32_t qb, int32_t start_pos, int32_t end_pos,
                                         const int32_t* d_exclude_class, uint64_t* d_keys, void* stream) {
    const int rc = check_other_class(g, d_queries, qb, start_pos, end_pos, d_keys != nullptr && (qb <= 0 || d_exclude_class != nullptr));
    if (rc) return rc < 0 ? rc : FIR_OK;
    GalleryCall call(g, stream);
    if (call.rc) return call.rc;
    g->call_launches = 0;
    g->warm_left = 0;
    return other_class_dev(g, d_queries, qb, start_pos, end_pos, d_exclude_class, d_keys, call.st);
}

int fir_search_top1_other_class(fir_gallery* g, const float* queries, int32_t qb, int32_t start_pos, int32_t end_pos, const int32_t* exclude_class,
                                int32_t* idx, float* dist) {
    const int rc = check_other_class(g, queries, qb, start_pos, end_pos, idx != nullptr && dist != nullptr && (qb <= 0 || exclude_class != nullptr));
    if (rc) return rc < 0 ? rc : FIR_OK;
    HostOut out{idx, dist};
    out.exclude = exclude_class;
    return search_host(g, queries, qb, start_pos, end_pos, FirSearch::other_class(nullptr, nullptr), out);
}

// ---- searches over a subset of the rows (fir_amd.h): each the unmasked sibling's checks with the mask among the NULL checks, then the
// exact scan form of its kind with the mask -- no route is consulted ----
int fir_search_top1_masked_keys_dev(fir_gallery* g, const float* d_queries, int32_t qb, int32_t start_pos, int32_t end_pos, const uint64_t* d_mask,
                                    uint64_t* d_keys, void* stream) {
    const int rc = check_search(g, d_queries, qb, start_pos, end_pos, d_keys != nullptr && mask_ok(g, d_mask));
    if (rc) return rc < 0 ? rc : FIR_OK;
    GalleryCall call(g, stream);
    if (call.rc) return call.rc;
    g->call_launches = 0;
    g->warm_left = 0;
    return masked_top1_dev(g, d_queries, qb, start_pos, end_pos, d_mask, d_keys, call.st);
}

int fir_search_top1_masked(fir_gallery* g, const float* queries, int32_t qb, int32_t start_pos, int32_t end_pos, const uint64_t* mask, int32_t* idx,
                           float* dist) {
    const int rc = check_search(g, queries, qb, start_pos, end_pos, mask_ok(g, mask));
    if (rc) return rc < 0 ? rc : FIR_OK;
    HostOut out{idx, dist};
    out.masked = true;
    return search_host(g, queries, qb, start_pos, end_pos, FirSearch::rows(1, nullptr).masked(mask), out);
}

int fir_search_knn_masked_keys_dev(fir_gallery* g, const float* d_queries, int32_t qb, int32_t start_pos, int32_t end_pos, const uint64_t* d_mask,
                                   int32_t k, uint64_t* d_keys, void* stream) {
    const int rc = check_search(g, d_queries, qb, start_pos, end_pos, d_keys != nullptr && mask_ok(g, d_mask), [&] { return check_knn_k(k); });
    if (rc) return rc < 0 ? rc : FIR_OK;
    GalleryCall call(g, stream);
    if (call.rc) return call.rc;
    return knn_dev(g, d_queries, qb, start_pos, end_pos, FirSearch::select(k, d_keys).masked(g->n > 0 ? d_mask : nullptr), call.st);
}

int fir_search_knn_masked(fir_gallery* g, const float* queries, int32_t qb, int32_t start_pos, int32_t end_pos, const uint64_t* mask, int32_t k,
                          int32_t* idx, float* dist) {
    const int rc = check_search(g, queries, qb, start_pos, end_pos, idx != nullptr && dist != nullptr && mask_ok(g, mask), [&] { return check_knn_k(k); });
    if (rc) return rc < 0 ? rc : FIR_OK;
    HostOut out{idx, dist};
    out.masked = true;
    return search_host(g, queries, qb, start_pos, end_pos, FirSearch::select(k, nullptr).masked(mask), out);
}

int fir_search_radius_masked_keys_dev(fir_gallery* g, const float* d_queries, int32_t qb, int32_t start_pos, int32_t end_pos, const uint64_t* d_mask,
                                      const float* d_radius, int32_t max_results, int32_t* d_count, uint64_t* d_keys, void* stream) {
    const bool pointers_ok = radius_pointers_ok(qb, d_radius, max_results, d_count, d_keys != nullptr, d_keys != nullptr) && mask_ok(g, d_mask);
    const int rc = check_search(g, d_queries, qb, start_pos, end_pos, pointers_ok, [&] { return check_max_results(max_results); });
    if (rc) return rc < 0 ? rc : FIR_OK;
    GalleryCall call(g, stream);
    if (call.rc) return call.rc;
    return knn_dev(g, d_queries, qb, start_pos, end_pos, FirSearch::within(d_radius, max_results, d_count, d_keys).masked(g->n > 0 ? d_mask : nullptr), call.st);
}

int fir_search_radius_masked(fir_gallery* g, const float* queries, int32_t qb, int32_t start_pos, int32_t end_pos, const uint64_t* mask,
                             const float* radius, int32_t max_results, int32_t* count, int32_t* idx, float* dist) {
    const bool pointers_ok = radius_pointers_ok(qb, radius, max_results, count, idx || dist, idx && dist) && mask_ok(g, mask);
    const int rc = check_search(g, queries, qb, start_pos, end_pos, pointers_ok, [&] { return check_max_results(max_results); });
    if (rc) return rc < 0 ? rc : FIR_OK;
    HostOut out{idx, dist, nullptr, radius, count};
    out.masked = true;
    return search_host(g, queries, qb, start_pos, end_pos, FirSearch::within(nullptr, max_results, nullptr, nullptr).masked(mask), out);
}

int fir_search_top_classes_masked_keys_dev(fir_gallery* g, const float* d_queries, int32_t qb, int32_t start_pos, int32_t end_pos, const uint64_t* d_mask,
                                           int32_t num_classes, int32_t k, uint64_t* d_keys, int32_t* d_classes, void* stream) {
    const int rc = check_top_classes(g, d_queries, qb, start_pos, end_pos, num_classes, k, mask_ok(g, d_mask));
    if (rc < 0) return rc;
    if (qb > 0 && !d_keys && !d_classes) return fir_fail_(FIR_ERR_ARG, "d_keys and d_classes are both NULL");
    if (rc) return FIR_OK;
    GalleryCall call(g, stream);
    if (call.rc) return call.rc;
    g->call_launches = 0;
    g->warm_left = 0;
    return top_classes_dev(g, d_queries, qb, start_pos, end_pos, num_classes, k, d_keys, d_classes, call.st, {}, 0, nullptr, g->n > 0 ? d_mask : nullptr);
}

int fir_search_top_classes_masked(fir_gallery* g, const float* queries, int32_t qb, int32_t start_pos, int32_t end_pos, const uint64_t* mask,
                                  int32_t num_classes, int32_t k, int32_t* class_out, int32_t* idx, float* dist) {
    const int rc = check_top_classes(g, queries, qb, start_pos, end_pos, num_classes, k, mask_ok(g, mask));
    if (rc) return rc < 0 ? rc : FIR_OK;
    HostOut out{idx, dist, class_out};
    out.masked = true;
    return search_host(g, queries, qb, start_pos, end_pos, FirSearch::distinct(num_classes, k, nullptr, nullptr).masked(mask), out);
}

namespace {
// The builders' checks, device and host form alike: 0 = go on, kNothingToDo = an empty gallery (no word to write), < 0 = the error
int check_mask_of_classes(const fir_gallery* g, const int32_t* classes, int32_t m, const uint64_t* mask_out) {
    if (!g || (m > 0 && !classes) || (!mask_out && g->n > 0)) return fir_fail_(FIR_ERR_ARG, "NULL argument");
    if (m < 0) return fir_fail_(FIR_ERR_ARG, "m < 0");
    if (!g->cls && g->n > 0) return fir_fail_(FIR_ERR_STATE, "gallery was created without class labels");      // (an empty gallery keeps none)
    return g->n == 0 ? kNothingToDo : FIR_OK;
}
int mask_of_classes_launch(fir_gallery* g, const int32_t* d_classes, int32_t m, int32_t invert, uint64_t* d_mask_out, hipStream_t st) {
    hipLaunchKernelGGL(k_mask_of_classes, dim3((unsigned)((g->tiles + kBlock / 64 - 1) / (kBlock / 64))), dim3(kBlock), 0, st, (const int32_t*)g->cls, g->n, g->tiles,
                       d_classes, m, invert, d_mask_out);
    FIR_HIP(hipGetLastError());
    return FIR_OK;
}
}  // namespace

int fir_gallery_mask_of_classes_dev(fir_gallery* g, const int32_t* d_classes, int32_t m, int32_t invert, uint64_t* d_mask_out, void* stream) {
    const int rc = check_mask_of_classes(g, d_classes, m, d_mask_out);
    if (rc) return rc < 0 ? rc : FIR_OK;
    GalleryCall call(g, stream);
    if (call.rc) return call.rc;
    return mask_of_classes_launch(g, d_classes, m, invert, d_mask_out, call.st);
}

int fir_gallery_mask_of_classes(fir_gallery* g, const int32_t* classes, int32_t m, int32_t invert, uint64_t* mask_out) {
    int rc = check_mask_of_classes(g, classes, m, mask_out);
    if (rc) return rc < 0 ? rc : FIR_OK;
    GalleryCall call(g);
    if (call.rc) return call.rc;
    std::vector<int32_t> sorted(classes, classes + m);
    std::sort(sorted.begin(), sorted.end());
    // scratch: the tile words first (8-byte aligned), the sorted list behind them
    const size_t list_words = ((size_t)m + 1) / 2;
    if ((rc = FIR_NEED(g->mclasses, (size_t)g->tiles + list_words + 1))) return rc;
    uint64_t* d_words = g->mclasses;
    int32_t* d_list = (int32_t*)(d_words + g->tiles);
    if (m > 0) FIR_HIP(hipMemcpyAsync(d_list, sorted.data(), (size_t)m * sizeof(int32_t), hipMemcpyHostToDevice, g->stream));
    if ((rc = mask_of_classes_launch(g, d_list, m, invert, d_words, g->stream))) return rc;
    FIR_HIP(hipMemcpyAsync(mask_out, d_words, (size_t)g->tiles * sizeof(uint64_t), hipMemcpyDeviceToHost, g->stream));
    FIR_HIP(hipStreamSynchronize(g->stream));
    call.done();
    return FIR_OK;
}

// ---- device-side subsets: compact by mask or row list, map back (include/fir_amd.h has the contract) --------------------------------
namespace {
// g->mseg: the total of the mask scan (one int64, two words) and the segment sums behind it
int64_t mask_segments(const fir_gallery* g) { return (FIR_MASK_WORDS(g->n) + kMaskSegWords - 1) / kMaskSegWords; }
int mseg_room(fir_gallery* g) { return FIR_NEED(g->mseg, (size_t)mask_segments(g) + 2); }
int64_t* mseg_total(const fir_gallery* g) { return (int64_t*)(int32_t*)g->mseg; }
// The first two launches of mask -> row list on `st`: the segment sums become their exclusive prefix sums, the total goes to
// mseg_total(g) and to d_count (may be NULL). n == 0: the scan alone, which writes 0.
int mask_count_launch(fir_gallery* g, const uint64_t* d_mask, int64_t* d_count, hipStream_t st) {
    const int64_t words = FIR_MASK_WORDS(g->n), nseg = mask_segments(g);
    int32_t* seg = g->mseg + 2;
    if (nseg > 0)
        hipLaunchKernelGGL(k_mask_seg_counts, dim3((unsigned)((nseg + kBlock / 64 - 1) / (kBlock / 64))), dim3(kBlock), 0, st, d_mask, g->n, words, seg);
    hipLaunchKernelGGL(k_mask_seg_scan, dim3(1), dim3(kBlock), 0, st, seg, nseg, mseg_total(g), d_count);
    FIR_HIP(hipGetLastError());
    return FIR_OK;
}
// ... and the third: d_rows_out[0, min(count, cap)) = the selected rows, ascending
int mask_rows_launch(fir_gallery* g, const uint64_t* d_mask, int32_t* d_rows_out, int64_t cap, hipStream_t st) {
    const int64_t nseg = mask_segments(g);
    if (nseg == 0 || cap <= 0) return FIR_OK;
    hipLaunchKernelGGL(k_mask_rows, dim3((unsigned)((nseg + kBlock / 64 - 1) / (kBlock / 64))), dim3(kBlock), 0, st, d_mask, g->n, (int64_t)FIR_MASK_WORDS(g->n),
                       (const int32_t*)(g->mseg + 2), d_rows_out, cap);
    FIR_HIP(hipGetLastError());
    return FIR_OK;
}
int check_rows_of_mask(const fir_gallery* g, const void* mask, const void* rows_out, int64_t cap, const void* count) {
    if (!g || !count || !mask_ok(g, mask) || (cap > 0 && !rows_out)) return fir_fail_(FIR_ERR_ARG, "NULL argument");
    if (cap < 0) return fir_fail_(FIR_ERR_ARG, "cap < 0");
    return FIR_OK;
}

// A fresh handle for m rows of src, labelled iff src is (and m > 0), with room for its row list. Nothing is queued.
int subset_alloc(fir_gallery* src, int64_t m, fir_gallery** out) {
    fir_gallery* g = nullptr;
    int rc = gallery_alloc(m, src->d, src->metric, src->device, &g);
    if (rc) return rc;
    hipError_t e = hipSuccess;
    if (m > 0) e = g->origin.reserve((size_t)m * sizeof(int32_t));
    if (e == hipSuccess && m > 0 && src->cls) e = labels_alloc(g);
    if (e != hipSuccess) {
        delete g;
        return fir_fail_(e == hipErrorOutOfMemory ? FIR_ERR_NOMEM : FIR_ERR_HIP, "hipMalloc of a subset's row list and labels: %s", hipGetErrorString(e));
    }
    g->is_subset = g->origin_ok = true;
    g->origin_n = m;
    g->origin_offset = src->row_offset;
    *out = g;
    return FIR_OK;
}
// Rows d_idx[0, g->n) of src into every tile of g, on `st`; own_list: d_idx is g->origin itself (else the kernel fills it in).
// Slabs of whole tiles keep the launch grid inside 2^31 blocks, as in fir_gallery_create_dev.
int gather_tiles_launch(fir_gallery* src, fir_gallery* g, const int32_t* d_idx, bool own_list, hipStream_t st) {
    const int64_t slab = std::max<int64_t>(1, ((int64_t)1 << 30) / ((int64_t)g->dp4 * 4) / kTileRows);      // tiles
    for (int64_t t0 = 0; t0 < g->tiles; t0 += slab) {
        const int64_t tiles = std::min(slab, g->tiles - t0);
        const int64_t blocks = (tiles * g->dp4 * 64 + kBlock - 1) / kBlock;
        hipLaunchKernelGGL(k_gather_tiles, dim3((unsigned)blocks), dim3(kBlock), 0, st, (const float4*)src->gal4, src->n, g->dp4, d_idx, g->n, t0, tiles,
                           (float4*)g->gal4, (int32_t*)g->range, (const int32_t*)src->cls, (int32_t*)g->cls, own_list ? (int32_t*)nullptr : (int32_t*)g->origin);
        FIR_HIP(hipGetLastError());
    }
    return FIR_OK;
}
// fir_gallery_create_from_rows[_dev] after the checks: the list is in host memory (checked) or in device memory.
int subset_from_list(fir_gallery* src, const int32_t* row_idx, int64_t m, bool host_list, void* stream, fir_gallery** out) {
    FIR_HIP(hipSetDevice(src->device));
    fir_gallery* g = nullptr;
    int rc = subset_alloc(src, m, &g);
    if (rc) return rc;
    if (m == 0) { *out = g; return FIR_OK; }
    GalleryCall call(src, stream);                         // a call on the SOURCE: after its queued appends, before its later mutations
    if (call.rc) { delete g; return call.rc; }
    if (host_list) {
        const hipError_t e = hipMemcpyAsync(g->origin, row_idx, (size_t)m * sizeof(int32_t), hipMemcpyHostToDevice, call.st);
        if (e != hipSuccess) rc = fir_fail_(FIR_ERR_HIP, "row list upload: %s", hipGetErrorString(e));
    }
    if (rc == FIR_OK) rc = gather_tiles_launch(src, g, host_list ? (const int32_t*)g->origin : row_idx, host_list, call.st);
    rc = created_dev(g, rc, call.st, out);
    if (rc == FIR_OK) call.done();
    return rc;
}
// fir_gallery_create_subset[_dev] after the checks: d_mask is in device memory and readable on `st` (a host mask was queued there).
int subset_from_mask(fir_gallery* src, GalleryCall& call, const uint64_t* d_mask, fir_gallery** out) {
    int rc = mseg_room(src);
    if (rc) return rc;
    if ((rc = mask_count_launch(src, d_mask, nullptr, call.st))) return rc;
    int64_t m = 0;
    FIR_HIP(hipMemcpyAsync(&m, mseg_total(src), sizeof m, hipMemcpyDeviceToHost, call.st));
    FIR_HIP(hipStreamSynchronize(call.st));                // the count decides the allocation
    fir_gallery* g = nullptr;
    if ((rc = subset_alloc(src, m, &g))) return rc;
    if (m == 0) { *out = g; call.done(); return FIR_OK; }
    rc = mask_rows_launch(src, d_mask, g->origin, m, call.st);
    if (rc == FIR_OK) rc = gather_tiles_launch(src, g, g->origin, true, call.st);
    rc = created_dev(g, rc, call.st, out);
    if (rc == FIR_OK) call.done();
    return rc;
}
int check_origin(const fir_gallery* sub) {
    if (!sub->is_subset) return fir_fail_(FIR_ERR_STATE, "the gallery was not made by fir_gallery_create_subset / fir_gallery_create_from_rows: it has no origin rows");
    if (!sub->origin_ok) return fir_fail_(FIR_ERR_STATE, "the subset was changed in place (rows were appended, overwritten or removed): its origin rows no longer apply");
    return FIR_OK;
}
}  // namespace

int fir_gallery_rows_of_mask_dev(fir_gallery* g, const uint64_t* d_mask, int32_t* d_rows_out, int64_t cap, int64_t* d_count, void* stream) {
    int rc = check_rows_of_mask(g, d_mask, d_rows_out, cap, d_count);
    if (rc) return rc;
    FIR_HIP(hipSetDevice(g->device));
    if ((rc = mseg_room(g))) return rc;
    GalleryCall call(g, stream);
    if (call.rc) return call.rc;
    if ((rc = mask_count_launch(g, d_mask, d_count, call.st))) return rc;
    return mask_rows_launch(g, d_mask, d_rows_out, cap, call.st);
}

int fir_gallery_rows_of_mask(fir_gallery* g, const uint64_t* mask, int32_t* rows_out, int64_t cap, int64_t* count) {
    int rc = check_rows_of_mask(g, mask, rows_out, cap, count);
    if (rc) return rc;
    *count = 0;
    if (g->n == 0) return FIR_OK;
    FIR_HIP(hipSetDevice(g->device));
    const int64_t words = FIR_MASK_WORDS(g->n), room = std::min(cap, g->n);       // (no more than n rows can come out)
    if ((rc = mseg_room(g)) || (rc = FIR_NEED(g->dmask, (size_t)words)) || (room > 0 && (rc = FIR_NEED(g->didx, (size_t)room)))) return rc;
    GalleryCall call(g);
    if (call.rc) return call.rc;
    FIR_HIP(hipMemcpyAsync(g->dmask, mask, (size_t)words * sizeof(uint64_t), hipMemcpyHostToDevice, g->stream));
    if ((rc = mask_count_launch(g, g->dmask, nullptr, g->stream)) || (rc = mask_rows_launch(g, g->dmask, g->didx, room, g->stream))) return rc;
    int64_t total = 0;
    FIR_HIP(hipMemcpyAsync(&total, mseg_total(g), sizeof total, hipMemcpyDeviceToHost, g->stream));
    FIR_HIP(hipStreamSynchronize(g->stream));
    const int64_t have = std::min(total, room);
    if (have > 0) FIR_HIP(hipMemcpy(rows_out, g->didx, (size_t)have * sizeof(int32_t), hipMemcpyDeviceToHost));
    call.done();
    *count = total;
    return FIR_OK;
}

int fir_gallery_gather_rows_dev(fir_gallery* g, const int32_t* d_row_idx, int64_t m, float* d_rows_out, int32_t* d_class_out, void* stream) {
    if (!g || (m > 0 && (!d_row_idx || !d_rows_out))) return fir_fail_(FIR_ERR_ARG, "NULL argument");
    if (m < 0) return fir_fail_(FIR_ERR_ARG, "m < 0");
    if (m == 0) return FIR_OK;
    if (d_class_out && !g->cls && g->n > 0) return fir_fail_(FIR_ERR_STATE, "gallery was created without class labels");
    GalleryCall call(g, stream);
    if (call.rc) return call.rc;
    const int64_t slab = std::max<int64_t>(kTileRows, ((int64_t)1 << 30) / g->dp4);      // list entries per launch: the grid stays inside 2^31 blocks
    for (int64_t r0 = 0; r0 < m; r0 += slab) {
        const int64_t have = std::min(slab, m - r0);
        hipLaunchKernelGGL(k_gather_rows, dim3((unsigned)((have * g->dp4 + kBlock - 1) / kBlock)), dim3(kBlock), 0, call.st, (const float4*)g->gal4, g->n, g->dp4, g->d,
                           d_row_idx + r0, have, d_rows_out + r0 * g->d, (const int32_t*)g->cls, d_class_out ? d_class_out + r0 : (int32_t*)nullptr);
        FIR_HIP(hipGetLastError());
    }
    return FIR_OK;
}

int fir_gallery_create_from_rows_dev(fir_gallery* src, const int32_t* d_row_idx, int64_t m, void* stream, fir_gallery** out) {
    if (out) *out = nullptr;
    if (!src || !out || (m > 0 && !d_row_idx)) return fir_fail_(FIR_ERR_ARG, "NULL argument");
    if (m < 0) return fir_fail_(FIR_ERR_ARG, "m < 0");
    return subset_from_list(src, d_row_idx, m, false, stream, out);
}

int fir_gallery_create_from_rows(fir_gallery* src, const int32_t* row_idx, int64_t m, fir_gallery** out) {
    if (out) *out = nullptr;
    if (!src || !out || (m > 0 && !row_idx)) return fir_fail_(FIR_ERR_ARG, "NULL argument");
    if (m < 0) return fir_fail_(FIR_ERR_ARG, "m < 0");
    for (int64_t i = 0; i < m; ++i)                        // every index before anything is allocated
        if (row_idx[i] < 0 || row_idx[i] >= src->n)
            return fir_fail_(FIR_ERR_ARG, "row index %d (entry %lld of the list) outside [0,%lld)", row_idx[i], (long long)i, (long long)src->n);
    return subset_from_list(src, row_idx, m, true, nullptr, out);
}

int fir_gallery_create_subset_dev(fir_gallery* src, const uint64_t* d_mask, void* stream, fir_gallery** out) {
    if (out) *out = nullptr;
    if (!src || !out || !mask_ok(src, d_mask)) return fir_fail_(FIR_ERR_ARG, "NULL argument");
    FIR_HIP(hipSetDevice(src->device));
    GalleryCall call(src, stream);
    if (call.rc) return call.rc;
    return subset_from_mask(src, call, d_mask, out);
}

int fir_gallery_create_subset(fir_gallery* src, const uint64_t* mask, fir_gallery** out) {
    if (out) *out = nullptr;
    if (!src || !out || !mask_ok(src, mask)) return fir_fail_(FIR_ERR_ARG, "NULL argument");
    FIR_HIP(hipSetDevice(src->device));
    const int64_t words = FIR_MASK_WORDS(src->n);
    int rc = FIR_NEED(src->dmask, (size_t)words);
    if (rc) return rc;
    GalleryCall call(src);
    if (call.rc) return call.rc;
    if (words > 0) FIR_HIP(hipMemcpyAsync(src->dmask, mask, (size_t)words * sizeof(uint64_t), hipMemcpyHostToDevice, src->stream));
    return subset_from_mask(src, call, src->dmask, out);
}

int fir_gallery_origin_rows(fir_gallery* sub, int64_t row0, int64_t m, int32_t* rows_out) {
    if (!sub || (m > 0 && !rows_out)) return fir_fail_(FIR_ERR_ARG, "NULL argument");
    if (m < 0) return fir_fail_(FIR_ERR_ARG, "m < 0");
    const int rc = check_origin(sub);
    if (rc) return rc;
    if (row0 < 0 || row0 > sub->origin_n || m > sub->origin_n - row0)
        return fir_fail_(FIR_ERR_ARG, "rows [%lld,+%lld) outside [0,%lld)", (long long)row0, (long long)m, (long long)sub->origin_n);
    if (m == 0) return FIR_OK;
    FIR_HIP(hipSetDevice(sub->device));
    FIR_HIP(hipMemcpy(rows_out, sub->origin + row0, (size_t)m * sizeof(int32_t), hipMemcpyDeviceToHost));      // (written before creation returned)
    return FIR_OK;
}

int fir_keys_to_origin_dev(fir_gallery* sub, uint64_t* d_keys, int64_t count, void* stream) {
    if (!sub || (count > 0 && !d_keys)) return fir_fail_(FIR_ERR_ARG, "NULL argument");
    if (count < 0) return fir_fail_(FIR_ERR_ARG, "count < 0");
    const int rc = check_origin(sub);
    if (rc) return rc;
    if (count == 0) return FIR_OK;
    GalleryCall call(sub, stream);                         // after the search that wrote the keys, whatever stream it ran on
    if (call.rc) return call.rc;
    const int64_t blocks = (count + kBlock - 1) / kBlock;
    if (blocks > 0x7FFFFFFF) return fir_fail_(FIR_ERR_ARG, "count=%lld keys in one call", (long long)count);
    hipLaunchKernelGGL(k_keys_to_origin, dim3((unsigned)blocks), dim3(kBlock), 0, call.st, d_keys, count, (const int32_t*)sub->origin, sub->origin_n, sub->row_offset,
                       sub->origin_offset);
    FIR_HIP(hipGetLastError());
    return FIR_OK;
}

int fir_keys_map_rows(uint64_t* keys, int64_t count, const int32_t* row_map, int64_t m, int64_t row_add) {
    if (count < 0) return fir_fail_(FIR_ERR_ARG, "count < 0");
    if (m < 0) return fir_fail_(FIR_ERR_ARG, "m < 0");
    if ((count > 0 && !keys) || (m > 0 && !row_map)) return fir_fail_(FIR_ERR_ARG, "NULL argument");
    for (int64_t i = 0; i < count; ++i)                    // every key before anything is written
        if (keys[i] != kKeyNone && (int64_t)(uint32_t)keys[i] >= m)
            return fir_fail_(FIR_ERR_ARG, "key %lld: row %u outside [0,%lld)", (long long)i, (uint32_t)keys[i], (long long)m);
    for (int64_t i = 0; i < count; ++i)
        if (keys[i] != kKeyNone) keys[i] = (keys[i] & 0xFFFFFFFF00000000ull) | (uint64_t)(uint32_t)((int64_t)row_map[(uint32_t)keys[i]] + row_add);
    return FIR_OK;
}

int fir_gallery_other_class_keys_dev(fir_gallery* g, int64_t row0, int64_t m, int32_t start_pos, int32_t end_pos, uint64_t* d_keys, void* stream) {
    int rc = check_self_join(g, start_pos, end_pos, d_keys != nullptr);
    if (rc) return rc;
    if (row0 < 0 || m < 0 || row0 > g->n || m > g->n - row0) return fir_fail_(FIR_ERR_ARG, "rows [%lld,%lld) not inside [0,%lld)", (long long)row0, (long long)(row0 + m), (long long)g->n);
    if (m == 0) return FIR_OK;
    GalleryCall call(g, stream);
    if (call.rc) return call.rc;
    g->call_launches = 0;
    g->warm_left = 0;
    for (int64_t r = 0; r < m; r += kSelfJoinBlock)
        if ((rc = self_join_block(g, row0 + r, (int32_t)std::min(kSelfJoinBlock, m - r), start_pos, end_pos, d_keys + r, call.st, false))) return rc;
    return FIR_OK;
}

int fir_gallery_other_class(fir_gallery* g, int32_t start_pos, int32_t end_pos, int32_t* idx, float* dist) {
    int rc = check_self_join(g, start_pos, end_pos, idx != nullptr && dist != nullptr);
    if (rc) return rc;
    if (g->n == 0) return FIR_OK;
    GalleryCall call(g);
    if (call.rc) return call.rc;
    if ((rc = FIR_NEED(g->dkeys, (size_t)g->n))) return rc;
    g->call_launches = 0;
    g->warm_left = 0;
    for (int64_t r = 0; r < g->n; r += kSelfJoinBlock)
        if ((rc = self_join_block(g, r, (int32_t)std::min(kSelfJoinBlock, g->n - r), start_pos, end_pos, g->dkeys + r, g->stream, true))) return rc;
    return deliver_copied(g, call, (size_t)g->n, nullptr, idx, dist);
}

int fir_gallery_far_threshold(fir_gallery* g, int32_t start_pos, int32_t end_pos, float false_accept_rate, float* threshold, float* min_dist,
                              float* max_dist, int64_t* rows_counted) {
    int rc = check_self_join(g, start_pos, end_pos, threshold != nullptr);
    if (rc) return rc;
    if (!(false_accept_rate >= 0.0f)) return fir_fail_(FIR_ERR_ARG, "false_accept_rate=%g is negative or not a number", (double)false_accept_rate);
    if (g->n == 0) return fir_fail_(FIR_ERR_STATE, "no row has a row of another class: nothing to place a threshold over");
    GalleryCall call(g);
    if (call.rc) return call.rc;
    // the statistic as one float row (a multiple of 4 long: k_knn_sample_kth reads float4), FarStats and the threshold behind it
    const size_t n4 = ((size_t)g->n + 3) / 4 * 4;
    static_assert(sizeof(FarStats) <= 8 * sizeof(float), "the threshold sits 8 floats behind FarStats");
    if ((rc = FIR_NEED(g->fardist, n4 + 16)) || (rc = FIR_NEED(g->selfkeys, (size_t)kSelfJoinBlock))) return rc;
    float* row = g->fardist;
    FarStats* d_stats = (FarStats*)(row + n4);
    float* d_bound = row + n4 + 8;
    g->call_launches = 0;
    g->warm_left = 0;
    for (int64_t r = 0; r < g->n; r += kSelfJoinBlock) {
        const int32_t m = (int32_t)std::min(kSelfJoinBlock, g->n - r);
        if ((rc = self_join_block(g, r, m, start_pos, end_pos, g->selfkeys, g->stream, true))) return rc;
        hipLaunchKernelGGL(k_keys_to_dist, dim3((m + kBlock - 1) / kBlock), dim3(kBlock), 0, g->stream, (const uint64_t*)g->selfkeys, (int64_t)m, row + r);
    }
    hipLaunchKernelGGL(k_far_stats, dim3(1), dim3(kBlock), 0, g->stream, (const float*)row, g->n, false_accept_rate, d_stats);
    hipLaunchKernelGGL(k_knn_sample_kth, dim3(1), dim3(kBlock), 0, g->stream, (const float*)row, (int64_t)n4, g->n, 1, d_bound, (const int32_t*)&d_stats->rank);
    FIR_HIP(hipGetLastError());
    struct { FarStats st; float pad[8 - sizeof(FarStats) / sizeof(float)]; float bound; } h;
    FIR_HIP(hipMemcpyAsync(&h, d_stats, 9 * sizeof(float), hipMemcpyDeviceToHost, g->stream));
    FIR_HIP(hipStreamSynchronize(g->stream));                    // the call's one synchronisation
    call.done();
    if (rows_counted) *rows_counted = h.st.count;
    if (h.st.count == 0) return fir_fail_(FIR_ERR_STATE, "no row has a row of another class: nothing to place a threshold over");
    if (min_dist) *min_dist = h.st.min_dist;
    if (max_dist) *max_dist = h.st.max_dist;
    if (!h.st.ind_ok)
        return fir_fail_(FIR_ERR_ARG, "false_accept_rate=%g: index (int)(%lld * rate) is not below the %lld rows counted", (double)false_accept_rate,
                         (long long)h.st.count, (long long)h.st.count);
    *threshold = h.bound;
    return FIR_OK;
}

int fir_class_keys_merge(const uint64_t* keys, const int32_t* classes, int32_t parts, int32_t qb, int32_t k, uint64_t* keys_out,
                         int32_t* classes_out) {
    if (parts < 0 || qb < 0 || k < 1) return fir_fail_(FIR_ERR_ARG, "bad merge shape parts=%d qb=%d k=%d", parts, qb, k);
    if ((size_t)parts * qb > 0 && (!keys || !classes)) return fir_fail_(FIR_ERR_ARG, "NULL argument");
    if (qb > 0 && (!keys_out || !classes_out)) return fir_fail_(FIR_ERR_ARG, "NULL argument");
    std::vector<std::pair<uint64_t, int32_t>> all;
    for (int32_t q = 0; q < qb; ++q) {
        all.clear();
        for (int32_t p = 0; p < parts; ++p)
            for (int32_t r = 0; r < k; ++r) {
                const size_t i = ((size_t)p * qb + q) * k + r;
                if (keys[i] != kKeyNone) all.emplace_back(keys[i], classes[i]);
            }
        // ascending keys: a class's first entry is its smallest key, every later one of that class is dropped
        std::sort(all.begin(), all.end());
        int32_t used = 0;
        for (size_t i = 0; i < all.size() && used < k; ++i) {
            bool seen = false;
            for (int32_t j = 0; j < used; ++j) seen = seen || classes_out[(size_t)q * k + j] == all[i].second;
            if (seen) continue;
            keys_out[(size_t)q * k + used] = all[i].first;
            classes_out[(size_t)q * k + used] = all[i].second;
            ++used;
        }
        for (; used < k; ++used) { keys_out[(size_t)q * k + used] = kKeyNone; classes_out[(size_t)q * k + used] = -1; }
    }
    return FIR_OK;
}

int fir_range_distances_dev(fir_gallery* g, const float* d_queries, int32_t qb, int32_t start_pos, int32_t end_pos,
                            float* d_out, void* stream) {
    const int rc = check_search(g, d_queries, qb, start_pos, end_pos, d_out != nullptr);
    if (rc) return rc < 0 ? rc : FIR_OK;
    GalleryCall call(g, stream);
    if (call.rc) return call.rc;
    return range_dev(g, d_queries, qb, start_pos, end_pos, d_out, call.st);
}

int fir_range_distances(fir_gallery* g, const float* queries, int32_t qb, int32_t start_pos, int32_t end_pos, float* out) {
    int rc = check_search(g, queries, qb, start_pos, end_pos, out != nullptr, [&] { return g->n == 0 ? kNothingToDo : FIR_OK; });
    if (rc) return rc < 0 ? rc : FIR_OK;
    GalleryCall call(g);
    if (call.rc) return call.rc;
    if ((rc = FIR_NEED(g->dq, (size_t)qb * g->d))) return rc;
    if ((rc = FIR_NEED(g->dout, (size_t)qb * g->n))) return rc;
    FIR_HIP(hipMemcpyAsync(g->dq, queries, (size_t)qb * g->d * sizeof(float), hipMemcpyHostToDevice, g->stream));
    if ((rc = range_dev(g, g->dq, qb, start_pos, end_pos, g->dout, g->stream))) return rc;
    FIR_HIP(hipMemcpyAsync(out, g->dout, (size_t)qb * g->n * sizeof(float), hipMemcpyDeviceToHost, g->stream));
    FIR_HIP(hipStreamSynchronize(g->stream));
    return FIR_OK;
}

// Tests only (declared in fir_internal.h): the candidate-list path of fir_search_top1 / fir_search_topk for qb <= 1024 host queries
// up to the lists themselves -- list_nominate, the steps topk_lists_dev runs, on the handle's stream -- without the re-rank, which
// rewrites the nomination values in place, and without the dispatch gates (n >= 65536, qb >= 8): small galleries go through it too.
// FIR_CHI2_NOMINATION, FIR_EXACT_SAMPLES and FIR_NO_CHI2_NOMINATION are honoured as the public calls honour them. Then it
// synchronises and copies out (any output pointer may be NULL; qpad = qb rounded up to whole gallery reads, at most qb + 15):
//   info[4]      the metric the append scan ran (0 / 1 / 2 the exact ones, 5 / 6 / 7 the nomination metrics), qpad, the stride of
//                skeys, the tiles per sample group
//   counts, tau  [qpad]: rows appended per query (a count above 4096 = overflow) and the widened threshold, -inf for the padding
//   sq, rowsum   metrics 6 and 7 only: the per-query constants [qpad], the per-row constants [n] and, at rowsum[n], the largest row sum
//   skeys        [k][info[2]]: the packed (value, row) key of every sample group's nearest row
//   lists        [qpad][4096]: the packed (nomination value, row) keys, counts[q] of them (at most 4096) per query
//   flag         what the kernels raised (operands outside the plain range, a sample group without a row)
// all_rows = 1 (n <= 4096 only): the thresholds of the live queries are +inf, every row is appended.
int fir_gallery_list_nominations_(fir_gallery* g, const float* queries, int32_t qb, int32_t start_pos, int32_t end_pos, int32_t k, int32_t all_rows,
                                  int32_t* info, int32_t* counts, float* tau, float* sq, float* rowsum, uint64_t* skeys, uint64_t* lists, int32_t* flag) {
    if (!g || !queries) return fir_fail_(FIR_ERR_ARG, "NULL argument");
    if (qb < 1 || qb > 1024) return fir_fail_(FIR_ERR_ARG, "qb=%d outside [1,1024]", qb);
    if (k < 1 || k > kKMax) return fir_fail_(FIR_ERR_ARG, "k=%d outside [1,%d]", k, kKMax);
    if (g->n < 1) return fir_fail_(FIR_ERR_ARG, "empty gallery");
    if (all_rows && g->n > kListCap) return fir_fail_(FIR_ERR_ARG, "all_rows: %lld rows, a list holds %d", (long long)g->n, kListCap);
    int rc = check_range(g, start_pos, end_pos);
    if (rc) return rc;
    GalleryCall call(g);
    if (call.rc) return call.rc;
    if ((rc = FIR_NEED(g->dq, (size_t)qb * g->d))) return rc;
    FIR_HIP(hipMemcpyAsync(g->dq, queries, (size_t)qb * g->d * sizeof(float), hipMemcpyHostToDevice, g->stream));
    ListCall c{g, g->dq, qb, start_pos, end_pos, k, g->stream};
    g->call_launches = 0;
    if ((rc = list_nominate(c, all_rows != 0))) return rc;
    FIR_HIP(hipGetLastError());
    FIR_HIP(hipStreamSynchronize(g->stream));
    call.done();
    if (info) { info[0] = c.nomination_metric(); info[1] = c.qpad; info[2] = c.sample_stride; info[3] = (int32_t)c.group_tiles; }
    if (counts) FIR_HIP(hipMemcpy(counts, c.counts, (size_t)c.qpad * sizeof(int32_t), hipMemcpyDeviceToHost));
    if (tau) FIR_HIP(hipMemcpy(tau, c.tau, (size_t)c.qpad * sizeof(float), hipMemcpyDeviceToHost));
    if (sq && c.sq) FIR_HIP(hipMemcpy(sq, c.sq, (size_t)c.qpad * sizeof(float), hipMemcpyDeviceToHost));
    if (rowsum && c.sq) FIR_HIP(hipMemcpy(rowsum, g->rowsum, (size_t)(g->n + 1) * sizeof(float), hipMemcpyDeviceToHost));
    if (skeys) FIR_HIP(hipMemcpy(skeys, c.skeys, (size_t)c.sample_stride * k * sizeof(uint64_t), hipMemcpyDeviceToHost));
    if (lists) FIR_HIP(hipMemcpy(lists, c.lists, (size_t)c.qpad * kListCap * sizeof(uint64_t), hipMemcpyDeviceToHost));
    if (flag) FIR_HIP(hipMemcpy(flag, c.flag, sizeof(int32_t), hipMemcpyDeviceToHost));
    return FIR_OK;
}

int fir_profile_enable(fir_gallery* g, int32_t on) {
    if (!g) return fir_fail_(FIR_ERR_ARG, "gallery is NULL");
    g->profiling = on != 0;
    g->ev_used = 0;
    return FIR_OK;
}

int fir_profile_read(fir_gallery* g, float* ms, int32_t cap, int32_t* count, double* bytes_per_launch) {
    if (!g) return fir_fail_(FIR_ERR_ARG, "gallery is NULL");
    FIR_HIP(hipSetDevice(g->device));
    const int32_t launches = (int32_t)(g->ev_used / 2);
    for (int32_t i = 0; i < launches; ++i) {
        FIR_HIP(hipEventSynchronize(g->ev[2 * i + 1]));
        float t = 0.f;
        FIR_HIP(hipEventElapsedTime(&t, g->ev[2 * i], g->ev[2 * i + 1]));
        if (ms && i < cap) ms[i] = t;
    }
    if (count) *count = launches;
    if (bytes_per_launch) *bytes_per_launch = g->last_bytes;
    g->ev_used = 0;
    return FIR_OK;
}

int fir_gallery_sync(fir_gallery* g) {
    if (!g) return fir_fail_(FIR_ERR_ARG, "gallery is NULL");
    FIR_HIP(hipSetDevice(g->device));
    const int rc = fir_gallery_wait_calls_(g);      // the most recent call, on whatever stream it was given (and so every call before it)
    if (rc) return rc;
    FIR_HIP(hipStreamSynchronize(g->stream));
    return FIR_OK;
}

int fir_gallery_value_range(fir_gallery* g, int32_t* gallery_plain, int32_t* last_queries_plain) {
    if (!g || !gallery_plain || !last_queries_plain) return fir_fail_(FIR_ERR_ARG, "fir_gallery_value_range: null argument");
    FIR_HIP(hipSetDevice(g->device));
    int32_t h[2] = {0, 0};
    const int rc = fir_gallery_wait_calls_(g);
    if (rc) return rc;
    FIR_HIP(hipStreamSynchronize(g->stream));
    FIR_HIP(hipMemcpy(h, g->range, sizeof h, hipMemcpyDeviceToHost));
    *gallery_plain = h[0] == 0;
    *last_queries_plain = g->q_serial != 0 && h[1] != g->q_serial;
    return FIR_OK;
}

int fir_gallery_set_tuning(fir_gallery* g, int32_t queries_per_pass, int32_t waves) {
    if (!g) return fir_fail_(FIR_ERR_ARG, "gallery is NULL");
    if (queries_per_pass < 0) g->qpp = 0;   // back to automatic
    if (queries_per_pass > 0) {
        if (queries_per_pass != 1 && queries_per_pass != 2 && queries_per_pass != 4 && queries_per_pass != 8 &&
            queries_per_pass != 16)
            return fir_fail_(FIR_ERR_ARG, "queries_per_pass must be 1, 2, 4, 8 or 16");
        g->qpp = queries_per_pass;
    }
    if (waves < 0 || (waves % 4) != 0) return fir_fail_(FIR_ERR_ARG, "waves must be a non-negative multiple of 4");
    g->waves_req = waves;
    return FIR_OK;
}

int fir_gallery_get_tuning(const fir_gallery* g, int32_t* queries_per_pass, int32_t* waves, int32_t* max_waves) {
    if (!g) return fir_fail_(FIR_ERR_ARG, "gallery is NULL");
    if (queries_per_pass) *queries_per_pass = effective_qpp(g);
    if (waves) *waves = g->last_waves;   // waves of the most recent scan launch (0 before the first)
    if (max_waves) *max_waves = g->max_waves;
    return FIR_OK;
}

}  // extern "C"

#include "fir_projection.h"
