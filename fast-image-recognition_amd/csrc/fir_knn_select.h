// fir_knn_select.h -- the K smallest of many packed keys, exactly: an MSB-first radix select over 64-bit keys, then a sort of
// the K survivors. Three users: fir_search_knn (fir_capi.hip: the keys are (orderable(distance), row) over a stored distance row),
// fir_search_radius (the same with `dist < radius[q]` in the qualification, a count of the qualifying rows in front and each query's
// own rank min(count, max_results): the RADIUS forms below) and the sharded handle's merge for K > 8 (fir_shard.hip: the keys are
// the ranks' gathered keys). The digit histogram, the rank
// step and the prefix test are the ones fir_dem.hip's select (k_dem_select_one / k_dem_select_pass) has always used: they live here
// and fir_dem.hip includes them.
//
// Why it is exact under ties: the row index is the low word of the key, so no two qualifying keys are equal and "the K-th smallest
// key" T names one row however many rows share its distance. Everything <= T is selected: exactly K keys (or every qualifying key,
// when fewer than K qualify), never "the rows at or below the K-th DISTANCE", which a cut inside a run of equal distances
// overshoots. Rows that do not qualify (dist < 100000 is false: NaN included) count as FIR_KEY_NONE, the largest key, so the
// histograms always hold n entries and a rank of min(K, n) always falls inside them; they are never compacted.
//
// The first part of this file is plain C++ (no HIP): the argument check and the tile / scratch sizing of fir_search_knn, so that
// a stand-alone host program can exercise them (define FIR_KNN_HOST_ONLY before including).
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace fir {

constexpr int kKnnMax = 1024;        // FIR_KNN_MAX
constexpr int kKnnTile = 16;         // queries per select launch at most (the control block below is sized for it)
constexpr int kKnnSlice = 8192;      // keys per workgroup and digit
constexpr int kKnnMaxBlocks = 4096;  // workgroups per query at most: longer rows get longer slices

// Nonzero when 1 <= k <= kKnnMax.
inline int knn_k_ok(int32_t k) { return k >= 1 && k <= kKnnMax; }

// One tile of t queries over n rows: the distance rows (each padded to whole float4s, so every row starts 16-byte aligned), then
// the control block. All in bytes from the start of the handle's slot.
struct KnnPlan {
    int64_t row_stride;      // floats from one query's distances to the next
    size_t dist_bytes;       // t * row_stride * 4, rounded up to 256: where the control block starts
    size_t bytes;            // the whole slot
};
inline KnnPlan knn_plan(int64_t n, int t, size_t ctl_bytes) {
    KnnPlan p;
    p.row_stride = (n + 3) / 4 * 4;
    const size_t raw = (size_t)t * (size_t)p.row_stride * sizeof(float);
    p.dist_bytes = (raw + 255) / 256 * 256;
    p.bytes = p.dist_bytes + ctl_bytes;
    return p;
}
// Keys per workgroup for a row of n keys: kKnnSlice, longer (in whole 1024s, what one workgroup reads per step) when that would
// take more than max_blocks workgroups.
inline int64_t knn_slice(int64_t n, int max_blocks) {
    if (max_blocks < 1) max_blocks = 1;
    int64_t s = (n + max_blocks - 1) / max_blocks;
    s = (s + 1023) / 1024 * 1024;
    return s < kKnnSlice ? kKnnSlice : s;
}
// The largest power of two <= min(x, cap), at least 1 (queries per tile; every scan of fir_capi.hip sizes its tiles with it).
inline int largest_pow2_le(int x, int cap) {
    int p = 1;
    while (p * 2 <= x && p * 2 <= cap) p *= 2;
    return p;
}

// ---- the row sample of the matrix-core form (fir_gemm_search_knn_keys_dev, fir_gemm_knn.h) ----
// The exact K-th smallest distance over a row sample is an upper bound of the gallery's K-th distance whatever the sample is (a
// subset of the rows); only how many rows the append pass lists below it depends on the choice. R = min(n, max(kKnnSampleFloor,
// n K / div)) rows in whole 64-row tiles, taken as up to kKnnSampleRuns runs of consecutive tiles spread evenly over the gallery:
// the reference's galleries are class-major, a leading sample would know nothing of the later classes. Run i holds sample tiles
// [i run_len, (i + 1) run_len) -- the last run may be shorter -- and starts floor(i slack / nruns) tiles further up in the gallery,
// slack = the gallery's tiles outside the sample: sample tile t is gallery tile t + floor((t / run_len) slack / nruns), which is
// what the store scan computes (ScanArgs::run_len, fir_kernels.h). The runs ascend and do not overlap.
constexpr int kKnnGemmMax = 256;                        // FIR_GEMM_KNN_MAX
constexpr int kKnnSampleRuns = 16;
constexpr int64_t kKnnSampleFloor = 32768;
constexpr int kKnnSampleDiv = 1024;                     // FIR_GEMM_KNN_SAMPLE_DIV replaces it for experiments
constexpr size_t kKnnSampleBytes = (size_t)64 << 20;    // stored sample distances of one group of queries at most
struct KnnSamplePlan {
    int64_t tiles;                          // sample tiles: the runs' tiles sum to it
    int64_t rows;                           // rows of the gallery among them: the sample tiles are full except, when the last run ends with
                                            // the gallery, the last one -- only the LAST positions of a query's stored distances can be missing
    int64_t run_len;                        // tiles per run (the last run: what is left)
    int64_t slack;                          // gallery tiles outside the sample
    int nruns;
    int64_t row_stride;                     // floats from one query's stored distances to the next: tiles * 64
    int group;                              // queries whose stored distances fit `budget` bytes: at least 1, whole eights from 8 on
    int64_t run_begin(int i) const { return i * run_len + i * slack / nruns; }                              // first gallery tile of run i
    int64_t run_tiles(int i) const { return i + 1 < nruns ? run_len : tiles - (int64_t)(nruns - 1) * run_len; }
};
inline KnnSamplePlan knn_sample_plan(int64_t n, int32_t k, int div, size_t budget) {
    KnnSamplePlan p{};
    if (n < 0) n = 0;
    if (k < 1) k = 1;
    if (div < 1) div = 1;
    const int64_t gallery_tiles = (n + 63) / 64;
    int64_t want = n / div * k + n % div * k / div;       // n k / div without leaving 64 bits
    if (want < kKnnSampleFloor) want = kKnnSampleFloor;
    if (want > n) want = n;
    p.tiles = (want + 63) / 64;
    p.run_len = (p.tiles + kKnnSampleRuns - 1) / kKnnSampleRuns;
    p.nruns = p.run_len > 0 ? (int)((p.tiles + p.run_len - 1) / p.run_len) : 0;
    p.slack = gallery_tiles - p.tiles;
    p.rows = p.tiles * 64;
    if (p.nruns > 0 && p.run_begin(p.nruns - 1) + p.run_tiles(p.nruns - 1) == gallery_tiles) p.rows -= gallery_tiles * 64 - n;
    p.row_stride = p.tiles * 64;
    const size_t per_query = (size_t)(p.row_stride > 0 ? p.row_stride : 64) * sizeof(float);
    size_t group = budget / per_query;
    if (group < 1) group = 1;
    if (group > 8192) group = 8192;
    if (group >= 8) group = group / 8 * 8;
    p.group = (int)group;
    return p;
}

}  // namespace fir

#ifndef FIR_KNN_HOST_ONLY
#include <hip/hip_runtime.h>

#include "fir_common.h"

namespace fir {

static_assert(kBlock == 256, "thread t of a workgroup is bin t of the 8-bit digit histograms (hist[threadIdx.x], sel_advance)");

struct SelState { unsigned long long prefix; int32_t rank; int32_t done; };   // before a digit: key bits decided, rank inside them

__device__ __forceinline__ bool sel_match(unsigned long long key, unsigned long long prefix, int pass) {
    return pass == 0 ? true : ((key ^ prefix) >> (64 - 8 * pass)) == 0;
}

// hist[digit] += 1 for the lanes with `match`; every lane of the wave calls it. The keys of one query share their top bytes,
// so the lanes of a wave mostly hit one bin: the first two distinct digits found are counted with a ballot and added once per
// wave, whatever is left lane by lane.
__device__ __forceinline__ void hist_add(unsigned* hist, bool match, unsigned digit) {
    const int lane = threadIdx.x & 63;
    unsigned long long rem = __ballot(match);
    for (int it = 0; it < 2 && rem; ++it) {
        const int leader = __ffsll((long long)rem) - 1;
        const unsigned d0 = __shfl(digit, leader, 64);
        const unsigned long long m = __ballot(match && digit == d0);
        if (lane == leader) atomicAdd(&hist[d0], (unsigned)__popcll(m));
        rem &= ~m;
    }
    if ((rem >> lane) & 1) atomicAdd(&hist[digit], 1u);
}

// The state after digit `pass`, from the state before it and the digit's histogram (thread t holds bin t): the bin the rank falls
// into (inclusive sums folded across the wave with shuffles, across the four waves through LDS). When the rank is the bin's
// whole count, everything in the bin is selected and the remaining digits are all ones: done. All kBlock threads call it.
__device__ inline SelState sel_advance(SelState s, unsigned count, int pass, unsigned* wsum, SelState* box) {
    if (s.done) return s;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, shift = 56 - 8 * pass;
    unsigned incl = count;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const unsigned o = __shfl_up(incl, off, 64);
        if (lane >= off) incl += o;
    }
    if (lane == 63) wsum[wave] = incl;
    if (threadIdx.x == 0) *box = SelState{s.prefix, s.rank, 1};   // (a rank outside the histogram: cannot happen, and must not hang)
    __syncthreads();
    for (int w = 0; w < wave; ++w) incl += wsum[w];
    const unsigned excl = incl - count, rank = (unsigned)s.rank;
    if (count > 0 && excl < rank && rank <= incl) {
        const int all = rank - excl == count;
        unsigned long long prefix = s.prefix | ((unsigned long long)threadIdx.x << shift);
        if (all) prefix |= (1ull << shift) - 1;
        *box = SelState{prefix, (int32_t)(rank - excl), all};
    }
    __syncthreads();
    s = *box;
    __syncthreads();
    return s;
}

// ---- the K-th smallest of a row of stored distances: the sample bound of the matrix-core form ----
// One workgroup per query (k_dem_select_one's shape), one launch for all queries of a group: bound[q] = the K-th smallest of
// dist[q * stride + i], i < rows, among the distances that qualify (dist < 100000), 100000 with fewer than K of them. Only the
// distance is wanted, not the row: four digits over the 32-bit orderable distance. A digit whose bin the rank takes whole does not
// end the select (sel_advance's `done` fills the lower digits with ones: a key at or above the K-th, not the K-th itself).
// stride is a multiple of 4 and dist 16-byte aligned.
// k_dev != NULL: the rank is read from the device, k_dev[0] (fir_gallery_far_threshold: it depends on a count made on the stream before).
static __global__ void __launch_bounds__(kBlock) k_knn_sample_kth(const float* __restrict__ dist, int64_t stride, int64_t rows, int32_t k,
                                                                   float* __restrict__ bound, const int32_t* __restrict__ k_dev = nullptr) {
    __shared__ unsigned hist[256];
    __shared__ unsigned wsum[kBlock / 64];
    __shared__ SelState box;
    const int q = blockIdx.x;
    if (k_dev) k = k_dev[0];                                             // (uniform)
    if (rows < k) {                                                      // (uniform) a rank outside the histogram
        if (threadIdx.x == 0) bound[q] = kNotFound;
        return;
    }
    const float* __restrict__ row = dist + (size_t)q * stride;
    SelState s{0ull, k, 0};
    for (int pass = 0; pass < 4; ++pass) {
        const int shift = 56 - 8 * pass;
        hist[threadIdx.x] = 0;
        __syncthreads();
        for (int64_t i0 = 0; i0 < rows; i0 += 4 * kBlock) {
            const int64_t i = i0 + 4 * (int64_t)threadIdx.x;
            float4 v = {0.0f, 0.0f, 0.0f, 0.0f};
            if (i < rows) v = *(const float4*)(row + i);                 // i + 3 < stride: both are multiples of 4
            const float d4[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                const bool valid = i + c < rows;
                const uint64_t key = valid && d4[c] < kNotFound ? (uint64_t)f32_orderable(d4[c] + 0.0f) << 32 : kKeyNone;
                hist_add(hist, valid && sel_match(key, s.prefix, pass), (unsigned)(key >> shift) & 255u);
            }
        }
        __syncthreads();
        s = sel_advance(s, hist[threadIdx.x], pass, wsum, &box);
        if (s.done) { s.prefix &= ~((1ull << shift) - 1); s.done = 0; }  // the bin taken whole: its digit is decided, the rest is not
    }
    if (threadIdx.x == 0) {
        const uint32_t o = (uint32_t)(s.prefix >> 32);
        bound[q] = o == 0xFFFFFFFFu ? kNotFound : f32_from_orderable(o);
    }
}

// ---- the K smallest keys of each of nq rows of keys ----------------------------------------------------------------------------
// Several workgroups per query, one launch per digit (no device-wide barrier): launch p folds digit p-1's histogram into the state
// (every workgroup by itself, workgroup 0 keeps it), then adds its slice's digit-p histogram -- built in LDS -- to the query's.
// k_knn_compact folds the last digit, writes the keys <= T behind an integer counter (their order there is whatever the atomics
// gave; the set is not) and k_knn_sort puts each query's K keys in order in LDS: two runs give the same bytes.
struct KnnCtl {
    unsigned hist[8][kKnnTile][256];
    SelState sel[8][kKnnTile];       // [p]: the state before digit p (p >= 1; before digit 0 it is {0, rank, 0})
    int32_t count[kKnnTile];         // keys compacted so far
    int32_t inside[kKnnTile];        // radius form: the rows that qualify (k_knn_count), however many
};

// Where the keys come from. dist != NULL: a row of float32 distances per query, dist[q * stride + i], i < n: key i is
// key_pack(dist, i + row_offset) when dist < 100000, FIR_KEY_NONE otherwise (stride a multiple of 4, dist 16-byte aligned).
// dist == NULL: parts of ascending key lists, keys[p * stride + q * k_in + j], j < k_in, p < n / k_in (the sharded merge).
// The radius form (RADIUS, fir_search_radius; dist != NULL): a row qualifies only when dist < radius[q] is true as well, and the
// rank is each query's own, min(ctl->inside[q], k), read on the device: `rank` is not used.
struct KnnArgs {
    const float* dist;
    const uint64_t* keys;
    int64_t n;             // keys per query
    int64_t stride;
    int64_t row_offset;
    int64_t slice;         // keys per workgroup (a multiple of 1024)
    int32_t k_in;
    int32_t k;             // keys wanted per query
    int32_t rank;          // min(k, n)
    KnnCtl* ctl;
    uint64_t* out;         // [nq][k]
    const float* radius;   // [nq] (radius form)
    int32_t* inside;       // [nq] <- ctl->inside (radius form)
};

// f(valid, key) for every key of this workgroup's slice of query q, wave-uniformly (every lane of a wave makes every call).
template <bool DIST, bool RADIUS, typename F>
__device__ __forceinline__ void knn_slice_keys(const KnnArgs& a, int q, F f) {
    static_assert(DIST || !RADIUS, "a radius is a bound on stored distances");
    const int64_t begin = (int64_t)blockIdx.x * a.slice;
    const int64_t end = begin + a.slice < a.n ? begin + a.slice : a.n;
    if constexpr (DIST) {
        const float* __restrict__ row = a.dist + (size_t)q * a.stride;
        float radius = 0.0f;
        if constexpr (RADIUS) radius = a.radius[q];
        for (int64_t i0 = begin; i0 < end; i0 += 4 * kBlock) {
            const int64_t i = i0 + 4 * (int64_t)threadIdx.x;
            float4 v = {0.0f, 0.0f, 0.0f, 0.0f};
            if (i < end) v = *(const float4*)(row + i);                      // i + 3 < stride: both are multiples of 4
            const float d4[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                const bool valid = i + c < end;
                bool inside = valid && d4[c] < kNotFound;
                if constexpr (RADIUS) inside = inside && d4[c] < radius;      // (false for a NaN radius)
                f(valid, inside ? key_pack(d4[c], (uint32_t)(i + c + a.row_offset)) : kKeyNone);
            }
        }
    } else {
        for (int64_t i0 = begin; i0 < end; i0 += kBlock) {
            const int64_t i = i0 + threadIdx.x;
            const bool valid = i < end;
            uint64_t key = kKeyNone;
            if (valid) {
                const int64_t p = i / a.k_in, j = i - p * a.k_in;
                key = a.keys[(size_t)p * a.stride + (size_t)q * a.k_in + j];
            }
            f(valid, key);
        }
    }
}

// The state before digit `pass` (pass in 1..8), as every workgroup works it out. rank: the query's (a.rank, or a.k in the radius form).
__device__ __forceinline__ SelState knn_state(const KnnArgs& a, int q, int pass, int32_t rank, unsigned* wsum, SelState* box) {
    SelState s = pass == 1 ? SelState{0ull, rank, 0} : a.ctl->sel[pass - 1][q];
    return sel_advance(s, a.ctl->hist[pass - 1][q][threadIdx.x], pass - 1, wsum, box);
}

// Radius form: ctl->inside[q] += the rows of this workgroup's slice that qualify. k_knn_select's grid.
static __global__ void __launch_bounds__(kBlock) k_knn_count(const KnnArgs a) {
    __shared__ int wcount[kBlock / 64];
    const int q = blockIdx.y, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int mine = 0;
    knn_slice_keys<true, true>(a, q, [&](bool, uint64_t key) { mine += key != kKeyNone; });
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) mine += __shfl_down(mine, off, 64);
    if (lane == 0) wcount[wave] = mine;
    __syncthreads();
    if (threadIdx.x == 0) {
        int sum = 0;
        for (int w = 0; w < kBlock / 64; ++w) sum += wcount[w];
        if (sum) atomicAdd(&a.ctl->inside[q], sum);
    }
}

template <bool DIST, bool RADIUS>
__global__ void __launch_bounds__(kBlock) k_knn_select(const KnnArgs a, int pass) {
    __shared__ unsigned hist[256];
    __shared__ unsigned wsum[kBlock / 64];
    __shared__ SelState box;
    const int q = blockIdx.y;
    int32_t rank = a.rank;
    if constexpr (RADIUS) {
        if (a.ctl->inside[q] <= a.k) return;          // (uniform) everything that qualifies is selected: no threshold to find
        rank = a.k;
    }
    SelState s{0ull, rank, 0};
    if (pass > 0) {
        s = knn_state(a, q, pass, rank, wsum, &box);
        if (blockIdx.x == 0 && threadIdx.x == 0) a.ctl->sel[pass][q] = s;
    }
    if (s.done) return;
    hist[threadIdx.x] = 0;
    __syncthreads();
    const int shift = 56 - 8 * pass;
    knn_slice_keys<DIST, RADIUS>(a, q, [&](bool valid, uint64_t key) {
        hist_add(hist, valid && sel_match(key, s.prefix, pass), (unsigned)(key >> shift) & 255u);
    });
    __syncthreads();
    if (hist[threadIdx.x]) atomicAdd(&a.ctl->hist[pass][q][threadIdx.x], hist[threadIdx.x]);
}

template <bool DIST, bool RADIUS>
__global__ void __launch_bounds__(kBlock) k_knn_compact(const KnnArgs a) {
    __shared__ unsigned wsum[kBlock / 64];
    __shared__ SelState box;
    const int q = blockIdx.y, lane = threadIdx.x & 63;
    uint64_t T = kKeyNone;                                                // radius form, at most k rows inside: all of them
    if (!RADIUS || a.ctl->inside[q] > a.k) T = knn_state(a, q, 8, RADIUS ? a.k : a.rank, wsum, &box).prefix;
    uint64_t* __restrict__ out = a.out + (size_t)q * a.k;
    knn_slice_keys<DIST, RADIUS>(a, q, [&](bool valid, uint64_t key) {
        const bool take = valid && key <= T && key != kKeyNone;
        const unsigned long long m = __ballot(take);
        if (m == 0) return;                                               // wave-uniform
        const int leader = __ffsll((long long)m) - 1;
        int base = 0;
        if (lane == leader) base = atomicAdd(&a.ctl->count[q], (int)__popcll(m));
        base = __shfl(base, leader, 64);
        const int slot = base + (int)__popcll(m & ((1ull << lane) - 1ull));
        if (take && slot < a.k) out[slot] = key;                          // (at most rank <= k keys are <= T: the check costs nothing)
    });
}

// out[q][0..k): the count[q] compacted keys ascending, FIR_KEY_NONE behind them. One workgroup per query, bitonic in LDS.
static __global__ void __launch_bounds__(kBlock) k_knn_sort(const KnnArgs a) {
    __shared__ uint64_t s[kKnnMax];
    const int q = blockIdx.x;
    uint64_t* __restrict__ out = a.out + (size_t)q * a.k;
    const int cnt = min(a.ctl->count[q], a.k);
    int P = 2;
    while (P < a.k) P *= 2;
    for (int i = threadIdx.x; i < P; i += kBlock) s[i] = i < cnt ? out[i] : kKeyNone;
    __syncthreads();
    for (int k2 = 2; k2 <= P; k2 <<= 1)
        for (int j = k2 >> 1; j > 0; j >>= 1) {
            for (int i = threadIdx.x; i < P; i += kBlock) {
                const int o = i ^ j;
                if (o > i) {
                    const uint64_t x = s[i], y = s[o];
                    if ((x > y) == ((i & k2) == 0)) { s[i] = y; s[o] = x; }
                }
            }
            __syncthreads();
        }
    for (int i = threadIdx.x; i < a.k; i += kBlock) out[i] = s[i];
}

// Queue the select for nq <= kKnnTile queries on st: a.ctl is cleared, then eight digit launches, the compaction and the sort.
// a.n >= 1. Nothing here synchronises. max_blocks: workgroups per query at most (kKnnMaxBlocks; 1 = the one-workgroup form).
// RADIUS: the count goes first and a.inside[0..nq) receives it; a.k == 0 ends there (the count-only call).
template <bool DIST, bool RADIUS = false>
inline hipError_t knn_select_launch(KnnArgs a, int nq, int max_blocks, hipStream_t st) {
    a.slice = knn_slice(a.n, max_blocks);
    a.rank = (int32_t)(a.n < a.k ? a.n : a.k);
    const dim3 grid((unsigned)((a.n + a.slice - 1) / a.slice), (unsigned)nq);
    hipError_t e = hipMemsetAsync(a.ctl, 0, sizeof(KnnCtl), st);
    if (e != hipSuccess) return e;
    if constexpr (RADIUS) {
        hipLaunchKernelGGL(k_knn_count, grid, dim3(kBlock), 0, st, a);
        e = hipMemcpyAsync(a.inside, a.ctl->inside, (size_t)nq * sizeof(int32_t), hipMemcpyDeviceToDevice, st);
        if (e != hipSuccess) return e;
        if (a.k == 0) return hipGetLastError();
    }
    for (int pass = 0; pass < 8; ++pass) hipLaunchKernelGGL((k_knn_select<DIST, RADIUS>), grid, dim3(kBlock), 0, st, a, pass);
    hipLaunchKernelGGL((k_knn_compact<DIST, RADIUS>), grid, dim3(kBlock), 0, st, a);
    hipLaunchKernelGGL(k_knn_sort, dim3(nq), dim3(kBlock), 0, st, a);
    return hipGetLastError();
}

}  // namespace fir
#endif  // FIR_KNN_HOST_ONLY
