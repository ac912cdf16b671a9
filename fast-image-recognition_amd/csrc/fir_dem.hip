// fir_dem.hip -- the pivot table of DirectedEnumeration's constructor (qt_cpp/ann.cpp:302-331, PIVOT build) on gfx950.
//
// The reference walks its pivots one after another: a full gallery scan against pivot ii, then a choice of pivot ii+1
// as the row farthest (in summed distance) from all pivots so far. The choice depends on the scan before it, so the
// work is n_pivots dependent gallery passes of ONE query each -- HBM-bound (n*d*4 bytes per pivot), served by the
// library's range-distance kernel in the reference's arithmetic order. Everything stays on the device between
// pivots (no host round trip per pivot):
//   k_dem_gather   pivot row (tiled gallery, fir_kernels.h layout) -> dense query vector
//   range scan     table[ii][j] = distance(row j, pivot)                         (fir_range_distances_dev)
//   k_dem_step     far[j] (double, running; -1000000 restart at a pivot, :313-318), per-block partials of
//                  "first row with the largest far > 0" (:319-322) and of the minimum distance to another class (:309-311)
//   k_dem_pick     one workgroup folds the partials, writes min_other[ii] and pivots[ii+1]
// The running far[j] is the reference's inner `ind` loop evaluated incrementally: the same additions in the same order.
//
// Query time (DirectedEnumeration::recognize, ann.cpp:411-507) looks like a sequential, early-exit walk, but it is one
// selection threshold, two minima and a count: fir_dem_recognize answers a batch on the device with no host step (the kernels
// are further down, "DirectedEnumeration::recognize on the device"; the host decides a call's shape once, RecPlan, and queues
// one step per stage, kRecSteps); its tie flag marks the queries whose answer hangs on the order of equal likelihoods. The C++
// shim (host/fir_classifiers.cpp) still walks on the host over two pieces until the new call has been timed against them
// (profiles/dem_recognize.txt): fir_dem_likelihoods (k_dem_lik + k_dem_lik_fix, the stage recognize queues too: n*P*4 bytes
// of table per batch of 8 queries instead of n*d*4 bytes of gallery) and fir_rows_distances (k_rows_dist, CHECK_FOR_BEST_DIST).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <cfloat>
#include <cstring>
#include <unordered_map>
#include <vector>

#include "../../include/fir_amd.h"
#include "fir_common.h"
#include "fir_internal.h"
#include "fir_knn_select.h"

namespace {

using fir::SelState;
using fir::sel_match;
using fir::hist_add;
using fir::sel_advance;

constexpr int kBlock = 256;
static_assert(kBlock == fir::kBlock, "thread t of a workgroup is bin t of the 8-bit digit histograms (hist[threadIdx.x], sel_advance)");
constexpr int kMaxBlocks = 1024;

struct Part {       // one block's partial result
    double far;     // largest far sum > 0 seen (0 = none)
    int32_t row;    // first row that reached it, -1 = none
    float min_other;
};

// pivots[ii] -> q[0..d). A pivot of -1 (the reference's "no row has a positive far sum", which it would crash on)
// yields a zero vector; the host reports the truncation.
__global__ void __launch_bounds__(kBlock) k_dem_gather(const float4* __restrict__ gal4, int dp4, int d, const int32_t* __restrict__ pivots,
                                                       int ii, float* __restrict__ q) {
    const int piv = pivots[ii];
    for (int c = blockIdx.x * kBlock + threadIdx.x; c < dp4; c += gridDim.x * kBlock) {
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (piv >= 0) v = gal4[((size_t)(piv >> 6) * dp4 + c) * 64 + (piv & 63)];
        const float e[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (c * 4 + k < d) q[c * 4 + k] = e[k];
    }
}

// (far desc, row asc) -- row -1 compares as the largest unsigned, so "none" loses every tie
__device__ __forceinline__ bool better(double fa, int ra, double fb, int rb) { return fa > fb || (fa == fb && (unsigned)ra < (unsigned)rb); }

__device__ __forceinline__ void block_fold(double& far, int& row, float& mo, Part* red) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        const double of = __shfl_xor(far, off, 64);
        const int orow = __shfl_xor(row, off, 64);
        const float om = __shfl_xor(mo, off, 64);
        if (better(of, orow, far, row)) { far = of; row = orow; }
        mo = om < mo ? om : mo;
    }
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = Part{far, row, mo};
    __syncthreads();
    far = red[0].far; row = red[0].row; mo = red[0].min_other;
#pragma unroll
    for (int w = 1; w < kBlock / 64; ++w) {
        if (better(red[w].far, red[w].row, far, row)) { far = red[w].far; row = red[w].row; }
        mo = red[w].min_other < mo ? red[w].min_other : mo;
    }
}

__global__ void __launch_bounds__(kBlock) k_dem_step(const float* __restrict__ dist, const int32_t* __restrict__ cls, int n,
                                                     const int32_t* __restrict__ pivots, int ii, double* __restrict__ farsum,
                                                     Part* __restrict__ parts) {
    __shared__ Part red[kBlock / 64];
    const int piv = pivots[ii];
    const int pcls = piv >= 0 ? cls[piv] : 0;
    double best = 0.0;
    int best_row = -1;
    float mo = FLT_MAX;
    for (int j = blockIdx.x * kBlock + threadIdx.x; j < n; j += gridDim.x * kBlock) {   // ascending j per thread
        const float dj = dist[j];
        if (piv >= 0 && cls[j] != pcls && dj < mo) mo = dj;
        const double prev = ii == 0 ? 0.0 : farsum[j];
        const double f = j == piv ? -1000000.0 : prev + (double)dj;
        farsum[j] = f;
        if (f > best) { best = f; best_row = j; }
    }
    block_fold(best, best_row, mo, red);
    if (threadIdx.x == 0) parts[blockIdx.x] = Part{best, best_row, mo};
}

__global__ void __launch_bounds__(kBlock) k_dem_pick(const Part* __restrict__ parts, int nparts, int ii, int n_pivots,
                                                     int32_t* __restrict__ pivots, float* __restrict__ min_other) {
    __shared__ Part red[kBlock / 64];
    double best = 0.0;
    int best_row = -1;
    float mo = FLT_MAX;
    for (int b = threadIdx.x; b < nparts; b += kBlock) {
        const Part p = parts[b];
        if (better(p.far, p.row, best, best_row)) { best = p.far; best_row = p.row; }
        mo = p.min_other < mo ? p.min_other : mo;
    }
    block_fold(best, best_row, mo, red);
    if (threadIdx.x == 0) {
        min_other[ii] = mo;
        if (ii < n_pivots - 1) pivots[ii + 1] = pivots[ii] >= 0 ? best_row : -1;
    }
}

constexpr int kMaxUsed = 32;   // ann.cpp:333-334: only the first 32 pivots are walked at query time
constexpr int kLikBatch = 8;
constexpr int kPinLikRows = 131072;

// lik[q][nu] = sum over the kept pivots i (in order) of (pd[q][i] - table[i][nu])^2, entries with table < 0 skipped (:441).
// pd[q][i] = distance(query q, pivot i). One lane per row; the translation unit is built with -ffp-contract=off.
template <int QB>
__global__ void __launch_bounds__(kBlock) k_dem_lik(const float* __restrict__ table, int n, int used, const float* __restrict__ pd, int nq,
                                                    float* __restrict__ lik) {
    __shared__ float spd[QB][kMaxUsed];
    for (int t = threadIdx.x; t < QB * kMaxUsed; t += kBlock) {
        const int q = t / kMaxUsed, i = t % kMaxUsed;
        spd[q][i] = (q < nq && i < used) ? pd[q * used + i] : 0.0f;
    }
    __syncthreads();
    for (int nu = blockIdx.x * kBlock + threadIdx.x; nu < n; nu += gridDim.x * kBlock) {
        float acc[QB];
#pragma unroll
        for (int q = 0; q < QB; ++q) acc[q] = 0.0f;
        for (int i = 0; i < used; ++i) {
            const float m = table[(size_t)i * n + nu];
            if (m >= 0.0f) {
#pragma unroll
                for (int q = 0; q < QB; ++q) {
                    const float tmp = spd[q][i] - m;
                    acc[q] = acc[q] + tmp * tmp;
                }
            }
        }
#pragma unroll
        for (int q = 0; q < QB; ++q)
            if (q < nq) lik[(size_t)q * n + nu] = acc[q];
    }
}

// The rows the reference's index bookkeeping (:431-432) updates a number of times other than once per pivot: they are
// recomputed with their multiplicities. mult[e][i] = how often exception row e is visited by the update loop of pivot i.
__global__ void k_dem_lik_fix(const float* __restrict__ table, int n, int used, const float* __restrict__ pd, int nq, const int32_t* __restrict__ rows,
                              const uint8_t* __restrict__ mult, int nexc, float* __restrict__ lik) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= nexc * nq) return;
    const int e = t % nexc, q = t / nexc;
    const int nu = rows[e];
    float acc = 0.0f;
    for (int i = 0; i < used; ++i) {
        const float m = table[(size_t)i * n + nu];
        if (m >= 0.0f) {
            const float tmp = pd[q * used + i] - m;
            for (int r = 0; r < mult[e * kMaxUsed + i]; ++r) acc = acc + tmp * tmp;
        }
    }
    lik[(size_t)q * n + nu] = acc;
}

// out[q][k] = distance(query q, gallery row rows[q][k]) over [start,end): lhs = query (ImageInfo::distance).
// A row of the tiled gallery is one float4 per 1 KiB, so a candidate is a gather. One WAVE per `cpw` candidates: its lanes
// fetch the row's float4s side by side (one memory latency instead of d/4 in a row -- the call is latency, not bandwidth),
// park them in LDS next to the query (read ONCE per workgroup: on small calls it sits in pinned host memory), and lane j
// then runs the reference's loop for candidate j in feature order (fir::accum, un-fused).
// Rows longer than `span` float4s go through LDS in pieces of `span` (the sums carry over in the lanes' registers).
// Dynamic LDS: (1 + 4 * cpw) * span float4.
template <int METRIC>
__global__ void __launch_bounds__(kBlock) k_rows_dist(const float4* __restrict__ gal4, int dp4, int64_t n, const float* __restrict__ queries, int d,
                                                      const int32_t* __restrict__ rows, int m, int start, int end, float* __restrict__ out, int cpw,
                                                      int span) {
    extern __shared__ __attribute__((aligned(16))) float4 rsm[];
    float* qs = (float*)rsm;
    const int q = blockIdx.y, wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    float4* mine = rsm + span + (size_t)wave * cpw * span;
    const int k0 = (blockIdx.x * (kBlock / 64) + wave) * cpw;
    const int c0 = start >> 2, c1 = (end - 1) >> 2;
    const int64_t my_row = lane < cpw && k0 + lane < m ? (int64_t)rows[(size_t)q * m + k0 + lane] : -1;
    const bool my_valid = my_row >= 0 && my_row < n;
    float acc = 0.0f;
    for (int cb = c0; cb <= c1; cb += span) {
        const int ce = min(c1, cb + span - 1);                   // chunks [cb, ce] of this piece
        for (int k = cb * 4 + threadIdx.x; k < (ce + 1) * 4; k += kBlock) qs[k - cb * 4] = k < d ? queries[(size_t)q * d + k] : 0.0f;
        for (int j = 0; j < cpw; ++j) {
            const int k = k0 + j;
            const int64_t row = k < m ? (int64_t)rows[(size_t)q * m + k] : -1;
            if (row < 0 || row >= n) continue;                     // wave-uniform
            const float4* __restrict__ base = gal4 + (size_t)(row >> 6) * dp4 * 64 + (row & 63);
            for (int c = cb + lane; c <= ce; c += 64) mine[(size_t)j * span + (c - cb)] = base[(size_t)c * 64];
        }
        __syncthreads();
        if (my_valid) {
            const float* __restrict__ gv = (const float*)(mine + (size_t)lane * span);
            const int f0 = max(start, cb * 4), f1 = min(end, (ce + 1) * 4);
            for (int f = f0; f < f1; ++f) acc = fir::accum<METRIC>(acc, qs[f - cb * 4], gv[f - cb * 4]);
        }
        __syncthreads();
    }
    if (lane < cpw && k0 + lane < m) out[(size_t)q * m + k0 + lane] = my_valid ? acc / (float)(end - start) : fir::kNotFound;
}

// The launch of k_rows_dist for nq queries with m candidate rows each (rows[nq][m] -> out[nq][m]), all pointers the device can read.
// Candidates per wave: 4 while the workgroup's 1 + 16 rows fit 64 KiB of LDS (d <= 960), else 1; rows beyond 2 048 features
// go through LDS in pieces of 512 float4.
void launch_rows_dist(const void* gal4, int dp4, int64_t n, int metric, int d, const float* queries, int nq, const int32_t* rows, int m, int start,
                      int end, float* out, hipStream_t st) {
    const int cpw = (size_t)17 * dp4 * 16 <= 64 * 1024 ? 4 : 1;
    const int span = std::min(dp4, 512);
    const size_t lds = (size_t)(1 + (kBlock / 64) * cpw) * span * 16;
    const int per_block = (kBlock / 64) * cpw;
    const dim3 grid((m + per_block - 1) / per_block, nq);
#define FIR_ROWS_LAUNCH(M) \
    hipLaunchKernelGGL(k_rows_dist<M>, grid, dim3(kBlock), lds, st, (const float4*)gal4, dp4, n, queries, d, rows, m, start, end, out, cpw, span)
    if (metric == FIR_METRIC_L2) FIR_ROWS_LAUNCH(fir::kL2);
    else if (metric == FIR_METRIC_CHI2) FIR_ROWS_LAUNCH(fir::kChi2);
    else FIR_ROWS_LAUNCH(fir::kKL);
#undef FIR_ROWS_LAUNCH
}

// ---- DirectedEnumeration::recognize on the device (fir_dem_recognize; the formulation is in include/fir_amd.h) ------------------
// After the pivot loop the walk of ann.cpp:455-462 needs no sort: the candidates are the Mc = imageCountToCheck - used POSITIONS
// p >= used of likelihood_indices with the smallest keys (likelihood bits, p), found by a radix select; the early exit is "the
// smallest selected key whose distance is below the threshold" (the running best is >= threshold while the walk goes on, so
// such a candidate always also beats it), the full walk "the smallest (distance, key)". Per internal batch of kLikBatch queries:
//   k_dem_head          replays the pivot loop (CHECK_FOR_BEST_DIST, :427-430) per query; queries that leave there are inactive below
//   k_dem_select_one    T = the Mc-th smallest key, 8-bit digits from the top, histogram in LDS: one workgroup per query with the
//                       likelihood bits parked in LDS (up to kSelOneGroupRows candidates), or
//   k_dem_select_pass   one launch per digit, workgroups of kSelSlice positions adding their LDS histogram to the query's
//   k_dem_mark          flags an unselected position that shares its likelihood with a selected one; for the gather form compacts
//                       the selected positions into an unordered list
//   candidate distances k_rows_dist over that list (Mc < n / kGatherDiv), else the range scan into [8][n] read under key <= T
//   k_dem_fold          per-block partials of the two minima, k_dem_finish one workgroup per query: row / dist / found
//   k_dem_count         distanceCalcCount of an early exit and the tie flag's counts, added to calc / tie
constexpr int kSelOneGroupRows = 8192;   // n - used up to which one workgroup per query selects (32 KiB of likelihood bits in LDS)
constexpr int kSelSlice = 2048;          // positions per workgroup and digit in the several-workgroups form
constexpr int kWalkMaxBlocks = 128;      // workgroups per query of mark / fold / count
// Gather while Mc < n / kGatherDiv. Per batch of 8 queries the gather reads 8 * Mc rows, the dense form the gallery once: by
// bytes the two meet at Mc = n / 8, and that is the value until the crossover has been measured on the device: the sweep of
// tools/dem_recognize_probe.py forces either form (fir_dem_probe_) over Mc / n; profiles/dem_recognize.txt holds what is known.
constexpr int kGatherDiv = 8;
constexpr unsigned long long kNoKey = ~0ull;

struct DemQ {               // one query of the batch
    float piv_best;         // the pivot loop's bestDistance / bestIndex
    int32_t piv_row;
    int32_t exit_k;         // the pivot at which the walk left (-1: it did not)
    int32_t active;         // candidates are checked for this query
    int32_t nan_piv;
    int32_t tie_a;
    int32_t n_listed;       // gather form: slots of the candidate list handed out
    int32_t same;           // k_dem_count: selected positions that share the winner's likelihood (and distance)
    int32_t mode;           // 0 nothing to count, 1 early exit at a candidate, 2 a candidate won the full walk
    uint32_t win_lik, win_dist;
    unsigned long long win_key;
    unsigned long long T;
};
// SelState, sel_match, hist_add, sel_advance: fir_knn_select.h (shared with the K-nearest-rows select)
struct FoldPart { unsigned long long exit_key; float exit_dist; uint32_t best_dist; unsigned long long best_key; };

__device__ __forceinline__ unsigned long long dem_key(const float* __restrict__ lik, const int32_t* __restrict__ order, int p) {
    return ((unsigned long long)fir::f32_orderable(lik[order[p]]) << 32) | (unsigned)p;
}
__global__ void __launch_bounds__(64) k_dem_head(const float* __restrict__ pd, int used, int nq, float thr, const int32_t* __restrict__ pivots, int mc,
                                                 int cnt, DemQ* __restrict__ Q, SelState* __restrict__ sel0) {
    const int q = threadIdx.x;
    if (q >= nq) return;
    DemQ s = {};
    s.piv_best = FLT_MAX;
    s.piv_row = -1;
    s.exit_k = -1;
    for (int k = 0; k < used; ++k) {
        const float dk = pd[q * used + k];
        if (dk != dk) s.nan_piv = 1;
        if (dk < s.piv_best) {
            s.piv_best = dk;
            s.piv_row = pivots[k];
            if (dk < thr) { s.exit_k = k; break; }
        }
    }
    s.active = s.exit_k < 0 && mc > 0;
    const int all = mc >= cnt;
    s.T = s.active && all ? kNoKey : 0ull;
    Q[q] = s;
    sel0[q] = SelState{s.T, mc, !s.active || all};
}

__global__ void __launch_bounds__(kBlock) k_dem_select_one(const float* __restrict__ lik, int n, int used, const int32_t* __restrict__ order,
                                                           DemQ* __restrict__ Q, const SelState* __restrict__ sel0) {
    __shared__ unsigned bits[kSelOneGroupRows];
    __shared__ unsigned hist[256];
    __shared__ unsigned wsum[kBlock / 64];
    __shared__ SelState box;
    const int q = blockIdx.x, cnt = min(n - used, kSelOneGroupRows);
    SelState s = sel0[q];
    if (s.done) return;                                               // (head has written T)
    const float* __restrict__ lq = lik + (size_t)q * n;
    for (int i = threadIdx.x; i < cnt; i += kBlock) bits[i] = fir::f32_orderable(lq[order[used + i]]);
    for (int pass = 0; pass < 8 && !s.done; ++pass) {
        hist[threadIdx.x] = 0;
        __syncthreads();
        const int shift = 56 - 8 * pass;
        for (int i0 = 0; i0 < cnt; i0 += kBlock) {
            const int i = i0 + threadIdx.x;
            const unsigned long long key = i < cnt ? ((unsigned long long)bits[i] << 32) | (unsigned)(used + i) : 0ull;
            hist_add(hist, i < cnt && sel_match(key, s.prefix, pass), (unsigned)(key >> shift) & 255u);
        }
        __syncthreads();
        s = sel_advance(s, hist[threadIdx.x], pass, wsum, &box);
    }
    if (threadIdx.x == 0) Q[q].T = s.prefix;
}

// Digit `pass` (0..7) of the several-workgroups form; pass 8 only turns the last histogram into T. sel[j][q] is the state before
// digit j: every workgroup works it out from sel[j-1] and hist[j-1] (complete: the launch before this one), workgroup 0 keeps it.
__global__ void __launch_bounds__(kBlock) k_dem_select_pass(const float* __restrict__ lik, int n, int used, const int32_t* __restrict__ order,
                                                            DemQ* __restrict__ Q, SelState* __restrict__ sel, unsigned* __restrict__ ghist, int pass) {
    __shared__ unsigned hist[256];
    __shared__ unsigned wsum[kBlock / 64];
    __shared__ SelState box;
    const int q = blockIdx.y, cnt = n - used;
    SelState s = sel[(pass == 0 ? 0 : pass - 1) * kLikBatch + q];
    if (pass > 0) {
        s = sel_advance(s, ghist[((size_t)(pass - 1) * kLikBatch + q) * 256 + threadIdx.x], pass - 1, wsum, &box);
        if (blockIdx.x == 0 && threadIdx.x == 0 && pass < 8) sel[pass * kLikBatch + q] = s;
    }
    if (pass == 8) {
        if (blockIdx.x == 0 && threadIdx.x == 0 && Q[q].active) Q[q].T = s.prefix;
        return;
    }
    if (s.done) return;
    hist[threadIdx.x] = 0;
    __syncthreads();
    const float* __restrict__ lq = lik + (size_t)q * n;
    const int shift = 56 - 8 * pass;
    const int i_end = min(cnt, (blockIdx.x + 1) * kSelSlice);
    for (int i0 = blockIdx.x * kSelSlice; i0 < i_end; i0 += kBlock) {
        const int i = i0 + threadIdx.x;
        const unsigned long long key = i < i_end ? dem_key(lq, order, used + i) : 0ull;
        hist_add(hist, i < i_end && sel_match(key, s.prefix, pass), (unsigned)(key >> shift) & 255u);
    }
    __syncthreads();
    if (hist[threadIdx.x]) atomicAdd(&ghist[((size_t)pass * kLikBatch + q) * 256 + threadIdx.x], hist[threadIdx.x]);
}

// rows == NULL: the dense form (only the flag). Otherwise pos[q][mc] / rows[q][mc] <- the selected positions and their rows, in
// no particular order (exactly mc of them; the slot is checked all the same); an inactive query's rows are -1.
__global__ void __launch_bounds__(kBlock) k_dem_mark(const float* __restrict__ lik, int n, int used, const int32_t* __restrict__ order,
                                                     DemQ* __restrict__ Q, int mc, int32_t* __restrict__ pos, int32_t* __restrict__ rows) {
    const int q = blockIdx.y, cnt = n - used, lane = threadIdx.x & 63;
    if (!Q[q].active) {
        if (rows)
            for (int i = blockIdx.x * kBlock + threadIdx.x; i < mc; i += gridDim.x * kBlock) rows[(size_t)q * mc + i] = -1;
        return;
    }
    const unsigned long long T = Q[q].T;
    const float* __restrict__ lq = lik + (size_t)q * n;
    int flag = 0;
    for (int i0 = blockIdx.x * kBlock; i0 < cnt; i0 += gridDim.x * kBlock) {
        const int i = i0 + threadIdx.x, p = used + i;
        const unsigned long long key = i < cnt ? dem_key(lq, order, p) : kNoKey;
        const bool sel = i < cnt && key <= T;
        // (a select that ended early left T's undecided low bits all ones: a key with T's likelihood bits is then never above T)
        if (i < cnt && !sel && (key >> 32) == (T >> 32)) flag = 1;
        if (rows) {
            const unsigned long long m = __ballot(sel);
            if (m) {
                const int leader = __ffsll((long long)m) - 1;
                int base = 0;
                if (lane == leader) base = atomicAdd(&Q[q].n_listed, (int)__popcll(m));
                base = __shfl(base, leader, 64);
                const int slot = base + (int)__popcll(m & ((1ull << lane) - 1));
                if (sel && slot < mc) {
                    pos[(size_t)q * mc + slot] = p;
                    rows[(size_t)q * mc + slot] = order[p];
                }
            }
        }
    }
    if (flag) atomicOr(&Q[q].tie_a, 1);
}

// The selected candidates of query q as mark / the scans left them: pos != NULL: slot i of the list, distance dist[q][mc];
// pos == NULL: position used + i under key <= T, distance dist[q][n] at its row.
struct DemCands {
    const float* __restrict__ lq;
    const int32_t* __restrict__ order;
    const int32_t* __restrict__ pos;
    const float* __restrict__ dist;
    unsigned long long T;
    int n, used, mc;
    __device__ int domain() const { return pos ? mc : n - used; }
    __device__ bool get(int i, unsigned long long* key, float* d) const {
        if (pos) {
            const int p = pos[i];
            if (p < used || p >= n) return false;
            *key = dem_key(lq, order, p);
            *d = dist[i] + 0.0f;
            return true;
        }
        const int p = used + i;
        *key = dem_key(lq, order, p);
        if (*key > T) return false;
        *d = dist[order[p]] + 0.0f;
        return true;
    }
};
__device__ __forceinline__ DemCands dem_cands(const float* lik, int n, int used, const int32_t* order, const DemQ& s, int mc, const int32_t* pos,
                                              const float* dist, int q) {
    return DemCands{lik + (size_t)q * n, order, pos ? pos + (size_t)q * mc : nullptr, dist + (size_t)q * (pos ? mc : n), s.T, n, used, mc};
}

__device__ __forceinline__ FoldPart fold_min(const FoldPart& a, const FoldPart& b) {
    FoldPart r = a;
    if (b.exit_key < r.exit_key) { r.exit_key = b.exit_key; r.exit_dist = b.exit_dist; }
    if (b.best_dist < r.best_dist || (b.best_dist == r.best_dist && b.best_key < r.best_key)) { r.best_dist = b.best_dist; r.best_key = b.best_key; }
    return r;
}
__device__ FoldPart fold_block(FoldPart v, FoldPart* sm) {
    sm[threadIdx.x] = v;
    __syncthreads();
    for (int s = kBlock / 2; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) sm[threadIdx.x] = fold_min(sm[threadIdx.x], sm[threadIdx.x + s]);
        __syncthreads();
    }
    return sm[0];
}

// parts[q][block]: the smallest key with distance < thr (the early exit, :397-398) and the smallest (distance, key) (the full walk).
// A NaN distance is never "< bestDistance": it takes no part.
__global__ void __launch_bounds__(kBlock) k_dem_fold(const float* __restrict__ lik, int n, int used, const int32_t* __restrict__ order,
                                                     const DemQ* __restrict__ Q, int mc, const int32_t* __restrict__ pos, const float* __restrict__ dist,
                                                     float thr, FoldPart* __restrict__ parts) {
    __shared__ FoldPart sm[kBlock];
    const int q = blockIdx.y;
    const DemQ s = Q[q];
    if (!s.active) return;
    const DemCands c = dem_cands(lik, n, used, order, s, mc, pos, dist, q);
    FoldPart v = {kNoKey, 0.0f, 0xFFFFFFFFu, kNoKey};
    for (int i = blockIdx.x * kBlock + threadIdx.x; i < c.domain(); i += gridDim.x * kBlock) {
        unsigned long long key;
        float d;
        if (!c.get(i, &key, &d) || d != d) continue;
        if (d < thr && key < v.exit_key) { v.exit_key = key; v.exit_dist = d; }
        const uint32_t ob = fir::f32_orderable(d);
        if (ob < v.best_dist || (ob == v.best_dist && key < v.best_key)) { v.best_dist = ob; v.best_key = key; }
    }
    v = fold_block(v, sm);
    if (threadIdx.x == 0) parts[(size_t)q * gridDim.x + blockIdx.x] = v;
}

// One workgroup per query: the pivots' result, or the candidates' when they change it. calc and tie are never NULL (k_dem_count
// adds to them); an early exit's calc starts at `used`.
__global__ void __launch_bounds__(kBlock) k_dem_finish(DemQ* __restrict__ Q, const FoldPart* __restrict__ parts, int nparts, int used, int mc,
                                                       const int32_t* __restrict__ order, int32_t* __restrict__ row, float* __restrict__ dist,
                                                       int32_t* __restrict__ found, int32_t* __restrict__ calc, int32_t* __restrict__ tie) {
    __shared__ FoldPart sm[kBlock];
    const int q = blockIdx.x;
    const DemQ s = Q[q];
    FoldPart v = {kNoKey, 0.0f, 0xFFFFFFFFu, kNoKey};
    if (s.active)
        for (int b = threadIdx.x; b < nparts; b += kBlock) v = fold_min(v, parts[(size_t)q * nparts + b]);
    v = fold_block(v, sm);
    if (threadIdx.x != 0) return;
    int r_row = s.piv_row, r_found = s.exit_k >= 0, r_calc = s.exit_k >= 0 ? s.exit_k + 1 : used, r_tie = 0, mode = 0;
    float r_dist = s.piv_best;
    unsigned long long win_key = kNoKey;
    if (s.active) {
        r_tie = s.tie_a | s.nan_piv;
        if (v.exit_key != kNoKey) {
            win_key = v.exit_key;
            r_dist = v.exit_dist;
            r_found = 1;
            mode = 1;                                                  // calc = used + #{selected keys <= win_key}
        } else {
            r_calc = used + mc;
            const float bd = fir::f32_from_orderable(v.best_dist);
            if (v.best_key != kNoKey && bd < s.piv_best) {
                win_key = v.best_key;
                r_dist = bd;
                mode = 2;
            }
        }
        if (mode) r_row = order[(unsigned)win_key];
    }
    uint32_t db;
    __builtin_memcpy(&db, &r_dist, 4);
    Q[q].mode = mode;
    Q[q].win_key = win_key;
    Q[q].win_lik = (uint32_t)(win_key >> 32);
    Q[q].win_dist = db;
    if (row) row[q] = r_row;
    if (dist) dist[q] = r_dist;
    if (found) found[q] = r_found;
    calc[q] = r_calc;
    tie[q] = r_tie;
}

__global__ void __launch_bounds__(kBlock) k_dem_count(const float* __restrict__ lik, int n, int used, const int32_t* __restrict__ order,
                                                      DemQ* __restrict__ Q, int mc, const int32_t* __restrict__ pos, const float* __restrict__ dist,
                                                      int32_t* __restrict__ calc, int32_t* __restrict__ tie) {
    __shared__ int sm[2][kBlock / 64];
    const int q = blockIdx.y;
    const DemQ s = Q[q];
    if (!s.active || s.mode == 0) return;
    const DemCands c = dem_cands(lik, n, used, order, s, mc, pos, dist, q);
    int upto = 0, same = 0;
    for (int i = blockIdx.x * kBlock + threadIdx.x; i < c.domain(); i += gridDim.x * kBlock) {
        unsigned long long key;
        float d;
        if (!c.get(i, &key, &d)) continue;
        uint32_t db;
        __builtin_memcpy(&db, &d, 4);
        if (s.mode == 1) {
            upto += key <= s.win_key;
            same += (uint32_t)(key >> 32) == s.win_lik;
        } else {
            same += (uint32_t)(key >> 32) == s.win_lik && db == s.win_dist;
        }
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        upto += __shfl_xor(upto, off, 64);
        same += __shfl_xor(same, off, 64);
    }
    if ((threadIdx.x & 63) == 0) { sm[0][threadIdx.x >> 6] = upto; sm[1][threadIdx.x >> 6] = same; }
    __syncthreads();
    if (threadIdx.x != 0) return;
    upto = same = 0;
    for (int w = 0; w < kBlock / 64; ++w) { upto += sm[0][w]; same += sm[1][w]; }
    if (upto) atomicAdd(&calc[q], upto);
    if (same && atomicAdd(&Q[q].same, same) + same > 1) atomicOr(&tie[q], 1);   // the winner itself counts once
}

// One thread, queued behind the kernels of a small host-pointer call whose results went to pinned host memory: the call's
// ticket. (A device-wide fence + arrival counter inside the producing kernel costs more than this launch: every
// workgroup's fence is an L2 write-back.)
__global__ void k_dem_ticket(unsigned long long* ticket_word, unsigned long long ticket) {
    __hip_atomic_store(ticket_word, ticket, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
}

// Last kernel of a small fir_dem_likelihoods call: the pivot distances go to pinned host memory, then the ticket.
__global__ void __launch_bounds__(64) k_dem_publish(const float* __restrict__ pd, int count, float* __restrict__ host_pd,
                                                     unsigned long long* ticket_word, unsigned long long ticket) {
    for (int i = threadIdx.x; i < count; i += 64) host_pd[i] = pd[i];
    __threadfence_system();
    __syncthreads();
    if (threadIdx.x == 0) __hip_atomic_store(ticket_word, ticket, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
}

// The PIVOT build. Table row ii goes to d_table + min(ii, keep_rows) * n (rows past keep_rows share one scratch row), the
// pivot's features to d_pivrows + min(ii, keep_piv) * d. Back on the host: pivots[n_pivots], min_other[n_pivots] and the
// number of pivots built (the rest are -1); the last two may be NULL.
int dem_build(fir_gallery* g, const fir_gallery_view& v, int first_pivot, int n_pivots, float* d_table, int keep_rows, float* d_pivrows,
              int keep_piv, int32_t* pivots, float* min_other, int32_t* built) {
    const void* gal4 = nullptr;
    int dp4 = 0;
    if (fir_gallery_tiled_(g, &gal4, &dp4) != FIR_OK || !gal4) return fir_fail_(FIR_ERR_STATE, "gallery has no tiled copy");
    const int n = (int)v.n;
    const int nblocks = std::min(kMaxBlocks, (n + kBlock - 1) / kBlock);
    FirBuf dfar, dparts, dpiv, dmo;
    FIR_HIP(dfar.reserve((size_t)n * 8));
    FIR_HIP(dparts.reserve((size_t)nblocks * sizeof(Part)));
    FIR_HIP(dpiv.reserve((size_t)n_pivots * 4));
    FIR_HIP(dmo.reserve((size_t)n_pivots * 4));
    FIR_HIP(hipMemsetAsync(dpiv.p, 0xff, (size_t)n_pivots * 4, v.stream));
    FIR_HIP(hipMemcpyAsync(dpiv.p, &first_pivot, 4, hipMemcpyHostToDevice, v.stream));
    for (int ii = 0; ii < n_pivots; ++ii) {
        float* row = d_table + (size_t)std::min(ii, keep_rows) * n;
        float* q = d_pivrows + (size_t)std::min(ii, keep_piv) * v.d;
        hipLaunchKernelGGL(k_dem_gather, dim3(std::max(1, std::min(64, (dp4 + kBlock - 1) / kBlock))), dim3(kBlock), 0, v.stream,
                           (const float4*)gal4, dp4, v.d, dpiv.as<int32_t>(), ii, q);
        FIR_HIP(hipGetLastError());
        const int rc = fir_range_distances_dev(g, q, 1, 0, v.d, row, v.stream);
        if (rc) return rc;
        hipLaunchKernelGGL(k_dem_step, dim3(nblocks), dim3(kBlock), 0, v.stream, row, v.cls, n, dpiv.as<int32_t>(), ii, dfar.as<double>(),
                           dparts.as<Part>());
        FIR_HIP(hipGetLastError());
        hipLaunchKernelGGL(k_dem_pick, dim3(1), dim3(kBlock), 0, v.stream, dparts.as<Part>(), nblocks, ii, n_pivots, dpiv.as<int32_t>(),
                           dmo.as<float>());
        FIR_HIP(hipGetLastError());
    }
    FIR_HIP(hipStreamSynchronize(v.stream));   // the four buffers are freed on return
    FIR_HIP(hipMemcpy(pivots, dpiv.p, (size_t)n_pivots * 4, hipMemcpyDeviceToHost));
    if (min_other) FIR_HIP(hipMemcpy(min_other, dmo.p, (size_t)n_pivots * 4, hipMemcpyDeviceToHost));
    if (built) *built = (int32_t)(std::find_if(pivots, pivots + n_pivots, [](int32_t p) { return p < 0; }) - pivots);
    return FIR_OK;
}

int check_build_args(fir_gallery* g, int32_t first_pivot, int32_t n_pivots, fir_gallery_view* v) {
    if (!g) return fir_fail_(FIR_ERR_ARG, "NULL gallery");
    if (fir_gallery_view_(g, v) != FIR_OK) return fir_fail_(FIR_ERR_ARG, "bad gallery");
    if (!v->cls) return fir_fail_(FIR_ERR_STATE, "gallery was created without class labels");
    if (n_pivots <= 0) return fir_fail_(FIR_ERR_ARG, "n_pivots=%d must be positive", n_pivots);
    if (v->n <= 0 || v->n >= (int64_t)1 << 30) return fir_fail_(FIR_ERR_ARG, "gallery of %lld rows outside [1, 2^30)", (long long)v->n);
    if (first_pivot < 0 || first_pivot >= v->n) return fir_fail_(FIR_ERR_ARG, "first_pivot=%d outside the gallery", first_pivot);
    return FIR_OK;
}

// The reference keeps the candidates in an index array and moves each pivot to its front with two plain writes (ann.cpp:431-432);
// the update loop (:437-446) then runs over the POSITIONS behind the front. Replay that on a sparse copy: which rows does each pivot's
// loop visit, and how often? Only rows in {0..used-1} + {pivots} can deviate from "once per pivot": they are `special`, mult[e][i] =
// visits of special[e] by the loop of pivot i, and order_mods = (position, value) wherever the index array is not the identity at the end.
void dem_replay_index(const int32_t* pivots, int used, std::vector<int32_t>* special, std::vector<uint8_t>* mult,
                      std::vector<std::pair<int32_t, int32_t> >* order_mods) {
    std::unordered_map<int32_t, int32_t> mod;   // position -> value, where it is not the identity
    auto at = [&](int32_t pos) { auto it = mod.find(pos); return it == mod.end() ? pos : it->second; };
    for (int i = 0; i < used; ++i) special->push_back(i);
    special->insert(special->end(), pivots, pivots + used);
    std::sort(special->begin(), special->end());
    special->erase(std::unique(special->begin(), special->end()), special->end());
    mult->assign(special->size() * kMaxUsed, 0);
    for (int i = 0; i < used; ++i) {
        const int32_t p = pivots[i];
        mod[p] = at(i);
        mod[i] = p;
        for (size_t e = 0; e < special->size(); ++e) {
            const int32_t w = (*special)[e];
            int cnt = (w > i && mod.find(w) == mod.end()) ? 1 : 0;
            for (const auto& kv : mod)
                if (kv.first > i && kv.second == w) ++cnt;
            (*mult)[e * kMaxUsed + i] = (uint8_t)std::min(cnt, 255);
        }
    }
    for (const auto& kv : mod)
        if (kv.first != kv.second) order_mods->push_back(kv);
    std::sort(order_mods->begin(), order_mods->end());
}

}  // namespace

struct fir_dem {
    fir_gallery* g = nullptr;        // borrowed
    fir_gallery* pivot_rows = nullptr;   // the kept pivots as a gallery of their own: distance(query, pivot i) is one tiny scan
    fir_gallery_view v;
    int n_pivots = 0, used = 0, built = 0, nexc = 0;   // nexc: exception rows of the likelihood update (exc_rows, exc_mult)
    std::vector<int32_t> pivots;
    std::vector<float> min_other;
    std::vector<std::pair<int32_t, int32_t> > order_mods;   // (position, value): where likelihood_indices differs from identity after the pivots
    FirBuf table, pivrows, exc_rows, exc_mult, q, pd, lik;
    // galleries up to kPinLikRows rows: queries in and pivot distances / likelihoods out through pinned, device-visible host
    // memory the kernels address directly, completion by a ticket word (no copy engine, no stream synchronisation): one block,
    // laid out at create, q[8][d] | pd[8][32] | lik[8][n] | the ticket word on the next 8-byte boundary; q == NULL: none
    struct Pin { float *q = nullptr, *pd = nullptr, *lik = nullptr; unsigned long long* tword = nullptr; } pin;
    unsigned long long ticket = 0;
    // fir_dem_recognize: allocated by its first call, of a size that depends on n only, its own (fir_dem_likelihoods may run between two
    // asynchronous calls); r_q / r_out (the host-pointer form's queries and results), r_dist (candidate distances, [8][Mc] gather, [8][n]
    // dense) and r_pos / r_rows (the gather's lists) are the call-sized scratch dem_grow grows.
    bool rec_ready = false;
    FirBuf d_order, d_pivots, r_state, r_pd, r_lik, r_dist, r_pos, r_rows, r_q, r_out;
    // measurement (fir_dem_probe_, tools/dem_recognize_probe.py): a forced candidate-distance form, events between the stages
    int probe_form = 0;
    bool probe_timing = false;
    std::vector<hipEvent_t> probe_ev;
    size_t probe_ev_used = 0;
};

namespace {

// lik[nq][n] <- the likelihoods of nq <= kLikBatch queries from their pivot distances pd[nq][used]: every row once per pivot,
// then the exception rows with their multiplicities. Device-visible pointers.
int dem_queue_lik(fir_dem* h, const float* pd, int nq, float* lik, hipStream_t st) {
    const int n = (int)h->v.n;
    hipLaunchKernelGGL(k_dem_lik<kLikBatch>, dim3(std::min(kMaxBlocks, (n + kBlock - 1) / kBlock)), dim3(kBlock), 0, st, h->table.as<float>(), n,
                       h->used, pd, nq, lik);
    FIR_HIP(hipGetLastError());
    hipLaunchKernelGGL(k_dem_lik_fix, dim3((h->nexc * nq + 63) / 64), dim3(64), 0, st, h->table.as<float>(), n, h->used, pd, nq,
                       h->exc_rows.as<int32_t>(), h->exc_mult.as<uint8_t>(), h->nexc, lik);
    FIR_HIP(hipGetLastError());
    return FIR_OK;
}

// fir_dem_create's query side: the exception rows of the likelihood update, fir_dem_likelihoods' scratch and (up to kPinLikRows rows) pinned block.
int dem_create_query_side(fir_dem* h) {
    const fir_gallery_view& v = h->v;
    std::vector<int32_t> special;
    std::vector<uint8_t> mult;
    dem_replay_index(h->pivots.data(), h->used, &special, &mult, &h->order_mods);
    h->nexc = (int)special.size();
    FIR_HIP(h->exc_rows.reserve(special.size() * 4));
    FIR_HIP(h->exc_mult.reserve(mult.size()));
    FIR_HIP(hipMemcpy(h->exc_rows.p, special.data(), special.size() * 4, hipMemcpyHostToDevice));
    FIR_HIP(hipMemcpy(h->exc_mult.p, mult.data(), mult.size(), hipMemcpyHostToDevice));
    FIR_HIP(h->q.reserve((size_t)kLikBatch * v.d * 4));
    FIR_HIP(h->pd.reserve((size_t)kLikBatch * kMaxUsed * 4));
    FIR_HIP(h->lik.reserve((size_t)kLikBatch * v.n * 4));
    if (v.n > kPinLikRows) return FIR_OK;
    const size_t bytes = (size_t)kLikBatch * ((size_t)v.d + kMaxUsed + (size_t)v.n) * 4 + 64;
    void* pin = nullptr;
    FIR_HIP(hipHostMalloc(&pin, bytes, hipHostMallocDefault));
    std::memset(pin, 0, bytes);
    h->pin.q = (float*)pin;
    h->pin.pd = h->pin.q + (size_t)kLikBatch * v.d;
    h->pin.lik = h->pin.pd + (size_t)kLikBatch * kMaxUsed;
    h->pin.tword = (unsigned long long*)(((uintptr_t)(h->pin.lik + (size_t)kLikBatch * v.n) + 7) & ~(uintptr_t)7);
    return FIR_OK;
}

// r_state, in device memory and addressed by member. sel[j]: the select's state before digit j; parts[q]: the fold's partials of query q
// (walk_blocks of them); calc / tie: stand-ins for outputs not asked for; hist[j]: digit j's histograms of the several-workgroups select.
struct RecState {
    DemQ Q[kLikBatch];
    SelState sel[9][kLikBatch];
    FoldPart parts[kLikBatch][kWalkMaxBlocks];
    int32_t calc[kLikBatch], tie[kLikBatch];
    unsigned hist[8][kLikBatch][256];
};
static_assert(sizeof(RecState) == kLikBatch * (sizeof(DemQ) + 9 * sizeof(SelState) + kWalkMaxBlocks * sizeof(FoldPart) + 2 * 4 + 8 * 256 * 4), "no padding");

int dem_recognize_prepare(fir_dem* h) {
    if (h->rec_ready) return FIR_OK;
    const size_t n = (size_t)h->v.n;
    std::vector<int32_t> order(n);
    for (size_t i = 0; i < n; ++i) order[i] = (int32_t)i;
    for (const auto& kv : h->order_mods) order[(size_t)kv.first] = kv.second;
    FIR_HIP(h->d_order.reserve(n * 4));
    FIR_HIP(h->d_pivots.reserve((size_t)kMaxUsed * 4));
    FIR_HIP(h->r_state.reserve(sizeof(RecState)));
    FIR_HIP(h->r_pd.reserve((size_t)kLikBatch * kMaxUsed * 4));
    FIR_HIP(h->r_lik.reserve((size_t)kLikBatch * n * 4));
    FIR_HIP(hipMemset(h->r_lik.p, 0, (size_t)kLikBatch * n * 4));
    FIR_HIP(hipMemset(h->r_state.p, 0, sizeof(RecState)));
    FIR_HIP(hipMemcpy(h->d_order.p, order.data(), n * 4, hipMemcpyHostToDevice));
    FIR_HIP(hipMemcpy(h->d_pivots.p, h->pivots.data(), (size_t)h->used * 4, hipMemcpyHostToDevice));
    h->rec_ready = true;
    return FIR_OK;
}

// Scratch whose size depends on the call (qb, Mc, the form): grown before anything is queued, after the handle's earlier calls have
// finished with the old buffer; a quarter more than asked for, zero-filled.
int dem_grow(fir_dem* h, FirBuf& b, size_t bytes) {
    if (bytes <= b.cap) return FIR_OK;
    int rc = fir_gallery_wait_calls_(h->g);
    if (rc) return rc;
    FIR_HIP(hipStreamSynchronize(h->v.stream));
    if ((rc = FIR_RESERVE(b, bytes + bytes / 4))) return rc;
    FIR_HIP(hipMemset(b.p, 0, b.cap));
    return FIR_OK;
}

// One call's shape, decided before anything is queued (dem_recognize_plan), and the device pointers its steps share (dem_recognize_reserve).
struct RecPlan {
    int M, mc, cnt;                       // images to check; candidates among them (M - used) out of cnt = n - used positions
    bool gather;                          // candidate distances by gather (else the dense scan)
    enum { kSelNone, kSelOne, kSelPasses } select;   // none: mc == cnt, every position is selected and head has said so
    int walk_blocks;                      // workgroups per query of mark / fold / count
    const void* gal4;                     // the gather's gallery, its row pitch and metric
    int dp4, metric;
    RecState* rs;                         // the handle's buffers, typed
    const int32_t* order;
    float *pd, *lik, *cdist;
    int32_t *pos, *rows;                  // NULL in the dense form
};

int dem_recognize_plan(fir_dem* h, int image_count, RecPlan* p) {
    const int n = (int)h->v.n, used = h->used;
    p->cnt = n - used;
    p->M = image_count > 0 && image_count < n ? image_count : n;
    p->mc = p->M - used;
    if (fir_gallery_tiled_(h->g, &p->gal4, &p->dp4) != FIR_OK || !p->gal4) return fir_fail_(FIR_ERR_STATE, "gallery has no tiled copy");
    // (the gallery's metric now, not h->v.metric: fir_gallery_set_metric may have run since create)
    const int rc = fir_gallery_info(h->g, nullptr, nullptr, &p->metric, nullptr);
    if (rc) return rc;
    p->gather = h->probe_form ? h->probe_form == 1 : p->mc < n / kGatherDiv;
    p->select = p->mc >= p->cnt ? RecPlan::kSelNone : p->cnt <= kSelOneGroupRows ? RecPlan::kSelOne : RecPlan::kSelPasses;
    p->walk_blocks = std::max(1, std::min(kWalkMaxBlocks, (p->cnt + 4 * kBlock - 1) / (4 * kBlock)));
    return FIR_OK;
}

// The plan's call-sized scratch, grown to its need, and the buffers bound.
int dem_recognize_reserve(fir_dem* h, RecPlan* p) {
    const size_t list = (size_t)kLikBatch * p->mc * 4;
    int rc;
    if (p->mc > 0 && (rc = dem_grow(h, h->r_dist, p->gather ? list : (size_t)kLikBatch * h->v.n * 4))) return rc;
    if (p->mc > 0 && p->gather && ((rc = dem_grow(h, h->r_pos, list)) || (rc = dem_grow(h, h->r_rows, list)))) return rc;
    p->rs = h->r_state.as<RecState>();
    p->order = h->d_order.as<int32_t>();
    p->pd = h->r_pd.as<float>();
    p->lik = h->r_lik.as<float>();
    p->cdist = h->r_dist.as<float>();
    p->pos = p->gather ? h->r_pos.as<int32_t>() : nullptr;
    p->rows = p->gather ? h->r_rows.as<int32_t>() : nullptr;
    return FIR_OK;
}

// The five results of a call or of one of its batches, any may be NULL; one internal batch (its calc / tie never are).
struct RecOut { int32_t* row; float* dist; int32_t *found, *calc, *tie; };
struct RecBatch { const float* q; int nq; float thr; RecOut out; hipStream_t st; };

// The steps of a batch, one per stage and probe interval, in the order of kStage*. The driver checks a step's last launch.
int rec_pivots(fir_dem* h, const RecPlan& p, const RecBatch& b) {
    const int rc = fir_range_distances_dev(h->pivot_rows, b.q, b.nq, 0, h->v.d, p.pd, b.st);   // pd[q][used]
    if (rc) return rc;
    hipLaunchKernelGGL(k_dem_head, dim3(1), dim3(64), 0, b.st, p.pd, h->used, b.nq, b.thr, h->d_pivots.as<int32_t>(), p.mc, p.cnt, p.rs->Q, p.rs->sel[0]);
    return FIR_OK;
}

int rec_lik(fir_dem* h, const RecPlan& p, const RecBatch& b) { return dem_queue_lik(h, p.pd, b.nq, p.lik, b.st); }

int rec_select(fir_dem* h, const RecPlan& p, const RecBatch& b) {
    const int n = (int)h->v.n;
    if (p.select == RecPlan::kSelOne) {
        hipLaunchKernelGGL(k_dem_select_one, dim3(b.nq), dim3(kBlock), 0, b.st, p.lik, n, h->used, p.order, p.rs->Q, p.rs->sel[0]);
    } else if (p.select == RecPlan::kSelPasses) {
        FIR_HIP(hipMemsetAsync(p.rs->hist, 0, sizeof(p.rs->hist), b.st));
        const dim3 grid((p.cnt + kSelSlice - 1) / kSelSlice, b.nq);
        for (int pass = 0; pass <= 8; ++pass)
            hipLaunchKernelGGL(k_dem_select_pass, pass < 8 ? grid : dim3(1, b.nq), dim3(kBlock), 0, b.st, p.lik, n, h->used, p.order, p.rs->Q,
                               p.rs->sel[0], p.rs->hist[0][0], pass);
    }
    return FIR_OK;
}

int rec_mark(fir_dem* h, const RecPlan& p, const RecBatch& b) {
    hipLaunchKernelGGL(k_dem_mark, dim3(p.walk_blocks, b.nq), dim3(kBlock), 0, b.st, p.lik, (int)h->v.n, h->used, p.order, p.rs->Q, p.mc, p.pos, p.rows);
    return FIR_OK;
}

int rec_dist(fir_dem* h, const RecPlan& p, const RecBatch& b) {
    const fir_gallery_view& v = h->v;
    if (!p.gather) return fir_range_distances_dev(h->g, b.q, b.nq, 0, v.d, p.cdist, b.st);
    launch_rows_dist(p.gal4, p.dp4, v.n, p.metric, v.d, b.q, b.nq, p.rows, p.mc, 0, v.d, p.cdist, b.st);
    return FIR_OK;
}

int rec_walk(fir_dem* h, const RecPlan& p, const RecBatch& b) {
    const int n = (int)h->v.n, used = h->used;
    if (p.mc > 0) {                                                     // (without candidates finish alone, over no partials)
        hipLaunchKernelGGL(k_dem_fold, dim3(p.walk_blocks, b.nq), dim3(kBlock), 0, b.st, p.lik, n, used, p.order, p.rs->Q, p.mc, p.pos, p.cdist, b.thr,
                           p.rs->parts[0]);
        FIR_HIP(hipGetLastError());
    }
    hipLaunchKernelGGL(k_dem_finish, dim3(b.nq), dim3(kBlock), 0, b.st, p.rs->Q, p.rs->parts[0], p.mc > 0 ? p.walk_blocks : 0, used, p.mc, p.order,
                       b.out.row, b.out.dist, b.out.found, b.out.calc, b.out.tie);
    FIR_HIP(hipGetLastError());
    if (p.mc > 0)
        hipLaunchKernelGGL(k_dem_count, dim3(p.walk_blocks, b.nq), dim3(kBlock), 0, b.st, p.lik, n, used, p.order, p.rs->Q, p.mc, p.pos, p.cdist,
                           b.out.calc, b.out.tie);
    return FIR_OK;
}

enum { kStagePivots, kStageLik, kStageSelect, kStageMark, kStageDist, kStageWalk, kStages };
using RecStep = int (*)(fir_dem*, const RecPlan&, const RecBatch&);
constexpr RecStep kRecSteps[kStages] = {rec_pivots, rec_lik, rec_select, rec_mark, rec_dist, rec_walk};

int dem_stage_mark(fir_dem* h, hipStream_t st) {
    if (!h->probe_timing) return FIR_OK;
    if (h->probe_ev_used == h->probe_ev.size()) {
        hipEvent_t e;
        FIR_HIP(hipEventCreate(&e));
        h->probe_ev.push_back(e);
    }
    FIR_HIP(hipEventRecord(h->probe_ev[h->probe_ev_used++], st));
    return FIR_OK;
}

// The kernels of one call, queued on st; every pointer is the device's. A probe mark in front of every stage and, with candidates,
// one behind the last: kStages + 1 per batch. Without candidates the batch is the pivots and finish (timing needs mc > 0).
int dem_recognize_queue(fir_dem* h, const RecPlan& p, const float* dq, int qb, float thr, const RecOut& out, hipStream_t st) {
    for (int q0 = 0; q0 < qb; q0 += kLikBatch) {
        const RecOut o = {out.row ? out.row + q0 : nullptr, out.dist ? out.dist + q0 : nullptr, out.found ? out.found + q0 : nullptr,
                          out.calc ? out.calc + q0 : p.rs->calc, out.tie ? out.tie + q0 : p.rs->tie};
        const RecBatch b = {dq + (size_t)q0 * h->v.d, std::min(kLikBatch, qb - q0), thr, o, st};
        int rc;
        for (int s = 0; s < kStages; ++s) {
            if (p.mc <= 0 && s != kStagePivots && s != kStageWalk) continue;
            if ((rc = dem_stage_mark(h, st)) || (rc = kRecSteps[s](h, p, b))) return rc;
            FIR_HIP(hipGetLastError());
        }
        if (p.mc > 0 && (rc = dem_stage_mark(h, st))) return rc;
    }
    return FIR_OK;
}

// Both entry points. host: queries and results are the host's: the call runs on the handle's own stream, the results come back
// through one device block of five columns [row | dist | found | calc | tie][qb], and it waits for them.
int dem_recognize_call(fir_dem* h, const float* queries, int32_t qb, float thr, int32_t image_count, const RecOut& out, bool host, void* stream) {
    if (!h) return fir_fail_(FIR_ERR_ARG, "fir_dem_recognize: NULL handle");
    if (qb <= 0) return fir_fail_(FIR_ERR_ARG, "fir_dem_recognize: qb=%d must be positive", qb);
    if (!queries) return fir_fail_(FIR_ERR_ARG, "fir_dem_recognize: queries is NULL");
    if (!out.row && !out.dist && !out.found && !out.calc && !out.tie) return fir_fail_(FIR_ERR_ARG, "fir_dem_recognize: every output is NULL");
    if (const int rcg = fir_gallery_stale_(h->g, h->v.generation, "fir_dem")) return rcg;     // (the table is [pivot][n of then])
    const fir_gallery_view& v = h->v;
    FIR_HIP(hipSetDevice(v.device));
    const hipStream_t st = !host && stream ? (hipStream_t)stream : v.stream;
    FirCallOrder order(h->g, st);
    if (order.rc) return order.rc;
    RecPlan p{};
    int rc;
    if ((rc = dem_recognize_prepare(h)) || (rc = dem_recognize_plan(h, image_count, &p)) || (rc = dem_recognize_reserve(h, &p))) return rc;
    if (!host) return dem_recognize_queue(h, p, queries, qb, thr, out, st);
    const size_t qbytes = (size_t)qb * v.d * 4, obytes = (size_t)qb * 4;
    if ((rc = dem_grow(h, h->r_q, qbytes)) || (rc = dem_grow(h, h->r_out, 5 * obytes))) return rc;
    int32_t* o = h->r_out.as<int32_t>();
    FIR_HIP(hipMemcpyAsync(h->r_q.p, queries, qbytes, hipMemcpyHostToDevice, st));
    const RecOut dev = {o, (float*)(o + qb), o + 2 * (size_t)qb, o + 3 * (size_t)qb, o + 4 * (size_t)qb};
    if ((rc = dem_recognize_queue(h, p, h->r_q.as<float>(), qb, thr, dev, st))) return rc;
    void* outs[5] = {out.row, out.dist, out.found, out.calc, out.tie};
    for (int k = 0; k < 5; ++k)
        if (outs[k]) FIR_HIP(hipMemcpyAsync(outs[k], o + (size_t)k * qb, obytes, hipMemcpyDeviceToHost, st));
    FIR_HIP(hipStreamSynchronize(st));
    order.done();
    return FIR_OK;
}

// The pinned, device-visible buffer a gallery handle lends to a small fir_rows_distances call: queries and rows share its query
// block (the rows on the next 16-byte boundary), the distances come back in its results block, whose last word (of 4096) is the ticket's.
struct RowsPin { float* q; int32_t* rows; float* out; unsigned long long* tword; };

// Small calls (the DEM walk: one query, a few hundred candidate rows): everything through the lent buffer -- no allocation, no
// copy engine, no stream synchronisation (a ticket written behind the kernel). false: the call does not fit, or the launch failed
// or never published -- the general path then runs it and reports why.
bool rows_dist_small(fir_gallery* g, const fir_gallery_view& v, const void* gal4, int dp4, const float* queries, int qb, const int32_t* rows, int m,
                     int start, int end, float* out) {
    const size_t qbytes = (size_t)qb * v.d * 4, rows_at = (qbytes + 15) & ~(size_t)15, rbytes = (size_t)qb * m * 4;
    void* base = nullptr;
    size_t cap = 0;
    uint64_t* res = nullptr;
    if ((size_t)qb * m > 8000 || fir_gallery_pin_(g, &base, &cap, &res) != FIR_OK || rows_at + rbytes > cap) return false;
    const RowsPin pin = {(float*)base, (int32_t*)((char*)base + rows_at), (float*)res, (unsigned long long*)(res + 4095)};
    std::memcpy(pin.q, queries, qbytes);
    std::memcpy(pin.rows, rows, rbytes);
    const unsigned long long ticket = fir_gallery_next_ticket_(g);
    launch_rows_dist(gal4, dp4, v.n, v.metric, v.d, pin.q, qb, pin.rows, m, start, end, pin.out, v.stream);
    hipLaunchKernelGGL(k_dem_ticket, dim3(1), dim3(1), 0, v.stream, pin.tword, ticket);
    if (hipGetLastError() == hipSuccess && fir_wait_ticket_(v.stream, (volatile uint64_t*)pin.tword, ticket) == FIR_OK) {
        std::memcpy(out, pin.out, rbytes);
        return true;
    }
    (void)hipStreamSynchronize(v.stream);
    return false;
}

}  // namespace

extern "C" {

int fir_dem_pivot_table(fir_gallery* g, int32_t first_pivot, int32_t n_pivots, int32_t* pivots_out, float* table_out, float* min_other_out,
                        int32_t* n_built_out) {
    fir_gallery_view v;
    int rc = check_build_args(g, first_pivot, n_pivots, &v);
    if (rc) return rc;
    if (!pivots_out) return fir_fail_(FIR_ERR_ARG, "pivots_out is NULL");
    FIR_HIP(hipSetDevice(v.device));
    const int keep = table_out ? n_pivots - 1 : 0;
    FirBuf dtable, dq;
    FIR_HIP(dtable.reserve((size_t)(keep + 1) * v.n * 4));
    FIR_HIP(dq.reserve((size_t)v.d * 4));
    if ((rc = dem_build(g, v, first_pivot, n_pivots, dtable.as<float>(), keep, dq.as<float>(), 0, pivots_out, min_other_out, n_built_out))) return rc;
    if (table_out) FIR_HIP(hipMemcpy(table_out, dtable.p, (size_t)n_pivots * v.n * 4, hipMemcpyDeviceToHost));
    return FIR_OK;
}

int fir_dem_create(fir_gallery* g, int32_t first_pivot, int32_t n_pivots, fir_dem** out) {
    fir_gallery_view v;
    int rc = check_build_args(g, first_pivot, n_pivots, &v);
    if (rc) return rc;
    if (!out) return fir_fail_(FIR_ERR_ARG, "out is NULL");
    *out = nullptr;
    FIR_HIP(hipSetDevice(v.device));
    fir_dem* h = new fir_dem();
    struct Guard { fir_dem* h; ~Guard() { if (h) fir_dem_destroy(h); } } guard{h};
    h->g = g; h->v = v; h->n_pivots = n_pivots;
    const int keep = std::min<int>(n_pivots, kMaxUsed);
    FIR_HIP(h->table.reserve((size_t)(keep + 1) * v.n * 4));
    FIR_HIP(h->pivrows.reserve((size_t)(keep + 1) * v.d * 4));
    h->pivots.resize((size_t)n_pivots);
    h->min_other.resize((size_t)n_pivots);
    if ((rc = dem_build(g, v, first_pivot, n_pivots, h->table.as<float>(), keep, h->pivrows.as<float>(), keep, h->pivots.data(), h->min_other.data(),
                        &h->built)))
        return rc;
    h->used = std::min(h->built, kMaxUsed);
    if ((rc = fir_gallery_create_dev(h->pivrows.as<float>(), h->used, v.d, nullptr, v.metric, v.device, v.stream, &h->pivot_rows))) return rc;
    if ((rc = dem_create_query_side(h))) return rc;
    guard.h = nullptr;
    *out = h;
    return FIR_OK;
}

int fir_dem_destroy(fir_dem* h) {
    if (!h) return FIR_OK;
    (void)hipSetDevice(h->v.device);
    if (h->pivot_rows) fir_gallery_destroy(h->pivot_rows);
    if (h->pin.q) (void)hipHostFree(h->pin.q);
    for (hipEvent_t e : h->probe_ev) (void)hipEventDestroy(e);
    delete h;
    return FIR_OK;
}

int fir_dem_info(const fir_dem* h, int32_t* n_pivots, int32_t* n_built, int32_t* n_used, int64_t* n) {
    if (!h) return fir_fail_(FIR_ERR_ARG, "NULL handle");
    if (n_pivots) *n_pivots = h->n_pivots;
    if (n_built) *n_built = h->built;
    if (n_used) *n_used = h->used;
    if (n) *n = h->v.n;
    return FIR_OK;
}

int fir_dem_get(fir_dem* h, int32_t* pivots_out, float* min_other_out, float* table_out, int32_t* order_out) {
    if (!h) return fir_fail_(FIR_ERR_ARG, "NULL handle");
    if (pivots_out) std::copy(h->pivots.begin(), h->pivots.end(), pivots_out);
    if (min_other_out) std::copy(h->min_other.begin(), h->min_other.end(), min_other_out);
    if (table_out) {
        FIR_HIP(hipSetDevice(h->v.device));
        FIR_HIP(hipMemcpy(table_out, h->table.p, (size_t)h->used * h->v.n * 4, hipMemcpyDeviceToHost));
    }
    if (order_out) {
        for (int64_t i = 0; i < h->v.n; ++i) order_out[i] = (int32_t)i;
        for (const auto& kv : h->order_mods) order_out[kv.first] = kv.second;
    }
    return FIR_OK;
}

int fir_dem_likelihoods(fir_dem* h, const float* queries, int32_t qb, float* pivot_dist_out, float* lik_out) {
    if (!h || (qb > 0 && !queries)) return fir_fail_(FIR_ERR_ARG, "NULL argument");
    if (qb < 0) return fir_fail_(FIR_ERR_ARG, "qb < 0");
    if (const int rcg = fir_gallery_stale_(h->g, h->v.generation, "fir_dem")) return rcg;
    const fir_gallery_view& v = h->v;
    FIR_HIP(hipSetDevice(v.device));
    const int n = (int)v.n, used = h->used;
    const fir_dem::Pin& pin = h->pin;
    float* pd = h->pd.as<float>();
    const float* dq = pin.q ? pin.q : h->q.as<float>();          // what the kernels read and write: the pinned block, or device scratch
    float* dlik = pin.q ? pin.lik : h->lik.as<float>();
    for (int q0 = 0; q0 < qb; q0 += kLikBatch) {
        const int nq = std::min(kLikBatch, qb - q0);
        const float* q = queries + (size_t)q0 * v.d;
        float* pd_out = pivot_dist_out ? pivot_dist_out + (size_t)q0 * used : nullptr;
        float* l_out = lik_out ? lik_out + (size_t)q0 * n : nullptr;
        int rc;
        if (pin.q) {
            std::memcpy(pin.q, q, (size_t)nq * v.d * 4);
        } else {
            FIR_HIP(hipMemcpyAsync(h->q.p, q, (size_t)nq * v.d * 4, hipMemcpyHostToDevice, v.stream));
        }
        if ((rc = fir_range_distances_dev(h->pivot_rows, dq, nq, 0, v.d, pd, v.stream))) return rc;   // pd[q][used]
        if (!pin.q && pd_out) FIR_HIP(hipMemcpyAsync(pd_out, pd, (size_t)nq * used * 4, hipMemcpyDeviceToHost, v.stream));
        if (l_out && (rc = dem_queue_lik(h, pd, nq, dlik, v.stream))) return rc;
        if (!pin.q) {
            if (l_out) FIR_HIP(hipMemcpyAsync(l_out, dlik, (size_t)nq * n * 4, hipMemcpyDeviceToHost, v.stream));
            FIR_HIP(hipStreamSynchronize(v.stream));
            continue;
        }
        const unsigned long long ticket = ++h->ticket;
        hipLaunchKernelGGL(k_dem_publish, dim3(1), dim3(64), 0, v.stream, pd, nq * used, pin.pd, pin.tword, ticket);
        FIR_HIP(hipGetLastError());
        if ((rc = fir_wait_ticket_(v.stream, (volatile uint64_t*)pin.tword, ticket))) return rc;
        if (pd_out) std::memcpy(pd_out, pin.pd, (size_t)nq * used * 4);
        if (l_out) std::memcpy(l_out, pin.lik, (size_t)nq * n * 4);
    }
    return FIR_OK;
}

int fir_rows_distances(fir_gallery* g, const float* queries, int32_t qb, const int32_t* rows, int32_t m, int32_t start_pos, int32_t end_pos,
                       float* out) {
    fir_gallery_view v;
    if (!g || (qb > 0 && m > 0 && (!queries || !rows || !out))) return fir_fail_(FIR_ERR_ARG, "NULL argument");
    if (fir_gallery_view_(g, &v) != FIR_OK) return fir_fail_(FIR_ERR_ARG, "bad gallery");
    if (qb < 0 || m < 0 || qb > 65535) return fir_fail_(FIR_ERR_ARG, "qb=%d / m=%d out of range", qb, m);
    if (end_pos == 0) end_pos = v.d;
    if (start_pos < 0 || end_pos > v.d || start_pos >= end_pos) return fir_fail_(FIR_ERR_ARG, "feature range [%d,%d) outside [0,%d)", start_pos, end_pos, v.d);
    if (qb == 0 || m == 0) return FIR_OK;
    const void* gal4 = nullptr;
    int dp4 = 0;
    if (fir_gallery_tiled_(g, &gal4, &dp4) != FIR_OK || !gal4) return fir_fail_(FIR_ERR_STATE, "gallery has no tiled copy");
    FIR_HIP(hipSetDevice(v.device));
    FirCallOrder order(g, v.stream);               // (a host-pointer call: on the handle's own stream, after its earlier calls)
    if (order.rc) return order.rc;
    if (rows_dist_small(g, v, gal4, dp4, queries, qb, rows, m, start_pos, end_pos, out)) return FIR_OK;
    const size_t qbytes = (size_t)qb * v.d * 4, rbytes = (size_t)qb * m * 4;
    void *dq = nullptr, *drows = nullptr, *dout = nullptr;
    int rc;
    if ((rc = fir_gallery_scratch_(g, 8, qbytes, &dq))) return rc;
    if ((rc = fir_gallery_scratch_(g, 9, rbytes, &drows))) return rc;
    if ((rc = fir_gallery_scratch_(g, 10, rbytes, &dout))) return rc;
    FIR_HIP(hipMemcpyAsync(dq, queries, qbytes, hipMemcpyHostToDevice, v.stream));
    FIR_HIP(hipMemcpyAsync(drows, rows, rbytes, hipMemcpyHostToDevice, v.stream));
    launch_rows_dist(gal4, dp4, v.n, v.metric, v.d, (const float*)dq, qb, (const int32_t*)drows, m, start_pos, end_pos, (float*)dout, v.stream);
    FIR_HIP(hipGetLastError());
    FIR_HIP(hipMemcpyAsync(out, dout, rbytes, hipMemcpyDeviceToHost, v.stream));
    FIR_HIP(hipStreamSynchronize(v.stream));
    return FIR_OK;
}

// Measurement hooks of tools/dem_recognize_probe.py (not in include/fir_amd.h; the tool resolves them by name). form: 0 = the library's choice, 1 = gather, 2 = dense
// candidate distances (the answers are the same); timing != 0: events between the stages of every internal batch from now on.
int fir_dem_probe_(fir_dem* h, int32_t form, int32_t timing) {
    if (!h || form < 0 || form > 2) return fir_fail_(FIR_ERR_ARG, "fir_dem_probe_: bad argument");
    h->probe_form = form;
    h->probe_timing = timing != 0;
    h->probe_ev_used = 0;
    return FIR_OK;
}
// ms[6] <- the device time of each stage (pivots, likelihoods, select, mark, candidate distances, fold + finish + count), summed
// over the batches queued since fir_dem_probe_ (calls with candidates to check only); starts the sums again.
int fir_dem_probe_times_(fir_dem* h, float* ms) {
    if (!h || !ms) return fir_fail_(FIR_ERR_ARG, "fir_dem_probe_times_: NULL argument");
    FIR_HIP(hipSetDevice(h->v.device));
    for (int k = 0; k < kStages; ++k) ms[k] = 0.0f;
    if (h->probe_ev_used % (kStages + 1)) return fir_fail_(FIR_ERR_STATE, "fir_dem_probe_times_: a timed call had no candidates to check");
    for (size_t b = 0; b + kStages < h->probe_ev_used; b += kStages + 1) {
        FIR_HIP(hipEventSynchronize(h->probe_ev[b + kStages]));
        for (int k = 0; k < kStages; ++k) {
            float t = 0.0f;
            FIR_HIP(hipEventElapsedTime(&t, h->probe_ev[b + k], h->probe_ev[b + k + 1]));
            ms[k] += t;
        }
    }
    h->probe_ev_used = 0;
    return FIR_OK;
}

int fir_dem_recognize_dev(fir_dem* h, const float* d_queries, int32_t qb, float threshold, int32_t image_count_to_check, int32_t* d_row,
                          float* d_dist, int32_t* d_found, int32_t* d_calc, int32_t* d_tie, void* stream) {
    return dem_recognize_call(h, d_queries, qb, threshold, image_count_to_check, RecOut{d_row, d_dist, d_found, d_calc, d_tie}, false, stream);
}

int fir_dem_recognize(fir_dem* h, const float* queries, int32_t qb, float threshold, int32_t image_count_to_check, int32_t* row, float* dist,
                      int32_t* found, int32_t* calc, int32_t* tie) {
    return dem_recognize_call(h, queries, qb, threshold, image_count_to_check, RecOut{row, dist, found, calc, tie}, true, nullptr);
}

}  // extern "C"
