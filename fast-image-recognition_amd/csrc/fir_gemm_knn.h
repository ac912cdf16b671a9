// fir_gemm_knn.h -- the K nearest rows for kTopKMax < K <= FIR_GEMM_KNN_MAX on the matrix cores (fir_gemm_search_knn_keys_dev;
// included by fir_gemm.hip, inside its anonymous namespace, behind fir_gemm_rerank.h and k_gemm_tau_class). The flow is the
// distinct-class form's, per super-batch:
//   a. D_s[q] = the exact K-th smallest reference distance over a row sample (fir_knn_sample_bound_dev_, fir_capi.hip): an order
//      statistic of a subset of the rows, so an upper bound of the gallery's K-th distance D_K whatever the sample is;
//   b. k_gemm_tau_class turns it into the append pass's bound: D_s in proxy units plus one rounding window -- every row with a
//      reference distance <= D_s has a proxy below it, so the K nearest rows are all appended;
//   c. the fp16 append pass below that bound (k_gemm_proxy_f16x<1, ...>, kBelowTau), untouched;
//   d. k_gemm_rerank_knn below: exact distances of the entries inside the window on the K-th smallest proxy, the K smallest exact
//      keys, and the certificate.
// What is not certified (a list that overflowed, NaN operands, a tie at the certificate's bound) is answered by the store + select
// form of fir_search_knn_keys_dev after the call's one synchronisation (gemm_finish_knn_, fir_gemm.hip): no second-chance rounds.
// fir_gemm_search_radius_keys_dev (every row within a per-query radius) is the same flow without step a: the radius is D_s, and
// k_gemm_rerank_radius at the end of this file takes the place of k_gemm_rerank_knn.
#pragma once

// The rank-th smallest (rank >= 1, at most `have`) of the wave's list of `have` unique 64-bit keys, by its top `ndig` bytes: an
// MSB-first radix select, one 256-bin histogram in LDS per digit (fir_knn_select.h's sel_match / hist_add; the rank step is
// sel_advance's, folded over one wave: lane l owns bins 4 l .. 4 l + 3). Returns the decided bytes, the rest zero. With ndig = 8
// that is the key itself; with ndig = 4 over (proxy, row) keys the orderable bits of the rank-th smallest proxy.
__device__ __forceinline__ unsigned long long wave_list_select_(const unsigned long long* L, int have, int rank_in, int ndig, unsigned* hist, int lane) {
    unsigned long long prefix = 0;
    unsigned rank = (unsigned)rank_in;
    for (int pass = 0; pass < ndig; ++pass) {
        const int shift = 56 - 8 * pass;
        for (int i = lane; i < 256; i += 64) hist[i] = 0;
        __syncthreads();
        for (int base = 0; base < have; base += 64) {                   // wave-uniform trip count: every lane makes every call
            const int i = base + lane;
            const unsigned long long v = i < have ? L[i] : 0ull;
            fir::hist_add(hist, i < have && fir::sel_match(v, prefix, pass), (unsigned)(v >> shift) & 255u);
        }
        __syncthreads();
        const unsigned c0 = hist[4 * lane], c1 = hist[4 * lane + 1], c2 = hist[4 * lane + 2], c3 = hist[4 * lane + 3];
        const unsigned tot = c0 + c1 + c2 + c3;
        unsigned incl = tot;
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const unsigned o = __shfl_up(incl, off, 64);
            if (lane >= off) incl += o;
        }
        unsigned e = incl - tot;
        const unsigned long long who = __ballot(tot > 0 && e < rank && rank <= incl);
        if (who == 0) return kKeyNone;                                  // (a rank outside the list: cannot happen, and must not hang)
        const int src = __ffsll((long long)who) - 1;
        int b = 0;
        if (rank > e + c0) { e += c0; b = 1; if (rank > e + c1) { e += c1; b = 2; if (rank > e + c2) { e += c2; b = 3; } } }
        const unsigned bin = (unsigned)__shfl(4 * lane + b, src, 64);
        rank = __shfl(rank - e, src, 64);
        prefix |= (unsigned long long)bin << shift;
        __syncthreads();                                                // the histogram is cleared again by the next digit
    }
    return prefix;
}

// The k smallest of the wave's list of exact keys (kKeyNone entries take no part), ascending, into out[0..k), kKeyNone behind them:
// a radix select for the take-th smallest key T, take = min(k, keys there are) -- keys are unique, the row is part of the key, so a
// cut inside a run of equal distances is exact --, the keys <= T compacted into `sorted` and sorted there. Returns how many keys
// the list holds (`valid`); sorted[0..min(valid, k)) stays readable. k = 0: only the count.
__device__ __forceinline__ int wave_list_smallest_(const unsigned long long* L, int have, int k, unsigned* hist, unsigned long long* sorted,
                                                   unsigned long long* out, int lane) {
    int valid = 0;
    for (int base = 0; base < have; base += 64) valid += __popcll(__ballot(base + lane < have && L[base + lane] != kKeyNone));
    const int take = valid < k ? valid : k;
    int P = 2;
    while (P < take) P *= 2;
    for (int i = lane; i < P; i += 64) sorted[i] = kKeyNone;
    unsigned long long T = 0;
    if (take > 0) T = wave_list_select_(L, have, take, 8, hist, lane);  // (ends with a barrier: `sorted` is cleared)
    else __syncthreads();
    int filled = 0;
    for (int base = 0; base < have && take > 0; base += 64) {
        const unsigned long long v = base + lane < have ? L[base + lane] : kKeyNone;
        const bool mine = v != kKeyNone && v <= T;
        const unsigned long long m = __ballot(mine);
        const int slot = filled + (int)__popcll(m & ((1ull << lane) - 1ull));
        if (mine && slot < P) sorted[slot] = v;                         // (exactly `take` keys are <= T: the check costs nothing)
        filled += (int)__popcll(m);
    }
    __syncthreads();
    for (int k2 = 2; k2 <= P; k2 <<= 1)
        for (int j = k2 >> 1; j > 0; j >>= 1) {
            for (int i = lane; i < P; i += 64) {
                const int o = i ^ j;
                if (o > i) {
                    const unsigned long long x = sorted[i], y = sorted[o];
                    if ((x > y) == ((i & k2) == 0)) { sorted[i] = y; sorted[o] = x; }
                }
            }
            __syncthreads();
        }
    for (int i = lane; i < k; i += 64) out[i] = i < take ? sorted[i] : kKeyNone;
    return valid;
}

// The re-rank of one append pass below k_gemm_tau_class's bound, for the K nearest rows (kTopKMax < K <= 256) and, RADIUS, for every
// row within radius[q]. One wave per query.
//   1. a list that overflowed is not certified: the exact form answers the query.
//   2. p_K = the K-th smallest proxy of the list (a radix select over the proxies: K rounds of list_kth_smallest_ would be ~10 000
//      wave steps at K = 256 over 2 500 entries), +inf for a list shorter than K: everything is re-ranked.
//   3. every entry with a proxy <= p_K + 2 E d is re-ranked in the reference's arithmetic (rerank_gather_f32_) and its exact key
//      written back over its list entry; entries outside the window, and rows with dist >= 100000, become kKeyNone.
//   4. the K smallest exact keys, ascending, padded with kKeyNone (wave_list_smallest_). LDS: 1 KiB of histogram + 2 KiB of keys
//      next to the re-rank's rows; the list itself stays in global memory (sorting 4 096 keys in LDS would take 32 KiB per wave
//      and leave the gathers three waves per CU).
// Certificate, against the K-th exact distance D (100000 with fewer than K found -- any qualifying row outside the re-ranked set
// would then belong to the answer): rerank_certified_ as k_gemm_rerank_classes calls it. Every row not appended or not re-ranked
// then has a reference distance above D, the K rows found are at or below D, so the K smallest keys over ALL rows are the K found.
// Strict '>': a NaN never certifies, a tie with the K-th does not either.
// RADIUS (the query brings its bound, no row sample was scanned) differs in three places: the window is +inf, so EVERY entry is
// re-ranked; a key is kept only if `dist < radius` as well; out_count[q] = the keys left, of which the min(count, k) smallest are
// written (k = 0: the count alone, `out` is never written), and the radius stands in the place of D (the cut-off 100000 for a
// radius at or above it, or NaN). A row never appended has a proxy >= tau, hence a reference distance >= (|q|^2 + tau) / d - E,
// which the certificate finds above the radius: `dist < radius` is false for it, it is not part of the answer, and every row that
// is was appended, re-ranked exactly and counted.
template <bool RADIUS>
__device__ __forceinline__ void gemm_rerank_list_(unsigned long long* lists, const int* __restrict__ counts, const float* __restrict__ tau,
                                                  const float* __restrict__ radius, const float4* __restrict__ gal4, const float* __restrict__ queries,
                                                  const float* __restrict__ qnorm, const float* __restrict__ gnorm_max_p, int64_t n, int d, int dp4,
                                                  int64_t row_offset, float e_rel, int ngroup, int k, unsigned long long* __restrict__ out_key,
                                                  int* __restrict__ out_count, int* __restrict__ ok, int qstride, const float4* __restrict__ rowmajor) {
    __shared__ unsigned hist[256];
    __shared__ unsigned long long sorted[fir::kKnnGemmMax];
    const int q = blockIdx.x, lane = threadIdx.x;
    const int cnt = counts[q];
    if (cnt > kListCap) {                           // rows below tau were dropped: the exact form answers this query
        if (lane == 0) ok[q] = 0;
        return;
    }
    const int have = cnt;
    unsigned long long* L = lists + (size_t)q * kListCap;
    unsigned long long* out = out_key + (size_t)q * k;
    const float qn = qnorm[q], gmax = gnorm_max_p[0], r = RADIUS ? radius[q] : 0.f;
    float pk = __builtin_huge_valf();                                   // a list shorter than K is re-ranked whole, a radius's always
    if (!RADIUS && have >= k) pk = fir::f32_from_orderable((uint32_t)(wave_list_select_(L, have, k, 4, hist, lane) >> 32));
    const RerankWindow w = rerank_window_(e_rel, qn, gmax, d, pk);
    extern __shared__ __attribute__((aligned(16))) float4 crow[];
    const RerankLds lds = rerank_lds_f32_(crow, ngroup, dp4, d, queries + (size_t)q * qstride, lane);
    const RerankWalk walk = rerank_walk_(L, have, w.win, lane, [&](int base, unsigned long long v, bool in, unsigned long long mask) {
        if (base + lane < have && !in) L[base + lane] = kKeyNone;       // (RADIUS: a NaN proxy, never appended)
        rerank_gather_f32_(mask, v, base, lane, ngroup, lds, gal4, rowmajor, dp4, d, [&](int i, unsigned long long cv, float dist) {
            const int64_t row = (int64_t)(uint32_t)(cv & 0xFFFFFFFFull);
            L[i] = (!RADIUS || dist < r) && dist < fir::kNotFound ? fir::key_pack(dist, (uint32_t)(row + row_offset)) : kKeyNone;
        });
    });
    __threadfence_block();                                              // the exact keys, written by other lanes, are read below
    __syncthreads();
    const int valid = wave_list_smallest_(L, have, k, hist, sorted, out, lane);
    if (lane != 0) return;
    if (RADIUS) {
        out_count[q] = valid;
        ok[q] = rerank_certified_<float>(cnt, tau[q], walk.p_out, qn, d, w.E, r < fir::kNotFound, r, n, walk.reranked) ? 1 : 0;
    } else {
        const unsigned long long kth_exact = valid >= k ? sorted[k - 1] : kKeyNone;
        ok[q] = rerank_certified_<float>(cnt, tau[q], walk.p_out, qn, d, w.E, kth_exact != kKeyNone, fir::f32_from_orderable((uint32_t)(kth_exact >> 32)), n,
                                         walk.reranked) ? 1 : 0;
    }
}

__global__ void __launch_bounds__(64) k_gemm_rerank_knn(unsigned long long* lists, const int* __restrict__ counts, const float* __restrict__ tau,
                                                         const float4* __restrict__ gal4, const float* __restrict__ queries,
                                                         const float* __restrict__ qnorm, const float* __restrict__ gnorm_max_p, int64_t n, int d, int dp4,
                                                         int64_t row_offset, float e_rel, int ngroup, int k, unsigned long long* __restrict__ out_key,
                                                         int* __restrict__ ok, int qstride, const float4* __restrict__ rowmajor) {
    gemm_rerank_list_<false>(lists, counts, tau, nullptr, gal4, queries, qnorm, gnorm_max_p, n, d, dp4, row_offset, e_rel, ngroup, k, out_key, nullptr, ok, qstride,
                             rowmajor);
}

// Every row within a per-query radius (fir_gemm_search_radius_keys_dev): gemm_rerank_list_'s RADIUS form.
__global__ void __launch_bounds__(64) k_gemm_rerank_radius(unsigned long long* lists, const int* __restrict__ counts, const float* __restrict__ tau,
                                                            const float* __restrict__ radius, const float4* __restrict__ gal4,
                                                            const float* __restrict__ queries, const float* __restrict__ qnorm,
                                                            const float* __restrict__ gnorm_max_p, int64_t n, int d, int dp4, int64_t row_offset, float e_rel,
                                                            int ngroup, int k, unsigned long long* __restrict__ out_key, int* __restrict__ out_count,
                                                            int* __restrict__ ok, int qstride, const float4* __restrict__ rowmajor) {
    gemm_rerank_list_<true>(lists, counts, tau, radius, gal4, queries, qnorm, gnorm_max_p, n, d, dp4, row_offset, e_rel, ngroup, k, out_key, out_count, ok, qstride,
                            rowmajor);
}
