// fir_gemm_rerank.h -- what every exact re-rank of the matrix-core path is built from (included by fir_gemm.hip, inside its
// anonymous namespace): the rounding windows, the walk over a query's candidate list, the exact f32 distances of the rows inside
// the window, the certificate, and the hand-over of an uncertified query to the second pass (fir_gemm_fb.h). Each piece exists
// once; k_gemm_rerank<KMAX> and k_gemm_rerank_classes (fir_gemm.hip) and k_gemm_rerank_f64 (fir_gemm_f64.h) are made of them, and
// tests/gemm_f16_form.py restates them in numpy.
//
// The translation unit is built with -ffp-contract=off: every helper below performs exactly the float operations it spells out,
// in that order.
#pragma once

constexpr int kTopKMax = 8;             // the K nearest rows: K at most this

// One rounding window in proxy units, with room: 2.5 E d against the re-rank's own 2 E d (rerank_window_).
__device__ __forceinline__ float rounding_window_(float e_rel, float qn, float gmax) { return 2.5f * e_rel * (qn + gmax); }
// ... with a per-query ABSOLUTE term next to the relative one (the int8 nomination, fir_gemm_i8.h: eabs_q, the measured
// quantisation residuals; already in proxy units). The forms without it are what every fp16, bf16 and f32 flow computes.
__device__ __forceinline__ float rounding_window_(float e_rel, float qn, float gmax, float eabs) { return 2.5f * (e_rel * (qn + gmax) + eabs); }
// A bound moved up by a relative 1e-6 (and off zero), so that ties with it are still below it.
__device__ __forceinline__ float nudge_up_(float v) { return v + fabsf(v) * 1e-6f + 1e-30f; }

// device words of one fir_gemm (int[kFbStateWords]): [0] count, [1] count2 -- cleared at the start of every call --, [2] notes taken,
// [4..5] and [6..7]: running totals (64-bit) of queries that took a second pass / the exact device scan, [8..39]: four floats for each
// of the first eight uncertified queries of the state's life (fir_gemm_uncertified_notes)
constexpr int kFbStateWords = 40;
__device__ __forceinline__ void fb_note(int* state, int cnt, float bound, float smallest, float qn) {
    if (state[2] < 8) {                                            // (racy on purpose: a cheap filter in front of the atomic)
        const int i = atomicAdd(&state[2], 1);
        if (i < 8) {
            float* o = (float*)(state + 8) + 4 * i;
            o[0] = (float)cnt; o[1] = bound; o[2] = smallest; o[3] = qn;
        }
    }
}
struct RerankFb {
    int* state;          // the state words above
    int* list;           // first pass: uncertified queries are appended here (index within the call)
    float* tau2;         // first pass: [query of the call] the bound the second-chance pass appends below
    int q_base;          // first pass: index within the call of block 0's query
    const int* qmap;     // second chance: block b re-ranks scratch slot b for query qmap[b] of the call ...
    int live_off;        // ... while b < state[0] - live_off
};

// The window of the re-rank, hung on an anchor proxy (the smallest of the list; the K-th smallest for the K nearest rows or
// classes; +inf when the list is too short for that: everything is re-ranked).
// Each proxy is within E d of its row's true |g|^2 - 2 q.g, so a row whose proxy exceeds the anchor by more than 2 E d cannot
// beat the row that has the anchor's proxy: the window [anchor, anchor + 2 E d] holds every possible winner -- a handful of rows on
// ordinary data, all the near-duplicates on clustered data (a fixed number of candidates, as used before, could not certify
// those and sent them to the exact scan). The window is only how candidates are CHOSEN; what proves the answer is the
// certificate at the end (rerank_certified_), which is independent of that reasoning.
// E bounds every rounding on both sides, in distance units: the f32 fma chain of the dot product (<= d u |q||g|,
// doubled), the two float norms (<= d u each), the reference's own d+3 roundings of the (q-g)^2 sum and its divide:
// (4d + 11) u (|q|^2 + |g|^2) / d in total; 8 d u (...) / d is used.  u = 2^-24.
// e_rel = 8 d u, plus 2^-14 for the bf16-split variant (dropped lo.lo / residual terms, 3 * 2^-18 |g||q|, doubled in p)
// or 2^-10 (1 + 2^-4) for the single fp16 term (both operands rounded to 11 bits)
struct RerankWindow {
    float E;             // the certificate's error bound, distance units
    float win;           // entries with a proxy <= win are re-ranked
};
__device__ __forceinline__ RerankWindow rerank_window_(float e_rel, float qn, float gmax, int d, float anchor) {
    const float E = e_rel * (qn + gmax) / (float)d;
    float win = anchor + 2.0f * E * (float)d;
    win += fabsf(win) * 1e-6f;
    return {E, win};
}

__device__ __forceinline__ RerankWindow rerank_window_(float e_rel, float qn, float gmax, int d, float anchor, float eabs) {
    const float E = (e_rel * (qn + gmax) + eabs) / (float)d;
    float win = anchor + 2.0f * E * (float)d;
    win += fabsf(win) * 1e-6f;
    return {E, win};
}

// The k-th smallest of the list's `have` keys (keys are unique: the row is part of the key): k rounds of "smallest key above the
// previous". found = how many rounds found one; the key of the last such round is returned (kKeyNone: an empty list).
__device__ __forceinline__ unsigned long long list_kth_smallest_(const unsigned long long* __restrict__ L, int have, int k, int lane, int& found) {
    unsigned long long prev = 0, kth = kKeyNone;
    found = 0;
    for (int r = 0; r < k; ++r) {
        unsigned long long m = kKeyNone;
        for (int i = lane; i < have; i += 64) {
            const unsigned long long v = L[i];
            if ((r == 0 || v > prev) && v < m) m = v;
        }
        m = fir::wave_min_u64(m);
        if (m == kKeyNone) break;
        prev = m;
        kth = m;
        ++found;
    }
    return kth;
}

// The walk over the list, 64 entries at a time: body(base, v, in, mask) gets the lane's entry v = L[base + lane] (kKeyNone past the
// end), whether it lies in the window, and the wave's ballot of that. Returns the smallest proxy NOT re-ranked (over the whole
// wave) and how many entries were.
struct RerankWalk {
    float p_out;
    int reranked;
};
template <class Body>
__device__ __forceinline__ RerankWalk rerank_walk_(const unsigned long long* L, int have, float win, int lane, Body body) {
    float p_out = __builtin_huge_valf();
    int reranked = 0;
    for (int base = 0; base < have; base += 64) {
        const int i = base + lane;
        const unsigned long long v = i < have ? L[i] : kKeyNone;
        const float p = fir::f32_from_orderable((uint32_t)(v >> 32));
        const bool in = i < have && p <= win;
        if (i < have && !in) p_out = fminf(p_out, p);
        const unsigned long long mask = __ballot(in);
        reranked += __popcll(mask);
        body(base, v, in, mask);                                        // (mask is wave-uniform)
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) p_out = fminf(p_out, __shfl_xor(p_out, off, 64));
    return {p_out, reranked};
}

// The f32 forms' dynamic LDS: [ngroup][cs] candidate rows, loaded by the whole wave, then [dp4] the query, zero-padded like the
// gallery rows (a (0-0)^2 term adds +0).
struct RerankLds {
    float4* crow;
    const float4* qrow;
    int cs;              // candidate-row stride, odd: the lanes' rows start in different banks
};
__device__ __forceinline__ RerankLds rerank_lds_f32_(float4* crow, int ngroup, int dp4, int d, const float* __restrict__ qv, int lane) {
    const int cs = dp4 | 1;
    float4* qrow = crow + (size_t)ngroup * cs;
    for (int k = lane; k < dp4 * 4; k += 64) ((float*)qrow)[k] = k < d ? qv[k] : 0.0f;
    __syncthreads();
    return {crow, qrow, cs};
}

// One batch of the walk, f32 rows: up to ngroup (<= kRerankGroup) candidates of `mask` at a time -- all lanes fetch their rows into
// LDS (the row-major shadow copy when there is one: one contiguous row, coalesced; else the tiled gallery: 16 bytes per KiB), then
// lane g re-computes candidate g's distance from there: db_features.cpp:22-42 order, un-fused (fir::accum<kL2>), one division.
// sink(i, key, dist): list index and list key (proxy, local row) of the lane's candidate and its exact distance.
template <class Sink>
__device__ __forceinline__ void rerank_gather_f32_(unsigned long long mask, unsigned long long v, int base, int lane, int ngroup, const RerankLds& lds,
                                                   const float4* __restrict__ gal4, const float4* __restrict__ rowmajor, int dp4, int d, Sink sink) {
    const int d4 = (d + 3) >> 2;                                  // float4 chunks of the compared features (a prefix of the row when d < its length)
    while (mask) {                                                  // wave-uniform
        unsigned long long mine = kKeyNone;
        int mine_i = 0, ng = 0;
        for (int g = 0; g < ngroup; ++g) {
            if (mask) {
                const int src = __ffsll((long long)mask) - 1;
                mask &= mask - 1;
                const unsigned long long cv = __shfl((unsigned long long)v, src, 64);
                const int64_t row = (int64_t)(uint32_t)(cv & 0xFFFFFFFFull);
                if (rowmajor) {
                    const float4* gr = rowmajor + (size_t)row * d4;
                    for (int c = lane; c < d4; c += 64) lds.crow[(size_t)g * lds.cs + c] = gr[c];
                } else {
                    const float4* gr = gal4 + (size_t)(row >> 6) * dp4 * 64 + (row & 63);
                    for (int c = lane; c < d4; c += 64) lds.crow[(size_t)g * lds.cs + c] = gr[(size_t)c * 64];
                }
                if (lane == g) { mine = cv; mine_i = base + src; }
                ++ng;
            }
        }
        __syncthreads();
        if (lane < ng) {
            const float4* my = lds.crow + (size_t)lane * lds.cs;
            float acc = 0.0f;
            for (int c = 0; c < d4; ++c) {
                const float4 g4 = my[c], q4 = lds.qrow[c];
                acc = fir::accum<fir::kL2>(acc, q4.x, g4.x);
                acc = fir::accum<fir::kL2>(acc, q4.y, g4.y);
                acc = fir::accum<fir::kL2>(acc, q4.z, g4.z);
                acc = fir::accum<fir::kL2>(acc, q4.w, g4.w);
            }
            sink(mine_i, mine, acc / (float)d);
        }
        __syncthreads();
    }
}

// Certificate. Every row NOT re-ranked has a proxy >= p_excl: the smallest list entry outside the window, or tau for rows that
// were never appended. Its reference distance is then >= (|q|^2 + p_excl)/d - E: above the K-th exact distance found (strict '>':
// no tie with it either), no such row belongs to the answer. With fewer than K found (have_kth false) any row below the
// reference's cut-off -- T = float: 100000; double: none, +inf -- outside the re-ranked set would belong to it.
// T: the arithmetic of the exact distances, which the bound is formed in.
template <typename T>
__device__ __forceinline__ bool rerank_certified_(int cnt, float tau, float p_out, float qn, int d, float E, bool have_kth, T kth_dist, int64_t n,
                                                  int reranked) {
    if (cnt > kListCap) return false;                           // rows below tau were dropped from the list
    const float p_excl = tau != tau ? tau : fminf(p_out, tau);  // a NaN bound must not certify anything
    const T lower = ((T)qn + (T)p_excl) / (T)d - (T)E;
    const T none = sizeof(T) == sizeof(float) ? (T)fir::kNotFound : (T)__builtin_huge_val();
    const T bd = have_kth ? kth_dist : none;
    return lower > bd || n <= reranked;                         // (false for NaN; every row was re-ranked)
}

// An uncertified query of a first pass goes on the call's list with the bound a second pass may append below: min(this pass's
// bound, anchor + one window). The anchor is the (K-th) smallest stored proxy, at or above the (K-th) smallest proxy of ALL rows (a
// stored proxy is some row's), so that list will hold every possible winner. NaN bounds stay NaN (nothing is appended, nothing
// certified: the exact scan answers).
// eabs != NULL: the windows carry the query's absolute term (above).
__device__ __forceinline__ void rerank_hand_over_(const RerankFb& fb, int q, int cnt, float tau, float anchor, float qn, float gmax, float e_rel,
                                                  const float* eabs = nullptr) {
    const float c = anchor + nudge_up_(eabs ? rounding_window_(e_rel, qn, gmax, eabs[q]) : rounding_window_(e_rel, qn, gmax));
    fb.tau2[fb.q_base + q] = c < tau ? c : tau;
    fb.list[atomicAdd(&fb.state[0], 1)] = fb.q_base + q;
    fb_note(fb.state, cnt, tau, anchor, qn);
}
