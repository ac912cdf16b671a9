// fir_twd_batch.h -- the kernels of fir_twd_conventional's matrix-core batch form (type 0, L2). Included by fir_twd.hip inside its
// unnamed namespace, behind posterior() and kLastFeature; the driver (conv_mfma) is there too.
//
// Both stages of ConventionalTWDClassifier::recognize (ImageTesting.cpp:108-186) are selections the matrix-core searches answer with
// the exact scan's bits: the first stage needs the five nearest DISTINCT classes over [0, reduced) (exp is non-increasing: the five
// largest class posteriors belong to the five smallest class distances), the second stage the row with the smallest
// v = (d1 * reduced + d2 * (256 - reduced)) / 256, which is the distance over [0, 256) up to rounding: the eight nearest rows over
// [0, 256) nominate, the reference's arithmetic decides among them, a certificate proves no other row can win.
#pragma once

enum { kVerdictReliable = 0, kVerdictUnreliable = 1, kVerdictStaged = 2 };
constexpr int kMfmaClasses = 5;    // top-5 posteriors (ImageTesting.cpp:141-146)
constexpr int kMfmaRows = 8;       // rows nominated for the second stage
// A verdict is taken from k_twd_batch_decide only when max_probab is further than this (relative) from the threshold: the kernel sums the
// posteriors of five class MINIMA, k_twd_conv_stage1 the maxima of every row's posterior -- the same numbers unless exp() rounds against
// its monotonicity somewhere, a difference of a few 2^-53 in five terms, thousands of times below the band.
constexpr double kMfmaBand = 0x1p-40;
// Second-stage certificate: dist(key[7]) * (1 - kMfmaCertRel) - kMfmaCertAbs > v_best. d_256 and v of one row are both within
// gamma_259 = 259 u / (1 - 259 u), u = 2^-24, of the real mean of its 256 squared differences, so a row outside the eight has
// v >= key[7] (1 - gamma) / (1 + gamma) >= key[7] (1 - 2^-14.9); squares that underflow add at most 2^-149 each.
constexpr double kMfmaCertRel = 0x1p-14;
constexpr double kMfmaCertAbs = 256.0 * 0x1p-149;

// keys / classes [nq][5]: fir_search_top_classes' answer over [0, reduced), ascending by (distance, row); absent slots kKeyNone / -1.
// The arithmetic of k_twd_conv_stage1's last step on the class minima: absent slots count 0 like the zero-initialised `probabs`, the
// sum is taken in descending order of the posteriors. class_out[q] <- the class of the nearest row (final for a reliable query).
__global__ void __launch_bounds__(kBlock) k_twd_batch_decide(const unsigned long long* __restrict__ keys, const int32_t* __restrict__ classes, int nq,
                                                             double threshold, int32_t* __restrict__ class_out, int32_t* __restrict__ verdict) {
    const int q = blockIdx.x * kBlock + threadIdx.x;
    if (q >= nq) return;
    const unsigned long long k0 = keys[(size_t)q * kMfmaClasses];
    double sum = 0.0;
#pragma unroll
    for (int j = 0; j < kMfmaClasses; ++j) {
        const unsigned long long kj = keys[(size_t)q * kMfmaClasses + j];
        sum += kj != fir::kKeyNone ? posterior((double)fir::f32_from_orderable((uint32_t)(kj >> 32))) : 0.0;
    }
    int v = kVerdictStaged;                                             // no row below 100000, a zero sum, a NaN, the band: the staged form
    if (k0 != fir::kKeyNone && sum > 0.0) {
        const double best_d = (double)fir::f32_from_orderable((uint32_t)(k0 >> 32));
        const double max_probab = exp(-best_d * 100) / sum;             // :130,147
        if (fabs(max_probab - threshold) > fabs(threshold) * kMfmaBand) v = max_probab > threshold ? kVerdictReliable : kVerdictUnreliable;   // :148
    }
    class_out[q] = classes[(size_t)q * kMfmaClasses];
    verdict[q] = v;
}

// One workgroup: the unreliable queries and the queries marked for the staged form, each in query order.
// lists[0] = unreliable count, lists[1] = staged count, lists[2 .. 2 + nq) the unreliable queries, lists[2 + nq ..) the staged ones;
// pos[q] = place of query q among the unreliable ones, -1 for the others.
__global__ void __launch_bounds__(kBlock) k_twd_batch_compact(const int32_t* __restrict__ verdict, int nq, int32_t* __restrict__ lists,
                                                              int32_t* __restrict__ pos) {
    __shared__ int wave_u[kBlock / 64], wave_s[kBlock / 64];
    __shared__ int base_u, base_s;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (threadIdx.x == 0) { base_u = 0; base_s = 0; }
    __syncthreads();
    for (int b = 0; b < nq; b += kBlock) {
        const int q = b + threadIdx.x;
        const int v = q < nq ? verdict[q] : kVerdictReliable;
        const unsigned long long mu = __ballot(v == kVerdictUnreliable), ms = __ballot(v == kVerdictStaged);
        if (lane == 0) { wave_u[wave] = __popcll(mu); wave_s[wave] = __popcll(ms); }
        __syncthreads();
        int off_u = base_u, off_s = base_s;
        for (int w = 0; w < wave; ++w) { off_u += wave_u[w]; off_s += wave_s[w]; }
        const unsigned long long below = (1ull << lane) - 1ull;
        if (q < nq) {
            int p = -1;
            if (v == kVerdictUnreliable) { p = off_u + __popcll(mu & below); lists[2 + p] = q; }
            if (v == kVerdictStaged) lists[2 + nq + off_s + __popcll(ms & below)] = q;
            pos[q] = p;
        }
        __syncthreads();
        if (threadIdx.x == 0) {
            for (int w = 0; w < kBlock / 64; ++w) { base_u += wave_u[w]; base_s += wave_s[w]; }
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) { lists[0] = base_u; lists[1] = base_s; }
}

// blockIdx.x = query: an unreliable query's vector goes to row pos[q] of `dst` (d floats per row on both sides).
__global__ void __launch_bounds__(64) k_twd_batch_gather(const float* __restrict__ queries, const int32_t* __restrict__ pos, int d, float* __restrict__ dst) {
    const int p = pos[blockIdx.x];
    if (p < 0) return;
    const float* src = queries + (size_t)blockIdx.x * d;
    float* out = dst + (size_t)p * d;
    for (int c = threadIdx.x; c < d; c += 64) out[c] = src[c];
}

// The second stage (ImageTesting.cpp:165-180) among the nominated rows. One wave per unreliable query i (blockIdx.x), queries[i] its
// vector, keys[i][8] its eight nearest rows over [0, 256) (fir_search_topk's keys: exact, ascending, index + row_offset).
// The rows are staged in LDS from the tiled gallery (lane = 16-byte chunk: a row's 256 compared features are 64 chunks), then lane g < 8
// walks row g in feature order: d1 over [0, reduced), d2 over [reduced, 256), each a float sum divided by its count -- the bits of the
// scan's range distances --, v exactly as k_twd_conv_stage1 forms it, and the first minimum by (v, row) with the strict '<' from 100000.
// ok[i] <- 1 and class_out[unrel[i]] <- the class of that row when the certificate holds (kMfmaCertRel), ok[i] <- 0 otherwise: fewer
// than eight keys, eight or more rows inside the window (duplicates), a row index outside the gallery, a NaN.
__global__ void __launch_bounds__(64) k_twd_batch_stage2(const float4* __restrict__ gal4, int dp4, int64_t n, int64_t row_offset,
                                                         const int32_t* __restrict__ cls, const float* __restrict__ queries, int d, int reduced,
                                                         const unsigned long long* __restrict__ keys, const int32_t* __restrict__ unrel,
                                                         int32_t* __restrict__ class_out, int32_t* __restrict__ ok) {
    constexpr int kChunks = kLastFeature / 4, kStride = kChunks | 1;     // odd stride: the eight walking lanes start in different banks
    __shared__ float4 crow[kMfmaRows * kStride];
    __shared__ float4 qrow[kChunks];
    const int i = blockIdx.x, lane = threadIdx.x;
    const float* qv = queries + (size_t)i * d;
    qrow[lane] = make_float4(qv[4 * lane], qv[4 * lane + 1], qv[4 * lane + 2], qv[4 * lane + 3]);
    const unsigned long long mykey = lane < kMfmaRows ? keys[(size_t)i * kMfmaRows + lane] : fir::kKeyNone;
    const int64_t myrow = (int64_t)(uint32_t)(mykey & 0xFFFFFFFFull) - row_offset;
    const bool have = mykey != fir::kKeyNone && myrow >= 0 && myrow < n;
    const unsigned long long have_mask = __ballot(have);
    for (int g = 0; g < kMfmaRows; ++g) {                               // wave-uniform
        if (!((have_mask >> g) & 1ull)) continue;
        const int64_t row = __shfl((long long)myrow, g, 64);
        crow[g * kStride + lane] = gal4[((size_t)(row >> 6) * dp4 + lane) * 64 + (row & 63)];
    }
    __syncthreads();
    double v = 100000.0;                                                // bestDist = 100000 (:168): only strictly smaller rows qualify
    unsigned int vrow = 0xFFFFFFFFu;
    if (have) {
        const float4* my = crow + lane * kStride;
        float acc1 = 0.0f, acc2 = 0.0f;
        const int r4 = reduced >> 2;
        for (int c = 0; c < r4; ++c) {
            const float4 g4 = my[c], q4 = qrow[c];
            acc1 = fir::accum<fir::kL2>(acc1, q4.x, g4.x);
            acc1 = fir::accum<fir::kL2>(acc1, q4.y, g4.y);
            acc1 = fir::accum<fir::kL2>(acc1, q4.z, g4.z);
            acc1 = fir::accum<fir::kL2>(acc1, q4.w, g4.w);
        }
        for (int c = r4; c < kChunks; ++c) {
            const float4 g4 = my[c], q4 = qrow[c];
            acc2 = fir::accum<fir::kL2>(acc2, q4.x, g4.x);
            acc2 = fir::accum<fir::kL2>(acc2, q4.y, g4.y);
            acc2 = fir::accum<fir::kL2>(acc2, q4.z, g4.z);
            acc2 = fir::accum<fir::kL2>(acc2, q4.w, g4.w);
        }
        const float d1 = acc1 / (float)reduced, d2 = acc2 / (float)(kLastFeature - reduced);      // db_features.cpp:40
        const float tail = d2 * (float)(kLastFeature - reduced);        // float * int -> float (:174)
        const double mine = ((double)d1 * reduced + tail) / kLastFeature;   // :173-174
        if (mine < v) { v = mine; vrow = (unsigned int)myrow; }
    }
#pragma unroll
    for (int off = 4; off >= 1; off >>= 1) {                            // (the lanes from 8 on hold (100000, none))
        const double ov = __shfl_xor(v, off, 64);
        const unsigned int orow = __shfl_xor(vrow, off, 64);
        if (ov < v || (ov == v && orow < vrow)) { v = ov; vrow = orow; }
    }
    if (lane == 0) {
        const unsigned long long k7 = keys[(size_t)i * kMfmaRows + kMfmaRows - 1];
        const bool all = (have_mask & 0xFFull) == 0xFFull && k7 != fir::kKeyNone;
        const double d7 = (double)fir::f32_from_orderable((uint32_t)(k7 >> 32));
        const bool certified = all && vrow != 0xFFFFFFFFu && d7 * (1.0 - kMfmaCertRel) - kMfmaCertAbs > v;      // strict: a tie, a NaN never certify
        ok[i] = certified ? 1 : 0;
        if (certified) class_out[unrel[i]] = cls[vrow];
    }
}
