// fir_gemm_i8.h -- the int8 nomination of large L2 top-1 batches (included by fir_gemm.hip, inside its anonymous namespace): the
// int8 copy of the gallery and the preparation of an int8 super-batch. The pass itself is k_gemm_proxy_f16x<.., I8 = 1>
// (fir_gemm_f16x.h); the re-rank and its certificate are the fp16 flow's, given the numbers of this file.
//
// L2 distance does not change when one vector is taken off both sides, so rows and queries are CENTRED with the gallery's column
// means first: mu[k] = mean_r g[r][k] (any f32 vector is sound; the mean is what makes the numbers small), c_g = fl(g - mu),
// c_q = fl(q - mu). One scale for the gallery, s_g = 127 / max|c_g|, one per query, s_q = 127 / max|c_q|; g8 = clamp(rint(s_g c_g)),
// q8 = clamp(rint(s_q c_q)). With g' = g8 / s_g and q' = q8 / s_q (reals) the pass computes
//     p = fl(gnorm_c - m2 * S),   S = sum q8 g8 (exact, |S| < 2^24),   m2 = 2 fl(1 / fl(s_q s_g)),   gnorm_c = |c_g|^2 in f32
// and the claim the windows and the certificate rest on is, with qnorm_c = |c_q|^2 in f32, d D the reference's sum of squares:
//     |(qnorm_c + p) - d D| <= eabs_q + e_rel (qnorm_c + G^2),     G^2 = max_r gnorm_c
//   quantisation   2 |q'.g' - c_q.c_g| = 2 |c_q.(g' - c_g) + (q' - c_q).c_g + (q' - c_q).(g' - c_g)|
//                  <= 2 (|c_q| R + e_q (G + R)) =: eabs_q  (Cauchy-Schwarz; R = max_r |g' - c_g|, e_q = |q' - c_q|: both MEASURED, in
//                  f64, and rounded up; evaluated in f32 and inflated by 1e-4 for that evaluation and for qnorm_c's own rounding)
//   centring       c = fl(x - mu) is within u |c| of x - mu per coordinate: |c_q - c_g|^2 moves by <= 4 u (|c_q|^2 + |c_g|^2)
//   m2             two roundings: 2 u * 2 |q'.g'| <= 2 u (|q'|^2 + |g'|^2) <= 3 u (qnorm_c + G^2)   (|q' - c_q| <= 0.13 |c_q| for d <= 1024)
//   the two norms  (d + 1) u each, of |c_q|^2 and |c_g|^2
//   fma, add       fl(gnorm_c - m2 S) and the certificate's qnorm_c + p: 2 roundings of numbers <= 2.3 (qnorm_c + G^2)
//   the reference  its d + 3 roundings of a sum <= 2 (|c_q|^2 + |c_g|^2) (translation invariant): (2 d + 6) u
// i.e. (4 + 3 + (d + 1) + 2 * 2.3 + 2 d + 6) u = (3 d + 18.6) u (1 + small) relative to qnorm_c + G^2, and e_rel = 8 d u covers it
// for every d >= 8 with room. All of it assumes ordinary (normal, finite) f32 numbers: k_gemm_qprep_i8 leaves a query to the exact scan
// unless s_q and fl(s_q s_g) both lie in (1e-30, 1e30).
// tests/test_gemm_int8_formulation.py restates all of this in numpy float64.
#pragma once

// device words of the int8 copy (float[8]): [0] max|c_g| (float bits, atomicMax), [1] s_g (NaN: a non-finite or degenerate gallery,
// every query is left to the exact scan), [2] G^2 (bits, atomicMax), [3] R (bits, atomicMax)
constexpr int kI8Slices = 64;           // row slices of the column sums

__device__ __forceinline__ float f64_up_to_f32_(double v) {      // the smallest f32 >= v, then one more part in 10^6
    float f = (float)v;
    if ((double)f < v) f = __uint_as_float(__float_as_uint(f) + 1u);      // (v >= 0: the next float up)
    return f + f * 1e-6f;
}
__device__ __forceinline__ int quant_i8_(float x, float s) {
    float v = __builtin_rintf(s * x);
    v = v == v ? v : 0.f;
    return (int)fminf(fmaxf(v, -127.f), 127.f);
}

// partial[(slice * d4 + c) * 4 + j] = sum of feature 4 c + j over the rows of the slice (f64); grid (d4, kI8Slices)
__global__ void __launch_bounds__(256) k_i8_colsum(const float4* __restrict__ gal4, int64_t tiles, int dp4, double* __restrict__ partial) {
    __shared__ double red[4][4];
    const int c = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t t0 = tiles * blockIdx.y / gridDim.y, t1 = tiles * (blockIdx.y + 1) / gridDim.y;
    double s[4] = {0., 0., 0., 0.};
    for (int64_t t = t0 + wave; t < t1; t += 4) {
        const float4 g = gal4[((size_t)t * dp4 + c) * 64 + lane];      // (rows past n are zero in the tiled gallery)
        s[0] += (double)g.x; s[1] += (double)g.y; s[2] += (double)g.z; s[3] += (double)g.w;
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) s[j] += __shfl_xor(s[j], off, 64);
        if (lane == 0) red[wave][j] = s[j];
    }
    __syncthreads();
    if (threadIdx.x < 4) partial[((size_t)blockIdx.y * gridDim.x + c) * 4 + threadIdx.x] = red[0][threadIdx.x] + red[1][threadIdx.x] + red[2][threadIdx.x] + red[3][threadIdx.x];
}
__global__ void __launch_bounds__(256) k_i8_mean(const double* __restrict__ partial, int d4, int d, int64_t n, float* __restrict__ mu, float* __restrict__ par) {
    const int k = blockIdx.x * 256 + threadIdx.x;
    if (k == 0) { par[0] = 0.f; par[2] = 0.f; par[3] = 0.f; }
    if (k >= d4 * 4) return;
    double s = 0.;
    for (int sl = 0; sl < kI8Slices; ++sl) s += partial[(size_t)sl * d4 * 4 + k];
    mu[k] = k < d ? (float)(s / (double)n) : 0.f;
}

// One thread per row. PASS 0: gnorm_c[row] = |c_g|^2, the maxima of |c_g[k]| and of the norms. PASS 1: the row's measured residual
// |g8 / s_g - c_g| in f64, its maximum rounded up.
template <int PASS>
__global__ void __launch_bounds__(256) k_i8_rows(const float4* __restrict__ gal4, int64_t n, int dp4, int d, const float* __restrict__ mu,
                                                  float* __restrict__ gnorm_c, float* __restrict__ par) {
    const int64_t row = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const float s_g = PASS == 1 ? par[1] : 0.f;
    float s = 0.f, m = 0.f;
    double r2 = 0.;
    bool bad = false;
    if (row < n) {
        const int d4 = (d + 3) >> 2;
        for (int c = 0; c < d4; ++c) {
            const float4 g = gal4[((row >> 6) * dp4 + c) * 64 + (row & 63)];
            const float gv[4] = {g.x, g.y, g.z, g.w};
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                if (4 * c + j >= d) continue;
                const float x = gv[j] - mu[4 * c + j];
                if (PASS == 0) {
                    s += x * x;
                    m = fmaxf(m, fabsf(x));
                    bad = bad || !(fabsf(x) < __builtin_huge_valf());
                } else {
                    const double t = (double)quant_i8_(x, s_g) / (double)s_g - (double)x;
                    r2 += t * t;
                }
            }
        }
        if (PASS == 0) gnorm_c[row] = s;
    }
    if (PASS == 0) {
        m = bad ? __builtin_huge_valf() : m;
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) {
            m = fmaxf(m, __shfl_xor(m, off, 64));
            s = fmaxf(s, __shfl_xor(s, off, 64));
        }
        if ((threadIdx.x & 63) == 0) {                                  // non-negative floats order like their bits
            atomicMax((unsigned int*)&par[0], __float_as_uint(m));
            atomicMax((unsigned int*)&par[2], __float_as_uint(s));
        }
    } else {
        float r = row < n ? f64_up_to_f32_(sqrt(r2)) : 0.f;
        r = r == r ? r : __builtin_huge_valf();
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) r = fmaxf(r, __shfl_xor(r, off, 64));
        if ((threadIdx.x & 63) == 0) atomicMax((unsigned int*)&par[3], __float_as_uint(r));
    }
}
// s_g from max|c_g|: a constant gallery (max = 0) packs zeros at scale 1 with R = 0; a scale outside [1e-30, 1e30] or a non-finite
// gallery value gives NaN
__global__ void k_i8_scale(float* __restrict__ par) {
    const float mx = par[0];
    float s = mx == 0.f ? 1.f : 127.f / mx;
    if (!(s > 1e-30f && s < 1e30f)) s = __builtin_nanf("");
    par[1] = s;
}

// c_g -> g8 in the 16-row piece order: piece 2 kk + s of row block rb, lane l: row 32 rb + 16 s + (l & 15), features
// 64 kk + 16 (l >> 4) + 0..15 as sixteen bytes (feature j in byte j); zero beyond n and d
__global__ void __launch_bounds__(256) k_i8_pack_gallery(const float4* __restrict__ gal4, int64_t n, int dp4, int dk8, int d, const float* __restrict__ mu,
                                                          const float* __restrict__ par, uint4* __restrict__ g8) {
    const int64_t o = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t rblocks = (n + 31) / 32;
    if (o >= rblocks * dk8 * 64) return;
    const int l = (int)(o & 63);
    const int64_t t = o >> 6;
    const int piece = (int)(t % dk8);
    const int64_t rb = t / dk8;
    const int kk = piece >> 1, s = piece & 1;
    const int64_t row = rb * 32 + 16 * s + (l & 15);
    const float s_g = par[1];
    unsigned int w[4] = {0u, 0u, 0u, 0u};
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        const int k0 = 64 * kk + 16 * (l >> 4) + 4 * c;
        if (row < n && k0 < d) {
            const float4 g = gal4[((row >> 6) * dp4 + (k0 >> 2)) * 64 + (row & 63)];
            const float gv[4] = {g.x, g.y, g.z, g.w};
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (k0 + j < d) w[c] |= ((unsigned int)quant_i8_(gv[j] - mu[k0 + j], s_g) & 0xFFu) << (8 * j);
        }
    }
    g8[o] = make_uint4(w[0], w[1], w[2], w[3]);
}

// Per query slot (one wave each) of an int8 super-batch: c_q, qnorm_c, s_q (-> qmul), qinv = 1 / (s_q s_g), the measured residual
// e_q, eabs_q, the adaptive pass's window and start value, the cleared count -- what k_gemm_qprep_f16 does for the fp16 flow. A
// query (or a gallery scale) that yields anything non-finite gets a NaN norm, scale and window: nothing is certified for it.
// list != NULL (a second-chance round, as k_gemm_sc_prep): slot i stands for query list[live_off + i] of the call, its bound is
// tau2_all[that query], the padding slots append nothing; win / t_bits are then not written.
__global__ void __launch_bounds__(64) k_gemm_qprep_i8(const float* __restrict__ q, int nq, int d, int qstride, const float* __restrict__ mu,
                                                       const float* __restrict__ par, float e_rel, float eabs_scale, float* __restrict__ qnorm,
                                                       float* __restrict__ qmul, float* __restrict__ qinv, float* __restrict__ eabs, int* __restrict__ counts,
                                                       float* __restrict__ win, unsigned int* __restrict__ t_bits, int* __restrict__ fb_state,
                                                       const int* __restrict__ state, const int* __restrict__ list, int live_off,
                                                       const float* __restrict__ tau2_all, float* __restrict__ tau) {
    const int slot = blockIdx.x;
    int qi = slot;
    if (list) {
        int live = state[0] - live_off;
        if (live <= 0) return;                                          // (uniform: nothing of this round runs)
        nq = live < kScQueries ? live : kScQueries;
        qi = slot < nq ? list[live_off + slot] : 0;
    }
    if (fb_state && threadIdx.x == 0 && slot == 0) { fb_state[0] = 0; fb_state[1] = 0; }
    const bool valid = slot < nq;
    float s = 0.f, m = 0.f;
    bool bad = false;
    if (valid)
        for (int k = threadIdx.x; k < d; k += 64) {
            const float x = q[(size_t)qi * qstride + k] - mu[k];
            s += x * x;
            m = fmaxf(m, fabsf(x));
            bad = bad || !(fabsf(x) < __builtin_huge_valf());
        }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        s += __shfl_xor(s, off, 64);
        m = fmaxf(m, __shfl_xor(m, off, 64));
    }
    bad = __any(bad);
    const float s_g = par[1];
    float s_q = m > 0.f ? 127.f / m : 1.f;
    // (the product too: s_q and s_g inside their own guards can still multiply to inf -- qinv = 0, every p = gnorm_c -- or to a
    // subnormal qinv of a few bits, and the bound's m2 term assumes two ordinary roundings. Inside (1e-30, 1e30) the product and
    // qinv are normal with eight decades of room, and max|c_q| max|c_g| > 1.6e-26 keeps qnorm_c + G^2 normal as well.)
    const float s_qg = s_q * s_g;
    if (!(s_q > 1e-30f && s_q < 1e30f) || !(s_qg > 1e-30f && s_qg < 1e30f)) bad = true;      // (a NaN s_g fails the second test)
    if (bad) s_q = 0.f;
    double r2 = 0.;
    if (valid && !bad)
        for (int k = threadIdx.x; k < d; k += 64) {
            const float x = q[(size_t)qi * qstride + k] - mu[k];
            const double t = (double)quant_i8_(x, s_q) / (double)s_q - (double)x;
            r2 += t * t;
        }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) r2 += __shfl_xor(r2, off, 64);
    if (threadIdx.x == 0) {
        const float nan = __builtin_nanf("");
        const float qn = (bad && valid) ? nan : s;
        const float e_q = f64_up_to_f32_(sqrt(r2));
        const float R = par[3], gmax = par[2];
        const float G = sqrtf(gmax) * (1.0f + 2e-7f);
        const float ea = (bad && valid) ? nan : eabs_scale * ((2.0f * (sqrtf(s) * (1.0f + 2e-7f) * R + e_q * (G + R))) * (1.0f + 1e-4f));
        qnorm[slot] = qn;
        qmul[slot] = s_q;
        qinv[slot] = !valid ? 0.f : bad ? nan : 1.0f / s_qg;
        eabs[slot] = ea;
        counts[slot] = 0;
        if (list) tau[slot] = valid ? tau2_all[qi] : -__builtin_huge_valf();
        if (win) {
            win[slot] = valid ? nudge_up_(rounding_window_(e_rel, qn, gmax, ea)) : 0.f;
            atomicExch(&t_bits[slot], valid ? 0x7F800000u : 0u);
        }
    }
}

// c_q * s_q -> q8 in the 16-row piece order (k_gemm_pack_queries_f16x's layout with 64-feature steps; dk8 / 2 steps); the same
// expression as k_gemm_qprep_i8 measured. blockIdx.y = pair; qmap as there.
__global__ void __launch_bounds__(256) k_gemm_pack_queries_i8(const float* q, int nq, int d, int dk8, const float* __restrict__ mu, const float* __restrict__ qmul,
                                                               uint4* q8, int qstride, const int* __restrict__ qmap = nullptr,
                                                               const int* __restrict__ state = nullptr, int live_off = 0) {
    if (qmap) {
        nq = state[0] - live_off;
        if (nq <= 0) return;
        nq = nq < 2 * kQT ? nq : 2 * kQT;
    }
    const int steps = dk8 >> 1;
    const int q_base = (int)blockIdx.y * 2 * kQT;
    q8 += (size_t)blockIdx.y * 8 * steps * 64;
    const int o = blockIdx.x * 256 + threadIdx.x;
    if (o >= 8 * steps * 64) return;
    const int l = o & 63;
    const int t = o >> 6;
    const int kk = t % steps, jb = t / steps;
    const int qi = q_base + jb * 16 + (l & 15);
    const float mul = qi < nq ? qmul[qi] : 0.f;
    unsigned int w[4] = {0u, 0u, 0u, 0u};
    if (qi < nq) {
        const float* src = q + (size_t)(qmap ? qmap[qi] : qi) * qstride;
#pragma unroll
        for (int j = 0; j < 16; ++j) {
            const int k = 64 * kk + 16 * (l >> 4) + j;
            if (k < d) w[j >> 2] |= ((unsigned int)quant_i8_(src[k] - mu[k], mul) & 0xFFu) << (8 * (j & 3));
        }
    }
    q8[o] = make_uint4(w[0], w[1], w[2], w[3]);
}
