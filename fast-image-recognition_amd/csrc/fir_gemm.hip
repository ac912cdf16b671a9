// fir_gemm.hip -- large-batch L2 top-1 through the matrix cores, with the reference's exact answer.
//
// The streaming scan (fir_kernels.h) is HBM-bound at 8 queries per gallery pass and VALU-bound
// beyond. For big query batches the N x Qb x d work is a GEMM: p(q, g) = |g|^2 - 2 q.g orders the
// rows of one query exactly like the squared distance does, and q.g runs on MFMA. gfx950 has an
// f32-input MFMA (v_mfma_f32_32x32x2_f32: exact products, f32 fma chain) at the f32 vector peak
// (157 TF), i.e. ONE matrix op per (row, query, feature) instead of the scan's three VALU ops.
//
// The GEMM only NOMINATES rows; the answer is still the reference's:
//   1. proxies of a row sample give, per query, an upper bound tau of its C-th smallest proxy;
//   2. the full pass appends every row with p < tau to the query's candidate list;
//   3. every appended row whose proxy lies within the rounding window of the smallest one is re-ranked
//      with the reference's own arithmetic (sequential, un-fused f32: fir::accum<kL2>), first-minimum
//      tie-break on (distance, row);
//   4. a rigorous bound certifies the winner: every other row has p >= p_excl, hence a reference
//      distance >= (|q|^2 + p_excl)/d - E, with E covering every rounding on both sides; if that does
//      not exceed the winner's exact distance (the window reaches tau, the list overflowed, NaN), the
//      query is re-run through the exact streaming scan.
// So results are bit-identical to the scan path's -- index and distance -- by construction.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/fir_amd.h"
#include "fir_internal.h"
#include "fir_common.h"
#include "fir_knn_select.h"
#include "fir_search_request.h"

namespace {

using fir::FirSearch;
using fir::kKeyNone;

#ifndef FIR_I8_AUTO_MIN_QUERIES
#define FIR_I8_AUTO_MIN_QUERIES 2048      // (0 compiles the automatic int8 rule out: gemm_wants_i8_)
#endif
#ifndef FIR_GEMM_BLOCK
#define FIR_GEMM_BLOCK 512
#endif
constexpr int kGemmBlock = FIR_GEMM_BLOCK;   // 512 = 8 waves: 2 per SIMD (one workgroup per CU: the query slab takes 128 KiB of LDS)
constexpr int kGemmMinBlocks = kGemmBlock <= 512 ? 2 : 1;
constexpr int kQT = 64;                // queries per pass (2 accumulator tiles of 32 per wave)
constexpr int kSlab8 = 64;             // query features staged in LDS at a time, in groups of 8 (512 features)
constexpr int kSlab16 = 32;            // bf16 variant: k-blocks of 16 features staged at a time (512 features)
constexpr int kPasses = 128;           // 64-query passes per super-batch at most (one set of launches, one set of scratch): 8192 queries
constexpr int kCand = 8;               // tau = the kCand-th smallest SAMPLED proxy (so ~kCand * n / sample rows get appended)
constexpr int kRerankGroup = 8;         // candidate rows staged in LDS at a time by the re-rank (fewer when rows are longer than ~4000 features)
constexpr size_t kRerankLdsMax = 144 * 1024;
constexpr int kListCap = 4096;         // appended (proxy, row) entries per query before "overflow"
constexpr int kClassSampleRows = 16384; // distinct classes: the bound comes from max(this, n K / 64) leading rows (exact class minima)
constexpr int kMinSampleRows = 8192;   // rows whose proxies seed tau: max(8192, n / 64) -> ~512 appended rows per query

typedef float f32x16 __attribute__((ext_vector_type(16)));


// MFMA operand layout shared by gallery and queries ("fragment order"): for a block of 32 vectors
// and a group kq of 8 features, lane l holds the float4
//   ( v[l&31][8kq+0+h], v[l&31][8kq+2+h], v[l&31][8kq+4+h], v[l&31][8kq+6+h] ),  h = l >> 5,
// so component i is the A (or B) operand of the MFMA that contracts features 8kq+2i, 8kq+2i+1
// (v_mfma_f32_32x32x2_f32: A[i = l&31][k = l>>5], B[k = l>>5][j = l&31]).
// tiled gallery (fir_kernels.h layout) -> fragment order + squared row norms.
__global__ void __launch_bounds__(256) k_gemm_pack_gallery(const float4* __restrict__ gal4, int64_t n, int dp4, int dq8,
                                                            float4* __restrict__ gm, float* __restrict__ gnorm) {
    const int64_t o = (int64_t)blockIdx.x * 256 + threadIdx.x;      // float4 index in gm
    const int64_t rblocks = (n + 31) / 32;
    if (o >= rblocks * dq8 * 64) return;
    const int l = (int)(o & 63);
    const int64_t t = o >> 6;
    const int kq = (int)(t % dq8);
    const int64_t rb = t / dq8;
    const int64_t row = rb * 32 + (l & 31);
    const int h = l >> 5;
    float v[4] = {0.f, 0.f, 0.f, 0.f};
    if (row < n) {
        const int64_t tile = row >> 6;
        const int r = (int)(row & 63);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int k = 8 * kq + 2 * i + h;
            if (k < dp4 * 4) {
                const float4 g = gal4[(tile * dp4 + (k >> 2)) * 64 + r];
                v[i] = (k & 3) == 0 ? g.x : (k & 3) == 1 ? g.y : (k & 3) == 2 ? g.z : g.w;
            }
        }
    }
    gm[o] = make_float4(v[0], v[1], v[2], v[3]);
    if (kq == 0 && h == 0 && row < n) {      // one thread per row: its squared norm (any summation order: covered by E)
        const int64_t tile = row >> 6;
        const int r = (int)(row & 63);
        float s = 0.f;
        for (int c = 0; c < dp4; ++c) {
            const float4 g = gal4[(tile * dp4 + c) * 64 + r];
            s += g.x * g.x + g.y * g.y + g.z * g.z + g.w * g.w;
        }
        gnorm[row] = s;
    }
}

// queries[nq][d] -> fragment order qm[jb][kq][lane] (float4), zero padded to kQT queries; qnorm[q] = |q|^2.
__global__ void __launch_bounds__(256) k_gemm_pack_queries(const float* q, int nq, int d, int dq8, float4* qm) {
    // blockIdx.y = pass: 64 queries each, packed back to back
    q += (size_t)blockIdx.y * kQT * d;
    nq -= (int)blockIdx.y * kQT;
    qm += (size_t)blockIdx.y * (kQT / 32) * dq8 * 64;
    const int o = blockIdx.x * 256 + threadIdx.x;
    if (o < (kQT / 32) * dq8 * 64) {
        const int l = o & 63;
        const int t = o >> 6;
        const int kq = t % dq8, jb = t / dq8;
        const int qi = jb * 32 + (l & 31), h = l >> 5;
        float v[4] = {0.f, 0.f, 0.f, 0.f};
        if (qi < nq) {
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int k = 8 * kq + 2 * i + h;
                if (k < d) v[i] = q[(size_t)qi * d + k];
            }
        }
        qm[o] = make_float4(v[0], v[1], v[2], v[3]);
    }
}

// qnorm[q] = |q|^2 (one wave per query; any summation order is covered by the certificate's E).
__global__ void __launch_bounds__(64) k_gemm_qnorm(const float* __restrict__ q, int nq, int d, float* __restrict__ qnorm) {
    const int qi = blockIdx.x;
    float s = 0.f;
    if (qi < nq)
        for (int k = threadIdx.x; k < d; k += 64) s += q[(size_t)qi * d + k] * q[(size_t)qi * d + k];
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) s += __shfl_xor(s, off, 64);
    if (threadIdx.x == 0) qnorm[qi] = s;
}

// One wave: 32 gallery rows x 64 queries; p = |g|^2 - 2 q.g.
// MODE 0: store the proxies of rows < sample_rows into sample[q][row] (seeding tau).
// MODE 1: append (p, row) with p < tau[q] to the query's list.
// Dynamic LDS: the query tile in fragment order, 2 * dq8 * 64 float4.
template <int MODE>
__global__ void __launch_bounds__(kGemmBlock, kGemmMinBlocks) k_gemm_proxy(const float4* __restrict__ gm, const float* __restrict__ gnorm,
                                                               const float4* qm, int64_t n, int64_t row_begin,
                                                               int64_t row_end, int dq8, const float* tau, unsigned long long* lists, int* counts, float* sample,
                                                               int sample_rows) {
    extern __shared__ __attribute__((aligned(16))) float4 lq[];
    __shared__ float tau_s[kQT];
    {   // blockIdx.y = pass (64 queries each); every per-pass buffer is laid out pass-major
        const size_t ps = blockIdx.y;
        qm += ps * (kQT / 32) * dq8 * 64;
        tau += ps * kQT;
        lists += ps * kQT * kListCap;
        counts += ps * kQT;
        sample += ps * kQT * sample_rows;
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int wpb = blockDim.x >> 6;      // 8 waves for the full pass, 2 for the (short) sample pass so that it covers every CU
    // The query tile is staged in LDS one SLAB of features at a time (<= kSlab8 groups of 8 = 512 features, 128 KiB for
    // 64 queries); d <= 512 needs one slab, loaded once; longer vectors (d = 1280: 3 slabs) re-stage per row group.
    const int sq8 = dq8 < kSlab8 ? dq8 : kSlab8;
    const int nslab = (dq8 + sq8 - 1) / sq8;
    if (MODE == 1 && threadIdx.x < kQT) tau_s[threadIdx.x] = tau[threadIdx.x];
    const int64_t rb_begin = row_begin / 32, rb_end = (row_end + 31) / 32;
    const int64_t nrg = (rb_end - rb_begin + wpb - 1) / wpb;            // row groups of wpb x 32 rows; uniform trip count per block
    bool staged = false;
    for (int64_t rg = blockIdx.x; rg < nrg; rg += gridDim.x) {
        const int64_t rb = rb_begin + rg * wpb + wave;
        const bool active = rb < rb_end;
        f32x16 acc0 = {0.f}, acc1 = {0.f};
        for (int sl = 0; sl < nslab; ++sl) {
            const int k0 = sl * sq8;
            const int kw = dq8 - k0 < sq8 ? dq8 - k0 : sq8;            // groups in this slab (a multiple of 4)
            if (nslab > 1 || !staged) {
                __syncthreads();                                          // everyone is done with the previous slab
                for (int i = threadIdx.x; i < 2 * kw * 64; i += blockDim.x) {
                    const int jb = i / (kw * 64), r = i - jb * kw * 64;
                    lq[(size_t)jb * sq8 * 64 + r] = qm[((size_t)jb * dq8 + k0) * 64 + r];
                }
                __syncthreads();
                staged = true;
            }
            if (!active) continue;
            const float4* a = gm + ((size_t)rb * dq8 + k0) * 64 + lane;
            // kw is a multiple of 4: EIGHT gallery fragments in flight (named registers, no runtime indexing), each
            // re-issued right after its 8 MFMAs, i.e. 7 steps = 3 584 MFMA cycles (x2 with two waves per SIMD) ahead of
            // its use -- with 2 waves per SIMD the loads must cover the HBM latency on their own.
            const int last = kw - 1;
            float4 a0 = a[0], a1 = a[(size_t)(1 < last ? 1 : last) * 64], a2 = a[(size_t)(2 < last ? 2 : last) * 64],
                   a3 = a[(size_t)(3 < last ? 3 : last) * 64], a4 = a[(size_t)(4 < last ? 4 : last) * 64],
                   a5 = a[(size_t)(5 < last ? 5 : last) * 64], a6 = a[(size_t)(6 < last ? 6 : last) * 64],
                   a7 = a[(size_t)(7 < last ? 7 : last) * 64];
            // query fragments come from LDS one step AHEAD of the MFMAs that use them (b0/b1 = this step, n0/n1 = next)
            float4 b0 = lq[lane], b1 = lq[(size_t)sq8 * 64 + lane];
#define FIR_GEMM_STEP(AV, KQ)                                                              \
            {                                                                              \
                const int kn = (KQ) + 1 < kw ? (KQ) + 1 : (KQ);                            \
                const float4 n0 = lq[(size_t)kn * 64 + lane];                              \
                const float4 n1 = lq[(size_t)(sq8 + kn) * 64 + lane];                      \
                __builtin_amdgcn_sched_barrier(0); /* keep the two ds_reads up here */    \
                acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(AV.x, b0.x, acc0, 0, 0, 0);    \
                acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(AV.x, b1.x, acc1, 0, 0, 0);    \
                acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(AV.y, b0.y, acc0, 0, 0, 0);    \
                acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(AV.y, b1.y, acc1, 0, 0, 0);    \
                acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(AV.z, b0.z, acc0, 0, 0, 0);    \
                acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(AV.z, b1.z, acc1, 0, 0, 0);    \
                acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(AV.w, b0.w, acc0, 0, 0, 0);    \
                acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(AV.w, b1.w, acc1, 0, 0, 0);    \
                b0 = n0;                                                                   \
                b1 = n1;                                                                   \
            }
            for (int kq = 0; kq < kw; kq += 8) {
                // (the tail re-loads clamp to the last fragment: harmless L2 hits, keeps the loop branch-free)
#define FIR_GEMM_NEXT(AV, OFF) AV = a[(size_t)(kq + (OFF) + 8 < kw ? kq + (OFF) + 8 : last) * 64];
                FIR_GEMM_STEP(a0, kq)
                FIR_GEMM_NEXT(a0, 0)
                FIR_GEMM_STEP(a1, kq + 1)
                FIR_GEMM_NEXT(a1, 1)
                FIR_GEMM_STEP(a2, kq + 2)
                FIR_GEMM_NEXT(a2, 2)
                FIR_GEMM_STEP(a3, kq + 3)
                FIR_GEMM_NEXT(a3, 3)
                if (kq + 4 < kw) {     // kw is a multiple of 4, not necessarily of 8
                    FIR_GEMM_STEP(a4, kq + 4)
                    FIR_GEMM_NEXT(a4, 4)
                    FIR_GEMM_STEP(a5, kq + 5)
                    FIR_GEMM_NEXT(a5, 5)
                    FIR_GEMM_STEP(a6, kq + 6)
                    FIR_GEMM_NEXT(a6, 6)
                    FIR_GEMM_STEP(a7, kq + 7)
                    FIR_GEMM_NEXT(a7, 7)
                }
#undef FIR_GEMM_NEXT
            }
#undef FIR_GEMM_STEP
        }
        if (!active) continue;
        // this wave's 32 squared row norms, one per lane (both halves), handed out by shuffles in the epilogue
        const int64_t nrow = rb * 32 + (lane & 31);
        const float gn_lane = nrow < n ? gnorm[nrow] : 0.0f;
        // C/D layout of the 32x32 MFMA: column (query) = lane & 31, row = (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5)
#pragma unroll
        for (int jb = 0; jb < 2; ++jb) {
            const int q = jb * 32 + (lane & 31);
#pragma unroll
            for (int reg = 0; reg < 16; ++reg) {
                const int roff = (reg & 3) + 8 * (reg >> 2) + 4 * (lane >> 5);
                const int64_t row = rb * 32 + roff;
                const float gn = __shfl(gn_lane, roff, 64);     // every lane takes part (before any divergence)
                if (row >= n || row < row_begin || row >= row_end) continue;
                const float dot = jb == 0 ? acc0[reg] : acc1[reg];
                const float p = gn - 2.0f * dot;
                if (MODE == 0) {
                    if (row < sample_rows) sample[(size_t)q * sample_rows + row] = p;
                } else if (p < tau_s[q]) {
                    const int slot = atomicAdd(&counts[q], 1);
                    if (slot < kListCap) lists[(size_t)q * kListCap + slot] = fir::key_pack(p, (uint32_t)row);
                }
            }
        }
    }
}

// ---------------------------------------------------------------------------------------------
// bf16-split variant. x = hi + lo + r with hi = bf16(x), lo = bf16(x - hi), |r| <= 2^-18 |x|: the dot product
// is taken as hi.hi + hi.lo + lo.hi on v_mfma_f32_32x32x16_bf16 (bf16 products are exact in f32; 16x the f32-MFMA
// rate, so three of them are still 5.3x faster); the dropped lo.lo and r terms are <= 3 * 2^-18 |g||q| and go
// into the certificate's E. Fragment order for this MFMA: lane l (r = l & 31, h = l >> 5) holds the 8 features
// 16 kb + 8 h .. + 7 of vector r of its 32-block as 8 bf16 (one uint4); hi and lo fragments are stored side by side.
// ---------------------------------------------------------------------------------------------
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));

__device__ __forceinline__ void split_bf16(float x, unsigned short& hi, unsigned short& lo) {
    const __bf16 h = (__bf16)x;                    // round to nearest even
    const __bf16 l = (__bf16)(x - (float)h);
    __builtin_memcpy(&hi, &h, 2);
    __builtin_memcpy(&lo, &l, 2);
}

// tiled f32 gallery -> gb[(rb * dk16 + kb) * 2 + {hi, lo}][lane] (uint4 = 8 bf16)
__global__ void __launch_bounds__(256) k_gemm_pack_gallery_bf16(const float4* __restrict__ gal4, int64_t n, int dp4, int dk16,
                                                                 uint4* __restrict__ gb) {
    const int64_t o = (int64_t)blockIdx.x * 256 + threadIdx.x;      // (rb, kb, lane)
    const int64_t rblocks = (n + 31) / 32;
    if (o >= rblocks * dk16 * 64) return;
    const int l = (int)(o & 63);
    const int64_t t = o >> 6;
    const int kb = (int)(t % dk16);
    const int64_t rb = t / dk16;
    const int64_t row = rb * 32 + (l & 31);
    const int h = l >> 5;
    unsigned short hi[8], lo[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const int k = 16 * kb + 8 * h + j;
        float x = 0.f;
        if (row < n && k < dp4 * 4) {
            const float4 g = gal4[((row >> 6) * dp4 + (k >> 2)) * 64 + (row & 63)];
            x = (k & 3) == 0 ? g.x : (k & 3) == 1 ? g.y : (k & 3) == 2 ? g.z : g.w;
        }
        split_bf16(x, hi[j], lo[j]);
    }
    uint4 vh, vl;
    __builtin_memcpy(&vh, hi, 16);
    __builtin_memcpy(&vl, lo, 16);
    gb[(size_t)(t * 2) * 64 + l] = vh;
    gb[(size_t)(t * 2 + 1) * 64 + l] = vl;
}

// queries -> qb[(jb * dk16 + kb) * 2 + {hi, lo}][lane], zero padded to kQT queries
__global__ void __launch_bounds__(256) k_gemm_pack_queries_bf16(const float* q, int nq, int d, int dk16, uint4* qbf) {
    q += (size_t)blockIdx.y * kQT * d;       // blockIdx.y = pass
    nq -= (int)blockIdx.y * kQT;
    qbf += (size_t)blockIdx.y * (kQT / 32) * dk16 * 128;
    const int o = blockIdx.x * 256 + threadIdx.x;
    if (o >= (kQT / 32) * dk16 * 64) return;
    const int l = o & 63;
    const int t = o >> 6;
    const int kb = t % dk16, jb = t / dk16;
    const int qi = jb * 32 + (l & 31), h = l >> 5;
    unsigned short hi[8], lo[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const int k = 16 * kb + 8 * h + j;
        const float x = (qi < nq && k < d) ? q[(size_t)qi * d + k] : 0.f;
        split_bf16(x, hi[j], lo[j]);
    }
    uint4 vh, vl;
    __builtin_memcpy(&vh, hi, 16);
    __builtin_memcpy(&vl, lo, 16);
    qbf[(size_t)(t * 2) * 64 + l] = vh;
    qbf[(size_t)(t * 2 + 1) * 64 + l] = vl;
}

__device__ __forceinline__ uint4 ld_nt(const uint4* p) {      // non-temporal: the gallery fragments are streamed once per pass
    typedef unsigned v4u __attribute__((ext_vector_type(4)));
    const v4u v = __builtin_nontemporal_load((const v4u*)p);
    return make_uint4(v.x, v.y, v.z, v.w);
}
__device__ __forceinline__ bf16x8 as_bf16x8(const uint4 v) {
    bf16x8 r;
    __builtin_memcpy(&r, &v, 16);
    return r;
}

// Same contract as k_gemm_proxy (one wave: 32 rows x 64 queries, MODE 0 sample / MODE 1 append), bf16-split operands.
// Dynamic LDS: one slab of the query tile: 2 query blocks x sk16 k-blocks x {hi, lo} x 64 uint4 (128 KiB at 512 features).
template <int MODE>
__global__ void __launch_bounds__(kGemmBlock, kGemmMinBlocks) k_gemm_proxy_bf16(const uint4* __restrict__ gb, const float* __restrict__ gnorm,
                                                                    const uint4* qbf, int64_t n, int64_t row_begin,
                                                                    int64_t row_end, int dk16, const float* tau, unsigned long long* lists, int* counts, float* sample,
                                                                    int sample_rows) {
    extern __shared__ __attribute__((aligned(16))) uint4 lqb[];
    __shared__ float tau_s[kQT];
    {   // blockIdx.y = pass (64 queries each); every per-pass buffer is laid out pass-major
        const size_t ps = blockIdx.y;
        qbf += ps * (kQT / 32) * dk16 * 128;
        tau += ps * kQT;
        lists += ps * kQT * kListCap;
        counts += ps * kQT;
        sample += ps * kQT * sample_rows;
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int wpb = blockDim.x >> 6;
    // MODE 0 (the short sample pass) reads the query fragments straight from global memory (L2-resident) and is launched
    // WITHOUT dynamic LDS, so its small workgroups fit next to the full pass's 128-KiB workgroups on the same CUs.
    const int sk16 = MODE == 0 ? dk16 : (dk16 < kSlab16 ? dk16 : kSlab16);
    const int nslab = (dk16 + sk16 - 1) / sk16;
    const uint4* bsrc = MODE == 0 ? qbf : lqb;
    if (MODE == 1 && threadIdx.x < kQT) tau_s[threadIdx.x] = tau[threadIdx.x];
    const int64_t rb_begin = row_begin / 32, rb_end = (row_end + 31) / 32;
    const int64_t nrg = (rb_end - rb_begin + wpb - 1) / wpb;
    bool staged = MODE == 0;
    for (int64_t rg = blockIdx.x; rg < nrg; rg += gridDim.x) {
        const int64_t rb = rb_begin + rg * wpb + wave;
        const bool active = rb < rb_end;
        f32x16 acc0 = {0.f}, acc1 = {0.f};
        for (int sl = 0; sl < nslab; ++sl) {
            const int k0 = sl * sk16;
            const int kw = dk16 - k0 < sk16 ? dk16 - k0 : sk16;            // k-blocks in this slab (a multiple of 4)
            if (MODE == 1 && (nslab > 1 || !staged)) {
                __syncthreads();
                for (int i = threadIdx.x; i < 2 * kw * 128; i += blockDim.x) {
                    const int jb = i / (kw * 128), r = i - jb * kw * 128;
                    lqb[(size_t)jb * sk16 * 128 + r] = qbf[((size_t)jb * dk16 + k0) * 128 + r];
                }
                __syncthreads();
                staged = true;
            }
            if (!active) continue;
            const uint4* a = gb + ((size_t)rb * dk16 + k0) * 128 + lane;      // +0: hi fragment, +64: lo fragment of a k-block
            const int last = kw - 1;
            // EIGHT k-blocks (hi + lo = 2 KiB per wave each, 16 KiB per wave) in flight, non-temporal, re-issued right after use:
            // this kernel is HBM-bound (the six MFMAs of a k-block take 192 cycles, its 2 KiB take longer to arrive)
#define FIR_BF_LD(IDX) ld_nt(a + (size_t)((IDX) < last ? (IDX) : last) * 128)
#define FIR_BF_LDL(IDX) ld_nt(a + (size_t)((IDX) < last ? (IDX) : last) * 128 + 64)
            uint4 h0 = FIR_BF_LD(0), l0 = FIR_BF_LDL(0), h1 = FIR_BF_LD(1), l1 = FIR_BF_LDL(1), h2 = FIR_BF_LD(2), l2 = FIR_BF_LDL(2),
                  h3 = FIR_BF_LD(3), l3 = FIR_BF_LDL(3), h4 = FIR_BF_LD(4), l4 = FIR_BF_LDL(4), h5 = FIR_BF_LD(5), l5 = FIR_BF_LDL(5),
                  h6 = FIR_BF_LD(6), l6 = FIR_BF_LDL(6), h7 = FIR_BF_LD(7), l7 = FIR_BF_LDL(7);
            // query fragments one step ahead: block 0 hi/lo, block 1 hi/lo
            const uint4* bq0 = bsrc + (size_t)(MODE == 0 ? k0 : 0) * 128 + lane;
            const uint4* bq1 = bq0 + (size_t)sk16 * 128;
            uint4 b0h = bq0[0], b0l = bq0[64], b1h = bq1[0], b1l = bq1[64];
#define FIR_BF_STEP(AH, AL, KB)                                                                                  \
            {                                                                                                    \
                const int kn = (KB) + 1 < kw ? (KB) + 1 : (KB);                                                  \
                const uint4 n0h = bq0[(size_t)kn * 128], n0l = bq0[(size_t)kn * 128 + 64];                       \
                const uint4 n1h = bq1[(size_t)kn * 128], n1l = bq1[(size_t)kn * 128 + 64];                       \
                __builtin_amdgcn_sched_barrier(0);                                                               \
                const bf16x8 ah = as_bf16x8(AH), al = as_bf16x8(AL);                                             \
                acc0 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, as_bf16x8(b0h), acc0, 0, 0, 0);               \
                acc1 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, as_bf16x8(b1h), acc1, 0, 0, 0);               \
                acc0 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, as_bf16x8(b0l), acc0, 0, 0, 0);               \
                acc1 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, as_bf16x8(b1l), acc1, 0, 0, 0);               \
                acc0 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(al, as_bf16x8(b0h), acc0, 0, 0, 0);               \
                acc1 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(al, as_bf16x8(b1h), acc1, 0, 0, 0);               \
                b0h = n0h; b0l = n0l; b1h = n1h; b1l = n1l;                                                      \
            }
#define FIR_BF_NEXT(AH, AL, OFF)                \
            {                                   \
                AH = FIR_BF_LD(kb + (OFF) + 8); \
                AL = FIR_BF_LDL(kb + (OFF) + 8);\
            }
            for (int kb = 0; kb < kw; kb += 8) {
                FIR_BF_STEP(h0, l0, kb)
                FIR_BF_NEXT(h0, l0, 0)
                FIR_BF_STEP(h1, l1, kb + 1)
                FIR_BF_NEXT(h1, l1, 1)
                FIR_BF_STEP(h2, l2, kb + 2)
                FIR_BF_NEXT(h2, l2, 2)
                FIR_BF_STEP(h3, l3, kb + 3)
                FIR_BF_NEXT(h3, l3, 3)
                if (kb + 4 < kw) {      // kw is a multiple of 4, not necessarily of 8
                    FIR_BF_STEP(h4, l4, kb + 4)
                    FIR_BF_NEXT(h4, l4, 4)
                    FIR_BF_STEP(h5, l5, kb + 5)
                    FIR_BF_NEXT(h5, l5, 5)
                    FIR_BF_STEP(h6, l6, kb + 6)
                    FIR_BF_NEXT(h6, l6, 6)
                    FIR_BF_STEP(h7, l7, kb + 7)
                    FIR_BF_NEXT(h7, l7, 7)
                }
            }
#undef FIR_BF_NEXT
#undef FIR_BF_STEP
#undef FIR_BF_LD
#undef FIR_BF_LDL
        }
        if (!active) continue;
        const int64_t nrow = rb * 32 + (lane & 31);
        const float gn_lane = nrow < n ? gnorm[nrow] : 0.0f;
#pragma unroll
        for (int jb = 0; jb < 2; ++jb) {
            const int q = jb * 32 + (lane & 31);
#pragma unroll
            for (int reg = 0; reg < 16; ++reg) {
                const int roff = (reg & 3) + 8 * (reg >> 2) + 4 * (lane >> 5);
                const int64_t row = rb * 32 + roff;
                const float gn = __shfl(gn_lane, roff, 64);
                if (row >= n || row < row_begin || row >= row_end) continue;
                const float dot = jb == 0 ? acc0[reg] : acc1[reg];
                const float p = gn - 2.0f * dot;
                if (MODE == 0) {
                    if (row < sample_rows) sample[(size_t)q * sample_rows + row] = p;
                } else if (p < tau_s[q]) {
                    const int slot = atomicAdd(&counts[q], 1);
                    if (slot < kListCap) lists[(size_t)q * kListCap + slot] = fir::key_pack(p, (uint32_t)row);
                }
            }
        }
    }
}

// ---------------------------------------------------------------------------------------------
// The append pass for TWO 64-query passes at once: one wave = 32 rows x 128 queries (four accumulator tiles, twelve
// MFMAs per k-block). The gallery stream -- what bounds k_gemm_proxy_bf16 (5.7 TB/s, MFMA pipe ~25 % busy) -- is read
// once per 128 queries instead of once per 64. The query fragments of 128 queries only fit LDS 256 features at a time
// (4 query blocks x 16 k-blocks x {hi, lo} x 1 KiB = 128 KiB), so every row group of a workgroup re-stages the slabs;
// the gallery fragments keep streaming through the staging barriers (a double buffer of eight k-blocks that runs on
// into the wave's next row block). What bounds this kernel is the re-staging itself -- two workgroup barriers around
// a 128 KiB copy per slab; changing the gallery ring into the double buffer left its 552 us per pass unchanged, whereas the
// fp16 kernel below, whose 128-query tile stays resident, went from 358 to 200 us. blockIdx.y = pair of passes; the per-pass scratch (tau, lists, counts, query fragments) is
// laid out pass-major, so the pair's 128 queries are simply consecutive.
// ---------------------------------------------------------------------------------------------
constexpr int kSlabW = 16;             // k-blocks (of 16 features) of the 128-query slab
constexpr int kUnitW = kSlabW / 2;     // k-blocks per unit of the gallery double buffer (hi + lo: 16 KiB per wave); dk16 is a multiple of it
constexpr int kWideLds = 4 * kSlabW * 128 * (int)sizeof(uint4);   // 128 KiB
__global__ void __launch_bounds__(kGemmBlock, 1) k_gemm_proxy_bf16_wide(const uint4* __restrict__ gb, const float* __restrict__ gnorm,
                                                                         const uint4* qbf, int64_t n, int dk16, const float* tau,
                                                                         unsigned long long* lists, int* counts) {
    extern __shared__ __attribute__((aligned(16))) uint4 lqb[];
    __shared__ float tau_s[2 * kQT];
    {
        const size_t pr = blockIdx.y;
        qbf += pr * 4 * dk16 * 128;
        tau += pr * 2 * kQT;
        lists += pr * 2 * kQT * kListCap;
        counts += pr * 2 * kQT;
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int wpb = blockDim.x >> 6;
    if (threadIdx.x < 2 * kQT) tau_s[threadIdx.x] = tau[threadIdx.x];
    const int64_t rb_end = (n + 31) / 32;
    const int64_t nrg = (rb_end + wpb - 1) / wpb;
    const int units = dk16 / kUnitW;
    int64_t rg = blockIdx.x;
    if (rg >= nrg) return;                           // uniform per workgroup
    // The gallery stream is a double buffer of kUnitW k-blocks (see k_gemm_proxy_f16x): all loads of the next unit -- of this
    // row block or of the wave's next one -- leave before the 96 MFMAs of the current unit.
#define FIR_W_BLOCK(RG) (gb + (size_t)(((RG) * wpb + wave) < rb_end ? ((RG) * wpb + wave) : rb_end - 1) * dk16 * 128 + lane)
    const uint4* a_cur = FIR_W_BLOCK(rg);            // inactive waves stream a valid block and drop it
    uint4 ch[kUnitW], cl[kUnitW], nh[kUnitW], nl[kUnitW];
#pragma unroll
    for (int u = 0; u < kUnitW; ++u) {
        ch[u] = ld_nt(a_cur + (size_t)u * 128);
        cl[u] = ld_nt(a_cur + (size_t)u * 128 + 64);
    }
    for (; rg < nrg; rg += gridDim.x) {
        const int64_t rb = rg * wpb + wave;
        const bool active = rb < rb_end;
        const int64_t rgn = rg + gridDim.x;
        const uint4* a_nxt = FIR_W_BLOCK(rgn < nrg ? rgn : rg);
        f32x16 acc0 = {0.f}, acc1 = {0.f}, acc2 = {0.f}, acc3 = {0.f};
        for (int h = 0; h < units; ++h) {
            const uint4* src = h + 1 < units ? a_cur + (size_t)(h + 1) * kUnitW * 128 : a_nxt;
#pragma unroll
            for (int u = 0; u < kUnitW; ++u) {
                nh[u] = ld_nt(src + (size_t)u * 128);
                nl[u] = ld_nt(src + (size_t)u * 128 + 64);
            }
            if ((h & 1) == 0) {                                             // a slab is two units; 128 queries never fit whole
                const int k0 = h * kUnitW;
                const int kw = dk16 - k0 < kSlabW ? dk16 - k0 : kSlabW;
                __syncthreads();                                            // everyone is done with the previous slab
                for (int i = threadIdx.x; i < 4 * kw * 128; i += blockDim.x) {
                    const int jb = i / (kw * 128), r = i - jb * kw * 128;
                    lqb[(size_t)jb * kSlabW * 128 + r] = qbf[((size_t)jb * dk16 + k0) * 128 + r];
                }
                __syncthreads();
            }
            const uint4* bq = lqb + lane + (size_t)(h & 1) * kUnitW * 128;
#pragma unroll
            for (int u = 0; u < kUnitW; ++u) {
                const uint4* bu = bq + (size_t)u * 128;
                const bf16x8 ah = as_bf16x8(ch[u]), al = as_bf16x8(cl[u]);
#pragma unroll
                for (int jb = 0; jb < 4; ++jb) {
                    const bf16x8 bh = as_bf16x8(bu[(size_t)jb * kSlabW * 128]), bl = as_bf16x8(bu[(size_t)jb * kSlabW * 128 + 64]);
                    f32x16& acc = jb == 0 ? acc0 : jb == 1 ? acc1 : jb == 2 ? acc2 : acc3;
                    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, bh, acc, 0, 0, 0);
                    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, bl, acc, 0, 0, 0);
                    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(al, bh, acc, 0, 0, 0);
                }
            }
#pragma unroll
            for (int u = 0; u < kUnitW; ++u) { ch[u] = nh[u]; cl[u] = nl[u]; }
        }
        a_cur = a_nxt;
        if (!active) continue;
        const int64_t nrow = rb * 32 + (lane & 31);
        const float gn_lane = nrow < n ? gnorm[nrow] : 0.0f;
#pragma unroll
        for (int jb = 0; jb < 4; ++jb) {
            const int q = jb * 32 + (lane & 31);
#pragma unroll
            for (int reg = 0; reg < 16; ++reg) {
                const int roff = (reg & 3) + 8 * (reg >> 2) + 4 * (lane >> 5);
                const int64_t row = rb * 32 + roff;
                const float gn = __shfl(gn_lane, roff, 64);
                if (row >= n) continue;
                const float dot = jb == 0 ? acc0[reg] : jb == 1 ? acc1[reg] : jb == 2 ? acc2[reg] : acc3[reg];
                const float p = gn - 2.0f * dot;
                if (p < tau_s[q]) {
                    const int slot = atomicAdd(&counts[q], 1);
                    if (slot < kListCap) lists[(size_t)q * kListCap + slot] = fir::key_pack(p, (uint32_t)row);
                }
            }
        }
    }
#undef FIR_W_BLOCK
}

// ---------------------------------------------------------------------------------------------
// FIR_GEMM_F16: ONE fp16 MFMA term, 128 queries per gallery read. The gallery fragments are half the bytes of the bf16
// split (2 B per feature) and each k-block costs four MFMAs instead of twelve; the price is a proxy that is only good
// to 2^-10 |q||g| -- which the certificate simply carries in E (k_gemm_rerank): on feature vectors the gap between the
// best row and the 8th-best proxy is an order of magnitude wider than that, and a query it cannot certify goes through
// the exact scan like any other. Operands are scaled by powers of two into fp16's normal range (the gallery by one
// factor, every query by its own; undone per query column in the epilogue, exact), so rounding is relative (2^-11 per
// operand) for every element within 2^-27 of the largest; smaller ones lose at most 2^-38 of that largest value each.
// The query tile (128 queries x 32 k-blocks x 1 KiB = 128 KiB at 512 features) stays in LDS for a whole pass when d <= 512;
// the gallery stream is double-buffered and runs on into the wave's NEXT row block, so it never drains between row groups.
// The kernels are in fir_gemm_f16x.h; what follows here is shared with fir_gemm_fb.h and fir_gemm_f64.h.
// ---------------------------------------------------------------------------------------------
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
__device__ __forceinline__ f16x8 as_f16x8(const uint4 v) {
    f16x8 r;
    __builtin_memcpy(&r, &v, 16);
    return r;
}
constexpr int kSlabH = 32;                                              // k-blocks (of 16 features) of the 128-query slab
constexpr int kHalfLds = 4 * kSlabH * 64 * (int)sizeof(uint4);          // 128 KiB
constexpr int kRing = 8;                                                // gallery k-blocks per double-buffer unit (8 KiB per wave); the fp16 dk16 is padded to it

#include "fir_gemm_rerank.h"

// max |x| over the tiled gallery (padding is zero) -> out[0]; out must be zeroed first. Non-finite values poison it (NaN -> +inf).
__global__ void __launch_bounds__(256) k_gemm_absmax(const float4* __restrict__ gal4, int64_t count4, float* __restrict__ out) {
    float m = 0.f;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < count4; i += (int64_t)gridDim.x * 256) {
        const float4 g = gal4[i];
        const float a = fmaxf(fmaxf(fabsf(g.x), fabsf(g.y)), fmaxf(fabsf(g.z), fabsf(g.w)));
        const bool bad = !(g.x == g.x && g.y == g.y && g.z == g.z && g.w == g.w);
        m = fmaxf(m, bad ? __builtin_huge_valf() : a);
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) m = fmaxf(m, __shfl_xor(m, off, 64));
    if ((threadIdx.x & 63) == 0) atomicMax((unsigned int*)out, __float_as_uint(m));     // non-negative floats order like their bits
}

// Per query (one wave each): |q|^2, its own power-of-two scale qmul (largest |q_k| -> [2^13, 2^14)) and
// qinv = 1 / (qmul * gallery scale), which turns the MFMA result back into q.g. Queries past nq: all zero.
// A query whose scale would leave [2^-100, 2^100], or with a non-finite value, gets qinv = NaN: every proxy is then NaN,
// nothing is certified and the exact scan answers it.
// counts != NULL: the query's candidate count is cleared here too (instead of a memset of its own); win != NULL: ... and the adaptive
// pass's window and start value are set (k_gemm_adapt_init's two lines): two launches less in front of every super-batch.
__global__ void __launch_bounds__(64) k_gemm_qprep_f16(const float* __restrict__ q, int nq, int d, int gallery_exp, float* __restrict__ qnorm,
                                                        float* __restrict__ qmul, float* __restrict__ qinv, int qstride, int* __restrict__ counts = nullptr,
                                                        float* __restrict__ win = nullptr, unsigned int* __restrict__ t_bits = nullptr,
                                                        const float* __restrict__ gnorm_max_p = nullptr, float e_rel = 0.f, int nslot = 0,
                                                        unsigned int* __restrict__ smin_init = nullptr, int* __restrict__ fb_state = nullptr) {
    // smin_init / fb_state (the few-query path): the words three hipMemsetAsync calls used to preset -- each a launch of its own in front of a
    // 250-us call
    const int qi = blockIdx.x;
    if (threadIdx.x == 0) {
        if (smin_init) smin_init[qi] = 0xFF800000u;
        if (fb_state && qi == 0) { fb_state[0] = 0; fb_state[1] = 0; }
    }
    float s = 0.f, m = 0.f;
    bool bad = false;
    if (qi < nq)
        for (int k = threadIdx.x; k < d; k += 64) {
            const float x = q[(size_t)qi * qstride + k];
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
    if (threadIdx.x == 0) {
        int ex = 0;
        if (m > 0.f) (void)frexpf(m, &ex);                 // m = f * 2^ex, f in [0.5, 1)
        int sh = m > 0.f ? 14 - ex : 0;                    // m * 2^sh in [2^13, 2^14)
        if (sh < -100 || sh > 100 || gallery_exp < -100 || gallery_exp > 100) bad = true;
        // bad: the proxies of this query are NaN and say nothing about any row -- a NaN norm keeps the certificate from holding
        const float qn = (bad && qi < nq) ? __builtin_nanf("") : s;
        qnorm[qi] = qn;
        qmul[qi] = bad ? 0.f : ldexpf(1.0f, sh);
        qinv[qi] = qi >= nq ? 0.f : bad ? __builtin_nanf("") : ldexpf(1.0f, -sh - gallery_exp);
        if (counts) counts[qi] = 0;
        if (win) {                                                   // (k_gemm_adapt_init)
            // (t_bits is the word the ranks exchange through memory-side atomics: it is only ever touched by atomics, so that no XCD's L2
            // holds a line of it that an atomic could be served from)
            // nslot > 0 (the K nearest rows, k_gemm_proxy_f16x<4, *>): eight slot words per query
            const unsigned int start = qi >= nq ? 0u : 0x7F800000u;
            if (qi >= nq) win[qi] = 0.f;
            else {
                win[qi] = nudge_up_(rounding_window_(e_rel, qn, gnorm_max_p[0]));
            }
            if (nslot > 0) { for (int sl = 0; sl < 8; ++sl) atomicExch(&t_bits[(size_t)qi * 8 + sl], start); }
            else atomicExch(&t_bits[qi], start);
        }
    }
}

#include "fir_gemm_f16x.h"

// tau[q] = kCand-th smallest sampled proxy, nudged up so that ties with it are appended too. One block per
// query, ONE pass over the samples: every thread keeps its kCand smallest keys sorted in registers, then kCand
// rounds of block-min pop the global order statistics.
// The bound is also kept at least one rounding window (k_gemm_rerank) above the SMALLEST sampled proxy: on a clustered
// gallery dozens of rows lie within the window of the best one, the kCand-th smallest would cut through them and the
// certificate could never hold (measured: 75 of 200 queries of a 600-identity gallery went to the exact scan).
__global__ void __launch_bounds__(256) k_gemm_tau(const float* __restrict__ sample, int sample_rows, float* __restrict__ tau,
                                                   int nq_valid, const float* __restrict__ qnorm, const float* __restrict__ gnorm_max_p, float e_rel,
                                                   int kth_window = 0) {
    // kth_window (top-K, K <= kCand): the bound is the kCand-th smallest sampled proxy PLUS one window -- at least K rows
    // lie at or below the kCand-th smallest, and every row within a window of the K-th best one must be appended for the
    // certificate of rank K to be able to hold
    __shared__ unsigned long long red[4];
    const int q = blockIdx.x;
    if (q >= nq_valid) {        // padding queries of a half-filled pass pair: nothing is appended for them
        if (threadIdx.x == 0) tau[q] = -__builtin_huge_valf();
        return;
    }
    const float* s = sample + (size_t)q * sample_rows;
    unsigned long long best[kCand];
#pragma unroll
    for (int i = 0; i < kCand; ++i) best[i] = kKeyNone;
    for (int i = threadIdx.x; i < sample_rows; i += 256) {
        unsigned long long v = fir::key_pack(s[i], (uint32_t)i);
        if (v < best[kCand - 1]) {
#pragma unroll
            for (int j = 0; j < kCand; ++j) {
                const bool sw = v < best[j];
                const unsigned long long t = best[j];
                best[j] = sw ? v : t;
                v = sw ? t : v;
            }
        }
    }
    unsigned long long m = kKeyNone, smallest = kKeyNone;
    for (int r = 0; r < kCand; ++r) {
        unsigned long long c = fir::wave_min_u64(best[0]);
        __syncthreads();
        if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = c;
        __syncthreads();
        m = red[0];
        for (int i = 1; i < 4; ++i) m = red[i] < m ? red[i] : m;
        if (r == 0) smallest = m;
        if (m == kKeyNone) break;
        if (best[0] == m) {     // keys are unique (row index): exactly one thread pops
#pragma unroll
            for (int j = 0; j + 1 < kCand; ++j) best[j] = best[j + 1];
            best[kCand - 1] = kKeyNone;
        }
    }
    if (threadIdx.x == 0) {
        // fewer than kCand sampled rows: no bound -> +inf appends everything (the list cap then decides)
        float t = __builtin_huge_valf();
        if (m != kKeyNone) {
            float v = fir::f32_from_orderable((uint32_t)(m >> 32));
            const float v1 = fir::f32_from_orderable((uint32_t)(smallest >> 32));
            const float window = rounding_window_(e_rel, qnorm[q], gnorm_max_p[0]);
            v = kth_window ? v + window : fmaxf(v, v1 + window);                     // (top-1) a NaN window leaves v as it is
            t = nudge_up_(v);
        }
        tau[q] = t;
    }
}

#include "fir_gemm_fb.h"
#include "fir_gemm_i8.h"

// The K nearest rows of every query (K <= KMAX; KMAX = 1: the nearest row, K a constant) from its candidate list: every appended
// entry inside the window of the K-th smallest proxy of the list (rerank_window_; a list of fewer than K is re-ranked whole) is
// re-ranked with the reference's arithmetic, every lane keeping the K smallest exact keys it computed, K rounds of wave-minimum at
// the end, and the certificate taken against the K-th exact distance: no row outside the re-ranked set can be among the K nearest,
// nor tie with the K-th. One wave per query. out_key[q * k + r], ascending; kKeyNone where fewer than K rows are below 100000;
// ok[q] = 1 when the certificate holds.
template <int KMAX>
__global__ void __launch_bounds__(64) k_gemm_rerank(const unsigned long long* __restrict__ lists, const int* __restrict__ counts,
                                                     const float* __restrict__ tau, const float4* __restrict__ gal4,
                                                     const float* __restrict__ queries, const float* __restrict__ qnorm,
                                                     const float* __restrict__ gnorm_max_p, int64_t n, int d, int dp4, int64_t row_offset,
                                                     float e_rel, int ngroup, int k_arg, unsigned long long* __restrict__ out_key,
                                                     int* __restrict__ ok, int qstride, const float4* __restrict__ rowmajor, const RerankFb fb,
                                                     const float* __restrict__ eabs = nullptr) {
    // eabs != NULL (an int8 super-batch, fir_gemm_i8.h): qnorm, gnorm_max_p and the proxies are those of the CENTRED vectors and the
    // windows carry eabs[q]; the distances below are still the reference's, on the rows and queries as they are
    const int k = KMAX == 1 ? 1 : k_arg;
    // q: the query's scratch slot (lists, counts, tau, qnorm); qo: its place in queries / out_key / ok -- the same for a super-batch's
    // own re-rank, the query's index in the call for a second-chance round (fir_gemm_fb.h)
    const int q = blockIdx.x, lane = threadIdx.x;
    int qo = q;
    if (fb.qmap) {
        if (q >= fb.state[0] - fb.live_off) return;               // (uniform per workgroup)
        qo = fb.qmap[q];
    }
    const int cnt = counts[q];
    const int have = cnt < kListCap ? cnt : kListCap;
    const unsigned long long* L = lists + (size_t)q * kListCap;
    int found;
    const unsigned long long kth = list_kth_smallest_(L, have, k, lane, found);
    const float qn = qnorm[q], gmax = gnorm_max_p[0];
    const float pk = found == k ? fir::f32_from_orderable((uint32_t)(kth >> 32)) : __builtin_huge_valf();
    const RerankWindow w = eabs ? rerank_window_(e_rel, qn, gmax, d, pk, eabs[q]) : rerank_window_(e_rel, qn, gmax, d, pk);
    extern __shared__ __attribute__((aligned(16))) float4 crow[];
    const RerankLds lds = rerank_lds_f32_(crow, ngroup, dp4, d, queries + (size_t)qo * qstride, lane);
    unsigned long long best[KMAX];
#pragma unroll
    for (int i = 0; i < KMAX; ++i) best[i] = kKeyNone;
    const RerankWalk walk = rerank_walk_(L, have, w.win, lane, [&](int base, unsigned long long v, bool, unsigned long long mask) {
        rerank_gather_f32_(mask, v, base, lane, ngroup, lds, gal4, rowmajor, dp4, d, [&](int, unsigned long long cv, float dist) {
            if (dist < fir::kNotFound) {
                const int64_t row = (int64_t)(uint32_t)(cv & 0xFFFFFFFFull);
                unsigned long long key = fir::key_pack(dist, (uint32_t)(row + row_offset));
#pragma unroll
                for (int j = 0; j < KMAX; ++j) {                    // sorted insert
                    const bool sw = key < best[j];
                    const unsigned long long t = best[j];
                    best[j] = sw ? key : t;
                    key = sw ? t : key;
                }
            }
        });
    });
    unsigned long long kth_exact = kKeyNone;
    for (int r = 0; r < k; ++r) {
        const unsigned long long m = fir::wave_min_u64(best[0]);
        if (lane == 0) out_key[(size_t)qo * k + r] = m;
        kth_exact = m;
        if (m != kKeyNone && best[0] == m) {                            // exactly one lane holds it
#pragma unroll
            for (int j = 0; j + 1 < KMAX; ++j) best[j] = best[j + 1];
            best[KMAX - 1] = kKeyNone;
        }
    }
    if (lane == 0) {
        const float t = tau[q];
        const bool certified = rerank_certified_<float>(cnt, t, walk.p_out, qn, d, w.E, kth_exact != kKeyNone,
                                                        fir::f32_from_orderable((uint32_t)(kth_exact >> 32)), n, walk.reranked);
        ok[qo] = certified ? 1 : 0;
        if (!certified && fb.list && !fb.qmap) rerank_hand_over_(fb, q, cnt, t, pk, qn, gmax, e_rel, eabs);
    }
}

// ---- calls of 1..8 queries against a gallery that does not fit the caches ----
// Such a call is one gallery pass whatever it computes, so it is bound by the bytes of that pass: the exact f32 scan reads n*d*4
// (337 us at 1M x 512), this nomination scan reads the fp16 copy, n*d*2. No matrix cores (eight queries would fill 1/16 of a
// tile): v_dot2c_f32_f16 on the same fragments (k_gemm_scan_f16x, fir_gemm_f16x.h). Every proxy is written out (n floats per
// query) together with the smallest one per query; tau = smallest proxy of ALL rows + one window (k_gemm_tau_min), the rows
// below it are collected (k_gemm_select) and re-ranked exactly with the usual certificate (k_gemm_rerank) -- which holds by
// construction here: every excluded row is a full window above the smallest proxy.
// lists[q] <- every row whose proxy is below tau[q] (blockIdx.y = query)
__global__ void __launch_bounds__(256) k_gemm_select(const float* __restrict__ proxies, int64_t n, const float* __restrict__ tau,
                                                      unsigned long long* __restrict__ lists, int* __restrict__ counts) {
    const int q = blockIdx.y;
    const float tq = tau[q];
    const float* p = proxies + (size_t)q * n;
    for (int64_t row = (int64_t)blockIdx.x * 256 + threadIdx.x; row < n; row += (int64_t)gridDim.x * 256) {
        const float v = p[row];
        if (v < tq) {
            const int slot = atomicAdd(&counts[q], 1);
            if (slot < kListCap) lists[(size_t)q * kListCap + slot] = fir::key_pack(v, (uint32_t)row);
        }
    }
}

// ---- the K nearest distinct classes (fir_gemm_search_top_classes_keys_dev) ----
// tau[q] holds D_s on entry: the exact K-th smallest class minimum of a row sample (fir_class_scan_dev_), an upper bound of the
// gallery's K-th class distance D_K. On exit it is that bound in proxy units plus one rounding window, as k_gemm_tau_min hangs
// it on a sampled proxy: a row whose reference distance is <= D_s has a true |g|^2 - 2 q.g within E d of D_s d - |q|^2 and a
// proxy within E d of that, so it lies below tau and is appended. D_s = 100000 (fewer than K classes in the sample): no bound,
// +inf appends everything and the list cap decides. A NaN norm gives a NaN tau: nothing is appended, nothing certified.
__global__ void __launch_bounds__(256) k_gemm_tau_class(float* __restrict__ tau, int nq_total, int nq_valid, int d, const float* __restrict__ qnorm,
                                                         const float* __restrict__ gnorm_max_p, float e_rel) {
    const int q = blockIdx.x * 256 + threadIdx.x;
    if (q >= nq_total) return;
    if (q >= nq_valid) { tau[q] = -__builtin_huge_valf(); return; }       // padding queries of a half-filled pair: nothing is appended
    const float ds = tau[q];
    float t = __builtin_huge_valf();
    if (ds < fir::kNotFound) {
        const float v = (ds * (float)d - qnorm[q]) + rounding_window_(e_rel, qnorm[q], gnorm_max_p[0]);
        t = nudge_up_(v);
    }
    tau[q] = t;
}

// The K nearest distinct classes (K <= 32) from the lists of one append pass below k_gemm_tau_class's bound. One wave per query.
//   1. p_K = the K-th smallest proxy over DISTINCT classes of the list (rows labelled outside [0, num_classes) take no part):
//      K rounds of "smallest key of a class not yet taken"; fewer than K classes: the whole list is re-ranked.
//   2. every entry with a proxy <= p_K + 2 E d is re-ranked in the reference's arithmetic (rerank_gather_f32_) and its exact
//      key written back over its list entry; entries outside the window, and rows that do not qualify (label, dist >= 100000),
//      become kKeyNone.
//   3. K rounds over the exact keys pick the classes: the smallest key of a class is its first minimum in row order, and the
//      rounds return the classes ascending by (distance, row).
// Certificate, against the K-th exact class distance D (100000 with fewer than K classes found): the list did not overflow and
// (|q|^2 + p_excl)/d - E > D, p_excl = min(smallest proxy not re-ranked, tau). Every row that was not appended or not re-ranked
// then has a reference distance above D. Each of the K classes found has a re-ranked row at or below D, so such a row can
// neither bring a new class in among the K nor be the best row of one that is among them (that row, at or below D, was
// re-ranked): keys and classes are the exact scan's. Strict '>': a NaN never certifies, a tie with the K-th does not either.
__global__ void __launch_bounds__(64) k_gemm_rerank_classes(unsigned long long* lists, const int* __restrict__ counts, const float* __restrict__ tau,
                                                             const float4* __restrict__ gal4, const float* __restrict__ queries,
                                                             const float* __restrict__ qnorm, const float* __restrict__ gnorm_max_p,
                                                             const int32_t* __restrict__ cls, int num_classes, int64_t n, int d, int dp4,
                                                             int64_t row_offset, float e_rel, int ngroup, int k, unsigned long long* __restrict__ out_key,
                                                             int32_t* __restrict__ out_cls, int* __restrict__ ok, int qstride,
                                                             const float4* __restrict__ rowmajor) {
    __shared__ int32_t taken[32];
    const int q = blockIdx.x, lane = threadIdx.x;
    const int cnt = counts[q];
    if (cnt > kListCap) {                           // rows below tau were dropped: the exact form answers this query
        if (lane == 0) ok[q] = 0;
        return;
    }
    const int have = cnt;
    unsigned long long* L = lists + (size_t)q * kListCap;
    // round r of "the smallest key of a class not yet taken" (keys carry rows roff + local row): every key at or below the previous
    // pick belongs to a taken class; a label is only looked up for a key that would improve the lane's candidate
    auto pick = [&](int r, unsigned long long prev, int64_t roff, int32_t& c_out) -> unsigned long long {
        unsigned long long cand = kKeyNone;
        int32_t cc = -1;
        for (int i = lane; i < have; i += 64) {
            const unsigned long long v = L[i];
            if (v >= cand || (r > 0 && v <= prev)) continue;
            const int32_t c = cls[(int64_t)(uint32_t)(v & 0xFFFFFFFFull) - roff];
            bool skip = (uint32_t)c >= (uint32_t)num_classes;
            for (int j = 0; j < r; ++j) skip = skip || taken[j] == c;
            if (!skip) { cand = v; cc = c; }
        }
        const unsigned long long m = fir::wave_min_u64(cand);
        const unsigned long long who = __ballot(m != kKeyNone && cand == m);      // keys are unique (the row is part of the key)
        c_out = who ? __shfl(cc, __ffsll((long long)who) - 1, 64) : -1;
        return m;
    };
    unsigned long long prev = 0;
    int found = 0;
    for (int r = 0; r < k; ++r) {
        int32_t c;
        const unsigned long long m = pick(r, prev, 0, c);
        if (m == kKeyNone) break;
        if (lane == 0) taken[r] = c;
        __syncthreads();
        prev = m;
        ++found;
    }
    const float qn = qnorm[q], gmax = gnorm_max_p[0];
    const float pk = found == k ? fir::f32_from_orderable((uint32_t)(prev >> 32)) : __builtin_huge_valf();   // a list short of classes is re-ranked whole
    const RerankWindow w = rerank_window_(e_rel, qn, gmax, d, pk);
    extern __shared__ __attribute__((aligned(16))) float4 crow[];
    const RerankLds lds = rerank_lds_f32_(crow, ngroup, dp4, d, queries + (size_t)q * qstride, lane);
    const RerankWalk walk = rerank_walk_(L, have, w.win, lane, [&](int base, unsigned long long v, bool in, unsigned long long mask) {
        if (base + lane < have && !in) L[base + lane] = kKeyNone;
        rerank_gather_f32_(mask, v, base, lane, ngroup, lds, gal4, rowmajor, dp4, d, [&](int i, unsigned long long cv, float dist) {
            const int64_t row = (int64_t)(uint32_t)(cv & 0xFFFFFFFFull);
            const bool counted = (uint32_t)cls[row] < (uint32_t)num_classes && dist < fir::kNotFound;
            L[i] = counted ? fir::key_pack(dist, (uint32_t)(row + row_offset)) : kKeyNone;
        });
    });
    __threadfence_block();                                              // the exact keys, written by other lanes, are read below
    __syncthreads();
    unsigned long long kth_exact = kKeyNone;
    prev = 0;
    int r = 0;
    for (; r < k; ++r) {
        int32_t c;
        const unsigned long long m = pick(r, prev, row_offset, c);
        if (m == kKeyNone) break;
        if (lane == 0) {
            taken[r] = c;
            if (out_key) out_key[(size_t)q * k + r] = m;
            if (out_cls) out_cls[(size_t)q * k + r] = c;
        }
        __syncthreads();
        prev = m;
        if (r == k - 1) kth_exact = m;
    }
    for (int i = r + lane; i < k; i += 64) {                            // unused slots
        if (out_key) out_key[(size_t)q * k + i] = kKeyNone;
        if (out_cls) out_cls[(size_t)q * k + i] = -1;
    }
    if (lane == 0)      // (fewer than K classes found: any qualifying row outside the re-ranked set could bring one in)
        ok[q] = rerank_certified_<float>(cnt, tau[q], walk.p_out, qn, d, w.E, kth_exact != kKeyNone, fir::f32_from_orderable((uint32_t)(kth_exact >> 32)), n,
                                         walk.reranked) ? 1 : 0;
}

// the running totals fir_gemm_stats_ex reads (kFbStateWords), for a call whose uncertified queries the host sent to the exact form
__global__ void k_gemm_fb_count(int* __restrict__ state, int count) {
    unsigned long long* tot = (unsigned long long*)(state + 4);
    tot[0] += (unsigned long long)count;
    tot[1] += (unsigned long long)count;
}

#include "fir_gemm_knn.h"

// rowmajor[row * d4 + c] = chunk c of row `row`: the re-rank's copy of the compared features. A row of the tiled gallery is d4
// separate 16-byte pieces 1 KiB apart (~4x its size in 64-byte sectors per gather); here it is one contiguous run.
__global__ void __launch_bounds__(256) k_gemm_untile(const float4* __restrict__ gal4, int64_t n, int dp4, int d4, float4* __restrict__ rowmajor) {
    // one workgroup per (tile of 64 rows, group of 32 chunks): read coalesced along the rows, written coalesced along the chunks
    __shared__ float4 t[32][65];
    const int64_t tile = blockIdx.x;
    const int c0 = blockIdx.y * 32;
    for (int i = threadIdx.x; i < 32 * 64; i += 256) {
        const int c = i >> 6, r = i & 63;
        if (c0 + c < d4) t[c][r] = gal4[((size_t)tile * dp4 + c0 + c) * 64 + r];
    }
    __syncthreads();
    for (int i = threadIdx.x; i < 64 * 32; i += 256) {
        const int r = i >> 5, c = i & 31;
        const int64_t row = tile * 64 + r;
        if (row < n && c0 + c < d4) rowmajor[(size_t)row * d4 + c0 + c] = t[c][r];
    }
}

// gnorm[row] = |g|^2 (one thread per row; any summation order is covered by the certificate's E).
__global__ void __launch_bounds__(256) k_gemm_row_norms(const float4* __restrict__ gal4, int64_t n, int dp4, float* __restrict__ gnorm, int d4) {
    const int64_t row = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (row >= n) return;
    float s = 0.f;
    for (int c = 0; c < d4; ++c) {
        const float4 g = gal4[((row >> 6) * dp4 + c) * 64 + (row & 63)];
        s += g.x * g.x + g.y * g.y + g.z * g.z + g.w * g.w;
    }
    gnorm[row] = s;
}

__global__ void k_gemm_max(const float* __restrict__ gnorm, int64_t n, float* __restrict__ out) {
    __shared__ float red[4];
    float m = 0.f;
    for (int64_t i = threadIdx.x; i < n; i += 256) m = fmaxf(m, gnorm[i]);
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) m = fmaxf(m, __shfl_xor(m, off, 64));
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = m;
    __syncthreads();
    if (threadIdx.x == 0) out[0] = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
}

// The adaptive flow (k_gemm_proxy_f16x<3, *>): per query the rounding window (2.5 E d, as k_gemm_tau_min) and the start value of
// T -- +inf, or 0 for the padding queries of a half-filled pair (nothing is ever below it) ...
__global__ void __launch_bounds__(256) k_gemm_adapt_init(float* __restrict__ win, unsigned int* __restrict__ t_bits, int nq_total, int nq_valid,
                                                          const float* __restrict__ qnorm, const float* __restrict__ gnorm_max_p, float e_rel) {
    const int q = blockIdx.x * 256 + threadIdx.x;
    if (q >= nq_total) return;
    if (q >= nq_valid) { win[q] = 0.f; t_bits[q] = 0u; return; }
    win[q] = nudge_up_(rounding_window_(e_rel, qnorm[q], gnorm_max_p[0]));        // (a NaN window: T never falls, nothing is certified)
    t_bits[q] = 0x7F800000u;
}
// ... and, after the pass, the bound the re-rank's certificate gets: every row that was not appended has a proxy >= tau
__global__ void __launch_bounds__(256) k_gemm_adapt_final(unsigned int* __restrict__ t_bits, const float* __restrict__ qnorm, float* __restrict__ tau,
                                                           int nq_total, int nq_valid, int nslot = 0) {
    const int q = blockIdx.x * 256 + threadIdx.x;
    if (q >= nq_total) return;
    // (read by an atomic, like every other access to these words)
    unsigned int t;
    if (nslot > 0) {                                  // the K nearest rows: the K-th smallest of the eight slot values (K = nslot)
        unsigned int v[8];
        for (int sl = 0; sl < 8; ++sl) v[sl] = atomicMin(&t_bits[(size_t)q * 8 + sl], 0xFFFFFFFFu);
        t = 0xFFFFFFFFu;
        for (int i = 0; i < 8; ++i) {
            int rank = 0;
            for (int j = 0; j < 8; ++j) rank += (v[j] < v[i] || (v[j] == v[i] && j < i)) ? 1 : 0;
            if (rank == nslot - 1) t = v[i];
        }
    } else t = atomicMin(&t_bits[q], 0xFFFFFFFFu);
    tau[q] = q < nq_valid ? __uint_as_float(t) - qnorm[q] : -__builtin_huge_valf();      // the same subtraction the kernel compares against
}

}  // namespace

// A FirBuf that reads as the T* it holds.
template <typename T>
struct GemmBuf : FirBuf {
    operator T*() const { return (T*)p; }
};

// One set of what a super-batch's preparation, passes and re-rank hand each other. A state's two sets and a float64 state's one are
// sized for kPasses passes; the second-chance round's (fir_gemm::sc) for one pair. Members a set never uses stay empty.
struct GemmScratch {
    GemmBuf<uint4> qbf;                   // query fragments: fp16 / int8, bf16 hi + lo; the f32 form reads them as<float4>()
    GemmBuf<float> qnorm, qmul, qinv;     // per query: |q|^2, the fragments' scale and what turns a sum back into a proxy
    GemmBuf<float> tau;                   // the bound the re-rank's certificate gets: every row that was not appended has a proxy >= tau
    GemmBuf<float> awin;                  // threshold found on the way (k_gemm_proxy_f16x<3 | 4, *>): the per-query windows ...
    GemmBuf<unsigned int> aT;             // ... and the workgroups' shared T (float bits; x 8: the K slot words of the K-nearest form)
    GemmBuf<unsigned int> smin;           // sample flow: smallest sampled proxy per query (orderable bits; top-K: per subset)
    GemmBuf<unsigned long long> lists;    // candidate lists (kListCap entries per query) and their lengths: grown to the super-batch in use
    GemmBuf<int> counts;                  //   by gemm_grow_lists_, the round's at creation
    GemmBuf<float> eabs;                  // int8 calls: the per-query absolute term (gemm_build_i8_)
    size_t bytes() const { return qbf.cap + qnorm.cap + qmul.cap + qinv.cap + tau.cap + awin.cap + aT.cap + smin.cap + lists.cap + counts.cap + eabs.cap; }
};

static void gemm_free_i8_(struct fir_gemm* m);

// The matrix-core state of one gallery (or of a prefix of its rows; or, f64, of a float64 training set). It owns everything it points
// to except the gallery: the buffers free themselves, the destructor releases the rest.
struct fir_gemm {
    // ---- what is searched: set when the state is created, never changed ----
    fir_gallery* g = nullptr;             // not owned (NULL for a float64 state)
    fir_gallery_view v;
    const float4* gal4 = nullptr;         // the gallery's tiled f32 rows: not owned
    int dp4 = 0, dq8 = 0;
    int feat = 0;                         // features compared: the gallery's d, or a prefix [0, feat) of every row (fir_gemm_create_range); v.d stays the row length
    int precision = 0;                    // 0: f32 MFMA, 1: bf16 split (hi.hi + hi.lo + lo.hi), 2: one fp16 term
    int dk16 = 0;                         // fp16: k-blocks of 16 features, whole double-buffer units; bf16: padded to a multiple of 8
    int gallery_exp = 0;                  // fp16: the gallery was multiplied by 2^gallery_exp (gemm_gallery_scale_)
    bool f64 = false;                     // the nomination state of a float64 training set owned by fir_cls.hip (fir_gemm_f64.h): gh, gnorm, gmax and set[0] only
    const double2* gal2 = nullptr; int dp2 = 0;   // ... its tiled rows: not owned
    // ---- the copies, built by the create ----
    GemmBuf<uint4> gh;                    // fp16 fragments (precision 2)
    GemmBuf<float4> gm;                   // f32 fragments (precision 0)
    GemmBuf<uint4> gb;                    // bf16 hi/lo fragments (precision 1)
    GemmBuf<float> gnorm, gmax;           // |g|^2 per row, and the largest
    GemmBuf<float4> rowmajor;             // row-major f32 copy of the compared features for the re-rank's gathers (absent when HBM is short: the tiled gallery serves)
    // ---- scratch of the calls ----
    GemmScratch set[2];                   // two sets: the re-rank of super-batch i runs on a side stream while super-batch i + 1 is computed
    GemmScratch sc;                       // one pair's scratch of a second-chance round (fir_gemm_fb.h)
    int lists_cap = 0;                    // queries the lists / counts of a set are sized for
    GemmBuf<float> sample;                // f32 / bf16: every sampled proxy of a super-batch (k_gemm_tau), allocated by the first call
    int sample_rows = 0;
    int rt_sample_rows = 0;               // fp16 sample flow: rows sampled (n / 32)
    GemmBuf<float> proxies;               // few-query calls: every row's proxy, proxies_nq x n floats (grown on first use)
    int proxies_nq = 0;
    // ---- uncertified queries, handled on the device in stream order (fir_gemm_fb.h); grown to the largest call seen (gemm_fb_reserve_) ----
    GemmBuf<int> fb_state;                // int[kFbStateWords]: count, count2, notes taken, -, running totals (2 x 64 bit), the first uncertified queries' numbers (fir_gemm_rerank.h)
    GemmBuf<int> ok; size_t ok_cap = 0;   // certificate flags of one call
    GemmBuf<int> fb_list;                 // [ok_cap] queries the first certificate did not hold for
    GemmBuf<int> fb_list2;                // [ok_cap] ... still uncertified after the second-chance rounds
    GemmBuf<float> fb_tau2;               // [ok_cap] the bound a second pass may append below
    size_t fb_lds = 0;                    // dynamic LDS of k_gemm_exact_fb
    int fb_grid = 0;
    int rerank_group = kRerankGroup;      // candidate rows the re-rank stages in LDS at a time
    // ---- streams and events (created with the state, none for a float64 state) ----
    hipStream_t side = nullptr;           // re-ranks, and a host-pointer call's preparations
    hipStream_t copy = nullptr;           // host-pointer calls: the queries of super-batch i + 1 are uploaded under super-batch i's full passes
    hipEvent_t main_done[2] = {nullptr, nullptr}, rerank_done[2] = {nullptr, nullptr}, prep_done[2] = {nullptr, nullptr}, copy_done[2] = {nullptr, nullptr};
    hipEvent_t queries_ready = nullptr;
    // ---- the int8 nomination of large top-1 batches (fir_gemm_i8.h): built by the first call that takes it (gemm_build_i8_), given back
    // whole when that fails (gemm_free_i8_). Query fragments, norms and scales of an int8 super-batch use the sets above ----
    int i8_tile = -1;                     // the int8 pass's 256-query tile (fir_gemm_set_int8_tile_): -1 the rule, 0 never, 1 whenever the shape allows
    int i8_mode = 0;                      // what the gallery handle allows the next call (fir_gemm_set_int8_): 0 never, 1 every eligible call, -1 the automatic rule
    bool i8_built = false, i8_off = false;   // i8_off: this gallery went back to fp16 for good (the automatic rule's R / G, too many second passes, no memory)
    const char* i8_off_why = "";
    std::string i8_note;                  // the kernel name fir_gallery_last_dispatch reports for a call that would have been int8 but for i8_off
    int dk8 = 0;                          // one-KiB int8 pieces per row block: whole units of 256 features
    GemmBuf<uint4> g8;                    // the int8 copy
    GemmBuf<float> i8_mu, i8_gnorm;       // column means; |c_g|^2
    GemmBuf<float> i8_par;                // max|c_g|, s_g, G^2, R
    float i8_R = 0.f, i8_G = 0.f;         // host copies, read once when the copy is built
    int* i8_pin = nullptr;                // pinned: the second-pass counter of the most recent int8 call, copied behind it ...
    hipEvent_t i8_ev = nullptr;           // ... and the event that says it has arrived (queried, never waited for)
    bool i8_pending = false;
    int i8_pending_qb = 0;
    // ---- knobs, each read once when the state is created (gemm_read_knobs_) ----
    int adaptive = 1;                     // fp16 top-1: the append threshold is found during the full pass (k_gemm_proxy_f16x<3, *>), no sample pass
                                          // (profiles/r03_adaptive_threshold.txt); FIR_GEMM_ADAPTIVE=0: the sample flow, 2: the pass on the way whatever the shape
    int adaptive_topk = 1;                // ... and for the K nearest rows (k_gemm_proxy_f16x<4, *>: K slot minima per query); FIR_GEMM_ADAPTIVE_TOPK=0: the sample flow
    int class_sample_div = 64;            // distinct classes: the bound's row sample is max(kClassSampleRows, n K / this) rows (FIR_GEMM_CLASS_SAMPLE_DIV: experiments; any size is sound)
    // audit knobs, honoured by the audit build only and never set in production
    float erel_scale = 1.0f;              // the certificate's relative error bound is multiplied by this (FIR_GEMM_EREL_SCALE); tests/test_gpu_gemm.py shows that a bound
                                          // shrunk to a quarter returns a wrong row on a crafted near-tie, i.e. that the suite can see an unsound bound
    int dbg_skip = 0;                     // timing forms (FIR_GEMM_DBG_SKIP): bits 0, 1, 2, 5 = no epilogue / gallery stream / query-fragment re-reads / MFMAs (wrong answers), 8 = stamps
    int adapt_dbg = 0;                    // nt_flags bits 2, 3 of the adaptive pass (FIR_GEMM_ADAPT_DBG): 1 = no refresh, 2 = no exchange of the bound between workgroups (still
                                          // sound: a looser bound appends more -- this is how the tests drive lists into overflow and the second-chance pass on benign data)
    bool debug_counts = false;            // appended rows per query of a call's last super-batch on stderr (FIR_GEMM_DEBUG_COUNTS; synchronises)
    hipEvent_t phase_ev[4] = {nullptr, nullptr, nullptr, nullptr};   // ... and its phases: before / after its preparation, after its full passes, after its re-rank
    std::string dump_phases;              // with FIR_GEMM_DBG_SKIP=256: the file the load-burst timestamps of the last super-batch's first pair go to (FIR_GEMM_DUMP_PHASES)
    // ---- host-side record of the calls ----
    int64_t passes = 0;
    int last_kind = 0;                    // the most recent call, for fir_gemm_nominations_ (tests): 0 = none yet, 1 = gemm_search, 2 = the few-query scan
    int last_b = 0, last_nq = 0;          // ... the scratch set of its last super-batch and that super-batch's queries
    int last_sc_rounds = 0;               // ... the second-chance rounds it queued
    bool last_i8 = false;                 // ... and whether it took the int8 pass (its norms and maximum are then the centred ones)

    fir_gemm() = default;
    fir_gemm(const fir_gemm&) = delete;
    fir_gemm& operator=(const fir_gemm&) = delete;
    // (whoever deletes a state that has run calls waits for them first: fir_gemm_destroy)
    ~fir_gemm() {
        for (hipStream_t s : {side, copy}) if (s) (void)hipStreamDestroy(s);
        for (hipEvent_t ev : {main_done[0], main_done[1], rerank_done[0], rerank_done[1], prep_done[0], prep_done[1], copy_done[0], copy_done[1], queries_ready,
                              phase_ev[0], phase_ev[1], phase_ev[2], phase_ev[3]})
            if (ev) (void)hipEventDestroy(ev);
        gemm_free_i8_(this);                // (the pinned word and its event; the buffers would go by themselves)
    }
    // device bytes beyond the fragment copies and the row-major one (fir_gemm_memory_bytes_)
    size_t scratch_bytes() const {
        return gnorm.cap + gmax.cap + set[0].bytes() + set[1].bytes() + sc.bytes() + sample.cap + proxies.cap + fb_state.cap + ok.cap + fb_list.cap + fb_list2.cap +
               fb_tau2.cap + i8_mu.cap + i8_gnorm.cap + i8_par.cap;
    }
};

// The knobs every kind of state honours (this file's and fir_gemm_f64.h's): each is read once, when the state is created.
static void gemm_read_knobs_(fir_gemm* m) {
    if (const char* w = fir_knob_("FIR_GEMM_ADAPTIVE")) m->adaptive = std::atoi(w);
    if (const char* w = fir_knob_("FIR_GEMM_ADAPTIVE_TOPK")) m->adaptive_topk = std::atoi(w) != 0;
    if (const char* w = fir_knob_("FIR_GEMM_CLASS_SAMPLE_DIV")) m->class_sample_div = std::max(1, std::atoi(w));
#ifdef FIR_AUDIT      // knobs that change answers: the audit build only (libfir_amd_audit.so; fir_internal.h)
    // (the DBG bits k_gemm_proxy_f16x reads; a combination kXTable has no row for runs the shipped form: pick_x)
    if (const char* w = fir_knob_("FIR_GEMM_DBG_SKIP")) m->dbg_skip = std::atoi(w) & (1 | 2 | 4 | 32 | 256);
    if (const char* w = fir_knob_("FIR_GEMM_EREL_SCALE")) m->erel_scale = (float)std::atof(w);
    if (const char* w = fir_knob_("FIR_GEMM_ADAPT_DBG")) m->adapt_dbg = (std::atoi(w) & 3) << 2;
    if (fir_knob_("FIR_GEMM_DEBUG_COUNTS")) m->debug_counts = true;
    if (const char* w = fir_knob_("FIR_GEMM_DUMP_PHASES")) m->dump_phases = w;
#endif
}

// The exact re-rank + certificate of nq queries on `st` (one wave each; k_gemm_rerank<1> for the nearest row, <kTopKMax> for the K
// nearest), from one scratch slot: a scratch set of a super-batch, or a second-chance round's. out_key / ok: of block 0's query, or of
// the call's query 0 for a second-chance round (fb.qmap).
struct RerankSlot {
    const unsigned long long* lists;
    const int* counts;
    const float* tau;
    const float* qnorm;
    const float* eabs = nullptr;          // an int8 super-batch: the per-query absolute term, and the centred rows' largest norm
    const float* gmax = nullptr;
};
static RerankSlot gemm_slot_(const fir_gemm* m, const GemmScratch& s, bool i8) {
    return {s.lists, s.counts, s.tau, s.qnorm, i8 ? (const float*)s.eabs : nullptr, i8 ? (const float*)m->i8_par + 2 : nullptr};
}
// dynamic LDS of the f32 re-rank kernels: rerank_group candidate rows and the query (rerank_lds_f32_)
static size_t gemm_rerank_lds_(const fir_gemm* m) { return (size_t)(m->rerank_group + 1) * (m->dp4 + 1) * sizeof(float4); }
static void gemm_launch_rerank_(fir_gemm* m, hipStream_t st, int nq, const RerankSlot& s, const float* d_queries, float e_rel, int k, uint64_t* out_key, int* ok,
                                const RerankFb& fb) {
    hipLaunchKernelGGL(k == 1 ? k_gemm_rerank<1> : k_gemm_rerank<kTopKMax>, dim3(nq), dim3(64), gemm_rerank_lds_(m), st, s.lists, s.counts, s.tau, m->gal4, d_queries,
                       s.qnorm, s.gmax ? s.gmax : (const float*)m->gmax, m->v.n, m->feat, m->dp4, m->v.row_offset, e_rel, m->rerank_group, k, (unsigned long long*)out_key,
                       ok, m->v.d, (const float4*)m->rowmajor, fb, s.eabs);
}

// fp16: up to kShareMax pairs of passes (x 128 queries) read the gallery together in one launch (k_gemm_proxy_f16x, `share`). Rows longer
// than the LDS tile (query slabs streamed per unit): 16 readers of one range drift apart, kShareStreamed measured better.
constexpr int kShareMax = 16, kShareStreamed = 8;
// fp16: rows longer than the 512 features whose 128-query tile fits LDS take the kernels that stream the query slabs (STREAMED = 1)
static bool gemm_streamed_(const fir_gemm* m) { return m->dk16 > kSlabH; }
// fp16: units (of kRing pieces) per row block as the kernels' ODD has them -- 0 = an even number, 1 = an odd one from three on, 2 = ONE
// unit. Every launch of a 16-row kernel takes its form from here: an ODD = 1 kernel walks a first, a middle and a last unit at least.
static int gemm_odd_(const fir_gemm* m) { return m->dk16 == kRing ? 2 : (m->dk16 / kRing) & 1; }
static int gemm_odd8_(const fir_gemm* m) { return m->dk8 == kRing ? 2 : (m->dk8 / kRing) & 1; }       // ... the int8 form's: units of 256 features
// pairs of passes the next launch takes: the largest power of two within what is left and within cap
static int launch_pairs_(int left, int cap) {
    int P = 1;
    while (P * 2 <= left && P * 2 <= cap) P *= 2;
    return P;
}

// The 16-row kernels: ONE table gives the function and the name fir_gallery_last_dispatch reports for it.
typedef void (*fir_x_fn)(const uint4*, const float*, const uint4*, const float*, int64_t, int64_t, int64_t, int, const float*, unsigned long long*, int*, float*,
                         int, int, int, unsigned int*, int);
struct fir_x_key {
    int mode;               // 1 = append below tau, 2 = the sample pass, 3 / 4 = the threshold found on the way (top-1 / the K nearest)
    bool streamed;          // the query slabs are streamed per unit (gemm_streamed_)
    int odd;                // units per row block: 0 = an even number, 1 = an odd one from three on, 2 = one (gemm_odd_, gemm_odd8_)
    int njb = 8;            // live query blocks: < 8 exists for mode 3 with an even number of units only, anything else takes the whole tile
    bool i8 = false;        // the int8 form (fir_gemm_i8.h): resident tiles only, modes 3 and 1 (the second-chance rounds), units of 256 features
    bool tile = false;      // ... its <3, 0> on a 256-query tile (QH = 2 of fir_gemm_f16x.h): two pairs per workgroup, every gallery fragment multiplied against both
    int dbg = 0;            // the timing forms of FIR_GEMM_DBG_SKIP: instantiated in the audit build only, the shipped library cannot select them
};
struct fir_x_entry {
    fir_x_key key;
    fir_x_fn fn;
    const char* name;
};
#define FIR_X(M, S, O) {{M, S, O}, k_gemm_proxy_f16x<M, S, O>, "fir::k_gemm_proxy_f16x<" #M ", " #S ", " #O ">"}
#define FIR_X_FEW(S, J) {{3, S, 0, J}, k_gemm_proxy_f16x<3, S, 0, 0, J>, "fir::k_gemm_proxy_f16x<3, " #S ", 0, 0, " #J ">"}
#define FIR_X8(M, O) {{M, false, O, 8, true}, k_gemm_proxy_f16x<M, 0, O, 0, 8, 1>, "fir::k_gemm_proxy_i8x<" #M ", " #O ">"}
#define FIR_X_DBG(D) {{3, false, 0, 8, false, false, D}, k_gemm_proxy_f16x<3, 0, 0, D>, "fir::k_gemm_proxy_f16x<3, 0, 0, " #D ">"}
#define FIR_X8_DBG(D) {{3, false, 0, 8, true, false, D}, k_gemm_proxy_f16x<3, 0, 0, D, 8, 1>, "fir::k_gemm_proxy_i8x<3, 0> (timing form " #D ")"}
#define FIR_X8T_DBG(D) {{3, false, 0, 8, true, true, D}, k_gemm_proxy_f16x<3, 0, 0, D, 8, 1, 2>, "fir::k_gemm_proxy_i8x<3, 0> (256-query tile, timing form " #D ")"}
static const fir_x_entry kXTable[] = {
    FIR_X(1, 0, 0), FIR_X(1, 0, 1), FIR_X(1, 1, 0), FIR_X(1, 1, 1), FIR_X(2, 0, 0), FIR_X(2, 0, 1), FIR_X(2, 1, 0), FIR_X(2, 1, 1),
    FIR_X(3, 0, 0), FIR_X(3, 0, 1), FIR_X(3, 1, 0), FIR_X(3, 1, 1), FIR_X(4, 0, 0), FIR_X(4, 0, 1), FIR_X(4, 1, 0), FIR_X(4, 1, 1),
    FIR_X_FEW(0, 1), FIR_X_FEW(1, 1), FIR_X_FEW(0, 2), FIR_X_FEW(1, 2),     // a call of <= 16 / <= 32 queries (top-1, threshold found on the way)
    FIR_X(1, 0, 2), FIR_X(2, 0, 2), FIR_X(3, 0, 2), FIR_X(4, 0, 2),         // one unit per row block (at most 128 features; resident by definition)
#ifdef FIR_AUDIT
    // wrong answers: 1, 2, 3, 5, 7 (bit 0 = no epilogue, bit 1 = no gallery stream, bit 2 = no query-fragment re-reads), 33 / 37 / 35 (no MFMAs, no epilogue:
    // both streams / the gallery stream alone / the re-reads alone). Right answers: 256 timestamps of workgroup 0's load bursts (FIR_GEMM_DUMP_PHASES)
    FIR_X_DBG(1), FIR_X_DBG(2), FIR_X_DBG(3), FIR_X_DBG(5), FIR_X_DBG(7), FIR_X_DBG(256), FIR_X_DBG(33), FIR_X_DBG(37), FIR_X_DBG(35),
#endif
    FIR_X8(3, 0), FIR_X8(3, 1), FIR_X8(3, 2), FIR_X8(1, 0), FIR_X8(1, 1), FIR_X8(1, 2),
    {{3, false, 0, 8, true, true}, k_gemm_proxy_f16x<3, 0, 0, 0, 8, 1, 2>, "fir::k_gemm_proxy_i8x<3, 0> (256-query tile)"},
#ifdef FIR_AUDIT
    FIR_X8_DBG(1), FIR_X8_DBG(3), FIR_X8_DBG(5), FIR_X8_DBG(7), FIR_X8_DBG(33), FIR_X8_DBG(35), FIR_X8_DBG(37),
    FIR_X8T_DBG(1), FIR_X8T_DBG(3), FIR_X8T_DBG(5), FIR_X8T_DBG(7), FIR_X8T_DBG(33), FIR_X8T_DBG(35), FIR_X8T_DBG(37),
#endif
};
#undef FIR_X
#undef FIR_X_FEW
#undef FIR_X8
#undef FIR_X_DBG
#undef FIR_X8_DBG
#undef FIR_X8T_DBG
static const fir_x_entry* lookup_x(const fir_x_key& k) {
    for (const fir_x_entry& e : kXTable)
        if (e.key.mode == k.mode && e.key.streamed == k.streamed && e.key.odd == k.odd && e.key.njb == k.njb && e.key.i8 == k.i8 && e.key.tile == k.tile && e.key.dbg == k.dbg)
            return &e;
    return nullptr;
}
// the shipped form a call of this shape runs, and is reported as running (dbg is not looked at)
static const fir_x_entry& find_x(fir_x_key k) {
    k.dbg = 0;
    if (k.i8) {
        k.streamed = false; k.njb = 8;
        if (k.tile) { k.mode = 3; k.odd = 0; }
        const fir_x_entry* e = lookup_x(k);
        return e ? *e : *lookup_x({3, false, 0, 8, true});                     // (not a form of the int8 pass: as its <3, 0>)
    }
    k.tile = false;
    if (!(k.mode == 3 && !k.odd && (k.njb == 1 || k.njb == 2))) k.njb = 8;
    if (const fir_x_entry* e = lookup_x(k)) return *e;
    if (const fir_x_entry* e = lookup_x({2, k.streamed, k.odd})) return *e;    // (not a mode: as the sample pass, which the table has for every shape)
    return *lookup_x({2, false, 0});                                           // (not a shape either: the sample pass of the even resident form)
}
// the function a launch takes: a timing form where one is asked for and exists (whatever njb), the shipped form otherwise
static fir_x_fn pick_x(fir_x_key k) {
    if (k.dbg) k.njb = 8;
#ifdef FIR_AUDIT
    if (k.dbg && k.mode == 3 && !k.streamed && !k.odd) {
        if (const fir_x_entry* e = lookup_x(k)) return e->fn;
    }
#endif
    return find_x(k).fn;
}
// every shipped kernel of the table may take the whole query tile as dynamic LDS
static hipError_t gemm_x_lds_attr_() {
    for (const fir_x_entry& e : kXTable) {
        if (e.key.dbg) continue;
        const hipError_t err = hipFuncSetAttribute((const void*)e.fn, hipFuncAttributeMaxDynamicSharedMemorySize, kHalfLds);
        if (err != hipSuccess) return err;
    }
    return hipSuccess;
}

// What a launch of the 16-row pass reads of the gallery: the fp16 copy, or the int8 one with the centred rows' norms.
struct GemmOperand {
    const uint4* frag;
    const float* gnorm;
    int dk;                 // one-KiB pieces per row block (dk16 | dk8)
};
static GemmOperand gemm_operand_(const fir_gemm* m, bool i8) {
    if (i8) return {m->g8, m->i8_gnorm, m->dk8};
    return {m->gh, m->gnorm, m->dk16};
}
// the set's per-query bound a launch appends below; the sample pass appends nothing and gets tau, lists and counts as the set has them
enum GemmBound { kBelowTau, kBelowAwin, kSampleOnly };
// the kernel's remaining arguments
struct GemmXRest {
    bool qnorm;             // the kernel's `qnorm` <- the pairs' |q|^2 (the threshold found on the way), NULL otherwise
    int nt_flags;
    unsigned int* words;    // `smin`: smin (the sample pass) or aT of the set, or the uncertified list's length (a second-chance round), ...
    int words_per_query;    // ... and how far a query of the set moves it
    int sub_stride;
    int tile_pairs = 1;     // pairs of a workgroup's tile: `share` counts tiles
};
// ONE launch of a 16-row kernel on `st`: pairs [p0, p0 + P) of scratch set s against rows [0, row_end) of the n, every rb_stride-th row block
static void gemm_launch_x_(fir_x_fn fn, dim3 grid, hipStream_t st, const GemmOperand& op, const GemmScratch& s, int p0, int P, int64_t n, int64_t row_end,
                           int rb_stride, GemmBound bound, const GemmXRest& r) {
    const size_t q0 = (size_t)p0 * 2 * kQT, qa = bound == kSampleOnly ? 0 : q0;
    hipLaunchKernelGGL(fn, grid, dim3(kGemmBlock), kHalfLds, st, op.frag, op.gnorm, s.qbf + (size_t)p0 * 4 * op.dk * 64, s.qinv + q0, n, (int64_t)0, row_end,
                       op.dk, (bound == kBelowAwin ? s.awin : s.tau) + qa, s.lists + qa * kListCap, s.counts + qa, r.qnorm ? s.qnorm + q0 : (float*)nullptr,
                       P / r.tile_pairs, r.nt_flags, rb_stride, r.words ? r.words + q0 * r.words_per_query : (unsigned int*)nullptr, r.sub_stride);
}

// (the int8 copy and what goes with it; also what a build that failed gives back)
static void gemm_free_i8_(fir_gemm* m) {
    for (FirBuf* b : std::initializer_list<FirBuf*>{&m->g8, &m->i8_mu, &m->i8_gnorm, &m->i8_par, &m->set[0].eabs, &m->set[1].eabs, &m->sc.eabs}) b->release();
    if (m->i8_pin) (void)hipHostFree(m->i8_pin);
    if (m->i8_ev) (void)hipEventDestroy(m->i8_ev);
    m->i8_pin = nullptr; m->i8_ev = nullptr;
    m->i8_built = false;
}

// ---- what the two creates (fir_gemm_create_range_ex_ here, fir_gemm_create_f64_ in fir_gemm_f64.h) share ----
// The buffers a create allocates, in the order it allocates them: states live next to small per-handle buffers whose placement a
// call's time depends on (profiles/cls_host_side.txt section 3), so number, sizes and order of the allocations are part of the design.
struct GemmAlloc {
    FirBuf* buf;
    size_t bytes;
    bool wanted;
};
static hipError_t gemm_alloc_(hipError_t e, std::initializer_list<GemmAlloc> table) {
    for (const GemmAlloc& a : table)
        if (e == hipSuccess && a.wanted) e = a.buf->reserve(a.bytes);
    return e;
}
// one scratch set for kPasses passes, all but lists and counts (gemm_grow_lists_) and eabs (gemm_build_i8_)
static hipError_t gemm_alloc_set_(hipError_t e, GemmScratch& s, size_t qbf_bytes) {
    const size_t per_query = (size_t)kPasses * kQT * 4;
    return gemm_alloc_(e, {{&s.qbf, qbf_bytes, true}, {&s.qnorm, per_query, true}, {&s.qmul, per_query, true}, {&s.qinv, per_query, true},
                           {&s.smin, kRtSubsets * per_query, true},       // top-K: one minimum per subset
                           {&s.tau, per_query, true}, {&s.awin, per_query, true},
                           {&s.aT, 8 * per_query, true}});                // (x 8: the K slot words of the K-nearest form)
}
// fp16: one power-of-two scale for the whole gallery -- its largest |value|, h_max, lands in [2^13, 2^14). Sets gallery_exp and returns
// the factor the packer multiplies by; 0 with a non-finite gallery value, where every query is left to the exact scan.
static float gemm_gallery_scale_(fir_gemm* m, float h_max) {
    int ex = 0;
    if (h_max > 0.f && h_max < __builtin_huge_valf()) { (void)std::frexp(h_max, &ex); m->gallery_exp = 14 - ex; }
    else m->gallery_exp = h_max > 0.f ? 1000 : 0;
    return (m->gallery_exp >= -100 && m->gallery_exp <= 100) ? std::ldexp(1.0f, m->gallery_exp) : 0.f;
}
// The certificate's relative error bound. fp16: both operands rounded to 11 bits -> |q~.g~ - q.g| <= (2^-10 + 2^-22) sum|q_k g_k| + the
// sub-normal tails (< 2^-27 |q||g| for d <= 2^20), doubled in p and with |q||g| <= (|q|^2 + max|g|^2) / 2: 2^-10 (1 + 2^-4) covers it.
// An int8 call: what is not relative is the query's eabs (fir_gemm_i8.h).
static float gemm_e_rel_(const fir_gemm* m, bool i8) {
    const float products = i8 ? 0.0f : m->precision == FIR_GEMM_BF16_SPLIT ? 6.1035156e-5f : m->precision == FIR_GEMM_F16 ? 9.765625e-4f * 1.0625f : 0.0f;
    return m->erel_scale * (8.0f * (float)m->feat * 5.9604645e-8f + products);
}

extern "C" {

int fir_gemm_create(fir_gallery* g, fir_gemm** out) { return fir_gemm_create_range(g, FIR_GEMM_F16, 0, out); }

int fir_gemm_create_ex(fir_gallery* g, int32_t precision, fir_gemm** out) { return fir_gemm_create_range(g, precision, 0, out); }

int fir_gemm_create_range(fir_gallery* g, int32_t precision, int32_t end_pos, fir_gemm** out) { return fir_gemm_create_range_ex_(g, precision, end_pos, -1, out); }

uint64_t fir_gemm_generation_(const fir_gemm* m) { return m ? m->v.generation : 0; }

void fir_gemm_memory_bytes_(const fir_gemm* m, int64_t* fragments, int64_t* rowmajor, int64_t* scratch) {
    if (fragments) *fragments = (int64_t)(m->gh.cap + m->gb.cap + m->gm.cap + m->g8.cap);
    if (rowmajor) *rowmajor = (int64_t)m->rowmajor.cap;
    if (scratch) *scratch = (int64_t)m->scratch_bytes();
}

int fir_gemm_create_range_ex_(fir_gallery* g, int32_t precision, int32_t end_pos, int32_t rowmajor_mode, fir_gemm** out) {
    if (!g || !out) return fir_fail_(FIR_ERR_ARG, "NULL argument");
    if (precision != FIR_GEMM_F32 && precision != FIR_GEMM_BF16_SPLIT && precision != FIR_GEMM_F16)
        return fir_fail_(FIR_ERR_ARG, "bad precision %d", precision);
    *out = nullptr;
    fir_gemm* m = new (std::nothrow) fir_gemm();
    if (!m) return fir_fail_(FIR_ERR_NOMEM, "host allocation failed");
    m->g = g;
    const void* gp = nullptr;
    if (fir_gallery_view_(g, &m->v) != FIR_OK || fir_gallery_tiled_(g, &gp, &m->dp4) != FIR_OK) { delete m; return fir_fail_(FIR_ERR_ARG, "bad gallery"); }
    m->gal4 = (const float4*)gp;
    m->precision = precision;
    if (precision == FIR_GEMM_F16 && !(m->v.cus >= 8 && (m->v.cus & 7) == 0)) {     // (as fir_gemm_create_f64_; no gfx950 partition mode has such a count)
        const int cus = m->v.cus;
        delete m;
        return fir_fail_(FIR_ERR_ARG, "the 16-row kernels want CUs in eights (%d)", cus);
    }
    // a prefix [0, end_pos) of every row (the reference's "BF, 64" / "BF, 256" classifiers, ImageTesting.cpp:526-529): its own
    // fp16 fragments and row norms; whole 16-feature k-blocks, fp16 form only
    m->feat = end_pos > 0 && end_pos < m->v.d ? end_pos : m->v.d;
    if (end_pos < 0 || end_pos > m->v.d || (m->feat != m->v.d && (m->feat % 16 != 0 || precision != FIR_GEMM_F16))) {
        const int dd = m->v.d;
        delete m;
        return fir_fail_(FIR_ERR_ARG, "feature prefix [0,%d) of %d: multiples of 16 inside the row, fp16 form only", end_pos, dd);
    }
    m->dq8 = (m->feat + 31) / 32 * 4;     // feature groups of 8, padded to a multiple of 4 groups (zeros)
    m->dk16 = (m->feat + 127) / 128 * 8;  // k-blocks of 16, padded to a multiple of 8 (the paired-pass kernel's double-buffer unit)
    if (precision == FIR_GEMM_F16) m->dk16 = (m->feat + 16 * kRing - 1) / (16 * kRing) * kRing;   // ... to whole double-buffer units
    const bool f32 = precision == FIR_GEMM_F32, bf16 = precision == FIR_GEMM_BF16_SPLIT, f16 = precision == FIR_GEMM_F16;
    hipError_t e = hipSetDevice(m->v.device);
    const int64_t rblocks = (std::max<int64_t>(m->v.n, 1) + 31) / 32;
    const int64_t np = std::max<int64_t>(m->v.n, 1);
    e = gemm_alloc_(e, {{&m->gm, (size_t)rblocks * m->dq8 * 64 * sizeof(float4), f32},
                        {&m->gb, (size_t)rblocks * m->dk16 * 128 * sizeof(uint4), bf16},
                        {&m->gh, (size_t)rblocks * m->dk16 * 64 * sizeof(uint4), f16},
                        {&m->gnorm, (size_t)np * sizeof(float), true},
                        {&m->gmax, 16, true}});
    const size_t qbf_bytes = f32 ? (size_t)kPasses * (kQT / 32) * m->dq8 * 64 * sizeof(float4) : (size_t)kPasses * (kQT / 32) * m->dk16 * (bf16 ? 128 : 64) * sizeof(uint4);
    for (int b = 0; b < 2; ++b) {
        e = gemm_alloc_set_(e, m->set[b], qbf_bytes);
        for (hipEvent_t* ev : {&m->main_done[b], &m->rerank_done[b], &m->prep_done[b]})
            if (e == hipSuccess) e = hipEventCreateWithFlags(ev, hipEventDisableTiming);
    }
    if (e == hipSuccess) e = hipEventCreateWithFlags(&m->queries_ready, hipEventDisableTiming);
    if (e == hipSuccess) e = hipStreamCreateWithFlags(&m->side, hipStreamNonBlocking);
    if (e == hipSuccess) e = hipStreamCreateWithFlags(&m->copy, hipStreamNonBlocking);
    for (int b = 0; b < 2 && e == hipSuccess; ++b) e = hipEventCreateWithFlags(&m->copy_done[b], hipEventDisableTiming);
    m->sample_rows = (int)std::min<int64_t>(np, std::max<int64_t>(kMinSampleRows, np / 64));
    m->rt_sample_rows = (int)std::min<int64_t>(np, std::max<int64_t>(kMinSampleRows, np / 32));    // n/16 .. n/48 measured: 1.022 / 1.038 / 1.028 M queries/s at 1M x 512
    if (const char* w = fir_knob_("FIR_GEMM_SAMPLE_DIV"))      // experiments
        m->rt_sample_rows = (int)std::min<int64_t>(np, std::max<int64_t>(kMinSampleRows, np / std::max(1, std::atoi(w))));
    e = gemm_alloc_(e, {{&m->fb_state, kFbStateWords * sizeof(int), true}});
    if (e == hipSuccess) e = hipMemset(m->fb_state, 0, kFbStateWords * sizeof(int));
    e = gemm_alloc_(e, {{&m->sc.qnorm, kScQueries * sizeof(float), true},
                        {&m->sc.qmul, kScQueries * sizeof(float), true},
                        {&m->sc.qinv, kScQueries * sizeof(float), true},
                        {&m->sc.tau, kScQueries * sizeof(float), true},
                        {&m->sc.counts, kScQueries * sizeof(int), true},
                        {&m->sc.lists, (size_t)kScQueries * kListCap * sizeof(unsigned long long), f16},
                        {&m->sc.qbf, (size_t)4 * m->dk16 * 64 * sizeof(uint4), f16}});
    {   // the exact device scan of the uncertified rest keeps eight queries in LDS
        m->fb_lds = (size_t)m->dp4 * 4 * 8 * sizeof(float);
        if (m->fb_lds > kRerankLdsMax) {
            const int dd = m->v.d;
            fir_gemm_destroy(m);
            return fir_fail_(FIR_ERR_ARG, "rows of %d features are too long for the matrix-core path's exact fallback", dd);
        }
        if (e == hipSuccess && m->fb_lds > 48 * 1024)
            e = hipFuncSetAttribute((const void*)k_gemm_exact_fb, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kRerankLdsMax);
        const int per_cu = (int)std::max<size_t>(1, std::min<size_t>(4, (size_t)(160 * 1024) / std::max<size_t>(m->fb_lds, 1)));
        m->fb_grid = std::max(1, m->v.cus) * per_cu;
    }
    const int lds_bytes = f32 ? (kQT / 32) * std::min(m->dq8, kSlab8) * 64 * (int)sizeof(float4) : (kQT / 32) * std::min(m->dk16, kSlab16) * 128 * (int)sizeof(uint4);
    for (const void* fn : {(const void*)k_gemm_proxy<0>, (const void*)k_gemm_proxy<1>, (const void*)k_gemm_proxy_bf16<0>, (const void*)k_gemm_proxy_bf16<1>})
        if (e == hipSuccess) e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, lds_bytes);
    if (e == hipSuccess) e = hipFuncSetAttribute((const void*)k_gemm_proxy_bf16_wide, hipFuncAttributeMaxDynamicSharedMemorySize, kWideLds);
    {   // The re-rank keeps the query and up to kRerankGroup candidate rows in LDS. At least six fit: the check above has let through rows
        // of at most kRerankLdsMax / 128 = 1152 float4, 18 448 bytes with the padding, and kRerankLdsMax holds seven of those and the query.
        const size_t row_bytes = (size_t)(m->dp4 + 1) * sizeof(float4);
        m->rerank_group = (int)std::min<size_t>(kRerankGroup, kRerankLdsMax / row_bytes - 1);
        // (k_gemm_rerank_knn adds 3 KiB of static LDS -- its histogram and sorted keys -- to the request: 147 KiB of the CU's 160 at most)
        static_assert(kRerankLdsMax + 256 * sizeof(unsigned) + fir::kKnnGemmMax * sizeof(unsigned long long) <= 160 * 1024, "k_gemm_rerank_knn's LDS");
        if (gemm_rerank_lds_(m) > 48 * 1024)
            for (const void* fn : {(const void*)k_gemm_rerank<1>, (const void*)k_gemm_rerank<kTopKMax>, (const void*)k_gemm_rerank_classes,
                                   (const void*)k_gemm_rerank_knn, (const void*)k_gemm_rerank_radius})
                if (e == hipSuccess) e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kRerankLdsMax);
    }
    if (e == hipSuccess && f16) e = gemm_x_lds_attr_();
    gemm_read_knobs_(m);
    if (e == hipSuccess && m->v.n > 0) {
        const int64_t n = m->v.n;
        const int d4 = (m->feat + 3) / 4;
        hipStream_t st = m->v.stream;
        // row norms come from the f32 packer (run on a one-group scratch when only the bf16 fragments are kept)
        if (bf16) {
            const int64_t totalb = rblocks * m->dk16 * 64;
            hipLaunchKernelGGL(k_gemm_pack_gallery_bf16, dim3((unsigned)((totalb + 255) / 256)), dim3(256), 0, st, m->gal4, n, m->dp4, m->dk16, m->gb);
            hipLaunchKernelGGL(k_gemm_row_norms, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, m->gal4, n, m->dp4, m->gnorm, d4);
        }
        if (f16) {
            float h_max = 0.f;
            e = hipMemsetAsync(m->gmax, 0, 16, st);
            const int64_t count4 = (int64_t)((n + 63) / 64) * m->dp4 * 64;
            hipLaunchKernelGGL(k_gemm_absmax, dim3((unsigned)std::min<int64_t>((count4 + 255) / 256, 4096)), dim3(256), 0, st, m->gal4, count4, m->gmax);
            if (e == hipSuccess) e = hipMemcpyAsync(&h_max, m->gmax, sizeof(float), hipMemcpyDeviceToHost, st);
            if (e == hipSuccess) e = hipStreamSynchronize(st);
            const float scale = gemm_gallery_scale_(m, h_max);
            const int64_t totalh = rblocks * m->dk16 * 64;
            hipLaunchKernelGGL(k_gemm_pack_gallery_f16x, dim3((unsigned)((totalh + 255) / 256)), dim3(256), 0, st, m->gal4, n, m->dp4, m->dk16, scale, m->gh,
                               m->feat == m->v.d ? m->dp4 * 4 : m->feat);
            hipLaunchKernelGGL(k_gemm_row_norms, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, m->gal4, n, m->dp4, m->gnorm, d4);
        }
        if (f32) {
            const int64_t total = rblocks * m->dq8 * 64;
            hipLaunchKernelGGL(k_gemm_pack_gallery, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, m->gal4, n, m->dp4, m->dq8, m->gm, m->gnorm);
        }
        hipLaunchKernelGGL(k_gemm_max, dim3(1), dim3(256), 0, st, m->gnorm, n, m->gmax);
        // The re-rank's row-major copy of the compared features, when it leaves at least three times its size of HBM free
        // (FIR_GEMM_ROWMAJOR=0 / 1: never / whenever it can be allocated)
        {
            const size_t want = (size_t)n * d4 * sizeof(float4);
            size_t free_b = 0, total_b = 0;
            int mode = rowmajor_mode;
            if (const char* w = fir_knob_("FIR_GEMM_ROWMAJOR")) { if (mode < 0) mode = std::atoi(w); }
            const bool room = hipMemGetInfo(&free_b, &total_b) == hipSuccess && free_b >= 4 * want;
            if (mode != 0 && (room || mode > 0) && m->rowmajor.reserve(want) == hipSuccess) {
                const int64_t tiles = (n + 63) / 64;
                for (int64_t t0 = 0; t0 < tiles; t0 += 65535 * 16) {      // gridDim.x limit: slabs of tiles
                    const int64_t nt = std::min<int64_t>(tiles - t0, 65535 * 16);
                    hipLaunchKernelGGL(k_gemm_untile, dim3((unsigned)nt, (unsigned)((d4 + 31) / 32)), dim3(256), 0, st, m->gal4 + (size_t)t0 * m->dp4 * 64,
                                       n - t0 * 64, m->dp4, d4, m->rowmajor + (size_t)t0 * 64 * d4);
                }
            } else (void)hipGetLastError();         // (no copy: a failed reserve leaves the buffer empty)
        }
        e = hipGetLastError();
        if (e == hipSuccess) e = hipStreamSynchronize(st);
    }
    if (e != hipSuccess) {
        const int rc = fir_fail_(e == hipErrorOutOfMemory ? FIR_ERR_NOMEM : FIR_ERR_HIP, "GEMM-path setup: %s", hipGetErrorString(e));
        fir_gemm_destroy(m);
        return rc;
    }
    *out = m;
    return FIR_OK;
}

int fir_gemm_destroy(fir_gemm* m) {
    if (!m) return FIR_OK;
    (void)hipSetDevice(m->v.device);
    (void)fir_gallery_wait_calls_(m->g);      // calls queued on the callers' streams may still use what the state frees
    if (m->v.stream || !m->f64) (void)hipStreamSynchronize(m->v.stream);
    for (hipStream_t s : {m->side, m->copy}) if (s) (void)hipStreamSynchronize(s);
    delete m;
    return FIR_OK;
}

// out[0] = 64-query passes queued so far, out[1] = queries whose first certificate did not hold (they took a second matrix-core
// pass or, beyond its rounds, went straight to the exact device scan), out[2] = queries the exact device scan answered. The two
// counters live on the device (fir_gemm_fb.h): this call waits for the device's work and reads them.
int fir_gemm_stats_ex(const fir_gemm* m, int64_t out[3]) {
    if (!m || !out) return fir_fail_(FIR_ERR_ARG, "NULL argument");
    FIR_HIP(hipSetDevice(m->v.device));
    FIR_HIP(hipDeviceSynchronize());
    unsigned long long tot[2] = {0, 0};
    FIR_HIP(hipMemcpy(tot, m->fb_state + 4, sizeof tot, hipMemcpyDeviceToHost));
    out[0] = m->passes;
    out[1] = (int64_t)tot[0];
    out[2] = (int64_t)tot[1];
    return FIR_OK;
}

// What the first (up to 8) queries whose FIRST certificate did not hold looked like, since this state was created: per query four
// floats -- entries its candidate list was asked to take (4096 fit), the bound the pass appended below (|g|^2 - 2 q.g units), the
// smallest stored proxy (the K-th smallest for the K nearest), |q|^2. *count = how many of the 8 slots are filled. Diagnostics for
// a benchmark line: a bound of +inf with a million entries is a pass that never found its threshold, a finite one with a few
// thousand a threshold that stayed loose.
int fir_gemm_uncertified_notes(const fir_gemm* m, float out[32], int32_t* count) {
    if (!m || !out || !count) return fir_fail_(FIR_ERR_ARG, "NULL argument");
    FIR_HIP(hipSetDevice(m->v.device));
    FIR_HIP(hipDeviceSynchronize());
    int h[kFbStateWords];
    FIR_HIP(hipMemcpy(h, m->fb_state, sizeof h, hipMemcpyDeviceToHost));
    *count = h[2] < 8 ? h[2] : 8;
    std::memcpy(out, h + 8, 32 * sizeof(float));
    return FIR_OK;
}

int fir_gemm_stats(const fir_gemm* m, int64_t* passes, int64_t* fallback_queries) {
    int64_t o[3];
    const int rc = fir_gemm_stats_ex(m, o);
    if (rc) return rc;
    if (passes) *passes = o[0];
    if (fallback_queries) *fallback_queries = o[2];
    return FIR_OK;
}

}  // extern "C"

// Everything a call still owes its uncertified queries, queued on `st` behind the last re-rank (fir_gemm_fb.h): second-chance rounds
// (sc_rounds > 0: the 16-row fp16 flow only), the collection of what is left, the exact device scan (K launches for the K nearest).
static int gemm_finish_(fir_gemm* m, const float* d_queries, int k, uint64_t* d_keys, hipStream_t st, float e_rel, int sc_rounds, bool streamed, bool i8 = false) {
    const int d = m->feat, qs = m->v.d;
    const int64_t n = m->v.n;
    const GemmOperand op = gemm_operand_(m, i8);
    GemmScratch& s = m->sc;
    // (an int8 call's rounds stay int8: tau2 is in the units of the centred int8 proxies)
    const fir_x_fn round_fn = pick_x({1, i8 ? false : streamed, i8 ? gemm_odd8_(m) : gemm_odd_(m), 8, i8});
    for (int r = 0; r < sc_rounds; ++r) {
        const int off = r * kScQueries;
        if (i8) {
            hipLaunchKernelGGL(k_gemm_qprep_i8, dim3(kScQueries), dim3(64), 0, st, d_queries, kScQueries, d, qs, (const float*)m->i8_mu, (const float*)m->i8_par, e_rel,
                               m->erel_scale, s.qnorm, s.qmul, s.qinv, s.eabs, s.counts, (float*)nullptr, (unsigned int*)nullptr, (int*)nullptr,
                               (const int*)m->fb_state, (const int*)m->fb_list, off, (const float*)m->fb_tau2, s.tau);
            hipLaunchKernelGGL(k_gemm_pack_queries_i8, dim3((4 * op.dk * 64 + 255) / 256, 1), dim3(256), 0, st, d_queries, kScQueries, d, op.dk, (const float*)m->i8_mu,
                               (const float*)s.qmul, s.qbf, qs, (const int*)m->fb_list + off, (const int*)m->fb_state, off);
        } else {
            hipLaunchKernelGGL(k_gemm_sc_prep, dim3(kScQueries), dim3(64), 0, st, d_queries, d, qs, m->gallery_exp, (const int*)m->fb_state, (const int*)m->fb_list, off,
                               (const float*)m->fb_tau2, s.qnorm, s.qmul, s.qinv, s.tau, s.counts);
            hipLaunchKernelGGL(k_gemm_pack_queries_f16x, dim3((4 * op.dk * 64 + 255) / 256, 1), dim3(256), 0, st, d_queries, kScQueries, d, op.dk, (const float*)s.qmul,
                               s.qbf, qs, (const int*)m->fb_list + off, (const int*)m->fb_state, off);
        }
        // one pair over all CUs (share = 1: 256 row ranges), the gallery stream read once (nt)
        gemm_launch_x_(round_fn, dim3(m->v.cus, 1), st, op, s, 0, 1, n, n, 1, kBelowTau, {false, 1, m->fb_state.as<unsigned int>(), 0, off});
        gemm_launch_rerank_(m, st, kScQueries, gemm_slot_(m, s, i8), d_queries, e_rel, k, d_keys, m->ok, {m->fb_state, nullptr, nullptr, 0, (const int*)m->fb_list + off, off});
    }
    hipLaunchKernelGGL(k_gemm_fb_collect, dim3(1), dim3(256), 0, st, m->fb_state, (const int*)m->fb_list, (const int*)m->ok, m->fb_list2, (unsigned long long*)d_keys, k);
    for (int r = 0; r < k; ++r)
        hipLaunchKernelGGL(k_gemm_exact_fb, dim3(m->fb_grid), dim3(256), m->fb_lds, st, m->gal4, n, m->dp4, d, m->v.row_offset, d_queries, qs, (const int*)m->fb_state,
                           (const int*)m->fb_list2, (unsigned long long*)d_keys, k, r);
    FIR_HIP(hipGetLastError());
    return FIR_OK;
}

// ---- one search call ----
// d_queries / d_keys: device pointers. Everything is queued on `stream` (and the handle's side streams, joined before the call
// returns control of `stream`): no host synchronisation -- the keys are final in stream order.
//
// super-batch = the queries of ONE set of launches (preparation, full passes, re-rank): up to kPasses passes of 64 queries.
// Two streams. `st` carries the full passes over the gallery, back to back; `side` carries the exact re-rank + certificate of
// super-batch i under super-batch i+1's full passes, and (host-pointer calls) the preparation of super-batch i+1 -- query norms /
// scales / fragments, the sample pass, tau -- behind its upload. prep(i+2) reuses the scratch set rerank(i) has just finished with.
struct GemmCall {
    const float* d_queries;
    const float* h_queries;     // non-NULL: the queries are still in host memory; d_queries is the device buffer they go to, one super-batch
                                // at a time, each upload queued (on its own stream) right before that super-batch's preparation
    int32_t qb;
    FirSearch s;                // what is searched for (fir_search_request.h): s.keys[q * s.k + r] ascending; kGemmKinds[s.kind] says how this file answers the kind
    int knn_div = fir::kKnnSampleDiv;   // kSearchSelect: the bound from a row sample's exact K-th distance (rows n K / knn_div: FIR_GEMM_KNN_SAMPLE_DIV)
    hipStream_t st;
    int d, qs;                  // features compared; floats between consecutive queries (and gallery rows): the whole row
    int64_t n;
    float e_rel;
    int grid;                   // one 512-thread workgroup per CU
    int sbq, nsb;               // queries per super-batch, super-batches of the call
    // A super-batch's preparation (query packing, the top-K sample pass) runs on the MAIN stream right in front of its full passes: alone on
    // the chip it is 25 us (top-K: + 0.3 ms of sample passes); on the side stream, "under" the previous super-batch's full passes, its small
    // kernels only got the CUs a full-pass workgroup had just left and slowed those passes down (1M x 512, 32 768 queries per call: top-1
    // 1.253 -> 1.296 M q/s, top-5 1.018 -> 1.071 M). Host-pointer calls keep the side stream: there the preparation waits for the
    // super-batch's upload, which is what overlaps the passes.
    bool serial_prep;
    // a call of ONE super-batch whose preparation runs on `st` has nothing to put under anything: its re-rank follows its pass on `st`
    // as well -- every hop to the side stream and back is 10-12 us of a 300-us call
    bool one_stream;
    bool streamed;              // fp16: gemm_streamed_
    int odd;                    // fp16: units per row block -- 0 = an even number, 1 = an odd one, 2 = one unit (the kernels' ODD)
    size_t lds;                 // f32 / bf16: dynamic LDS of the pass kernels
    bool i8 = false;            // this call's passes are the int8 form (gemm_wants_i8_): odd is then in units of 256 features, streamed false
    bool i8_went_back = false;  // the automatic rule would have taken the int8 pass, but this gallery went back to fp16: last_dispatch says so

    int sb_queries(int sb) const { return std::min(sbq, qb - sb * sbq); }
    const float* sb_first(int sb) const { return d_queries + (size_t)sb * sbq * qs; }
};
// ---- the kinds of search (fir_search_request.h) as this file answers them: one row per kind, in SearchKind's order. A new kind is a new row, its
// arm in gemm_prep_f16_ (how the bound is made) and in gemm_rerank_ (which kernel), and an exact form. Only kSearchRows has second-chance rounds (gemm_finish_).
struct GemmKind {
    int k_min, k_max;           // the k-limit; its error text is "k=%d outside [1,%d]" (a radius call's max_results is the entry point's to report)
    bool adaptive;              // the fp16 pass may find its bound on the way (adaptive_for_)
    bool i8;                    // the int8 nomination is eligible (gemm_wants_i8_; top-1 only)
    // nq queries answered exactly into `out`, over features [0, c.d) on the call's stream: every query of an empty gallery, each run of uncertified ones
    int (*exact)(fir_gemm* m, const GemmCall& c, const float* dq, int32_t nq, const FirSearch& out);
};
static const GemmKind kGemmKinds[fir::kSearchKinds] = {
    {1, kTopKMax, true, true, [](fir_gemm* m, const GemmCall& c, const float* dq, int32_t nq, const FirSearch& o) {                  // kSearchRows: the exact scans
         return c.s.k == 1 ? fir_search_top1_exact_keys_dev_(m->g, dq, nq, 0, c.d, o.keys, c.st) : fir_search_topk_exact_keys_dev_(m->g, dq, nq, c.d, c.s.k, o.keys, c.st); }},
    {1, fir::kKnnGemmMax, false, false, [](fir_gemm* m, const GemmCall& c, const float* dq, int32_t nq, const FirSearch& o) {       // kSearchSelect: store + select
         return fir_search_knn_keys_dev(m->g, dq, nq, 0, c.d, c.s.k, o.keys, c.st); }},     // (K slot minima per query stop at kTopKMax: the sample flow, fir_gemm_knn.h)
    {0, fir::kKnnGemmMax, false, false, [](fir_gemm* m, const GemmCall& c, const float* dq, int32_t nq, const FirSearch& o) {       // kSearchRadius: store + count + select
         return fir_search_radius_keys_dev(m->g, dq, nq, 0, c.d, o.radius, c.s.k, o.count, o.keys, c.st); }},
    {1, 32, false, false, [](fir_gemm* m, const GemmCall& c, const float* dq, int32_t nq, const FirSearch& o) {                     // kSearchClasses: the class-minimum scan
         return fir_class_scan_dev_(m->g, dq, nq, c.d, o.num_classes, c.s.k, 0, o.keys, o.classes, nullptr, c.st); }},             // (a bound on the K-th CLASS is not a row order statistic)
};

// ---- the int8 nomination: which calls take it, and the copy they need (fir_gemm_i8.h) ----
// The automatic rule's two constants, measured on one MI355X at 1M x 512 (profiles/int8_nomination.txt, tools/int8_nomination_sweep.py;
// fp16 -> int8, M queries/s, identical keys, no second pass anywhere):
//   kI8AutoMinQueries, the smallest call the rule sends to the int8 pass: 2 048 queries per call 1.09 -> 1.90 (x 1.73), 8 192 1.31 -> 2.27,
//     32 768 1.38 -> 2.39, 131 072 1.40 -> 2.43; 512 still gains (0.99 -> 1.37) but was measured once only and stays fp16. 0 compiles
//     the rule out: only fir_gallery_set_int8_nomination(g, 1) then reaches the pass.
//   kI8AutoMaxRG, the largest R / G (the worst row's quantisation residual over the largest centred norm) it is taken at: one row in a
//     thousand with one outlier coordinate of growing size, 32 768 queries per call -- R / G 0.0047 (none) x 1.73, 0.0053 x 1.71, 0.0084
//     x 1.62, 0.0123 x 1.43, 0.0162 x 1.08, 0.0206 x 0.62 (the lists reach into the tail of the row distances), 0.037 x 0.012 (nearly
//     every query ends in the exact device scan). The limit sits behind the last clear gain.
constexpr int kI8AutoMinQueries = FIR_I8_AUTO_MIN_QUERIES;
constexpr float kI8AutoMaxRG = 0.0125f;
// Builds the int8 copy on `st` (one synchronisation). On any failure the state is left as gemm_free_i8_ leaves it.
static int gemm_build_i8_(fir_gemm* m, hipStream_t st) {
    const int64_t n = m->v.n, rblocks = (std::max<int64_t>(n, 1) + 31) / 32, tiles = (n + 63) / 64;
    const int d4 = (m->feat + 3) / 4;
    m->dk8 = (m->feat + 32 * kRing - 1) / (32 * kRing) * kRing;
    auto undo = fir_on_exit([m] { if (!m->i8_built) gemm_free_i8_(m); });
    GemmBuf<double> partial;              // column sums per row slice: this build's only
    int rc = FIR_OK;
    if ((rc = FIR_RESERVE(m->g8, (size_t)rblocks * m->dk8 * 64 * sizeof(uint4)))) return rc;
    if ((rc = FIR_RESERVE(m->i8_mu, (size_t)d4 * 4 * sizeof(float)))) return rc;
    if ((rc = FIR_RESERVE(m->i8_gnorm, (size_t)std::max<int64_t>(n, 1) * sizeof(float)))) return rc;
    if ((rc = FIR_RESERVE(m->i8_par, 8 * sizeof(float)))) return rc;
    for (int b = 0; b < 2; ++b)
        if ((rc = FIR_RESERVE(m->set[b].eabs, kPasses * kQT * sizeof(float)))) return rc;
    if ((rc = FIR_RESERVE(m->sc.eabs, kScQueries * sizeof(float)))) return rc;
    FIR_HIP(hipHostMalloc((void**)&m->i8_pin, 64, hipHostMallocDefault));
    FIR_HIP(hipEventCreateWithFlags(&m->i8_ev, hipEventDisableTiming));
    if ((rc = FIR_RESERVE(partial, (size_t)kI8Slices * d4 * 4 * sizeof(double)))) return rc;
    hipLaunchKernelGGL(k_i8_colsum, dim3(d4, kI8Slices), dim3(256), 0, st, m->gal4, tiles, m->dp4, partial);
    hipLaunchKernelGGL(k_i8_mean, dim3((d4 * 4 + 255) / 256), dim3(256), 0, st, (const double*)partial, d4, m->feat, n, m->i8_mu, m->i8_par);
    hipLaunchKernelGGL(k_i8_rows<0>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, m->gal4, n, m->dp4, m->feat, (const float*)m->i8_mu, m->i8_gnorm, m->i8_par);
    hipLaunchKernelGGL(k_i8_scale, dim3(1), dim3(1), 0, st, m->i8_par);
    hipLaunchKernelGGL(k_i8_rows<1>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, m->gal4, n, m->dp4, m->feat, (const float*)m->i8_mu, m->i8_gnorm, m->i8_par);
    const int64_t total = rblocks * m->dk8 * 64;
    hipLaunchKernelGGL(k_i8_pack_gallery, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, m->gal4, n, m->dp4, m->dk8, m->feat, (const float*)m->i8_mu,
                       (const float*)m->i8_par, m->g8);
    float h[4] = {0.f, 0.f, 0.f, 0.f};
    FIR_HIP(hipGetLastError());
    FIR_HIP(hipMemcpyAsync(h, m->i8_par, sizeof h, hipMemcpyDeviceToHost, st));
    FIR_HIP(hipStreamSynchronize(st));                  // the copy's one synchronisation
    m->i8_G = std::sqrt(h[2]);
    m->i8_R = h[3];
    m->i8_built = true;
    return FIR_OK;
}
// L2 (every fir_gemm state is), top-1, the whole row of at most 1 024 features (the 128-query int8 tile is resident), more than 32
// queries (the few-block forms stay fp16), the fp16 state of an f32 gallery. i8_mode 1 takes every such call; -1 (the gallery handle
// sets it for automatic matrix-core dispatch over at least kAutoMfmaRows rows only) asks the rule, and goes back to fp16 for good
// when more than one query in sixteen of an int8 call needed a second pass -- seen without waiting: the counter is copied to pinned
// memory behind the call and looked at here only once its event has fired.
static int gemm_wants_i8_(fir_gemm* m, GemmCall& c, bool* out) {
    *out = false;
    if (m->i8_pending) {
        const hipError_t eq = hipEventQuery(m->i8_ev);
        if (eq == hipSuccess) {
            m->i8_pending = false;
            if ((int64_t)m->i8_pin[0] * 16 > (int64_t)m->i8_pending_qb) { m->i8_off = true; m->i8_off_why = "second passes"; }
        } else if (eq == hipErrorNotReady) (void)hipGetLastError();     // (not an error: the counter is looked at by a later call)
    }
    if (m->i8_mode == 0 || m->precision != FIR_GEMM_F16 || m->f64 || c.s.k != 1 || !kGemmKinds[c.s.kind].i8 || m->feat != m->v.d || m->feat > 1024 || m->feat < 8 ||
        c.qb <= 32 || (m->dbg_skip && m->i8_mode != 1))        // (the timing forms reach int8 only where the handle asks for int8 outright)
        return FIR_OK;
    if (m->i8_mode < 0 && (kI8AutoMinQueries <= 0 || c.qb < kI8AutoMinQueries)) return FIR_OK;
    if (m->i8_mode < 0 && m->i8_off) { c.i8_went_back = true; return FIR_OK; }
    if (!m->i8_built && m->i8_off) { c.i8_went_back = true; return FIR_OK; }      // (the copy could not be built: not tried again)
    if (!m->i8_built) {
        const int rc = gemm_build_i8_(m, c.st);
        if (rc) {
            // No room for the copy: in EVERY mode this call and all later ones are answered by the fp16 pass (the same keys), what was
            // allocated has been given back, and fir_gallery_last_dispatch says "int8 nomination off for this gallery: no memory". Any
            // other failure is the call's error.
            (void)hipGetLastError();
            if (rc != FIR_ERR_NOMEM) return rc;
            m->i8_off = true; m->i8_off_why = "no memory";
            c.i8_went_back = true;
            return FIR_OK;
        }
        if (!(m->i8_R <= kI8AutoMaxRG * m->i8_G)) { m->i8_off = true; m->i8_off_why = "R / G"; }
    }
    if (m->i8_mode < 0 && m->i8_off) { c.i8_went_back = true; return FIR_OK; }
    if (!m->i8_built) return FIR_OK;
    *out = true;
    return FIR_OK;
}

// Which fp16 super-batches find their threshold on the way. Until round 4's second half the answer depended on how many row groups a
// workgroup sees ((row groups) * (pairs per launch) / CUs: below a dozen the bound is still loose when the workgroup ends, 1 000-2 400
// appended rows per query at 100k x 512 with 256 queries) and such super-batches kept the sample flow. Since an appended row no longer
// waits for the gallery prefetch and a wave's first row block is summed once, the pass on the way is never slower for top-1 and
// 10-23 % faster wherever the sample flow used to run (8 192 .. 700 000 rows x 128 .. 4 096 queries, no second pass anywhere:
// profiles/r04_adaptive_cutoff.txt): top-1 always takes it. The K-nearest form (eight slots per query fill more slowly) wins from eight
// pairs per launch on and on cache-sized galleries, and loses 3-35 % with one or two pairs over 100 000+ rows: those keep the sample flow.
static bool adaptive_for_(const fir_gemm* m, const GemmCall& c, int nq_sb) {
    if (m->precision != FIR_GEMM_F16 || m->adaptive <= 0 || (c.s.k > 1 && !m->adaptive_topk)) return false;
    if (!kGemmKinds[c.s.kind].adaptive) return false;                   // (kGemmKinds says why not)
    if (m->adaptive > 1 || c.s.k == 1) return true;                       // FIR_GEMM_ADAPTIVE=2: always
    const int pairs_sb = ((nq_sb + kQT - 1) / kQT + 1) / 2;
    const int P = launch_pairs_(pairs_sb, c.streamed ? kShareStreamed : kShareMax);
    const int64_t row_groups = ((c.n + 31) / 32 + kGemmBlock / 64 - 1) / (kGemmBlock / 64);
    // (256 queries against 1M x 512 measured 479 k q/s against the sample flow's 514 k, 4 096 queries 1.02 M against 0.92 M --
    // profiles/r04_topk_slots.txt)
    return P >= 8 || c.n <= 65536 || row_groups * P / std::max(c.grid, 1) >= 100;
}

// the per-call buffers of the uncertified-query lists (and the certificate flags), grown to the largest call seen
static int gemm_fb_reserve_(fir_gemm* m, int32_t qb) {
    if ((size_t)qb <= m->ok_cap) return FIR_OK;
    FIR_HIP(hipDeviceSynchronize());                        // (an earlier call's kernels may still read the old ones)
    m->ok_cap = 0;
    for (FirBuf* b : std::initializer_list<FirBuf*>{&m->ok, &m->fb_list, &m->fb_list2, &m->fb_tau2}) b->release();
    const size_t cap = (size_t)std::max(qb, 1024);
    int rc = FIR_OK;
    if ((rc = FIR_RESERVE(m->ok, cap * sizeof(int))) || (rc = FIR_RESERVE(m->fb_list, cap * sizeof(int))) || (rc = FIR_RESERVE(m->fb_list2, cap * sizeof(int))) ||
        (rc = FIR_RESERVE(m->fb_tau2, cap * sizeof(float))))
        return rc;
    m->ok_cap = cap;
    return FIR_OK;
}

// Candidate lists and counts of the first `sets` scratch sets, for super-batches of up to nq queries: sized by the super-batch in use
// (whole 128-query pairs), not by the largest one possible -- a cache-resident gallery that gets 128-query calls holds 8 MiB of lists,
// not 512. Before the old ones go, `wait` is synchronised: the streams whose queued work may still use them.
static int gemm_grow_lists_(fir_gemm* m, int sets, int nq, std::initializer_list<hipStream_t> wait) {
    const int need = (nq + 2 * kQT - 1) / (2 * kQT) * (2 * kQT);
    if (need <= m->lists_cap) return FIR_OK;
    for (hipStream_t s : wait) FIR_HIP(hipStreamSynchronize(s));
    m->lists_cap = 0;
    for (int b = 0; b < sets; ++b) { m->set[b].lists.release(); m->set[b].counts.release(); }
    for (int b = 0; b < sets; ++b) {
        int rc = FIR_OK;
        if ((rc = FIR_RESERVE(m->set[b].lists, (size_t)need * kListCap * sizeof(unsigned long long))) || (rc = FIR_RESERVE(m->set[b].counts, (size_t)need * sizeof(int)))) return rc;
    }
    m->lists_cap = need;
    return FIR_OK;
}

// What a call needs beyond the state's fixed scratch: the lists of its uncertified queries, candidate lists for its super-batches and,
// f32 / bf16, the sample of the order-statistic flow (every sampled proxy), on first use.
static int gemm_reserve_(fir_gemm* m, const GemmCall& c) {
    int rc = gemm_fb_reserve_(m, c.qb);
    if (rc || (rc = gemm_grow_lists_(m, 2, std::min(c.sbq, c.qb), {c.st, m->side}))) return rc;
    if (m->precision != FIR_GEMM_F16) return FIR_RESERVE(m->sample, (size_t)kPasses * kQT * m->sample_rows * sizeof(float));
    return FIR_OK;
}

// The sample flow's sample pass on `st` (k_gemm_proxy_f16x<2, *>): per query of the set's first `pairs` pairs, smin <- the smallest proxy over
// rt_sample_rows rows -- for the K > 1 nearest as kRtSubsets disjoint subsets' minima, kPasses * kQT words apart ...
static int gemm_sample_stride_(int k) { return k > 1 ? kPasses * kQT : 0; }
static int gemm_sample_pass_(fir_gemm* m, const GemmScratch& s, hipStream_t st, bool streamed, int odd, int pairs, int k) {
    const int sub_stride = gemm_sample_stride_(k);
    FIR_HIP(hipMemsetD32Async((hipDeviceptr_t)s.smin, (int)0xFF800000u, sub_stride ? (size_t)kRtSubsets * sub_stride : (size_t)pairs * 2 * kQT, st));
    // every rb_stride-th row block: the sample is spread over the whole gallery
    const int64_t sample_blocks = ((int64_t)m->rt_sample_rows + 31) / 32;
    const int rb_stride = (int)std::max<int64_t>(1, ((m->v.n + 31) / 32) / sample_blocks);
    for (int p0 = 0; p0 < pairs;) {
        const int P = launch_pairs_(pairs - p0, kShareMax);
        gemm_launch_x_(pick_x({2, streamed, odd}), dim3(m->v.cus), st, gemm_operand_(m, false), s, p0, P, m->v.n, sample_blocks * 32, rb_stride, kSampleOnly,
                       {false, P <= 1 ? 1 : 0, s.smin, 1, sub_stride});
        p0 += P;
    }
    return FIR_OK;
}
// ... and the bound from it: tau = the smallest sampled proxy + one window (top-1: k_gemm_tau_min), the K-th smallest of the subsets'
// minima + one window (top-K: k_gemm_tau_kmin)
static void gemm_sample_tau_(fir_gemm* m, const GemmScratch& s, hipStream_t st, int pairs, int nq, int k, float e_rel) {
    if (k > 1)
        hipLaunchKernelGGL(k_gemm_tau_kmin, dim3((pairs * 2 * kQT + 255) / 256), dim3(256), 0, st, s.smin, gemm_sample_stride_(k), k, s.tau, pairs * 2 * kQT, nq, s.qnorm,
                           m->gmax, e_rel);
    else
        hipLaunchKernelGGL(k_gemm_tau_min, dim3((pairs * 2 * kQT + 255) / 256), dim3(256), 0, st, s.smin, s.tau, pairs * 2 * kQT, nq, s.qnorm, m->gmax, e_rel);
}

// fp16 preparation of one super-batch on `ps`: per-query norms and scales, the query fragments and -- unless the full pass finds its
// threshold on the way -- the sample flow (gemm_sample_pass_, gemm_sample_tau_).
static int gemm_prep_f16_(fir_gemm* m, const GemmCall& c, hipStream_t ps, int sb) {
    const int b = sb & 1, nq = c.sb_queries(sb), k = c.s.k;
    GemmScratch& s = m->set[b];
    const int pairs = ((nq + kQT - 1) / kQT + 1) / 2;        // 128 queries per gallery read; a half-filled pair is zero-padded
    const float* dq = c.sb_first(sb);
    if (c.i8) {                                             // (fir_gemm_i8.h: always the threshold found on the way)
        hipLaunchKernelGGL(k_gemm_qprep_i8, dim3(pairs * 2 * kQT), dim3(64), 0, ps, dq, nq, c.d, c.qs, (const float*)m->i8_mu, (const float*)m->i8_par, c.e_rel,
                           m->erel_scale, s.qnorm, s.qmul, s.qinv, s.eabs, s.counts, s.awin, s.aT, sb == 0 ? m->fb_state : (int*)nullptr,
                           (const int*)nullptr, (const int*)nullptr, 0, (const float*)nullptr, (float*)nullptr);
        hipLaunchKernelGGL(k_gemm_pack_queries_i8, dim3((4 * m->dk8 * 64 + 255) / 256, pairs), dim3(256), 0, ps, dq, nq, c.d, m->dk8, (const float*)m->i8_mu,
                           (const float*)s.qmul, s.qbf, c.qs);
        return FIR_OK;
    }
    const bool adaptive = adaptive_for_(m, c, nq);
    // (the candidate counts are cleared, the call's two list lengths by its first super-batch and, for the adaptive pass, the per-query
    // windows and start values are set by the same launch)
    hipLaunchKernelGGL(k_gemm_qprep_f16, dim3(pairs * 2 * kQT), dim3(64), 0, ps, dq, nq, c.d, m->gallery_exp, s.qnorm, s.qmul, s.qinv, c.qs,
                       s.counts, adaptive ? s.awin : (float*)nullptr, adaptive ? s.aT : (unsigned int*)nullptr,
                       (const float*)m->gmax, c.e_rel, k > 1 ? k : 0, (unsigned int*)nullptr, sb == 0 ? m->fb_state : (int*)nullptr);
    hipLaunchKernelGGL(k_gemm_pack_queries_f16x, dim3((4 * m->dk16 * 64 + 255) / 256, pairs), dim3(256), 0, ps, dq, nq, c.d, m->dk16, s.qmul,
                       s.qbf, c.qs);
    if (adaptive) return FIR_OK;
    int rc = FIR_OK;
    if (c.s.kind == fir::kSearchRows) {
        if ((rc = gemm_sample_pass_(m, s, ps, c.streamed, c.odd, pairs, k))) return rc;
        gemm_sample_tau_(m, s, ps, pairs, nq, k, c.e_rel);
        return FIR_OK;
    }
    if (c.s.kind == fir::kSearchClasses) {
        // distinct classes: D_s = the exact K-th smallest class minimum over the leading sample rows (four times list_row_samples' sizing:
        // profiles/class_rank_matrix_cores.txt)
        const int64_t rows = std::min<int64_t>(c.n, std::max<int64_t>(kClassSampleRows, c.n * k / m->class_sample_div));
        rc = fir_class_scan_dev_(m->g, dq, nq, c.d, c.s.num_classes, k, rows, nullptr, nullptr, s.tau, ps);
    } else if (c.s.is_radius())     // (the query's own radius is the bound -- any value: k_gemm_tau_class's guarantee does not ask where it came from)
        FIR_HIP(hipMemcpyAsync(s.tau, c.s.radius + (size_t)sb * c.sbq, (size_t)nq * sizeof(float), hipMemcpyDeviceToDevice, ps));
    else                            // D_s = the exact K-th smallest distance over a row sample spread over the gallery (fir_knn_select.h: knn_sample_plan)
        rc = fir_knn_sample_bound_dev_(m->g, dq, nq, c.d, k, c.knn_div, s.tau, ps);
    if (rc) return rc;
    // the exact bound D_s turned into the append pass's bound in place; padding queries get -inf
    hipLaunchKernelGGL(k_gemm_tau_class, dim3((pairs * 2 * kQT + 255) / 256), dim3(256), 0, ps, s.tau, pairs * 2 * kQT, nq, c.d, s.qnorm, m->gmax, c.e_rel);
    return FIR_OK;
}

// f32 / bf16-split preparation of one super-batch on `ps`: norms, fragments, every proxy of the first sample_rows rows, tau = the
// kCand-th smallest of them (k_gemm_tau)
static int gemm_prep_f32_bf16_(fir_gemm* m, const GemmCall& c, hipStream_t ps, int sb) {
    const int b = sb & 1, nq = c.sb_queries(sb), np = (nq + kQT - 1) / kQT;
    GemmScratch& s = m->set[b];
    const float* dq = c.sb_first(sb);
    const int sample_rows = m->sample_rows, sample_grid = (sample_rows + 63) / 64;
    hipLaunchKernelGGL(k_gemm_qnorm, dim3(np * kQT), dim3(64), 0, ps, dq, nq, c.d, s.qnorm);
    FIR_HIP(hipMemsetAsync(s.counts, 0, (size_t)np * kQT * sizeof(int), ps));
    if (m->precision == FIR_GEMM_F32) {
        hipLaunchKernelGGL(k_gemm_pack_queries, dim3(((kQT / 32) * m->dq8 * 64 + 255) / 256, np), dim3(256), 0, ps, dq, nq, c.d, m->dq8, s.qbf.as<float4>());
        hipLaunchKernelGGL(k_gemm_proxy<0>, dim3(sample_grid, np), dim3(128), c.lds, ps, m->gm, m->gnorm, s.qbf.as<float4>(), c.n, (int64_t)0,
                           (int64_t)sample_rows, m->dq8, s.tau, s.lists, s.counts, m->sample, sample_rows);
    } else {
        hipLaunchKernelGGL(k_gemm_pack_queries_bf16, dim3(((kQT / 32) * m->dk16 * 64 + 255) / 256, np), dim3(256), 0, ps, dq, nq, c.d, m->dk16,
                           s.qbf);
        hipLaunchKernelGGL(k_gemm_proxy_bf16<0>, dim3(sample_grid, np), dim3(128), 0, ps, m->gb, m->gnorm, s.qbf, c.n, (int64_t)0,
                           (int64_t)sample_rows, m->dk16, s.tau, s.lists, s.counts, m->sample, sample_rows);
    }
    hipLaunchKernelGGL(k_gemm_tau, dim3(np * kQT), dim3(256), 0, ps, m->sample, sample_rows, s.tau, 0x7FFFFFFF, s.qnorm, m->gmax, c.e_rel,
                       c.s.k > 1 ? 1 : 0);
    return FIR_OK;
}

// audit builds with FIR_GEMM_DEBUG_COUNTS: phase boundary i of the super-batch in hand, on the stream the phase runs on
static void gemm_audit_mark_(fir_gemm* m, int i, hipStream_t s) {
#ifdef FIR_AUDIT
    if (!m->debug_counts) return;
    if (!m->phase_ev[i]) (void)hipEventCreate(&m->phase_ev[i]);
    if (m->phase_ev[i]) (void)hipEventRecord(m->phase_ev[i], s);
#else
    (void)m; (void)i; (void)s;
#endif
}

// Preparation of super-batch sb: (host-pointer calls) its upload, then everything its full passes need, on the stream GemmCall::serial_prep names
static int gemm_prep_(fir_gemm* m, const GemmCall& c, int sb) {
    hipStream_t ps = c.serial_prep ? c.st : m->side;
    const int b = sb & 1;
    if (c.serial_prep && sb >= 2) FIR_HIP(hipStreamWaitEvent(c.st, m->rerank_done[b], 0));      // the re-rank of sb - 2 read this buffer
    if (c.h_queries) {
        const size_t off = (size_t)sb * c.sbq * c.qs;
        FIR_HIP(hipMemcpyAsync((void*)(c.d_queries + off), c.h_queries + off, (size_t)c.sb_queries(sb) * c.qs * sizeof(float), hipMemcpyHostToDevice, m->copy));
        FIR_HIP(hipEventRecord(m->copy_done[b], m->copy));
        FIR_HIP(hipStreamWaitEvent(ps, m->copy_done[b], 0));
    }
    gemm_audit_mark_(m, 0, ps);
    const int rc = m->precision == FIR_GEMM_F16 ? gemm_prep_f16_(m, c, ps, sb) : gemm_prep_f32_bf16_(m, c, ps, sb);
    if (rc) return rc;
    FIR_HIP(hipGetLastError());
    gemm_audit_mark_(m, 1, ps);
    FIR_HIP(hipEventRecord(m->prep_done[b], ps));
    return FIR_OK;
}

// The fp16 full passes of one super-batch on `st` -- the launches fir_profile_read times and fir_gallery_last_dispatch names. The pairs
// of the super-batch read the gallery together, a power of two of them per launch. Two shapes: the threshold found on the way
// (k_gemm_proxy_f16x<3 | 4, *>, then k_gemm_adapt_final hands the re-rank its bound) or, after the sample flow, append below tau (<1, *>).
// An int8 call (always the threshold found on the way) makes the same launches over the int8 copy -- half the pieces per row block, the
// centred rows' norms -- and differs in its tile: with two units per row block (257-512 features) and two pairs or more in the launch it
// takes the 256-query tile -- P / 2 workgroups share a row range, each with two pairs' queries in LDS (two 64-KiB images fill what the
// fp16 tile takes) and every gallery fragment multiplied against both, so the fragments cross from L2 to the CUs half as often. A
// one-pair launch (the odd pair of a call) and every other row length keep the 128-query forms. Such a launch takes up to 2 kShareMax
// pairs -- sixteen tiles over sixteen row ranges, 4 096 queries per read of the gallery -- which measured 3 % over sixteen pairs from
// 32 768 queries per call on. The rule: always (profiles/int8_tile256.txt).
static int gemm_pass_f16_(fir_gemm* m, const GemmCall& c, int sb) {
    const int b = sb & 1, nq = c.sb_queries(sb), k = c.s.k;
    const int pairs = ((nq + kQT - 1) / kQT + 1) / 2;
    const int64_t n = c.n;
    const GemmOperand op = gemm_operand_(m, c.i8);
    const GemmScratch& s = m->set[b];
    const bool adaptive = c.i8 || adaptive_for_(m, c, nq);
    const bool tile256 = c.i8 && m->i8_tile != 0 && m->dk8 == 2 * kRing && pairs >= 2;
    const int share_cap = tile256 ? 2 * kShareMax : c.streamed ? kShareStreamed : kShareMax;
    // (a super-batch of at most 16 / 32 queries: one / two query blocks of the tile are live -- the fp16 pass multiplies against those only;
    // whole, even numbers of the form's units per row: eight pieces streamed, sixteen resident)
    const bool njb_shape = c.streamed ? !c.odd : (m->dk16 % (4 * kRing)) == 0;
    const int njb = (!c.i8 && k == 1 && adaptive && !m->dbg_skip && njb_shape) ? (nq <= 16 ? 1 : nq <= 32 ? 2 : 8) : 8;
    const int mode = adaptive ? (k > 1 ? 4 : 3) : 1;
    // algorithmic bytes of ONE launch (what fir_profile_read's event pairs bracket): the fragments once for the pairs that
    // read them together, every pair's query tile and keys
    auto launch_bytes = [&](int P) { return (double)((n + 31) / 32) * op.dk * 1024.0 + P * (4.0 * op.dk * 1024.0 + 128.0 * 8.0); };
    int nlaunch = 0, p_first = 1, rc = FIR_OK;
    for (int p0 = 0; p0 < pairs; ++nlaunch) {
        const int P = launch_pairs_(pairs - p0, share_cap);
        if (p0 == 0) p_first = P;
        const int nt = P <= 1 ? 1 : 0;                           // read once per launch: non-temporal
        const bool tile = tile256 && P >= 2;
        const fir_x_fn fn = pick_x({mode, c.streamed, c.odd, njb, c.i8, tile, k > 1 ? 0 : m->dbg_skip});
        if ((rc = fir_gallery_profile_begin_(m->g, c.st))) return rc;
        if (adaptive)
            gemm_launch_x_(fn, dim3(c.grid, 1), c.st, op, s, p0, P, n, n, 1, kBelowAwin,
                           {true, nt | m->adapt_dbg, s.aT, k > 1 ? 8 : 1, k > 1 ? k : 0, tile ? 2 : 1});
        else
            gemm_launch_x_(fn, dim3(c.grid, 1), c.st, op, s, p0, P, n, n, 1, kBelowTau, {false, nt, nullptr, 0, 0});
        if ((rc = fir_gallery_profile_end_(m->g, c.st, launch_bytes(P)))) return rc;
        p0 += P;
    }
    const fir_x_entry& ran = find_x({mode, c.streamed, c.odd, njb, c.i8, tile256});
    const char* ran_name = ran.name;
    if (c.i8_went_back) {
        if (sb == 0) m->i8_note = std::string(ran.name) + " (int8 nomination off for this gallery: " + m->i8_off_why + ")";
        ran_name = m->i8_note.c_str();
    }
    fir_gallery_note_dispatch_(m->g, (const void*)ran.fn, ran_name, sb == 0, c.grid, nlaunch, kGemmBlock, kHalfLds, 128 * p_first, launch_bytes(p_first),
                               2.0 * (double)n * c.d * 128.0 * p_first);
    if (adaptive)
        hipLaunchKernelGGL(k_gemm_adapt_final, dim3((pairs * 2 * kQT + 255) / 256), dim3(256), 0, c.st, s.aT, s.qnorm, s.tau, pairs * 2 * kQT, nq, k > 1 ? k : 0);
    return FIR_OK;
}

// The f32 / bf16-split full passes of one super-batch on `st`: every row below tau is appended
static void gemm_pass_f32_bf16_(fir_gemm* m, const GemmCall& c, int sb) {
    const int b = sb & 1, np = (c.sb_queries(sb) + kQT - 1) / kQT, grid = c.grid, sample_rows = m->sample_rows;
    GemmScratch& s = m->set[b];
    const int64_t n = c.n;
    if (m->precision == FIR_GEMM_F32) {
        hipLaunchKernelGGL(k_gemm_proxy<1>, dim3(grid, np), dim3(kGemmBlock), c.lds, c.st, m->gm, m->gnorm, s.qbf.as<float4>(), n, (int64_t)0, n, m->dq8,
                           s.tau, s.lists, s.counts, m->sample, sample_rows);
        fir_gallery_note_dispatch_(m->g, (const void*)k_gemm_proxy<1>, "fir::k_gemm_proxy<1>", sb == 0, grid, np, kGemmBlock, c.lds, 64,
                                   np * ((double)((n + 31) / 32) * m->dq8 * 1024.0), 2.0 * (double)n * c.d * 64.0 * np);
        return;
    }
    // pairs of passes share one read of the gallery (128 queries per wave); an odd last pass goes alone
    const int pairs = np / 2;
    if (pairs > 0)
        hipLaunchKernelGGL(k_gemm_proxy_bf16_wide, dim3(grid, pairs), dim3(kGemmBlock), kWideLds, c.st, m->gb, m->gnorm, s.qbf, n, m->dk16,
                           s.tau, s.lists, s.counts);
    if (np > 2 * pairs) {
        const size_t p0 = (size_t)2 * pairs;
        hipLaunchKernelGGL(k_gemm_proxy_bf16<1>, dim3(grid, np - 2 * pairs), dim3(kGemmBlock), c.lds, c.st, m->gb, m->gnorm,
                           s.qbf + p0 * (kQT / 32) * m->dk16 * 128, n, (int64_t)0, n, m->dk16, s.tau + p0 * kQT,
                           s.lists + p0 * kQT * kListCap, s.counts + p0 * kQT, m->sample + p0 * kQT * sample_rows, sample_rows);
    }
    fir_gallery_note_dispatch_(m->g, (const void*)k_gemm_proxy_bf16_wide, pairs > 0 ? "fir::k_gemm_proxy_bf16_wide" : "fir::k_gemm_proxy_bf16<1>", sb == 0,
                               grid, pairs > 0 ? pairs : np, kGemmBlock, pairs > 0 ? (size_t)kWideLds : c.lds, pairs > 0 ? 128 : 64,
                               (pairs + (np - 2 * pairs)) * ((double)((n + 31) / 32) * m->dk16 * 2048.0), 2.0 * (double)n * c.d * 64.0 * np);
}

// exact re-rank + certificate of super-batch sb on `rs`; uncertified queries go on the call's list. A launch the runtime refuses is the
// call's error: the flags and keys of this super-batch would otherwise be whatever an earlier call left.
static int gemm_rerank_(fir_gemm* m, const GemmCall& c, int sb, hipStream_t rs) {
    const int b = sb & 1, q0 = sb * c.sbq, nq = c.sb_queries(sb), k = c.s.k;
    GemmScratch& s = m->set[b];
    const FirSearch o = c.s.at(q0);         // the super-batch's slots of the call's outputs
    if (c.s.kind == fir::kSearchClasses)
        hipLaunchKernelGGL(k_gemm_rerank_classes, dim3(nq), dim3(64), gemm_rerank_lds_(m), rs, s.lists, s.counts, s.tau, m->gal4, c.sb_first(sb), s.qnorm, m->gmax,
                           m->v.cls, o.num_classes, c.n, c.d, m->dp4, m->v.row_offset, c.e_rel, m->rerank_group, k, (unsigned long long*)o.keys, o.classes, m->ok + q0, c.qs, m->rowmajor);
    else if (c.s.is_radius())
        hipLaunchKernelGGL(k_gemm_rerank_radius, dim3(nq), dim3(64), gemm_rerank_lds_(m), rs, s.lists, s.counts, s.tau, o.radius, m->gal4, c.sb_first(sb), s.qnorm,
                           m->gmax, c.n, c.d, m->dp4, m->v.row_offset, c.e_rel, m->rerank_group, k, (unsigned long long*)o.keys, o.count, m->ok + q0, c.qs, m->rowmajor);
    else if (c.s.kind == fir::kSearchSelect)
        hipLaunchKernelGGL(k_gemm_rerank_knn, dim3(nq), dim3(64), gemm_rerank_lds_(m), rs, s.lists, s.counts, s.tau, m->gal4, c.sb_first(sb), s.qnorm, m->gmax, c.n,
                           c.d, m->dp4, m->v.row_offset, c.e_rel, m->rerank_group, k, (unsigned long long*)o.keys, m->ok + q0, c.qs, m->rowmajor);
    else
        gemm_launch_rerank_(m, rs, nq, gemm_slot_(m, s, c.i8), c.sb_first(sb), c.e_rel, k, o.keys, m->ok + q0, {m->fb_state, m->fb_list, m->fb_tau2, q0, nullptr, 0});
    FIR_HIP(hipGetLastError());
    return FIR_OK;
}

#ifdef FIR_AUDIT
// audit builds: what FIR_GEMM_DUMP_PHASES / FIR_GEMM_DEBUG_COUNTS ask for about the call's last super-batch (synchronises)
static int gemm_audit_report_(fir_gemm* m, const GemmCall& c) {
    const int last = c.nsb - 1, b = last & 1;
    GemmScratch& s = m->set[b];
    if (!m->dump_phases.empty()) {                     // with FIR_GEMM_DBG_SKIP=256: the load-burst timestamps of the first pair
        FIR_HIP(hipStreamSynchronize(c.st));
        std::vector<unsigned long long> h(8 * 256);
        FIR_HIP(hipMemcpy(h.data(), s.lists + (size_t)(2 * kQT - 1) * kListCap + 2048, h.size() * 8, hipMemcpyDeviceToHost));
        if (FILE* f = std::fopen(m->dump_phases.c_str(), "w")) {
            for (int w = 0; w < 8; ++w)
                for (int u = 0; u < 240; ++u) std::fprintf(f, "%d %d %llu %llu\n", w, u, h[(size_t)w * 256 + u] >> 20, h[(size_t)w * 256 + u] & 0xFFFFFull);
            // the end of every wave's walk: units walked, s_memtime at the kernel's entry, behind the row loop, behind the workgroup's flush
            for (int w = 0; w < 8; ++w)
                std::fprintf(f, "# end %d %llu %llu %llu %llu\n", w, h[(size_t)w * 256 + 240], h[(size_t)w * 256 + 241], h[(size_t)w * 256 + 242], h[(size_t)w * 256 + 243]);
            std::fclose(f);
        }
    }
    if (m->debug_counts) {                             // appended rows per query
        FIR_HIP(hipStreamSynchronize(c.st));
        const int nql = c.sb_queries(last);
        std::vector<int> hc((size_t)nql), h_ok((size_t)nql);
        FIR_HIP(hipMemcpy(hc.data(), s.counts, (size_t)nql * sizeof(int), hipMemcpyDeviceToHost));
        FIR_HIP(hipMemcpy(h_ok.data(), m->ok + (size_t)last * c.sbq, (size_t)nql * sizeof(int), hipMemcpyDeviceToHost));
        long long sum = 0;
        int mx = 0, bad = 0, over = 0;
        for (int v : hc) { sum += v; mx = std::max(mx, v); over += v > kListCap ? 1 : 0; }
        for (int v : h_ok) bad += v ? 0 : 1;
        std::vector<float> ht((size_t)nql);
        FIR_HIP(hipMemcpy(ht.data(), s.tau, (size_t)nql * sizeof(float), hipMemcpyDeviceToHost));
        double ts = 0;
        int ninf = 0;
        for (float v : ht) { if (v < 1e30f) ts += v; else ++ninf; }
        float ms[3] = {0.f, 0.f, 0.f};                 // (serial preparation: the three phases follow one another on the device)
        if (c.serial_prep && m->phase_ev[3])
            for (int i = 0; i < 3; ++i) (void)hipEventElapsedTime(&ms[i], m->phase_ev[i], m->phase_ev[i + 1]);
        std::fprintf(stderr, "fir_gemm: appended rows per query (last super-batch of %d): mean %.1f, max %d; tau: mean %.6f, %d not finite; %d uncertified; "
                     "%d lists overflowed; preparation %.3f ms, full passes %.3f ms, re-rank %.3f ms\n", nql,
                     (double)sum / nql, mx, ts / std::max(1, nql - ninf), ninf, bad, over, ms[0], ms[1], ms[2]);
    }
    return FIR_OK;
}
#endif

// The uncertified queries of a call of any kind but kSearchRows (which has gemm_finish_): the call's one synchronisation of `st`, then the kind's
// exact form for every run of consecutive uncertified queries, straight into that run's output slots (no second-chance rounds)
static int gemm_finish_runs_(fir_gemm* m, const GemmCall& c) {
    std::vector<int> h_ok((size_t)c.qb);
    FIR_HIP(hipMemcpyAsync(h_ok.data(), m->ok, (size_t)c.qb * sizeof(int), hipMemcpyDeviceToHost, c.st));
    FIR_HIP(hipStreamSynchronize(c.st));
    int uncertified = 0;
    for (int q0 = 0; q0 < c.qb;) {
        int q1 = q0;
        while (q1 < c.qb && !h_ok[q1]) ++q1;
        if (q1 == q0) { ++q0; continue; }
        const int rc = kGemmKinds[c.s.kind].exact(m, c, c.d_queries + (size_t)q0 * c.qs, q1 - q0, c.s.at(q0));
        if (rc) return rc;
        uncertified += q1 - q0;
        q0 = q1;
    }
    if (uncertified) hipLaunchKernelGGL(k_gemm_fb_count, dim3(1), dim3(1), 0, c.st, m->fb_state, uncertified);
    FIR_HIP(hipGetLastError());
    return FIR_OK;
}

// One search of any kind (s: fir_search_request.h) through the matrix cores. The entry points below have made their own checks,
// in their own order; the ones here are what fir_gemm_search_top1 / _topk_keys_dev and fir_gemm_search_staged_ report.
static int gemm_search(fir_gemm* m, const float* d_queries, int32_t qb, const FirSearch& s, void* stream, const float* h_queries = nullptr) {
    const GemmKind& kind = kGemmKinds[s.kind];
    if (!m || !s.outputs_ok() || (qb > 0 && !d_queries)) return fir_fail_(FIR_ERR_ARG, "NULL argument");
    if (qb < 0) return fir_fail_(FIR_ERR_ARG, "qb < 0");
    if (s.k < kind.k_min || s.k > kind.k_max) return fir_fail_(FIR_ERR_ARG, "k=%d outside [1,%d]", s.k, kind.k_max);
    if (qb == 0) return FIR_OK;
    if (const int rcg = fir_gallery_stale_(m->g, m->v.generation, "fir_gemm")) return rcg;      // (m->v.n and the tiled buffer are the gallery's of then)
    FIR_HIP(hipSetDevice(m->v.device));
    hipStream_t st = stream ? (hipStream_t)stream : m->v.stream;
    FirCallOrder order(m->g, st);   // this state's scratch, and the gallery's, is shared with every other call on the gallery
    if (order.rc) return order.rc;
    GemmCall c;
    c.d_queries = d_queries; c.h_queries = h_queries; c.qb = qb; c.s = s; c.st = st;
    if (const char* w = s.kind == fir::kSearchSelect ? fir_knob_("FIR_GEMM_KNN_SAMPLE_DIV") : nullptr) c.knn_div = std::max(1, std::atoi(w));
    c.d = m->feat; c.qs = m->v.d; c.n = m->v.n; c.grid = m->v.cus;
    if (c.n == 0 && h_queries) FIR_HIP(hipMemcpyAsync((void*)d_queries, h_queries, (size_t)qb * c.qs * sizeof(float), hipMemcpyHostToDevice, st));
    if (c.n == 0) return kind.exact(m, c, d_queries, qb, s);        // every slot unused / FIR_KEY_NONE, every count 0
    c.streamed = gemm_streamed_(m);
    c.odd = gemm_odd_(m);
    {
        const int rc8 = gemm_wants_i8_(m, c, &c.i8);
        if (rc8) return rc8;
    }
    if (c.i8) { c.streamed = false; c.odd = gemm_odd8_(m); }
    c.lds = m->precision == FIR_GEMM_F32 ? (size_t)(kQT / 32) * std::min(m->dq8, kSlab8) * 64 * sizeof(float4)
                                         : (size_t)(kQT / 32) * std::min(m->dk16, kSlab16) * 128 * sizeof(uint4);
    c.e_rel = gemm_e_rel_(m, c.i8);
    // Large super-batches amortise the boundaries between full passes (where the small kernels run: they cannot share a CU with a
    // full-pass workgroup), but a call needs a few super-batches for its preparation / re-rank to overlap anything: a quarter of the
    // call, in whole 1 024-query launches.
    // Galleries whose 1 024-query launch is short (n d <= 1.5e8: under ~0.25 ms) take the whole call (up to kPasses passes) as ONE
    // super-batch: between two super-batches the next one's preparation queues behind the previous one's re-rank, which runs squeezed
    // between the full pass's workgroups (100 000 x 512, 4 096 queries: ~65 us of bubble per boundary and a re-rank four times
    // slower than alone, for 110 us launches -- profiles/r03_small_call_timeline.txt)
    const bool short_launches = (double)c.n * (double)c.d <= 1.5e8;
    c.sbq = std::min(kPasses * kQT, std::max(1024, ((short_launches ? qb : qb / 4) + 1023) / 1024 * 1024));
    c.nsb = (qb + c.sbq - 1) / c.sbq;
    c.serial_prep = !h_queries;
    c.one_stream = c.nsb == 1 && c.serial_prep;
    int rc = gemm_reserve_(m, c);
    if (rc) return rc;
    // this call's two list lengths (the fp16 form clears them in the first super-batch's query preparation: one launch less per call)
    if (m->precision != FIR_GEMM_F16) FIR_HIP(hipMemsetAsync(m->fb_state, 0, 2 * sizeof(int), st));
    if (!c.one_stream) {
        FIR_HIP(hipEventRecord(m->queries_ready, st));
        FIR_HIP(hipStreamWaitEvent(m->side, m->queries_ready, 0));
    }
    // order on `side` when it prepares: prep(0) prep(1) rerank(0) prep(2) rerank(1) ...
    if ((rc = gemm_prep_(m, c, 0))) return rc;
    for (int sb = 0; sb < c.nsb; ++sb) {
        const int b = sb & 1;
        if (c.serial_prep) { if (sb >= 1 && (rc = gemm_prep_(m, c, sb))) return rc; }
        else if (sb + 1 < c.nsb && (rc = gemm_prep_(m, c, sb + 1))) return rc;
        FIR_HIP(hipStreamWaitEvent(st, m->prep_done[b], 0));
        if (m->precision == FIR_GEMM_F16) { if ((rc = gemm_pass_f16_(m, c, sb))) return rc; }
        else gemm_pass_f32_bf16_(m, c, sb);
        FIR_HIP(hipEventRecord(m->main_done[b], st));
        gemm_audit_mark_(m, 2, st);
        // on the side stream, the re-rank runs under the next super-batch's full passes
        hipStream_t rs = c.one_stream ? st : m->side;
        if (!c.one_stream) FIR_HIP(hipStreamWaitEvent(m->side, m->main_done[b], 0));
        if ((rc = gemm_rerank_(m, c, sb, rs))) return rc;
        gemm_audit_mark_(m, 3, rs);
        FIR_HIP(hipEventRecord(m->rerank_done[b], rs));
        m->passes += (c.sb_queries(sb) + kQT - 1) / kQT;
    }
    if (!c.one_stream) FIR_HIP(hipStreamWaitEvent(st, m->rerank_done[(c.nsb - 1) & 1], 0));   // join the side stream (it is in order: the last re-rank is the last thing on it)
    FIR_HIP(hipGetLastError());
    m->last_kind = 1; m->last_b = (c.nsb - 1) & 1; m->last_nq = c.sb_queries(c.nsb - 1); m->last_sc_rounds = 0; m->last_i8 = c.i8;
#ifdef FIR_AUDIT
    if ((rc = gemm_audit_report_(m, c))) return rc;
#endif
    if (s.kind != fir::kSearchRows) return gemm_finish_runs_(m, c);
    // uncertified queries: a second matrix-core pass with the tightest bound the first one can justify, then the exact device scan
    // (calls of at most 32 queries skip the second-chance rounds: the exact device scan reads the gallery once per eight queries, about what
    // one more matrix-core pass costs, and four launches fewer are 20 us of such a call)
    const int sc_rounds = m->precision == FIR_GEMM_F16 && qb > 32 ? std::min(kScRounds, (qb + kScQueries - 1) / kScQueries) : 0;
    m->last_sc_rounds = sc_rounds;
    if ((rc = gemm_finish_(m, d_queries, c.s.k, s.keys, st, c.e_rel, sc_rounds, c.streamed, c.i8))) return rc;
    if (c.i8 && m->i8_mode < 0 && !m->i8_pending) {
        // (the automatic rule's way back, gemm_wants_i8_: how many queries of this call needed a second pass, copied behind the call)
        FIR_HIP(hipMemcpyAsync(m->i8_pin, m->fb_state, sizeof(int), hipMemcpyDeviceToHost, st));
        FIR_HIP(hipEventRecord(m->i8_ev, st));
        m->i8_pending = true;
        m->i8_pending_qb = qb;
    }
    return FIR_OK;
}

extern "C" {

void fir_gemm_set_int8_(fir_gemm* m, int32_t mode) { if (m) m->i8_mode = mode > 0 ? 1 : mode < 0 ? -1 : 0; }
void fir_gemm_set_int8_tile_(fir_gemm* m, int32_t mode) { if (m) m->i8_tile = mode > 0 ? 1 : mode < 0 ? -1 : 0; }

int fir_gemm_search_top1_keys_dev(fir_gemm* m, const float* d_queries, int32_t qb, uint64_t* d_keys, void* stream) {
    return gemm_search(m, d_queries, qb, FirSearch::rows(1, d_keys), stream);
}

int fir_gemm_search_topk_keys_dev(fir_gemm* m, const float* d_queries, int32_t qb, int32_t k, uint64_t* d_keys, void* stream) {
    return gemm_search(m, d_queries, qb, FirSearch::rows(k, d_keys), stream);
}

int fir_gemm_search_top_classes_keys_dev(fir_gemm* m, const float* d_queries, int32_t qb, int32_t num_classes, int32_t k, uint64_t* d_keys,
                                         int32_t* d_classes, void* stream) {
    if (!m || (qb > 0 && !d_queries)) return fir_fail_(FIR_ERR_ARG, "NULL argument");
    if (m->precision != FIR_GEMM_F16 || m->f64) return fir_fail_(FIR_ERR_ARG, "the distinct-class form needs a FIR_GEMM_F16 state");
    if (qb < 0) return fir_fail_(FIR_ERR_ARG, "qb < 0");
    if (k < 1 || k > 32) return fir_fail_(FIR_ERR_ARG, "k=%d outside [1,32]", k);
    if (num_classes < 1 || num_classes > (1 << 24)) return fir_fail_(FIR_ERR_ARG, "num_classes=%d outside [1,%d]", num_classes, 1 << 24);
    if (!m->v.cls && m->v.n > 0) return fir_fail_(FIR_ERR_STATE, "gallery was created without class labels");
    if (qb > 0 && !d_keys && !d_classes) return fir_fail_(FIR_ERR_ARG, "d_keys and d_classes are both NULL");
    if (qb == 0) return FIR_OK;
    return gemm_search(m, d_queries, qb, FirSearch::distinct(num_classes, k, d_keys, d_classes), stream);
}

// K <= kTopKMax: the top-1 / top-K forms as they are (they do not synchronise); beyond it the sample flow of fir_gemm_knn.h, which
// synchronises `stream` once
int fir_gemm_search_knn_keys_dev(fir_gemm* m, const float* d_queries, int32_t qb, int32_t k, uint64_t* d_keys, void* stream) {
    if (!m || !d_keys || (qb > 0 && !d_queries)) return fir_fail_(FIR_ERR_ARG, "NULL argument");
    if (qb < 0) return fir_fail_(FIR_ERR_ARG, "qb < 0");
    if (k < 1 || k > FIR_GEMM_KNN_MAX) return fir_fail_(FIR_ERR_ARG, "k=%d outside [1,%d]", k, FIR_GEMM_KNN_MAX);
    if (k <= kTopKMax) return gemm_search(m, d_queries, qb, FirSearch::rows(k, d_keys), stream);
    if (m->precision != FIR_GEMM_F16 || m->f64) return fir_fail_(FIR_ERR_ARG, "the K > %d nearest-rows form needs a FIR_GEMM_F16 state", kTopKMax);
    if (qb == 0) return FIR_OK;
    return gemm_search(m, d_queries, qb, FirSearch::select(k, d_keys), stream);
}

// Every row within radius[q] (fir_amd.h): the flow of fir_gemm_knn.h without its sample -- tau from the radius, the append pass,
// k_gemm_rerank_radius; synchronises `stream` once, then the store + count + select form answers what was not certified.
int fir_gemm_search_radius_keys_dev(fir_gemm* m, const float* d_queries, int32_t qb, const float* d_radius, int32_t max_results, int32_t* d_count,
                                    uint64_t* d_keys, void* stream) {
    const bool in_range = max_results >= 0 && max_results <= FIR_GEMM_KNN_MAX;
    if (!m || !d_count || (qb > 0 && (!d_queries || !d_radius)) || (in_range && (max_results == 0 ? d_keys != nullptr : d_keys == nullptr)))
        return fir_fail_(FIR_ERR_ARG, "NULL argument");
    if (qb < 0) return fir_fail_(FIR_ERR_ARG, "qb < 0");
    if (!in_range) return fir_fail_(FIR_ERR_ARG, "max_results=%d outside [0,%d]", max_results, FIR_GEMM_KNN_MAX);
    if (m->precision != FIR_GEMM_F16 || m->f64) return fir_fail_(FIR_ERR_ARG, "the radius form needs a FIR_GEMM_F16 state");
    if (qb == 0) return FIR_OK;
    return gemm_search(m, d_queries, qb, FirSearch::within(d_radius, max_results, d_count, d_keys), stream);
}

// 1..8 queries against a gallery too large for the caches: one pass over the fp16 copy (k_gemm_scan_f16x), the rows within one
// window of the smallest proxy of ALL rows, exact re-rank, certificate; everything on `stream`, one synchronisation.
int fir_gemm_search_few_keys_dev(fir_gemm* m, const float* d_queries, int32_t qb, uint64_t* d_keys, void* stream) {
    if (!m || !d_keys || !d_queries) return fir_fail_(FIR_ERR_ARG, "NULL argument");
    if (qb < 1 || qb > 8) return fir_fail_(FIR_ERR_ARG, "qb=%d outside [1,8]", qb);
    if (m->precision != FIR_GEMM_F16) return fir_fail_(FIR_ERR_ARG, "the few-query form needs the fp16 copy");
    if (const int rcg = fir_gallery_stale_(m->g, m->v.generation, "fir_gemm")) return rcg;
    FIR_HIP(hipSetDevice(m->v.device));
    hipStream_t st = stream ? (hipStream_t)stream : m->v.stream;
    FirCallOrder order(m->g, st);
    if (order.rc) return order.rc;
    const int d = m->feat, qs = m->v.d;
    const int64_t n = m->v.n;
    if (n == 0) return fir_search_top1_exact_keys_dev_(m->g, d_queries, qb, 0, d, d_keys, st);
    const int nqt = qb <= 1 ? 1 : qb <= 2 ? 2 : qb <= 4 ? 4 : 8;
    if (nqt > m->proxies_nq) {
        m->proxies_nq = 0;
        m->proxies.release();
        const int rcp = FIR_RESERVE(m->proxies, (size_t)nqt * n * sizeof(float));     // (FIR_ERR_NOMEM: the caller takes the exact scan)
        if (rcp) return rcp;
        m->proxies_nq = nqt;
    }
    {
        int rcr = gemm_grow_lists_(m, 2, 2 * kQT, {});          // (no wait of its own: the first growth of a state, or none)
        if (rcr || (rcr = gemm_fb_reserve_(m, qb))) return rcr;
    }
    const float e_rel = gemm_e_rel_(m, false);
    const int b = 0;
    GemmScratch& s = m->set[b];
    hipLaunchKernelGGL(k_gemm_qprep_f16, dim3(2 * kQT), dim3(64), 0, st, d_queries, qb, d, m->gallery_exp, s.qnorm, s.qmul, s.qinv, qs, s.counts,
                       (float*)nullptr, (unsigned int*)nullptr, (const float*)nullptr, 0.f, 0, s.smin, m->fb_state);
    hipLaunchKernelGGL(k_gemm_pack_queries_f16x, dim3((4 * m->dk16 * 64 + 255) / 256, 1), dim3(256), 0, st, d_queries, qb, d, m->dk16, s.qmul, s.qbf, qs);
    const dim3 grid((unsigned)std::min<int64_t>((int64_t)m->v.cus * 8, ((n + 31) / 32 + 3) / 4));
    const size_t lds = (size_t)m->dk16 * 2 * nqt * sizeof(uint4);
    typedef void (*scan_fn)(const uint4*, const float*, const uint4*, const float*, int64_t, int, float*, unsigned int*);
    const scan_fn scan = nqt == 1 ? k_gemm_scan_f16x<1> : nqt == 2 ? k_gemm_scan_f16x<2> : nqt == 4 ? k_gemm_scan_f16x<4> : k_gemm_scan_f16x<8>;
    const double bytes = (double)((n + 31) / 32) * m->dk16 * 1024.0 + (double)nqt * n * 4.0;
    {
        int rcp = fir_gallery_profile_begin_(m->g, st);              // (no-ops unless profiling is on: a profiled run takes the same path as an unprofiled one)
        if (rcp) return rcp;
        hipLaunchKernelGGL(scan, grid, dim3(256), lds, st, m->gh, m->gnorm, s.qbf, s.qinv, n, m->dk16, m->proxies, s.smin);
        if ((rcp = fir_gallery_profile_end_(m->g, st, bytes))) return rcp;
    }
    fir_gallery_note_dispatch_(m->g, (const void*)scan, "fir::k_gemm_scan_f16x", 1, (int)grid.x, 1, 256, lds, nqt, bytes, 2.0 * (double)n * d * nqt);
    hipLaunchKernelGGL(k_gemm_tau_min, dim3(1), dim3(256), 0, st, s.smin, s.tau, 2 * kQT, qb, s.qnorm, m->gmax, e_rel);
    hipLaunchKernelGGL(k_gemm_select, dim3((unsigned)std::min<int64_t>(1024, (n + 255) / 256), qb), dim3(256), 0, st, m->proxies, n, s.tau, s.lists, s.counts);
    gemm_launch_rerank_(m, st, qb, gemm_slot_(m, s, false), d_queries, e_rel, 1, d_keys, m->ok,
                        {m->fb_state, m->fb_list, m->fb_tau2, 0, nullptr, 0});
    FIR_HIP(hipGetLastError());
    m->passes += 1;
    m->last_kind = 2; m->last_b = b; m->last_nq = qb; m->last_sc_rounds = 0; m->last_i8 = false;
    // (the bound of this form already is the smallest proxy of ALL rows + one window: a second pass could not do better; what is
    // not certified -- NaN operands, thousands of ties -- goes to the exact device scan, in stream order)
    return gemm_finish_(m, d_queries, 1, d_keys, st, e_rel, 0, gemm_streamed_(m));
}

// Read-only diagnostics for the tests of the nomination pass (not part of the public ABI; declared in fir_internal.h): waits for the
// device's work, then copies out what the re-rank of the most recent call's LAST super-batch was handed for query slots
// [q0, q0 + nq) of that super-batch -- counts[i], tau[i] (after k_gemm_adapt_final where the bound is found on the way), qnorm[i] and
// the first min(count, kListCap, max_entries) list entries of each slot (orderable proxy bits << 32 | row) at lists[i * max_entries ..].
// which = 1: the same for the scratch of the call's last second-chance round that had queries (fir_gemm_fb.h); qmap[i] = the query of
// the call slot q0 + i stands for, *live = the slots of that round that hold a query (0: no round ran). which = 0: qmap[i] = q0 + i,
// *live = the super-batch's queries. proxies (the few-query scan only): row i = all n proxies of query q0 + i. *gmax = the largest
// squared row norm as the windows use it. Any output pointer may be NULL. It changes no scratch and launches nothing.
// A float64 state (fir_gemm_f64.h, through fir_cls_knn_state_) is read the same way with which = 0: fir_gemm_knn_f64_ keeps the record.
int fir_gemm_nominations_(fir_gemm* m, int32_t which, int32_t q0, int32_t nq, int32_t max_entries, int32_t* counts, float* tau, float* qnorm,
                          uint64_t* lists, float* proxies, float* gmax, int32_t* qmap, int32_t* live) {
    if (!m || (m->f64 && which != 0)) return fir_fail_(FIR_ERR_ARG, "not a fir_gemm nomination state");     // (a float64 state has no second chance)
    if (which < 0 || which > 1 || q0 < 0 || nq < 0 || max_entries < 0 || max_entries > kListCap) return fir_fail_(FIR_ERR_ARG, "bad range");
    if (!m->last_kind) return fir_fail_(FIR_ERR_STATE, "no call has run on this state yet");
    FIR_HIP(hipSetDevice(m->v.device));
    FIR_HIP(hipDeviceSynchronize());
    const GemmScratch& s = which ? m->sc : m->set[m->last_b];
    int have = m->last_nq, off = 0;
    if (which == 1) {
        int cnt = 0;
        FIR_HIP(hipMemcpy(&cnt, m->fb_state, sizeof(int), hipMemcpyDeviceToHost));
        const int rounds = std::min(m->last_sc_rounds, (cnt + kScQueries - 1) / kScQueries);
        if (m->last_kind != 1 || rounds <= 0 || !m->sc.lists) have = 0;
        else { off = (rounds - 1) * kScQueries; have = std::min(kScQueries, cnt - off); }
    }
    if (live) *live = have;
    if (gmax) FIR_HIP(hipMemcpy(gmax, m->last_i8 ? m->i8_par + 2 : m->gmax, sizeof(float), hipMemcpyDeviceToHost));
    if (nq == 0) return FIR_OK;
    if (q0 + nq > have) return fir_fail_(FIR_ERR_ARG, "slots [%d,%d) of %d", q0, q0 + nq, have);
    if (counts) FIR_HIP(hipMemcpy(counts, s.counts + q0, (size_t)nq * sizeof(int), hipMemcpyDeviceToHost));
    if (tau) FIR_HIP(hipMemcpy(tau, s.tau + q0, (size_t)nq * sizeof(float), hipMemcpyDeviceToHost));
    if (qnorm) FIR_HIP(hipMemcpy(qnorm, s.qnorm + q0, (size_t)nq * sizeof(float), hipMemcpyDeviceToHost));
    if (lists && max_entries > 0)
        FIR_HIP(hipMemcpy2D(lists, (size_t)max_entries * 8, s.lists + (size_t)q0 * kListCap, (size_t)kListCap * 8, (size_t)max_entries * 8, (size_t)nq,
                            hipMemcpyDeviceToHost));
    if (qmap) {
        if (which) FIR_HIP(hipMemcpy(qmap, m->fb_list + off + q0, (size_t)nq * sizeof(int), hipMemcpyDeviceToHost));
        else for (int i = 0; i < nq; ++i) qmap[i] = q0 + i;
    }
    if (proxies) {
        if (m->last_kind != 2 || !m->proxies) return fir_fail_(FIR_ERR_STATE, "the most recent call was not the few-query scan");
        FIR_HIP(hipMemcpy(proxies, m->proxies + (size_t)q0 * m->v.n, (size_t)nq * m->v.n * sizeof(float), hipMemcpyDeviceToHost));
    }
    return FIR_OK;
}

// Host-pointer form for fir_search_top1 / fir_search_topk: h_queries -> d_stage (qb rows of the gallery's length) super-batch by
// super-batch, under the full passes of the one before; keys as the device-pointer forms.
int fir_gemm_search_staged_(fir_gemm* m, const float* h_queries, float* d_stage, int32_t qb, int32_t k, uint64_t* d_keys, void* stream) {
    if (!h_queries || !d_stage) return fir_fail_(FIR_ERR_ARG, "NULL argument");
    return gemm_search(m, d_stage, qb, FirSearch::rows(k, d_keys), stream, h_queries);
}

}  // extern "C"

#include "fir_gemm_f64.h"
