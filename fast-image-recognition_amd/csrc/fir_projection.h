// fir_projection.h -- linear projection / PCA on the device (include/fir_amd.h has the contract): the feature statistics and the
// scatter matrix of the rows a mask selects, and a p x d linear map applied to every row of a handle into a new handle.
// Included at the end of fir_capi.hip (one translation unit: -ffp-contract=off holds, struct fir_gallery, gallery_alloc, created_dev
// and GalleryCall are in scope).
//
// Row segments. The tiles of a handle are cut into segments of pj_plan(tiles, most).seg_tiles whole tiles -- at least kPjSegMinTiles,
// a function of n and d alone. Every (segment, work item) writes one partial to scratch and a second small kernel adds the partials in
// ascending segment order: no floating-point atomics, the same bytes from run to run.
//
// The matrix-core instruction. v_mfma_f64_16x16x4_f64 wants A[row = lane & 15][k = lane >> 4] and B[k = lane >> 4][col = lane & 15],
// one double per lane; C/D: col = lane & 15, row = (lane >> 4) + 4 * reg (fir_cls_pnn_mfma.h).
//   scatter:    k = the ROWS of the gallery. A workgroup owns one pair of 64-feature blocks (a <= b) and one row segment; per half tile
//               (32 rows) it loads the two slabs coalesced, widens, subtracts the centre, zeroes rows that are masked out or at or past n
//               AFTER centring (a centred padding row is -c, not 0), writes float64 operands to LDS and runs 8 k-steps; wave w keeps the
//               32 x 32 quarter (w >> 1, w & 1) of the 64 x 64 block in 16 accumulator doubles per lane for the whole segment.
//               LDS row stride 80 doubles: the two 16-lane groups of a half wave read rows k and k + 1, 640 bytes = 32 banks apart.
//   projection: k = the features. The basis block is A, the gallery tile B. A's row i holds output feature 4 * (i & 3) + (i >> 2) of the
//               block, so D's rows (lane >> 4) + 4 * reg are the four CONSECUTIVE features 4 * (lane >> 4) + reg: one float4 store into
//               the destination tile per lane and 16 x 16 result block. Lane (lr, lk) loads the float4 of chunk 4 s + lk of row
//               16 rb + lr; its components feed four MFMAs whose k-sets are {4 (4 s + kk) + comp, kk = 0..3} (the pairing of
//               fir_cls_pnn_mfma.h). The basis is kept in exactly that order: wp[(block * nss + s) * 64 + lane] is the lane's four A
//               values of super-step s, one 32-byte load, read from global memory / L2 per step (256 x 1536 doubles do not fit LDS).
//               Every output element is one accumulator chain over s = 0 .. nss - 1, comp = 0 .. 3, whatever path the row came by.
namespace {

typedef double pj_double4 __attribute__((ext_vector_type(4)));
constexpr int64_t kPjSegMinTiles = 8;                          // rows per segment >= 512
constexpr int64_t kPjStatSegs = 256;                           // the column sums: at most this many segments
constexpr size_t kPjScatterPartials = (size_t)256 << 20;       // bytes the scatter's partials may take
constexpr int64_t kPjScatterWorkgroups = 2048;                 // ... and the workgroups it aims for (pairs x segments)
constexpr int kPjLdsStride = 80;                               // doubles per LDS row of the scatter's operands (64 + 16)
constexpr int kPjMaxDim = 4096;                                // scatter: d; projection: p
constexpr size_t kPjApplyBytes = (size_t)64 << 20;             // tiled input + output of one slab of fir_projection_apply

struct PjPlan { int64_t seg_tiles, nseg; };
PjPlan pj_plan(int64_t tiles, int64_t most) {
    const int64_t seg = std::max(kPjSegMinTiles, (tiles + most - 1) / std::max<int64_t>(most, 1));
    return PjPlan{seg, (tiles + seg - 1) / seg};
}
int pj_pairs(int nb) { return nb * (nb + 1) / 2; }
PjPlan pj_scatter_plan(int64_t tiles, int nb) {
    const int64_t pairs = pj_pairs(nb);
    const int64_t fit = std::max<int64_t>(1, (int64_t)(kPjScatterPartials / ((size_t)pairs * 4096 * sizeof(double))));
    return pj_plan(tiles, std::min(fit, (kPjScatterWorkgroups + pairs - 1) / pairs));
}

// the mask word of tile t with the bits of rows at or past n cleared (mask NULL: every row); t < ceil(n / 64)
__device__ __forceinline__ uint64_t pj_tile_word(const uint64_t* __restrict__ mask, int64_t t, int64_t n) {
    uint64_t w = mask ? mask[t] : ~0ull;
    const int64_t left = n - t * kTileRows;
    if (left < 64) w &= (1ull << left) - 1ull;
    return w;
}
__device__ __forceinline__ float pj_comp(const float4& v, int j) { return j == 0 ? v.x : j == 1 ? v.y : j == 2 ? v.z : v.w; }

// part[seg][0..3][dk]: sum, sum of squares, min, max of the selected rows of segment blockIdx.x, per feature (dk = 4 dp4). One wave per
// (segment, chunk): lane r keeps the four features of row r of every tile in registers, one wave reduction at the end. The mask word
// of a tile is wave-uniform; a tile with an empty word is never read.
__global__ void __launch_bounds__(kBlock) k_pj_col_stats(const float4* __restrict__ gal4, int64_t n, int64_t tiles, int dp4, const uint64_t* __restrict__ mask,
                                                          int64_t seg_tiles, double* __restrict__ part) {
    const int lane = threadIdx.x & 63;
    const int c = blockIdx.y * (kBlock / 64) + (threadIdx.x >> 6);
    if (c >= dp4) return;                                               // wave-uniform; the kernel has no barrier
    const int64_t seg = blockIdx.x;
    const int64_t t0 = seg * seg_tiles, t1 = t0 + seg_tiles < tiles ? t0 + seg_tiles : tiles;
    double s[4] = {0.0, 0.0, 0.0, 0.0}, q[4] = {0.0, 0.0, 0.0, 0.0};
    float lo[4] = {FLT_MAX, FLT_MAX, FLT_MAX, FLT_MAX}, hi[4] = {-FLT_MAX, -FLT_MAX, -FLT_MAX, -FLT_MAX};
    for (int64_t t = t0; t < t1; ++t) {
        const uint64_t w = pj_tile_word(mask, t, n);
        if (w == 0ull) continue;
        const float4 g = gal4[((size_t)t * dp4 + c) * 64 + lane];
        if ((w >> lane) & 1ull) {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const float x = pj_comp(g, j);
                const double xd = (double)x;
                s[j] = s[j] + xd;
                q[j] = q[j] + xd * xd;                                  // (the square of an f32 is exact in double)
                if (x < lo[j]) lo[j] = x;
                if (x > hi[j]) hi[j] = x;
            }
        }
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            s[j] = s[j] + __shfl_xor(s[j], off, 64);
            q[j] = q[j] + __shfl_xor(q[j], off, 64);
            const float ol = __shfl_xor(lo[j], off, 64), oh = __shfl_xor(hi[j], off, 64);
            if (ol < lo[j]) lo[j] = ol;
            if (oh > hi[j]) hi[j] = oh;
        }
    }
    if (lane == 0) {
        const int dk = dp4 * 4;
        double* o = part + (size_t)seg * 4 * dk + c * 4;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            o[j] = s[j];
            o[dk + j] = q[j];
            o[2 * dk + j] = (double)lo[j];
            o[3 * dk + j] = (double)hi[j];
        }
    }
}
// out[0..3][dk] = the segments' partials folded in ascending order. One thread per feature.
__global__ void __launch_bounds__(kBlock) k_pj_col_fold(const double* __restrict__ part, int64_t nseg, int dk, double* __restrict__ out) {
    const int k = blockIdx.x * kBlock + threadIdx.x;
    if (k >= dk) return;
    double s = 0.0, q = 0.0, lo = (double)FLT_MAX, hi = -(double)FLT_MAX;
    for (int64_t seg = 0; seg < nseg; ++seg) {
        const double* p = part + (size_t)seg * 4 * dk + k;
        s = s + p[0];
        q = q + p[dk];
        if (p[2 * dk] < lo) lo = p[2 * dk];
        if (p[3 * dk] > hi) hi = p[3 * dk];
    }
    out[k] = s;
    out[dk + k] = q;
    out[2 * dk + k] = lo;
    out[3 * dk + k] = hi;
}

// blockIdx.x -> the pair (ba <= bb) of 64-feature blocks, row-major over the upper triangle
__device__ __forceinline__ void pj_pair(int pair, int nb, int& ba, int& bb) {
    ba = 0;
    while (pair >= nb - ba) { pair -= nb - ba; ++ba; }
    bb = ba + pair;
}
// part[(seg * pairs + pair) * 4096 + a * 64 + b] = sum over the selected rows of segment blockIdx.y of (x_a - c_a)(x_b - c_b), a / b inside
// the feature blocks of pair blockIdx.x. cen[nb * 64]: the centre, 0 for features at or past d.
__global__ void __launch_bounds__(kBlock) k_pj_scatter(const float4* __restrict__ gal4, int64_t n, int64_t tiles, int dp4, const uint64_t* __restrict__ mask,
                                                        const double* __restrict__ cen, int nb, int64_t seg_tiles, double* __restrict__ part) {
    __shared__ __attribute__((aligned(16))) double xs[2][32 * kPjLdsStride];
    int ba, bb;
    pj_pair((int)blockIdx.x, nb, ba, bb);
    const bool diag = ba == bb;
    const int tid = threadIdx.x, lane = tid & 63, lr = lane & 15, lk = lane >> 4, wv = tid >> 6;
    const int ar = (wv >> 1) * 32, bc = (wv & 1) * 32;
    const int r = tid & 31, cc = tid >> 5;                              // the loader's row of the half tile; its chunks cc and cc + 8 of a slab
    double ca[2][4], cb[2][4];
#pragma unroll
    for (int h = 0; h < 2; ++h)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            ca[h][j] = cen[ba * 64 + (cc + 8 * h) * 4 + j];
            cb[h][j] = cen[bb * 64 + (cc + 8 * h) * 4 + j];
        }
    pj_double4 acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) acc[i][j] = (pj_double4){0.0, 0.0, 0.0, 0.0};
    const double* xa = xs[0];
    const double* xb = diag ? xs[0] : xs[1];
    const float4 zero4 = make_float4(0.f, 0.f, 0.f, 0.f);
    const int64_t t0 = (int64_t)blockIdx.y * seg_tiles, t1 = t0 + seg_tiles < tiles ? t0 + seg_tiles : tiles;
    for (int64_t t = t0; t < t1; ++t) {
        const uint64_t w = pj_tile_word(mask, t, n);
        if (w == 0ull) continue;                                        // (uniform over the workgroup, like every branch around a barrier below)
        for (int half = 0; half < 2; ++half) {
            const uint32_t wh = (uint32_t)(w >> (32 * half));
            if (wh == 0u) continue;
            const bool on = (wh >> r) & 1u;
            const size_t at = (size_t)t * dp4 * 64 + half * 32 + r;
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                const int sc = cc + 8 * h;
                const int cha = ba * 16 + sc, chb = bb * 16 + sc;
                const float4 va = on && cha < dp4 ? gal4[at + (size_t)cha * 64] : zero4;
                double* da = &xs[0][r * kPjLdsStride + sc * 4];
#pragma unroll
                for (int j = 0; j < 4; ++j) da[j] = on ? (double)pj_comp(va, j) - ca[h][j] : 0.0;
                if (!diag) {
                    const float4 vb = on && chb < dp4 ? gal4[at + (size_t)chb * 64] : zero4;
                    double* db = &xs[1][r * kPjLdsStride + sc * 4];
#pragma unroll
                    for (int j = 0; j < 4; ++j) db[j] = on ? (double)pj_comp(vb, j) - cb[h][j] : 0.0;
                }
            }
            __syncthreads();
#pragma unroll
            for (int ks = 0; ks < 8; ++ks) {
                const int o = (ks * 4 + lk) * kPjLdsStride + lr;
                const double a0 = xa[o + ar], a1 = xa[o + ar + 16], b0 = xb[o + bc], b1 = xb[o + bc + 16];
                acc[0][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b0, acc[0][0], 0, 0, 0);
                acc[0][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b1, acc[0][1], 0, 0, 0);
                acc[1][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b0, acc[1][0], 0, 0, 0);
                acc[1][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b1, acc[1][1], 0, 0, 0);
            }
            __syncthreads();                                            // the next half tile overwrites the operands
        }
    }
    // D: col = lane & 15 -> feature b; row = (lane >> 4) + 4 * reg -> feature a
    double* o = part + ((size_t)blockIdx.y * gridDim.x + blockIdx.x) * 4096;
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int reg = 0; reg < 4; ++reg) o[(ar + 16 * i + lk + 4 * reg) * 64 + bc + 16 * j + lr] = acc[i][j][reg];
}
// S[a][b] = S[b][a] = the partials of (a, b) added in ascending segment order; in a diagonal block only a <= b is read. grid (pairs, 16).
__global__ void __launch_bounds__(kBlock) k_pj_scatter_fold(const double* __restrict__ part, int64_t nseg, int nb, int d, double* __restrict__ S) {
    int ba, bb;
    pj_pair((int)blockIdx.x, nb, ba, bb);
    const int e = blockIdx.y * kBlock + threadIdx.x;
    const int ai = e >> 6, bj = e & 63;
    const int a = ba * 64 + ai, b = bb * 64 + bj;
    if (a >= d || b >= d || (ba == bb && ai > bj)) return;
    double sum = 0.0;
    for (int64_t seg = 0; seg < nseg; ++seg) sum = sum + part[((size_t)seg * gridDim.x + blockIdx.x) * 4096 + e];
    S[(size_t)a * d + b] = sum;
    S[(size_t)b * d + a] = sum;
}

// dst4 (tiled, dp4o chunks a row) <- the projection of src4 (tiled, dp4 chunks a row), tiles [0, tiles). grid (workgroups, groups of
// NOB 16-feature output blocks); a wave takes one tile at a time, 4 x NOB result blocks of 16 rows x 16 features. Rows at or past n and
// features at or past p are written as zeros (the layout invariant); range[0] is set as k_retile sets it (range NULL: a scratch tile).
template <int NOB>
__global__ void __launch_bounds__(kBlock) k_pj_project(const float4* __restrict__ src4, int64_t n, int64_t tiles, int dp4, int nss, const pj_double4* __restrict__ wp,
                                                        const double* __restrict__ bias, int p, int dp4o, float4* __restrict__ dst4, int32_t* __restrict__ range) {
    const int lane = threadIdx.x & 63, lr = lane & 15, lk = lane >> 4;
    const int ob0 = blockIdx.y * NOB;
    const float4 zero4 = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int64_t t = (int64_t)blockIdx.x * (kBlock / 64) + (threadIdx.x >> 6); t < tiles; t += (int64_t)gridDim.x * (kBlock / 64)) {
        const float4* s = src4 + (size_t)t * dp4 * 64 + lr;
        pj_double4 acc[NOB][4];
#pragma unroll
        for (int ob = 0; ob < NOB; ++ob)
#pragma unroll
            for (int rb = 0; rb < 4; ++rb) acc[ob][rb] = (pj_double4){0.0, 0.0, 0.0, 0.0};
        float4 g[4];
#pragma unroll
        for (int rb = 0; rb < 4; ++rb) g[rb] = lk < dp4 ? s[(size_t)lk * 64 + rb * 16] : zero4;
        for (int ss = 0; ss < nss; ++ss) {
            float4 gn[4];                                               // the next super-step's rows are in flight under this one's MFMAs
            const int cn = 4 * (ss + 1) + lk;
#pragma unroll
            for (int rb = 0; rb < 4; ++rb) gn[rb] = cn < dp4 ? s[(size_t)cn * 64 + rb * 16] : zero4;
            pj_double4 w[NOB];
#pragma unroll
            for (int ob = 0; ob < NOB; ++ob) w[ob] = wp[((size_t)(ob0 + ob) * nss + ss) * 64 + lane];
#pragma unroll
            for (int comp = 0; comp < 4; ++comp) {
                double gd[4];
#pragma unroll
                for (int rb = 0; rb < 4; ++rb) gd[rb] = (double)pj_comp(g[rb], comp);
#pragma unroll
                for (int ob = 0; ob < NOB; ++ob)
#pragma unroll
                    for (int rb = 0; rb < 4; ++rb) acc[ob][rb] = __builtin_amdgcn_mfma_f64_16x16x4f64(w[ob][comp], gd[rb], acc[ob][rb], 0, 0, 0);
            }
#pragma unroll
            for (int rb = 0; rb < 4; ++rb) g[rb] = gn[rb];
        }
        // D: col = lane & 15 -> row 16 rb + lr of the tile; row = lk + 4 * reg -> output feature 16 (ob0 + ob) + 4 lk + reg
        bool plain = true;
#pragma unroll
        for (int ob = 0; ob < NOB; ++ob) {
            const int chunk = (ob0 + ob) * 4 + lk;
            if (chunk >= dp4o) continue;
            double b[4];
#pragma unroll
            for (int reg = 0; reg < 4; ++reg) b[reg] = bias[chunk * 4 + reg];
#pragma unroll
            for (int rb = 0; rb < 4; ++rb) {
                const int64_t row = t * kTileRows + rb * 16 + lr;
                float v[4];
#pragma unroll
                for (int reg = 0; reg < 4; ++reg) v[reg] = row < n && chunk * 4 + reg < p ? (float)(acc[ob][rb][reg] - b[reg]) : 0.0f;
                plain = plain && in_plain_range(v[0]) && in_plain_range(v[1]) && in_plain_range(v[2]) && in_plain_range(v[3]);
                dst4[((size_t)t * dp4o + chunk) * 64 + rb * 16 + lr] = make_float4(v[0], v[1], v[2], v[3]);
            }
        }
        if (range && !plain) range[0] = 1;
    }
}

// ---- host side ---------------------------------------------------------------------------------------------------------------------
// The selected rows of a host mask over n rows (NULL: all of them).
int64_t pj_count(const uint64_t* mask, int64_t n) {
    if (!mask) return n;
    int64_t c = 0;
    const int64_t words = FIR_MASK_WORDS(n);
    for (int64_t i = 0; i < words; ++i) {
        uint64_t w = mask[i];
        if (i == words - 1 && (n & 63)) w &= (1ull << (n & 63)) - 1ull;
        c += __builtin_popcountll(w);
    }
    return c;
}
int pj_check_gallery(const fir_gallery* g) {
    if (!g) return fir_fail_(FIR_ERR_ARG, "NULL argument");
    if (g->n == 0) return fir_fail_(FIR_ERR_ARG, "the gallery is empty");
    return FIR_OK;
}
// Room for the column statistics: the partials and, behind them, the folded [4][dk].
int pj_stats_room(fir_gallery* g, PjPlan& plan) {
    plan = pj_plan(g->tiles, kPjStatSegs);
    return FIR_NEED(g->pjstat, (size_t)(plan.nseg + 1) * 4 * g->dp4 * 4);
}
double* pj_stats_out(const fir_gallery* g, const PjPlan& plan) { return g->pjstat + (size_t)plan.nseg * 4 * g->dp4 * 4; }
// ... and the two launches, on `st`. d_mask: device words or NULL.
int pj_stats_launch(fir_gallery* g, const PjPlan& plan, const uint64_t* d_mask, hipStream_t st) {
    const int dk = g->dp4 * 4;
    hipLaunchKernelGGL(k_pj_col_stats, dim3((unsigned)plan.nseg, (unsigned)((g->dp4 + kBlock / 64 - 1) / (kBlock / 64))), dim3(kBlock), 0, st,
                       (const float4*)g->gal4, g->n, g->tiles, g->dp4, d_mask, plan.seg_tiles, (double*)g->pjstat);
    hipLaunchKernelGGL(k_pj_col_fold, dim3((unsigned)((dk + kBlock - 1) / kBlock)), dim3(kBlock), 0, st, (const double*)g->pjstat, plan.nseg, dk,
                       pj_stats_out(g, plan));
    FIR_HIP(hipGetLastError());
    return FIR_OK;
}
// The host mask into g->dmask on the handle's stream (room was made): the device words, NULL for a NULL mask.
int pj_mask_upload(fir_gallery* g, const uint64_t* mask, const uint64_t** d_mask) {
    *d_mask = nullptr;
    if (!mask) return FIR_OK;
    FIR_HIP(hipMemcpyAsync(g->dmask, mask, (size_t)FIR_MASK_WORDS(g->n) * sizeof(uint64_t), hipMemcpyHostToDevice, g->stream));
    *d_mask = g->dmask;
    return FIR_OK;
}

}  // namespace

// A p x d linear map on one device: the basis in the A operand's order, the bias, the re-tiling scratch of the row-major form, and
// the order of its own calls (an event, as a gallery handle keeps one).
struct fir_projection {
    int device = 0, cus = 0;
    int p = 0, d = 0, dp4 = 0, dp4o = 0, nss = 0;
    FirBuf wp, bias;              // [blocks][nss][64] pj_double4; [blocks * 16] doubles, blocks = 4 * ceil(p / 64)
    FirBuf tin, tout;             // one slab of rows, tiled: the input and its projection
    FirBuf hin, hout;             // fir_projection_apply: the slab's row-major rows and results
    hipStream_t stream = nullptr;
    hipEvent_t last_done = nullptr;
    bool used = false;            // last_done has been recorded
    ~fir_projection() {
        if (last_done) (void)hipEventDestroy(last_done);
        if (stream) (void)hipStreamDestroy(stream);
    }
};

namespace {

int pj_project_launch(const fir_projection* pr, const float4* src4, int64_t n, int64_t tiles, float4* dst4, int32_t* range, hipStream_t st) {
    const int nob = pr->p <= 16 ? 1 : pr->p <= 32 ? 2 : 4;
    const int groups = (pr->p + 16 * nob - 1) / (16 * nob);
    const int64_t wgs = std::min<int64_t>((tiles + kBlock / 64 - 1) / (kBlock / 64), (int64_t)pr->cus * 8);
    const dim3 grid((unsigned)wgs, (unsigned)groups);
    const pj_double4* wp = pr->wp.as<pj_double4>();
    const double* bias = pr->bias.as<double>();
    if (nob == 1) hipLaunchKernelGGL(k_pj_project<1>, grid, dim3(kBlock), 0, st, src4, n, tiles, pr->dp4, pr->nss, wp, bias, pr->p, pr->dp4o, dst4, range);
    else if (nob == 2) hipLaunchKernelGGL(k_pj_project<2>, grid, dim3(kBlock), 0, st, src4, n, tiles, pr->dp4, pr->nss, wp, bias, pr->p, pr->dp4o, dst4, range);
    else hipLaunchKernelGGL(k_pj_project<4>, grid, dim3(kBlock), 0, st, src4, n, tiles, pr->dp4, pr->nss, wp, bias, pr->p, pr->dp4o, dst4, range);
    FIR_HIP(hipGetLastError());
    return FIR_OK;
}
int64_t pj_apply_slab(const fir_projection* pr) {
    return std::max<int64_t>(kTileRows, (int64_t)(kPjApplyBytes / ((size_t)(pr->dp4 + pr->dp4o) * 16)) / kTileRows * kTileRows);
}
// Room for slabs of up to `rows` rows. Growing frees the old blocks: earlier calls have to be through with them.
int pj_apply_room(fir_projection* pr, int64_t rows, bool host) {
    const size_t tiles = (size_t)((rows + kTileRows - 1) / kTileRows);
    const size_t in = tiles * pr->dp4 * 64 * sizeof(float4), out = tiles * pr->dp4o * 64 * sizeof(float4);
    const size_t hin = host ? (size_t)rows * pr->d * sizeof(float) : 0, hout = host ? (size_t)rows * pr->p * sizeof(float) : 0;
    if (in <= pr->tin.cap && out <= pr->tout.cap && hin <= pr->hin.cap && hout <= pr->hout.cap) return FIR_OK;
    if (pr->used) FIR_HIP(hipEventSynchronize(pr->last_done));
    int rc;
    if ((rc = FIR_RESERVE(pr->tin, in)) || (rc = FIR_RESERVE(pr->tout, out))) return rc;
    if (host && ((rc = FIR_RESERVE(pr->hin, hin)) || (rc = FIR_RESERVE(pr->hout, hout)))) return rc;
    return FIR_OK;
}
// One slab, row-major device rows -> row-major device results, on `st`: re-tile, project, un-tile.
int pj_apply_slab_dev(fir_projection* pr, const float* d_rows, int64_t have, float* d_out, hipStream_t st) {
    const int64_t tiles = (have + kTileRows - 1) / kTileRows;
    hipLaunchKernelGGL(k_retile, dim3((unsigned)((tiles * pr->dp4 * 64 + kBlock - 1) / kBlock)), dim3(kBlock), 0, st, d_rows, have, (int64_t)0, have, pr->d, pr->dp4,
                       pr->tin.as<float4>(), (int32_t*)nullptr);
    int rc = pj_project_launch(pr, pr->tin.as<float4>(), have, tiles, pr->tout.as<float4>(), nullptr, st);
    if (rc) return rc;
    hipLaunchKernelGGL(k_untile_rows, dim3((unsigned)((have * pr->dp4o + kBlock - 1) / kBlock)), dim3(kBlock), 0, st, (const float4*)pr->tout.as<float4>(), pr->dp4o,
                       pr->p, (int64_t)0, have, d_out);
    FIR_HIP(hipGetLastError());
    return FIR_OK;
}
// The order of a projection's calls: `st` waits for the previous call; the end of this one is recorded when the scope is left.
struct PjCall {
    fir_projection* pr;
    hipStream_t st;
    int rc = FIR_OK;
    PjCall(fir_projection* pr_, hipStream_t st_) : pr(pr_), st(st_) {
        if (pr->used && hipStreamWaitEvent(st, pr->last_done, 0) != hipSuccess) rc = fir_fail_(FIR_ERR_HIP, "hipStreamWaitEvent (projection call order)");
    }
    ~PjCall() { if (hipEventRecord(pr->last_done, st) == hipSuccess) pr->used = true; }
};

}  // namespace

extern "C" {

// h[0..3][dk] <- the folded column statistics of the selected rows (sum, sum of squares, min, max), dk = 4 dp4: one call on the handle.
static int pj_feature_stats(fir_gallery* g, const uint64_t* mask, std::vector<double>& h) {
    int rc = pj_check_gallery(g);
    if (rc) return rc;
    FIR_HIP(hipSetDevice(g->device));
    PjPlan plan;
    if ((mask && (rc = FIR_NEED(g->dmask, (size_t)FIR_MASK_WORDS(g->n)))) || (rc = pj_stats_room(g, plan))) return rc;
    GalleryCall call(g);
    if (call.rc) return call.rc;
    const uint64_t* d_mask = nullptr;
    if ((rc = pj_mask_upload(g, mask, &d_mask)) || (rc = pj_stats_launch(g, plan, d_mask, g->stream))) return rc;
    h.resize((size_t)4 * g->dp4 * 4);
    FIR_HIP(hipMemcpyAsync(h.data(), pj_stats_out(g, plan), h.size() * sizeof(double), hipMemcpyDeviceToHost, g->stream));
    FIR_HIP(hipStreamSynchronize(g->stream));
    call.done();
    return FIR_OK;
}

int fir_gallery_feature_sums_(fir_gallery* g, const uint64_t* mask, double* sum, double* sum_sq) {
    if (!sum || !sum_sq) return fir_fail_(FIR_ERR_ARG, "NULL argument");
    std::vector<double> h;
    const int rc = pj_feature_stats(g, mask, h);
    if (rc) return rc;
    const int dk = g->dp4 * 4;
    std::copy(h.begin(), h.begin() + g->d, sum);
    std::copy(h.begin() + dk, h.begin() + dk + g->d, sum_sq);
    return FIR_OK;
}

int fir_gallery_feature_stats(fir_gallery* g, const uint64_t* mask, int64_t* count, double* min, double* max, double* avg, double* sd) {
    std::vector<double> h;
    const int rc = pj_feature_stats(g, mask, h);
    if (rc) return rc;
    const int dk = g->dp4 * 4;
    const int64_t m = pj_count(mask, g->n);
    if (count) *count = m;
    const double cnt = (double)m;
    for (int k = 0; k < g->d; ++k) {
        const double a = h[(size_t)k] / cnt;
        if (min) min[k] = h[(size_t)2 * dk + k];
        if (max) max[k] = h[(size_t)3 * dk + k];
        if (avg) avg[k] = a;
        if (sd) sd[k] = sqrt((h[(size_t)dk + k] - a * a * cnt) / (cnt - 1.0));
    }
    return FIR_OK;
}

int fir_gallery_scatter(fir_gallery* g, const uint64_t* mask, const double* center, double* scatter, double* mean_out, int64_t* count) {
    int rc = pj_check_gallery(g);
    if (rc) return rc;
    if (!scatter) return fir_fail_(FIR_ERR_ARG, "NULL argument");
    if (g->d > kPjMaxDim) return fir_fail_(FIR_ERR_ARG, "d=%d: fir_gallery_scatter takes at most %d features", g->d, kPjMaxDim);
    FIR_HIP(hipSetDevice(g->device));
    const int d = g->d, nb = (d + 63) / 64, pairs = pj_pairs(nb);
    const PjPlan plan = pj_scatter_plan(g->tiles, nb);
    PjPlan splan;
    // everything the call needs, before anything is queued
    if ((mask && (rc = FIR_NEED(g->dmask, (size_t)FIR_MASK_WORDS(g->n)))) || (!center && (rc = pj_stats_room(g, splan))) ||
        (rc = FIR_NEED(g->pjcen, (size_t)nb * 64)) || (rc = FIR_NEED(g->pjpart, (size_t)plan.nseg * pairs * 4096)) || (rc = FIR_NEED(g->pjout, (size_t)d * d)))
        return rc;
    GalleryCall call(g);
    if (call.rc) return call.rc;
    const uint64_t* d_mask = nullptr;
    if ((rc = pj_mask_upload(g, mask, &d_mask))) return rc;
    const int64_t m = pj_count(mask, g->n);
    std::vector<double> cen((size_t)nb * 64, 0.0);
    if (center) std::copy(center, center + d, cen.begin());
    else {
        if ((rc = pj_stats_launch(g, splan, d_mask, g->stream))) return rc;
        std::vector<double> sums((size_t)d);
        FIR_HIP(hipMemcpyAsync(sums.data(), pj_stats_out(g, splan), (size_t)d * sizeof(double), hipMemcpyDeviceToHost, g->stream));
        FIR_HIP(hipStreamSynchronize(g->stream));
        if (m > 0)
            for (int k = 0; k < d; ++k) cen[(size_t)k] = sums[(size_t)k] / (double)m;
    }
    FIR_HIP(hipMemcpyAsync(g->pjcen, cen.data(), cen.size() * sizeof(double), hipMemcpyHostToDevice, g->stream));
    hipLaunchKernelGGL(k_pj_scatter, dim3((unsigned)pairs, (unsigned)plan.nseg), dim3(kBlock), 0, g->stream, (const float4*)g->gal4, g->n, g->tiles, g->dp4, d_mask,
                       (const double*)g->pjcen, nb, plan.seg_tiles, (double*)g->pjpart);
    hipLaunchKernelGGL(k_pj_scatter_fold, dim3((unsigned)pairs, 4096 / kBlock), dim3(kBlock), 0, g->stream, (const double*)g->pjpart, plan.nseg, nb, d, (double*)g->pjout);
    FIR_HIP(hipGetLastError());
    FIR_HIP(hipMemcpyAsync(scatter, g->pjout, (size_t)d * d * sizeof(double), hipMemcpyDeviceToHost, g->stream));
    FIR_HIP(hipStreamSynchronize(g->stream));
    call.done();
    if (mean_out) std::copy(cen.begin(), cen.begin() + d, mean_out);
    if (count) *count = m;
    return FIR_OK;
}

int fir_projection_create(const double* basis, int32_t p, int32_t d, const double* center, int32_t device, fir_projection** out) {
    if (out) *out = nullptr;
    if (!basis || !out) return fir_fail_(FIR_ERR_ARG, "NULL argument");
    if (p < 1 || p > kPjMaxDim) return fir_fail_(FIR_ERR_ARG, "p=%d outside [1,%d]", p, kPjMaxDim);
    if (d < 1) return fir_fail_(FIR_ERR_ARG, "d=%d must be positive", d);
    int rc = set_device(device);
    if (rc) return rc;
    hipDeviceProp_t prop;
    FIR_HIP(hipGetDeviceProperties(&prop, device));
    if (strncmp(prop.gcnArchName, "gfx950", 6) != 0) return fir_fail_(FIR_ERR_NODEVICE, "device %d is %s; this library is built for gfx950 only", device, prop.gcnArchName);
    fir_projection* pr = new (std::nothrow) fir_projection();
    if (!pr) return fir_fail_(FIR_ERR_NOMEM, "host allocation failed");
    const auto fail = [pr](int code) { delete pr; return code; };
    pr->device = device;
    pr->cus = prop.multiProcessorCount;
    pr->p = p;
    pr->d = d;
    pr->dp4 = (d + 3) / 4;
    pr->dp4o = (p + 3) / 4;
    pr->nss = (pr->dp4 + 3) / 4;
    const int blocks = (p + 63) / 64 * 4;                                // 16-feature output blocks, whole groups of any NOB
    // the A operand's order: lane (lr, lk) of super-step s holds W[16 ob + 4 (lr & 3) + (lr >> 2)][4 (4 s + lk) + comp], comp = 0..3
    std::vector<double> wp((size_t)blocks * pr->nss * 64 * 4, 0.0), bias((size_t)blocks * 16, 0.0);
    for (int ob = 0; ob < blocks; ++ob)
        for (int lr = 0; lr < 16; ++lr) {
            const int k = ob * 16 + 4 * (lr & 3) + (lr >> 2);
            if (k >= p) continue;
            const double* w = basis + (size_t)k * d;
            for (int s = 0; s < pr->nss; ++s)
                for (int lk = 0; lk < 4; ++lk)
                    for (int comp = 0; comp < 4; ++comp) {
                        const int f = 4 * (4 * s + lk) + comp;
                        if (f < d) wp[(((size_t)ob * pr->nss + s) * 64 + lk * 16 + lr) * 4 + comp] = w[f];
                    }
            if (center) {
                double b = 0.0;
                for (int f = 0; f < d; ++f) b = b + center[f] * w[f];
                bias[(size_t)k] = b;
            }
        }
    if ((rc = FIR_RESERVE(pr->wp, wp.size() * sizeof(double))) || (rc = FIR_RESERVE(pr->bias, bias.size() * sizeof(double)))) return fail(rc);
    hipError_t e = hipStreamCreateWithFlags(&pr->stream, hipStreamNonBlocking);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&pr->last_done, hipEventDisableTiming);
    if (e == hipSuccess) e = hipMemcpyAsync(pr->wp.p, wp.data(), wp.size() * sizeof(double), hipMemcpyHostToDevice, pr->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(pr->bias.p, bias.data(), bias.size() * sizeof(double), hipMemcpyHostToDevice, pr->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(pr->stream);
    if (e != hipSuccess) return fail(fir_fail_(FIR_ERR_HIP, "projection upload: %s", hipGetErrorString(e)));
    *out = pr;
    return FIR_OK;
}

int fir_projection_destroy(fir_projection* pr) {
    if (!pr) return FIR_OK;
    (void)hipSetDevice(pr->device);
    if (pr->used) (void)hipEventSynchronize(pr->last_done);
    if (pr->stream) (void)hipStreamSynchronize(pr->stream);
    delete pr;
    return FIR_OK;
}

int fir_projection_info(const fir_projection* pr, int32_t* p, int32_t* d, int32_t* device) {
    if (!pr) return fir_fail_(FIR_ERR_ARG, "projection is NULL");
    if (p) *p = pr->p;
    if (d) *d = pr->d;
    if (device) *device = pr->device;
    return FIR_OK;
}

int fir_projection_apply_dev(fir_projection* pr, const float* d_rows, int64_t m, float* d_out, void* stream) {
    if (!pr || (m > 0 && (!d_rows || !d_out))) return fir_fail_(FIR_ERR_ARG, "NULL argument");
    if (m < 0) return fir_fail_(FIR_ERR_ARG, "m < 0");
    if (m == 0) return FIR_OK;
    FIR_HIP(hipSetDevice(pr->device));
    const int64_t slab = std::min(pj_apply_slab(pr), m);
    int rc = pj_apply_room(pr, slab, false);
    if (rc) return rc;
    PjCall call(pr, stream ? (hipStream_t)stream : pr->stream);
    if (call.rc) return call.rc;
    for (int64_t r0 = 0; r0 < m; r0 += slab)
        if ((rc = pj_apply_slab_dev(pr, d_rows + r0 * pr->d, std::min(slab, m - r0), d_out + r0 * pr->p, call.st))) return rc;
    return FIR_OK;
}

int fir_projection_apply(fir_projection* pr, const float* rows, int64_t m, float* out) {
    if (!pr || (m > 0 && (!rows || !out))) return fir_fail_(FIR_ERR_ARG, "NULL argument");
    if (m < 0) return fir_fail_(FIR_ERR_ARG, "m < 0");
    if (m == 0) return FIR_OK;
    FIR_HIP(hipSetDevice(pr->device));
    const int64_t slab = std::min(pj_apply_slab(pr), m);
    int rc = pj_apply_room(pr, slab, true);
    if (rc) return rc;
    PjCall call(pr, pr->stream);
    if (call.rc) return call.rc;
    for (int64_t r0 = 0; r0 < m; r0 += slab) {
        const int64_t have = std::min(slab, m - r0);
        FIR_HIP(hipMemcpyAsync(pr->hin.p, rows + r0 * pr->d, (size_t)have * pr->d * sizeof(float), hipMemcpyHostToDevice, pr->stream));
        if ((rc = pj_apply_slab_dev(pr, pr->hin.as<float>(), have, pr->hout.as<float>(), pr->stream))) return rc;
        FIR_HIP(hipMemcpyAsync(out + r0 * pr->p, pr->hout.p, (size_t)have * pr->p * sizeof(float), hipMemcpyDeviceToHost, pr->stream));
        FIR_HIP(hipStreamSynchronize(pr->stream));              // the staging buffers are reused by the next slab
    }
    return FIR_OK;
}

int fir_gallery_create_projected(fir_gallery* src, fir_projection* pr, fir_gallery** out) {
    if (out) *out = nullptr;
    if (!src || !pr || !out) return fir_fail_(FIR_ERR_ARG, "NULL argument");
    if (src->n == 0) return fir_fail_(FIR_ERR_ARG, "the gallery is empty");
    if (pr->d != src->d) return fir_fail_(FIR_ERR_ARG, "the projection maps %d features, the gallery has %d", pr->d, src->d);
    if (pr->device != src->device) return fir_fail_(FIR_ERR_ARG, "the projection is on device %d, the gallery on device %d", pr->device, src->device);
    FIR_HIP(hipSetDevice(src->device));
    fir_gallery* g = nullptr;
    int rc = gallery_alloc(src->n, pr->p, src->metric, src->device, &g);
    if (rc) return rc;
    if (src->cls) {
        const hipError_t e = labels_alloc(g);
        if (e != hipSuccess) {
            delete g;
            return fir_fail_(e == hipErrorOutOfMemory ? FIR_ERR_NOMEM : FIR_ERR_HIP, "hipMalloc of the projected handle's labels: %s", hipGetErrorString(e));
        }
    }
    g->row_offset = src->row_offset;
    GalleryCall call(src);                                   // a call on the SOURCE: after its queued appends, before its later mutations
    if (call.rc) { delete g; return call.rc; }
    PjCall pcall(pr, call.st);                               // ... and on the projection
    rc = pcall.rc;
    if (rc == FIR_OK) rc = pj_project_launch(pr, (const float4*)src->gal4, src->n, src->tiles, (float4*)g->gal4, (int32_t*)g->range, call.st);
    if (rc == FIR_OK && src->cls) {
        const hipError_t e = hipMemcpyAsync(g->cls, src->cls, (size_t)src->n * sizeof(int32_t), hipMemcpyDeviceToDevice, call.st);
        if (e != hipSuccess) rc = fir_fail_(FIR_ERR_HIP, "class copy: %s", hipGetErrorString(e));
    }
    rc = created_dev(g, rc, call.st, out);
    if (rc == FIR_OK) call.done();
    return rc;
}

}  // extern "C"
