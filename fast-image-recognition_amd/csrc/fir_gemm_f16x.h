// fir_gemm_f16x.h -- the fp16 matrix-core kernels (FIR_GEMM_F16), on v_mfma_f32_16x16x32_f16 (included by fir_gemm.hip,
// inside its anonymous namespace). One wave computes 32 rows x 128 queries with the query tile in LDS. This is the only fp16
// form: a 32x32x16 kernel at the same per-wave tile (same bytes per MFMA cycle from LDS and from the gallery stream; the chip
// clocks the two MFMA shapes differently under load) and a kernel with the query fragments in registers were measured against
// it and removed (profiles/r03_mfma_shape_ab.txt, profiles/fp16_single_form_ab.txt). Both operands are in the "16-row"
// fragment order:
//
//   gallery  gh[(rb * dk16 + 2 * kk + s) * 64 + l]   row 32 rb + 16 s + (l & 15),   features 32 kk + 8 (l >> 4) + 0..7
//   queries  qh[((pair * 8 + jb) * dk32 + kk) * 64 + l]   query 128 pair + 16 jb + (l & 15),   the same features
//
// (dk32 = dk16 / 2; a row block is dk16 consecutive one-KiB pieces, dk16 a multiple of kRing: the fp16 fragments are padded to
// whole double-buffer units.) Accumulator tile (s, jb): f32x4, lane l holds query 16 jb + (l & 15) against
// rows 16 s + 4 (l >> 4) + 0..3 of the block.
#pragma once
#include <type_traits>

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef int i32x4 __attribute__((ext_vector_type(4)));

// rows of the tiled f32 gallery * scale (a power of two) -> 16-row fragment order (see above), round to nearest even
// kmax: features [0, kmax) of every row are packed, the rest of the fragments is zero (kmax = dp4 * 4: the whole row)
__global__ void __launch_bounds__(256) k_gemm_pack_gallery_f16x(const float4* __restrict__ gal4, int64_t n, int dp4, int dk16, float scale,
                                                                 uint4* __restrict__ gh, int kmax) {
    const int64_t o = (int64_t)blockIdx.x * 256 + threadIdx.x;      // (rb, piece, lane)
    const int64_t rblocks = (n + 31) / 32;
    if (o >= rblocks * dk16 * 64) return;
    const int l = (int)(o & 63);
    const int64_t t = o >> 6;
    const int piece = (int)(t % dk16);
    const int64_t rb = t / dk16;
    const int kk = piece >> 1, s = piece & 1;
    const int64_t row = rb * 32 + 16 * s + (l & 15);
    f16x8 v;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const int k = 32 * kk + 8 * (l >> 4) + j;
        float x = 0.f;
        if (row < n && k < kmax) {
            const float4 g = gal4[((row >> 6) * dp4 + (k >> 2)) * 64 + (row & 63)];
            x = (k & 3) == 0 ? g.x : (k & 3) == 1 ? g.y : (k & 3) == 2 ? g.z : g.w;
        }
        v[j] = (_Float16)(x * scale);
    }
    uint4 u;
    __builtin_memcpy(&u, &v, 16);
    gh[o] = u;
}

// queries * qmul -> 16-row fragment order; blockIdx.y = pair of 64-query passes
// qmap (a second-chance round, fir_gemm_fb.h): slot i of the one pair is query qmap[i] of the call, state[0] - live_off slots are live
__global__ void __launch_bounds__(256) k_gemm_pack_queries_f16x(const float* q, int nq, int d, int dk16, const float* __restrict__ qmul, uint4* qh,
                                                                 int qstride, const int* __restrict__ qmap = nullptr, const int* __restrict__ state = nullptr,
                                                                 int live_off = 0) {
    if (qmap) {
        nq = state[0] - live_off;
        if (nq <= 0) return;
        nq = nq < 2 * kQT ? nq : 2 * kQT;
    }
    const int dk32 = dk16 >> 1;
    const int q_base = (int)blockIdx.y * 2 * kQT;
    qh += (size_t)blockIdx.y * 8 * dk32 * 64;
    const int o = blockIdx.x * 256 + threadIdx.x;
    if (o >= 8 * dk32 * 64) return;
    const int l = o & 63;
    const int t = o >> 6;
    const int kk = t % dk32, jb = t / dk32;
    const int qi = q_base + jb * 16 + (l & 15);
    const float mul = qi < nq ? qmul[qi] : 0.f;
    f16x8 v;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const int k = 32 * kk + 8 * (l >> 4) + j;
        const float x = (qi < nq && k < d) ? q[(size_t)(qmap ? qmap[qi] : qi) * qstride + k] : 0.f;
        v[j] = (_Float16)(x * mul);
    }
    uint4 u;
    __builtin_memcpy(&u, &v, 16);
    qh[o] = u;
}

// the MFMA of the 16-row kernels by accumulator type: f32 sums of fp16 products, or (the int8 form) i32 sums of the same registers' bytes
__device__ __forceinline__ f32x4 mfma_x_(const f16x8 a, const f16x8 b, const f32x4 c) { return __builtin_amdgcn_mfma_f32_16x16x32_f16(a, b, c, 0, 0, 0); }
__device__ __forceinline__ i32x4 mfma_x_(const f16x8 a, const f16x8 b, const i32x4 c) {
    i32x4 ai, bi;
    __builtin_memcpy(&ai, &a, 16);
    __builtin_memcpy(&bi, &b, 16);
    return __builtin_amdgcn_mfma_i32_16x16x64_i8(ai, bi, c, 0, 0, 0);
}

// One wave: 32 rows x 128 queries. Dynamic LDS: kHalfLds. All per-pass scratch is laid out pass-major (128 consecutive queries
// per pair of passes). Which pair and which row groups a workgroup takes:
// share == 0: blockIdx.y = pair, row groups blockIdx.x, + gridDim.x, ...
// share == P (a power of two): ONE workgroup per CU, all resident at once; the P pairs of the launch read the gallery TOGETHER:
// the row groups are cut into gridDim.x / P contiguous ranges and P workgroups -- one per pair, placed on the same XCD (blocks b
// and b + 8 share one) -- walk the same range at the same time, so the fp16 gallery stream leaves HBM once per P * 128 queries and
// the other P - 1 readers hit in the XCD's L2 (or, when they drift apart, in the Infinity Cache).
// The gallery stream is a double buffer of kRing pieces: the loads of the NEXT unit -- of this row block, or the first of the
// wave's next row block -- are all issued before the MFMA steps of the current one, so the only wait per unit is at its end. (A
// ring that reloads each slot right after use needs counted waits inside a loop, which the compiler turns into vmcnt(0) per
// step: one memory latency per k-block -- measured 358 us per pass against 158 us of gallery stream.)
// ODD = units (of kRing pieces) per row block is odd: only then do the two gallery buffers end a row block in swapped roles
// and need a copy; with the even form compiled separately the common row lengths (256, 512, 1280 features) carry neither the
// copy nor the merge point the compiler hung an s_waitcnt vmcnt(0) on. ODD = 1: three units or more; ODD = 2: ONE unit (at most 128
// features), which is the row block's first and last unit at once -- a form of its own, so that every kernel's row loop is one
// sequence of units (as two run-time paths inside the ODD = 1 kernels it cost those 500 bytes of scratch per lane).
// MODE is 1, 2, 3 or 4 (4 = MODE 3 for the K nearest rows: at kSlots, inside the kernel).
// MODE 1: the full pass, every row below tau is appended; MODE 2: the sample of the smallest-proxy flow -- row blocks
// 0, rb_stride, 2 rb_stride, ... of the gallery ((row_end - row_begin) / 32 of them, spread over all of it: the reference's
// galleries are ordered by class), smin[q] <- the smallest proxy seen (fir::f32_orderable bits, atomicMin, caller presets +inf);
// with sub_stride != 0 (top-K) as kRtSubsets disjoint subsets' minima, smin[subset * sub_stride + q] (k_gemm_tau_kmin).
// MODE 3: the full pass with the threshold found ON THE WAY (top-1; no sample pass, no threshold kernel): per query the ranks
// keep T = (smallest proxy seen so far + |q|^2) + one rounding window, as float bits >= 0 so that an unsigned atomicMin orders
// them -- in LDS per workgroup, mirrored to `smin` (global) by atomicMin whenever a workgroup lowers it (that is where the final
// bound comes from); the workgroups exchange once, behind their warm-up walk, which leaves every one of them with the minimum
// over the first row blocks of about half the chip (tens of thousands of rows: what the sample pass used to provide) -- a
// re-read of `smin` into a register held across the row block measured slower than the appends it saved (256 VGPRs: it spilled a
// loop-carried pointer), and loads of `smin` -- plain, sc1 or LDS-DMA -- turned out to be served from stale lines of the XCD's own
// L2; each wave therefore posts-and-fetches its sixteen queries' T with ONE returning atomicMin on a thinning schedule
// (profiles/r03_adaptive_threshold.txt). A row is appended when its proxy is below tq = T - |q|^2 AT THAT MOMENT. T only ever
// falls, so whatever was not appended has a proxy >= fl(T_final - |q|^2) =: tau, which k_gemm_adapt_final hands to the
// re-rank's certificate; and every row within the window of the smallest proxy of ALL rows IS appended (its proxy is below
// every T the pass ever held). With T = +inf at the start the first row block of a wave would append all its rows: its sums
// are therefore looked at twice -- once only lowering T (then the workgroup exchanges T with `smin`), then, still in the
// registers, for real. Here `tau` carries the windows, `qnorm` the |q|^2, `smin` the global T.
// A unit is kRing = 8 gallery pieces = four 32-feature steps; per step two A fragments (the row halves) against eight B
// fragments: sixteen MFMAs of 16 cycles. The eight B fragments are ONE register set that rolls: fragment j is re-read for
// the next step right behind the two MFMAs that used it, fourteen MFMAs before its next use.
// `nt_flags` bit 0: the gallery stream is read once per launch (non-temporal loads; pairs that share it use ordinary loads, so that
// the line stays in L2 for the other readers). Bits 2, 3: the audit build's looser adaptive bound (no refresh / no exchange).
// No other bit is read. The experiments that further `nt_flags` bits and further DBG bits once switched were measured, not kept, and are
// gone from the kernel: what they were and what they gave is in DESIGN.md section 4, "The 16-row kernels", and under profiles/.
constexpr int kXStage = 16;             // staged appends per query and workgroup
// NJB: query blocks of 16 the wave multiplies against (8 = the whole 128-query tile). A call of at most 16 / 32 queries fills one / two
// blocks; with NJB = 1 / 2 the pass does an eighth / a quarter of the MFMAs and LDS reads and is what such a call should be: one read
// of the fp16 fragments at the rate the memory system gives (the tile's layout in LDS and in `qh` is unchanged).
// DBG (timing experiments only, FIR_GEMM_DBG_SKIP; own instantiations so that the production kernels' register allocation is not
// touched -- as runtime flags the two tests made the row loop spill): bit 0 = no epilogue, bit 1 = no gallery stream, bit 2 = no
// re-read of the query fragments, bit 5 = no MFMAs (values 1, 2, 4, 32). The answers of such a kernel are wrong. Right answers: bit 8
// (value 256) = timestamps of workgroup 0's waves.
// I8: the int8 form (v_mfma_i32_16x16x64_i8, twice the features per instruction). A one-KiB piece is then 16 rows x 64 features -- lane
// l holds row l & 15, the sixteen features 64 kk + 16 (l >> 4) + 0..15 as bytes -- so a unit of kRing pieces is 256 features and the loop
// over `dk16` pieces is the fp16 form's at half the features: the gallery is `g8` of fir_gemm_i8.h (rows minus the column means, one
// scale), `gnorm` the norms of the centred rows, `qinv` 1 / (s_q s_g). The sums are exact integers (|sum| <= 1024 * 127^2 < 2^24: their
// conversion to f32 is exact); the check takes the lane's maximum on the integers and converts once (conversion is monotone: the
// argument of check_jb holds), everything else converts the sum it reads. Resident tiles only, MODE 1 and 3.
// QH: tile halves of 128 queries a workgroup holds (2: the 256-query tile of <3, 0, 0, DBG, 8, I8 = 1> -- two pairs' int8 images of up to
// 512 features in the 128 KiB of dynamic LDS, `share` counts tiles, every gallery fragment is multiplied against both halves: see `unit`).
template <int MODE, int STREAMED, int ODD, int DBG = 0, int NJB = 8, int I8 = 0, int QH = 1>
__global__ void __launch_bounds__(kGemmBlock, 1) k_gemm_proxy_f16x(const uint4* __restrict__ gh, const float* __restrict__ gnorm, const uint4* qh,
                                                                    const float* __restrict__ qinv, int64_t n, int64_t row_begin, int64_t row_end,
                                                                    int dk16, const float* tau, unsigned long long* lists, int* counts,
                                                                    float* qnorm, int share, int nt_flags,
                                                                    int rb_stride, unsigned int* smin, int sub_stride) {
    extern __shared__ __attribute__((aligned(16))) uint4 lqx[];
    // MODE 1 as a second-chance round (fir_gemm_fb.h): `smin` is the list's length, `sub_stride` the part of it earlier rounds took --
    // nothing left for this round: every workgroup returns at once (a kernel boundary lies between the writers and this load)
    if (MODE == 1 && smin != nullptr && (int)smin[0] - sub_stride <= 0) return;
    const int nt = nt_flags & 1;
    static_assert(QH == 1 || (QH == 2 && MODE == 3 && !STREAMED && !ODD && NJB == 8 && I8 && !(DBG & 256)), "QH = 2: the int8 top-1 pass of two units only");
    constexpr int kTQ = 2 * kQT * QH;                // queries of the workgroup's tile
    constexpr int kStage = QH == 2 ? kXStage / 2 : kXStage;      // (256 queries: eight staged slots each, the same 16 KiB)
    constexpr int kHalfImg = 4 * kRing * 2 * 64;     // QH = 2: uint4 per 128-query image of 512 int8 features (64 KiB)
    __shared__ float tau_s[kTQ], qinv_s[kTQ];
    // MODE 1: appends are staged per workgroup in LDS (an LDS atomic counts in lgkmcnt and returns in ~100 cycles; a returning GLOBAL
    // atomic sits in the in-order vmcnt queue behind the prefetched gallery loads -- every append drained the wave's stream) and
    // flushed to the global lists once, at the end; a query that fills its kXStage slots appends directly (rare, correct)
    // MODE 4: MODE 3 for the K nearest rows (K = sub_stride, 2..8). Per query EIGHT slot minima over disjoint row sets -- slot i = the rows a
    // lane holds in position i of its eight (rows 16 (i >> 2) + 4 (lane >> 4) + (i & 3) of every row block): four rows of EVERY block feed
    // every slot, so a cluster of a few dozen near rows fills all eight at once (slots by row block left the slots of a class-ordered
    // training set to different classes: profiles/r04_knn_matrix_cores.txt) -- the K smallest slot minima belong to K distinct rows, so T = (the K-th smallest slot minimum + |q|^2) +
    // window bounds the K-th smallest proxy of all rows from above -- what the K-nearest re-rank's certificate needs (k_gemm_rerank<kTopKMax>:
    // window hung on the K-th smallest proxy of the list). Every slot only falls, so T only falls, and the MODE 3 argument carries over
    // word for word. The slots live in LDS (slot_s, as the float bits of (slot minimum + |q|^2) + window, >= 0) and in `smin` (8 words
    // per query), exchanged by the same atomics on the same schedule; the hot path still compares against one bound per query (tq_s / tqr).
    constexpr bool kAdapt = MODE == 3 || MODE == 4;
    constexpr bool kSlots = MODE == 4;
    const int kth = kSlots ? sub_stride : 1;
    // the K-th smallest of a query's eight slot words (rank by value, then slot: every word gets a distinct rank)
    auto kth_of_slots = [&](const unsigned int* sl) -> unsigned int {
        const uint4 lo = *(const uint4*)sl, hi = *(const uint4*)(sl + 4);          // (sl is 32-byte aligned: a query's eight words)
        const unsigned int v[8] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
        unsigned int res = 0xFFFFFFFFu;
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            int rank = 0;
#pragma unroll
            for (int j = 0; j < 8; ++j) rank += (v[j] < v[i] || (v[j] == v[i] && j < i)) ? 1 : 0;
            res = rank == kth - 1 ? v[i] : res;
        }
        return res;
    };
    constexpr bool kAppend = MODE == 1 || kAdapt;
    __shared__ unsigned long long skeys[kAppend ? kTQ * kStage : 1];
    __shared__ int scnt[kAppend ? kTQ : 1];
    __shared__ float qn_s[kAdapt ? kTQ : 1], win_s[kAdapt ? kTQ : 1];
    __shared__ __attribute__((aligned(16))) unsigned int slot_s[kSlots ? 2 * kQT * 8 : 8];
    // MODE 3: tq_s = T - |q|^2 as the hot path compares it, rewritten by whoever lowers T (tau_s holds T itself). A racing store may leave
    // the value of an OLDER (larger) T: harmless -- any T the pass ever held is >= the final one, so whatever fails the test against
    // it has a proxy >= fl(T_final - |q|^2), the bound the certificate is given
    __shared__ float tq_s[kAdapt ? kTQ : 1];
    // The shared form of the resident adaptive passes hands its row blocks out at run time (`next_blk`, below); everything else --
    // the streamed ring (a barrier per unit: every wave has to walk the same units), the sample pass (its subsets go by wave), MODE 1 --
    // keeps the static ownership. These forms know the shared form only (every caller launches them with share >= 1 and gridDim.y == 1,
    // where share <= 0 means the same as 1: it is taken as 1).
    constexpr bool kDynForm = !STREAMED && kAdapt;
    if (kDynForm && share <= 0) share = 1;
    __shared__ int next_blk;
    unsigned long long t_entry = 0;                   // (DBG & 256)
    if (DBG & 256) t_entry = __builtin_amdgcn_s_memtime();
    int pair_of_wg = (int)blockIdx.y;
    int64_t rg_first = blockIdx.x, rg_step = gridDim.x, rg_last = -1;
    int range = (int)blockIdx.x;
    if (share > 0) {
        const int w = (int)blockIdx.x, xcd = w & 7, slot = w >> 3;
        const int ranges = ((int)gridDim.x >> 3) / share * 8;
        range = xcd + 8 * (slot / share);
        if (range >= ranges) return;                                       // uniform per workgroup
        pair_of_wg = slot % share;
        const int64_t nrg_all = (((row_end + 31) / 32 - row_begin / 32) + (blockDim.x >> 6) - 1) / (blockDim.x >> 6);
        rg_first = nrg_all * range / ranges;
        rg_last = nrg_all * (range + 1) / ranges;
        rg_step = 1;
    }
    const int dk32 = dk16 >> 1;
    {
        const size_t pr = (size_t)pair_of_wg * QH;        // (QH = 2: the workgroup's tile is pairs 2 t and 2 t + 1, contiguous in every per-pair array)
        qh += pr * 8 * dk32 * 64;
        qinv += pr * 2 * kQT;
        tau += pr * 2 * kQT;
        lists += pr * 2 * kQT * kListCap;
        counts += pr * 2 * kQT;
        if (MODE == 2 || MODE == 3) smin += pr * 2 * kQT;
        if (MODE == 4) smin += pr * 2 * kQT * 8;
        if (kAdapt) qnorm += pr * 2 * kQT;
    }
    const int64_t rbs = MODE == 2 ? rb_stride : 1;                        // gallery row blocks per row block of the pass
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int wpb = blockDim.x >> 6;
    if (threadIdx.x < kTQ) {
        if (kSlots) {
            unsigned int v8[8];
#pragma unroll
            for (int sl = 0; sl < 8; ++sl) v8[sl] = atomicMin(&smin[threadIdx.x * 8 + sl], 0xFFFFFFFFu);
#pragma unroll
            for (int sl = 0; sl < 8; ++sl) slot_s[threadIdx.x * 8 + sl] = v8[sl];
            tau_s[threadIdx.x] = __uint_as_float(kth_of_slots(&slot_s[threadIdx.x * 8]));
        } else
        tau_s[threadIdx.x] = MODE == 1 ? tau[threadIdx.x] : MODE == 3 ? __uint_as_float(atomicMin(&smin[threadIdx.x], 0xFFFFFFFFu)) : 0.f;    // (MODE 3: an atomic, see the refresh below)
        qinv_s[threadIdx.x] = qinv[threadIdx.x];
        if (kAppend) scnt[threadIdx.x] = 0;
        if (kDynForm && threadIdx.x == 0) next_blk = wpb;          // (published by the barrier behind the tile's staging)
        if (kAdapt) {
            qn_s[threadIdx.x] = qnorm[threadIdx.x];
            win_s[threadIdx.x] = tau[threadIdx.x];
            tq_s[threadIdx.x] = tau_s[threadIdx.x] - qn_s[threadIdx.x];
        }
    }
    const int64_t rb_begin = row_begin / 32, rb_end = (row_end + 31) / 32;
    const int64_t nrg = (rb_end - rb_begin + wpb - 1) / wpb;
    // a unit of the few-block forms is SIXTEEN gallery pieces (eight steps): such a pass is one read of the fragments and nothing else, and
    // what it reads at is set by the bytes a wave keeps in flight -- 16 KiB instead of 8 (registers are not scarce with one or two
    // query blocks). Resident tiles only (the streamed ring's slots and its vmcnt(12) are sized for eight pieces).
    constexpr int RING = (!STREAMED && NJB < 8) ? 2 * kRing : kRing;
    const int units = dk16 / RING;
    int64_t rg_end = rg_last >= 0 ? rg_last : nrg;
    int64_t rg = rg_first;
    if (rg >= rg_end) return;                        // uniform per workgroup
    // Dynamic hand-out (the shared form of kDynForm): the two waves of a SIMD do not share the matrix pipe evenly -- the older one
    // walks at 1.4 times the pace of the younger (profiles/r04_wave_phases.txt) -- so with an equal share of the range's row blocks
    // each the older four were done while the younger four still had a quarter of theirs, and the workgroup ran one wave per SIMD,
    // with nobody to hide the deferred epilogue, to the end of every launch (profiles/top1_wave_balance.txt). The range's row blocks
    // are counted one by one here (`rg` is a row BLOCK, not a group of wpb); wave w starts with block w of the range -- every wave has
    // a first block, the warm-up rule and its barrier stay uniform -- and takes every further one from `next_blk`, in ascending order:
    // the workgroups that share the range still walk it together.
    const int64_t blk0 = rb_begin + rg_first * wpb;         // (kDynForm: `rg` is the row block of the pass itself)
    if (kDynForm) {
        rg = blk0 + wave;
        rg_end = rb_begin + rg_end * wpb;
    }
#define FIR_X_LD(P) (nt ? ld_nt(P) : *(P))
    // (wave-uniform block pointers: the lane index is added in the load itself, so that the loads take the scalar-base form --
    // one 32-bit lane offset register instead of a 64-bit address per pointer)
#define FIR_X_RBP(RG) (kDynForm ? (RG) : rb_begin + (RG) * wpb + wave)
#define FIR_X_BLOCK(RG) (gh + (size_t)((FIR_X_RBP(RG) < rb_end ? FIR_X_RBP(RG) : rb_end - 1) * rbs) * dk16 * 64)
    const uint4* a_cur = FIR_X_BLOCK(rg);
    uint4 cur[RING], nxt[RING];
#pragma unroll
    for (int u = 0; u < RING; ++u) cur[u] = FIR_X_LD(a_cur + (size_t)u * 64 + lane);
    constexpr int kUnitsPerSlab = kSlabH / RING;                         // units of the LDS-resident tile (512 features)
    // (the caller streams whatever does not fit: dk16 > kSlabH)
    // STREAMED (rows longer than the 512 features whose 128-query tile fits LDS): the query fragments go through a ring of FOUR
    // 32-KiB LDS slots of one unit (four steps x eight query blocks) each. Units are numbered c = 0, 1, 2, ... over the whole walk of
    // the workgroup (slab of unit c: c mod units); slot c & 3 holds unit c. The slab of unit c + 3 is requested DURING unit c -- this
    // wave's four one-KiB pieces by LDS-DMA, one behind each step's MFMAs (a request holds the issuing wave for 60-180 cycles: spread
    // out, the SIMD's other wave covers them) -- into the slot unit c - 1 was read from, which every wave left before the barrier
    // that ended unit c - 1. At the end of unit c every wave waits for its pieces of unit c + 2 (requested a whole unit earlier:
    // vmcnt(12) = this unit's eight gallery loads and four requests may stay in flight) and ONE barrier publishes them; so the
    // fragments of unit c + 1's first step, which the rolling re-read fetches during unit c's last step, were published one barrier
    // earlier, and the fragment pipeline runs on through unit borders as in the resident form -- the barrier no longer drains it.
    // The requests are inline assembly: the compiler orders every LDS read behind a pending LDS-DMA it knows about with
    // s_waitcnt vmcnt(0), and it cannot see that ring slots do not alias. Its own counted waits for the gallery loads stay
    // correct with requests it does not know in the queue: vmcnt(N) leaves the N YOUNGEST operations outstanding, whatever they are.
    const uint32_t lds_base = (uint32_t)(uintptr_t)(void __attribute__((address_space(3)))*)lqx;
    auto request_piece = [&](int hq, int slot, int i) {              // piece i of this wave: (step i, query block `wave`) of slab hq
        const uint4* src = qh + ((size_t)wave * dk32 + (size_t)hq * 4 + i) * 64 + lane;
        const uint32_t dst = __builtin_amdgcn_readfirstlane(lds_base + (uint32_t)slot * (4 * RING * 1024) + (uint32_t)(i * 8 + wave) * 1024);
        asm volatile("s_mov_b32 m0, %0\n\tglobal_load_lds_dwordx4 %1, off" ::"s"(dst), "v"(src) : "memory");
    };
    int ring_c = 0, hq3 = 0;                         // unit counter of the walk; slab index of unit ring_c + 3
    if (STREAMED) {
        int hq = 0;
        for (int cc = 0; cc < 3; ++cc) {             // units 0, 1, 2 before the walk starts
#pragma unroll
            for (int i = 0; i < 4; ++i) request_piece(hq, cc, i);
            hq = hq + 1 == units ? 0 : hq + 1;
        }
        hq3 = hq;
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");               // (also the prologue's gallery loads: once per kernel)
        __syncthreads();
    } else {
        // LDS image: step-major, the eight query blocks of a step side by side -- (kk * 8 + jb) * 1 KiB
        for (int i = threadIdx.x; i < NJB * dk32 * 64; i += blockDim.x) {                   // (the live query blocks: NJB of the tile's eight)
            const int jb = i / (dk32 * 64), r = i - jb * dk32 * 64;
            lqx[(size_t)((r >> 6) * 8 + jb) * 64 + (r & 63)] = qh[(size_t)jb * dk32 * 64 + r];
        }
        if (QH == 2) {                                                   // the second pair's image, in the same layout, behind the first's
            for (int i = threadIdx.x; i < NJB * dk32 * 64; i += blockDim.x) {
                const int jb = i / (dk32 * 64), r = i - jb * dk32 * 64;
                lqx[kHalfImg + (size_t)((r >> 6) * 8 + jb) * 64 + (r & 63)] = qh[(size_t)(8 + jb) * dk32 * 64 + r];
            }
        }
        __syncthreads();
    }
    float smallest[NJB];                             // MODE 2: running minima of this lane's NJB queries
#pragma unroll
    for (int j = 0; j < NJB; ++j) smallest[j] = __builtin_huge_valf();
    uint4 B[NJB];                                    // the fragments of the first step of the first unit (slot 0 / the resident tile's start)
#pragma unroll
    for (int j = 0; j < NJB; ++j) B[j] = lqx[lane + j * 64];
    // The append forms DEFER a full row block's epilogue into the next row block's first step: the first step's MFMAs start the sums
    // from a zero C operand, so query block j's sixteen sums stay readable until the two MFMAs of index j of that step overwrite
    // them -- the check of query block j (four v_max3, an fma, a compare; rarely the eight proxies and an append) sits right in
    // front of them and runs beside the MFMAs of the blocks before it, instead of leaving the matrix pipe to a partner wave that,
    // alone, waits for its own LDS reads (profiles/r03_gemm_time_decomposition.txt: the epilogue cost 0.18 of 1.56 ms).
    constexpr bool kDefer = kAppend && !(DBG & 1);
    using acc_t = typename std::conditional<I8 != 0, i32x4, f32x4>::type;
    acc_t acc[2][NJB];                               // (written by the MFMAs of a row block's first step, against a zero C operand)
    if (kDefer) {                                    // (a wave's first first step reads them, against p_gmin = +inf: see `pend`)
#pragma unroll
        for (int j = 0; j < NJB; ++j) acc[0][j] = acc[1][j] = acc_t{0, 0, 0, 0};
    }
    // `pend`: a full row block's checks are still owed. The first step does NOT test it: what it is given when nothing is owed -- a
    // wave's first row block, the block behind one that was not full -- is p_gmin = +inf, against which the check's lower bound is
    // +inf or NaN and below no bound at all, so the check of a query block is the same seven instructions either way and carries no
    // scalar test (the sums it then reads are zeros or a block's nobody needs). `pend` itself is read behind the row loop only.
    bool pend = false;
    int64_t p_rb = 0;
    float4 pg[2] = {};
    float p_gmin = __builtin_huge_valf();
    float m2r[kDefer ? NJB : 1], tqr[kDefer ? NJB : 1];  // per query block of this lane: 2 / scale, and the bound as of the last row block's end
    if (kDefer) {
#pragma unroll
        for (int jb = 0; jb < NJB; ++jb) {
            m2r[jb] = 2.0f * qinv_s[jb * 16 + (lane & 15)];
            tqr[jb] = kAdapt ? tq_s[jb * 16 + (lane & 15)] : tau_s[jb * 16 + (lane & 15)];
        }
    }
    bool warm = kAdapt;                              // MODE 3 / 4: the first row block's sums are looked at twice (below)
    // MODE 4: the K-th smallest slot value as the new T of query q (a value read a moment ago is >= the slot's current one, so this is a bound)
    auto slots_to_T = [&](int q) {
        const unsigned int tk = kth_of_slots(&slot_s[q * 8]);
        if (tk < atomicMin((unsigned int*)&tau_s[q], tk)) tq_s[q] = __uint_as_float(tk) - qn_s[q];
    };
    // a new smallest proxy `mn` (= the smallest of the lane's eight proxies pv) for query q: T falls, here and (through `smin`) for everybody else
    auto lower_T = [&](int q, const float (&pv)[8], float mn) {
        if (!kSlots) {
            const float tn = fmaxf((mn + qn_s[q]) + win_s[q], 0.f);
            if (tn < tau_s[q]) {
                if (__float_as_uint(tn) < atomicMin((unsigned int*)&tau_s[q], __float_as_uint(tn))) tq_s[q] = tn - qn_s[q];
                atomicMin(&smin[q], __float_as_uint(tn));
            }
        } else {
            // (the eight slot words in ONE round trip to the LDS, as two 16-byte reads: read one by one between the conditional atomics
            // they cost an append event eight round trips in a row. A slot another wave lowers in between is compared against its
            // older, larger value: one atomic more, the same minimum.)
            const uint4 s_lo = *(const uint4*)&slot_s[q * 8], s_hi = *(const uint4*)&slot_s[q * 8 + 4];
            const unsigned int have[8] = {s_lo.x, s_lo.y, s_lo.z, s_lo.w, s_hi.x, s_hi.y, s_hi.z, s_hi.w};
            const float qn = qn_s[q], win = win_s[q];
            bool fell = false;
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                const float tn = fmaxf((pv[i] + qn) + win, 0.f);        // (a NaN proxy: fmaxf(NaN, 0) = 0 -- kept out by the test on pv[i] itself)
                if (pv[i] == pv[i] && tn < __uint_as_float(have[i])) {
                    atomicMin(&slot_s[q * 8 + i], __float_as_uint(tn));
                    atomicMin(&smin[q * 8 + i], __float_as_uint(tn));
                    fell = true;
                }
            }
            if (fell) slots_to_T(q);
        }
    };
    // the workgroup's first-row-block minima go out, everybody else's come in (uniform over the workgroup: every wave's first row block
    // is its warm-up block)
    auto exchange_T = [&]() {
            // the workgroup's warm-up minima go out, everybody else's come in
        __syncthreads();
        if (threadIdx.x < kTQ) {
            if (kSlots) {
                unsigned int mine[8], old[8];
#pragma unroll
                for (int sl = 0; sl < 8; ++sl) mine[sl] = slot_s[threadIdx.x * 8 + sl];
#pragma unroll
                for (int sl = 0; sl < 8; ++sl) old[sl] = (nt_flags & 8) ? mine[sl] : atomicMin(&smin[threadIdx.x * 8 + sl], mine[sl]);
#pragma unroll
                for (int sl = 0; sl < 8; ++sl) slot_s[threadIdx.x * 8 + sl] = old[sl] < mine[sl] ? old[sl] : mine[sl];
                tau_s[threadIdx.x] = __uint_as_float(kth_of_slots(&slot_s[threadIdx.x * 8]));
            } else {
            const unsigned int mine = __float_as_uint(tau_s[threadIdx.x]);
            unsigned int zx = 0;                         // (QH = 2: the address is made here -- prepared in front of the row loop it was spilled)
            if (QH == 2) asm volatile("v_mov_b32 %0, 0" : "=v"(zx));
            const unsigned int old = (nt_flags & 8) ? mine : atomicMin(&smin[threadIdx.x + zx], mine);
            tau_s[threadIdx.x] = __uint_as_float(old < mine ? old : mine);
            }
            tq_s[threadIdx.x] = tau_s[threadIdx.x] - qn_s[threadIdx.x];
        }
        __syncthreads();
    };
    int blk_no = 0;
    int dbg_units = 0;                               // (DBG & 256: units walked so far)
    int64_t rg_next = rg;
    for (; rg < rg_end; rg = rg_next) {
        const bool warm_it = warm;                        // this wave's first row block: T is still what it was preset to
        warm = false;
        rg_next = rg + rg_step;
        // kDynForm, the block after this one: ONE lane asks here, a row block ahead of the burst that needs its address, and the answer
        // is taken where that burst is issued -- at the head of this block's last unit (`next_block`). Taken here it was waited for
        // here: an s_waitcnt lgkmcnt(0) at the head of every row block, i.e. behind the query fragments the last step had just
        // re-read for the first step. Three units later the answer has long landed.
        // (atomicInc, not atomicAdd: the compiler rewrites an add for a whole wave -- count the active lanes, one lane adds, the
        // result goes through v_readfirstlane right behind the atomic -- which puts the wait back here for an "optimisation" of one lane.
        // With a limit of 2^32 - 1 the increment is the add.)
        int tk = 0;
        // (QH = 2: a wave's warm-up walk only observes -- the same block is walked again, for real, so it takes no ticket)
        if (kDynForm && lane == 0 && !(QH == 2 && warm_it)) tk = (int)atomicInc((unsigned int*)&next_blk, 0xFFFFFFFFu);
        const int64_t rbp = FIR_X_RBP(rg);                // row block of the pass ...
        const int64_t rb = rbp * rbs;                     // ... and of the gallery
        const bool active = rbp < rb_end;
        const uint4* a_nxt = a_cur;                       // (the next block's fragments: set by next_block)
        auto next_block = [&]() {
            if (kDynForm) rg_next = (QH == 2 && warm_it) ? rg : blk0 + __builtin_amdgcn_readfirstlane(tk);
            const int64_t rgn = rg_next;
            a_nxt = FIR_X_BLOCK(rgn < rg_end ? rgn : rg);
        };
        if (!kDynForm) next_block();
        if (kAdapt) {
            if (!warm_it && wave < NJB && !(nt_flags & 4)) {
                // What the other workgroups have reached since. Only ATOMICS read `smin`: they execute at the memory side, so what they
                // return is the value every XCD's updates have been folded into -- a load, even an sc1 one, can be served by a line this
                // XCD's L2 took in earlier (measured: whole XCDs' workgroups never saw the others' bounds and appended 16 rows each per
                // query, 4 000+ per query with one pair over 256 row ranges). One returning atomicMin posts this wave's sixteen
                // queries' T and fetches the global one; its result is used at once (nothing is held across the row block -- at 256
                // registers that spills), on a schedule that thins out: row blocks 2, 3, 4, 6, 8, 12, 16, 24, ... (T settles early).
                const int v = blk_no >> __builtin_ctz((unsigned)blk_no | 0x40000000u);
                if ((v == 1 || v == 3) && lane < 16 * QH) {
                    int zl;                                   // (the lane index from the hardware, as in check_jb: keeps the addresses from being hoisted out of the row loop and spilled)
                    asm volatile("v_mbcnt_lo_u32_b32 %0, -1, 0\n\tv_mbcnt_hi_u32_b32 %0, -1, %0" : "=v"(zl));
                    const int ql = QH == 2 ? 128 * (zl >> 4) + 16 * wave + (zl & 15) : 16 * wave + zl;    // (QH = 2: the wave's query block of either half)
                    if (kSlots) {
                        // (all eight round trips in flight together: one after the other they cost a refresh eight memory latencies)
                        unsigned int mine[8], old[8];
#pragma unroll
                        for (int sl = 0; sl < 8; ++sl) mine[sl] = slot_s[ql * 8 + sl];
#pragma unroll
                        for (int sl = 0; sl < 8; ++sl) old[sl] = atomicMin(&smin[ql * 8 + sl], mine[sl]);
                        bool fell = false;
#pragma unroll
                        for (int sl = 0; sl < 8; ++sl)
                            if (old[sl] < mine[sl]) { atomicMin(&slot_s[ql * 8 + sl], old[sl]); fell = true; }
                        if (fell) slots_to_T(ql);
                    } else {
                    const unsigned int mine = __float_as_uint(tau_s[ql]);
                    const unsigned int old = atomicMin(&smin[ql], mine);
                    if (old < mine && old < atomicMin((unsigned int*)&tau_s[ql], old)) tq_s[ql] = __uint_as_float(old) - qn_s[ql];
                    }
                }
            }
            ++blk_no;
        }
        float4 gns[2];                               // squared norms of rows 16 s + 4 (lane >> 4) + 0..3 of the block
        // Where the block's last unit reads them from -- ALWAYS, whether the block is full or not (see `unit`), so the 32 floats have to
        // lie inside an allocation for every block a wave can walk: a straddling one, one past the end of the range, a sample block
        // (rb = rbp * rbs). `gnorm` holds exactly max(n, 1) floats -- nothing behind row n - 1 -- so it is the CLAMP that makes the
        // access safe, not the allocation: the window starts at min(32 rb, (n - 32) & ~3) (a multiple of four floats: the loads stay
        // 16-byte aligned), which is 32 rb itself for every full block (32 rb + 32 <= n). With fewer than 32 rows there is no such
        // window in `gnorm` at all (and no full block): the loads then read the head of the fp16 fragments, one row block = dk16 KiB
        // >= 8 KiB that every gallery has. The values are used under `full_block` only.
        const float* gn_blk = n >= 32 ? gnorm + (rb * 32 < ((n - 32) & ~(int64_t)3) ? rb * 32 : ((n - 32) & ~(int64_t)3)) : (const float*)gh;
        const bool full_block = active && rbp * 32 >= row_begin && rbp * 32 + 32 <= row_end && rb * 32 + 32 <= n;
        // MODE 2, sub_stride: eight positions x eight waves = kRtSubsets disjoint subsets of the sampled rows (below)
        unsigned int* smin_blk = MODE == 2 ? smin + (size_t)(wave & 7) * sub_stride : nullptr;       // (position 0's subset of this wave)
        // one query block of a full row block `rbq` against the bound (the append forms, not the warm-up walk); g0 / g1 / gminq = the
        // block's row norms and their minimum
        auto check_jb = [&](int jb, int64_t rbq, const float4 g0, const float4 g1, float gminq, int half = 0) {
            // (called by a first step only, i.e. under kDefer. The lane's scale and bound come from registers -- an LDS read here would wait,
            // in order, behind the query fragments just requested for the next step; a bound that is a row block old is a larger one: it
            // appends more, never less)
            const float m2 = m2r[jb];
            const float tq = tqr[jb];
            // with m2 > 0, fl(gmin - m2 amax) <= fl(gn_r - m2 acc_r) for every row r of the lane (gmin <= gn_r, amax >= acc_r, rounding is
            // monotone): `lb >= tq` proves that no row of the block is appended -- seven instructions instead of sixteen. NaN sums never
            // enter amax, as they never enter the minimum below. (v_max3_f32 by hand: fmaxf() on MFMA results quiets every operand first.)
            // Everything behind the test is the rare path: marked unlikely, so that it is laid out of line and the common path falls
            // through into the query block's MFMAs.
            float amax;
            if (I8) {                        // (the maximum on the integers, one conversion)
                int imax;
                asm("v_max3_i32 %0, %1, %2, %3\n\tv_max3_i32 %0, %0, %4, %5\n\tv_max3_i32 %0, %0, %6, %7\n\tv_max_i32 %0, %0, %8"
                    : "=&v"(imax)
                    : "v"(acc[0][jb][0]), "v"(acc[0][jb][1]), "v"(acc[0][jb][2]), "v"(acc[0][jb][3]), "v"(acc[1][jb][0]), "v"(acc[1][jb][1]),
                      "v"(acc[1][jb][2]), "v"(acc[1][jb][3]));
                amax = (float)imax;
            } else
            asm("v_max3_f32 %0, %1, %2, %3\n\tv_max3_f32 %0, %0, %4, %5\n\tv_max3_f32 %0, %0, %6, %7\n\tv_max_f32 %0, %0, %8"
                : "=&v"(amax)
                : "v"(acc[0][jb][0]), "v"(acc[0][jb][1]), "v"(acc[0][jb][2]), "v"(acc[0][jb][3]), "v"(acc[1][jb][0]), "v"(acc[1][jb][1]),
                  "v"(acc[1][jb][2]), "v"(acc[1][jb][3]));
            if (__builtin_expect(!(__builtin_fmaf(-m2, amax, gminq) < tq), 1)) return;
            const float gnv[8] = {g0.x, g0.y, g0.z, g0.w, g1.x, g1.y, g1.z, g1.w};
            float pv[8];
            float mn = __builtin_huge_valf();
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                pv[i] = __builtin_fmaf(-m2, (float)acc[i >> 2][jb][i & 3], gnv[i]);
                mn = fminf(mn, pv[i]);                                   // NaN never enters, like k_gemm_tau's ordering
            }
            if (mn < tq) {
                // The rare path works on its OWN copy of the query index, made here from the hardware's lane count: every address below
                // (scnt, skeys, the slots, the lists) is then computed where it is used. From `q` itself the compiler hoisted eight sets
                // of them out of the row loop, spilled them, and reloaded them here -- a scratch load and an s_waitcnt vmcnt(0) per
                // appended row, i.e. every append waited for the gallery prefetch in flight (~1.2 us per event:
                // profiles/r04_append_path.txt).
                int lz;                                               // the lane index, from the hardware: no register of the hot loop is read
                asm volatile("v_mbcnt_lo_u32_b32 %0, -1, 0\n\tv_mbcnt_hi_u32_b32 %0, -1, %0" : "=v"(lz));
                const int qr = half * 2 * kQT + jb * 16 + (lz & 15);
#pragma unroll
                for (int i = 0; i < 8; ++i) {
                    if (pv[i] < tq) {
                        const int64_t row = rbq * 32 + 16 * (i >> 2) + 4 * (lz >> 4) + (i & 3);
                        const unsigned long long key = fir::key_pack(pv[i], (uint32_t)row);
                        const int st = atomicAdd(&scnt[qr], 1);
                        if (st < kStage) {
                            skeys[qr * kStage + st] = key;
                        } else {
                            const int slot = atomicAdd(&counts[qr], 1);
                            if (slot < kListCap) lists[(size_t)qr * kListCap + slot] = key;
                            // the list is full: this query is uncertified whatever else happens (fir_gemm_fb.h gives it a second pass), so the
                            // workgroup stops appending for it -- a pass whose bound stays loose must not turn into millions of atomics on
                            // one counter (~11 ns each: a whole gallery's worth is 11 ms). The next lowering of T writes tq_s again.
                            else if (kAdapt) tq_s[qr] = -__builtin_huge_valf();
                        }
                    }
                }
                if (kAdapt) lower_T(qr, pv, mn);
            }
        };
        // QH = 2, between the halves of a row block (MODE 3 only), on half `half`'s sums as they stand in the accumulators:
        // observe_half -- a wave's warm-up walk: the smallest proxy of the block's 32 rows lowers T in LDS, nothing is appended (what the
        // one-half forms do behind their first row block, below);
        // straddle_half -- a block that straddles the end of the rows, row by row against the bound in LDS (as behind the units, below).
        auto observe_half = [&](int half) __attribute__((always_inline)) {
            int lw;                                              // (the lane index from the hardware, as in check_jb)
            asm volatile("v_mbcnt_lo_u32_b32 %0, -1, 0\n\tv_mbcnt_hi_u32_b32 %0, -1, %0" : "=v"(lw));
#pragma unroll
            for (int jb = 0; jb < NJB; ++jb) {
                const int q = half * 2 * kQT + jb * 16 + (lw & 15);
                const float m2 = 2.0f * qinv_s[q];
                const float gnv[8] = {gns[0].x, gns[0].y, gns[0].z, gns[0].w, gns[1].x, gns[1].y, gns[1].z, gns[1].w};
                float mn = __builtin_huge_valf();
#pragma unroll
                for (int i = 0; i < 8; ++i) mn = fminf(mn, __builtin_fmaf(-m2, (float)acc[i >> 2][jb][i & 3], gnv[i]));      // NaN never enters
                float o = __shfl_xor(mn, 16, 64);
                mn = o < mn ? o : mn;
                o = __shfl_xor(mn, 32, 64);
                mn = o < mn ? o : mn;
                const float tn = fmaxf((mn + qn_s[q]) + win_s[q], 0.f);
                if (lw < 16 && tn < tau_s[q]) atomicMin((unsigned int*)&tau_s[q], __float_as_uint(tn));
            }
        };
        auto straddle_half = [&](int half) __attribute__((always_inline)) {
            int ls;                                              // (the lane index from the hardware, as in check_jb)
            asm volatile("v_mbcnt_lo_u32_b32 %0, -1, 0\n\tv_mbcnt_hi_u32_b32 %0, -1, %0" : "=v"(ls));
#pragma unroll
            for (int jb = 0; jb < NJB; ++jb) {
                const int q = half * 2 * kQT + jb * 16 + (ls & 15);
                const float m2 = 2.0f * qinv_s[q];
                const float tq = tq_s[q];
#pragma unroll
                for (int i = 0; i < 8; ++i) {
                    const int64_t row = rb * 32 + 16 * (i >> 2) + 4 * (ls >> 4) + (i & 3);
                    if (row >= n || row < row_begin || row >= row_end) continue;
                    const float p = __builtin_fmaf(-m2, (float)acc[i >> 2][jb][i & 3], gnorm[row]);
                    if (p < tq) {
                        const int slot = atomicAdd(&counts[q], 1);
                        if (slot < kListCap) lists[(size_t)q * kListCap + slot] = fir::key_pack(p, (uint32_t)row);
                    }
                }
            }
        };
        // RULE of the row loop: on its common path there must be no vector-memory operation that some other path into the same unit
        // head lacks. The compiler's wait at a unit head -- "all but the N youngest vector-memory operations have returned" -- has to
        // hold on every path that joins there, so it takes the smallest N of them; an operation that only SOME paths issue behind a burst
        // makes the head's wait, on the paths that have it, reach into the burst issued a few instructions earlier: a whole memory round
        // trip with nothing to wait for. (The row norms used to be loaded under `h == units - 1 && full_block`: once per row block every
        // wave stood still for it -- profiles/top1_last_unit.txt.) Hence the last unit is a compile-time place (`last_tag`; the unit
        // sequences below peel it) and loads the norms unconditionally.
        // QH = 2 (the 256-query tile of the int8 pass): the block's two units are walked once per tile half, half 0 (queries 0..127 of the
        // tile: the first image in LDS) then half 1, into the same accumulators -- four units h0.U0, h0.U1, h1.U0, h1.U1 per gallery
        // fragment read. `first_tag` then says "U0 of a half" (its first step starts the half's sums and checks the sums before them: half
        // 1's of the previous block in h0.U0, half 0's of THIS block in h1.U0), `last_tag` marks h1.U1 alone. Bursts: h0.U0 requests U1,
        // h1.U1 the next block's U0; h0.U1 loads the block's norms (h1.U0 needs them already; at h0.U0 they would be in flight while
        // the previous block's, in pg, are still being checked against: eight registers more) and h1.U0 requests nothing, so
        // every burst is still one unit ahead of its use. The bounds (and scales) of the half whose sums are checked next are read from
        // LDS in front of the unit before (the row loop does that, not `unit`): half 0's before h0.U1, half 1's before h1.U1 -- sixteen
        // registers, as with one half.
        auto unit = [&](uint4 (&C)[RING], uint4 (&N)[RING], int h, auto first_tag, auto last_tag, auto half_tag) {
            constexpr bool kFirst = decltype(first_tag)::value;      // the first unit of the row block: its first step starts the sums
            constexpr bool kLast = decltype(last_tag)::value;        // the last one: its burst is the next row block's first unit, the norms follow it
            constexpr int kHalf = decltype(half_tag)::value;         // QH = 2: the tile half this unit multiplies against
            constexpr bool kBurst = QH == 1 || (kHalf == 0 ? kFirst : kLast);
            constexpr bool kNorms = QH == 1 ? kLast : (kHalf == 0 && !kFirst);
            if (QH == 1 && kLast && !kFirst && kDefer && kAdapt) {
                // The bounds the NEXT row block's first step checks this block's sums against, read a unit early: in front of this unit's
                // fragment re-reads, so that the first deferred check finds them landed instead of draining the rolling re-reads to get
                // at the last LDS operations in front of it. A bound that is one unit older is a larger one (T only ever falls): it
                // appends more, never less, and what is not appended still has a proxy >= fl(T_final - |q|^2). (A one-unit row block
                // checks against these registers in this very unit: it refreshes them behind its steps, below. A wave's warm-up block
                // reads them again behind the exchange: what stands in tq_s before it is the preset.)
#pragma unroll
                for (int jb = 0; jb < NJB; ++jb) tqr[jb] = tq_s[jb * 16 + (lane & 15)];
            }
            if (kLast && kDynForm) next_block();
            const uint4* src = kLast ? a_nxt : a_cur + (size_t)(h + 1) * RING * 64;
            // QH = 2: this lane's address in the image of tile half `half`, as ONE 32-bit LDS address the compiler cannot see through: every
            // fragment of the half is then that register plus an immediate offset (< 64 KiB). From `lqx + constant` it built the second
            // image's addresses -- all beyond the 16-bit offset field -- as sixteen registers of their own, some of them inside the loop.
            auto image_of_half = [&](int half) __attribute__((always_inline)) -> const uint4* {
                uint32_t o = (uint32_t)(uintptr_t)(void __attribute__((address_space(3)))*)lqx + (uint32_t)(half * kHalfImg + lane) * 16u;
                asm volatile("" : "+v"(o));
#if defined(__HIP_DEVICE_COMPILE__)
                return (const uint4*)(const uint4 __attribute__((address_space(3)))*)o;
#else
                return lqx + o;                              // (the host pass only parses this: its pointers are not 32 bits wide)
#endif
            };
            const uint4* bq = STREAMED ? lqx + lane + (size_t)(ring_c & 3) * 4 * RING * 64
                              : QH == 2 ? image_of_half(kHalf) + (size_t)(h % kUnitsPerSlab) * RING * 4 * 64
                                       : lqx + lane + (size_t)(h % kUnitsPerSlab) * RING * 4 * 64;
            // The next unit's gallery pieces are requested in one burst in front of the unit (two per step measured 5-6 % slower:
            // profiles/r03_gemm_time_decomposition.txt).
            unsigned long long t_burst0 = 0;
            if (DBG & 256) t_burst0 = __builtin_amdgcn_s_memtime();
            if (kBurst && !(DBG & 2)) {
                if (nt) {
#pragma unroll
                    for (int u = 0; u < RING; ++u) N[u] = ld_nt(src + (size_t)u * 64 + lane);
                } else {
#pragma unroll
                    for (int u = 0; u < RING; ++u) N[u] = src[(size_t)u * 64 + lane];
                }
            }
            if (DBG & 256) {
                // (timing probe, audit build: when this wave started issuing the unit's eight loads and when the last of them had been issued --
                // s_memtime is a scalar instruction: it issues in order behind them -- for the first 240 units of workgroup 0's waves, kept in the
                // unused tail of the pair's last candidate list: profiles/r04_wave_phases.txt)
                const unsigned long long t_burst1 = __builtin_amdgcn_s_memtime();
                if (blockIdx.x == 0 && dbg_units < 240 && lane == 0) {
                    unsigned long long* dst = lists + (size_t)(2 * kQT - 1) * kListCap + 2048 + (size_t)wave * 256;
                    dst[dbg_units] = (t_burst0 << 20) | ((t_burst1 - t_burst0) & 0xFFFFFull);
                }
                ++dbg_units;
            }
            if (kNorms) {
                // the block's row norms, directly behind the burst and on every path (the rule above; gn_blk is always readable)
                // (wave-uniform base + a lane offset made here: hoisted out of the row loop, `gnorm + 4 (lane >> 4)` is a 64-bit register
                // pair per lane that the K-nearest form spilled -- a scratch reload and an s_waitcnt vmcnt(0) in every row block)
                unsigned int zl;
                asm volatile("v_mov_b32 %0, 0" : "=v"(zl));
                const float* gb = gn_blk;
                const unsigned int off = 4u * ((unsigned int)lane >> 4) + zl;
                gns[0] = *(const float4*)(gb + off);
                gns[1] = *(const float4*)(gb + off + 16);
            }
            // the unit's vector-memory operations stay in front of its steps: sunk behind the first MFMAs, a burst leaves the unit head's
            // wait with nothing younger than the data it waits for, and the exact count for that is "everything"
            __builtin_amdgcn_sched_barrier(0);
            // (QH = 2: behind U0 the half's U1, behind U1 the other half's U0)
            const uint4* bq_after = STREAMED ? lqx + lane + (size_t)((ring_c + 1) & 3) * 4 * RING * 64
                                    : QH == 2 ? (kFirst ? image_of_half(kHalf) + (size_t)RING * 4 * 64 : image_of_half(kHalf ^ 1))
                                             : lqx + lane + (size_t)((kLast ? 0 : h + 1) % kUnitsPerSlab) * RING * 4 * 64;
#pragma unroll
            for (int t = 0; t < RING / 2; ++t) {
                const uint4* bn = t + 1 < RING / 2 ? bq + (size_t)(t + 1) * 8 * 64 : bq_after;
                const f16x8 a0 = as_f16x8(C[2 * t]), a1 = as_f16x8(C[2 * t + 1]);
#pragma unroll
                for (int j = 0; j < NJB; ++j) {
                    if (kDefer && kFirst && t == 0) {
                        // (QH = 2: h0.U0 checks half 1's sums of the previous block, h1.U0 half 0's of this one -- both as p_rb / pg / p_gmin name them)
                        check_jb(j, p_rb, pg[0], pg[1], p_gmin, QH == 2 ? kHalf ^ 1 : 0);      // the previous row block's sums of query block j, about to be overwritten (nothing owed: p_gmin = +inf)
                    }
                    const f16x8 b = as_f16x8(B[j]);
                    const acc_t zero = {0, 0, 0, 0};
                    if (!(DBG & 32)) {
                        acc[0][j] = mfma_x_(a0, b, kFirst && t == 0 ? zero : acc[0][j]);
                        acc[1][j] = mfma_x_(a1, b, kFirst && t == 0 ? zero : acc[1][j]);
                    } else {                                      // (DBG & 32: no MFMAs -- the operands are only kept alive: what the two streams cost by themselves)
                        asm volatile("" ::"v"(a0), "v"(a1), "v"(b));
                        if (kFirst && t == 0) { acc[0][j] = zero; acc[1][j] = zero; }
                    }
                    if (!(DBG & 4)) B[j] = bn[j * 64];
                    __builtin_amdgcn_sched_barrier(0);            // the re-read stays right behind its fragment's last use
                }
                if (STREAMED) request_piece(hq3, (ring_c + 3) & 3, t);      // unit ring_c + 3's slab, into the slot unit ring_c - 1 has left
            }
            if (STREAMED) {
                // vmcnt(12): all but the twelve youngest vector-memory operations have returned. Younger than this wave's pieces of unit
                // ring_c + 2 (requested during the unit before this one) are this unit's eight gallery loads and four requests -- twelve --
                // and, in a row block's last unit, the two norm loads behind the burst: fourteen. The count is the same 12 there: the pieces
                // are older than all fourteen, so they have landed a fortiori, and what the wait asks for beyond them is the first two
                // loads of a burst issued a whole unit (64 MFMAs) earlier. (12 there on purpose, not the exact 14: one instruction text for
                // every unit of the ring, and a wait that asks for loads a unit old costs nothing that has been measured; vmcnt(14) in the
                // last unit was not measured.)
                asm volatile("s_waitcnt vmcnt(12)" ::: "memory");          // this wave's pieces of unit ring_c + 2 have landed ...
                __builtin_amdgcn_s_barrier();                               // ... and everyone's: published
                ++ring_c;
                hq3 = hq3 + 1 == units ? 0 : hq3 + 1;
            }
            if (kLast && kFirst && kDefer && kAdapt) {                      // (a one-unit row block: see the unit's head)
#pragma unroll
                for (int jb = 0; jb < NJB; ++jb) tqr[jb] = tq_s[jb * 16 + (lane & 15)];
            }
            if (kFirst) {                                                   // the checks are done: nothing is owed until this block's end says so
                pend = false;
                p_gmin = __builtin_huge_valf();
            }
        };
        // first unit, the middle units two by two, the peeled last unit (an even number of units: at least two, no middle with two; an odd
        // number: three or more have the one middle unit that pairs up with nothing in front of the last; ODD = 2: the one unit is both)
        const std::true_type yes;
        const std::false_type no;
        const std::integral_constant<int, 0> h0;
        const std::integral_constant<int, 1> h1;
        float gmin_blk = 0.f;                        // QH = 2: the smallest row norm of this block
        if (QH == 2) {
            // the bounds and scales of tile half `half`, read from LDS a unit ahead of the first step that checks against them
            auto bounds_of_half = [&](int half) __attribute__((always_inline)) {
                if (!kDefer) return;
#pragma unroll
                for (int jb = 0; jb < NJB; ++jb) {
                    tqr[jb] = tq_s[half * 2 * kQT + jb * 16 + (lane & 15)];
                    m2r[jb] = 2.0f * qinv_s[half * 2 * kQT + jb * 16 + (lane & 15)];
                }
            };
            unit(cur, nxt, 0, yes, no, h0);                  // burst nxt <- U1
            bounds_of_half(0);
            unit(nxt, cur, 1, no, no, h0);                   // the block's norms (no burst: cur keeps U0)
            // Between the halves: half 0's sums are complete and h1.U0's first step overwrites them. A full block's are checked there,
            // beside the MFMAs, as a deferred check like any other (p_rb / pg / p_gmin); a warm-up walk only lowers T with them (nothing
            // is checked: +inf); a block that straddles the end of the rows is taken row by row here. Nothing a unit needs is in flight
            // at this point -- the last burst is two units old -- so the rare paths' memory operations tighten no wait of the common path.
            gmin_blk = fminf(fminf(fminf(gns[0].x, gns[0].y), fminf(gns[0].z, gns[0].w)), fminf(fminf(gns[1].x, gns[1].y), fminf(gns[1].z, gns[1].w)));
            p_rb = rb;
            pg[0] = gns[0];
            pg[1] = gns[1];
            p_gmin = (full_block && !warm_it) ? gmin_blk : __builtin_huge_valf();
            if (DBG & 1) {                                   // (no epilogue: half 0's sums are only kept alive, as half 1's are behind the units)
#pragma unroll
                for (int jb = 0; jb < NJB; ++jb) asm volatile("" ::"v"(acc[0][jb]), "v"(acc[1][jb]));
                if (DBG & 4) {                               // (no re-reads: half 1 multiplies against the same registers -- made opaque, or its MFMAs are half 0's and go)
#pragma unroll
                    for (int jb = 0; jb < NJB; ++jb) asm volatile("" : "+v"(B[jb].x));
                }
            } else {
                if (__builtin_expect(warm_it, 0)) { if (full_block) observe_half(0); }
                else if (__builtin_expect(active && !full_block, 0)) straddle_half(0);
            }
            unit(cur, nxt, 0, yes, no, h1);                  // (no burst)
            bounds_of_half(1);
            unit(nxt, cur, 1, no, yes, h1);                  // the ticket; burst cur <- the next block's U0
        } else
        if (!ODD) {
            unit(cur, nxt, 0, yes, no, h0);
            for (int h = 1; h + 1 < units; h += 2) {
                unit(nxt, cur, h, no, no, h0);
                unit(cur, nxt, h + 1, no, no, h0);
            }
            unit(nxt, cur, units - 1, no, yes, h0);
        } else {
            if (ODD == 2) {
                unit(cur, nxt, 0, yes, yes, h0);
            } else {
                unit(cur, nxt, 0, yes, no, h0);
                for (int h = 1; h + 2 < units; h += 2) {
                    unit(nxt, cur, h, no, no, h0);
                    unit(cur, nxt, h + 1, no, no, h0);
                }
                unit(nxt, cur, units - 2, no, no, h0);
                unit(cur, nxt, units - 1, no, yes, h0);
            }
#pragma unroll
            for (int u = 0; u < RING; ++u) cur[u] = nxt[u];         // an odd number of units: the next row block's first unit sits in nxt
        }
        a_cur = a_nxt;
        // (The rule of `unit` once more: the norms are used under `full_block` only; behind a block that is not full they would still be
        // on their way when the next last unit loads into the same registers, and the wait for that would sit between its burst and its
        // norm loads -- in the one-unit form it waited for the burst just issued. Used here on the paths that do not use them below,
        // where the common path waits for them anyway -- under the condition, so that the wait stays out of the last unit's block. The
        // one-unit form needs it on every path: there the compiler kept the wait between burst and norm loads otherwise, and the norms
        // of a block whose only unit has just ended are waited for right here in any case.)
        if (ODD == 2 || !full_block) asm volatile("" ::"v"(gns[0].x), "v"(gns[0].y), "v"(gns[0].z), "v"(gns[0].w), "v"(gns[1].x), "v"(gns[1].y), "v"(gns[1].z), "v"(gns[1].w));
        if (DBG & 1) {                   // (no epilogue: the sums are only kept alive)
#pragma unroll
            for (int jb = 0; jb < NJB; ++jb) asm volatile("" ::"v"(acc[0][jb]), "v"(acc[1][jb]));
            continue;
        }
        if (kAdapt && warm_it) {
            // This wave's first row block, T still at its preset: the sums are looked at twice. First only to lower T (LDS) -- then the
            // workgroup exchanges with `smin` -- then, still in their registers, for the block's checks like any other block's.
            if (active && full_block) {
                int lw;                                          // (the lane index from the hardware, as in check_jb: nothing of this once-per-wave path is prepared in front of the row loop)
                asm volatile("v_mbcnt_lo_u32_b32 %0, -1, 0\n\tv_mbcnt_hi_u32_b32 %0, -1, %0" : "=v"(lw));
#pragma unroll
                for (int jb = 0; jb < NJB; ++jb) {
                    const int q = (QH - 1) * 2 * kQT + jb * 16 + (lw & 15);          // (QH = 2: half 1's sums; half 0's were observed between the halves)
                    const float m2 = 2.0f * qinv_s[q];
                    float pv[8];
                    float mn = __builtin_huge_valf();
#pragma unroll
                    for (int s = 0; s < 2; ++s) {
                        const float gnv[4] = {gns[s].x, gns[s].y, gns[s].z, gns[s].w};
#pragma unroll
                        for (int reg = 0; reg < 4; ++reg) {
                            pv[4 * s + reg] = __builtin_fmaf(-m2, (float)acc[s][jb][reg], gnv[reg]);
                            mn = fminf(mn, pv[4 * s + reg]);                   // NaN never enters, like k_gemm_tau's ordering
                        }
                    }
                    if (kSlots) {
                        // every lane's eight proxies lower their slots (LDS; the exchange turns the slots into T)
#pragma unroll
                        for (int i = 0; i < 8; ++i) {
                            const float tn = fmaxf((pv[i] + qn_s[q]) + win_s[q], 0.f);
                            if (pv[i] == pv[i] && tn < __uint_as_float(slot_s[q * 8 + i])) atomicMin(&slot_s[q * 8 + i], __float_as_uint(tn));
                        }
                    } else {
                        // the smallest proxy of the block's 32 rows lowers T (LDS)
                        float o = __shfl_xor(mn, 16, 64);
                        mn = o < mn ? o : mn;
                        o = __shfl_xor(mn, 32, 64);
                        mn = o < mn ? o : mn;
                        const float tn = fmaxf((mn + qn_s[q]) + win_s[q], 0.f);     // (NaN operands: fmaxf gives 0 only if both are NaN; a NaN tn fails the test below)
                        if (lw < 16 && tn < tau_s[q]) atomicMin((unsigned int*)&tau_s[q], __float_as_uint(tn));
                    }
                }
            }
            exchange_T();
            // QH = 2: half 0's sums are gone, so the walk above only observed -- both halves' queries now hold an exchanged T, and the same
            // block comes again (next_block), for real. No other block is walked twice.
            if (QH == 2) continue;
            if (kDefer) {                                                    // (the last unit read the preset: the exchanged bounds)
#pragma unroll
                for (int jb = 0; jb < NJB; ++jb) tqr[jb] = tq_s[jb * 16 + (lane & 15)];
                // (used here, so waited for here, once per wave -- not by every row block's first check: see the straddling block below)
#pragma unroll
                for (int jb = 0; jb < NJB; ++jb) asm volatile("" ::"v"(tqr[jb]));
            }
        }
        if (!active) continue;
        if (full_block) {
            const float gmin = QH == 2 ? gmin_blk : fminf(fminf(fminf(gns[0].x, gns[0].y), fminf(gns[0].z, gns[0].w)), fminf(fminf(gns[1].x, gns[1].y), fminf(gns[1].z, gns[1].w)));
            if (kAppend) {                                                   // (= kDefer here: the form without epilogue has left the loop body)
                pend = true;                                                 // checked in the next row block's first step (or behind the loop)
                p_rb = rb;                                                   // (against tqr, which the last unit refreshed)
                pg[0] = gns[0];
                pg[1] = gns[1];
                p_gmin = gmin;
                continue;
            }
#pragma unroll
            for (int jb = 0; jb < NJB; ++jb) {
                const int q = jb * 16 + (lane & 15);
                const float m2 = 2.0f * qinv_s[q];
                float pv[8];
                float mn = __builtin_huge_valf();
#pragma unroll
                for (int s = 0; s < 2; ++s) {
                    const float gnv[4] = {gns[s].x, gns[s].y, gns[s].z, gns[s].w};
#pragma unroll
                    for (int reg = 0; reg < 4; ++reg) {
                        pv[4 * s + reg] = __builtin_fmaf(-m2, (float)acc[s][jb][reg], gnv[reg]);
                        mn = fminf(mn, pv[4 * s + reg]);                   // NaN never enters, like k_gemm_tau's ordering
                    }
                }
                if (!sub_stride) {                                           // (MODE 2: every other mode appends and has left above)
                    smallest[jb] = fminf(smallest[jb], mn);
                } else {
                    // the K-nearest sample: kRtSubsets = 8 positions (of a lane's eight rows) x 8 waves disjoint subsets -- every sampled row
                    // block feeds eight of them (a class of a few dozen rows then shows in eight subsets, not in one)
#pragma unroll
                    for (int i = 0; i < 8; ++i) {
                        float v = pv[i] == pv[i] ? pv[i] : __builtin_huge_valf();
                        float o = __shfl_xor(v, 16, 64);
                        v = o < v ? o : v;
                        o = __shfl_xor(v, 32, 64);
                        v = o < v ? o : v;
                        if (lane < 16 && v < __builtin_huge_valf()) atomicMin(&smin[(size_t)(i * 8 + (wave & 7)) * sub_stride + q], fir::f32_orderable(v));
                    }
                }
            }
            continue;
        }
        // a block that straddles the end of the rows: row by row
        int ls;
        // (the lane index from the hardware, as in check_jb -- from `lane` the compiler built this path's eight list addresses in front
        // of the row loop and spilled them)
        asm volatile("v_mbcnt_lo_u32_b32 %0, -1, 0\n\tv_mbcnt_hi_u32_b32 %0, -1, %0" : "=v"(ls));
#pragma unroll
        for (int jb = 0; jb < NJB; ++jb) {
            const int q = (QH - 1) * 2 * kQT + jb * 16 + (ls & 15);                  // (QH = 2: half 1's sums; half 0's were taken between the halves)
            const float m2 = 2.0f * qinv_s[q];
            const float tq = kAdapt ? tq_s[q] : tau_s[q];
            float mn = __builtin_huge_valf();
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                const int64_t row = rb * 32 + 16 * (i >> 2) + 4 * (ls >> 4) + (i & 3);
                if (row >= n || (MODE != 2 && (row < row_begin || row >= row_end))) continue;
                const float p = __builtin_fmaf(-m2, (float)acc[i >> 2][jb][i & 3], gnorm[row]);
                if (MODE == 2) {
                    mn = p < mn ? p : mn;
                } else if (p < tq) {
                    const int slot = atomicAdd(&counts[q], 1);
                    if (slot < kListCap) lists[(size_t)q * kListCap + slot] = fir::key_pack(p, (uint32_t)row);
                }
            }
            // (The rule of `unit`, for LDS: the bound is looked at under `p < tq` only; where no row of the lane gets that far, its read
            // would still be on its way at the row loop's head, and the compiler would have the COMMON path wait for every LDS
            // operation there -- the fragments just re-read for the first step -- before it reuses the register. Used here, it is
            // waited for here.)
            asm volatile("" ::"v"(tq), "v"(m2));
            if (MODE == 2 && !sub_stride) {
                smallest[jb] = fminf(smallest[jb], mn);
            } else if (MODE == 2) {
                float o = __shfl_xor(mn, 16, 64);
                mn = o < mn ? o : mn;
                o = __shfl_xor(mn, 32, 64);
                mn = o < mn ? o : mn;
                if (lane < 16 && mn < __builtin_huge_valf()) atomicMin(&smin_blk[q], fir::f32_orderable(mn));     // (a straddling block: one subset takes its minimum)
            }
        }
    }
    if ((DBG & 256) && blockIdx.x == 0 && lane == 0) {
        // (the end of the wave's walk: units walked, the kernel's entry and now -- slots 240.. of the wave's 256)
        unsigned long long* dst = lists + (size_t)(2 * kQT - 1) * kListCap + 2048 + (size_t)wave * 256;
        dst[240] = (unsigned long long)dbg_units;
        dst[241] = t_entry;
        dst[242] = __builtin_amdgcn_s_memtime();
    }
    if (kDefer && pend) {
        // the last full row block of this wave (no first step followed it); check_jb is the row loop's lambda -- the same code, here
        // against the values the loop left behind
        int lt;                                          // (the lane index from the hardware: the tail's addresses are not held across the row loop)
        asm volatile("v_mbcnt_lo_u32_b32 %0, -1, 0\n\tv_mbcnt_hi_u32_b32 %0, -1, %0" : "=v"(lt));
        auto last_jb = [&](int jb) {
            const int q = (QH - 1) * 2 * kQT + jb * 16 + (lt & 15);                  // (QH = 2: half 1's sums; half 0's were checked in h1.U0)
            const float m2 = 2.0f * qinv_s[q];
            const float tq = kAdapt ? tq_s[q] : tau_s[q];
            const float gnv[8] = {pg[0].x, pg[0].y, pg[0].z, pg[0].w, pg[1].x, pg[1].y, pg[1].z, pg[1].w};
            float pv[8];
            float mn = __builtin_huge_valf();
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                pv[i] = __builtin_fmaf(-m2, (float)acc[i >> 2][jb][i & 3], gnv[i]);
                mn = fminf(mn, pv[i]);
            }
            if (mn < tq) {
#pragma unroll
                for (int i = 0; i < 8; ++i) {
                    if (pv[i] < tq) {
                        const int64_t row = p_rb * 32 + 16 * (i >> 2) + 4 * (lt >> 4) + (i & 3);
                        const unsigned long long key = fir::key_pack(pv[i], (uint32_t)row);
                        const int st = atomicAdd(&scnt[q], 1);
                        if (st < kStage) {
                            skeys[q * kStage + st] = key;
                        } else {
                            const int slot = atomicAdd(&counts[q], 1);
                            if (slot < kListCap) lists[(size_t)q * kListCap + slot] = key;
                        }
                    }
                }
                if (kAdapt) lower_T(q, pv, mn);
            }
        };
#pragma unroll
        for (int jb = 0; jb < NJB; ++jb) last_jb(jb);
    }
    if (kAppend) {
        __syncthreads();                             // every wave's staged appends are in
        if (threadIdx.x < kTQ) {
            const int q = threadIdx.x;
            const int cnt = scnt[q] < kStage ? scnt[q] : kStage;
            if (cnt > 0) {
                const int base = atomicAdd(&counts[q], cnt);
                for (int st = 0; st < cnt; ++st)
                    if (base + st < kListCap) lists[(size_t)q * kListCap + base + st] = skeys[q * kStage + st];
            }
        }
    }
    if ((DBG & 256) && blockIdx.x == 0 && lane == 0)      // (... and the workgroup's end: behind the flush of the staged appends)
        lists[(size_t)(2 * kQT - 1) * kListCap + 2048 + (size_t)wave * 256 + 243] = __builtin_amdgcn_s_memtime();
    if (MODE == 2 && !sub_stride) {
#pragma unroll
        for (int jb = 0; jb < NJB; ++jb) {
            float v = smallest[jb];
            v = fminf(v, __shfl_xor(v, 16, 64));
            v = fminf(v, __shfl_xor(v, 32, 64));
            if (lane < 16 && v < __builtin_huge_valf()) atomicMin(&smin[jb * 16 + lane], fir::f32_orderable(v));
        }
    }
#undef FIR_X_BLOCK
#undef FIR_X_RBP
#undef FIR_X_LD
}

// tau for the smallest-proxy sample flow (MODE 2 above is its sample pass): the smallest SAMPLED proxy plus one rounding window (2.5 E d, as k_gemm_rerank's 2 E d
// with room). Every row that can still be the nearest has a proxy within 2 E d of the smallest proxy of ALL rows, which is
// not above the smallest sampled one: it is appended. And the certificate holds for the rest with room to spare: a row
// that was not appended has p >= tau, i.e. a reference distance >= (|q|^2 + p_s + 2.5 E d)/d - E, while the winner's is
// <= (|q|^2 + p_s)/d + E. About n / sample_rows + (rows inside the window) rows pass per query -- tens, not hundreds, which
// is what keeps the append path out of the full pass's way.
constexpr int kRtSubsets = 64;
// Top-K form of k_gemm_tau_min: the sample arrives as kRtSubsets disjoint subsets' minima per query; K of them are at or below the
// K-th smallest of these minima, so at least K rows of the gallery are: tau = that + one window appends every row that can be
// among the K nearest, and leaves room for the certificate of rank K. (With K << kRtSubsets the K smallest sampled proxies sit
// in different subsets almost always: the bound is within a rank or two of the K-th smallest of the whole sample.)
__global__ void __launch_bounds__(256) k_gemm_tau_kmin(const unsigned int* __restrict__ smin, int sub_stride, int k, float* __restrict__ tau,
                                                        int nq_total, int nq_valid, const float* __restrict__ qnorm,
                                                        const float* __restrict__ gnorm_max_p, float e_rel) {
    const int q = blockIdx.x * 256 + threadIdx.x;
    if (q >= nq_total) return;
    if (q >= nq_valid) { tau[q] = -__builtin_huge_valf(); return; }
    unsigned int best[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) best[i] = 0xFFFFFFFFu;
    for (int s = 0; s < kRtSubsets; ++s) {
        unsigned int v = smin[(size_t)s * sub_stride + q];
        if (v == 0xFF800000u) continue;                                    // an empty subset (+inf preset)
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const bool sw = v < best[i];
            const unsigned int t = best[i];
            best[i] = sw ? v : t;
            v = sw ? t : v;
        }
    }
    unsigned int kth = 0xFFFFFFFFu;
#pragma unroll
    for (int i = 0; i < 8; ++i) kth = i == k - 1 ? best[i] : kth;
    float t = __builtin_huge_valf();                                      // fewer than K sampled subsets: everything passes, the list cap decides
    if (kth != 0xFFFFFFFFu) {
        const float v = fir::f32_from_orderable(kth) + rounding_window_(e_rel, qnorm[q], gnorm_max_p[0]);
        t = nudge_up_(v);
    }
    tau[q] = t;
}

__global__ void __launch_bounds__(256) k_gemm_tau_min(const unsigned int* __restrict__ smin, float* __restrict__ tau, int nq_total, int nq_valid,
                                                       const float* __restrict__ qnorm, const float* __restrict__ gnorm_max_p, float e_rel) {
    const int q = blockIdx.x * 256 + threadIdx.x;
    if (q >= nq_total) return;
    if (q >= nq_valid) { tau[q] = -__builtin_huge_valf(); return; }       // padding queries of a half-filled pair: nothing is appended
    const unsigned int o = smin[q];
    float t = __builtin_huge_valf();                                      // no sampled proxy (NaN operands): everything passes, the list cap decides
    if (o != 0xFF800000u) {
        const float v1 = fir::f32_from_orderable(o);
        const float v = v1 + rounding_window_(e_rel, qnorm[q], gnorm_max_p[0]);      // a NaN window gives a NaN tau: nothing passes, nothing is certified
        t = nudge_up_(v);
    }
    tau[q] = t;
}

// The one-to-eight-query nomination scan (fir_gemm_search_few_keys_dev in fir_gemm.hip) on the 16-row fragment order: lane l of
// piece 2 kk + s holds row 16 s + (l & 15), feature quarter l >> 4 of step kk.
typedef _Float16 f16x2x __attribute__((ext_vector_type(2)));
template <int NQ>
__global__ void __launch_bounds__(256) k_gemm_scan_f16x(const uint4* __restrict__ gh, const float* __restrict__ gnorm, const uint4* __restrict__ qh,
                                                         const float* __restrict__ qinv, int64_t n, int dk16, float* __restrict__ proxies,
                                                         unsigned int* __restrict__ smin) {
    extern __shared__ __attribute__((aligned(16))) uint4 qsx[];           // [step][feature quarter][query]
    const int dk32 = dk16 >> 1;
    for (int idx = threadIdx.x; idx < dk32 * 4 * NQ; idx += blockDim.x) {
        const int i = idx % NQ, qt = (idx / NQ) & 3, kk = idx / (4 * NQ);
        qsx[idx] = qh[(size_t)kk * 64 + 16 * qt + i];                     // queries 0..7 sit in query block 0 of the pair's fragments
    }
    __syncthreads();
    const int lane = threadIdx.x & 63, qt = lane >> 4;
    const int64_t gw = (int64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6), nw = (int64_t)gridDim.x * (blockDim.x >> 6);
    const int64_t nrb = (n + 31) / 32;
    float m2[NQ], smallest[NQ];
#pragma unroll
    for (int i = 0; i < NQ; ++i) { m2[i] = 2.0f * qinv[i]; smallest[i] = __builtin_huge_valf(); }
    for (int64_t rb = gw; rb < nrb; rb += nw) {
        const uint4* a = gh + (size_t)rb * dk16 * 64 + lane;
        float acc[2][NQ];
#pragma unroll
        for (int i = 0; i < NQ; ++i) acc[0][i] = acc[1][i] = 0.f;
        for (int kb0 = 0; kb0 < dk16; kb0 += 8) {                          // dk16 is a multiple of 8
            uint4 g[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) g[u] = ld_nt(a + (size_t)(kb0 + u) * 64);
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                f16x2x gv[4];
                __builtin_memcpy(gv, &g[u], 16);
#pragma unroll
                for (int i = 0; i < NQ; ++i) {
                    const uint4 qq = qsx[(((kb0 + u) >> 1) * 4 + qt) * NQ + i];
                    f16x2x qv[4];
                    __builtin_memcpy(qv, &qq, 16);
#pragma unroll
                    for (int t = 0; t < 4; ++t) acc[u & 1][i] = __builtin_amdgcn_fdot2(gv[t], qv[t], acc[u & 1][i], false);
                }
            }
        }
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            const int64_t row = rb * 32 + 16 * s + (lane & 15);
            const float gn = row < n ? gnorm[row] : 0.f;
#pragma unroll
            for (int i = 0; i < NQ; ++i) {
                float dot = acc[s][i] + __shfl_xor(acc[s][i], 16, 64);    // the four feature quarters of the row
                dot += __shfl_xor(dot, 32, 64);
                if (lane < 16 && row < n) {
                    const float p = __builtin_fmaf(-m2[i], dot, gn);
                    proxies[(size_t)i * n + row] = p;
                    smallest[i] = fminf(smallest[i], p);                   // NaN never enters
                }
            }
        }
    }
#pragma unroll
    for (int i = 0; i < NQ; ++i) {
        float v = smallest[i];
#pragma unroll
        for (int off = 8; off >= 1; off >>= 1) v = fminf(v, __shfl_xor(v, off, 64));
        if (lane == 0 && v < __builtin_huge_valf()) atomicMin(&smin[i], fir::f32_orderable(v));
    }
}
