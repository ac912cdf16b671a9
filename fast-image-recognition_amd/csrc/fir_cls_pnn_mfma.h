// fir_cls_pnn_mfma.h -- PNNClassifier::predict_bf (classification.cpp:188-226) for batches, on the float64 matrix cores.
// Included by fir_cls.hip (one translation unit: -ffp-contract=off holds, struct fir_cls and its helpers are in scope).
//
// Formulation. The scan evaluates S[q][t] = sum_k ((g-avg) - (q-avg))^2 with three vector operations per element. Here
//   S[q][t] = (|q-avg|^2 + |g-avg|^2) - 2 (q-avg).(g-avg),
// the dot products by v_mfma_f64_16x16x4_f64 -- one matrix-pipe operation per element. The table lands in c->sums[q][t] where the
// scan puts it, and k_cls_pnn (exp, per-class sums) and k_cls_argbest run on it unchanged: no floating-point atomics anywhere, the
// scores are the same bits from run to run. The three-term form is not the scan's bits. First order, in any summation order,
//   |dS| <= 2 u (d + 2) (|q-avg|^2 + |g-avg|^2),  u = 2^-53,
// so every term exp(-S / (2 d var)) of a class score, and with it the score, moves by at most the relative
//   E(q) = 2 u (d + 2) (|q-avg|^2 + max_t |g_t-avg|^2) / (2 d var);
// 2^-40 on top covers the device exp and k_cls_pnn's summation order. E(q) bounds the form against exact arithmetic, to first order;
// the scan's own sum is rounded too (about (d + 2) u S, S <= 2 (|q-avg|^2 + |g-avg|^2)), so against the SCAN's score the worst case
// approaches 2 E(q) -- the factor 2 in B below is that. Differences seen are a thousandth of E(q) (profiles/pnn_matrix_cores.txt).
// k_cls_pnn_band looks at the two largest scores s1 >= s2 of every query: unless s2 (1 + B) < s1 (1 - B), B = 2 (E(q) + 2^-40), the
// scan's arg-max could differ, and the scan answers that query (class and scores). So does it for a query with a NaN score or with
// every score 0.
//
// Operands. gal2[(t*dp2 + c)*64 + r] is a double2: features 2c, 2c+1 of row 64t + r, centred. The instruction wants
// A[row = lane&15][k = lane>>4] and B[k = lane>>4][col = lane&15], one double per lane; C/D col = lane&15, row = (lane>>4) + 4*reg.
// Queries are A, training rows B (a register of D is then 16 consecutive training rows of one query: 128-byte stores). Lane l loads
// the double2 of chunk c0 + (l>>4), row 16*rb + (l&15): .x and .y feed two MFMAs whose k-sets are the even and the odd features of
// four chunks; the query side (LDS, [chunk][query] double2) presents the same pairing. No second copy of the training set.
//
// k_cls_row_norms: |g_t-avg|^2 and their maximum, once per handle. k_cls_pnn_prep: the centred queries in the order the A operand reads
// them ([chunk][query] double2 per group of queries) + |q-avg|^2.
// k_cls_pnn_mfma<NQB>: 16*NQB queries share one read of the rows; their operands stay in LDS for the life of the workgroup.
namespace {

typedef double pm_double4 __attribute__((ext_vector_type(4)));
constexpr int kPmBlock = 512;                 // eight waves, a 64-row tile each
constexpr size_t kPmLdsMax = 160 * 1024;      // the whole LDS of a compute unit: 32 queries of up to 640 features, 16 of up to 1280

// ng[row] = sum_k (g-avg)^2 in feature order; *ng_max = their maximum as the bits of a non-negative double (unsigned order = value order,
// NaN above everything: a NaN row sends every query to the scan). One thread per row.
__global__ void __launch_bounds__(kBlock) k_cls_row_norms(const double2* __restrict__ gal2, int64_t nt, int dp2, double* __restrict__ ng,
                                                           unsigned long long* __restrict__ ng_max) {
    const int64_t row = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    double acc = 0.0;
    if (row < nt) {
        const double2* p = gal2 + (size_t)(row >> 6) * dp2 * 64 + (row & 63);
        for (int c = 0; c < dp2; ++c) {
            const double2 g = p[(size_t)c * 64];
            acc = acc + g.x * g.x;
            acc = acc + g.y * g.y;                                     // the padding feature of an odd d holds 0
        }
        ng[row] = acc;
    }
    unsigned long long m = (unsigned long long)__double_as_longlong(acc);
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        const unsigned long long o = (unsigned long long)__shfl_xor((long long)m, off, 64);
        m = o > m ? o : m;
    }
    if ((threadIdx.x & 63) == 0) atomicMax(ng_max, m);
}

// One wave per query slot (groups of NQ slots, slots past nq are zeros): qp[(group*dp2 + c)*NQ + s] = features 2c, 2c+1 of the centred
// query, nqv[slot] = its squared norm.
__global__ void __launch_bounds__(kBlock) k_cls_pnn_prep(const double* __restrict__ qc, int nq, int d, int dp2, int NQ, double2* __restrict__ qp,
                                                          double* __restrict__ nqv) {
    const int slot = blockIdx.x * (kBlock / 64) + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    const int grp = slot / NQ, s = slot % NQ;
    double acc = 0.0;
    for (int c = lane; c < dp2; c += 64) {
        double2 v = make_double2(0.0, 0.0);
        if (slot < nq) {
            v.x = qc[(size_t)slot * d + 2 * c];
            if (2 * c + 1 < d) v.y = qc[(size_t)slot * d + 2 * c + 1];
        }
        qp[((size_t)grp * dp2 + c) * NQ + s] = v;
        acc = acc + v.x * v.x;
        acc = acc + v.y * v.y;
    }
    acc = wave_sum(acc);
    if (lane == 0) nqv[slot] = acc;
}

// sums[q][row] = (nqv[q] + ng[row]) - 2 dot. grid (workgroups, groups of NQ = 16*NQB queries); wave w of workgroup b takes the tiles
// b*8 + w, + 8*gridDim.x, ... Dynamic LDS: dp2 * NQ double2.
template <int NQB>
__global__ void __launch_bounds__(kPmBlock) k_cls_pnn_mfma(const double2* __restrict__ gal2, const double2* __restrict__ qp, const double* __restrict__ nqv,
                                                            const double* __restrict__ ng, int64_t nt, int tiles, int dp2, int nq, double* __restrict__ sums) {
    constexpr int NQ = NQB * 16;
    extern __shared__ __attribute__((aligned(16))) double2 pm_q[];      // [chunk][query of the group]
    const int grp = blockIdx.y;
    {
        const double2* src = qp + (size_t)grp * dp2 * NQ;
        for (int i = threadIdx.x; i < dp2 * NQ; i += kPmBlock) pm_q[i] = src[i];
    }
    __syncthreads();
    const int lane = threadIdx.x & 63, lr = lane & 15, lk = lane >> 4;
    const int q0 = grp * NQ;
    const int full = dp2 & ~3;                                           // chunks [0, full): whole k-steps of four chunks
    const double2 zero2 = make_double2(0.0, 0.0);
    double qnorm[NQB][4];                                                // of the queries this lane's D registers belong to (nqv covers every slot of the group)
#pragma unroll
    for (int qb = 0; qb < NQB; ++qb)
#pragma unroll
        for (int r = 0; r < 4; ++r) qnorm[qb][r] = nqv[q0 + qb * 16 + lk + 4 * r];
    for (int t = blockIdx.x * (kPmBlock / 64) + (threadIdx.x >> 6); t < tiles; t += gridDim.x * (kPmBlock / 64)) {
        const double2* p = gal2 + (size_t)t * dp2 * 64 + lr;
        pm_double4 acc[4][NQB];
#pragma unroll
        for (int rb = 0; rb < 4; ++rb)
#pragma unroll
            for (int qb = 0; qb < NQB; ++qb) acc[rb][qb] = (pm_double4){0.0, 0.0, 0.0, 0.0};
        // the rows of two k-steps ahead are in flight under a step's MFMAs: at 32 queries per read the pass wants more of HBM than one
        // step ahead keeps moving (two waves per SIMD, 4 KB per wave and step)
        double2 g[4], g1[4];
#pragma unroll
        for (int rb = 0; rb < 4; ++rb) {
            g[rb] = full > 0 ? p[(size_t)lk * 64 + rb * 16] : zero2;
            g1[rb] = full > 4 ? p[(size_t)(4 + lk) * 64 + rb * 16] : zero2;
        }
        for (int c0 = 0; c0 < full; c0 += 4) {
            double2 gn[4];
            if (c0 + 8 < full) {
#pragma unroll
                for (int rb = 0; rb < 4; ++rb) gn[rb] = p[(size_t)(c0 + 8 + lk) * 64 + rb * 16];
            } else {
#pragma unroll
                for (int rb = 0; rb < 4; ++rb) gn[rb] = zero2;
            }
            double2 qv[NQB];
#pragma unroll
            for (int qb = 0; qb < NQB; ++qb) qv[qb] = pm_q[(c0 + lk) * NQ + qb * 16 + lr];
#pragma unroll
            for (int rb = 0; rb < 4; ++rb)
#pragma unroll
                for (int qb = 0; qb < NQB; ++qb) acc[rb][qb] = __builtin_amdgcn_mfma_f64_16x16x4f64(qv[qb].x, g[rb].x, acc[rb][qb], 0, 0, 0);
#pragma unroll
            for (int rb = 0; rb < 4; ++rb)
#pragma unroll
                for (int qb = 0; qb < NQB; ++qb) acc[rb][qb] = __builtin_amdgcn_mfma_f64_16x16x4f64(qv[qb].y, g[rb].y, acc[rb][qb], 0, 0, 0);
#pragma unroll
            for (int rb = 0; rb < 4; ++rb) { g[rb] = g1[rb]; g1[rb] = gn[rb]; }
        }
        if (full < dp2) {                                                // the last one to three chunks: lanes past dp2 contribute 0 and read nothing
            const bool ok = full + lk < dp2;
            double2 qv[NQB];
#pragma unroll
            for (int rb = 0; rb < 4; ++rb) g[rb] = ok ? p[(size_t)(full + lk) * 64 + rb * 16] : zero2;
#pragma unroll
            for (int qb = 0; qb < NQB; ++qb) qv[qb] = ok ? pm_q[(full + lk) * NQ + qb * 16 + lr] : zero2;
#pragma unroll
            for (int rb = 0; rb < 4; ++rb)
#pragma unroll
                for (int qb = 0; qb < NQB; ++qb) acc[rb][qb] = __builtin_amdgcn_mfma_f64_16x16x4f64(qv[qb].x, g[rb].x, acc[rb][qb], 0, 0, 0);
#pragma unroll
            for (int rb = 0; rb < 4; ++rb)
#pragma unroll
                for (int qb = 0; qb < NQB; ++qb) acc[rb][qb] = __builtin_amdgcn_mfma_f64_16x16x4f64(qv[qb].y, g[rb].y, acc[rb][qb], 0, 0, 0);
        }
        // D: col = lane&15 -> training row 16*rb + lr; row = (lane>>4) + 4*reg -> query 16*qb + lk + 4*reg of the group
#pragma unroll
        for (int rb = 0; rb < 4; ++rb) {
            const int64_t row = (int64_t)t * kTileRows + rb * 16 + lr;
            if (row < nt) {                                              // the padding rows of the last tile are not in sums[q][nt]
                const double gnorm = ng[row];
#pragma unroll
                for (int qb = 0; qb < NQB; ++qb)
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const int q = q0 + qb * 16 + lk + 4 * r;
                        if (q < nq) sums[(size_t)q * nt + row] = (qnorm[qb][r] + gnorm) - 2.0 * acc[rb][qb][r];
                    }
            }
        }
    }
}

// One wave per query: flags[q] = 0 when the two largest scores are further apart than the form's error can bridge, else 1 (the scan
// answers). efac = 2 * 2^-53 * (d + 2) / (2 d var).
__global__ void __launch_bounds__(64) k_cls_pnn_band(const double* __restrict__ scores, int num_classes, const double* __restrict__ nqv,
                                                      const unsigned long long* __restrict__ ng_max, double efac, int32_t* __restrict__ flags) {
    const int q = blockIdx.x, lane = threadIdx.x;
    const double* s = scores + (size_t)q * num_classes;
    double s1 = 0.0, s2 = 0.0;                                           // scores are >= 0
    bool nan = false;
    for (int i = lane; i < num_classes; i += 64) {
        const double v = s[i];
        if (v != v) nan = true;
        else if (v > s1) { s2 = s1; s1 = v; }
        else if (v > s2) s2 = v;
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        const double o1 = __shfl_xor(s1, off, 64), o2 = __shfl_xor(s2, off, 64);
        const double lo = s1 < o1 ? s1 : o1, hi2 = s2 > o2 ? s2 : o2;
        s1 = s1 > o1 ? s1 : o1;
        s2 = lo > hi2 ? lo : hi2;
    }
    nan = __any(nan) != 0;
    if (lane != 0) return;
    const double e = efac * (nqv[q] + __longlong_as_double((long long)*ng_max));
    const double b = 2.0 * (e + 0x1p-40);
    const bool settled = !nan && s1 > 0.0 && s2 * (1.0 + b) < s1 * (1.0 - b);      // NaN / inf bound: false
    flags[q] = settled ? 0 : 1;
}

// 0 = the call is answered, 1 = this shape stays with the scan (no query tile fits LDS; nothing was queued), < 0 = error.
// qb <= cls_batch(c), nt > 0, var > 0, the device is current.
int cls_pnn_mfma(fir_cls* c, const double* queries, int32_t qb, double var, double* scores, int32_t* best_class) {
    const size_t per_query = (size_t)c->dp2 * sizeof(double2);
    const int nqt = 32 * per_query <= kPmLdsMax ? 32 : 16 * per_query <= kPmLdsMax ? 16 : 0;
    if (!nqt) return 1;
    int rc;
    typedef void (*mfma_fn)(const double2*, const double2*, const double*, const double*, int64_t, int, int, int, double*);
    const mfma_fn fn = nqt == 32 ? k_cls_pnn_mfma<2> : k_cls_pnn_mfma<1>;
    const char* name = nqt == 32 ? "fir::k_cls_pnn_mfma<2>" : "fir::k_cls_pnn_mfma<1>";
    if ((rc = cls_lds_attributes(c))) return rc;
    // |g-avg|^2 per row: word 0 of the buffer is the maximum, the norms follow
    if (!c->pm_ng_ready) {
        if ((rc = FIR_RESERVE(c->pm_ng, ((size_t)c->nt + 1) * sizeof(double)))) return rc;
        FIR_HIP(hipMemsetAsync(c->pm_ng.p, 0, sizeof(double), c->stream));
        hipLaunchKernelGGL(k_cls_row_norms, dim3((unsigned)((c->nt + kBlock - 1) / kBlock)), dim3(kBlock), 0, c->stream, c->gal2, c->nt, c->dp2,
                           c->pm_ng.as<double>() + 1, c->pm_ng.as<unsigned long long>());
        FIR_HIP(hipGetLastError());
        c->pm_ng_ready = true;
    }
    const unsigned long long* ng_max = c->pm_ng.as<unsigned long long>();
    const double* ng = c->pm_ng.as<double>() + 1;
    const int groups = (qb + nqt - 1) / nqt, slots = groups * nqt;
    const double* dq = nullptr;
    if ((rc = cls_stage_queries(c, queries, qb, &dq))) return rc;
    const size_t qp_count = (size_t)groups * c->dp2 * nqt;                     // double2 each, then the query norms
    if ((rc = FIR_RESERVE(c->qc, (size_t)qb * c->d * sizeof(double))) || (rc = FIR_RESERVE(c->sums, (size_t)qb * c->nt * sizeof(double))) ||
        (rc = FIR_RESERVE(c->scores, (size_t)qb * c->num_classes * sizeof(double))) ||     // (before anything is queued: not inside cls_queue_pnn's event pair)
        (rc = FIR_RESERVE(c->best, (size_t)qb * sizeof(int32_t))) || (rc = FIR_RESERVE(c->pm_q, qp_count * sizeof(double2) + (size_t)slots * sizeof(double))) ||
        (rc = FIR_RESERVE(c->pm_flags, (size_t)qb * sizeof(int32_t))))
        return rc;
    double2* qp = c->pm_q.as<double2>();
    double* nqv = (double*)(qp + qp_count);
    int32_t* flags = c->pm_flags.as<int32_t>();
    const int64_t count = (int64_t)qb * c->d;
    hipLaunchKernelGGL(k_cls_center_queries, dim3((unsigned)((count + kBlock - 1) / kBlock)), dim3(kBlock), 0, c->stream, dq, count, c->d, c->avg, c->qc.as<double>());
    hipLaunchKernelGGL(k_cls_pnn_prep, dim3(slots / (kBlock / 64)), dim3(kBlock), 0, c->stream, c->qc.as<double>(), qb, c->d, c->dp2, nqt, qp, nqv);
    const int wgs = (int)std::min<int64_t>((c->tiles + kPmBlock / 64 - 1) / (kPmBlock / 64), c->cus);
    const size_t lds = (size_t)nqt * per_query;
    // profiled: three event pairs per batch, in this order -- the matrix-core pass, k_cls_pnn, k_cls_pnn_band; the dispatch record is the first's
    cls_prof(c, 0, 0.0, nullptr);
    hipLaunchKernelGGL(fn, dim3(wgs, groups), dim3(kPmBlock), lds, c->stream, c->gal2, qp, nqv, ng, c->nt, (int)c->tiles, c->dp2, qb, c->sums.as<double>());
    cls_prof(c, 1, 0.0, name);
    cls_prof(c, 0, 0.0, nullptr);
    if ((rc = cls_queue_pnn(c, qb, var))) return rc;
    cls_prof(c, 1, 0.0, nullptr);
    cls_queue_argbest(c, qb, 0, c->best.as<int32_t>());
    cls_prof(c, 0, 0.0, nullptr);
    hipLaunchKernelGGL(k_cls_pnn_band, dim3(qb), dim3(64), 0, c->stream, c->scores.as<double>(), c->num_classes, nqv, ng_max,
                       2.0 * 0x1p-53 * (double)(c->d + 2) / ((double)(2 * (size_t)c->d) * var), flags);
    cls_prof(c, 1, 0.0, nullptr);
    if (c->profiling) {
        // algorithmic bytes of the pass: one read of the training rows (and their norms) per group of queries, the query operands, the sums written
        c->last.bytes = (double)groups * ((double)c->tiles * 64.0 * c->dp2 * 16.0 + 8.0 * (double)c->nt) + (double)groups * (double)lds + 8.0 * (double)qb * (double)c->nt;
        c->last.flops = 2.0 * (double)c->nt * (double)c->d * (double)qb;
    }
    FIR_HIP(hipGetLastError());
    std::vector<int32_t> hflags((size_t)qb);
    if (scores) FIR_HIP(hipMemcpyAsync(scores, c->scores.p, (size_t)qb * c->num_classes * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    if (best_class) FIR_HIP(hipMemcpyAsync(best_class, c->best.p, (size_t)qb * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
    FIR_HIP(hipMemcpyAsync(hflags.data(), flags, (size_t)qb * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
    FIR_HIP(hipStreamSynchronize(c->stream));
    c->pm_queries += qb;
    // inside the band (or NaN, or every score 0): the scan form answers, class and scores, into the query's slots
    std::vector<int32_t> which;
    for (int32_t i = 0; i < qb; ++i)
        if (hflags[(size_t)i]) which.push_back(i);
    c->pm_fallback += (int64_t)which.size();
    return cls_answer_exactly(c, queries, which, false, best_class, scores,
                              [&](const double* q, int32_t n, double* sc, int32_t* best) { return cls_pnn_exact(c, q, n, var, sc, best); });
}

}  // namespace
