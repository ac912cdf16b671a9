// fir_cls_kmedoids.h -- PNNwithClusteringClassifier::train (classification.cpp:320-388): k-medoids per class, on the device.
// Included by fir_cls.hip (one translation unit: -ffp-contract=off holds, struct fir_cls and its helpers are in scope).
//
// Formulation. For a class of n rows the reference recomputes dist(t, t1) = (sum_f (a_f - b_f)^2) / d inside both loops of
// every step (:337-343, :358-364). The value depends on the pair only, so it is computed once into a table T[n][n]:
//   T[t][t1] = S / d,  S = the sum fir_cls_distance_sums returns for query = training row t and row t1
// (subtract, multiply, add, un-fused, in feature order; one IEEE division). T is symmetric bit for bit: swapping the pair only
// changes the sign of every difference. A step is then a deterministic map on the medoid vector:
//   assign:  t -> the first cluster c (ascending) with a live medoid whose T[medoid_c][t] is the strict minimum from DBL_MAX;
//   update:  medoid_c -> the first member t (ascending) whose sum over members t1 (ascending, plain double sum) of T[t][t1]
//            is the strict minimum from DBL_MAX; a cluster without such a member is dead (-1) and stays dead.
// A step that leaves the medoid vector unchanged has reached a fixed point of that map: every later step would repeat it, so
// stopping there gives the result of all `steps` steps.
//
// k_kmed_detile + k_kmed_pairs fill the tables of a group of classes, k_kmed_iterate runs the steps, one workgroup per class.
namespace {

constexpr int kKmQB = 8;                  // rows of a class taken as the "query" side per wave pass
constexpr int kKmBlock = 1024;            // threads of the iteration's workgroup
constexpr int kKmMaxClusters = 256;
constexpr int kKmMaxRows = 32768;         // 16-bit cluster id per row in LDS
constexpr unsigned kKmNone = 0xFFFFu;     // row belongs to no cluster

// The "query" side: block b of eight consecutive rows of a class (qdesc[b] = class, first row inside the class), de-tiled from
// gal2 (which holds g - avg) into k_cls_scan's form qn[b][feature][8]; rows past the end of the class are zeros.
__global__ void __launch_bounds__(kBlock) k_kmed_detile(const double2* __restrict__ gal2, int dp2, const int32_t* __restrict__ class_off,
                                                         const int2* __restrict__ qdesc, int nqb, double* __restrict__ qn) {
    const int kk = dp2 * 2;
    const int64_t o = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (o >= (int64_t)nqb * kk * kKmQB) return;
    const int q = (int)(o & (kKmQB - 1));
    const int k = (int)((o / kKmQB) % kk);
    const int2 qd = qdesc[(o / kKmQB) / kk];
    const int64_t row = (int64_t)class_off[qd.x] + qd.y + q;
    double v = 0.0;
    if (row < class_off[qd.x + 1]) {
        const double2 g = gal2[((row >> 6) * dp2 + (k >> 1)) * 64 + (row & 63)];
        v = (k & 1) ? g.y : g.x;
    }
    qn[o] = v;
}

// T[q0 + q][row - r0] of one class for query block blockIdx.x and the blockIdx.y-th tile the class touches. One wave per
// block, a lane owns a row of the tile; the arithmetic and its order are k_cls_scan<8>'s (the same bits as
// fir_cls_distance_sums), then the division by d (:343, :364). Rows of the tile outside the class are computed and not written.
__global__ void __launch_bounds__(64) k_kmed_pairs(const double2* __restrict__ gal2, const double* __restrict__ qn, const int32_t* __restrict__ class_off,
                                                    const int2* __restrict__ qdesc, const int64_t* __restrict__ table_off, int dp2, int d,
                                                    double* __restrict__ table) {
    const int lane = threadIdx.x;
    const int2 qd = qdesc[blockIdx.x];
    const int r0 = class_off[qd.x], r1 = class_off[qd.x + 1], n = r1 - r0;
    const int t = (r0 >> 6) + (int)blockIdx.y;
    if (t > ((r1 - 1) >> 6)) return;
    sdouble_p qc = (sdouble_p)(uintptr_t)(qn + (size_t)blockIdx.x * dp2 * 2 * kKmQB);
    const double2* p = gal2 + (size_t)t * dp2 * 64 + lane;
    double acc[kKmQB];
#pragma unroll
    for (int q = 0; q < kKmQB; ++q) acc[q] = 0.0;
    int c = 0;
    for (; c + 4 <= dp2; c += 4) {
        double2 g[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) g[u] = p[(size_t)(c + u) * 64];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const double gv[2] = {g[u].x, g[u].y};
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                const int k = (c + u) * 2 + j;
                if (k < d) {
#pragma unroll
                    for (int q = 0; q < kKmQB; ++q) {
                        const double diff = gv[j] - qc[k * kKmQB + q];       // :339-341
                        acc[q] = acc[q] + diff * diff;                       // :342
                    }
                }
            }
        }
    }
    for (; c < dp2; ++c) {
        const double2 g = p[(size_t)c * 64];
        const double gv[2] = {g.x, g.y};
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int k = c * 2 + j;
            if (k < d) {
#pragma unroll
                for (int q = 0; q < kKmQB; ++q) {
                    const double diff = gv[j] - qc[k * kKmQB + q];
                    acc[q] = acc[q] + diff * diff;
                }
            }
        }
    }
    const int row = t * kTileRows + lane;
    if (row < r0 || row >= r1) return;
    double* T = table + table_off[qd.x] + (size_t)qd.y * n + (row - r0);
#pragma unroll
    for (int q = 0; q < kKmQB; ++q)
        if (qd.y + q < n) T[(size_t)q * n] = acc[q] / (double)d;            // dist /= num_of_cont_features (:343)
}

// The steps of class class0 + blockIdx.x. res: [num_classes][K] medoid rows (positions in train_rows, live medoids in cluster
// order, then -1), [num_classes] medoid counts, [num_classes] steps computed. colsum[nt]: a candidate's sum between the two
// passes of the update (written and read back by the same thread).
// Dynamic LDS: K x 8 bytes (smallest sum per cluster, as bits) + 2 K ints (medoids, winners) + n x 2 bytes (cluster of a row).
__global__ void __launch_bounds__(kKmBlock) k_kmed_iterate(const double* __restrict__ table, const int64_t* __restrict__ table_off,
                                                            const int32_t* __restrict__ class_off, int class0, int num_classes, int K, int steps,
                                                            double* __restrict__ colsum, int32_t* __restrict__ res) {
    extern __shared__ __attribute__((aligned(16))) unsigned long long km_best[];   // [K]
    int* med = (int*)(km_best + K);                                                 // [K]
    int* win = med + K;                                                             // [K]
    unsigned short* asg = (unsigned short*)(win + K);                               // [n]
    __shared__ int changed_s;
    const int tid = threadIdx.x;
    const int cl = class0 + (int)blockIdx.x;
    const int r0 = class_off[cl], n = class_off[cl + 1] - r0;
    int32_t* out_rows = res + (size_t)cl * K;
    int32_t* out_count = res + (size_t)num_classes * K + cl;
    int32_t* out_steps = out_count + num_classes;
    if (n <= K) {                                                                   // every row stays, in order (:381-385)
        for (int j = tid; j < K; j += kKmBlock) out_rows[j] = j < n ? r0 + j : -1;
        if (tid == 0) { *out_count = n; *out_steps = 0; }
        return;
    }
    const double* T = table + table_off[cl];
    for (int c = tid; c < K; c += kKmBlock) med[c] = c;                             // :322-324
    __syncthreads();
    int run = 0;
    for (int step = 0; step < steps; ++step) {
        for (int t = tid; t < n; t += kKmBlock) {                                   // :331-350
            double best = DBL_MAX;
            unsigned a = kKmNone;
            for (int c = 0; c < K; ++c) {
                const int m = med[c];
                if (m < 0) continue;
                const double dist = T[(size_t)m * n + t];
                if (dist < best) { best = dist; a = (unsigned)c; }
            }
            asg[t] = (unsigned short)a;
        }
        for (int c = tid; c < K; c += kKmBlock) { km_best[c] = ~0ull; win[c] = 0x7FFFFFFF; }
        if (tid == 0) changed_s = 0;
        __syncthreads();
        // :351-375. Candidate t adds its cluster's members in ascending t1; T[t1][t] = T[t][t1], and adjacent lanes read adjacent
        // addresses. The loads do not depend on the membership, eight are in flight; the sums are non-negative or NaN, so the
        // bits of those below DBL_MAX order like the values.
        for (int t = tid; t < n; t += kKmBlock) {
            const unsigned a = asg[t];
            if (a == kKmNone) continue;
            const double* col = T + t;
            double sum = 0.0;
            int t1 = 0;
            for (; t1 + 8 <= n; t1 += 8) {
                double v[8];
#pragma unroll
                for (int u = 0; u < 8; ++u) v[u] = col[(size_t)(t1 + u) * n];
#pragma unroll
                for (int u = 0; u < 8; ++u)
                    if (asg[t1 + u] == a) sum = sum + v[u];
            }
            for (; t1 < n; ++t1)
                if (asg[t1] == a) sum = sum + col[(size_t)t1 * n];
            colsum[r0 + t] = sum;
            if (sum < DBL_MAX) atomicMin(&km_best[a], (unsigned long long)__double_as_longlong(sum));
        }
        __syncthreads();
        for (int t = tid; t < n; t += kKmBlock) {                                   // the first member with that sum
            const unsigned a = asg[t];
            if (a == kKmNone) continue;
            const double sum = colsum[r0 + t];
            if (sum < DBL_MAX && (unsigned long long)__double_as_longlong(sum) == km_best[a]) atomicMin(&win[a], t);
        }
        __syncthreads();
        for (int c = tid; c < K; c += kKmBlock) {
            const int m = win[c] == 0x7FFFFFFF ? -1 : win[c];                       // no member, or none below DBL_MAX: dead
            if (m != med[c]) changed_s = 1;
            med[c] = m;
        }
        ++run;
        __syncthreads();
        const int changed = changed_s;
        __syncthreads();
        if (!changed) break;                                                        // a fixed point: the later steps repeat this one
    }
    if (tid == 0) {
        int m = 0;
        for (int c = 0; c < K; ++c)
            if (med[c] >= 0) out_rows[m++] = r0 + med[c];
        *out_count = m;
        *out_steps = run;
        for (; m < K; ++m) out_rows[m] = -1;
    }
}

}  // namespace

extern "C" int fir_cls_kmedoids(fir_cls* c, int32_t num_clusters, int32_t steps, int64_t scratch_bytes, int32_t* medoid_rows, int32_t* medoid_count,
                                int32_t* steps_run) {
    if (!c || !medoid_rows || !medoid_count) return fir_fail_(FIR_ERR_ARG, "NULL argument");
    if (num_clusters < 1 || num_clusters > kKmMaxClusters) return fir_fail_(FIR_ERR_ARG, "num_clusters=%d outside [1,%d]", num_clusters, kKmMaxClusters);
    if (steps < 0) return fir_fail_(FIR_ERR_ARG, "steps < 0");
    if (scratch_bytes < 0) return fir_fail_(FIR_ERR_ARG, "scratch_bytes < 0");
    const int K = num_clusters, nc = c->num_classes;
    const std::vector<int32_t>& off = c->class_off_h;
    for (int i = 0; i < nc; ++i) {
        const int n = off[(size_t)i + 1] - off[(size_t)i];
        if (n > K && n > kKmMaxRows) return fir_fail_(FIR_ERR_ARG, "class %d has %d rows; at most %d can be clustered", i, n, kKmMaxRows);
    }
    FIR_HIP(hipSetDevice(c->device));
    int64_t bound = scratch_bytes;
    if (bound == 0) {                                                               // automatic: half of what is free now
        size_t free_b = 0, total_b = 0;
        FIR_HIP(hipMemGetInfo(&free_b, &total_b));
        bound = (int64_t)(free_b / 2);
    }
    auto table_doubles = [&](int i) -> int64_t {
        const int64_t n = off[(size_t)i + 1] - off[(size_t)i];
        return n > K ? n * n : 0;
    };
    for (int i = 0; i < nc; ++i)
        if (table_doubles(i) * 8 > bound)
            return fir_fail_(FIR_ERR_NOMEM, "the distance table of class %d (%lld bytes) exceeds the scratch bound (%lld bytes)", i,
                             (long long)table_doubles(i) * 8, (long long)bound);
    // groups of consecutive classes whose tables fit the bound together
    struct Group { int c0, c1, qb0, qb1, max_n, max_tiles; };
    std::vector<Group> groups;
    std::vector<int64_t> toff((size_t)nc, 0);
    std::vector<int2> qdesc;
    int64_t max_table = 0;
    int max_qb = 0;
    for (int c0 = 0; c0 < nc;) {
        Group g = {c0, c0, (int)qdesc.size(), 0, 0, 0};
        int64_t used = 0;
        for (; g.c1 < nc && (used + table_doubles(g.c1)) * 8 <= bound; ++g.c1) {
            const int i = g.c1, r0 = off[(size_t)i], n = off[(size_t)i + 1] - r0;
            toff[(size_t)i] = used;
            if (n <= K) continue;
            used += table_doubles(i);
            for (int q0 = 0; q0 < n; q0 += kKmQB) qdesc.push_back(make_int2(i, q0));
            g.max_n = std::max(g.max_n, n);
            g.max_tiles = std::max(g.max_tiles, ((r0 + n - 1) >> 6) - (r0 >> 6) + 1);
        }
        g.qb1 = (int)qdesc.size();
        max_table = std::max(max_table, used);
        max_qb = std::max(max_qb, g.qb1 - g.qb0);
        groups.push_back(g);
        c0 = g.c1;
    }
    auto drain = fir_on_exit([&] { (void)hipStreamSynchronize(c->stream); });      // the copies below read and write host memory of this call
    const int kk = c->dp2 * 2;
    auto up256 = [](size_t b) { return (b + 255) / 256 * 256; };
    // device scratch: tables of a group | its de-tiled rows | the candidates' sums; descriptors: table offsets | query blocks | results
    const size_t b_table = up256((size_t)max_table * 8), b_qn = up256((size_t)max_qb * kk * kKmQB * 8), b_col = up256((size_t)std::max<int64_t>(c->nt, 1) * 8);
    const size_t b_toff = up256((size_t)nc * 8), b_qd = up256(qdesc.size() * sizeof(int2)), b_res = (size_t)nc * (K + 2) * sizeof(int32_t);
    int rc;
    if ((rc = FIR_RESERVE(c->km, b_table + b_qn + b_col)) || (rc = FIR_RESERVE(c->km_meta, b_toff + b_qd + b_res)) || (rc = cls_lds_attributes(c))) return rc;
    double* d_table = c->km.as<double>();
    double* d_qn = (double*)(c->km.as<char>() + b_table);
    double* d_col = (double*)(c->km.as<char>() + b_table + b_qn);
    int64_t* d_toff = c->km_meta.as<int64_t>();
    int2* d_qd = (int2*)(c->km_meta.as<char>() + b_toff);
    int32_t* d_res = (int32_t*)(c->km_meta.as<char>() + b_toff + b_qd);
    FIR_HIP(hipMemcpyAsync(d_toff, toff.data(), (size_t)nc * 8, hipMemcpyHostToDevice, c->stream));
    if (!qdesc.empty()) FIR_HIP(hipMemcpyAsync(d_qd, qdesc.data(), qdesc.size() * sizeof(int2), hipMemcpyHostToDevice, c->stream));
    const int run_steps = steps == 0 ? 100 : steps;                                 // :330
    for (const Group& g : groups) {
        const int nqb = g.qb1 - g.qb0;
        const size_t lds = (size_t)K * 16 + (((size_t)g.max_n * 2 + 15) & ~(size_t)15);
        if (nqb > 0) {
            const int64_t total = (int64_t)nqb * kk * kKmQB;
            hipLaunchKernelGGL(k_kmed_detile, dim3((unsigned)((total + kBlock - 1) / kBlock)), dim3(kBlock), 0, c->stream, c->gal2, c->dp2, c->class_off,
                               d_qd + g.qb0, nqb, d_qn);
            cls_prof(c, 0, 0.0, nullptr);
            hipLaunchKernelGGL(k_kmed_pairs, dim3(nqb, g.max_tiles), dim3(64), 0, c->stream, c->gal2, d_qn, c->class_off, d_qd + g.qb0, d_toff, c->dp2, c->d,
                               d_table);
            cls_prof(c, 1, 0.0, "fir::k_kmed_pairs");
        }
        cls_prof(c, 0, 0.0, nullptr);
        hipLaunchKernelGGL(k_kmed_iterate, dim3(g.c1 - g.c0), dim3(kKmBlock), lds, c->stream, d_table, d_toff, c->class_off, g.c0, nc, K, run_steps, d_col, d_res);
        cls_prof(c, 1, 0.0, "fir::k_kmed_iterate");
        FIR_HIP(hipGetLastError());
    }
    FIR_HIP(hipMemcpyAsync(medoid_rows, d_res, (size_t)nc * K * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
    FIR_HIP(hipMemcpyAsync(medoid_count, d_res + (size_t)nc * K, (size_t)nc * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
    if (steps_run) FIR_HIP(hipMemcpyAsync(steps_run, d_res + (size_t)nc * (K + 1), (size_t)nc * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
    FIR_HIP(hipStreamSynchronize(c->stream));
    return FIR_OK;
}
