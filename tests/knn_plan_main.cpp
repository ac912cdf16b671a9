// Stand-alone host program over the plain-C++ part of csrc/fir_knn_select.h: fir_search_knn's k check and its tile / scratch
// sizing. tests/test_knn_select_formulation.py builds it with the address and undefined-behaviour sanitizers and runs it; it
// prints "ok" and returns 0 when every invariant below holds. No device code, no library.
#define FIR_KNN_HOST_ONLY
#include "../fast-image-recognition_amd/csrc/fir_knn_select.h"

#include <cstdio>
#include <vector>

#define REQUIRE(c)                                                          \
    do {                                                                    \
        if (!(c)) { std::printf("failed: %s (line %d)\n", #c, __LINE__); return 1; } \
    } while (0)

int main() {
    using namespace fir;
    REQUIRE(!knn_k_ok(0) && knn_k_ok(1) && knn_k_ok(kKnnMax) && !knn_k_ok(kKnnMax + 1) && !knn_k_ok(-1) && !knn_k_ok(INT32_MIN) && !knn_k_ok(INT32_MAX));
    const size_t ctl = 133000;
    const std::vector<int64_t> ns = {1, 2, 3, 4, 5, 63, 64, 65, 4097, 8191, 8192, 8193, 1000000, ((int64_t)1 << 31) - 65};
    for (int64_t n : ns)
        for (int t = 1; t <= kKnnTile; t *= 2) {
            const KnnPlan p = knn_plan(n, t, ctl);
            REQUIRE(p.row_stride >= n && p.row_stride < n + 4 && p.row_stride % 4 == 0);
            REQUIRE(p.dist_bytes >= (size_t)t * (size_t)p.row_stride * 4 && p.dist_bytes % 256 == 0);
            REQUIRE(p.bytes == p.dist_bytes + ctl);
            // the last float4 a workgroup loads ends inside the last query's row
            const size_t last = ((size_t)(t - 1) * (size_t)p.row_stride + (size_t)((n - 1) / 4 * 4) + 4) * 4;
            REQUIRE(last <= p.dist_bytes);
            if (t > 1) REQUIRE(knn_plan(n, t / 2, ctl).bytes <= p.bytes);     // halving the tile never asks for more
        }
    for (int64_t n : ns)
        for (int mb : {-3, 0, 1, 2, 7, kKnnMaxBlocks, 1 << 20}) {
            const int64_t s = knn_slice(n, mb);
            REQUIRE(s >= kKnnSlice && s % 1024 == 0);
            const int64_t blocks = (n + s - 1) / s;
            REQUIRE(blocks >= 1 && blocks <= (mb < 1 ? 1 : mb) && blocks * s >= n && blocks <= 0x7FFFFFFF);
        }
    for (int x = 1; x <= 300; ++x)
        for (int cap : {1, 2, 4, 8, 16}) {
            const int p = largest_pow2_le(x, cap);
            REQUIRE(p >= 1 && p <= x && p <= cap && (p & (p - 1)) == 0 && (p * 2 > x || p * 2 > cap));
        }
    REQUIRE(largest_pow2_le(0, 8) == 1);
    // a call's tile loop covers every query once with tiles no larger than the plan's
    for (int qb = 1; qb <= 70; ++qb)
        for (int t0 : {1, 2, 4, 8}) {
            const int t = largest_pow2_le(qb, t0);
            int done = 0;
            for (int q0 = 0; q0 < qb;) {
                const int tt = largest_pow2_le(qb - q0, t);
                REQUIRE(tt >= 1 && tt <= t && q0 + tt <= qb);
                q0 += tt;
                done += tt;
            }
            REQUIRE(done == qb);
        }
    std::printf("ok\n");
    return 0;
}
