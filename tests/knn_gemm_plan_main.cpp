// Stand-alone host program over the plain-C++ part of csrc/fir_knn_select.h: the row sample of fir_gemm_search_knn_keys_dev
// (knn_sample_plan: R, the runs, the group size for a scratch bound). tests/test_knn_gemm_formulation.py builds it with the
// address and undefined-behaviour sanitizers and runs it; it prints one line per (n, k, div) it is given on the command line --
// "n k div tiles rows group stride b0:t0 b1:t1 ..." -- for the numpy restatement to compare with, then "ok", and returns 0 when
// every invariant below holds. No device code, no library.
#define FIR_KNN_HOST_ONLY
#include "../fast-image-recognition_amd/csrc/fir_knn_select.h"

#include <cstdio>
#include <cstdlib>
#include <vector>

#define REQUIRE(c)                                                          \
    do {                                                                    \
        if (!(c)) { std::printf("failed: %s (line %d)\n", #c, __LINE__); return 1; } \
    } while (0)

static int check(int64_t n, int32_t k, int div, size_t budget, bool print) {
    using namespace fir;
    const KnnSamplePlan p = knn_sample_plan(n, k, div, budget);
    const int64_t gallery_tiles = (n + 63) / 64;
    // R = min(n, max(floor, n k / div)) in whole tiles
    int64_t want = (int64_t)((__int128)n * k / div);
    if (want < kKnnSampleFloor) want = kKnnSampleFloor;
    if (want > n) want = n;
    REQUIRE(p.tiles == (want + 63) / 64);
    REQUIRE(p.tiles <= gallery_tiles && (n == 0) == (p.tiles == 0));
    REQUIRE(p.nruns >= 0 && p.nruns <= kKnnSampleRuns && (p.tiles < kKnnSampleRuns ? p.nruns == (int)p.tiles : p.nruns > kKnnSampleRuns / 2));
    REQUIRE(p.slack == gallery_tiles - p.tiles);
    // whole tiles inside [0, tiles), ascending, not overlapping, summing to R; every run run_len tiles, the last one what is left
    int64_t sum = 0, end_prev = 0, rows = 0;
    for (int i = 0; i < p.nruns; ++i) {
        const int64_t begin = p.run_begin(i), tiles = p.run_tiles(i);
        REQUIRE(tiles >= 1 && tiles <= p.run_len && (i + 1 == p.nruns || tiles == p.run_len) && begin >= end_prev && begin + tiles <= gallery_tiles);
        // the kernel's form of the same map: sample tile t -> gallery tile t + floor((t / run_len) slack / nruns)
        for (int64_t t : {sum, sum + tiles - 1}) REQUIRE(t + (t / p.run_len) * p.slack / p.nruns == begin + (t - sum));
        end_prev = begin + tiles;
        sum += tiles;
        const int64_t first = begin * 64, last = end_prev * 64 < n ? end_prev * 64 : n;
        REQUIRE(last > first);
        rows += last - first;
        // only the very last positions of a query's stored distances can be missing (the gallery's part-full last tile)
        if (last - first != tiles * 64) REQUIRE(i == p.nruns - 1);
    }
    REQUIRE(sum == p.tiles && rows == p.rows && p.rows <= n && p.rows > p.tiles * 64 - 64);
    // spread: the sample reaches into the last stretch of the gallery (a class-major gallery's last classes are seen)
    if (p.nruns > 1) REQUIRE(end_prev * p.nruns >= gallery_tiles * (p.nruns - 1));
    if (p.tiles == gallery_tiles) REQUIRE(p.rows == n);
    // the scratch bound: a group's stored distances fit the budget unless one query alone does not
    REQUIRE(p.row_stride == p.tiles * 64 && p.row_stride % 4 == 0);
    REQUIRE(p.group >= 1 && p.group <= 8192 && (p.group < 8 || p.group % 8 == 0));
    if (p.group > 1) REQUIRE((size_t)p.group * (size_t)p.row_stride * 4 <= budget);
    if (print) {
        std::printf("%lld %d %d %lld %lld %d %lld", (long long)n, (int)k, div, (long long)p.tiles, (long long)p.rows, p.group, (long long)p.row_stride);
        for (int i = 0; i < p.nruns; ++i) std::printf(" %lld:%lld", (long long)p.run_begin(i), (long long)p.run_tiles(i));
        std::printf("\n");
    }
    return 0;
}

int main(int argc, char** argv) {
    using namespace fir;
    static_assert(kKnnGemmMax == 256 && kKnnSampleRuns == 16 && kKnnSampleFloor == 32768 && kKnnSampleDiv == 1024, "the documented constants");
    const std::vector<int64_t> ns = {0,     1,     63,    64,     65,     200,     333,      1023,       1024,      4097,
                                     32767, 32768, 32769, 32832,  66000,  100000,  3728270,  3728399,    1000000,   ((int64_t)1 << 31) - 65,
                                     (int64_t)1 << 33};
    for (int64_t n : ns)
        for (int32_t k : {9, 10, 33, 64, 255, 256})
            for (int div : {1, 64, 1024, 2048})
                for (size_t budget : {(size_t)1, (size_t)1 << 20, kKnnSampleBytes})
                    if (check(n, k, div, budget, false)) return 1;
    // n k / 1024 just past the floor: K = 9 at n = 3 728 270 (32 767.99..) and 3 728 399 (32 769.1..)
    REQUIRE(knn_sample_plan(3728270, 9, 1024, kKnnSampleBytes).tiles == 512 && knn_sample_plan(3728399, 9, 1024, kKnnSampleBytes).tiles == 513);
    REQUIRE(knn_sample_plan(1000000, 256, 1024, kKnnSampleBytes).tiles == 250000 / 64 + 1 && knn_sample_plan(1000000, 256, 1024, kKnnSampleBytes).group == 64);
    REQUIRE(knn_sample_plan(1000000, 9, 1024, kKnnSampleBytes).group == 512);
    // hostile arguments are clamped, not trusted
    {
        const KnnSamplePlan p = knn_sample_plan(-5, 0, 0, 0);
        REQUIRE(p.tiles == 0 && p.rows == 0 && p.nruns == 0 && p.group == 1);
    }
    for (int i = 1; i + 2 < argc; i += 3)
        if (check(std::atoll(argv[i]), std::atoi(argv[i + 1]), std::atoi(argv[i + 2]), kKnnSampleBytes, true)) return 1;
    std::printf("ok\n");
    return 0;
}
