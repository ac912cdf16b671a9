// split_driver.cpp -- fir::recognize_split_bf (fir_db.h): one whole train / test split of the reference's experiments on the device,
// over ONE cached upload of the total image set -- the gallery is the subset handle of the split's rows, the queries are all the
// other rows, gathered out of the upload itself. Over a feature file of any dimension, for the two splits of subset_driver (split A:
// the rows with index % 3 != 0; split B: the rows whose index, hashed, is even): the answers of recognize_split_bf and, for the same
// split and the same test rows, the answers of recognize_images_bf_subset (the masked search over the same upload). Printed as JSON
// for tests/test_gpu_split_shim.py, with the number of uploads the whole run performed.
//   split_driver <features.txt> <features per image>
#include <cstdio>
#include <cstdlib>

#include "fir_db.h"
#include "fir_loader.h"

static void print_vec(const char* key, const std::vector<int>& v, bool comma) {
    std::printf("\"%s\": [", key);
    for (size_t i = 0; i < v.size(); ++i) std::printf("%s%d", i ? ", " : "", v[i]);
    std::printf("]%s\n", comma ? "," : "");
}

int main(int argc, char** argv) {
    if (argc < 3) { std::fprintf(stderr, "usage: split_driver <features.txt> <features per image>\n"); return 2; }
    const int d = std::atoi(argv[2]);
    fir::PackedFeatures packed;
    if (d < 1 || fir::load_features_packed(argv[1], d, fir::metric(), packed) <= 0) { std::fprintf(stderr, "split_driver: cannot load %s\n", argv[1]); return 1; }
    std::vector<FeaturesVector> feats;
    feats.reserve((size_t)packed.n);
    for (int64_t r = 0; r < packed.n; ++r) feats.emplace_back(&packed.rows[(size_t)r * d], &packed.rows[(size_t)(r + 1) * d]);
    std::vector<ImageInfo> total;
    total.reserve((size_t)packed.n);
    for (int64_t r = 0; r < packed.n; ++r) total.emplace_back(packed.class_no[(size_t)r], (int)r, feats[(size_t)r]);
    fir::set_cache_validation(fir::FIR_CACHE_VALIDATE_ALWAYS);

    std::vector<char> take[2];
    for (int s = 0; s < 2; ++s) take[s].assign((size_t)packed.n, 0);
    for (int64_t r = 0; r < packed.n; ++r) {
        take[0][(size_t)r] = r % 3 != 0;
        take[1][(size_t)r] = (((uint64_t)r * 0x9E3779B97F4A7C15ull) >> 40 & 1) == 0;
    }

    std::printf("{\n\"images\": %lld,\n", (long long)packed.n);
    const long uploads0 = fir::GalleryCache::uploads();
    for (int s = 0; s < 2; ++s) {
        std::vector<int> test_rows;
        const std::vector<int> split = fir::recognize_split_bf(total, take[s], d, nullptr, &test_rows);
        std::vector<ImageInfo> tests;
        for (size_t i = 0; i < test_rows.size(); ++i) tests.push_back(total[(size_t)test_rows[i]]);
        const std::vector<int> masked = fir::recognize_images_bf_subset(total, take[s], tests, d);
        print_vec(s ? "b_test_rows" : "a_test_rows", test_rows, true);
        print_vec(s ? "b_split" : "a_split", split, true);
        print_vec(s ? "b_masked" : "a_masked", masked, true);
    }
    std::printf("\"uploads\": %ld\n}\n", fir::GalleryCache::uploads() - uploads0);
    fir::GalleryCache::clear();
    return 0;
}
