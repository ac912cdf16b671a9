// subset_driver.cpp -- fir::recognize_images_bf_subset (fir_db.h): the random-split loop of the reference's experiments over ONE
// upload of the total image set. Over a feature file of any dimension: every image is a gallery row and a query; two different
// splits of the same cached vector (split A: the rows with index % 3 != 0; split B: the rows whose index, hashed, is even) are
// searched through the mask, and each split again through a cold cache over the COMPACTED vector, the way a caller without masks
// has to do it. Printed as JSON for tests/test_gpu_masked_shim.py: per split the rows taken, the masked answers (indices into the
// total set) and the compacted answers (indices into the compacted vector), and the number of uploads the masked part performed.
//   subset_driver <features.txt> <features per image>
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
    if (argc < 3) { std::fprintf(stderr, "usage: subset_driver <features.txt> <features per image>\n"); return 2; }
    const int d = std::atoi(argv[2]);
    fir::PackedFeatures packed;
    if (d < 1 || fir::load_features_packed(argv[1], d, fir::metric(), packed) <= 0) { std::fprintf(stderr, "subset_driver: cannot load %s\n", argv[1]); return 1; }
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
    std::vector<int> masked[2];
    for (int s = 0; s < 2; ++s) masked[s] = fir::recognize_images_bf_subset(total, take[s], total, d);
    std::printf("\"masked_uploads\": %ld,\n", fir::GalleryCache::uploads() - uploads0);
    fir::GalleryCache::clear();
    for (int s = 0; s < 2; ++s) {
        std::vector<int> rows;
        std::vector<ImageInfo> compact;
        for (int64_t r = 0; r < packed.n; ++r)
            if (take[s][(size_t)r]) { rows.push_back((int)r); compact.push_back(total[(size_t)r]); }
        const std::vector<int> cold = fir::recognize_images_bf(compact, total, d);
        fir::GalleryCache::clear();
        print_vec(s ? "b_rows" : "a_rows", rows, true);
        print_vec(s ? "b_masked" : "a_masked", masked[s], true);
        print_vec(s ? "b_cold" : "a_cold", cold, s == 0);
    }
    std::printf("}\n");
    return 0;
}
