// update_driver.cpp -- fir::GalleryCache::appended (fir_db.h): rows pushed back onto a gallery vector the cache holds reach the
// device as an append, not as a new upload. Over a feature file of any dimension: the first <gallery rows> images are the gallery,
// the others are pushed back later; every image of the file is a query. Printed as JSON for tests/test_gpu_gallery_update_shim.py:
// the answers after the in-place append and those of a cold cache over the same vector, then the same with a row of the prefix
// edited before the push_backs (the cache has to fall back to a whole upload).
//   update_driver <features.txt> <features per image> <gallery rows>
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
    if (argc < 4) { std::fprintf(stderr, "usage: update_driver <features.txt> <features per image> <gallery rows>\n"); return 2; }
    const int d = std::atoi(argv[2]);
    const long n0 = std::atol(argv[3]);
    fir::PackedFeatures packed;
    if (d < 1 || fir::load_features_packed(argv[1], d, fir::metric(), packed) <= 0) { std::fprintf(stderr, "update_driver: cannot load %s\n", argv[1]); return 1; }
    if (n0 < 1 || n0 >= packed.n) { std::fprintf(stderr, "update_driver: %ld gallery rows of %lld images\n", n0, (long long)packed.n); return 2; }
    std::vector<FeaturesVector> feats;
    feats.reserve((size_t)packed.n);
    for (int64_t r = 0; r < packed.n; ++r) feats.emplace_back(&packed.rows[(size_t)r * d], &packed.rows[(size_t)(r + 1) * d]);
    std::vector<ImageInfo> tests;
    tests.reserve((size_t)packed.n);
    for (int64_t r = 0; r < packed.n; ++r) tests.emplace_back(packed.class_no[(size_t)r], (int)r, feats[(size_t)r]);
    fir::set_cache_validation(fir::FIR_CACHE_VALIDATE_ALWAYS);

    std::printf("{\n\"images\": %lld,\n", (long long)packed.n);
    for (int edited = 0; edited < 2; ++edited) {
        std::vector<ImageInfo> db;                            // (no reserve: the push_backs below reallocate it)
        for (long r = 0; r < n0; ++r) db.emplace_back(packed.class_no[(size_t)r], (int)r, feats[(size_t)r]);
        const std::vector<int> before = fir::recognize_images_bf(db, tests, d);      // uploads the first n0 rows
        if (edited) feats[2][0] += 0.5f;                      // a row of the prefix changes behind the cache's back
        for (int64_t r = n0; r < packed.n; ++r) db.emplace_back(packed.class_no[(size_t)r], (int)r, feats[(size_t)r]);
        const int extended = fir::GalleryCache::appended(db, (size_t)n0);
        const std::vector<int> warm = fir::recognize_images_bf(db, tests, d);
        fir::GalleryCache::clear();
        const std::vector<int> cold = fir::recognize_images_bf(db, tests, d);
        fir::GalleryCache::clear();
        std::printf("\"%s_extended\": %d,\n", edited ? "edited" : "plain", extended);
        print_vec(edited ? "edited_before" : "plain_before", before, true);
        print_vec(edited ? "edited_warm" : "plain_warm", warm, true);
        print_vec(edited ? "edited_cold" : "plain_cold", cold, edited == 0);
    }
    std::printf("}\n");
    return 0;
}
