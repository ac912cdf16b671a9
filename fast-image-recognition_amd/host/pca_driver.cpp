// pca_driver.cpp -- fir_pca.h end to end, over a feature file of any dimension (class-major, as the loader expects). Printed as JSON
// for tests/test_gpu_pca_shim.py:
//   rows      the images' features as loaded (float32, "%.9g" round-trips them), class-major
//   class_no  their classes
//   pca       extractPCA's output in the same order
//   bf_orig / bf_pca   fir::recognize_images_bf of the images with index % 3 == 0 against the others, over the original and over the
//             extractPCA database (indices into the gallery side)
//   fit_*     fir::fit_pca of the cached vector with take = (index % 2 == 1), all components: mean, values, basis ("%.17g")
//   direct_*  fir_gallery_scatter with the matching mask on a handle of its own + fir::symmetric_eigen: scatter count, eigenvalues
//             of the scatter matrix, vectors
//   projected_equal   1 when fir::project_gallery's rows equal fir::project of the same images bit for bit
//   pca_driver <features.txt> <features per image>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "fir_eigen.h"
#include "fir_loader.h"
#include "fir_pca.h"

static void print_f32(const char* key, const float* v, size_t n) {
    std::printf("\"%s\": [", key);
    for (size_t i = 0; i < n; ++i) std::printf("%s%.9g", i ? ", " : "", (double)v[i]);
    std::printf("],\n");
}
static void print_f64(const char* key, const std::vector<double>& v) {
    std::printf("\"%s\": [", key);
    for (size_t i = 0; i < v.size(); ++i) std::printf("%s%.17g", i ? ", " : "", v[i]);
    std::printf("],\n");
}
static void print_int(const char* key, const std::vector<int>& v) {
    std::printf("\"%s\": [", key);
    for (size_t i = 0; i < v.size(); ++i) std::printf("%s%d", i ? ", " : "", v[i]);
    std::printf("],\n");
}

int main(int argc, char** argv) {
    if (argc < 3) { std::fprintf(stderr, "usage: pca_driver <features.txt> <features per image>\n"); return 2; }
    const int d = std::atoi(argv[2]);
    fir::PackedFeatures packed;
    if (d < 1 || fir::load_features_packed(argv[1], d, fir::metric(), packed) <= 0) { std::fprintf(stderr, "pca_driver: cannot load %s\n", argv[1]); return 1; }
    const size_t n = (size_t)packed.n;
    ImagesDatabase db;
    std::vector<int> class_no;
    for (size_t r = 0; r < n; ++r) {
        if (r == 0 || packed.class_no[r] != packed.class_no[r - 1]) db.push_back(ImagesDatabase::value_type());
        db.back().emplace_back(&packed.rows[r * d], &packed.rows[(r + 1) * d]);
        class_no.push_back(packed.class_no[r]);
    }
    ImagesDatabase pca;
    extractPCA(db, pca);
    if (pca.size() != db.size()) { std::fprintf(stderr, "pca_driver: extractPCA failed\n"); return 1; }
    std::vector<float> flat;
    for (size_t c = 0; c < pca.size(); ++c) {
        if (pca[c].size() != db[c].size()) { std::fprintf(stderr, "pca_driver: class %zu changed size\n", c); return 1; }
        for (const FeaturesVector& f : pca[c]) flat.insert(flat.end(), f.begin(), f.end());
    }
    std::printf("{\n\"images\": %zu,\n\"classes\": %zu,\n", n, db.size());
    print_f32("rows", packed.rows.data(), n * d);
    print_int("class_no", class_no);
    print_f32("pca", flat.data(), flat.size());

    // brute force before and after: gallery = images with index % 3 != 0, queries = the others
    for (int pass = 0; pass < 2; ++pass) {
        const ImagesDatabase& base = pass ? pca : db;
        std::vector<ImageInfo> gallery, tests;
        size_t r = 0;
        for (size_t c = 0; c < base.size(); ++c)
            for (const FeaturesVector& f : base[c]) {
                (r % 3 ? gallery : tests).emplace_back(class_no[r], (int)r, f);
                ++r;
            }
        print_int(pass ? "bf_pca" : "bf_orig", fir::recognize_images_bf(gallery, tests, d));
        fir::GalleryCache::clear();
    }

    // fit_pca with a take list against scatter + symmetric_eigen by hand
    std::vector<ImageInfo> total;
    {
        size_t r = 0;
        for (size_t c = 0; c < db.size(); ++c)
            for (const FeaturesVector& f : db[c]) { total.emplace_back(class_no[r], (int)r, f); ++r; }
    }
    std::vector<char> take(n, 0);
    std::vector<uint64_t> mask(FIR_MASK_WORDS(n), 0);
    for (size_t r = 1; r < n; r += 2) { take[r] = 1; mask[r >> 6] |= (uint64_t)1 << (r & 63); }
    const fir::PcaModel model = fir::fit_pca(total, take, 0, d);
    if (!model.ok()) { std::fprintf(stderr, "pca_driver: fit_pca failed\n"); return 1; }
    print_f64("fit_mean", model.mean);
    print_f64("fit_values", model.values);
    print_f64("fit_basis", model.basis);
    fir_gallery* g = nullptr;
    if (fir_gallery_create(packed.rows.data(), packed.n, d, nullptr, fir::metric(), fir::device(), &g) != FIR_OK) { fir::log_error("pca_driver"); return 1; }
    std::vector<double> scatter((size_t)d * d), mean((size_t)d), values((size_t)d), vectors((size_t)d * d);
    int64_t count = 0;
    if (fir_gallery_scatter(g, mask.data(), nullptr, scatter.data(), mean.data(), &count) != FIR_OK) { fir::log_error("pca_driver"); return 1; }
    fir_gallery_destroy(g);
    fir::symmetric_eigen(scatter.data(), d, values.data(), vectors.data());
    std::printf("\"direct_count\": %lld,\n", (long long)count);
    print_f64("direct_mean", mean);
    print_f64("direct_values", values);
    print_f64("direct_basis", vectors);

    // the projected handle of the cached vector against the projected queries
    int equal = 0;
    fir_gallery* pg = fir::project_gallery(model, total, d);
    if (pg) {
        std::vector<float> got(n * (size_t)model.components);
        std::vector<FeaturesVector> feats;
        for (const ImageInfo& im : total) feats.push_back(im.features);
        const std::vector<FeaturesVector> q = fir::project(model, feats);
        if (fir_gallery_read_rows(pg, 0, packed.n, got.data(), nullptr) == FIR_OK && q.size() == n) {
            equal = 1;
            for (size_t r = 0; r < n; ++r) equal &= std::memcmp(&got[r * model.components], q[r].data(), (size_t)model.components * sizeof(float)) == 0;
        }
        fir_gallery_destroy(pg);
    }
    std::printf("\"projected_equal\": %d\n}\n", equal);
    return 0;
}
