// far_driver.cpp -- fir::other_class_distances and fir::far_threshold (fir_classifiers.h: the reference's otherClassesDists,
// ann.cpp:286-298, and getThreshold, ann.cpp:84-93, for a whole gallery on the device) over a feature file of any dimension,
// printed as JSON for tests/test_gpu_other_class.py to compare with the oracle.
//   far_driver <features.txt> <features per image> <false accept rate>
#include <cstdio>
#include <cstdlib>
#include <iostream>

#include "fir_classifiers.h"
#include "fir_loader.h"

int main(int argc, char** argv) {
    if (argc < 4) { std::fprintf(stderr, "usage: far_driver <features.txt> <features per image> <false accept rate>\n"); return 2; }
    const int d = std::atoi(argv[2]);
    const float rate = (float)std::atof(argv[3]);
    fir::PackedFeatures packed;
    if (d < 1 || fir::load_features_packed(argv[1], d, fir::metric(), packed) <= 0) { std::fprintf(stderr, "far_driver: cannot load %s\n", argv[1]); return 1; }
    // every image of the file is a gallery image, in the file's class-major order (the order of loadImages' ImagesDatabase)
    std::vector<FeaturesVector> feats;
    feats.reserve((size_t)packed.n);
    for (int64_t r = 0; r < packed.n; ++r) feats.emplace_back(&packed.rows[(size_t)r * d], &packed.rows[(size_t)(r + 1) * d]);
    std::vector<ImageInfo> dbImages;
    dbImages.reserve((size_t)packed.n);
    for (int64_t r = 0; r < packed.n; ++r) dbImages.emplace_back(packed.class_no[(size_t)r], (int)r, feats[(size_t)r]);

    std::vector<float> dists;
    const int counted = fir::other_class_distances(dbImages, dists);
    std::streambuf* cout_buf = std::cout.rdbuf(nullptr);   // far_threshold prints what the reference prints (std::cout); stdout carries JSON here
    const float threshold = fir::far_threshold(dbImages, rate);
    std::cout.rdbuf(cout_buf);
    if (counted < 0) return 1;
    std::printf("{\n\"images\": %lld, \"counted\": %d, \"threshold\": %.9g,\n\"dists\": [", (long long)packed.n, counted, (double)threshold);
    for (size_t i = 0; i < dists.size(); ++i) std::printf("%s%.9g", i ? ", " : "", (double)dists[i]);
    std::printf("]\n}\n");
    return 0;
}
