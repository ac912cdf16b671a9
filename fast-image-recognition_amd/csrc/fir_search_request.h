// fir_search_request.h -- what one search call is looking for, as one plain value that fir_capi.hip, fir_gemm.hip and fir_shard.hip pass down and ask for
// sizes and layouts. A new kind is a new enum value, one table row per layer (fir_gemm.hip: kGemmKinds) and an exact form. Plain C++17, no HIP runtime.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include "../../include/fir_amd.h"

namespace fir {
enum SearchKind : int {
    kSearchRows = 0,    // the K nearest rows, list form: top-1 / top-K, 1 <= k <= 8
    kSearchSelect,      // the K nearest rows, select form (fir_search_knn): 1 <= k <= FIR_KNN_MAX, matrix cores up to FIR_GEMM_KNN_MAX
    kSearchRadius,      // every row within radius[q]: k = max_results, 0 <= k <= FIR_KNN_MAX (0: counts only), count[q] out
    kSearchClasses,     // the K nearest distinct classes: 1 <= k <= 32 of num_classes; keys and / or classes out
    kSearchKinds,       // the kinds above: the ones fir_gemm.hip answers itself (kGemmKinds has a row for each)
    // the nearest row of a class other than exclude[q] (fir_search_top1_other_class): k = 1. No matrix-core row of its own: a routed batch is
    // kSearchClasses with k = 2 and a pick (fir_capi.hip: other_class_routed)
    kSearchOtherClass = kSearchKinds
};
struct FirSearch {
    SearchKind kind;
    int32_t k;                  // slots per query
    int32_t num_classes;        // kSearchClasses
    uint64_t* keys;             // [qb * k], ascending per query; NULL: radius with k = 0, classes when only classes are asked for
    int32_t* classes;           // kSearchClasses: [qb * k]; may be NULL when keys is not
    const float* radius;        // kSearchRadius: [qb]
    int32_t* count;             // kSearchRadius: [qb] <- the rows inside, however many
    const int32_t* exclude;     // kSearchOtherClass: [qb], the class each query passes over
    // the rows that take part (fir_amd.h, "searches over a subset of the rows"): FIR_MASK_WORDS(n) words, NULL = every row. Last, with a
    // default: the factories and every older aggregate initialisation leave it NULL; masked() sets it
    const uint64_t* mask = nullptr;
    FirSearch masked(const uint64_t* m) const { FirSearch s = *this; s.mask = m; return s; }
    static FirSearch rows(int32_t k, uint64_t* keys) { return {kSearchRows, k, 0, keys, nullptr, nullptr, nullptr, nullptr}; }
    static FirSearch select(int32_t k, uint64_t* keys) { return {kSearchSelect, k, 0, keys, nullptr, nullptr, nullptr, nullptr}; }
    static FirSearch within(const float* radius, int32_t max_results, int32_t* count, uint64_t* keys) { return {kSearchRadius, max_results, 0, keys, nullptr, radius, count, nullptr}; }
    static FirSearch distinct(int32_t num_classes, int32_t k, uint64_t* keys, int32_t* classes) { return {kSearchClasses, k, num_classes, keys, classes, nullptr, nullptr, nullptr}; }
    static FirSearch other_class(const int32_t* exclude, uint64_t* keys) { return {kSearchOtherClass, 1, 0, keys, nullptr, nullptr, nullptr, exclude}; }
    bool is_radius() const { return kind == kSearchRadius; }
    // which outputs may be NULL: keys only where the kind has another output (the counts alone for k = 0; the classes)
    bool outputs_ok() const { return is_radius() ? count && (k == 0 ? !keys : keys != nullptr) : keys || (kind == kSearchClasses && classes); }
    // the sharded exchange's payload of one rank, in 64-bit words: qb * k keys, then the counts (two per word), then the status element
    size_t key_words(int32_t qb) const { return (size_t)qb * k; }
    size_t count_words(int32_t qb) const { return is_radius() ? ((size_t)qb + 1) / 2 : 0; }
    size_t status_index(int32_t qb) const { return key_words(qb) + count_words(qb); }
    // the radii riding behind a batch of queries, in whole 8 bytes
    size_t radii_bytes(int32_t qb) const { return is_radius() ? ((size_t)qb + (qb & 1)) * sizeof(float) : 0; }
    // ... and the excluded classes, the same way
    size_t exclude_bytes(int32_t qb) const { return kind == kSearchOtherClass ? ((size_t)qb + (qb & 1)) * sizeof(int32_t) : 0; }
    // the same request for queries [q0, ...): every pointer it has, advanced by its stride
    FirSearch at(int32_t q0) const {
        return {kind, k, num_classes, keys ? keys + (size_t)q0 * k : nullptr, classes ? classes + (size_t)q0 * k : nullptr, radius ? radius + q0 : nullptr, count ? count + q0 : nullptr,
                exclude ? exclude + q0 : nullptr, mask};
    }
};
}  // namespace fir
