// Stand-alone host program over csrc/fir_search_request.h: for every kind, batch size and K of the lists below it prints what the
// request says about sizes and layouts -- one line "kind qb k slots keys counts status radii" -- and checks the offset view at(q0)
// itself. tests/test_search_request.py builds it with the address and undefined-behaviour sanitizers, runs it and compares the
// lines with the formulas the library used before the request type existed. No device code, no library.
#include "../fast-image-recognition_amd/csrc/fir_search_request.h"

#include <cstdio>
#include <initializer_list>

#define REQUIRE(c)                                                          \
    do {                                                                    \
        if (!(c)) { std::printf("failed: %s (line %d)\n", #c, __LINE__); return 1; } \
    } while (0)

using fir::FirSearch;

static FirSearch make(int kind, int32_t k, uint64_t* keys, int32_t* classes, const float* radius, int32_t* count) {
    switch (kind) {
    case fir::kSearchRows: return FirSearch::rows(k, keys);
    case fir::kSearchSelect: return FirSearch::select(k, keys);
    case fir::kSearchRadius: return FirSearch::within(radius, k, count, keys);
    default: return FirSearch::distinct(11, k, keys, classes);
    }
}

int main() {
    constexpr int32_t kQ0Max = 1000, kKMaxHere = 1024;               // (the arrays reach as far as at(q0) points: one past the end at most)
    static uint64_t keys[(size_t)kQ0Max * kKMaxHere];
    static int32_t classes[(size_t)kQ0Max * kKMaxHere], count[kQ0Max];
    static float radius[kQ0Max];
    for (int kind = 0; kind < fir::kSearchKinds; ++kind)
        for (int32_t qb : {0, 1, 2, 3, 1024})
            for (int32_t k : {0, 1, 8, 9, 1024}) {
                if (k == 0 && kind != fir::kSearchRadius) continue;
                const FirSearch s = make(kind, k, keys, classes, radius, count);
                std::printf("%d %d %d %d %zu %zu %zu %zu\n", kind, qb, k, s.k, s.key_words(qb), s.count_words(qb), s.status_index(qb), s.radii_bytes(qb));
                // at(q0): keys and classes by q0 * k, radii and counts by q0; NULL stays NULL; kind, k and num_classes as they were
                for (int32_t q0 : {0, 1, 3, kQ0Max}) {
                    const FirSearch o = s.at(q0);
                    REQUIRE(o.kind == s.kind && o.k == k && o.num_classes == s.num_classes);
                    // (compared as integers)
                    REQUIRE((uintptr_t)o.keys == (uintptr_t)keys + (size_t)q0 * k * sizeof(uint64_t));
                    REQUIRE(s.classes ? (uintptr_t)o.classes == (uintptr_t)classes + (size_t)q0 * k * sizeof(int32_t) : o.classes == nullptr);
                    REQUIRE(s.radius ? (uintptr_t)o.radius == (uintptr_t)radius + (size_t)q0 * sizeof(float) : o.radius == nullptr);
                    REQUIRE(s.count ? (uintptr_t)o.count == (uintptr_t)count + (size_t)q0 * sizeof(int32_t) : o.count == nullptr);
                    const FirSearch none = make(kind, k, nullptr, nullptr, nullptr, nullptr).at(q0);
                    REQUIRE(!none.keys && !none.classes && !none.radius && !none.count);
                }
                REQUIRE((kind == fir::kSearchClasses) == (s.classes != nullptr) && (kind == fir::kSearchRadius) == (s.radius && s.count));
            }
    // which outputs may be NULL
    REQUIRE(FirSearch::rows(1, keys).outputs_ok() && !FirSearch::rows(1, nullptr).outputs_ok() && !FirSearch::select(9, nullptr).outputs_ok());
    REQUIRE(FirSearch::distinct(11, 3, nullptr, classes).outputs_ok() && FirSearch::distinct(11, 3, keys, nullptr).outputs_ok());
    REQUIRE(!FirSearch::distinct(11, 3, nullptr, nullptr).outputs_ok());
    REQUIRE(FirSearch::within(radius, 0, count, nullptr).outputs_ok() && !FirSearch::within(radius, 0, count, keys).outputs_ok());
    REQUIRE(FirSearch::within(radius, 9, count, keys).outputs_ok() && !FirSearch::within(radius, 9, count, nullptr).outputs_ok());
    REQUIRE(!FirSearch::within(radius, 9, nullptr, keys).outputs_ok());
    std::printf("ok\n");
    return 0;
}
