// fir_db.h -- host-side mirror of the reference's data model and match entry points
// (qt_cpp/db_features.h, qt_cpp/db.h), backed by the MI355X library through its C ABI
// (include/fir_amd.h). Source-compatible with the reference's callers: the same type names,
// function names, argument order and defaults, the same "-1 means not found" convention.
//
// What differs, by design:
//   * distances are computed on the GPU: recognize_image_bf packs the borrowed gallery views into
//     one row-major block, uploads it (cached per gallery vector, see GalleryCache) and runs the
//     scan kernel; feature_distance runs a one-lane kernel. There is no host arithmetic path.
//   * batched overloads (recognize_images_bf) are added: one gallery pass serves 8 queries.
#ifndef FIR_DB_H
#define FIR_DB_H

#include <cstdint>
#include <map>
#include <string>
#include <unordered_map>
#include <vector>

#include "../../include/fir_amd.h"

// qt_cpp/db.h:79-91 -- the reference fixes the feature dimension at compile time.
#ifndef FEATURES_COUNT
#define FEATURES_COUNT 1536
#endif
// qt_cpp/db.h:71-78 (Caltech build)
#ifndef FIR_FRACTION
#define FIR_FRACTION 0.03
#endif
#ifndef DB_H   // the reference's own db.h (pure configuration, qt_cpp/db.h:1-2), when included first, already defines FRACTION
const double FRACTION = FIR_FRACTION;
#endif

// qt_cpp/db_features.h:12 -- compile-time metric switch, kept as a macro and mapped to the
// runtime enum: define FIR_USE_CHI2 or FIR_USE_KL to get the other arms of db_features.cpp:25-39.
#if defined(FIR_USE_KL)
#define FIR_DEFAULT_METRIC FIR_METRIC_KL
#elif defined(FIR_USE_CHI2)
#define FIR_DEFAULT_METRIC FIR_METRIC_CHI2
#else
#define USE_L2_DISTANCE
#define FIR_DEFAULT_METRIC FIR_METRIC_L2
#endif

typedef std::vector<float> FeaturesVector;                              // db_features.h:14
typedef std::vector<std::vector<FeaturesVector> > ImagesDatabase;       // db_features.h:15

// db_features.h:17, db_features.cpp:22-42
float feature_distance(const FeaturesVector& lhs, const FeaturesVector& rhs, int start_pos = 0, int end_pos = FEATURES_COUNT);

// db_features.h:19-29 -- a non-owning view of one image's features.
class ImageInfo {
public:
    ImageInfo(int no, int ind, const FeaturesVector& feat) : classNo(no), indexInDatabase(ind), features(feat) {}
    float distance(const ImageInfo& rhs, int start_pos = 0, int end_pos = FEATURES_COUNT) const {
        return feature_distance(features, rhs.features, start_pos, end_pos);
    }
    const int classNo, indexInDatabase;
    const FeaturesVector& features;
};

// db_features.h:31, db_features.cpp:44-116 -- text feature file -> database (class-major).
int loadImages(ImagesDatabase& imagesDb, std::string features_file, std::unordered_map<std::string, int>& person2indexMap,
               bool early_stop = false);
// db_features.h:32, db_features.cpp:117-162
void getTrainingAndTestImages(const ImagesDatabase& totalImages, std::vector<ImageInfo>& dbImages,
                              std::vector<ImageInfo>& testImages, bool randomize = true);
// db_features.h:33, db_features.cpp:319-335 -- row index of the nearest gallery image or -1.
int recognize_image_bf(const std::vector<ImageInfo>& dbImages, const ImageInfo& testImageInfo, int max_features = 0);

// video.cpp:21,35-96 -- person -> videos -> frames of the YouTube-Faces feature file. The reference hard-wires the
// file name (video.cpp:23-33); it is a defaulted argument here.
typedef std::map<std::string, std::vector<std::vector<FeaturesVector> > > MapOfVideos;
void loadVideos(MapOfVideos& dbVideos, const std::string& video_features_file = "vgg_mean_dnn_features.txt");

namespace fir {

// Batched form of recognize_image_bf: out[i] = row index for tests[i] (or -1). One call costs
// ceil(n / 8) gallery passes instead of n.
std::vector<int> recognize_images_bf(const std::vector<ImageInfo>& dbImages, const std::vector<ImageInfo>& tests,
                                     int max_features = 0, std::vector<float>* best_dist = nullptr);

// The random-split loop of the reference's experiments (testRecognitionMethod, ImageTesting.cpp:445-466: TESTS splits of one image
// set by getTrainingAndTestImages) without one upload per split: dbImages is the TOTAL set, uploaded once through GalleryCache, and
// take[j] != 0 marks the rows of this split's training side (take.size() == dbImages.size()). out[i] = the index INTO dbImages of
// the nearest row of tests[i] among them (first minimum in row order), -1 without one -- fir_search_top1_masked, n / 8 bytes per
// split. Single device only: with fir::set_devices in force it logs an error and returns -1 for every test.
std::vector<int> recognize_images_bf_subset(const std::vector<ImageInfo>& dbImages, const std::vector<char>& take,
                                            const std::vector<ImageInfo>& tests, int max_features = 0, std::vector<float>* best_dist = nullptr);

// One whole split of that loop on the device, over the same cached upload of the TOTAL set: the gallery is the subset handle of
// the take[j] != 0 rows (fir_gallery_create_subset: compacted inside device memory, so the search may take every routed form, the
// matrix cores included), the queries are ALL the other rows, taken out of the upload in batches (fir_gallery_rows_of_mask of the
// inverted mask + fir_gallery_gather_rows_dev), searched with fir_search_top1_keys_dev and mapped back with fir_keys_to_origin_dev.
// out[i] = the index INTO total of the nearest taken row of the i-th test row (test rows ascending; *test_rows, when asked for, =
// their indices into total), -1 without one -- the answers recognize_images_bf_subset gives for the same split and test rows. No
// upload beyond the cached one (GalleryCache::uploads() does not move for a cached set); the subset handle lives for the call and
// costs the taken rows' bytes a second time while it does. Single device only, like the masked form.
std::vector<int> recognize_split_bf(const std::vector<ImageInfo>& total, const std::vector<char>& take, int max_features = 0,
                                    std::vector<float>* best_dist = nullptr, std::vector<int>* test_rows = nullptr);

// The device copy of one `std::vector<ImageInfo>` gallery. The reference's classifiers only keep
// a pointer to the caller's vector (ImageTesting.cpp:40, ann.h:28) and read it afresh on every call; here the rows are
// packed and uploaded on first use and the handle is reused while the SAME gallery is presented again, which is checked
// on every lookup: the vector object, its size and a signature over EVERY row's feature pointer, length and classNo
// (any reallocation, reorder or relabel re-uploads at once), plus a 64-bit hash of all feature bytes taken at upload
// time and re-verified per fir::set_cache_validation -- by default whenever 20 ms have passed since the entry was last
// verified, so an in-place edit of any row is caught by the next run over the gallery, and a tight loop of per-image
// calls pays a few per cent. fir::invalidate(dbImages) forces the re-upload immediately (train() calls it).
class GalleryCache {
public:
    static fir_gallery* get(const std::vector<ImageInfo>& dbImages, int dim);
    static void invalidate(const std::vector<ImageInfo>& dbImages);
    // Rows [old_n, dbImages.size()) were pushed back onto a vector the cache holds: every single-device upload of it that still
    // matches the first old_n rows (size, signature, content hash) gets only the new rows (fir_gallery_append) and its size,
    // signature and hash refreshed; an upload that is sharded, or whose first old_n rows were edited, reordered or relabelled, is
    // dropped, and the next lookup uploads the whole vector as ever. Returns the number of uploads that were extended in place.
    static int appended(const std::vector<ImageInfo>& dbImages, size_t old_n);
    // Whole-gallery uploads made so far in this process (an in-place extension by appended() is not one).
    static long uploads();
    static void clear();
};
inline void invalidate(const std::vector<ImageInfo>& dbImages) { GalleryCache::invalidate(dbImages); }

// Galleries uploaded from now on: fir_gallery_set_large_batch_mfma(min_queries). The library's default (-1) already sends
// whole-range L2 batches of >= 128 test images against >= 65536 rows (fewer on larger galleries) through the matrix-core path (same answers);
// > 0 sets another threshold, 0 switches the path off.
void set_large_batch_mfma(int min_queries);
void set_device(int device);   // default 0
// Several GPUs: galleries uploaded from now on are split by rows over `devices` (one shard each, or shards_per_device
// logical shards each) and recognize_image(s)_bf / BruteForce / BruteForceClassifier scan all shards at once; the nearest
// row over the whole gallery is the integer minimum of the shards' packed keys, reduced by RCCL inside libfir_amd.so
// (fir_sharded_search_top1). An empty list (or one device, one shard) is the single-device path on fir::device().
void set_devices(const std::vector<int>& devices, int shards_per_device = 1);
// How often a cached upload's CONTENT is re-verified against the caller's rows (see GalleryCache).
enum { FIR_CACHE_VALIDATE_NEVER = 0, FIR_CACHE_VALIDATE_THROTTLED = 1, FIR_CACHE_VALIDATE_ALWAYS = 2 };
void set_cache_validation(int mode);   // default FIR_CACHE_VALIDATE_THROTTLED
int device();
int metric();                  // FIR_DEFAULT_METRIC unless set_metric was called
void set_metric(int metric);

// Thrown by nothing: errors are reported the reference's way (-1 / empty) and logged to stderr.
void log_error(const char* where);

}  // namespace fir

#endif  // FIR_DB_H
