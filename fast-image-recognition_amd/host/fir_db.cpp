// fir_db.cpp -- host side of the drop-in (see fir_db.h). IO, packing and handle caching only:
// every distance is computed by libfir_amd.so on the GPU.
#include "fir_db.h"

#include <iostream>
#include "fir_loader.h"

#include <hip/hip_runtime_api.h>      // recognize_split_bf's device buffers: memory and one stream, no kernel of its own

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <map>
#include <sstream>
#include <tuple>

namespace fir {

namespace {
int g_device = 0;
int g_metric = FIR_DEFAULT_METRIC;
int g_large_batch = -1;
std::vector<int> g_devices;          // more than one entry (or g_shards_per_device > 1): galleries are row-sharded (fir_sharded_*)
int g_shards_per_device = 1;
int g_validation = FIR_CACHE_VALIDATE_THROTTLED;
long g_uploads = 0;                  // GalleryCache::uploads

// One uploaded gallery. What identifies the caller's `std::vector<ImageInfo>` is checked on EVERY lookup: the vector
// object, its size, and a signature over every row's (feature pointer, length, classNo) -- any reallocation, reorder or
// relabel is seen at once. What the rows CONTAIN is a 64-bit hash of all feature bytes taken at upload time; it is
// re-verified on a lookup when the policy says so (fir::set_cache_validation): always, never, or -- the default -- when
// at least 20 ms have passed since this entry was last verified, so that a loop of per-image recognize() calls (the
// reference's own pattern, ~35 us each) pays a few per cent for it while an edit made between two runs is caught.
struct Entry {
    const void* vec = nullptr;
    size_t n = 0;
    int dim = 0, metric = 0;
    uint64_t signature = 0, content = 0;
    std::chrono::steady_clock::time_point verified;
    fir_gallery* g = nullptr;
    fir_sharded* s = nullptr;
};
std::vector<Entry> g_cache;

inline uint64_t mix(uint64_t h, uint64_t v) {
    h ^= v * 0x9E3779B97F4A7C15ull;
    h = (h << 27) | (h >> 37);
    return h * 0x94D049BB133111EBull + 0x632BE59BD9B4E019ull;
}

// (count: the leading rows the value covers -- all of them, or the rows an entry held before push_backs: GalleryCache::appended)
uint64_t signature_of(const std::vector<ImageInfo>& db, size_t count) {
    uint64_t h = 0x243F6A8885A308D3ull ^ count;
    for (size_t j = 0; j < count; ++j) {
        const ImageInfo& im = db[j];
        h = mix(h, (uint64_t)(uintptr_t)im.features.data());
        h = mix(h, ((uint64_t)im.features.size() << 32) ^ (uint32_t)im.classNo);
    }
    return h;
}

uint64_t content_of(const std::vector<ImageInfo>& db, int dim, size_t count) {
    uint64_t h[4] = {1, 2, 3, 4};                              // four independent lanes: the multiplies overlap
    for (size_t j = 0; j < count; ++j) {
        const ImageInfo& im = db[j];
        const size_t have = std::min<size_t>(im.features.size(), (size_t)dim);
        const float* f = im.features.data();
        size_t k = 0;
        for (; k + 8 <= have; k += 8) {
            uint64_t w[4];
            std::memcpy(w, f + k, 32);
            h[0] = mix(h[0], w[0]); h[1] = mix(h[1], w[1]); h[2] = mix(h[2], w[2]); h[3] = mix(h[3], w[3]);
        }
        for (; k < have; ++k) { uint32_t w; std::memcpy(&w, f + k, 4); h[k & 3] = mix(h[k & 3], w); }
    }
    return mix(mix(h[0], h[1]), mix(h[2], h[3]));
}

void drop(Entry& e) {
    if (e.g) fir_gallery_destroy(e.g);
    if (e.s) fir_sharded_destroy(e.s);
    e.g = nullptr;
    e.s = nullptr;
}

// rows [first, db.size()) as one row-major block of `dim` floats each (rows shorter than dim are zero padded) and their classes
void pack_rows(const std::vector<ImageInfo>& db, size_t first, int dim, std::vector<float>& rows, std::vector<int32_t>& cls) {
    rows.assign((db.size() - first) * (size_t)dim, 0.0f);
    cls.resize(db.size() - first);
    for (size_t j = first; j < db.size(); ++j) {
        const FeaturesVector& f = db[j].features;
        const size_t have = std::min<size_t>(f.size(), (size_t)dim);
        std::memcpy(&rows[(j - first) * dim], f.data(), have * sizeof(float));
        cls[j - first] = db[j].classNo;
    }
}

bool sharded_mode() { return g_devices.size() > 1 || g_shards_per_device > 1; }

// The entry for (db, dim) under the current metric / device set, uploaded if it is not there or no longer valid.
Entry* lookup(const std::vector<ImageInfo>& db, int dim) {
    const uint64_t sig = signature_of(db, db.size());
    const auto now = std::chrono::steady_clock::now();
    for (size_t i = 0; i < g_cache.size(); ++i) {
        Entry& e = g_cache[i];
        if (e.vec != (const void*)&db || e.dim != dim || e.metric != g_metric || (e.s != nullptr) != sharded_mode()) continue;
        bool valid = e.n == db.size() && e.signature == sig;
        if (valid && (g_validation == FIR_CACHE_VALIDATE_ALWAYS ||
                      (g_validation == FIR_CACHE_VALIDATE_THROTTLED && now - e.verified >= std::chrono::milliseconds(20)))) {
            valid = content_of(db, dim, db.size()) == e.content;
            e.verified = std::chrono::steady_clock::now();
        }
        if (valid) return &e;
        drop(e);                                                 // a different split (or edited rows) behind the same vector object
        g_cache.erase(g_cache.begin() + (long)i);
        break;
    }
    // every other upload of this vector with these features is stale too if the rows changed; uploads of other widths are
    // checked when they are looked up
    std::vector<float> rows;
    std::vector<int32_t> cls;
    pack_rows(db, 0, dim, rows, cls);
    Entry e;
    e.vec = &db; e.n = db.size(); e.dim = dim; e.metric = g_metric; e.signature = sig;
    e.content = content_of(db, dim, db.size());
    e.verified = std::chrono::steady_clock::now();
    if (sharded_mode()) {
        std::vector<int32_t> devs(g_devices.begin(), g_devices.end());
        if (devs.empty()) devs.push_back(g_device);
        fir_shard_opts o;
        std::memset(&o, 0, sizeof o);
        o.struct_bytes = (int32_t)sizeof o;
        o.shards_per_device = g_shards_per_device;
        if (fir_gallery_create_sharded_ex(rows.data(), (int64_t)db.size(), dim, cls.data(), g_metric, devs.data(), (int32_t)devs.size(), &o, &e.s) != FIR_OK) {
            log_error("sharded gallery upload");
            return nullptr;
        }
        if (g_large_batch >= 0) {
            int32_t nsh = 0;
            fir_sharded_info(e.s, nullptr, nullptr, nullptr, &nsh, nullptr, nullptr);
            for (int32_t i = 0; i < nsh; ++i) {
                fir_gallery* part = nullptr;
                if (fir_sharded_shard(e.s, i, &part, nullptr, nullptr) == FIR_OK && part) fir_gallery_set_large_batch_mfma(part, g_large_batch);
            }
        }
    } else {
        if (fir_gallery_create(rows.data(), (int64_t)db.size(), dim, cls.data(), g_metric, g_device, &e.g) != FIR_OK) {
            log_error("gallery upload");
            return nullptr;
        }
        if (g_large_batch >= 0) fir_gallery_set_large_batch_mfma(e.g, g_large_batch);
    }
    ++g_uploads;
    g_cache.push_back(e);
    return &g_cache.back();
}
}  // namespace

void set_large_batch_mfma(int min_queries) { g_large_batch = min_queries; }
void set_device(int device) { g_device = device; }
void set_devices(const std::vector<int>& devices, int shards_per_device) {
    GalleryCache::clear();
    g_devices = devices;
    g_shards_per_device = shards_per_device > 0 ? shards_per_device : 1;
    if (!devices.empty()) g_device = devices[0];
}
void set_cache_validation(int mode) { g_validation = mode; }
int device() { return g_device; }
int metric() { return g_metric; }
void set_metric(int m) { g_metric = m; }
void log_error(const char* where) { std::fprintf(stderr, "fir: %s: %s\n", where, fir_last_error()); }

fir_gallery* GalleryCache::get(const std::vector<ImageInfo>& db, int dim) {
    // the single-device handle (TWD classifiers, DirectedEnumeration): always on fir::device(), whatever set_devices said
    const std::vector<int> devs = g_devices;
    const int spd = g_shards_per_device;
    g_devices.clear();
    g_shards_per_device = 1;
    Entry* e = lookup(db, dim);
    g_devices = devs;
    g_shards_per_device = spd;
    return e ? e->g : nullptr;
}

void GalleryCache::invalidate(const std::vector<ImageInfo>& db) {
    for (size_t i = 0; i < g_cache.size();) {
        if (g_cache[i].vec == (const void*)&db) { drop(g_cache[i]); g_cache.erase(g_cache.begin() + (long)i); } else ++i;
    }
}

int GalleryCache::appended(const std::vector<ImageInfo>& db, size_t old_n) {
    int extended = 0;
    for (size_t i = 0; i < g_cache.size();) {
        Entry& e = g_cache[i];
        if (e.vec != (const void*)&db) { ++i; continue; }
        // in place: a single-device upload of exactly the first old_n rows as they are now (the vector may have reallocated: the views
        // it holds still point at the same features); anything else is dropped and uploaded again by the next lookup
        bool ok = e.g && !e.s && e.n == old_n && old_n <= db.size() && e.signature == signature_of(db, old_n) && e.content == content_of(db, e.dim, old_n);
        if (ok && db.size() > old_n) {
            std::vector<float> rows;
            std::vector<int32_t> cls;
            pack_rows(db, old_n, e.dim, rows, cls);
            ok = fir_gallery_append(e.g, rows.data(), (int64_t)cls.size(), cls.data()) == FIR_OK;
            if (!ok) log_error("gallery append");
        }
        if (!ok) { drop(e); g_cache.erase(g_cache.begin() + (long)i); continue; }
        e.n = db.size();
        e.signature = signature_of(db, db.size());
        e.content = content_of(db, e.dim, db.size());
        e.verified = std::chrono::steady_clock::now();
        ++extended;
        ++i;
    }
    return extended;
}

long GalleryCache::uploads() { return g_uploads; }

void GalleryCache::clear() {
    for (Entry& e : g_cache) drop(e);
    g_cache.clear();
}

std::vector<int> recognize_images_bf(const std::vector<ImageInfo>& dbImages, const std::vector<ImageInfo>& tests,
                                     int max_features, std::vector<float>* best_dist) {
    if (max_features == 0) max_features = FEATURES_COUNT;          // db_features.cpp:320-321
    std::vector<int> out(tests.size(), -1);
    if (best_dist) best_dist->assign(tests.size(), FIR_NOT_FOUND_DIST);
    if (tests.empty() || dbImages.empty()) return out;
    // the gallery is uploaded with as many features as the scan reads
    const int dim = max_features;
    Entry* e = lookup(dbImages, dim);
    if (!e) return out;
    std::vector<float> q((size_t)tests.size() * dim, 0.0f);
    for (size_t i = 0; i < tests.size(); ++i) {
        const FeaturesVector& f = tests[i].features;
        std::memcpy(&q[i * dim], f.data(), std::min<size_t>(f.size(), (size_t)dim) * sizeof(float));
    }
    std::vector<int32_t> idx(tests.size());
    std::vector<float> dist(tests.size());
    // several devices: every shard scans the batch, RCCL reduces the packed keys inside the library (fir_sharded_search_top1)
    const int rc = e->s ? fir_sharded_search_top1(e->s, q.data(), (int32_t)tests.size(), 0, max_features, idx.data(), dist.data())
                        : fir_search_top1(e->g, q.data(), (int32_t)tests.size(), 0, max_features, idx.data(), dist.data());
    if (rc != FIR_OK) {
        log_error("search_top1");
        return out;
    }
    for (size_t i = 0; i < tests.size(); ++i) out[i] = idx[i];
    if (best_dist) *best_dist = dist;
    return out;
}

std::vector<int> recognize_images_bf_subset(const std::vector<ImageInfo>& dbImages, const std::vector<char>& take,
                                            const std::vector<ImageInfo>& tests, int max_features, std::vector<float>* best_dist) {
    if (max_features == 0) max_features = FEATURES_COUNT;          // db_features.cpp:320-321
    std::vector<int> out(tests.size(), -1);
    if (best_dist) best_dist->assign(tests.size(), FIR_NOT_FOUND_DIST);
    if (tests.empty() || dbImages.empty()) return out;
    if (take.size() != dbImages.size()) {
        std::fprintf(stderr, "fir: recognize_images_bf_subset: %zu marks for %zu rows\n", take.size(), dbImages.size());
        return out;
    }
    if (sharded_mode()) {
        std::fprintf(stderr, "fir: recognize_images_bf_subset: no masked search on a sharded gallery\n");
        return out;
    }
    const int dim = max_features;
    Entry* e = lookup(dbImages, dim);
    if (!e) return out;
    std::vector<uint64_t> mask(FIR_MASK_WORDS(dbImages.size()), 0);
    for (size_t j = 0; j < take.size(); ++j)
        if (take[j]) mask[j >> 6] |= (uint64_t)1 << (j & 63);
    std::vector<float> q((size_t)tests.size() * dim, 0.0f);
    for (size_t i = 0; i < tests.size(); ++i) {
        const FeaturesVector& f = tests[i].features;
        std::memcpy(&q[i * dim], f.data(), std::min<size_t>(f.size(), (size_t)dim) * sizeof(float));
    }
    std::vector<int32_t> idx(tests.size());
    std::vector<float> dist(tests.size());
    if (fir_search_top1_masked(e->g, q.data(), (int32_t)tests.size(), 0, max_features, mask.data(), idx.data(), dist.data()) != FIR_OK) {
        log_error("search_top1_masked");
        return out;
    }
    for (size_t i = 0; i < tests.size(); ++i) out[i] = idx[i];
    if (best_dist) *best_dist = dist;
    return out;
}

namespace {
// what recognize_split_bf holds on the device for the length of one call
struct DevMem {
    void* p = nullptr;
    ~DevMem() { if (p) (void)hipFree(p); }
    bool alloc(size_t bytes) { return hipMalloc(&p, bytes ? bytes : 16) == hipSuccess; }
};
struct DevStream {
    hipStream_t s = nullptr;
    ~DevStream() { if (s) (void)hipStreamDestroy(s); }
};
struct SubsetHandle {
    fir_gallery* g = nullptr;
    ~SubsetHandle() { if (g) fir_gallery_destroy(g); }
};
}  // namespace

std::vector<int> recognize_split_bf(const std::vector<ImageInfo>& total, const std::vector<char>& take, int max_features,
                                    std::vector<float>* best_dist, std::vector<int>* test_rows) {
    if (max_features == 0) max_features = FEATURES_COUNT;          // db_features.cpp:320-321
    if (test_rows) test_rows->clear();
    if (best_dist) best_dist->clear();
    if (take.size() != total.size()) {
        std::fprintf(stderr, "fir: recognize_split_bf: %zu marks for %zu rows\n", take.size(), total.size());
        return std::vector<int>();
    }
    size_t tests = 0;
    for (size_t j = 0; j < take.size(); ++j) tests += take[j] == 0;
    std::vector<int> out(tests, -1);
    if (best_dist) best_dist->assign(tests, FIR_NOT_FOUND_DIST);
    if (test_rows)
        for (size_t j = 0; j < take.size(); ++j)
            if (!take[j]) test_rows->push_back((int)j);
    if (tests == 0 || tests == total.size()) return out;           // no test row, or no gallery row to find
    if (sharded_mode()) {
        std::fprintf(stderr, "fir: recognize_split_bf: no subset of a sharded gallery\n");
        return out;
    }
    const int dim = max_features;
    Entry* e = lookup(total, dim);
    if (!e) return out;
    std::vector<uint64_t> train(FIR_MASK_WORDS(total.size()), 0), test(FIR_MASK_WORDS(total.size()), 0);
    for (size_t j = 0; j < take.size(); ++j) (take[j] ? train : test)[j >> 6] |= (uint64_t)1 << (j & 63);
    // the split's gallery: the `take` rows compacted inside device memory (the mask is the only thing that goes up) ...
    SubsetHandle sub;
    if (fir_gallery_create_subset(e->g, train.data(), &sub.g) != FIR_OK) { log_error("create_subset"); return out; }
    if (g_large_batch >= 0) fir_gallery_set_large_batch_mfma(sub.g, g_large_batch);
    // ... and its queries: the complement rows, listed by the inverted mask and taken out of the same upload in batches
    std::vector<int32_t> rows(tests);
    int64_t count = 0;
    if (fir_gallery_rows_of_mask(e->g, test.data(), rows.data(), (int64_t)tests, &count) != FIR_OK || count != (int64_t)tests) {
        log_error("rows_of_mask");
        return out;
    }
    const size_t batch = std::min<size_t>(tests, 8192);
    DevMem d_idx, d_q, d_keys;
    DevStream st;
    if (hipSetDevice(g_device) != hipSuccess || hipStreamCreateWithFlags(&st.s, hipStreamNonBlocking) != hipSuccess || !d_idx.alloc(tests * sizeof(int32_t)) ||
        !d_q.alloc(batch * (size_t)dim * sizeof(float)) || !d_keys.alloc(batch * sizeof(uint64_t)) ||
        hipMemcpyAsync(d_idx.p, rows.data(), tests * sizeof(int32_t), hipMemcpyHostToDevice, st.s) != hipSuccess) {
        std::fprintf(stderr, "fir: recognize_split_bf: no device memory for %zu test rows\n", tests);
        return out;
    }
    std::vector<uint64_t> keys(batch);
    std::vector<int32_t> idx(batch);
    std::vector<float> dist(batch);
    for (size_t b0 = 0; b0 < tests; b0 += batch) {
        const size_t nb = std::min(batch, tests - b0);
        // one stream for the three calls: they are calls on two handles, and only a stream orders those
        if (fir_gallery_gather_rows_dev(e->g, (const int32_t*)d_idx.p + b0, (int64_t)nb, (float*)d_q.p, nullptr, st.s) != FIR_OK ||
            fir_search_top1_keys_dev(sub.g, (const float*)d_q.p, (int32_t)nb, 0, max_features, (uint64_t*)d_keys.p, st.s) != FIR_OK ||
            fir_keys_to_origin_dev(sub.g, (uint64_t*)d_keys.p, (int64_t)nb, st.s) != FIR_OK) {
            log_error("split search");
            return std::vector<int>(tests, -1);
        }
        if (hipMemcpyAsync(keys.data(), d_keys.p, nb * sizeof(uint64_t), hipMemcpyDeviceToHost, st.s) != hipSuccess || hipStreamSynchronize(st.s) != hipSuccess) {
            std::fprintf(stderr, "fir: recognize_split_bf: reading the keys back failed\n");
            return std::vector<int>(tests, -1);
        }
        fir_keys_unpack(keys.data(), (int32_t)nb, idx.data(), dist.data());
        for (size_t i = 0; i < nb; ++i) {
            out[b0 + i] = idx[i];
            if (best_dist) (*best_dist)[b0 + i] = dist[i];
        }
    }
    return out;                                                    // (the subset handle and the buffers go here)
}

}  // namespace fir

float feature_distance(const FeaturesVector& lhs, const FeaturesVector& rhs, int start_pos, int end_pos) {
    float d = 0.0f;
    const int len = (int)std::min(lhs.size(), rhs.size());
    if (fir_feature_distance(lhs.data(), rhs.data(), len, start_pos, end_pos, fir::metric(), fir::device(), &d) != FIR_OK) {
        fir::log_error("feature_distance");
        return std::nanf("");
    }
    return d;
}

int recognize_image_bf(const std::vector<ImageInfo>& dbImages, const ImageInfo& testImageInfo, int max_features) {
    std::vector<ImageInfo> one(1, testImageInfo);
    return fir::recognize_images_bf(dbImages, one, max_features)[0];
}

// ---- feature file: "<path>\n<class>\n<f0> <f1> ... \n" per image (dnn_feature_extractor.py:58-64) ----
// db_features.cpp:44-116 through the fast packed loader (fir_loader.cpp: memory-mapped, threaded, exact float
// parsing; rows bit-identical to the reference's -- tests/test_host_loader.py), then scattered into the
// reference's ImagesDatabase shape.
int loadImages(ImagesDatabase& imagesDb, std::string features_file, std::unordered_map<std::string, int>& person2indexMap,
               bool /*early_stop*/) {
    person2indexMap.clear();
    fir::PackedFeatures packed;
    const int64_t total = fir::load_features_packed(features_file, FEATURES_COUNT, fir::metric(), packed);
    if (total <= 0) return 0;                                        // silently empty, db_features.cpp:49,115
    const size_t first_new = imagesDb.size();                        // the reference appends to whatever the caller passed
    imagesDb.resize(first_new + packed.class_names.size());
    for (size_t c = 0; c < packed.class_names.size(); ++c) person2indexMap.emplace(packed.class_names[c], (int)c);
    for (int64_t r = 0; r < packed.n; ++r) {
        const float* src = &packed.rows[(size_t)r * FEATURES_COUNT];
        imagesDb[first_new + (size_t)packed.class_no[(size_t)r]].emplace_back(src, src + FEATURES_COUNT);
    }
    double avg_count = 0;                                            // db_features.cpp:107-112
    for (size_t i = 0; i < imagesDb.size(); ++i) avg_count += (double)imagesDb[i].size();
    avg_count /= (double)imagesDb.size();
    std::cout << "total size=" << imagesDb.size() << " totalImages=" << total << " avg_count=" << avg_count << std::endl;
    return (int)total;
}

// video.cpp:35-96 through fir_loader's exact parser. Entries are (re)built the way the reference's map ends up:
// a repeated person name re-sizes and overwrites the earlier entry's videos.
void loadVideos(MapOfVideos& dbVideos, const std::string& video_features_file) {
    fir::PackedVideos pv;
    if (fir::load_videos_packed(video_features_file, FEATURES_COUNT, fir::metric(), pv) <= 0) return;
    for (size_t p = 0; p < pv.person.size(); ++p) {
        std::vector<std::vector<FeaturesVector> >& videos = dbVideos[pv.person[p]];
        videos.clear();
        for (int32_t v = pv.video_first[p]; v < pv.video_first[p + 1]; ++v) {
            videos.emplace_back();
            for (int64_t r = pv.frame_first[(size_t)v]; r < pv.frame_first[(size_t)v + 1]; ++r)
                videos.back().emplace_back(&pv.rows[(size_t)r * FEATURES_COUNT], &pv.rows[(size_t)(r + 1) * FEATURES_COUNT]);
        }
    }
    std::cout << "total size=" << dbVideos.size() << " totalVideos=" << pv.total_videos << " totalImages=" << pv.total_images << std::endl;   // :92
}

void getTrainingAndTestImages(const ImagesDatabase& totalImages, std::vector<ImageInfo>& dbImages,
                              std::vector<ImageInfo>& testImages, bool randomize) {
    const int kIndices = 400;                                        // db_features.cpp:119
    int order[kIndices];
    for (int i = 0; i < kIndices; ++i) order[i] = i;
    if (randomize) {
        // what std::random_shuffle(first, last) does in libstdc++ (removed from C++17): rand()-driven swaps
        for (int i = 1; i < kIndices; ++i) {
            const int j = std::rand() % (i + 1);
            if (i != j) std::swap(order[i], order[j]);
        }
    }
    dbImages.clear();
    testImages.clear();
    int base = 0;
    for (size_t c = 0; c < totalImages.size(); ++c) {
        const int count = (int)totalImages[c].size();
#ifndef FIR_SPLIT_BY_FRACTION
        int gallery_size = 30;                                       // Caltech rule, :132-133
#else
        float want = count * FRACTION;                               // :135-142
        int gallery_size = (int)std::ceil(want);
        if (gallery_size == count) gallery_size = count - 1;
        if (gallery_size == 0) gallery_size = 1;
#endif
        int taken = 0;
        for (int i = 0; i < kIndices; ++i) {
            if (order[i] >= count) continue;
            ImageInfo view((int)c, base + order[i], totalImages[c][order[i]]);
            (taken < gallery_size ? dbImages : testImages).push_back(view);
            ++taken;
        }
        base += count;
    }
}
