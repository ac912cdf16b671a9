// fir_pca.cpp -- fir_pca.h over the C ABI: no arithmetic proportional to the number of rows runs here.
#include "fir_pca.h"

#include <algorithm>
#include <cstdio>
#include <cstring>

#include "fir_eigen.h"

namespace fir {

namespace {
struct Projection {
    fir_projection* p = nullptr;
    ~Projection() { if (p) fir_projection_destroy(p); }
    bool make(const PcaModel& m) {
        return m.ok() && fir_projection_create(m.basis.data(), m.components, m.d, m.mean.data(), device(), &p) == FIR_OK;
    }
};
struct Handle {
    fir_gallery* g = nullptr;
    ~Handle() { if (g) fir_gallery_destroy(g); }
};
}  // namespace

PcaModel fit_pca(fir_gallery* g, const uint64_t* mask, int components) {
    PcaModel model;
    int32_t d = 0;
    if (!g || fir_gallery_info(g, nullptr, &d, nullptr, nullptr) != FIR_OK) { log_error("fit_pca"); return model; }
    if (components <= 0 || components > d) components = d;
    const size_t n = (size_t)d;
    std::vector<double> scatter(n * n), mean(n), values(n), vectors(n * n);
    int64_t count = 0;
    if (fir_gallery_scatter(g, mask, nullptr, scatter.data(), mean.data(), &count) != FIR_OK) { log_error("fit_pca: scatter"); return model; }
    if (count < 1) { std::fprintf(stderr, "fir: fit_pca: no training row\n"); return model; }
    if (symmetric_eigen(scatter.data(), d, values.data(), vectors.data()) < 0) return model;
    model.d = d;
    model.components = components;
    model.mean = mean;
    model.basis.assign(vectors.begin(), vectors.begin() + (size_t)components * n);
    model.values.resize((size_t)components);
    for (int k = 0; k < components; ++k) model.values[(size_t)k] = values[(size_t)k] / (double)count;
    return model;
}

PcaModel fit_pca(const std::vector<ImageInfo>& total, const std::vector<char>& take, int components, int max_features) {
    if (max_features == 0) max_features = FEATURES_COUNT;
    if (!take.empty() && take.size() != total.size()) {
        std::fprintf(stderr, "fir: fit_pca: %zu marks for %zu rows\n", take.size(), total.size());
        return PcaModel();
    }
    fir_gallery* g = total.empty() ? nullptr : GalleryCache::get(total, max_features);
    if (!g) { std::fprintf(stderr, "fir: fit_pca: no single-device upload of the gallery\n"); return PcaModel(); }
    std::vector<uint64_t> mask(FIR_MASK_WORDS(total.size()), 0);
    for (size_t j = 0; j < take.size(); ++j)
        if (take[j]) mask[j >> 6] |= (uint64_t)1 << (j & 63);
    return fit_pca(g, take.empty() ? nullptr : mask.data(), components);
}

fir_gallery* project_gallery(const PcaModel& model, const std::vector<ImageInfo>& total, int max_features) {
    if (max_features == 0) max_features = FEATURES_COUNT;
    fir_gallery* g = total.empty() ? nullptr : GalleryCache::get(total, max_features);
    Projection pr;
    fir_gallery* out = nullptr;
    if (!g || !pr.make(model) || fir_gallery_create_projected(g, pr.p, &out) != FIR_OK) { log_error("project_gallery"); return nullptr; }
    return out;
}

std::vector<FeaturesVector> project(const PcaModel& model, const std::vector<FeaturesVector>& queries) {
    std::vector<FeaturesVector> out;
    Projection pr;
    if (queries.empty()) return out;
    if (!pr.make(model)) { log_error("project"); return out; }
    const size_t d = (size_t)model.d, p = (size_t)model.components;
    std::vector<float> rows(queries.size() * d, 0.0f), res(queries.size() * p);
    for (size_t i = 0; i < queries.size(); ++i) std::memcpy(&rows[i * d], queries[i].data(), std::min(queries[i].size(), d) * sizeof(float));
    if (fir_projection_apply(pr.p, rows.data(), (int64_t)queries.size(), res.data()) != FIR_OK) { log_error("project"); return out; }
    out.reserve(queries.size());
    for (size_t i = 0; i < queries.size(); ++i) out.emplace_back(&res[i * p], &res[(i + 1) * p]);
    return out;
}

}  // namespace fir

void extractPCA(const ImagesDatabase& orig_database, ImagesDatabase& new_database) {
    size_t total = 0, d = 0;
    for (const auto& person : orig_database) {
        total += person.size();
        if (d == 0 && !person.empty()) d = person.front().size();
    }
    if (total == 0 || d == 0) return;
    std::vector<float> rows(total * d, 0.0f);
    size_t ind = 0;
    for (const auto& person : orig_database)
        for (const FeaturesVector& f : person) std::memcpy(&rows[ind++ * d], f.data(), std::min(f.size(), d) * sizeof(float));
    fir::Handle h;
    if (fir_gallery_create(rows.data(), (int64_t)total, (int32_t)d, nullptr, fir::metric(), fir::device(), &h.g) != FIR_OK) { fir::log_error("extractPCA"); return; }
    const fir::PcaModel model = fir::fit_pca(h.g, nullptr, 0);
    fir::Projection pr;
    fir::Handle projected;
    if (!pr.make(model) || fir_gallery_create_projected(h.g, pr.p, &projected.g) != FIR_OK ||
        fir_gallery_read_rows(projected.g, 0, (int64_t)total, rows.data(), nullptr) != FIR_OK) {
        fir::log_error("extractPCA");
        return;
    }
    ind = 0;
    new_database.reserve(orig_database.size());
    for (const auto& person : orig_database) {
        ImagesDatabase::value_type list;
        list.reserve(person.size());
        for (size_t i = 0; i < person.size(); ++i, ++ind) list.emplace_back(&rows[ind * d], &rows[(ind + 1) * d]);
        new_database.push_back(list);
    }
}
