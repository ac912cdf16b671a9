// fir_pca.h -- PCA over the device primitives of include/fir_amd.h ("linear projection / PCA"): the reference's
// extract_pca_features (classification.cpp:864-940) and extractPCA (db_features.cpp:218-315) without OpenCV. Everything proportional
// to the number of rows runs on the device (fir_gallery_scatter, fir_projection, fir_gallery_create_projected); the eigen-decomposition
// of the d x d scatter matrix runs on the host (fir_eigen.h).
#ifndef FIR_PCA_H
#define FIR_PCA_H

#include <vector>

#include "fir_db.h"

namespace fir {

// mean[d]; basis[components][d] row-major, rows = unit eigenvectors of the covariance, leading first (OpenCV's eigenvectors layout);
// values[components] = the eigenvalues of the covariance matrix scatter / count (cv::PCA's convention), descending.
struct PcaModel {
    int d = 0, components = 0;
    std::vector<double> mean, basis, values;
    bool ok() const { return components > 0; }
};

// Fits on the rows of `total` with take[j] != 0 (as in recognize_split_bf; an empty `take` = every row): the upload is GalleryCache's,
// the scatter matrix the device's, the eigen solve the host's. components 0 = all d of them. max_features 0 = FEATURES_COUNT.
// Single device only. On an error it logs and returns a model with ok() == false.
PcaModel fit_pca(const std::vector<ImageInfo>& total, const std::vector<char>& take, int components = 0, int max_features = 0);
// fit_pca on a handle the caller holds (mask: FIR_MASK_WORDS(n) host words or NULL).
PcaModel fit_pca(fir_gallery* g, const uint64_t* mask, int components = 0);

// The projected gallery of `total` (its cached upload mapped on the device: labels, metric and row offset carried). The handle is
// the caller's: fir_gallery_destroy it. NULL on an error (logged).
fir_gallery* project_gallery(const PcaModel& model, const std::vector<ImageInfo>& total, int max_features = 0);
// queries[i] -> its model.components projected features, through the same kernel (the same bits as the projected gallery's rows).
std::vector<FeaturesVector> project(const PcaModel& model, const std::vector<FeaturesVector>& queries);

}  // namespace fir

// db_features.h:34, the #else form of db_features.cpp:272-315: PCA fitted on every image of the database, all components kept,
// every image projected; classes and images in the same order. The feature count is the first image's (the reference's
// FEATURES_COUNT); with fewer images than features the trailing components belong to zero eigenvalues (cv::PCA drops them).
void extractPCA(const ImagesDatabase& orig_database, ImagesDatabase& new_database);

#endif  // FIR_PCA_H
