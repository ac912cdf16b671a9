// fir_eigen.h -- the eigen-decomposition of a real symmetric matrix, plain C++ with no dependency: what cv::eigen / cv::PCA do
// with the d x d covariance matrix in the reference (classification.cpp:864-940, db_features.cpp:218-315). Everything proportional
// to the number of rows runs on the device (fir_gallery_scatter, fir_projection); this is the d x d rest.
#pragma once

namespace fir {

// a[d][d] row-major, symmetric (only the upper triangle a[i][j], i <= j, is read). values[d] <- the eigenvalues, descending, equal
// ones in the order of their index; vectors[d][d] <- the unit eigenvectors as ROWS, vectors[k] belonging to values[k] (OpenCV's
// eigenvectors layout). The sign of a vector is fixed: its component of largest magnitude is positive, the first such on ties.
// Cyclic Jacobi in double: O(d^3) a sweep, a handful of sweeps; meant for a few hundred features. Returns the number of sweeps,
// -1 when d < 1 or a pointer is NULL.
int symmetric_eigen(const double* a, int d, double* values, double* vectors);

}  // namespace fir
