// fir_eigen.cpp -- cyclic Jacobi for real symmetric matrices (fir_eigen.h).
#include "fir_eigen.h"

#include <algorithm>
#include <cmath>
#include <numeric>
#include <vector>

namespace fir {

int symmetric_eigen(const double* a, int d, double* values, double* vectors) {
    if (!a || !values || !vectors || d < 1) return -1;
    const size_t n = (size_t)d;
    std::vector<double> m(n * n), v(n * n, 0.0);        // m: the working matrix, kept symmetric; v: ROWS are the vectors so far
    for (size_t i = 0; i < n; ++i) {
        for (size_t j = i; j < n; ++j) m[i * n + j] = m[j * n + i] = a[i * n + j];
        v[i * n + i] = 1.0;
    }
    double norm2 = 0.0;
    for (double x : m) norm2 += x * x;
    int sweeps = 0;
    for (; sweeps < 64; ++sweeps) {
        double off = 0.0;
        for (size_t i = 0; i < n; ++i)
            for (size_t j = i + 1; j < n; ++j) off += 2.0 * m[i * n + j] * m[i * n + j];
        if (off <= norm2 * 1e-32 || off == 0.0) break;  // the off-diagonal part is below 1e-16 of the matrix in norm
        for (size_t p = 0; p + 1 < n; ++p)
            for (size_t q = p + 1; q < n; ++q) {
                const double apq = m[p * n + q];
                if (apq == 0.0) continue;
                // the rotation that zeroes m[p][q] (Golub & Van Loan, Algorithm 8.5.1: the smaller of the two angles)
                const double tau = (m[q * n + q] - m[p * n + p]) / (2.0 * apq);
                const double t = (tau >= 0.0 ? 1.0 : -1.0) / (std::fabs(tau) + std::sqrt(1.0 + tau * tau));
                const double c = 1.0 / std::sqrt(1.0 + t * t), s = t * c;
                for (size_t k = 0; k < n; ++k) {        // columns p and q ...
                    const double kp = m[k * n + p], kq = m[k * n + q];
                    m[k * n + p] = c * kp - s * kq;
                    m[k * n + q] = s * kp + c * kq;
                }
                for (size_t k = 0; k < n; ++k) {        // ... rows p and q, and the same rotation of the vectors
                    const double pk = m[p * n + k], qk = m[q * n + k];
                    m[p * n + k] = c * pk - s * qk;
                    m[q * n + k] = s * pk + c * qk;
                    const double vp = v[p * n + k], vq = v[q * n + k];
                    v[p * n + k] = c * vp - s * vq;
                    v[q * n + k] = s * vp + c * vq;
                }
                m[p * n + q] = m[q * n + p] = 0.0;
            }
    }
    std::vector<int> order(n);
    std::iota(order.begin(), order.end(), 0);
    std::stable_sort(order.begin(), order.end(), [&](int x, int y) { return m[(size_t)x * n + x] > m[(size_t)y * n + y]; });
    for (size_t k = 0; k < n; ++k) {
        const size_t src = (size_t)order[k];
        values[k] = m[src * n + src];
        const double* row = &v[src * n];
        double len2 = 0.0;
        size_t big = 0;
        for (size_t j = 0; j < n; ++j) {
            len2 += row[j] * row[j];
            if (std::fabs(row[j]) > std::fabs(row[big])) big = j;
        }
        const double scale = (row[big] < 0.0 ? -1.0 : 1.0) / std::sqrt(len2);
        for (size_t j = 0; j < n; ++j) vectors[k * n + j] = row[j] * scale;
    }
    return sweeps;
}

}  // namespace fir
