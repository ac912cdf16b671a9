// Stand-alone driver of host/fir_eigen.cpp for tests/test_pca_eigen.py: reads "d" and d*d doubles (row-major) per matrix from stdin
// until end of file, prints for each the sweep count, then d eigenvalues, then the d x d eigenvectors (rows), "%.17g" each.
// The lower triangle handed to symmetric_eigen is poisoned: only the upper one may be read.
#include <cmath>
#include <cstdio>
#include <vector>

#include "../fast-image-recognition_amd/host/fir_eigen.h"

int main() {
    int d;
    while (std::scanf("%d", &d) == 1) {
        if (d < 1 || d > 4096) return 2;
        const size_t n = (size_t)d;
        std::vector<double> a(n * n), values(n), vectors(n * n);
        for (double& x : a)
            if (std::scanf("%lf", &x) != 1) return 3;
        for (size_t i = 0; i < n; ++i)
            for (size_t j = 0; j < i; ++j) a[i * n + j] = std::nan("");
        const int sweeps = fir::symmetric_eigen(a.data(), d, values.data(), vectors.data());
        if (sweeps < 0) return 4;
        std::printf("%d\n", sweeps);
        for (double x : values) std::printf("%.17g\n", x);
        for (double x : vectors) std::printf("%.17g\n", x);
    }
    if (fir::symmetric_eigen(nullptr, 1, nullptr, nullptr) != -1) return 5;
    std::printf("ok\n");
    return 0;
}
