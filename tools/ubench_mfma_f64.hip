// Micro-benchmark (gfx950): sustained rate of v_mfma_f64_16x16x4_f64 -- the roof of the matrix-core PNN (csrc/fir_cls_pnn_mfma.h).
// One launch fills the chip; every wave runs 8 independent accumulator tiles (64 VGPRs), no memory traffic inside the loop.
// The clock held is read in the kernel: delta s_memtime (shader cycles) / delta s_memrealtime (100 MHz), median over waves.
// Build: hipcc --offload-arch=gfx950 -O3 -o ubench_mfma_f64 tools/ubench_mfma_f64.hip
// Run:   ./ubench_mfma_f64 [warm-up seconds, default 2]
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <vector>

typedef double d4 __attribute__((ext_vector_type(4)));
constexpr int kTiles = 8;        // independent accumulators per wave: two rounds of them hide the instruction's latency

__global__ void __launch_bounds__(256) k_mfma_f64(double* out, unsigned long long* stamps, int iters, double s) {
    d4 acc[kTiles];
    const double a = 1.0 + (double)(threadIdx.x & 63) * s, b = 0.5 - (double)(threadIdx.x >> 2) * s;     // non-trivial operands: the power draw is part of the answer
#pragma unroll
    for (int i = 0; i < kTiles; ++i) acc[i] = (d4){(double)i, 0.0, 0.0, 0.0};
    const unsigned long long t0 = __builtin_amdgcn_s_memtime(), r0 = __builtin_amdgcn_s_memrealtime();
    for (int it = 0; it < iters; ++it) {
#pragma unroll
        for (int i = 0; i < kTiles; ++i) acc[i] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, acc[i], 0, 0, 0);
#pragma unroll
        for (int i = 0; i < kTiles; ++i) acc[i] = __builtin_amdgcn_mfma_f64_16x16x4f64(b, a, acc[i], 0, 0, 0);
    }
    const unsigned long long t1 = __builtin_amdgcn_s_memtime(), r1 = __builtin_amdgcn_s_memrealtime();
    double sum = 0.0;
#pragma unroll
    for (int i = 0; i < kTiles; ++i) sum += acc[i][0] + acc[i][1] + acc[i][2] + acc[i][3];
    const size_t gid = (size_t)blockIdx.x * 256 + threadIdx.x;
    out[gid] = sum;
    if ((threadIdx.x & 63) == 0) {
        stamps[(gid >> 6) * 2] = t1 - t0;
        stamps[(gid >> 6) * 2 + 1] = r1 - r0;
    }
}

#define CHECK(x)                                                                                    \
    do {                                                                                            \
        hipError_t e_ = (x);                                                                        \
        if (e_ != hipSuccess) { std::fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e_)); return 1; } \
    } while (0)

int main(int argc, char** argv) {
    const double warm_s = argc > 1 ? std::atof(argv[1]) : 2.0;
    hipDeviceProp_t p;
    CHECK(hipGetDeviceProperties(&p, 0));
    const int cus = p.multiProcessorCount, iters = 8192;
    std::printf("device %s, %d CUs, nominal clock %d kHz\n", p.gcnArchName, cus, p.clockRate);
    const int max_blocks = cus * 4;                      // up to 4 waves per SIMD
    double* out;
    unsigned long long* stamps;
    CHECK(hipMalloc((void**)&out, (size_t)max_blocks * 256 * sizeof(double)));
    CHECK(hipMalloc((void**)&stamps, (size_t)max_blocks * 4 * 2 * sizeof(unsigned long long)));
    hipEvent_t e0, e1;
    CHECK(hipEventCreate(&e0));
    CHECK(hipEventCreate(&e1));
    for (int wps = 1; wps <= 4; wps *= 2) {
        const int blocks = cus * wps;                    // a block of 256 threads = one wave on every SIMD of a compute unit
        const auto w0 = std::chrono::steady_clock::now();
        do {                                             // back-to-back launches until the clock has settled under this load
            hipLaunchKernelGGL(k_mfma_f64, dim3(blocks), dim3(256), 0, 0, out, stamps, iters, 1e-3);
            CHECK(hipDeviceSynchronize());
        } while (std::chrono::duration<double>(std::chrono::steady_clock::now() - w0).count() < warm_s);
        std::vector<double> tf, ghz;
        for (int rep = 0; rep < 7; ++rep) {
            CHECK(hipEventRecord(e0));
            hipLaunchKernelGGL(k_mfma_f64, dim3(blocks), dim3(256), 0, 0, out, stamps, iters, 1e-3);
            CHECK(hipEventRecord(e1));
            CHECK(hipEventSynchronize(e1));
            float ms;
            CHECK(hipEventElapsedTime(&ms, e0, e1));
            const double mfmas = (double)blocks * 4 * iters * 2 * kTiles;            // wave-level instructions, 16*16*4*2 flops each
            tf.push_back(mfmas * 2048.0 / (ms * 1e-3) / 1e12);
            std::vector<unsigned long long> h((size_t)blocks * 4 * 2);
            CHECK(hipMemcpy(h.data(), stamps, h.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost));
            std::vector<double> clk;
            for (size_t w = 0; w < h.size() / 2; ++w)
                if (h[2 * w + 1]) clk.push_back((double)h[2 * w] / (double)h[2 * w + 1] * 0.1);      // GHz
            std::sort(clk.begin(), clk.end());
            ghz.push_back(clk.empty() ? 0.0 : clk[clk.size() / 2]);
        }
        std::sort(tf.begin(), tf.end());
        std::sort(ghz.begin(), ghz.end());
        const double t = tf[tf.size() / 2], g = ghz[ghz.size() / 2];
        // cycles one instruction occupies a SIMD's matrix pipe: flops per cycle and SIMD -> 2048 / that
        const double cyc = g > 0 ? 2048.0 / (t * 1e12 / (g * 1e9) / (cus * 4.0)) : 0.0;
        std::printf("waves/SIMD=%d  v_mfma_f64_16x16x4_f64: %.2f TFLOP/s median of 7 (%.2f..%.2f), clock held %.3f GHz (%.3f..%.3f), %.1f cycles per instruction and SIMD\n",
                    wps, t, tf.front(), tf.back(), g, ghz.front(), ghz.back(), cyc);
    }
    return 0;
}
