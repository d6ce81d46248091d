// Host-side layout helpers of the closed loop (ftmpc_loop.hip): the caller's per-vehicle arrays are vehicle-major [B][K], the loop
// kernels read component-major [K][B].  Plain C++ with no HIP include, so that a stand-alone program can compile and test them.
#pragma once

#include <algorithm>
#include <cstdint>

namespace ftmpc {

// dst [K][B] = src [B][K]^T, 64 vehicles at a time so that each of the K write streams fills whole cache lines
inline void pack_kb(const double* src, int64_t B, int64_t K, double* dst) {
    for (int64_t b0 = 0; b0 < B; b0 += 64) {
        const int64_t b1 = std::min(B, b0 + 64);
        for (int64_t k = 0; k < K; ++k)
            for (int64_t b = b0; b < b1; ++b) dst[k * B + b] = src[b * K + k];
    }
}

// dst [B][K] = src [K][B]^T: the way back, blocked the same way
inline void unpack_kb(const double* src, int64_t B, int64_t K, double* dst) {
    for (int64_t b0 = 0; b0 < B; b0 += 64) {
        const int64_t b1 = std::min(B, b0 + 64);
        for (int64_t k = 0; k < K; ++k)
            for (int64_t b = b0; b < b1; ++b) dst[b * K + k] = src[k * B + b];
    }
}

}  // namespace ftmpc
