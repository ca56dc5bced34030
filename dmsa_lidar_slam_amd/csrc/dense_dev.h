// dense_dev.h — what the kernel files of the dense cloud share (dense_cloud.hip, dense_grid.hip, dense_normals.hip, dense_outliers.hip,
// dense_carve.hip), each stated once: the workgroup size, its launch arithmetic and the hash of both open-addressing tables.
#pragma once
#include <hip/hip_runtime.h>

namespace dmsa {

constexpr int kBlock = 256;

inline unsigned blocks_for(unsigned long long n) { return (unsigned)((n + kBlock - 1) / kBlock); }

__device__ __forceinline__ unsigned long long mix64(unsigned long long x) {  // the finaliser of MurmurHash3
    x ^= x >> 33;
    x *= 0xff51afd7ed558ccdull;
    x ^= x >> 33;
    x *= 0xc4ceb9fe1a85ec53ull;
    x ^= x >> 33;
    return x;
}

}  // namespace dmsa
