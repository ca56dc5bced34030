// wave_prims.h — device helpers every kernel file may use, each stated once: wave64 lane movement and reductions, and the point
// arithmetic whose operation order is the reference's (a kernel that rounds differently from another breaks bit parity).
// Device-only, everything __forceinline__: a kernel compiles to the same instructions as with the helper written out beside it.
#pragma once
#include <hip/hip_runtime.h>

namespace dmsa {

// ------------------------------------------------------------------------------------------------------------
// wave64 helpers
// ------------------------------------------------------------------------------------------------------------
// DPP (data-parallel primitive) lane movement keeps wave-wide sums in the VALU instead of round trips through the LDS
// crossbar (ds_bpermute): row_shr:1/2/4/8 inside each 16-lane row, then row_bcast:15 / row_bcast:31 across rows (gfx9).
template <int kCtrl, int kRowMask>
__device__ __forceinline__ float dpp_mov(float v) {
    return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), kCtrl, kRowMask, 0xf, true));
}
template <int kCtrl, int kRowMask>
__device__ __forceinline__ int dpp_mov(int v) {
    return __builtin_amdgcn_update_dpp(0, v, kCtrl, kRowMask, 0xf, true);
}
template <int kCtrl, int kRowMask>
__device__ __forceinline__ double dpp_mov(double v) {
    const int lo = __builtin_amdgcn_update_dpp(0, __double2loint(v), kCtrl, kRowMask, 0xf, true);
    const int hi = __builtin_amdgcn_update_dpp(0, __double2hiint(v), kCtrl, kRowMask, 0xf, true);
    return __hiloint2double(hi, lo);
}
template <class T>
__device__ __forceinline__ T wave_incl_scan_dpp(T v) {
    v += dpp_mov<0x111, 0xf>(v);  // row_shr:1
    v += dpp_mov<0x112, 0xf>(v);  // row_shr:2
    v += dpp_mov<0x114, 0xf>(v);  // row_shr:4
    v += dpp_mov<0x118, 0xf>(v);  // row_shr:8
    v += dpp_mov<0x142, 0xa>(v);  // row_bcast:15 -> rows 1 and 3
    v += dpp_mov<0x143, 0xc>(v);  // row_bcast:31 -> rows 2 and 3
    return v;
}
__device__ __forceinline__ float wave_allsum(float v) {
    v = wave_incl_scan_dpp(v);
    return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 63));
}
__device__ __forceinline__ double wave_allsum(double v) {
    v = wave_incl_scan_dpp(v);
    return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(v), 63), __builtin_amdgcn_readlane(__double2loint(v), 63));
}
// butterfly sum over the 64 lanes: every lane ends with the same bits (each step adds the same two partial sums, in either order).
// NOT wave_allsum: that one adds the lanes as a scan, another summation order and so other bits
template <class T>  // double, unsigned long long
__device__ __forceinline__ T wave_sum(T v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}
__device__ __forceinline__ int wave_allmin(int v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v = min(v, __shfl_xor(v, m));
    return v;
}
__device__ __forceinline__ int wave_allmax(int v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v = max(v, __shfl_xor(v, m));
    return v;
}
__device__ __forceinline__ float wave_allminf(float v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v = fminf(v, __shfl_xor(v, m));
    return v;
}
__device__ __forceinline__ float wave_allmaxf(float v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v = fmaxf(v, __shfl_xor(v, m));
    return v;
}
__device__ __forceinline__ float bcast_lane(float v, int k) { return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), k)); }
__device__ __forceinline__ double readlane_f64(double v, int lane) {
    const int lo = __builtin_amdgcn_readlane(__double2loint(v), lane), hi = __builtin_amdgcn_readlane(__double2hiint(v), lane);
    return __hiloint2double(hi, lo);
}
// LDS barrier that leaves global loads in flight (a __syncthreads() also waits for vmcnt(0), which would serialise a prefetch from
// global memory with every phase)
__device__ __forceinline__ void lds_barrier() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }

// ------------------------------------------------------------------------------------------------------------
// point arithmetic in the reference's (Eigen 3.4's) operation order
// ------------------------------------------------------------------------------------------------------------
// Matrix4f * Vector4f with w == 1, evaluated column-wise like Eigen's packet product: ((c0*x + c1*y) + c2*z) + c3
__device__ __forceinline__ float3 apply_row3(const float4 r0, const float4 r1, const float4 r2, const float x, const float y, const float z) {
    float3 g;
    g.x = ((r0.x * x + r0.y * y) + r0.z * z) + r0.w;
    g.y = ((r1.x * x + r1.y * y) + r1.z * z) + r1.w;
    g.z = ((r2.x * x + r2.y * y) + r2.z * z) + r2.w;
    return g;
}
// Eigen's redux of three terms (Matrix3f * Vector3f coefficients, squaredNorm of a Vector3f): x0 + (x1 + x2)
__device__ __forceinline__ float sum3f(float a, float b, float c) { return a + (b + c); }

}  // namespace dmsa
