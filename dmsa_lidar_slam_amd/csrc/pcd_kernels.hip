// pcd_kernels.hip — the ASCII rows of PointCloud.pcd formatted on the device (layout and arithmetic: pcd_kernels.h).
#include "pcd_kernels.h"

namespace dmsa {

namespace {
constexpr int kDecodeBlock = 256;
// the workgroup's output span starts up to 3 bytes behind a dword boundary
constexpr int kRenderWords = (kPcdRenderBlock * kPcdMaxRowBytes + 3 + 3) / 4;

// One thread per row.  The seven conversions run as one loop (not unrolled: the conversion is a few hundred instructions); the value
// of a turn is picked from registers.
__global__ __launch_bounds__(kDecodeBlock) void k_pcd_decode(const float4* __restrict__ xyz, const float4* __restrict__ normal, const float* __restrict__ curvature,
                                                             int64_t n, uint64_t* __restrict__ dec, int32_t* __restrict__ len) {
    const int64_t i = (int64_t)blockIdx.x * kDecodeBlock + threadIdx.x;
    if (i > n) return;
    if (i == n) {
        len[n] = 0;
        return;
    }
    const float4 p = xyz[i], q = normal[i];
    const float c = curvature ? curvature[i] : 0.0f;
    int total = kPcdValues;  // six separators and the newline
#pragma unroll 1
    for (int j = 0; j < kPcdValues; ++j) {
        const float v = j == 0 ? p.x : j == 1 ? p.y : j == 2 ? p.z : j == 3 ? q.x : j == 4 ? q.y : j == 5 ? q.z : c;
        const uint64_t d = pcd_decode(__float_as_uint(v));
        dec[i * kPcdValues + j] = d;
        total += pcd_value_length(d);
    }
    len[i] = total;
}

// One workgroup per kPcdRenderBlock rows.  off[] is ascending with steps of at most kPcdMaxRowBytes (the scan of k_pcd_decode's
// lengths), so the workgroup's span [off[r0], off[r1]) is at most 256 x 105 bytes and every row lies inside the LDS image.
__global__ __launch_bounds__(kPcdRenderBlock) void k_pcd_render(const uint64_t* __restrict__ dec, const int32_t* __restrict__ off, int64_t n, char* __restrict__ text) {
    __shared__ uint32_t s_words[kRenderWords];
    char* s_bytes = reinterpret_cast<char*>(s_words);
    const int64_t r0 = (int64_t)blockIdx.x * kPcdRenderBlock;
    const int64_t r1 = r0 + kPcdRenderBlock < n ? r0 + kPcdRenderBlock : n;
    const int64_t i = r0 + threadIdx.x;
    const uint32_t begin = (uint32_t)off[r0], end = (uint32_t)off[r1];
    const uint32_t abegin = begin & ~3u;  // the LDS image starts at the dword that holds the span's first byte
    if (i < r1) {
        const uint32_t at = (uint32_t)off[i] - abegin;
        if (at + kPcdMaxRowBytes <= (uint32_t)sizeof(s_words)) {  // always true for offsets that come from the scan
            char* p = s_bytes + at;
#pragma unroll 1
            for (int j = 0; j < kPcdValues; ++j) {
                p = pcd_render_value(dec[i * kPcdValues + j], p);
                *p++ = j == kPcdValues - 1 ? '\n' : ' ';
            }
        }
    }
    __syncthreads();
    const uint32_t nbytes = end - abegin, lead = begin - abegin;
    if (nbytes > (uint32_t)sizeof(s_words)) return;  // (never, see above)
    const uint32_t w_first = lead ? 1u : 0u, w_end = nbytes >> 2;
    uint32_t* out_words = reinterpret_cast<uint32_t*>(text + abegin);
    for (uint32_t w = w_first + threadIdx.x; w < w_end; w += kPcdRenderBlock) out_words[w] = s_words[w];
    if (threadIdx.x < 4) {
        // head: the bytes of the first dword that belong to this span (the ones in front belong to the previous workgroup's)
        const uint32_t h = threadIdx.x;
        if (lead && h >= lead && h < nbytes) text[abegin + h] = s_bytes[h];
        // tail: the bytes behind the last whole dword
        const uint32_t t = 4u * (w_end > w_first ? w_end : w_first) + threadIdx.x;
        if (t < nbytes) text[abegin + t] = s_bytes[t];
    }
}
}  // namespace

void launch_pcd_decode(const float4* xyz, const float4* normal, const float* curvature, int64_t n, uint64_t* dec, int32_t* len, hipStream_t s) {
    if (n <= 0 || n > kPcdMaxChunkRows) return;
    hipLaunchKernelGGL(k_pcd_decode, dim3((unsigned)((n + 1 + kDecodeBlock - 1) / kDecodeBlock)), dim3(kDecodeBlock), 0, s, xyz, normal, curvature, n, dec, len);
}
void launch_pcd_render(const uint64_t* dec, const int32_t* off, int64_t n, char* text, hipStream_t s) {
    if (n <= 0 || n > kPcdMaxChunkRows) return;
    hipLaunchKernelGGL(k_pcd_render, dim3((unsigned)((n + kPcdRenderBlock - 1) / kPcdRenderBlock)), dim3(kPcdRenderBlock), 0, s, dec, off, n, text);
}

}  // namespace dmsa
