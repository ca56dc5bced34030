// pcd_kernels.h — the ASCII rows of PointCloud.pcd on the device (include/dmsa_wire_formats.h: dmsa_format_pcd_rows, dmsa_save_pcd_ascii).
// A row is "x y z normal_x normal_y normal_z curvature\n", every value as C's printf("%.8g", (double)v): 8 significant digits, EXACTLY
// rounded (ties to even on the binary value).  Doubles cannot do that; the conversion below holds the exact value as a multi-limb
// integer: |v| = m * 2^e with a 24-bit m and e in [-149, 104], so
//   e >= 0   the integer m << e has at most 128 bits: 4 limbs, peeled into base-10^9 groups by division (at most 5 groups);
//   e <  0   the integer part m >> -e is below 2^24, the fraction is a 160-bit fixed-point number (5 limbs) whose multiplication by
//            10^9 pushes the next nine decimal digits out of the top limb (the smallest denormal, 1.4e-45, shows its first digit in the
//            fifth group; one more group decides the rounding: 6 steps at most).
// The first non-zero group A, the group B behind it and "anything non-zero further down" give the 8 digits and the exact comparison of
// the remainder with one half.  Every loop has a constant bound.
//
// Two kernels per chunk of rows, the project's prefix scan between them:
//   k_pcd_decode   one thread per row: seven values -> seven packed decimals (8 BCD digits, decimal exponent, sign, class) + the row's length;
//   (exclusive_scan_i32 over the lengths: row offsets, the chunk's byte count behind the last row)
//   k_pcd_render   one workgroup per 256 rows: every thread writes its row's characters into the workgroup's LDS image of its contiguous
//                  output span, then the workgroup stores the span as dwords (head and tail bytes singly).
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define DMSA_PCD_HD __host__ __device__ __forceinline__
#else
#define DMSA_PCD_HD inline
#endif

namespace dmsa {

constexpr int kPcdValues = 7;          // x y z normal_x normal_y normal_z curvature
constexpr int kPcdMaxValueChars = 14;  // "-1.1754944e-38"
constexpr int kPcdMaxRowBytes = kPcdValues * kPcdMaxValueChars + (kPcdValues - 1) + 1;  // 105
constexpr int kPcdRenderBlock = 256;   // rows per workgroup of k_pcd_render: 256 x 105 B = 26.25 KiB of LDS, five workgroups (20 waves) per CU
constexpr int64_t kPcdMaxChunkRows = (int64_t)1 << 24;  // row offsets inside a chunk are int32: 2^24 x 105 < 2^31

// A decoded value: bits 0-31 eight BCD digits (most significant digit in the top nibble, never 0 for a finite non-zero value),
// bits 32-39 decimal exponent + 64, bit 40 sign, bits 41-42 class.
enum : uint32_t { kPcdFinite = 0, kPcdZero = 1, kPcdInf = 2, kPcdNan = 3 };
DMSA_PCD_HD uint64_t pcd_pack(uint32_t bcd, int x10, uint32_t neg, uint32_t cls) {
    return (uint64_t)bcd | ((uint64_t)(uint32_t)(x10 + 64) << 32) | ((uint64_t)neg << 40) | ((uint64_t)cls << 41);
}
DMSA_PCD_HD uint32_t pcd_pow10(int k) {  // k = 0 .. 9
    switch (k) {
        case 0: return 1u;
        case 1: return 10u;
        case 2: return 100u;
        case 3: return 1000u;
        case 4: return 10000u;
        case 5: return 100000u;
        case 6: return 1000000u;
        case 7: return 10000000u;
        case 8: return 100000000u;
        default: return 1000000000u;
    }
}

// the bits of a float -> its packed "%.8g" decimal
DMSA_PCD_HD uint64_t pcd_decode(uint32_t u) {
    const uint32_t neg = u >> 31, ex = (u >> 23) & 255u, fr = u & 0x7FFFFFu;
    if (ex == 255u) return fr ? pcd_pack(0u, 0, 0u, kPcdNan) : pcd_pack(0u, 0, neg, kPcdInf);
    if (ex == 0u && fr == 0u) return pcd_pack(0u, 0, neg, kPcdZero);
    const uint32_t m = ex ? (fr | 0x800000u) : fr;
    const int e = (ex ? (int)ex : 1) - 150;  // |v| = m * 2^e
    uint32_t A = 0u, B = 0u;  // first non-zero base-10^9 group and the one behind it
    bool sticky = false;      // a non-zero digit behind B
    int x10;                  // decimal exponent of A's last digit's group: the leading digit's exponent is x10 + digits(A) - 1
    if (e >= 0) {
        uint32_t L[4] = {0u, 0u, 0u, 0u};
        const int w = e >> 5;
        const uint64_t v = (uint64_t)m << (e & 31);
#pragma unroll
        for (int k = 0; k < 4; ++k) L[k] = k == w ? (uint32_t)v : (k == w + 1 ? (uint32_t)(v >> 32) : 0u);
        uint32_t g[5];
#pragma unroll
        for (int j = 0; j < 5; ++j) {
            uint64_t rem = 0u;
#pragma unroll
            for (int k = 3; k >= 0; --k) {
                const uint64_t cur = (rem << 32) | L[k];
                L[k] = (uint32_t)(cur / 1000000000u);
                rem = cur % 1000000000u;
            }
            g[j] = (uint32_t)rem;
        }
        int t = -1;
#pragma unroll
        for (int j = 4; j >= 0; --j) {
            if (t < 0) {
                if (g[j] != 0u) t = j, A = g[j];
            } else if (t == j + 1) {
                B = g[j];
            } else {
                sticky = sticky || g[j] != 0u;
            }
        }
        x10 = 9 * t;
    } else {
        const int s = -e;  // 1 .. 149
        const uint32_t I = s < 24 ? m >> s : 0u;
        const uint32_t f = s < 24 ? m & ((1u << s) - 1u) : m;
        uint32_t L[5] = {0u, 0u, 0u, 0u, 0u};  // fraction * 2^160
        const int sh = 160 - s, w = sh >> 5;
        const uint64_t v = (uint64_t)f << (sh & 31);
#pragma unroll
        for (int k = 0; k < 5; ++k) L[k] = k == w ? (uint32_t)v : (k == w + 1 ? (uint32_t)(v >> 32) : 0u);
        bool haveA = I != 0u, haveB = false;
        A = I, x10 = 0;
#pragma unroll 1
        for (int j = 1; j <= 6; ++j) {
            if (haveB) break;
            uint32_t carry = 0u;
#pragma unroll
            for (int k = 0; k < 5; ++k) {
                const uint64_t cur = (uint64_t)L[k] * 1000000000u + carry;
                L[k] = (uint32_t)cur;
                carry = (uint32_t)(cur >> 32);
            }
            if (haveA) {
                B = carry, haveB = true;
            } else if (carry != 0u) {
                A = carry, haveA = true, x10 = -9 * j;
            }
        }
        sticky = (L[0] | L[1] | L[2] | L[3] | L[4]) != 0u;
    }
    int d = 1;
#pragma unroll
    for (int k = 1; k <= 8; ++k) d += A >= pcd_pow10(k) ? 1 : 0;
    x10 += d - 1;
    uint32_t q;
    bool up;
    if (d <= 8) {
        const uint32_t p = pcd_pow10(d + 1), r = B % p, half = 5u * pcd_pow10(d);
        q = A * pcd_pow10(8 - d) + B / p;
        up = r > half || (r == half && (sticky || (q & 1u)));
    } else {
        const uint32_t r = A % 10u;
        q = A / 10u;
        up = r > 5u || (r == 5u && (B != 0u || sticky || (q & 1u)));
    }
    q += up ? 1u : 0u;
    if (q == 100000000u) q = 10000000u, x10 += 1;
    uint32_t bcd = 0u;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        bcd |= (q % 10u) << (4 * k);
        q /= 10u;
    }
    return pcd_pack(bcd, x10, neg, kPcdFinite);
}

// significant digits left after the trailing zeros are removed (finite non-zero values: the top nibble is not 0)
DMSA_PCD_HD int pcd_num_digits(uint32_t bcd) {
    int nd = 8;
#pragma unroll
    for (int k = 0; k < 7; ++k) {
        if ((bcd & 15u) != 0u) break;
        bcd >>= 4, --nd;
    }
    return nd;
}

// characters of a packed value
DMSA_PCD_HD int pcd_value_length(uint64_t dec) {
    const uint32_t cls = (uint32_t)(dec >> 41) & 3u, neg = (uint32_t)(dec >> 40) & 1u;
    if (cls == kPcdZero) return 1 + (int)neg;
    if (cls != kPcdFinite) return 3 + (int)neg;
    const int X = (int)((dec >> 32) & 255u) - 64, nd = pcd_num_digits((uint32_t)dec);
    if (X < -4 || X >= 8) return (int)neg + (nd > 1 ? nd + 1 : 1) + 4;  // d[.ddd]e+XX
    if (X >= 0) return (int)neg + (nd > X + 1 ? nd + 1 : X + 1);       // ddd[.ddd]
    return (int)neg + 1 - X + nd;                                      // 0.000ddd
}

// writes the characters of a packed value at p, returns the position behind them
template <class CharPtr>
DMSA_PCD_HD CharPtr pcd_render_value(uint64_t dec, CharPtr p) {
    const uint32_t cls = (uint32_t)(dec >> 41) & 3u, neg = (uint32_t)(dec >> 40) & 1u, bcd = (uint32_t)dec;
    if (neg) *p++ = '-';
    if (cls == kPcdZero) {
        *p++ = '0';
        return p;
    }
    if (cls == kPcdInf) {
        *p++ = 'i', *p++ = 'n', *p++ = 'f';
        return p;
    }
    if (cls == kPcdNan) {
        *p++ = 'n', *p++ = 'a', *p++ = 'n';
        return p;
    }
    const int X = (int)((dec >> 32) & 255u) - 64, nd = pcd_num_digits(bcd);
    auto digit = [bcd](int i) { return (char)('0' + ((bcd >> (4 * (7 - i))) & 15u)); };  // i = 0: the leading digit
    if (X < -4 || X >= 8) {
        *p++ = digit(0);
        if (nd > 1) {
            *p++ = '.';
            for (int i = 1; i < 8; ++i)
                if (i < nd) *p++ = digit(i);
        }
        const int ax = X < 0 ? -X : X;
        *p++ = 'e', *p++ = X < 0 ? '-' : '+', *p++ = (char)('0' + ax / 10), *p++ = (char)('0' + ax % 10);
    } else if (X >= 0) {
        for (int i = 0; i < 8; ++i) {
            if (i == X + 1 && nd > X + 1) *p++ = '.';
            if (i <= X || i < nd) *p++ = digit(i);
        }
    } else {
        *p++ = '0', *p++ = '.';
        for (int i = 1; i < 4; ++i)
            if (i < -X) *p++ = '0';
        for (int i = 0; i < 8; ++i)
            if (i < nd) *p++ = digit(i);
    }
    return p;
}

#if defined(__HIPCC__)
// rows 0 .. n-1 of a chunk (n <= kPcdMaxChunkRows): xyz / normal n x 4 floats (the fourth is not read), curvature n floats or null (= 0);
// dec: 7 n packed values, len: n + 1 row lengths in bytes (len[n] = 0, so that an exclusive scan over n + 1 entries ends with the total)
void launch_pcd_decode(const float4* xyz, const float4* normal, const float* curvature, int64_t n, uint64_t* dec, int32_t* len, hipStream_t s);
// off: the exclusive scan of len (n + 1 entries); text: off[n] bytes, 4-byte aligned
void launch_pcd_render(const uint64_t* dec, const int32_t* off, int64_t n, char* text, hipStream_t s);
#endif

}  // namespace dmsa
