// dense_align_plane_solve.cpp — the host-only side of include/dmsa_dense_align_plane.h: the defaults, P3's exact
// re-centring of the 64 sums in 128-bit integers, P4's scaled LDL^T step and P5's measures.  No device, no context.  Built with
// -ffp-contract=off: every operation below is rounded on its own, in the order written, and tests/dense_align_plane_model.py repeats them
// in Python floats bit for bit.
#include "../../include/dmsa_dense_align_plane.h"

#include <cmath>

namespace {

typedef __int128 i128;

// P2's order
enum { W_N = 0, W_NO_NORMAL = 1, W_SP = 2, W_NN = 5, W_CN = 11, W_CC = 29, W_NE = 47, W_CE = 53, W_EE = 62 };
constexpr int kSym[3][3] = {{0, 1, 2}, {1, 3, 4}, {2, 4, 5}};  // xx xy xz yy yz zz

bool limbs_in_range(const int64_t* w, int limbs, int64_t n, int top_bits) {
    for (int k = 0; k + 1 < limbs; ++k)
        if (w[k] < 0 || w[k] >= (n << 32)) return false;
    const int64_t top = n << top_bits;
    return w[limbs - 1] <= top && w[limbs - 1] >= -top;
}

// P2's ranges: whatever passes them keeps P3's integers below 2^120
bool sums_in_range(const int64_t* s) {
    const int64_t n = s[W_N], cap = (int64_t)1 << 26;
    if (n < 1 || n > cap || s[W_NO_NORMAL] < 0 || s[W_NO_NORMAL] > cap - n) return false;
    for (int a = 0; a < 3; ++a)
        if (s[W_SP + a] > (n << 30) || s[W_SP + a] < -(n << 30)) return false;
    for (int k = 0; k < 6; ++k)
        if (s[W_NN + k] > (n << 29) || s[W_NN + k] < -(n << 29)) return false;
    if (s[W_NN + 0] < 0 || s[W_NN + 3] < 0 || s[W_NN + 5] < 0) return false;
    for (int k = 0; k < 9; ++k)
        if (!limbs_in_range(s + W_CN + 2 * k, 2, n, 28)) return false;
    for (int k = 0; k < 6; ++k)
        if (!limbs_in_range(s + W_CC + 3 * k, 3, n, 27)) return false;
    for (int k = 0; k < 3; ++k)
        if (!limbs_in_range(s + W_NE + 2 * k, 2, n, 14) || !limbs_in_range(s + W_CE + 3 * k, 3, n, 13)) return false;
    return limbs_in_range(s + W_EE, 2, n, 30) && s[W_EE + 1] >= 0;
}

i128 value2(const int64_t* w) { return (i128)w[1] * ((i128)1 << 32) + (i128)w[0]; }
i128 value3(const int64_t* w) { return ((i128)w[2] * ((i128)1 << 32) + (i128)w[1]) * ((i128)1 << 32) + (i128)w[0]; }

int64_t floor_div(int64_t a, int64_t b) {  // b > 0
    const int64_t q = a / b;
    return (a % b != 0 && a < 0) ? q - 1 : q;
}

void identity_step(double dT[12]) {
    for (int i = 0; i < 12; ++i) dT[i] = (i % 5 == 0) ? 1.0 : 0.0;
}

}  // namespace

extern "C" {

void dmsa_default_dense_align_plane_config(dmsa_dense_align_plane_config* cfg) {
    if (!cfg) return;
    cfg->max_distance = 1.0f, cfg->max_iterations = 30, cfg->min_pairs = 6, cfg->pad = 0;
    cfg->stop_translation = 1e-4, cfg->stop_rotation = 1e-5;
}

int dmsa_dense_align_plane_solve(const int64_t sums[DMSA_ALIGN_PLANE_SUMS], double scale_c, double dT[12], double* shift_m, double* rotation_rad, double* min_pivot) {
    if (!sums || !dT || !std::isfinite(scale_c) || !(scale_c > 0.0) || !sums_in_range(sums)) return DMSA_ERR_INVALID;
    identity_step(dT);
    if (shift_m) *shift_m = 0.0;
    if (rotation_rad) *rotation_rad = 0.0;
    if (min_pivot) *min_pivot = 0.0;
    // P3
    const int64_t n = sums[W_N];
    int64_t C[3];
    for (int a = 0; a < 3; ++a) C[a] = floor_div(2 * sums[W_SP + a] + n, 2 * n);
    const i128 K[3][3] = {{0, -(i128)C[2], (i128)C[1]}, {(i128)C[2], 0, -(i128)C[0]}, {-(i128)C[1], (i128)C[0], 0}};
    i128 NN[3][3], cN[3][3], cc[3][3], Ne[3], ce[3], cNp[3][3], ccp[3][3], cep[3];
    for (int a = 0; a < 3; ++a) {
        Ne[a] = value2(sums + W_NE + 2 * a), ce[a] = value3(sums + W_CE + 3 * a);
        for (int b = 0; b < 3; ++b) NN[a][b] = (i128)sums[W_NN + kSym[a][b]], cN[a][b] = value2(sums + W_CN + 2 * (3 * a + b)), cc[a][b] = value3(sums + W_CC + 3 * kSym[a][b]);
    }
    for (int a = 0; a < 3; ++a) {
        cep[a] = ce[a];
        for (int k = 0; k < 3; ++k) cep[a] -= K[a][k] * Ne[k];
        for (int b = 0; b < 3; ++b) {
            cNp[a][b] = cN[a][b];
            for (int k = 0; k < 3; ++k) cNp[a][b] -= K[a][k] * NN[k][b];
        }
    }
    for (int a = 0; a < 3; ++a)
        for (int b = 0; b < 3; ++b) {
            ccp[a][b] = cc[a][b];
            for (int k = 0; k < 3; ++k) ccp[a][b] -= K[a][k] * cN[b][k] + cNp[a][k] * K[b][k];
        }
    double A[6][6], rhs[6];  // the lower triangle is what P4 reads
    for (int a = 0; a < 3; ++a) {
        rhs[a] = (double)cep[a], rhs[3 + a] = (double)Ne[a];  // one rounding each, to nearest even
        for (int b = 0; b < 3; ++b) A[a][b] = (double)ccp[a][b], A[3 + a][b] = (double)cNp[b][a], A[a][3 + b] = (double)cNp[a][b], A[3 + a][3 + b] = (double)NN[a][b];
    }
    // P4
    double s[6], M[6][6], r[6], L[6][6], D[6], x[6];
    for (int i = 0; i < 6; ++i) {
        if (!(A[i][i] > 0.0)) return DMSA_ALIGN_PLANE_DEGENERATE;
        s[i] = 1.0 / std::sqrt(A[i][i]);
    }
    for (int i = 0; i < 6; ++i) {
        r[i] = rhs[i] * s[i];
        for (int j = 0; j <= i; ++j) M[i][j] = (A[i][j] * s[i]) * s[j];
    }
    const double least = std::ldexp(1.0, -40);
    double smallest = 0.0;
    for (int j = 0; j < 6; ++j) {
        double v = M[j][j];
        for (int k = 0; k < j; ++k) v = v - (L[j][k] * D[k]) * L[j][k];
        D[j] = v;
        if (!(v > least)) {
            if (min_pivot) *min_pivot = v;
            return DMSA_ALIGN_PLANE_DEGENERATE;
        }
        if (j == 0 || v < smallest) smallest = v;
        for (int i = j + 1; i < 6; ++i) {
            double u = M[i][j];
            for (int k = 0; k < j; ++k) u = u - (L[i][k] * D[k]) * L[j][k];
            L[i][j] = u / v;
        }
    }
    for (int i = 0; i < 6; ++i) {
        double y = r[i];
        for (int k = 0; k < i; ++k) y = y - L[i][k] * x[k];
        x[i] = y;
    }
    for (int i = 0; i < 6; ++i) x[i] = x[i] / D[i];
    for (int i = 5; i >= 0; --i) {
        double y = x[i];
        for (int k = i + 1; k < 6; ++k) y = y - L[k][i] * x[k];
        x[i] = y;
    }
    for (int i = 0; i < 6; ++i) x[i] = x[i] * s[i];
    const double hx = x[0] * 0.5, hy = x[1] * 0.5, hz = x[2] * 0.5;
    const double nr = std::sqrt(((1.0 + hx * hx) + hy * hy) + hz * hz);
    const double w = 1.0 / nr, qx = hx / nr, qy = hy / nr, qz = hz / nr;
    const double xx = qx * qx, yy = qy * qy, zz = qz * qz, xy = qx * qy, xz = qx * qz, yz = qy * qz, wx = w * qx, wy = w * qy, wz = w * qz;
    double R[3][3];
    R[0][0] = 1.0 - 2.0 * (yy + zz), R[0][1] = 2.0 * (xy - wz), R[0][2] = 2.0 * (xz + wy);
    R[1][0] = 2.0 * (xy + wz), R[1][1] = 1.0 - 2.0 * (xx + zz), R[1][2] = 2.0 * (yz - wx);
    R[2][0] = 2.0 * (xz - wy), R[2][1] = 2.0 * (yz + wx), R[2][2] = 1.0 - 2.0 * (xx + yy);
    const double Cd[3] = {(double)C[0], (double)C[1], (double)C[2]};  // (exact: |C| <= 2^30)
    for (int a = 0; a < 3; ++a) {
        dT[4 * a + 0] = R[a][0], dT[4 * a + 1] = R[a][1], dT[4 * a + 2] = R[a][2];
        dT[4 * a + 3] = ((Cd[a] + x[3 + a]) - ((R[a][0] * Cd[0] + R[a][1] * Cd[1]) + R[a][2] * Cd[2])) / scale_c;
    }
    if (shift_m) *shift_m = std::sqrt((x[3] * x[3] + x[4] * x[4]) + x[5] * x[5]) / scale_c;
    if (rotation_rad) *rotation_rad = 2.0 * std::sqrt((xx + yy) + zz);
    if (min_pivot) *min_pivot = smallest;
    return DMSA_OK;
}

}  // extern "C"
