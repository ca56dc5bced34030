// dense_align_solve.cpp — the host-only side of include/dmsa_dense_align.h: the defaults, A2's scale, A3's step from
// the 25 exact sums (the centred cross sums in 128-bit integers, Horn's matrix, cyclic Jacobi), A4's measures and A5's composition.  No
// device, no context.  Built with -ffp-contract=off: every operation below is rounded on its own, in the order written, and
// tests/dense_align_model.py repeats them in Python floats bit for bit.
#include "../../include/dmsa_dense_align.h"

#include <cmath>
#include <cstring>

namespace {

typedef __int128 i128;

// A2's ranges: whatever passes them keeps A3's integers below 2^113
bool sums_in_range(const int64_t* s) {
    const int64_t n = s[0];
    if (n < 1 || n > ((int64_t)1 << 26)) return false;
    const int64_t lin = n << 30, hi_max = n << 28, lo_end = n << 32;
    for (int k = 1; k <= 6; ++k)
        if (s[k] > lin || s[k] < -lin) return false;
    for (int k = 0; k < 9; ++k) {
        const int64_t lo = s[7 + 2 * k], hi = s[8 + 2 * k];
        if (lo < 0 || lo >= lo_end || hi > hi_max || hi < -hi_max) return false;
    }
    return true;
}

// A3's eigenvector: the quaternion (w, x, y, z) of the rotation that takes the P to the G
void horn_quaternion(const double S[3][3], double q[4]) {
    double A[4][4], V[4][4];
    A[0][0] = (S[0][0] + S[1][1]) + S[2][2];
    A[1][1] = (S[0][0] - S[1][1]) - S[2][2];
    A[2][2] = (S[1][1] - S[0][0]) - S[2][2];
    A[3][3] = (S[2][2] - S[0][0]) - S[1][1];
    A[0][1] = A[1][0] = S[1][2] - S[2][1];
    A[0][2] = A[2][0] = S[2][0] - S[0][2];
    A[0][3] = A[3][0] = S[0][1] - S[1][0];
    A[1][2] = A[2][1] = S[0][1] + S[1][0];
    A[1][3] = A[3][1] = S[2][0] + S[0][2];
    A[2][3] = A[3][2] = S[1][2] + S[2][1];
    for (int r = 0; r < 4; ++r)
        for (int c = 0; c < 4; ++c) V[r][c] = r == c ? 1.0 : 0.0;
    for (int sweep = 0; sweep < 16; ++sweep) {
        const double off = ((((A[0][1] * A[0][1] + A[0][2] * A[0][2]) + A[0][3] * A[0][3]) + A[1][2] * A[1][2]) + A[1][3] * A[1][3]) + A[2][3] * A[2][3];
        if (off == 0.0) break;
        for (int p = 0; p < 3; ++p)
            for (int qq = p + 1; qq < 4; ++qq) {
                const double apq = A[p][qq];
                if (apq == 0.0) continue;
                const double theta = (A[qq][qq] - A[p][p]) / (2.0 * apq);
                const double root = std::fabs(theta) + std::sqrt(theta * theta + 1.0);
                const double t = theta < 0.0 ? -1.0 / root : 1.0 / root;
                const double c = 1.0 / std::sqrt(t * t + 1.0);
                const double s = t * c;
                A[p][p] = A[p][p] - t * apq;
                A[qq][qq] = A[qq][qq] + t * apq;
                A[p][qq] = A[qq][p] = 0.0;
                for (int r = 0; r < 4; ++r) {
                    if (r == p || r == qq) continue;
                    const double arp = A[r][p], arq = A[r][qq];
                    A[r][p] = A[p][r] = c * arp - s * arq;
                    A[r][qq] = A[qq][r] = s * arp + c * arq;
                }
                for (int r = 0; r < 4; ++r) {
                    const double vrp = V[r][p], vrq = V[r][qq];
                    V[r][p] = c * vrp - s * vrq;
                    V[r][qq] = s * vrp + c * vrq;
                }
            }
    }
    int best = 0;
    for (int i = 1; i < 4; ++i)
        if (A[i][i] > A[best][best]) best = i;
    for (int r = 0; r < 4; ++r) q[r] = V[r][best];
    const double norm = std::sqrt(((q[0] * q[0] + q[1] * q[1]) + q[2] * q[2]) + q[3] * q[3]);
    for (int r = 0; r < 4; ++r) q[r] = q[r] / norm;
    bool flip = q[0] < 0.0;
    if (q[0] == 0.0)
        for (int r = 1; r < 4; ++r)
            if (q[r] != 0.0) {
                flip = q[r] < 0.0;
                break;
            }
    if (flip)
        for (int r = 0; r < 4; ++r) q[r] = -q[r];
}

}  // namespace

extern "C" {

void dmsa_default_dense_align_config(dmsa_dense_align_config* cfg) {
    if (!cfg) return;
    cfg->max_distance = 1.0f, cfg->max_iterations = 30, cfg->min_pairs = 3, cfg->pad = 0;
    cfg->stop_translation = 1e-4, cfg->stop_rotation = 1e-5;
}

double dmsa_dense_align_scale(float voxel_size) {
    if (!std::isfinite(voxel_size) || !(voxel_size > 0.0f)) return 0.0;
    int e = 0;
    (void)std::frexp(voxel_size, &e);
    return std::ldexp(1.0, 10 - e);
}

int dmsa_dense_align_solve(const int64_t sums[DMSA_ALIGN_SUMS], double scale_c, double dT[12], double* shift_m, double* rotation_rad) {
    if (!sums || !dT || !std::isfinite(scale_c) || !(scale_c > 0.0) || !sums_in_range(sums)) return DMSA_ERR_INVALID;
    const int64_t n = sums[0];
    const int64_t* Sp = sums + 1;
    const int64_t* Sg = sums + 4;
    double M[3][3], mx = 0.0;
    for (int a = 0; a < 3; ++a)
        for (int b = 0; b < 3; ++b) {
            const int64_t lo = sums[7 + 2 * (3 * a + b)], hi = sums[8 + 2 * (3 * a + b)];
            const i128 spg = (i128)hi * ((i128)1 << 32) + (i128)lo;
            const i128 m = (i128)n * spg - (i128)Sp[a] * (i128)Sg[b];
            M[a][b] = (double)m;  // one rounding, to nearest even
            if (std::fabs(M[a][b]) > mx) mx = std::fabs(M[a][b]);
        }
    double q[4] = {1.0, 0.0, 0.0, 0.0};
    if (mx != 0.0) {
        double S[3][3];
        for (int a = 0; a < 3; ++a)
            for (int b = 0; b < 3; ++b) S[a][b] = M[a][b] / mx;
        horn_quaternion(S, q);
    }
    const double w = q[0], x = q[1], y = q[2], z = q[3];
    const double xx = x * x, yy = y * y, zz = z * z, xy = x * y, xz = x * z, yz = y * z, wx = w * x, wy = w * y, wz = w * z;
    double R[3][3];
    R[0][0] = 1.0 - 2.0 * (yy + zz), R[0][1] = 2.0 * (xy - wz), R[0][2] = 2.0 * (xz + wy);
    R[1][0] = 2.0 * (xy + wz), R[1][1] = 1.0 - 2.0 * (xx + zz), R[1][2] = 2.0 * (yz - wx);
    R[2][0] = 2.0 * (xz - wy), R[2][1] = 2.0 * (yz + wx), R[2][2] = 1.0 - 2.0 * (xx + yy);
    double pm[3], gm[3], sh[3];
    for (int a = 0; a < 3; ++a) pm[a] = (double)Sp[a] / (double)n, gm[a] = (double)Sg[a] / (double)n;
    for (int a = 0; a < 3; ++a) {
        dT[4 * a + 0] = R[a][0], dT[4 * a + 1] = R[a][1], dT[4 * a + 2] = R[a][2];
        dT[4 * a + 3] = (gm[a] - ((R[a][0] * pm[0] + R[a][1] * pm[1]) + R[a][2] * pm[2])) / scale_c;
        sh[a] = (gm[a] - pm[a]) / scale_c;
    }
    if (shift_m) *shift_m = std::sqrt((sh[0] * sh[0] + sh[1] * sh[1]) + sh[2] * sh[2]);
    if (rotation_rad) *rotation_rad = 2.0 * std::sqrt((xx + yy) + zz);
    return DMSA_OK;
}

int dmsa_dense_align_compose(const double D[12], const double T[12], double out[12]) {
    if (!D || !T || !out) return DMSA_ERR_INVALID;
    double r[12];
    for (int a = 0; a < 3; ++a)
        for (int c = 0; c < 4; ++c) {
            const double v = (D[4 * a + 0] * T[c] + D[4 * a + 1] * T[4 + c]) + D[4 * a + 2] * T[8 + c];
            r[4 * a + c] = c == 3 ? v + D[4 * a + 3] : v;
        }
    std::memcpy(out, r, sizeof r);
    return DMSA_OK;
}

}  // extern "C"
