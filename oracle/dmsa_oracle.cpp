// dmsa_oracle.cpp — CPU ORACLE for the DMSA inner loop.  TEST INFRASTRUCTURE ONLY.
//
// A plain C++17 restatement (no Eigen / PCL / Boost) of
//   DmsaOptimizer<PointT>::optimizeSet and helpers   include/DMSA/DmsaOptimizer.h:54-363
//   Gaussians / splitSet                              include/DMSA/Gaussians.h:19-202
//   ContinuousTrajectory hot methods                  include/DMSA/ContinuousTrajectory.h:75-226, 570-668
//   MapManagement hot methods                         include/DMSA/MapManagement.h:73-252
//   Poses / ConsecutivePoses / helpers                include/DMSA/Poses.h:64-76, ConsecutivePoses.h:26-67, helpers.h:18-65
// Every function cites the reference lines it follows.  Only tests/, __graft_entry__.smoke() and
// bench.py's cpu_baseline leg may load this library; the product never links it.
//
// PARITY UNPINNED.  The reference has no tests and cannot be built here (Eigen 3.4, PCL 1.10,
// Boost 1.71 and ROS are absent).  Third-party arithmetic is restated from the published algorithms:
//   * pcl::octree::OctreePointCloud  — bounding-box growth, key generation, depth-first leaf order
//   * boost::math::barycentric_rational (Floater–Hormann, d = 2)                                   
//   * Eigen: skew().exp() == Rodrigues, R.log() via the unit quaternion, Quaterniond::slerp,
//     AngleAxisd(q), Matrix3f::inverse() (cofactors), fixed-size product evaluation order        
// The fit's float reductions (Gaussians.h:146-147, :172-176) follow Eigen 3.4's own evaluators wherever its source settles the order:
//   * colwise().mean() / VectorXf::mean(): the linear vectorised redux on a contiguous float column is a pure function of the length
//     and of the column's offset inside its 16-byte aligned buffer (eigen_linear_sum_f32 below);
//   * centered^T * centered: the coefficient-based lazy product below 14 members, else general_matrix_matrix_product, where 3 rows and
//     3 columns leave everything to gebp's scalar tail loop -- per coefficient a float chain C = C + a_k b_k over one depth block of kc
//     members, res += 1.0f * C block after block, then a float division by float(n - 1).  kc is the one machine-dependent number: Eigen
//     derives it from the L1 data cache of the machine the reference runs on (680 for 32 KB, 1016 for 48 KB); orc_set_eigen_l1_bytes
//     states it, and every Gaussian with at most kc members has a machine-independent order;
//   * numPointsPerSet.cast<float>().array().pow(-1): Eigen promotes the int exponent to float and calls std::pow per coefficient
//     (scalar_pow_op has no packet path in 3.4.0), i.e. libm's powf(n, -1.0f), which is not correctly rounded (glibc 2.27+: 9857 of the
//     n < 2^24 differ from 1.0f / n by one ulp); this file calls the libm of the machine it runs on, as the reference does.
// MatrixXd products (J^T J, up to four threads) accumulate in a stated block order, see blocked_dot.  EigenSolver<Matrix3f> (general
// QR, Gaussians.h:184-188) follows Eigen 3.4.0's RealSchur / HessenbergDecomposition / Householder / EigenSolver sources statement by
// statement (oracle/eigensolver3f.h, round 6); the covariance is rebuilt as V * D * V^-1 with the cofactor inverse like Gaussians.h:200.
// Build with -ffp-contract=off.
//
// sin / cos / acos / atan2 of the pose-table path (axang2rotm, slerp; the float trigonometry of the normals) are NOT glibc's:
// they are include/dmsa_detmath.h, fixed sequences of correctly rounded IEEE operations (fdlibm's algorithms) shared with the
// product's host code and device kernels, so that a pose table built on the GPU can be compared with this file bit for bit.
// Against glibc they differ by at most 1 ulp (atan2: 2 ulp outside the first quadrant) in ~3 % of the arguments
// (tests/test_detmath.py) -- a deviation from the reference, which calls glibc through Eigen.

#include "dmsa_oracle.h"

#include "../include/dmsa_detmath.h"
#include "eigensolver3f.h"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <memory>
#include <numeric>
#include <stdexcept>
#include <vector>

// ---- hypothesis switches ---------------------------------------------------------------------------------------------
// Where this file states an evaluation order or an arithmetic the reference's sources do not spell out (Eigen internals recalled,
// not read; orders chosen so that a GPU computes them naturally), a compile-time switch selects the plausible alternative.  The
// shipped oracle defines none of them; scripts/oracle_sensitivity.py builds one library per switch (make -C oracle hypotheses) and
// reports how far the optimised poses move -- which hypotheses the 1e-4 m / 1e-4 rad claim depends on.
//   ORC_VAR_TRANSFORM_PAIRWISE  Matrix4f * Vector4f as (c0 x + c1 y) + (c2 z + c3) instead of ((c0 x + c1 y) + c2 z) + c3
//   ORC_VAR_SUM3_LEFT           3-term fixed-size redux as (x0 + x1) + x2 instead of x0 + (x1 + x2)
//   ORC_VAR_MAHA_ASSOC          w * ((d^T A) d) instead of ((w d^T) A) d                       (DmsaOptimizer.h:263)
//   ORC_VAR_FIT_FLOAT           every fit sum (mean, centred products, weight mean) as a scalar float chain in member order
//   ORC_VAR_FIT_MEAN_TREE       colwise().mean() / VectorXf::mean() as 64-wide trees in double (this file's statement until round 4)
//                               instead of Eigen's own float redux order
//   ORC_VAR_FIT_COV_TREE        centered^T * centered as 64-wide pairwise trees in double, divided in double and rounded once (this file's
//                               statement until round 5) instead of the float order of Eigen 3.4's product kernels
//   ORC_VAR_WEIGHT_DIV          1.0f / n (correctly rounded; what a compiler that folds pow(x, -1) emits) instead of libm's powf(n, -1.0f)
//   ORC_VAR_LIMITCOV_VT         limitCovariance rebuilds V * D * V^T (symmetric by construction) instead of V * D * V^-1 (Gaussians.h:200)
//   ORC_VAR_LIMITCOV_JACOBI     limitCovariance's eigenpairs from a fixed 6-sweep cyclic Jacobi iteration in float (this file's statement until round 6)
//                               instead of EigenSolver<Matrix3f> as Eigen 3.4.0 evaluates it (oracle/eigensolver3f.h)
//   ORC_VAR_EIG_BACK_HALVES     the one 3-term sum of that solver (back transformation of the last eigenvector) as x0 + (x1 + x2) instead of (x0 + x1) + x2
//   ORC_VAR_EIG_NORMALIZE_SCALAR eigenvectors()'s normalize() as re / nrm in every row instead of Eigen's Packet2cf division (re * nrm) / (nrm * nrm) in rows 0, 1
//   ORC_VAR_STEP_LEFT_ASSOC     the LM step as Eigen associates it, ((-alpha H^-1) J^T) e with a P x rows temporary, instead of (-alpha H^-1)(J^T e)
//   ORC_VAR_LM_BLOCKED_LU       H^-1 from a right-looking LU in 8-column panels (the shape of Eigen's PartialPivLU) instead of Gauss-Jordan on [H | I]
//   ORC_VAR_JTJ_NOFMA           J^T J, J^T e, e^T e for P > 64 with separately rounded multiply and add (the reference has no FMA)
//   ORC_VAR_GLIBC_TRIG          sin / cos / acos / atan2 from glibc instead of include/dmsa_detmath.h
#ifdef ORC_VAR_GLIBC_TRIG
#define ORC_SIN(x) std::sin(x)
#define ORC_COS(x) std::cos(x)
#define ORC_ACOS(x) std::acos(x)
#define ORC_ATAN2(y, x) std::atan2(y, x)
#else
#define ORC_SIN(x) dmsa_det::det_sin(x)
#define ORC_COS(x) dmsa_det::det_cos(x)
#define ORC_ACOS(x) dmsa_det::det_acos(x)
#define ORC_ATAN2(y, x) dmsa_det::det_atan2(y, x)
#endif

namespace {

// ------------------------------------------------------------------------------------------------
// small fixed-size double algebra
// ------------------------------------------------------------------------------------------------
struct M3 {
    double m[3][3];  // m[row][col]
};
static inline M3 eye3() { return M3{{{1, 0, 0}, {0, 1, 0}, {0, 0, 1}}}; }
static inline M3 mul(const M3& a, const M3& b) {
    M3 c;
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) c.m[i][j] = a.m[i][0] * b.m[0][j] + a.m[i][1] * b.m[1][j] + a.m[i][2] * b.m[2][j];
    return c;
}
static inline M3 transpose(const M3& a) {
    M3 c;
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) c.m[i][j] = a.m[j][i];
    return c;
}
static inline void matvec(const M3& a, const double* v, double* out) {
    double r[3];
    for (int i = 0; i < 3; ++i) r[i] = a.m[i][0] * v[0] + a.m[i][1] * v[1] + a.m[i][2] * v[2];
    out[0] = r[0], out[1] = r[1], out[2] = r[2];
}
static inline double norm3(const double* a) { return std::sqrt(a[0] * a[0] + a[1] * a[1] + a[2] * a[2]); }

// helpers.h:51-57 axang2rotm: identity below EPSILON_ROT (helpers.h:18), else skew(axang).exp().
// The matrix exponential of a skew matrix is Rodrigues' formula; 1-cos is written 2 sin^2(t/2).
static M3 axang2rotm(const double* w) {
    const double theta = norm3(w);
    if (theta < 0.00001) return eye3();
    const double s = ORC_SIN(theta) / theta;  // sin / cos / acos / atan2 of the pose-table path: include/dmsa_detmath.h
    const double sh = ORC_SIN(0.5 * theta);
    const double c = 2.0 * sh * sh / (theta * theta);
    const double x = w[0], y = w[1], z = w[2];
    M3 R;
    // I + s*K + c*K^2 with K^2 = w w^T - theta^2 I
    R.m[0][0] = 1.0 + c * (x * x - theta * theta);
    R.m[1][1] = 1.0 + c * (y * y - theta * theta);
    R.m[2][2] = 1.0 + c * (z * z - theta * theta);
    R.m[0][1] = c * x * y - s * z;
    R.m[1][0] = c * x * y + s * z;
    R.m[0][2] = c * x * z + s * y;
    R.m[2][0] = c * x * z - s * y;
    R.m[1][2] = c * y * z - s * x;
    R.m[2][1] = c * y * z + s * x;
    return R;
}

// helpers.h:59-65 rotm2axang: principal matrix logarithm of a rotation, read as (S(2,1), S(0,2), S(1,0)).
// Restated through the unit quaternion (Shepperd) so that it stays accurate near 0 and near pi.
static void rotm2axang(const M3& R, double* out) {
    const double m00 = R.m[0][0], m11 = R.m[1][1], m22 = R.m[2][2];
    const double tr = m00 + m11 + m22;
    double qw, qx, qy, qz;
    if (tr > 0.0) {
        const double s = std::sqrt(tr + 1.0) * 2.0;
        qw = 0.25 * s;
        qx = (R.m[2][1] - R.m[1][2]) / s;
        qy = (R.m[0][2] - R.m[2][0]) / s;
        qz = (R.m[1][0] - R.m[0][1]) / s;
    } else if (m00 > m11 && m00 > m22) {
        const double s = std::sqrt(1.0 + m00 - m11 - m22) * 2.0;
        qw = (R.m[2][1] - R.m[1][2]) / s;
        qx = 0.25 * s;
        qy = (R.m[0][1] + R.m[1][0]) / s;
        qz = (R.m[0][2] + R.m[2][0]) / s;
    } else if (m11 > m22) {
        const double s = std::sqrt(1.0 + m11 - m00 - m22) * 2.0;
        qw = (R.m[0][2] - R.m[2][0]) / s;
        qx = (R.m[0][1] + R.m[1][0]) / s;
        qy = 0.25 * s;
        qz = (R.m[1][2] + R.m[2][1]) / s;
    } else {
        const double s = std::sqrt(1.0 + m22 - m00 - m11) * 2.0;
        qw = (R.m[1][0] - R.m[0][1]) / s;
        qx = (R.m[0][2] + R.m[2][0]) / s;
        qy = (R.m[1][2] + R.m[2][1]) / s;
        qz = 0.25 * s;
    }
    const double n = std::sqrt(qx * qx + qy * qy + qz * qz);
    if (n == 0.0) {
        out[0] = out[1] = out[2] = 0.0;
        return;
    }
    const double angle = 2.0 * ORC_ATAN2(n, std::fabs(qw));
    const double k = angle / (qw < 0.0 ? -n : n);
    out[0] = qx * k, out[1] = qy * k, out[2] = qz * k;
}

// helpers.h:24-37 slerp of two axis-angle vectors, with Eigen 3.4 semantics of
// Quaterniond(AngleAxisd(norm, normalized)), QuaternionBase::slerp and AngleAxisd(Quaterniond).
static void slerp(const double* aa1, const double* aa2, double t, double* out) {
    double q1[4], q2[4];  // w, x, y, z
    const double* aas[2] = {aa1, aa2};
    double* qs[2] = {q1, q2};
    for (int i = 0; i < 2; ++i) {
        const double* a = aas[i];
        const double sq = a[0] * a[0] + a[1] * a[1] + a[2] * a[2];
        const double ang = std::sqrt(sq);
        double ax[3] = {a[0], a[1], a[2]};
        if (sq > 0.0) {  // Eigen normalized(): zero vector stays zero
            ax[0] = a[0] / ang, ax[1] = a[1] / ang, ax[2] = a[2] / ang;
        }
        const double sh = ORC_SIN(0.5 * ang);
        qs[i][0] = ORC_COS(0.5 * ang);
        qs[i][1] = sh * ax[0], qs[i][2] = sh * ax[1], qs[i][3] = sh * ax[2];
    }
    const double one = 1.0 - std::numeric_limits<double>::epsilon();
    const double d = q1[0] * q2[0] + q1[1] * q2[1] + q1[2] * q2[2] + q1[3] * q2[3];
    const double absD = std::fabs(d);
    double scale0, scale1;
    if (absD >= one) {
        scale0 = 1.0 - t;
        scale1 = t;
    } else {
        const double theta = ORC_ACOS(absD);
        const double sinTheta = ORC_SIN(theta);
        scale0 = ORC_SIN((1.0 - t) * theta) / sinTheta;
        scale1 = ORC_SIN(t * theta) / sinTheta;
    }
    if (d < 0.0) scale1 = -scale1;
    double q[4];
    for (int i = 0; i < 4; ++i) q[i] = scale0 * q1[i] + scale1 * q2[i];
    // AngleAxisd(q)
    double n = std::sqrt(q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
    if (n != 0.0) {
        const double angle = 2.0 * ORC_ATAN2(n, std::fabs(q[0]));
        if (q[0] < 0.0) n = -n;
        out[0] = (q[1] / n) * angle, out[1] = (q[2] / n) * angle, out[2] = (q[3] / n) * angle;
    } else {
        out[0] = 0.0, out[1] = 0.0, out[2] = 0.0;  // angle 0, axis (1,0,0)
    }
}

// boost::math::barycentric_rational<double> (ContinuousTrajectory.h:214-217): Floater–Hormann weights and
// barycentric evaluation with the exact-node short-circuit.
struct BarycentricRational {
    std::vector<double> x, y, w;
    BarycentricRational(const double* xs, const double* ys, int n, int d) : x(xs, xs + n), y(ys, ys + n), w(n, 0.0) {
        for (int64_t k = 0; k < n; ++k) {
            int64_t i_min = std::max<int64_t>(k - d, 0);
            int64_t i_max = k;
            if (k >= n - d) i_max = n - d - 1;
            for (int64_t i = i_min; i <= i_max; ++i) {
                double inv_product = 1.0;
                const int64_t j_max = std::min<int64_t>(i + d, n - 1);
                for (int64_t j = i; j <= j_max; ++j) {
                    if (j == k) continue;
                    const double diff = x[k] - x[j];
                    if (std::fabs(diff) < std::numeric_limits<double>::min()) throw std::logic_error("coincident nodes");
                    inv_product *= diff;
                }
                if (i % 2 == 0)
                    w[k] += 1.0 / inv_product;
                else
                    w[k] -= 1.0 / inv_product;
            }
        }
    }
    double operator()(double t) const {
        double numerator = 0.0, denominator = 0.0;
        for (size_t i = 0; i < x.size(); ++i) {
            if (t == x[i]) return y[i];
            const double q = w[i] / (t - x[i]);
            numerator += q * y[i];
            denominator += q;
        }
        return numerator / denominator;
    }
    // barycentric_rational_imp<Real>::prime (Boost 1.71 detail/barycentric_rational_detail.hpp), used by updateInitialGuess :418
    double prime(double t) const {
        const double rx = (*this)(t);
        double numerator = 0.0, denominator = 0.0;
        for (size_t i = 0; i < x.size(); ++i) {
            if (t == x[i]) {
                double sum = 0.0;
                for (size_t j = 0; j < x.size(); ++j) {
                    if (j == i) continue;
                    sum += w[j] * (y[i] - y[j]) / (x[i] - x[j]);
                }
                return -sum / w[i];
            }
            const double q = w[i] / (t - x[i]);
            const double diff = (rx - y[i]) / (t - x[i]);
            numerator += q * diff;
            denominator += q;
        }
        return numerator / denominator;
    }
};

// Poses.h:16-76: 3xn column-major axis-angle + translations.
struct Poses {
    int n = 0;
    std::vector<double> O, T;
    void resize(int k) {
        n = k;
        O.assign(3 * (size_t)k, 0.0);
        T.assign(3 * (size_t)k, 0.0);
    }
    // Poses.h:64-70: [Orientations cols 1..n-1 | Translations cols 1..n-1], pose 0 excluded
    void getParamsAsVector(std::vector<double>& p) const {
        p.resize(6 * (size_t)(n - 1));
        std::copy(O.begin() + 3, O.end(), p.begin());
        std::copy(T.begin() + 3, T.end(), p.begin() + 3 * (n - 1));
    }
    // Poses.h:72-76
    void setParamsFromVector(const std::vector<double>& p) {
        std::copy(p.begin(), p.begin() + 3 * (n - 1), O.begin() + 3);
        std::copy(p.begin() + 3 * (n - 1), p.end(), T.begin() + 3);
    }
};

// ConsecutivePoses.h:17-75
struct ConsecutivePoses {
    Poses rel, glob;
    int numPoses = 0;
    void resize(int n) {
        rel.resize(n), glob.resize(n);
        numPoses = n;
    }
    // ConsecutivePoses.h:26-43
    void relative2global() {
        M3 R = eye3();
        double T[3] = {0, 0, 0};
        for (int k = 0; k < numPoses; ++k) {
            double rt[3];
            matvec(R, &rel.T[3 * k], rt);
            T[0] = T[0] + rt[0], T[1] = T[1] + rt[1], T[2] = T[2] + rt[2];
            glob.T[3 * k] = T[0], glob.T[3 * k + 1] = T[1], glob.T[3 * k + 2] = T[2];
            R = mul(R, axang2rotm(&rel.O[3 * k]));
            rotm2axang(R, &glob.O[3 * k]);
        }
    }
    // ConsecutivePoses.h:45-67
    void global2relative() {
        for (int c = 0; c < 3; ++c) rel.O[c] = glob.O[c], rel.T[c] = glob.T[c];
        for (int k = numPoses - 1; k > 0; --k) {
            const M3 R1 = axang2rotm(&glob.O[3 * (k - 1)]);
            const M3 R2 = axang2rotm(&glob.O[3 * k]);
            const M3 R1t = transpose(R1);
            rotm2axang(mul(R1t, R2), &rel.O[3 * k]);
            const double d[3] = {glob.T[3 * k] - glob.T[3 * (k - 1)], glob.T[3 * k + 1] - glob.T[3 * (k - 1) + 1],
                                 glob.T[3 * k + 2] - glob.T[3 * (k - 1) + 2]};
            matvec(R1t, d, &rel.T[3 * k]);
        }
    }
};

// ------------------------------------------------------------------------------------------------
// float helpers that pin Eigen's fixed-size evaluation order (SURVEY 8(a) "evaluation-order assumptions")
// ------------------------------------------------------------------------------------------------
// Matrix4f * Vector4f with w = 1 (ContinuousTrajectory.h:151, MapManagement.h:142): ((c0*x + c1*y) + c2*z) + c3*1
static inline void tform_point(const float* T /* 12: row-major 3x4 */, const float* p, float* out) {
#ifdef ORC_VAR_TRANSFORM_PAIRWISE
    for (int r = 0; r < 3; ++r) out[r] = (T[4 * r + 0] * p[0] + T[4 * r + 1] * p[1]) + (T[4 * r + 2] * p[2] + T[4 * r + 3]);
#else
    for (int r = 0; r < 3; ++r) out[r] = ((T[4 * r + 0] * p[0] + T[4 * r + 1] * p[1]) + T[4 * r + 2] * p[2]) + T[4 * r + 3];
#endif
}
// 3-term fixed-size inner product: Eigen's unrolled redux splits in halves -> x0 + (x1 + x2)
#ifdef ORC_VAR_SUM3_LEFT
static inline float sum3(float a, float b, float c) { return (a + b) + c; }
#else
static inline float sum3(float a, float b, float c) { return a + (b + c); }
#endif
// Matrix3f * Vector3f (MapManagement.h:144)
static inline void rot_vec(const float* T, const float* v, float* out) {
    for (int r = 0; r < 3; ++r) out[r] = sum3(T[4 * r + 0] * v[0], T[4 * r + 1] * v[1], T[4 * r + 2] * v[2]);
}
static inline float normf3(float x, float y, float z) { return std::sqrt(sum3(x * x, y * y, z * z)); }

// Matrix3f::inverse(): cofactor closed form (Eigen/src/LU/InverseImpl.h, size 3)
static void inverse3f(const float m[3][3], float inv[3][3]) {
    auto cof = [&](int i, int j) {
        const int i1 = (i + 1) % 3, i2 = (i + 2) % 3, j1 = (j + 1) % 3, j2 = (j + 2) % 3;
        return m[i1][j1] * m[i2][j2] - m[i1][j2] * m[i2][j1];
    };
    const float c0 = cof(0, 0), c1 = cof(1, 0), c2 = cof(2, 0);
    const float det = sum3(c0 * m[0][0], c1 * m[1][0], c2 * m[2][0]);
    const float invdet = 1.0f / det;
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c) inv[r][c] = cof(c, r) * invdet;
}

// Gaussians.h:181-201 limitCovariance: EigenSolver<Matrix3f> as Eigen 3.4.0 evaluates it (oracle/eigensolver3f.h: scaling, one Householder
// reflector to Hessenberg form, Francis QR steps to the real Schur form, eigenvalues off T's diagonal IN THAT ORDER, back substitution, back
// transformation, normalised columns, real parts), the clamp >= 1e-4 (:191-194), then the reference's own rebuild
// `eigenVectors * diagonal_matrix * eigenVectors.inverse()` (:200): (V D)(i,k) = V(i,k) * d(k), the fixed-size product with the cofactor
// inverse of V coefficient by coefficient as a 3-term redux.  V is orthogonal only up to rounding, so the result is NOT exactly symmetric --
// like the reference's.  Hypotheses: ORC_VAR_LIMITCOV_JACOBI (this file's statement until round 6: a fixed 6-sweep cyclic Jacobi iteration in
// float -- same mathematics, other eigenvalue order, other rounding), ORC_VAR_LIMITCOV_VT (V * D * V^T), ORC_VAR_EIG_BACK_HALVES, ORC_VAR_EIG_NORMALIZE_SCALAR.
struct LimitCovStats {
    int64_t calls = 0, qr_iterations = 0, max_iterations = 0, complex_pairs = 0, not_converged = 0;
};
static LimitCovStats g_limitcov_stats;  // test telemetry (orc_limitcov_stats); updated under omp critical
#ifdef ORC_VAR_LIMITCOV_JACOBI
static void limit_covariance_eig(const float c[3][3], float v[3][3], float lam[3]) {
    float a[3][3];
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) a[i][j] = c[i][j], v[i][j] = i == j ? 1.0f : 0.0f;
    static const int PQ[3][2] = {{0, 1}, {0, 2}, {1, 2}};
    for (int sweep = 0; sweep < 6; ++sweep) {
        for (int r = 0; r < 3; ++r) {
            const int p = PQ[r][0], q = PQ[r][1];
            const float apq = a[p][q];
            if (apq == 0.0f) continue;
            const float theta = (a[q][q] - a[p][p]) / (2.0f * apq);
            const float at = std::fabs(theta);
            float t = 1.0f / (at + std::sqrt(theta * theta + 1.0f));
            if (theta < 0.0f) t = -t;
            const float cs = 1.0f / std::sqrt(t * t + 1.0f);
            const float sn = t * cs;
            const int k = 3 - p - q;  // the remaining index
            const float app = a[p][p], aqq = a[q][q];
            a[p][p] = app - t * apq;
            a[q][q] = aqq + t * apq;
            a[p][q] = 0.0f, a[q][p] = 0.0f;
            const float akp = a[k][p], akq = a[k][q];
            a[k][p] = cs * akp - sn * akq;
            a[p][k] = a[k][p];
            a[k][q] = sn * akp + cs * akq;
            a[q][k] = a[k][q];
            for (int i = 0; i < 3; ++i) {
                const float vip = v[i][p], viq = v[i][q];
                v[i][p] = cs * vip - sn * viq;
                v[i][q] = sn * vip + cs * viq;
            }
        }
    }
    for (int k = 0; k < 3; ++k) lam[k] = a[k][k];
}
#else
static void limit_covariance_eig(const float c[3][3], float v[3][3], float lam[3]) {
    eigen34::Matrix3f A;
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) A(i, j) = c[i][j];
    eigen34::EigenSolver3f es;
    eigen34::eigensolver_compute(A, es);
#pragma omp critical(limitcov_stats)
    {
        g_limitcov_stats.calls++, g_limitcov_stats.qr_iterations += es.iterations, g_limitcov_stats.complex_pairs += es.complex_pairs;
        g_limitcov_stats.max_iterations = std::max<int64_t>(g_limitcov_stats.max_iterations, es.iterations);
        g_limitcov_stats.not_converged += es.info != 0;
    }
    if (es.info != 0) {  // not restated (see eigensolver3f.h): keep the diagonal
        for (int i = 0; i < 3; ++i)
            for (int j = 0; j < 3; ++j) v[i][j] = i == j ? 1.0f : 0.0f;
        for (int k = 0; k < 3; ++k) lam[k] = c[k][k];
        return;
    }
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) v[i][j] = es.V_re(i, j);
    for (int k = 0; k < 3; ++k) lam[k] = es.eivalues_re[k];
}
#endif
static void limit_covariance(float c[3][3]) {
    float v[3][3], lam[3];
    limit_covariance_eig(c, v, lam);
    for (int k = 0; k < 3; ++k) lam[k] = std::max(lam[k], 0.0001f);  // Gaussians.h:191-194
#ifdef ORC_VAR_LIMITCOV_VT
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) c[i][j] = sum3((v[i][0] * lam[0]) * v[j][0], (v[i][1] * lam[1]) * v[j][1], (v[i][2] * lam[2]) * v[j][2]);
#else
    float vinv[3][3];
    inverse3f(v, vinv);
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) c[i][j] = sum3((v[i][0] * lam[0]) * vinv[0][j], (v[i][1] * lam[1]) * vinv[1][j], (v[i][2] * lam[2]) * vinv[2][j]);
#endif
}

// L1 data cache size Eigen's product blocking is derived from on the reference's machine (orc_set_eigen_l1_bytes; Eigen's default when
// cpuid reports nothing is 32 KB as well)
static int g_eigen_l1_bytes = 32 * 1024;

// ------------------------------------------------------------------------------------------------
// PCL OctreePointCloud, restated without building a tree.
// ------------------------------------------------------------------------------------------------
struct VoxelResult {
    dmsa_voxel_level_info info{};
    std::vector<uint64_t> code;   // per point, UINT64_MAX for skipped (non-finite) points
    std::vector<uint32_t> key;    // per point x 3, final keys
    std::vector<int32_t> order;   // valid point indices sorted by (code, index)
};

static int voxelize(const float* xyz4, int64_t n, double resolution, VoxelResult& out) {
    const double eps = (double)std::numeric_limits<float>::epsilon();  // "minValue" in PCL
    bool defined = false;
    double mn[3] = {0, 0, 0}, mx[3] = {0, 0, 0};
    unsigned depth = 0;
    struct Event {
        uint32_t shift[3];
    };
    std::vector<Event> events;
    std::vector<int32_t> epoch((size_t)n, -1);
    out.code.assign((size_t)n, UINT64_MAX);
    out.key.assign((size_t)n * 3, 0u);
    int64_t num_valid = 0;
    for (int64_t i = 0; i < n; ++i) {
        const float* p = xyz4 + 4 * i;
        if (!(std::isfinite(p[0]) && std::isfinite(p[1]) && std::isfinite(p[2]))) continue;  // addPointsFromInputCloud
        // adoptBoundingBoxToPoint
        while (true) {
            bool lo[3], hi[3];
            for (int a = 0; a < 3; ++a) lo[a] = (double)p[a] < mn[a], hi[a] = (double)p[a] >= mx[a];
            if (!(lo[0] || lo[1] || lo[2] || hi[0] || hi[1] || hi[2] || !defined)) break;
            if (defined) {
                double side = (double)(1u << depth) * resolution;
                Event ev{};
                for (int a = 0; a < 3; ++a) {
                    if (!hi[a]) {
                        mn[a] -= side;
                        ev.shift[a] = 1u << depth;  // old root becomes the upper child on this axis
                    }
                }
                events.push_back(ev);
                depth += 1;
                if (depth > 21) return DMSA_ERR_DEPTH;
                side = (double)(1u << depth) * resolution - eps;
                for (int a = 0; a < 3; ++a) mx[a] = mn[a] + side;
            } else {
                for (int a = 0; a < 3; ++a) {
                    mn[a] = (double)p[a] - resolution / 2;
                    mx[a] = (double)p[a] + resolution / 2;
                }
                // getKeyBitSize()
                unsigned max_key[3];
                for (int a = 0; a < 3; ++a) max_key[a] = (unsigned)std::ceil((mx[a] - mn[a] - eps) / resolution);
                const unsigned max_voxels = std::max(std::max(std::max(max_key[0], max_key[1]), max_key[2]), 2u);
                depth = std::max(std::min(32u, (unsigned)std::ceil(std::log((double)max_voxels) / std::log(2.0) - eps)), 0u);
                const double side = (double)(1u << depth) * resolution;
                for (int a = 0; a < 3; ++a) {  // leaf_count_ == 0
                    const double oversize = (side - (mx[a] - mn[a])) / 2.0;
                    if (oversize > eps) {
                        mn[a] -= oversize;
                        mx[a] += oversize;
                    }
                }
                defined = true;
            }
        }
        // genOctreeKeyforPoint, truncated to the tree depth at insertion time (createLeafRecursive only
        // looks at depth_mask bits)
        const uint32_t mask = (depth >= 32) ? 0xffffffffu : ((1u << depth) - 1u);
        for (int a = 0; a < 3; ++a) out.key[3 * i + a] = (uint32_t)(((double)p[a] - mn[a]) / resolution) & mask;
        epoch[i] = (int32_t)events.size();
        ++num_valid;
    }
    // later growth re-roots the tree: add the shifts of all events after the insertion epoch
    std::vector<Event> suffix(events.size() + 1, Event{});
    for (int64_t e = (int64_t)events.size() - 1; e >= 0; --e)
        for (int a = 0; a < 3; ++a) suffix[e].shift[a] = suffix[e + 1].shift[a] + events[e].shift[a];
    out.order.clear();
    out.order.reserve((size_t)num_valid);
    for (int64_t i = 0; i < n; ++i) {
        if (epoch[i] < 0) continue;
        uint64_t code = 0;
        uint32_t k[3];
        for (int a = 0; a < 3; ++a) k[a] = out.key[3 * i + a] += suffix[epoch[i]].shift[a];
        // depth-first leaf order, children visited 0..7 with child = (xbit<<2)|(ybit<<1)|zbit from the MSB down
        for (int l = (int)depth - 1; l >= 0; --l) code = (code << 3) | (((k[0] >> l) & 1u) << 2) | (((k[1] >> l) & 1u) << 1) | ((k[2] >> l) & 1u);
        out.code[i] = code;
        out.order.push_back((int32_t)i);
    }
    std::stable_sort(out.order.begin(), out.order.end(), [&](int32_t a, int32_t b) { return out.code[a] < out.code[b]; });
    int64_t leaves = 0;
    for (size_t j = 0; j < out.order.size(); ++j)
        if (j == 0 || out.code[out.order[j]] != out.code[out.order[j - 1]]) ++leaves;
    out.info.resolution = resolution;
    out.info.min_xyz[0] = mn[0], out.info.min_xyz[1] = mn[1], out.info.min_xyz[2] = mn[2];
    out.info.depth = (int32_t)depth;
    out.info.num_events = (int32_t)events.size();
    out.info.num_leaves = leaves;
    out.info.num_valid = num_valid;
    return DMSA_OK;
}

// ------------------------------------------------------------------------------------------------
// Gaussians (Gaussians.h:87-202)
// ------------------------------------------------------------------------------------------------
struct Gaussians {
    std::vector<int32_t> segOffset{0};  // connectedPointIds, flattened
    std::vector<int32_t> members;
    std::vector<float> info;     // M x 9, column-major Matrix3f
    std::vector<float> weights;  // rebalancingWeights
    std::vector<float> obsWeights;
    // intermediate results of the fit, kept for the stage dump ('fit_sums' stage of tests/ref_stage_checks.py): subset.colwise().mean(),
    // the covariance BEFORE limitCovariance (column-major), and pow(-1) of the member counts before the division by their mean
    std::vector<float> fitMean, fitCov, rawWeights;
    int numPointSets = 0;
    int numLevel1 = 0;

    void reset() {  // Gaussians.h:121-128
        segOffset.assign(1, 0);
        members.clear(), info.clear(), weights.clear(), obsWeights.clear();
        fitMean.clear(), fitCov.clear(), rawWeights.clear();
        numPointSets = 0;
    }
    // Gaussians.h:130-168
    // blockedSum: the order this file stated for the fit's sums until Eigen's own orders were restated (now only behind the switches
    // ORC_VAR_FIT_COV_TREE / FIT_MEAN_TREE / FIT_FLOAT): double accumulation over consecutive blocks of kSumBlock = 64 members, every
    // block reduced by the balanced pairwise tree (v[i] += v[i - w] for w = 1, 2, 4 .. 32; missing members count as +0.0), the block
    // sums added in block order.
    static constexpr size_t kSumBlock = 64;
    template <typename Term>
    static double blockedSum(size_t n, Term term) {
#ifdef ORC_VAR_FIT_FLOAT
        float chain = 0.0f;  // a scalar float loop in member order
        for (size_t j = 0; j < n; ++j) chain = chain + (float)term(j);
        return (double)chain;
#endif
        double total = 0.0;
        for (size_t j0 = 0; j0 < n; j0 += kSumBlock) {
            double v[kSumBlock];
            for (size_t i = 0; i < kSumBlock; ++i) v[i] = j0 + i < n ? term(j0 + i) : 0.0;
            for (size_t w = 1; w < kSumBlock; w <<= 1)
                for (size_t i = 2 * w - 1; i < kSumBlock; i += 2 * w) v[i] = v[i] + v[i - w];
            total += v[kSumBlock - 1];
        }
        return total;
    }
    // DenseBase::sum() of a contiguous float vector of n entries whose first entry lies `offset` floats behind a 16-byte boundary:
    // Eigen 3.4 Redux.h, redux_impl<scalar_sum_op, ..., LinearVectorizedTraversal, NoUnrolling> with SSE2's Packet4f (the reference
    // is built without -march, CMakeLists.txt:13-17) --
    //   alignedStart = entries up to the first aligned one (first_default_aligned), alignedSize = whole packets behind it,
    //   alignedSize2 = whole PAIRS of packets;  two packet accumulators take the packets alternately, res0 += res1, one more packet
    //   if their number is odd, predux = (a0 + a2) + (a1 + a3) (_mm_movehl_ps, then _mm_add_ss with lane 1), then the scalars in
    //   front of alignedStart and the scalars behind the last packet, in index order;  fewer than one whole packet: a scalar loop.
    // A pure function of (n, offset): column c of the n x 3 column-major `subset` starts c * n floats behind its aligned buffer
    // (MatrixX3f, Gaussians.h:130,146; copyPointsIntoEigMatrix, DmsaOptimizer.h:352-363), `rebalancingWeights.head(M)` at offset 0.
    template <typename Get>
    static float eigen_linear_sum_f32(size_t n, size_t offset, Get x) {
        if (n == 0) return 0.0f;  // DenseBase::sum() of an empty vector
        const size_t first = (4 - (offset & 3)) & 3;
        const size_t aStart = first < n ? first : n;
        const size_t aSize = ((n - aStart) / 4) * 4, aSize2 = ((n - aStart) / 8) * 8;
        const size_t aEnd = aStart + aSize, aEnd2 = aStart + aSize2;
        float res;
        if (aSize) {
            float p0[4], p1[4];
            for (int l = 0; l < 4; ++l) p0[l] = x(aStart + l);
            if (aSize > 4) {
                for (int l = 0; l < 4; ++l) p1[l] = x(aStart + 4 + l);
                for (size_t i = aStart + 8; i < aEnd2; i += 8)
                    for (int l = 0; l < 4; ++l) p0[l] = p0[l] + x(i + l), p1[l] = p1[l] + x(i + 4 + l);
                for (int l = 0; l < 4; ++l) p0[l] = p0[l] + p1[l];
                if (aEnd > aEnd2)
                    for (int l = 0; l < 4; ++l) p0[l] = p0[l] + x(aEnd2 + l);
            }
            res = (p0[0] + p0[2]) + (p0[1] + p0[3]);
            for (size_t i = 0; i < aStart; ++i) res = res + x(i);
            for (size_t i = aEnd; i < n; ++i) res = res + x(i);
        } else {
            res = x(0);
            for (size_t i = 1; i < n; ++i) res = res + x(i);
        }
        return res;
    }
    // mean of a contiguous float vector, Eigen's `sum() / Scalar(size)` (VectorwiseOp::mean, DenseBase::mean)
    template <typename Get>
    static float eigen_mean_f32(size_t n, size_t offset, Get x) {
#if defined(ORC_VAR_FIT_FLOAT) || defined(ORC_VAR_FIT_MEAN_TREE)
        (void)offset;
        return (float)(blockedSum(n, [&](size_t j) { return (double)x(j); }) / (double)n);
#else
        return eigen_linear_sum_f32(n, offset, x) / (float)n;
#endif
    }
    // centered.adjoint() * centered (Gaussians.h:147) as Eigen 3.4.0 evaluates a (3 x n) * (n x 3) float product whose result has dynamic size
    // (`centered` is a MatrixXf):
    //  * generic_product_impl<.., GemmProduct>::evalTo (GeneralMatrixMatrix.h) takes the coefficient-based lazy product while
    //    rhs.rows() + dst.rows() + dst.cols() < EIGEN_GEMM_TO_COEFFBASED_THRESHOLD = 20, i.e. n < 14.  Its evaluator has no packet access
    //    (the lhs is a transpose of a column-major matrix, the rhs is not row-major), so every coefficient is
    //    (lhs.row(i).transpose().cwiseProduct(rhs.col(j))).sum(): the linear vectorised redux of the element-wise products; the
    //    expression has no direct access, so first_default_aligned() is 0 and the packets start at element 0.
    //  * else dst.setZero() and general_matrix_matrix_product -> gebp_kernel with mr = 8, nr = 4 (SSE, no FMA).  3 rows < LhsProgress
    //    and 3 columns < nr, so all nine coefficients go through gebp's last loop ("remaining columns" x "remaining rows"):
    //        ResScalar C0(0);  for (k < depth) C0 = cj.pmadd(A0, B_0, C0);  res(i, j) += alpha * C0;      (alpha = 1.0f)
    //    once per depth block of kc members, the blocks in order.  One thread: parallelize_gemm gives max(1, cols / nr) = 1.
    //  * kc (evaluateProductBlockingSizesHeuristic, one thread): untouched when max(k, m, n) < 48; else
    //    max_kc = ((l1 - k_sub) / k_div) & ~(k_peeling - 1) with k_sub = mr * nr * 4 = 128, k_div = mr * 4 + nr * 4 = 48, k_peeling = 8,
    //    and a depth above max_kc is split into nearly equal blocks that are multiples of 8.  l1 = g_eigen_l1_bytes.
    // Coefficients (i, j) and (j, i) multiply the same floats in the same order: the product is exactly symmetric.
    static size_t gemm_kc(size_t k) {
        if (k < 48) return k;
        const size_t l1 = (size_t)g_eigen_l1_bytes, k_peeling = 8, k_div = 1 * (8 * 4 + 4 * 4), k_sub = 8 * 4 * 4;
        const size_t max_kc = std::max<size_t>(((l1 - k_sub) / k_div) & ~(k_peeling - 1), 1);
        if (k <= max_kc) return k;
        return (k % max_kc) == 0 ? max_kc : max_kc - k_peeling * ((max_kc - 1 - (k % max_kc)) / (k_peeling * (k / max_kc + 1)));
    }
    template <typename A, typename B>
    static float gemm_dot_f32(size_t n, A a, B b) {
        if (n + 6 < 20) return eigen_linear_sum_f32(n, 0, [&](size_t k) { return a(k) * b(k); });
        const size_t kc = gemm_kc(n);
        float res = 0.0f;
        for (size_t k0 = 0; k0 < n; k0 += kc) {
            float C = 0.0f;
            for (size_t k = k0; k < std::min(n, k0 + kc); ++k) C = C + a(k) * b(k);
            res = res + 1.0f * C;
        }
        return res;
    }
    void addPointSet(const std::vector<int>& ids, const float* xyz4, float observationWeight) {
        const size_t n = ids.size();
        float mean[3];  // subset.colwise().mean(), Gaussians.h:146
        for (int c = 0; c < 3; ++c) mean[c] = eigen_mean_f32(n, (size_t)c * n, [&](size_t j) { return xyz4[4 * (size_t)ids[j] + c]; });
        float cov[3][3];
        static const int ia[6] = {0, 0, 0, 1, 1, 2}, ib[6] = {0, 1, 2, 1, 2, 2};  // xx xy xz yy yz zz
#if defined(ORC_VAR_FIT_COV_TREE) || defined(ORC_VAR_FIT_FLOAT)
        double acc[6];
        for (int q = 0; q < 6; ++q)
            acc[q] = blockedSum(n, [&](size_t j) {
                const float* p = xyz4 + 4 * (size_t)ids[j];
                const float ca = p[ia[q]] - mean[ia[q]], cb = p[ib[q]] - mean[ib[q]];
                return (double)ca * (double)cb;
            });
        const double denom = (double)((long)n - 1);
        for (int q = 0; q < 6; ++q) cov[ia[q]][ib[q]] = cov[ib[q]][ia[q]] = (float)(acc[q] / denom);
#else
        // MatrixXf centered = subset.rowwise() - mean (float subtraction per element), then the product above, Gaussians.h:146-147
        float acc[6];
        for (int q = 0; q < 6; ++q)
            acc[q] = gemm_dot_f32(
                n, [&](size_t j) { return xyz4[4 * (size_t)ids[j] + ia[q]] - mean[ia[q]]; }, [&](size_t j) { return xyz4[4 * (size_t)ids[j] + ib[q]] - mean[ib[q]]; });
        // (...) / float(subset.rows() - 1): a float division of every coefficient.  (Dividing the two floats in double and rounding once gives
        // the same bits -- double rounding is innocuous for the quotient of two floats, 53 >= 2 * 24 + 2 -- so "float or double division" is
        // not a separate hypothesis once the sums are floats.)
        const float fd = (float)((long)n - 1);
        for (int q = 0; q < 6; ++q) cov[ia[q]][ib[q]] = cov[ib[q]][ia[q]] = acc[q] / fd;
#endif
        for (int c = 0; c < 3; ++c) fitMean.push_back(mean[c]);
        for (int c = 0; c < 3; ++c)
            for (int r = 0; r < 3; ++r) fitCov.push_back(cov[r][c]);
        limit_covariance(cov);
        float inv[3][3];
        inverse3f(cov, inv);
        for (int c = 0; c < 3; ++c)
            for (int r = 0; r < 3; ++r) info.push_back(inv[r][c]);
        obsWeights.push_back(observationWeight);
        members.insert(members.end(), ids.begin(), ids.end());
        segOffset.push_back((int32_t)members.size());
        ++numPointSets;
    }
    // Gaussians.h:170-179
    void updateRebalancingWeights() {
        weights.resize((size_t)numPointSets);
        rawWeights.resize((size_t)numPointSets);
        for (int k = 0; k < numPointSets; ++k) {
            // numPointsPerSet.cast<float>().array().pow(-1) (:172): scalar_pow_op<float, float> -> std::pow(float, float) = libm's powf
            const float nk = (float)(segOffset[k + 1] - segOffset[k]);
#ifdef ORC_VAR_WEIGHT_DIV
            weights[k] = (1.0f / nk) * obsWeights[k];
#else
            volatile float minus_one = -1.0f;  // (volatile: the compiler must not fold the call into a division)
            weights[k] = powf(nk, minus_one) * obsWeights[k];
#endif
            rawWeights[k] = weights[k];
        }
        // VectorXf::mean() (Gaussians.h:176): `rebalancingWeights.head(M)` starts at its aligned buffer
        const float mean = eigen_mean_f32((size_t)numPointSets, 0, [&](size_t k) { return weights[k]; });
        for (int k = 0; k < numPointSets; ++k) weights[k] = weights[k] / mean;
    }
};

// Gaussians.h:27-85 splitSet for PointNormal clouds
static bool split_set(const float* nrm4, std::vector<int>& ids, std::vector<int>& ids2) {
    float minDiff = std::numeric_limits<float>::max();
    int best1 = 0, best2 = 0;
    for (int id1 : ids) {
        for (int id2 : ids) {
            if (id1 == id2) continue;
            const float* a = nrm4 + 4 * (size_t)id1;
            const float* b = nrm4 + 4 * (size_t)id2;
            const float d = normf3(a[0] + b[0], a[1] + b[1], a[2] + b[2]);
            if (d < minDiff) minDiff = d, best1 = id1, best2 = id2;
        }
    }
    if (minDiff > 0.5f) return false;
    const float r1[3] = {nrm4[4 * (size_t)best1], nrm4[4 * (size_t)best1 + 1], nrm4[4 * (size_t)best1 + 2]};
    const float r2[3] = {nrm4[4 * (size_t)best2], nrm4[4 * (size_t)best2 + 1], nrm4[4 * (size_t)best2 + 2]};
    std::vector<int> s1, s2;
    for (int id : ids) {
        const float* v = nrm4 + 4 * (size_t)id;
        const float d1 = normf3(r1[0] - v[0], r1[1] - v[1], r1[2] - v[2]);
        const float d2 = normf3(r2[0] - v[0], r2[1] - v[1], r2[2] - v[2]);
        if (d1 < d2)
            s1.push_back(id);
        else
            s2.push_back(id);
    }
    ids = s1, ids2 = s2;
    return true;
}

// DmsaOptimizer.h:275-350 createGaussianSets
static int create_gaussian_sets(Gaussians& g, const float* xyz4, const float* nrm4, const int32_t* ids, int64_t n, float resolution,
                                int minNumberPts, bool splitEnabled) {
    VoxelResult vox;
    const int rc = voxelize(xyz4, n, (double)resolution, vox);
    if (rc != DMSA_OK) return rc;
    std::vector<int> indices, indices2;
    auto diverse = [&](const std::vector<int>& idx) {
        if (idx.empty()) return false;
        int mx = std::numeric_limits<int>::min(), mn = std::numeric_limits<int>::max();
        for (int i : idx) mx = std::max(mx, ids[i]), mn = std::min(mn, ids[i]);
        return mx != mn;
    };
    size_t j = 0;
    const size_t total = vox.order.size();
    while (j < total) {
        size_t e = j + 1;
        while (e < total && vox.code[vox.order[e]] == vox.code[vox.order[j]]) ++e;
        indices.assign(vox.order.begin() + j, vox.order.begin() + e);
        indices2.clear();
        j = e;
        if ((int)indices.size() >= minNumberPts && diverse(indices)) {
            if (splitEnabled && nrm4 != nullptr && split_set(nrm4, indices, indices2)) {
                // quirks kept: strict '>' and the second diversity test reads `indices`, not `indices2`
                const bool div1 = diverse(indices);
                if ((int)indices.size() > minNumberPts && div1) g.addPointSet(indices, xyz4, 1.0f);
                if ((int)indices2.size() > minNumberPts && div1) g.addPointSet(indices2, xyz4, 1.0f);
            } else {
                g.addPointSet(indices, xyz4, 1.0f);
            }
        }
    }
    return DMSA_OK;
}

// DmsaOptimizer.h:242-268: point-to-Gaussian rows of updateErrorTerms
static void eval_residuals(const Gaussians& g, const float* xyz4, double* e) {
    for (int k = 0; k < g.numPointSets; ++k) {
        const int32_t b = g.segOffset[k], en = g.segOffset[k + 1];
        float mean[3] = {0.0f, 0.0f, 0.0f};
        for (int32_t j = b; j < en; ++j) {
            const float* p = xyz4 + 4 * (size_t)g.members[j];
            mean[0] = mean[0] + p[0], mean[1] = mean[1] + p[1], mean[2] = mean[2] + p[2];
        }
        const float nf = (float)(en - b);
        mean[0] = mean[0] / nf, mean[1] = mean[1] / nf, mean[2] = mean[2] / nf;
        const float* A = &g.info[9 * (size_t)k];  // column-major: A(r,c) = A[3*c + r]
        const float w = g.weights[k];
        double acc = 0.0;
        for (int32_t j = b; j < en; ++j) {
            const float* p = xyz4 + 4 * (size_t)g.members[j];
            const float d0 = p[0] - mean[0], d1 = p[1] - mean[1], d2 = p[2] - mean[2];
            // ((float(w) * d^T) * A) * d, 3-term sums as x0 + (x1 + x2); the float 1x1 result is added to a double
#ifdef ORC_VAR_MAHA_ASSOC
            const float u0 = sum3(d0 * A[0], d1 * A[1], d2 * A[2]);
            const float u1 = sum3(d0 * A[3], d1 * A[4], d2 * A[5]);
            const float u2 = sum3(d0 * A[6], d1 * A[7], d2 * A[8]);
            const float q = w * sum3(u0 * d0, u1 * d1, u2 * d2);
#else
            const float wd0 = w * d0, wd1 = w * d1, wd2 = w * d2;
            const float v0 = sum3(wd0 * A[0], wd1 * A[1], wd2 * A[2]);
            const float v1 = sum3(wd0 * A[3], wd1 * A[4], wd2 * A[5]);
            const float v2 = sum3(wd0 * A[6], wd1 * A[7], wd2 * A[8]);
            const float q = sum3(v0 * d0, v1 * d1, v2 * d2);
#endif
            acc += (double)q;
        }
        e[k] = std::sqrt(std::fabs(acc));
    }
}

// ------------------------------------------------------------------------------------------------
// OptimizablePointSet (OptimizablePointSet.h:18-56)
// ------------------------------------------------------------------------------------------------
struct PointSet {
    std::vector<float> globalPoints;  // n x 4
    std::vector<float> globalNormals; // n x 4 (keyframe model only)
    std::vector<int32_t> ids;
    float minGridSize = 0.3f;
    bool hasNormals = false;
    virtual ~PointSet() {}
    virtual std::vector<double>& getAdditionalErrorTerms() = 0;
    virtual void updateGlobalPoints() = 0;
    virtual int updateAdditionalErrors() = 0;
    virtual void getPoseParameters(std::vector<double>& p) = 0;
    virtual void setPoseParameters(const std::vector<double>& p) = 0;
    virtual void centralize() = 0;
    virtual void decentralize() = 0;
    virtual PointSet* clone() const = 0;  // independent copy (parallel evaluation variant of the CPU baseline)
    int64_t numPoints() const { return (int64_t)ids.size(); }
};

// ContinuousTrajectory.h:24-669 (hot methods only)
struct WindowModel : PointSet {
    PointSet* clone() const override { return new WindowModel(*this); }
    ConsecutivePoses controlPoses;
    std::vector<double> stamps, trajTime;
    int n_total = 0;
    Poses denseGlobalPoses;
    std::vector<float> denseTforms;  // n_total x 12
    std::vector<float> local;        // N x 4
    std::vector<int32_t> tformId;
    int64_t N = 0, S = 0;
    bool useImuErrorTerms = false;
    double dt_res = 0.001, balancingImu = 0.001, gravity[3] = {0, 0, -9.805};
    std::vector<int32_t> paramIndices;
    std::vector<double> preintRot, preintPos, preintVel, covInv;
    std::vector<double> imuFactorError;
    double origin[3] = {0, 0, 0};

    explicit WindowModel(const dmsa_window_problem& p) {
        const int C = p.num_control_poses;
        controlPoses.resize(C);
        std::copy(p.rel_orient, p.rel_orient + 3 * C, controlPoses.rel.O.begin());
        std::copy(p.rel_transl, p.rel_transl + 3 * C, controlPoses.rel.T.begin());
        stamps.assign(p.stamps, p.stamps + C);
        n_total = p.n_total;
        trajTime.assign(p.traj_time, p.traj_time + n_total);
        denseGlobalPoses.resize(n_total);
        denseTforms.assign((size_t)n_total * 12, 0.0f);
        N = p.num_points, S = p.num_static;
        local.assign(p.xyz_local, p.xyz_local + 4 * N);
        tformId.assign(p.tform_idx, p.tform_idx + N);
        globalPoints.assign((size_t)(N + S) * 4, 1.0f);
        ids.resize((size_t)(N + S));
        std::copy(p.ring_id, p.ring_id + N, ids.begin());
        for (int64_t k = 0; k < S; ++k) {  // addStaticPoints :158-172
            for (int c = 0; c < 3; ++c) globalPoints[4 * (size_t)(N + k) + c] = p.xyz_static[4 * k + c];
            ids[(size_t)(N + k)] = p.ring_id_static[k];
        }
        minGridSize = p.min_grid_size;
        useImuErrorTerms = p.use_imu != 0;
        if (useImuErrorTerms) {
            dt_res = p.dt_res, balancingImu = p.balancing_imu;
            for (int c = 0; c < 3; ++c) gravity[c] = p.gravity[c];
            paramIndices.assign(p.param_indices, p.param_indices + C);
            preintRot.assign(p.preint_rot, p.preint_rot + 9 * C);
            preintPos.assign(p.preint_pos, p.preint_pos + 3 * C);
            preintVel.assign(p.preint_vel, p.preint_vel + 3 * C);
            covInv.assign(p.cov_pvrot_inv, p.cov_pvrot_inv + 81 * C);
            imuFactorError.assign((size_t)(C - 1), 0.0);
        }
    }
    // :75-88
    void centralize() override {
        for (int c = 0; c < 3; ++c) origin[c] = controlPoses.rel.T[c], controlPoses.rel.T[c] = 0.0;
        controlPoses.relative2global();
        for (int64_t k = N; k < N + S; ++k)
            for (int c = 0; c < 3; ++c) globalPoints[4 * (size_t)k + c] = globalPoints[4 * (size_t)k + c] - (float)origin[c];
    }
    // :89-100
    void decentralize() override {
        controlPoses.global2relative();
        for (int c = 0; c < 3; ++c) controlPoses.rel.T[c] = origin[c];
        controlPoses.relative2global();
        for (int64_t k = N; k < N + S; ++k)
            for (int c = 0; c < 3; ++c) globalPoints[4 * (size_t)k + c] = globalPoints[4 * (size_t)k + c] + (float)origin[c];
    }
    std::vector<double>& getAdditionalErrorTerms() override { return imuFactorError; }
    int updateAdditionalErrors() override {  // :107-117
        if (useImuErrorTerms) {
            updateImuError();
            return (int)imuFactorError.size();
        }
        return 0;
    }
    void getPoseParameters(std::vector<double>& p) override { controlPoses.rel.getParamsAsVector(p); }
    void setPoseParameters(const std::vector<double>& p) override { controlPoses.rel.setParamsFromVector(p); }
    // :570-591
    void getInterpRotation(double t, double* out) const {
        const int C = controlPoses.numPoses;
        const double* beg = stamps.data();
        const double* it = std::lower_bound(beg, beg + C - 1, t);
        const long rightIndex = it - beg;
        if (rightIndex > 0) {
            const double t_rel = (t - stamps[rightIndex - 1]) / (stamps[rightIndex] - stamps[rightIndex - 1]);
            slerp(&controlPoses.glob.O[3 * (rightIndex - 1)], &controlPoses.glob.O[3 * rightIndex], t_rel, out);
        } else {
            for (int c = 0; c < 3; ++c) out[c] = controlPoses.glob.O[c];
        }
    }
    // :189-226
    void updateTrajDenseTforms() {
        controlPoses.relative2global();
        for (int k = 0; k < n_total; ++k) getInterpRotation(trajTime[k], &denseGlobalPoses.O[3 * (size_t)k]);
        const int C = controlPoses.numPoses;
        std::vector<double> tr((size_t)C);
        for (int a = 0; a < 3; ++a) {
            for (int k = 0; k < C; ++k) tr[k] = controlPoses.glob.T[3 * k + a];
            BarycentricRational s(stamps.data(), tr.data(), C, 2);
            for (int j = 0; j < n_total; ++j) denseGlobalPoses.T[3 * (size_t)j + a] = s(trajTime[j]);
        }
        for (int k = 0; k < n_total; ++k) {
            const M3 R = axang2rotm(&denseGlobalPoses.O[3 * (size_t)k]);
            float* T = &denseTforms[12 * (size_t)k];
            for (int r = 0; r < 3; ++r) {
                for (int c = 0; c < 3; ++c) T[4 * r + c] = (float)R.m[r][c];
                T[4 * r + 3] = (float)denseGlobalPoses.T[3 * (size_t)k + r];
            }
        }
    }
    // :129-156
    void updateGlobalPoints() override {
        updateTrajDenseTforms();
        for (int64_t i = 0; i < N; ++i) tform_point(&denseTforms[12 * (size_t)tformId[i]], &local[4 * (size_t)i], &globalPoints[4 * (size_t)i]);
    }
    // :603-663
    void updateImuError() {
        controlPoses.global2relative();
        std::fill(imuFactorError.begin(), imuFactorError.end(), 0.0);
        const double one_div_t_res = 1.0 / dt_res;
        const int C = controlPoses.numPoses;
        const double* DT = denseGlobalPoses.T.data();
        for (int k = 1; k < C; ++k) {
            const M3 Rs = axang2rotm(&controlPoses.glob.O[3 * (k - 1)]);
            const M3 Rst = transpose(Rs);
            const double delta_t = stamps[k] - stamps[k - 1];
            double v_start[3], v_end[3], tmp[3], dp_model[3], dv_model[3], rot_err[3];
            const int i0 = paramIndices[k - 1], i1 = paramIndices[k];
            for (int c = 0; c < 3; ++c) {
                v_start[c] = one_div_t_res * (DT[3 * (size_t)(i0 + 1) + c] - DT[3 * (size_t)i0 + c]);
                v_end[c] = one_div_t_res * (DT[3 * (size_t)i1 + c] - DT[3 * (size_t)(i1 - 1) + c]);
            }
            const double half_dt2 = 0.5 * std::pow(delta_t, 2);
            for (int c = 0; c < 3; ++c)
                tmp[c] = controlPoses.glob.T[3 * k + c] - controlPoses.glob.T[3 * (k - 1) + c] - v_start[c] * delta_t - half_dt2 * gravity[c];
            matvec(Rst, tmp, dp_model);
            const M3 Rend = axang2rotm(&controlPoses.rel.O[3 * k]);
            M3 P;  // preintImuRots[k], column-major storage
            for (int r = 0; r < 3; ++r)
                for (int c = 0; c < 3; ++c) P.m[r][c] = preintRot[9 * (size_t)k + 3 * c + r];
            rotm2axang(mul(transpose(P), Rend), rot_err);
            for (int c = 0; c < 3; ++c) tmp[c] = v_end[c] - v_start[c] - gravity[c] * delta_t;
            matvec(Rst, tmp, dv_model);
            double ce[9];
            for (int c = 0; c < 3; ++c) {
                ce[c] = rot_err[c];
                ce[3 + c] = dv_model[c] - preintVel[3 * (size_t)k + c];
                ce[6 + c] = dp_model[c] - preintPos[3 * (size_t)k + c];
            }
            // combined_error^T * CovPVRot_inv[k] * combined_error
            const double* Ci = &covInv[81 * (size_t)k];  // column-major 9x9
            double row[9];
            for (int j = 0; j < 9; ++j) {
                double s = 0.0;
                for (int i = 0; i < 9; ++i) s += ce[i] * Ci[9 * j + i];
                row[j] = s;
            }
            double q = 0.0;
            for (int j = 0; j < 9; ++j) q += row[j] * ce[j];
            q *= balancingImu;
            imuFactorError[(size_t)(k - 1)] = std::sqrt(q);
        }
    }
};

// MapManagement.h:20-390 (hot methods only)
struct KeyframeModel : PointSet {
    PointSet* clone() const override { return new KeyframeModel(*this); }
    ConsecutivePoses keyframePoses;
    int F = 0;
    std::vector<int64_t> frameOffset;
    std::vector<float> local, localNormals;
    std::vector<float> tforms;  // F x 12
    bool useGravity = false, useOdometry = false;
    double gravity[3] = {0, 0, -9.805};
    double covGravInv[9], balancingGrav = 1.0, balancingOdom = 1000.0;
    std::vector<double> measuredGravity, odomTransl, odomOrientMat;
    std::vector<int32_t> gravityPlausible;
    double odomTranslCovInv[9], odomOrientCovInv[9];
    std::vector<double> gravityErrorTerm, odometryErrorTerm, additionalErrors;

    explicit KeyframeModel(const dmsa_keyframe_problem& p) {
        F = p.num_frames;
        keyframePoses.resize(F);
        std::copy(p.rel_orient, p.rel_orient + 3 * F, keyframePoses.rel.O.begin());
        std::copy(p.rel_transl, p.rel_transl + 3 * F, keyframePoses.rel.T.begin());
        keyframePoses.relative2global();
        frameOffset.assign(p.frame_offset, p.frame_offset + F + 1);
        const int64_t n = frameOffset[F];
        local.assign(p.xyz_local, p.xyz_local + 4 * n);
        localNormals.assign(p.normal_local, p.normal_local + 4 * n);
        ids.assign(p.ring_id, p.ring_id + n);
        globalPoints.assign((size_t)n * 4, 1.0f);
        globalNormals.assign((size_t)n * 4, 0.0f);
        hasNormals = true;
        tforms.assign((size_t)F * 12, 0.0f);
        minGridSize = p.min_grid_size;
        useGravity = p.use_gravity != 0, useOdometry = p.use_odometry != 0;
        for (int c = 0; c < 3; ++c) gravity[c] = p.gravity[c];
        std::copy(p.cov_grav_inv, p.cov_grav_inv + 9, covGravInv);
        balancingGrav = p.balancing_grav, balancingOdom = p.balancing_odom;
        if (useGravity) {
            measuredGravity.assign(p.measured_gravity, p.measured_gravity + 3 * F);
            gravityPlausible.assign(p.gravity_plausible, p.gravity_plausible + F);
        }
        if (useOdometry) {
            odomTransl.assign(p.odom_rel_transl, p.odom_rel_transl + 3 * F);
            odomOrientMat.assign(p.odom_rel_orient_mat, p.odom_rel_orient_mat + 9 * F);
            std::copy(p.odom_transl_cov_inv, p.odom_transl_cov_inv + 9, odomTranslCovInv);
            std::copy(p.odom_orient_cov_inv, p.odom_orient_cov_inv + 9, odomOrientCovInv);
        }
    }
    void centralize() override {}    // MapManagement.h:73-79 returns immediately
    void decentralize() override {}  // :80-86
    // :120-149 (minGridSize is constant here: the per-keyframe gridSize values are folded into min_grid_size)
    void updateGlobalPoints() override {
        for (int k = 0; k < F; ++k) {
            const M3 R = axang2rotm(&keyframePoses.glob.O[3 * k]);
            float* T = &tforms[12 * (size_t)k];
            for (int r = 0; r < 3; ++r) {
                for (int c = 0; c < 3; ++c) T[4 * r + c] = (float)R.m[r][c];
                T[4 * r + 3] = (float)keyframePoses.glob.T[3 * k + r];
            }
            for (int64_t i = frameOffset[k]; i < frameOffset[k + 1]; ++i) {
                tform_point(T, &local[4 * (size_t)i], &globalPoints[4 * (size_t)i]);
                rot_vec(T, &localNormals[4 * (size_t)i], &globalNormals[4 * (size_t)i]);
            }
        }
    }
    std::vector<double>& getAdditionalErrorTerms() override {  // :151-160
        if (useGravity && !useOdometry) return gravityErrorTerm;
        if (!useGravity && useOdometry) return odometryErrorTerm;
        return additionalErrors;
    }
    int updateAdditionalErrors() override {  // :162-190
        if (!useGravity && !useOdometry) return 0;
        if (useGravity && !useOdometry) {
            updateGravityErrors();
            return (int)gravityErrorTerm.size();
        }
        if (!useGravity && useOdometry) {
            updateOdometryErrors();
            return (int)odometryErrorTerm.size();
        }
        updateGravityErrors();
        updateOdometryErrors();
        additionalErrors = gravityErrorTerm;
        additionalErrors.insert(additionalErrors.end(), odometryErrorTerm.begin(), odometryErrorTerm.end());
        return (int)additionalErrors.size();
    }
    void getPoseParameters(std::vector<double>& p) override { keyframePoses.rel.getParamsAsVector(p); }
    void setPoseParameters(const std::vector<double>& p) override {  // :197-202
        keyframePoses.rel.setParamsFromVector(p);
        keyframePoses.relative2global();
    }
    static double quad3(const double* d, const double* Ci /* col-major 3x3 */) {
        double row[3];
        for (int j = 0; j < 3; ++j) row[j] = d[0] * Ci[3 * j] + d[1] * Ci[3 * j + 1] + d[2] * Ci[3 * j + 2];
        return row[0] * d[0] + row[1] * d[1] + row[2] * d[2];
    }
    // :210-232
    void updateGravityErrors() {
        gravityErrorTerm.assign((size_t)F, 0.0);
        for (int k = 1; k < F; ++k) {
            if (!gravityPlausible[k]) continue;
            double d[3];
            matvec(axang2rotm(&keyframePoses.glob.O[3 * k]), &measuredGravity[3 * (size_t)k], d);
            for (int c = 0; c < 3; ++c) d[c] -= gravity[c];
            double q = quad3(d, covGravInv);
            q *= balancingGrav;
            gravityErrorTerm[(size_t)k] = std::sqrt(q);
        }
    }
    // :234-252
    void updateOdometryErrors() {
        odometryErrorTerm.assign((size_t)(F - 1), 0.0);
        for (int k = 1; k < F; ++k) {
            double td[3], od[3];
            for (int c = 0; c < 3; ++c) td[c] = odomTransl[3 * (size_t)k + c] - keyframePoses.rel.T[3 * k + c];
            M3 Rm;
            for (int r = 0; r < 3; ++r)
                for (int c = 0; c < 3; ++c) Rm.m[r][c] = odomOrientMat[9 * (size_t)k + 3 * c + r];
            rotm2axang(mul(transpose(axang2rotm(&keyframePoses.rel.O[3 * k])), Rm), od);
            double q = 0.0;
            q += quad3(td, odomTranslCovInv);
            q += quad3(od, odomOrientCovInv);
            q *= balancingOdom;
            odometryErrorTerm[(size_t)(k - 1)] = std::sqrt(q);
        }
    }
};

// ------------------------------------------------------------------------------------------------
// dense double algebra for the LM step (DmsaOptimizer.h:107-113)
// ------------------------------------------------------------------------------------------------
// MatrixXd::inverse() == partial-pivot LU; Gauss-Jordan with partial pivoting on [H | I]
#ifndef ORC_VAR_LM_BLOCKED_LU
static bool invert_dense(std::vector<double> A /* col-major PxP */, int P, std::vector<double>& inv) {
    inv.assign((size_t)P * P, 0.0);
    for (int i = 0; i < P; ++i) inv[(size_t)i * P + i] = 1.0;
    auto at = [&](std::vector<double>& M, int r, int c) -> double& { return M[(size_t)c * P + r]; };
    for (int col = 0; col < P; ++col) {
        int piv = col;
        double best = std::fabs(at(A, col, col));
        for (int r = col + 1; r < P; ++r)
            if (std::fabs(at(A, r, col)) > best) best = std::fabs(at(A, r, col)), piv = r;
        if (piv != col)
            for (int c = 0; c < P; ++c) std::swap(at(A, col, c), at(A, piv, c)), std::swap(at(inv, col, c), at(inv, piv, c));
        const double d = at(A, col, col);
        for (int c = 0; c < P; ++c) at(A, col, c) /= d, at(inv, col, c) /= d;
        for (int r = 0; r < P; ++r) {
            if (r == col) continue;
            const double f = at(A, r, col);
            if (f == 0.0) continue;
            for (int c = 0; c < P; ++c) at(A, r, c) -= f * at(A, col, c), at(inv, r, c) -= f * at(inv, col, c);
        }
    }
    return true;
}
#else
// ORC_VAR_LM_BLOCKED_LU: the shape of Eigen 3.4's PartialPivLU behind MatrixXd::inverse() (Eigen/src/LU/PartialPivLU.h: partial_lu_impl::
// blocked_lu) -- right-looking LU in column panels of blockSize = min(max((size / 8 / 16) * 16, 8), 256) columns (8 for P = 30 .. 255; at most
// 16 columns are factored unblocked), each panel factored by rank-1 updates with partial pivoting, A12 <- L11^-1 A12 by forward substitution,
// A22 <- A22 - A21 * A12 with the PRODUCT summed first over the panel's depth and subtracted once (what gebp's `res += alpha * C` does with
// alpha = -1); then inverse() = U^-1 L^-1 P by two triangular solves on the permuted identity.  The sums inside the solves and the products
// are sequential in the depth index; Eigen's register blocking is not restated -- this switch measures what the blocked ORDER is worth.
static bool invert_dense(std::vector<double> A /* col-major PxP */, int P, std::vector<double>& inv) {
    auto at = [&](std::vector<double>& M, int r, int c) -> double& { return M[(size_t)c * P + r]; };
    std::vector<int> transp((size_t)P);
    auto unblocked = [&](int k0, int bs) {  // unblocked_lu on rows k0 .. P-1, columns k0 .. k0+bs-1
        for (int k = k0; k < k0 + bs; ++k) {
            int piv = k;
            double best = std::fabs(at(A, k, k));
            for (int r = k + 1; r < P; ++r)
                if (std::fabs(at(A, r, k)) > best) best = std::fabs(at(A, r, k)), piv = r;
            transp[(size_t)k] = piv;
            if (best != 0.0) {
                if (piv != k)
                    for (int c = k0; c < k0 + bs; ++c) std::swap(at(A, k, c), at(A, piv, c));
                const double d = at(A, k, k);
                for (int r = k + 1; r < P; ++r) at(A, r, k) /= d;
            }
            for (int c = k + 1; c < k0 + bs; ++c)
                for (int r = k + 1; r < P; ++r) at(A, r, c) -= at(A, r, k) * at(A, k, c);
        }
    };
    int blockSize = P / 8;
    blockSize = (blockSize / 16) * 16;
    blockSize = std::min(std::max(blockSize, 8), 256);
    if (P <= 16) blockSize = P;
    for (int k = 0; k < P; k += blockSize) {
        const int bs = std::min(P - k, blockSize);
        for (int kk = k; kk < k + bs; kk += 16) unblocked(kk, std::min(16, k + bs - kk));  // (a 16-column inner blocking would recurse the same way; bs <= 16 here for P <= 255)
        for (int i = k; i < k + bs; ++i) {  // the panel's row swaps on the columns left and right of it
            const int piv = transp[(size_t)i];
            if (piv == i) continue;
            for (int c = 0; c < k; ++c) std::swap(at(A, i, c), at(A, piv, c));
            for (int c = k + bs; c < P; ++c) std::swap(at(A, i, c), at(A, piv, c));
        }
        for (int c = k + bs; c < P; ++c) {  // A12 = L11^-1 A12 (unit lower), then A22 -= A21 * A12
            for (int i = k; i < k + bs; ++i) {
                const double b = at(A, i, c);
                for (int r = i + 1; r < k + bs; ++r) at(A, r, c) -= b * at(A, r, i);
            }
            for (int r = k + bs; r < P; ++r) {
                double C = 0.0;
                for (int i = k; i < k + bs; ++i) C = at(A, r, i) * at(A, i, c) + C;
                at(A, r, c) += -1.0 * C;
            }
        }
    }
    // inverse(): dst = P * I; L (unit lower) solve; U solve
    inv.assign((size_t)P * P, 0.0);
    // P * I: the transpositions applied to the identity's rows in order
    std::vector<double> B((size_t)P * P, 0.0);
    for (int i = 0; i < P; ++i) B[(size_t)i * P + i] = 1.0;
    for (int i = 0; i < P; ++i) {
        const int piv = transp[(size_t)i];
        if (piv != i)
            for (int c = 0; c < P; ++c) std::swap(B[(size_t)c * P + i], B[(size_t)c * P + piv]);
    }
    for (int c = 0; c < P; ++c) {
        double* x = &B[(size_t)c * P];
        for (int i = 0; i < P; ++i) {  // forward, unit diagonal, column-oriented like Eigen's small-panel kernel
            const double b = x[i];
            if (b != 0.0)
                for (int r = i + 1; r < P; ++r) x[r] -= b * at(A, r, i);
        }
        for (int i = P - 1; i >= 0; --i) {  // backward
            x[i] /= at(A, i, i);
            const double b = x[i];
            if (b != 0.0)
                for (int r = 0; r < i; ++r) x[r] -= b * at(A, r, i);
        }
    }
    inv = B;
    return true;
}
#endif

// Summation order of H = J^T J, g = J^T e and e^T e (DmsaOptimizer.h:101-113).  The reference computes them with Eigen's blocked,
// vectorised (and up to 4-thread) GEMM / GEMV / dot, whose order cannot be known; this restatement fixes one that is easy to state
// and easy to parallelise: rows are cut into consecutive blocks of reduction_block_rows(rows, P), every block is summed row by
// row, the block sums are added in order.  (The HIP kernels use the same rule, so the two agree to the last bit.)
static int reduction_block_rows(int rows, int P) {
    int rs = 256;
    if (P > 64) {
        const int want = (rows + 31) / 32;
        rs = ((want + 31) / 32) * 32;
        if (rs < 256) rs = 256;
    }
    return rs;
}
// x^T y in that order.  For P <= 64 every step is a separately rounded multiply and add (the reference is built without FMA,
// CMakeLists.txt:13-17).  For P > 64 -- the keyframe pass, where J^T J is a real contraction and runs on the matrix cores -- every
// step is ONE fused multiply-add, s = fma(x[r], y[r], s), row by row: exactly what chained v_mfma_f64_16x16x4_f64 instructions
// compute (verified bit for bit: scripts/microbench/mfma_f64_semantics.hip).  Eigen's GEMM order and rounding are unknowable either
// way; what matters is that H, g, e0^T e0 and the line search's e^T e all follow ONE rule.
static double blocked_dot(int rows, int P, const double* x, const double* y) {
    const int rs = reduction_block_rows(rows, P);
#ifdef ORC_VAR_JTJ_NOFMA
    const bool fused = false;
#else
    const bool fused = P > 64;
#endif
    double total = 0.0;
    for (int r0 = 0; r0 < rows; r0 += rs) {
        double s = 0.0;
        for (int r = r0; r < std::min(rows, r0 + rs); ++r) s = fused ? std::fma(x[r], y[r], s) : s + x[r] * y[r];
        total += s;
    }
    return total;
}

// :110-113 on a given damped H (col-major P x P, need not be symmetric) and g: the explicit inverse, then
// step = -alpha * H^-1 * g   (evaluated as (-alpha*H^-1) * g).  The one statement behind lm_step and orc_lm_solve.
static void lm_solve(const std::vector<double>& H, const double* g, int P, double alpha, std::vector<double>& step) {
    std::vector<double> Hinv;
    invert_dense(H, P, Hinv);
    step.assign((size_t)P, 0.0);
    for (int i = 0; i < P; ++i) {
        double s = 0.0;
        for (int j = 0; j < P; ++j) s += (-alpha * Hinv[(size_t)j * P + i]) * g[(size_t)j];
        step[(size_t)i] = s;
    }
}

static void lm_step(const double* e0, const double* J /* col-major rows x P */, int rows, int P, double lambda, double alpha,
                    std::vector<double>& H, std::vector<double>& g, std::vector<double>& step) {
    H.assign((size_t)P * P, 0.0);
    g.assign((size_t)P, 0.0);
    for (int i = 0; i < P; ++i) {
        const double* Ji = J + (size_t)i * rows;
        for (int j = i; j < P; ++j) {
            const double* Jj = J + (size_t)j * rows;
            const double s = blocked_dot(rows, P, Ji, Jj);
            H[(size_t)j * P + i] = s, H[(size_t)i * P + j] = s;
        }
        g[(size_t)i] = blocked_dot(rows, P, Ji, e0);
    }
    for (int i = 0; i < P; ++i) H[(size_t)i * P + i] += lambda;  // :110
#ifdef ORC_VAR_STEP_LEFT_ASSOC
    std::vector<double> Hinv;
    invert_dense(H, P, Hinv);
    step.assign((size_t)P, 0.0);
    // Eigen evaluates the chain left to right: T1 = (-alpha) * H^-1 coefficient-wise (an Inverse has no direct access, the scaled expression is
    // evaluated into a temporary), T2 = T1 * J^T by the general matrix product (P x P by P x rows: per coefficient one chain over the depth
    // P < kc, starting from the first product, stored as 0 + 1 * C), step = T2 * e by the column-major matrix-vector kernel: columns in blocks
    // of 16 (rows * 8 bytes < 32000), per block a chain c = c + T2(i, j) e(j), res(i) = res(i) + 1 * c.
    {
        std::vector<double> T1((size_t)P * P), T2((size_t)P * rows);
        for (size_t k = 0; k < T1.size(); ++k) T1[k] = -alpha * Hinv[k];
        for (int r = 0; r < rows; ++r)
            for (int i = 0; i < P; ++i) {
                double C = 0.0;
                for (int k = 0; k < P; ++k) C = T1[(size_t)k * P + i] * J[(size_t)k * rows + r] + C;
                T2[(size_t)r * P + i] = 0.0 + 1.0 * C;
            }
        for (int i = 0; i < P; ++i) {
            double res = 0.0;
            for (int j0 = 0; j0 < rows; j0 += 16) {
                double c = 0.0;
                for (int j = j0; j < std::min(rows, j0 + 16); ++j) c = T2[(size_t)j * P + i] * e0[j] + c;
                res = c * 1.0 + res;
            }
            step[(size_t)i] = res;
        }
    }
#else
    lm_solve(H, g.data(), P, alpha, step);
#endif
}

// ------------------------------------------------------------------------------------------------
// DmsaOptimizer (DmsaOptimizer.h:41-364)
// ------------------------------------------------------------------------------------------------
// Number of threads for the evaluation-parallel variant of the CPU baseline (orc_set_threads).  1 = the reference's own
// execution order (it runs every evaluation on one thread, DmsaOptimizer.h:56-57 only caps Eigen's GEMM threads).  With T > 1
// the P forward differences and the 9 line-search trials run on independent copies of the point set; the LAST evaluation of
// each batch still runs on the caller's set, so the state the reference leaves behind (quirks q2, q9) is unchanged.  Results are
// bit-identical to T = 1 unless IMU rows are on: updateImuError carries state from one evaluation to the next, which copies
// cannot reproduce (differences ~1e-12).  Parity tests always run with T = 1.
static int g_threads = 1;

struct Optimizer {
    Gaussians currentGauss;
    std::vector<double> Jacobian;  // col-major rows x P
    int evaluations = 0;

    // updateErrorTerms on an arbitrary copy of the set, without touching the optimizer's own state
    void evalOn(PointSet& set, std::vector<double>& errorVec) const {
        const int numAdd = set.updateAdditionalErrors();
        errorVec.resize((size_t)currentGauss.numPointSets + numAdd);
        eval_residuals(currentGauss, set.globalPoints.data(), errorVec.data());
        if (numAdd > 0) {
            const std::vector<double>& add = set.getAdditionalErrorTerms();
            std::copy(add.begin(), add.begin() + numAdd, errorVec.begin() + currentGauss.numPointSets);
        }
    }

    // :234-273
    void updateErrorTerms(PointSet& set, std::vector<double>& errorVec) {
        const int numAdd = set.updateAdditionalErrors();
        errorVec.resize((size_t)currentGauss.numPointSets + numAdd);
        eval_residuals(currentGauss, set.globalPoints.data(), errorVec.data());
        if (numAdd > 0) {
            const std::vector<double>& add = set.getAdditionalErrorTerms();
            std::copy(add.begin(), add.begin() + numAdd, errorVec.begin() + currentGauss.numPointSets);
        }
        ++evaluations;
    }
    static double dot(const std::vector<double>& a) {
        double s = 0.0;
        for (double v : a) s += v * v;
        return s;
    }
    // e^T e in the blocked order of the normal equations (see reduction_block_rows)
    static double dotRows(const std::vector<double>& a, int P) {
        return blocked_dot((int)a.size(), P, a.data(), a.data());
    }
    // :199-232
    void calcNumericJacobian(std::vector<double>& error0, PointSet& set) {
        std::vector<double> origin, loop, errorVec;
        set.getPoseParameters(origin);
        const size_t rows = error0.size(), P = origin.size();
        Jacobian.assign(rows * P, 0.0);
        const double increment = 1.0 * std::sqrt((double)std::numeric_limits<float>::epsilon());
        const double one_div_incr = 1.0 / increment;
        size_t k_serial = 0;
#ifdef _OPENMP
        if (g_threads > 1 && P > 1) {
#pragma omp parallel num_threads(g_threads)
            {
                std::unique_ptr<PointSet> mine(set.clone());
                std::vector<double> lp, ev;
#pragma omp for schedule(dynamic, 1)
                for (long k = 0; k < (long)P - 1; ++k) {
                    lp = origin;
                    lp[(size_t)k] += increment;
                    mine->setPoseParameters(lp);
                    mine->updateGlobalPoints();
                    evalOn(*mine, ev);
                    for (size_t r = 0; r < rows; ++r) Jacobian[(size_t)k * rows + r] = one_div_incr * (ev[r] - error0[r]);
                }
            }
            evaluations += (int)P - 1;
            k_serial = P - 1;
        }
#endif
        for (size_t k = k_serial; k < P; ++k) {
            loop = origin;
            loop[k] += increment;
            set.setPoseParameters(loop);
            set.updateGlobalPoints();
            updateErrorTerms(set, errorVec);
            for (size_t r = 0; r < rows; ++r) Jacobian[k * rows + r] = one_div_incr * (errorVec[r] - error0[r]);
        }
        set.setPoseParameters(origin);
    }
    // :152-182
    int adaptiveStepSize(PointSet& set, std::vector<double>& params, const std::vector<double>& step, double error0) {
        double minError = error0;
        int best = 0;
        const std::vector<double> raw = params;
        std::vector<double> errorVec, test(raw.size());
        double trialError[10] = {0};
        int k_serial = 1;
#ifdef _OPENMP
        if (g_threads > 1) {
#pragma omp parallel num_threads(g_threads)
            {
                std::unique_ptr<PointSet> mine(set.clone());
                std::vector<double> tp(raw.size()), ev;
#pragma omp for schedule(dynamic, 1)
                for (int k = 1; k < 9; ++k) {
                    for (size_t i = 0; i < raw.size(); ++i) tp[i] = raw[i] + 0.1 * (double)k * step[i];
                    mine->setPoseParameters(tp);
                    mine->updateGlobalPoints();
                    evalOn(*mine, ev);
                    trialError[k] = dotRows(ev, (int)raw.size());
                }
            }
            evaluations += 8;
            k_serial = 9;
        }
#endif
        for (int k = 1; k < 10; ++k) {
            for (size_t i = 0; i < raw.size(); ++i) test[i] = raw[i] + 0.1 * (double)k * step[i];
            double errorTest;
            if (k >= k_serial) {
                set.setPoseParameters(test);
                set.updateGlobalPoints();
                updateErrorTerms(set, errorVec);
                errorTest = dotRows(errorVec, (int)raw.size());
            } else {
                errorTest = trialError[k];
            }
            if (errorTest < minError) params = test, minError = errorTest, best = k;
        }
        return best;
    }
    // Iteration 0 of optimizeSet (:62-128) stage by stage, every intermediate result written to `path` in the 'DMSAST03' layout of
    // dmsa_lidar_slam_amd/dump.py -- the same file oracle/ref_harness/ref_main.cpp writes from the REAL reference, so that a run of the
    // harness elsewhere can be compared with this restatement statement by statement (tests/test_ref_fixtures.py).  inject_info /
    // inject_weights (optional, M x 9 / M floats): the reference's own information matrices and weights replace the fitted ones after
    // the Gaussians are built, which isolates the residual / Jacobian statements from the fit's.
    int stageDump(PointSet& set, const dmsa_settings& s, int model, const float* table, int table_rows, const float* inject_info,
                  const float* inject_weights, int inject_M, const char* path) {
        std::vector<double> paramVec, errorVec, optimStep;
        if (s.use_centralization) set.centralize();
        set.getPoseParameters(paramVec);
        set.updateGlobalPoints();
        currentGauss.reset();
        const float* nrm = set.hasNormals ? set.globalNormals.data() : nullptr;
        if (s.grid_size_1_factor > std::numeric_limits<float>::min()) {
            const int rc = create_gaussian_sets(currentGauss, set.globalPoints.data(), nrm, set.ids.data(), set.numPoints(), s.grid_size_1_factor * set.minGridSize,
                                                s.min_num_points_per_set, s.gauss_split != 0);
            if (rc != DMSA_OK) return rc;
        }
        currentGauss.numLevel1 = currentGauss.numPointSets;
        if (s.grid_size_2_factor > std::numeric_limits<float>::min()) {
            const int rc = create_gaussian_sets(currentGauss, set.globalPoints.data(), nrm, set.ids.data(), set.numPoints(), s.grid_size_2_factor * set.minGridSize,
                                                s.min_num_points_per_set, s.gauss_split != 0);
            if (rc != DMSA_OK) return rc;
        }
        currentGauss.updateRebalancingWeights();
        const int M = currentGauss.numPointSets;
        if (inject_info || inject_weights) {
            if (inject_M != M) return DMSA_ERR_INVALID;
            if (inject_info) std::copy(inject_info, inject_info + 9 * (size_t)M, currentGauss.info.begin());
            if (inject_weights) std::copy(inject_weights, inject_weights + (size_t)M, currentGauss.weights.begin());
        }
        const std::vector<float> global0 = set.globalPoints, normal0 = set.globalNormals;  // the Jacobian leaves the last perturbation behind (q2)
        updateErrorTerms(set, errorVec);
        const int P = (int)paramVec.size(), rows = (int)errorVec.size(), a = rows - M;
        const double error0 = dotRows(errorVec, P);
        calcNumericJacobian(errorVec, set);
        std::vector<double> H, g;
        lm_step(errorVec.data(), Jacobian.data(), rows, P, (double)s.lambda_diag, s.step_length_optim, H, g, optimStep);
        const std::vector<double> stepRaw = optimStep;
        double mx = -std::numeric_limits<double>::infinity(), mn = std::numeric_limits<double>::infinity();
        for (double v : optimStep) mx = std::max(mx, v), mn = std::min(mn, v);
        const double maxElem = std::max(mx, -mn);
        if (maxElem > s.max_step)
            for (double& v : optimStep) v = (s.max_step / maxElem) * v;
        const int bestK = adaptiveStepSize(set, paramVec, optimStep, error0);
        FILE* f = std::fopen(path, "wb");
        if (!f) return DMSA_ERR_INVALID;
        const int64_t Mm = (int64_t)currentGauss.members.size(), n = set.numPoints();
        const int32_t hdr[6] = {model, P, a, M, currentGauss.numLevel1, table_rows};
        std::fwrite("DMSAST03", 1, 8, f), std::fwrite(hdr, 4, 6, f), std::fwrite(&Mm, 8, 1, f), std::fwrite(&n, 8, 1, f);
        std::fwrite(table, 4, (size_t)table_rows * 12, f);
        std::fwrite(global0.data(), 4, (size_t)n * 4, f);
        if (model == 2) std::fwrite(normal0.data(), 4, (size_t)n * 4, f);
        std::fwrite(currentGauss.segOffset.data(), 4, (size_t)M + 1, f), std::fwrite(currentGauss.members.data(), 4, (size_t)Mm, f);
        std::fwrite(currentGauss.info.data(), 4, (size_t)M * 9, f), std::fwrite(currentGauss.weights.data(), 4, (size_t)M, f);
        std::fwrite(currentGauss.fitMean.data(), 4, (size_t)M * 3, f), std::fwrite(currentGauss.fitCov.data(), 4, (size_t)M * 9, f);
        std::fwrite(currentGauss.rawWeights.data(), 4, (size_t)M, f);
        {   // 'DMSAST03': eigensolver.eigenvalues().real() and eigensolver.eigenvectors().real() (column-major) of every covariance (Gaussians.h:184-188)
            std::vector<float> eigVal((size_t)M * 3), eigVec((size_t)M * 9);
            for (int k = 0; k < M; ++k) {
                float c[3][3], v[3][3], lam[3];
                for (int cc = 0; cc < 3; ++cc)
                    for (int r = 0; r < 3; ++r) c[r][cc] = currentGauss.fitCov[(size_t)k * 9 + 3 * cc + r];
                limit_covariance_eig(c, v, lam);
                for (int cc = 0; cc < 3; ++cc) {
                    eigVal[(size_t)k * 3 + cc] = lam[cc];
                    for (int r = 0; r < 3; ++r) eigVec[(size_t)k * 9 + 3 * cc + r] = v[r][cc];
                }
            }
            std::fwrite(eigVal.data(), 4, eigVal.size(), f), std::fwrite(eigVec.data(), 4, eigVec.size(), f);
        }
        std::fwrite(errorVec.data(), 8, (size_t)rows, f), std::fwrite(Jacobian.data(), 8, (size_t)rows * P, f);
        std::fwrite(H.data(), 8, (size_t)P * P, f), std::fwrite(stepRaw.data(), 8, (size_t)P, f), std::fwrite(optimStep.data(), 8, (size_t)P, f);
        const int32_t tail[2] = {bestK, 0};
        std::fwrite(&error0, 8, 1, f), std::fwrite(tail, 4, 2, f), std::fwrite(paramVec.data(), 8, (size_t)P, f);
        std::fclose(f);
        return DMSA_OK;
    }
    // :54-150
    int optimizeSet(PointSet& set, const dmsa_settings& s, dmsa_report* rep, orc_iter_trace* trace, int trace_cap, bool fixed_iters) {
        std::vector<double> paramVec, errorVec, optimStep;
        int stop = DMSA_STOP_NUM_ITER, iters = 0;
        double error0 = 0.0, stepNorm = 0.0;
        int bestK = 0;
        if (s.use_centralization) set.centralize();
        for (int iter = 0; iter < s.num_iter; ++iter) {
            ++iters;
            set.getPoseParameters(paramVec);
            set.updateGlobalPoints();
            currentGauss.reset();
            const float* nrm = set.hasNormals ? set.globalNormals.data() : nullptr;
            if (s.grid_size_1_factor > std::numeric_limits<float>::min()) {
                const int rc = create_gaussian_sets(currentGauss, set.globalPoints.data(), nrm, set.ids.data(), set.numPoints(),
                                                    s.grid_size_1_factor * set.minGridSize, s.min_num_points_per_set, s.gauss_split != 0);
                if (rc != DMSA_OK) return rc;
            }
            currentGauss.numLevel1 = currentGauss.numPointSets;
            if (s.grid_size_2_factor > std::numeric_limits<float>::min()) {
                const int rc = create_gaussian_sets(currentGauss, set.globalPoints.data(), nrm, set.ids.data(), set.numPoints(),
                                                    s.grid_size_2_factor * set.minGridSize, s.min_num_points_per_set, s.gauss_split != 0);
                if (rc != DMSA_OK) return rc;
            }
            if (trace && iter < trace_cap) {
                trace[iter] = orc_iter_trace{};
                trace[iter].M = currentGauss.numPointSets, trace[iter].M1 = currentGauss.numLevel1;
                trace[iter].Mm = (int64_t)currentGauss.members.size();
            }
            if (currentGauss.numPointSets < s.min_num_gaussians) {
                stop = DMSA_STOP_FEW_GAUSSIANS;
                break;
            }
            currentGauss.updateRebalancingWeights();
            updateErrorTerms(set, errorVec);
            error0 = dotRows(errorVec, (int)paramVec.size());
            calcNumericJacobian(errorVec, set);
            const int P = (int)paramVec.size(), rows = (int)errorVec.size();
            std::vector<double> H, g;
            lm_step(errorVec.data(), Jacobian.data(), rows, P, (double)s.lambda_diag, s.step_length_optim, H, g, optimStep);
            bool anyNan = false;
            for (double v : optimStep) anyNan = anyNan || std::isnan(v);
            if (anyNan) {
                set.setPoseParameters(paramVec);
                stop = DMSA_STOP_NAN;
                break;
            }
            double maxElem = 0.0;
            {
                double mx = -std::numeric_limits<double>::infinity(), mn = std::numeric_limits<double>::infinity();
                for (double v : optimStep) mx = std::max(mx, v), mn = std::min(mn, v);
                maxElem = std::max(mx, -mn);
            }
            if (maxElem > s.max_step)
                for (double& v : optimStep) v = (s.max_step / maxElem) * v;
            bestK = adaptiveStepSize(set, paramVec, optimStep, error0);
            stepNorm = std::sqrt(dot(optimStep));
            if (trace && iter < trace_cap) trace[iter].error0 = error0, trace[iter].step_norm = stepNorm, trace[iter].best_k = bestK;
            if (bestK == 0 && !fixed_iters) {
                stop = DMSA_STOP_NO_IMPROVEMENT;
                break;
            }
            set.setPoseParameters(paramVec);
            if (stepNorm < s.epsilon && !fixed_iters) {
                stop = DMSA_STOP_EPSILON;
                break;
            }
        }
        if (s.use_centralization) set.decentralize();
        set.updateGlobalPoints();
        if (rep) {
            rep->iterations = iters, rep->stop_reason = stop;
            rep->num_gaussians = currentGauss.numPointSets, rep->num_gaussians_l1 = currentGauss.numLevel1;
            rep->num_memberships = (int64_t)currentGauss.members.size();
            rep->error0 = error0, rep->last_step_norm = stepNorm, rep->last_line_search_k = bestK;
            rep->evaluations = evaluations;
        }
        return DMSA_OK;
    }
};

}  // namespace

// ------------------------------------------------------------------------------------------------
// DmsaSlam::addStaticPoints, isVisible, getOverlap (DmsaSlam.h:264-414) and
// randomGridDownsampling (helpers.h:67-182).  Third-party pieces restated from their published behaviour:
//   * pcl::KdTreeFLANN<..>::nearestKSearch(q, 1, ..) with flann::L2_Simple<float>: the exact nearest neighbour under
//     dist(a, b) = ((0 + d0*d0) + d1*d1) + d2*d2 in float.  The reference only tests `dist(nearest) <= radius^2`, which is the
//     predicate "some point lies within the radius" -- independent of how the tree is walked.
//   * glibc srand()/rand(): the TYPE_3 additive feedback generator of random_r.c (degree 31, separation 3, 310 warm-up
//     draws), checked against the C library of this machine in tests/test_oracle_static.py.
// ------------------------------------------------------------------------------------------------
// fixed-size 3-vector inner product, Eigen's unrolled redux: x0 + (x1 + x2) (the order used for the quadratic form, see above)
static inline float dot3f(const float* a, const float* b) { return a[0] * b[0] + (a[1] * b[1] + a[2] * b[2]); }
static inline float l2_simple(const float* a, const float* b) {
    float result = 0.0f;
    for (int i = 0; i < 3; ++i) {
        const float diff = a[i] - b[i];
        result += diff * diff;
    }
    return result;
}

// "is there a cloud point within `radius` of q": sorted-cell grid (cells of 1.001 * radius, so every point within the radius
// sits in the 27 cells around the query's cell) + the exact float distance.  `brute` = plain loop over the cloud (the
// definition; used by the tests to check the grid).
struct RadiusGrid {
    const float* pts = nullptr;
    int64_t n = 0;
    double lo[3] = {0, 0, 0}, inv = 1.0;
    std::vector<std::pair<uint64_t, int32_t>> cells;  // (cell code, point index), sorted
    float r2 = 0.0f;

    static uint64_t code(int64_t ix, int64_t iy, int64_t iz) { return (uint64_t)ix | ((uint64_t)iy << 21) | ((uint64_t)iz << 42); }
    bool cell_of(const float* p, int64_t c[3]) const {
        for (int a = 0; a < 3; ++a) {
            if (!std::isfinite(p[a])) return false;
            c[a] = (int64_t)std::floor(((double)p[a] - lo[a]) * inv);
        }
        return true;
    }
    int build(const float* xyz4, int64_t count, float radius) {
        pts = xyz4, n = count, r2 = radius * radius;
        inv = 1.0 / (1.001 * (double)radius);
        bool any = false;
        double hi[3] = {0, 0, 0};
        for (int64_t i = 0; i < n; ++i) {
            const float* p = pts + 4 * i;
            if (!(std::isfinite(p[0]) && std::isfinite(p[1]) && std::isfinite(p[2]))) continue;
            for (int a = 0; a < 3; ++a) {
                if (!any || p[a] < lo[a]) lo[a] = p[a];
                if (!any || p[a] > hi[a]) hi[a] = p[a];
            }
            any = true;
        }
        cells.clear();
        if (!any) return DMSA_OK;
        for (int a = 0; a < 3; ++a)
            if ((hi[a] - lo[a]) * inv >= 2097150.0) return DMSA_ERR_DEPTH;
        cells.reserve((size_t)n);
        for (int64_t i = 0; i < n; ++i) {
            int64_t c[3];
            if (cell_of(pts + 4 * i, c)) cells.emplace_back(code(c[0], c[1], c[2]), (int32_t)i);
        }
        std::sort(cells.begin(), cells.end());
        return DMSA_OK;
    }
    bool within(const float* q) const {
        int64_t c[3];
        if (cells.empty() || !cell_of(q, c)) return false;
        for (int64_t dz = -1; dz <= 1; ++dz)
            for (int64_t dy = -1; dy <= 1; ++dy)
                for (int64_t dx = -1; dx <= 1; ++dx) {
                    const int64_t x = c[0] + dx, y = c[1] + dy, z = c[2] + dz;
                    if (x < 0 || y < 0 || z < 0 || x > 2097151 || y > 2097151 || z > 2097151) continue;
                    const uint64_t key = code(x, y, z);
                    auto it = std::lower_bound(cells.begin(), cells.end(), std::make_pair(key, (int32_t)INT32_MIN));
                    for (; it != cells.end() && it->first == key; ++it)
                        if (l2_simple(q, pts + 4 * (int64_t)it->second) <= r2) return true;
                }
        return false;
    }
    bool within_brute(const float* q) const {
        for (int64_t i = 0; i < n; ++i)
            if (l2_simple(q, pts + 4 * i) <= r2) return true;  // NaN distances compare false
        return false;
    }
};

// DmsaSlam.h:360-375
static inline bool is_visible(const float* pos, const float* point, const float* normal) {
    const float d = dot3f(point, normal);
    const float res = dot3f(pos, normal) - d;
    return (double)res >= -0.00001;
}

// glibc random_r.c, TYPE_3
struct GlibcRand {
    int32_t r[31];
    int f = 3, b = 0;
    explicit GlibcRand(uint32_t seed) {
        if (seed == 0) seed = 1;
        r[0] = (int32_t)seed;
        for (int i = 1; i < 31; ++i) {
            const long hi = r[i - 1] / 127773, lo = r[i - 1] % 127773;
            long word = 16807 * lo - 2836 * hi;
            if (word < 0) word += 2147483647;
            r[i] = (int32_t)word;
        }
        for (int i = 0; i < 310; ++i) (void)next();
    }
    int32_t next() {
        const uint32_t v = (uint32_t)r[f] + (uint32_t)r[b];
        r[f] = (int32_t)v;
        f = (f + 1) % 31, b = (b + 1) % 31;
        return (int32_t)(v >> 1);
    }
};

// ====================================================================================================
// C API
// ====================================================================================================
struct orc_gaussians {
    Gaussians g;
};

extern "C" {

void orc_set_threads(int n) { g_threads = n < 1 ? 1 : n; }
void orc_set_eigen_l1_bytes(int bytes) { g_eigen_l1_bytes = bytes >= 1024 ? bytes : 32 * 1024; }
int orc_get_eigen_l1_bytes(void) { return g_eigen_l1_bytes; }
int64_t orc_eigen_gemm_kc(int64_t depth) { return (int64_t)Gaussians::gemm_kc((size_t)depth); }
float orc_eigen_gemm_dot_f32(const float* a, const float* b, int64_t n) {
    return Gaussians::gemm_dot_f32((size_t)n, [&](size_t k) { return a[k]; }, [&](size_t k) { return b[k]; });
}
int orc_get_threads(void) { return g_threads; }

// EigenSolver<Matrix3f> (oracle/eigensolver3f.h) on `count` matrices (column-major 3 x 3): eigenvalues in T's diagonal order, real parts of the
// normalised eigenvectors, Francis QR iterations, info (0 Success / 1 NumericalIssue / 2 NoConvergence), complex pairs.  Outputs may be NULL.
void orc_eigensolver3f(const float* A9, int64_t count, float* evals_re, float* evals_im, float* V9, int32_t* iterations, int32_t* info, int32_t* pairs) {
    for (int64_t g = 0; g < count; ++g) {
        eigen34::Matrix3f A;
        for (int r = 0; r < 3; ++r)
            for (int c = 0; c < 3; ++c) A(r, c) = A9[9 * g + 3 * c + r];
        eigen34::EigenSolver3f es;
        eigen34::eigensolver_compute(A, es);
        for (int k = 0; k < 3; ++k) {
            if (evals_re) evals_re[3 * g + k] = es.eivalues_re[k];
            if (evals_im) evals_im[3 * g + k] = es.eivalues_im[k];
        }
        if (V9)
            for (int r = 0; r < 3; ++r)
                for (int c = 0; c < 3; ++c) V9[9 * g + 3 * c + r] = es.V_re(r, c);
        if (iterations) iterations[g] = es.iterations;
        if (info) info[g] = es.info;
        if (pairs) pairs[g] = es.complex_pairs;
    }
}
// Gaussians::limitCovariance (Gaussians.h:181-201) on `count` covariances (column-major), in place semantics: out9 = V max(D, 1e-4) V^-1
void orc_limit_covariance(const float* cov9, int64_t count, float* out9) {
    for (int64_t g = 0; g < count; ++g) {
        float c[3][3];
        for (int r = 0; r < 3; ++r)
            for (int k = 0; k < 3; ++k) c[r][k] = cov9[9 * g + 3 * k + r];
        limit_covariance(c);
        for (int r = 0; r < 3; ++r)
            for (int k = 0; k < 3; ++k) out9[9 * g + 3 * k + r] = c[r][k];
    }
}
// covariance -> limitCovariance -> inverse = the information matrix (Gaussians.h:150-154), on `count` column-major covariances
void orc_info_from_covariance(const float* cov9, int64_t count, float* info9) {
    for (int64_t g = 0; g < count; ++g) {
        float c[3][3], inv[3][3];
        for (int r = 0; r < 3; ++r)
            for (int k = 0; k < 3; ++k) c[r][k] = cov9[9 * g + 3 * k + r];
        limit_covariance(c);
        inverse3f(c, inv);
        for (int r = 0; r < 3; ++r)
            for (int k = 0; k < 3; ++k) info9[9 * g + 3 * k + r] = inv[r][k];
    }
}
// what limitCovariance decomposes with (the EigenSolver restatement, or the hypothesis the library was built with): eigenvalues, eigenvectors (column-major)
void orc_limitcov_eigenpairs(const float* cov9, int64_t count, float* evals3, float* V9) {
    for (int64_t g = 0; g < count; ++g) {
        float c[3][3], v[3][3], lam[3];
        for (int r = 0; r < 3; ++r)
            for (int k = 0; k < 3; ++k) c[r][k] = cov9[9 * g + 3 * k + r];
        limit_covariance_eig(c, v, lam);
        for (int k = 0; k < 3; ++k) {
            evals3[3 * g + k] = lam[k];
            for (int r = 0; r < 3; ++r) V9[9 * g + 3 * k + r] = v[r][k];
        }
    }
}
// telemetry of limitCovariance since the library was loaded (or since reset != 0): calls, QR iterations (sum, max), complex pairs, not converged
void orc_limitcov_stats(int64_t* out5, int reset) {
    if (out5) {
        out5[0] = g_limitcov_stats.calls, out5[1] = g_limitcov_stats.qr_iterations, out5[2] = g_limitcov_stats.max_iterations;
        out5[3] = g_limitcov_stats.complex_pairs, out5[4] = g_limitcov_stats.not_converged;
    }
    if (reset) g_limitcov_stats = LimitCovStats{};
}

void orc_axang2rotm(const double* w, double* R9) {
    const M3 R = axang2rotm(w);
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c) R9[3 * c + r] = R.m[r][c];
}
void orc_rotm2axang(const double* R9, double* w) {
    M3 R;
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c) R.m[r][c] = R9[3 * c + r];
    rotm2axang(R, w);
}
void orc_slerp(const double* a, const double* b, double t, double* out) { slerp(a, b, t, out); }
void orc_relative2global(int n, const double* ro, const double* rt, double* go, double* gt) {
    ConsecutivePoses cp;
    cp.resize(n);
    std::copy(ro, ro + 3 * n, cp.rel.O.begin()), std::copy(rt, rt + 3 * n, cp.rel.T.begin());
    cp.relative2global();
    std::copy(cp.glob.O.begin(), cp.glob.O.end(), go), std::copy(cp.glob.T.begin(), cp.glob.T.end(), gt);
}
void orc_global2relative(int n, const double* go, const double* gt, double* ro, double* rt) {
    ConsecutivePoses cp;
    cp.resize(n);
    std::copy(go, go + 3 * n, cp.glob.O.begin()), std::copy(gt, gt + 3 * n, cp.glob.T.begin());
    cp.global2relative();
    std::copy(cp.rel.O.begin(), cp.rel.O.end(), ro), std::copy(cp.rel.T.begin(), cp.rel.T.end(), rt);
}
int orc_barycentric_rational(const double* x, const double* y, int n, int d, const double* t, int nt, double* out) {
    try {
        BarycentricRational s(x, y, n, d);
        for (int i = 0; i < nt; ++i) out[i] = s(t[i]);
    } catch (const std::logic_error&) {
        return DMSA_ERR_INVALID;
    }
    return DMSA_OK;
}

int orc_detmath_eval(int fn, const double* x, const double* y, long n, double* out) {
    for (long i = 0; i < n; ++i)
        out[i] = fn == 0 ? dmsa_det::det_sin(x[i]) : fn == 1 ? dmsa_det::det_cos(x[i]) : fn == 2 ? dmsa_det::det_acos(x[i]) : dmsa_det::det_atan2(y[i], x[i]);
    return 0;
}
int orc_window_pose_table(const dmsa_window_problem* p, float* table, double* dense_transl) {
    dmsa_window_problem q = *p;
    q.num_points = 0, q.num_static = 0, q.use_imu = 0;
    WindowModel m(q);
    m.updateTrajDenseTforms();
    std::copy(m.denseTforms.begin(), m.denseTforms.end(), table);
    if (dense_transl) std::copy(m.denseGlobalPoses.T.begin(), m.denseGlobalPoses.T.end(), dense_transl);
    return DMSA_OK;
}
int orc_keyframe_pose_table(const dmsa_keyframe_problem* p, float* table) {
    ConsecutivePoses cp;
    const int F = p->num_frames;
    cp.resize(F);
    std::copy(p->rel_orient, p->rel_orient + 3 * F, cp.rel.O.begin());
    std::copy(p->rel_transl, p->rel_transl + 3 * F, cp.rel.T.begin());
    cp.relative2global();
    for (int k = 0; k < F; ++k) {
        const M3 R = axang2rotm(&cp.glob.O[3 * k]);
        for (int r = 0; r < 3; ++r) {
            for (int c = 0; c < 3; ++c) table[12 * k + 4 * r + c] = (float)R.m[r][c];
            table[12 * k + 4 * r + 3] = (float)cp.glob.T[3 * k + r];
        }
    }
    return DMSA_OK;
}
void orc_transform_points(const float* table, const float* xyz4, const int32_t* row, int64_t n, float* out4) {
    for (int64_t i = 0; i < n; ++i) {
        tform_point(table + 12 * (size_t)row[i], xyz4 + 4 * i, out4 + 4 * i);
        out4[4 * i + 3] = 1.0f;
    }
}

int orc_voxelize(const float* xyz4, int64_t n, double resolution, dmsa_voxel_level_info* info, uint64_t* leaf_code, uint32_t* key_xyz,
                 int32_t* sorted_point_idx) {
    VoxelResult v;
    const int rc = voxelize(xyz4, n, resolution, v);
    if (rc != DMSA_OK) return rc;
    if (info) *info = v.info;
    if (leaf_code) std::copy(v.code.begin(), v.code.end(), leaf_code);
    if (key_xyz) std::copy(v.key.begin(), v.key.end(), key_xyz);
    if (sorted_point_idx) std::copy(v.order.begin(), v.order.end(), sorted_point_idx);
    return DMSA_OK;
}

orc_gaussians* orc_build_gaussians(const float* xyz4, const float* normal4, const int32_t* ids, int64_t n, float min_grid_size,
                                   const dmsa_settings* s) {
    auto* h = new orc_gaussians();
    h->g.reset();
    // DmsaOptimizer.h:78-96
    if (s->grid_size_1_factor > std::numeric_limits<float>::min())
        create_gaussian_sets(h->g, xyz4, normal4, ids, n, s->grid_size_1_factor * min_grid_size, s->min_num_points_per_set, s->gauss_split != 0);
    h->g.numLevel1 = h->g.numPointSets;
    if (s->grid_size_2_factor > std::numeric_limits<float>::min())
        create_gaussian_sets(h->g, xyz4, normal4, ids, n, s->grid_size_2_factor * min_grid_size, s->min_num_points_per_set, s->gauss_split != 0);
    if (h->g.numPointSets > 0) h->g.updateRebalancingWeights();
    return h;
}
void orc_gaussians_free(orc_gaussians* g) { delete g; }
int32_t orc_gaussians_count(const orc_gaussians* g) { return g->g.numPointSets; }
int32_t orc_gaussians_count_level1(const orc_gaussians* g) { return g->g.numLevel1; }
int64_t orc_gaussians_memberships(const orc_gaussians* g) { return (int64_t)g->g.members.size(); }
void orc_gaussians_get(const orc_gaussians* g, int32_t* seg_offset, int32_t* member_idx, float* info_mats, float* weights) {
    if (seg_offset) std::copy(g->g.segOffset.begin(), g->g.segOffset.end(), seg_offset);
    if (member_idx) std::copy(g->g.members.begin(), g->g.members.end(), member_idx);
    if (info_mats) std::copy(g->g.info.begin(), g->g.info.end(), info_mats);
    if (weights) std::copy(g->g.weights.begin(), g->g.weights.end(), weights);
}
void orc_gaussians_get_fit(const orc_gaussians* g, float* mean3, float* cov9, float* raw_weights) {
    if (mean3) std::copy(g->g.fitMean.begin(), g->g.fitMean.end(), mean3);
    if (cov9) std::copy(g->g.fitCov.begin(), g->g.fitCov.end(), cov9);
    if (raw_weights) std::copy(g->g.rawWeights.begin(), g->g.rawWeights.end(), raw_weights);
}
void orc_gaussians_set_info(orc_gaussians* g, const float* info_mats, const float* weights) {
    if (info_mats) std::copy(info_mats, info_mats + 9 * (size_t)g->g.numPointSets, g->g.info.begin());
    if (weights) std::copy(weights, weights + (size_t)g->g.numPointSets, g->g.weights.begin());
}
void orc_eval_residuals(const orc_gaussians* g, const float* xyz4_global, double* e_out) { eval_residuals(g->g, xyz4_global, e_out); }
// the mean of a contiguous float vector as the Gaussian fit states it (Gaussians::eigen_mean_f32): test hook
float orc_eigen_mean_f32(const float* x, int64_t n, int64_t offset_floats) {
    return Gaussians::eigen_mean_f32((size_t)n, (size_t)offset_floats, [&](size_t j) { return x[j]; });
}

int orc_optimize_window(dmsa_window_problem* p, const dmsa_settings* s, dmsa_report* rep, float* global_out, orc_iter_trace* trace,
                        int32_t trace_capacity, int32_t fixed_iters) {
    try {
        WindowModel m(*p);
        Optimizer opt;
        const int rc = opt.optimizeSet(m, *s, rep, trace, trace_capacity, fixed_iters != 0);
        if (rc != DMSA_OK) return rc;
        const int C = p->num_control_poses;
        std::copy(m.controlPoses.rel.O.begin(), m.controlPoses.rel.O.begin() + 3 * C, p->rel_orient);
        std::copy(m.controlPoses.rel.T.begin(), m.controlPoses.rel.T.begin() + 3 * C, p->rel_transl);
        if (global_out) std::copy(m.globalPoints.begin(), m.globalPoints.end(), global_out);
    } catch (const std::exception&) {
        return DMSA_ERR_INVALID;
    }
    return DMSA_OK;
}
int orc_optimize_keyframes(dmsa_keyframe_problem* p, const dmsa_settings* s, dmsa_report* rep, float* global_out, orc_iter_trace* trace,
                           int32_t trace_capacity, int32_t fixed_iters) {
    try {
        KeyframeModel m(*p);
        Optimizer opt;
        const int rc = opt.optimizeSet(m, *s, rep, trace, trace_capacity, fixed_iters != 0);
        if (rc != DMSA_OK) return rc;
        const int F = p->num_frames;
        std::copy(m.keyframePoses.rel.O.begin(), m.keyframePoses.rel.O.begin() + 3 * F, p->rel_orient);
        std::copy(m.keyframePoses.rel.T.begin(), m.keyframePoses.rel.T.begin() + 3 * F, p->rel_transl);
        if (global_out) std::copy(m.globalPoints.begin(), m.globalPoints.end(), global_out);
    } catch (const std::exception&) {
        return DMSA_ERR_INVALID;
    }
    return DMSA_OK;
}

int orc_window_additional_errors(const dmsa_window_problem* p, double* rows_out) {
    dmsa_window_problem q = *p;
    q.num_points = 0, q.num_static = 0;
    WindowModel m(q);
    m.updateTrajDenseTforms();
    const int n = m.updateAdditionalErrors();
    if (n > 0) std::copy(m.imuFactorError.begin(), m.imuFactorError.begin() + n, rows_out);
    return n;
}
int orc_keyframe_additional_errors(const dmsa_keyframe_problem* p, double* rows_out) {
    dmsa_keyframe_problem q = *p;
    std::vector<int64_t> off((size_t)p->num_frames + 1, 0);
    q.frame_offset = off.data();
    KeyframeModel m(q);
    const int n = m.updateAdditionalErrors();
    if (n > 0) {
        const std::vector<double>& a = m.getAdditionalErrorTerms();
        std::copy(a.begin(), a.begin() + n, rows_out);
    }
    return n;
}

int orc_stage_dump_window(dmsa_window_problem* p, const dmsa_settings* s, const float* inject_info, const float* inject_weights, int32_t inject_M, const char* path) {
    try {
        WindowModel m(*p);
        WindowModel t(*p);  // the table of the start poses as the optimiser sees them: after centralize()
        if (s->use_centralization) t.centralize();
        t.updateGlobalPoints();
        Optimizer opt;
        return opt.stageDump(m, *s, 1, t.denseTforms.data(), t.n_total, inject_info, inject_weights, inject_M, path);
    } catch (...) {
        return DMSA_ERR_INVALID;
    }
}
int orc_stage_dump_keyframes(dmsa_keyframe_problem* p, const dmsa_settings* s, const float* inject_info, const float* inject_weights, int32_t inject_M, const char* path) {
    try {
        KeyframeModel m(*p);
        KeyframeModel t(*p);
        t.updateGlobalPoints();
        Optimizer opt;
        return opt.stageDump(m, *s, 2, t.tforms.data(), t.F, inject_info, inject_weights, inject_M, path);
    } catch (...) {
        return DMSA_ERR_INVALID;
    }
}
// H = J^T J + lambda I and the step from a GIVEN Jacobian (col-major rows x P): isolates the normal-equation / solve statements
int orc_lm_step_from_jacobian(const double* e0, const double* J, int32_t rows, int32_t P, double lambda, double alpha, double* H_out, double* g_out, double* step_out) {
    std::vector<double> H, g, step;
    lm_step(e0, J, rows, P, lambda, alpha, H, g, step);
    if (H_out) std::copy(H.begin(), H.end(), H_out);
    if (g_out) std::copy(g.begin(), g.end(), g_out);
    if (step_out) std::copy(step.begin(), step.end(), step_out);
    return DMSA_OK;
}

int orc_lm_step(const double* e0, const double* e_batch, int32_t rows, int32_t P, double h, double lambda, double alpha, double* H_out,
                double* g_out, double* step_out) {
    std::vector<double> J((size_t)rows * P);
    const double one_div_incr = 1.0 / h;
    for (int k = 0; k < P; ++k)
        for (int r = 0; r < rows; ++r) J[(size_t)k * rows + r] = one_div_incr * (e_batch[(size_t)k * rows + r] - e0[r]);
    std::vector<double> H, g, step;
    lm_step(e0, J.data(), rows, P, lambda, alpha, H, g, step);
    if (H_out) std::copy(H.begin(), H.end(), H_out);
    if (g_out) std::copy(g.begin(), g.end(), g_out);
    if (step_out) std::copy(step.begin(), step.end(), step_out);
    return DMSA_OK;
}

// The solve alone on a GIVEN damped system (col-major P x P, any matrix): what lm_step does behind its normal equations
int orc_lm_solve(const double* H_damped, const double* g, int32_t P, double alpha, double* step_out) {
    if (!H_damped || !g || !step_out || P < 1) return DMSA_ERR_INVALID;
    std::vector<double> H(H_damped, H_damped + (size_t)P * P), step;
    lm_solve(H, g, P, alpha, step);
    std::copy(step.begin(), step.end(), step_out);
    return DMSA_OK;
}
// blocked_dot for a batch of column pairs: Hp(i, j) = A_i^T A_j for the n1 columns of A (column-major rows x n1), every element its own
// chain, and out[b] = E_b^T E_b for the B rows of E (B x rows).  P selects the block size and the fused rule as everywhere.
int orc_blocked_gram(const double* A, int32_t n1, int32_t rows, int32_t P, double* Hp_out) {
    if (!A || !Hp_out || n1 < 1 || rows < 1 || P < 1) return DMSA_ERR_INVALID;
#pragma omp parallel for schedule(static)
    for (int32_t j = 0; j < n1; ++j)
        for (int32_t i = 0; i < n1; ++i) Hp_out[(size_t)j * n1 + i] = blocked_dot(rows, P, A + (size_t)i * rows, A + (size_t)j * rows);
    return DMSA_OK;
}
int orc_blocked_squares(const double* E, int32_t B, int32_t rows, int32_t P, double* out) {
    if (!E || !out || B < 1 || rows < 1 || P < 1) return DMSA_ERR_INVALID;
    for (int32_t b = 0; b < B; ++b) out[b] = blocked_dot(rows, P, E + (size_t)b * rows, E + (size_t)b * rows);
    return DMSA_OK;
}

// Not a statement of the reference: the check's exact products.  Four interleaved accumulators only change the order of the long double
// sums, which the bound's gamma_n(2^-64) covers for any order.
void orc_gram_long_double(const double* A, const double* B, int64_t rows, int32_t p, int32_t q, long double* out, int32_t threads) {
#pragma omp parallel for schedule(dynamic, 1) num_threads(threads < 1 ? 1 : threads)
    for (int32_t i = 0; i < p; ++i) {
        const double* a = A + (size_t)i * rows;
        for (int32_t j = 0; j < q; ++j) {
            const double* b = B + (size_t)j * rows;
            long double s0 = 0.0L, s1 = 0.0L, s2 = 0.0L, s3 = 0.0L;
            int64_t r = 0;
            for (; r + 4 <= rows; r += 4) {
                s0 += (long double)a[r] * (long double)b[r];
                s1 += (long double)a[r + 1] * (long double)b[r + 1];
                s2 += (long double)a[r + 2] * (long double)b[r + 2];
                s3 += (long double)a[r + 3] * (long double)b[r + 3];
            }
            for (; r < rows; ++r) s0 += (long double)a[r] * (long double)b[r];
            out[(size_t)i * q + j] = (s0 + s1) + (s2 + s3);
        }
    }
}

// ---- SURVEY 8(f) f1/f2 ---------------------------------------------------------------------------------------------
int orc_radius_exists(const float* cloud, int64_t n_cloud, const float* query, int64_t n_query, float radius, uint8_t* flag_out, int brute) {
    RadiusGrid g;
    if (brute) {
        g.pts = cloud, g.n = n_cloud, g.r2 = radius * radius;
    } else {
        const int rc = g.build(cloud, n_cloud, radius);
        if (rc != DMSA_OK) return rc;
    }
    for (int64_t i = 0; i < n_query; ++i) flag_out[i] = (brute ? g.within_brute(query + 4 * i) : g.within(query + 4 * i)) ? 1 : 0;
    return DMSA_OK;
}

// DmsaSlam.h:264-344, the loop over the closest keyframes (the distance gate of :304 is applied by the caller)
int orc_select_static_points(const dmsa_static_select_problem* p, float* static_xyz_out, int32_t* static_id_out, int64_t capacity,
                             int32_t* overlap_per_keyframe, dmsa_static_select_result* res) {
    RadiusGrid kdtree;
    const float sqrdMaxDist = (float)std::pow((double)(1.0f * p->min_grid_size), 2);  // std::pow(float, int) -> double -> float
    const int rc = kdtree.build(p->window_xyz, p->num_window, p->min_grid_size);
    if (rc != DMSA_OK) return rc;
    kdtree.r2 = sqrdMaxDist;
    int keyframeId = 0, maxOverlapKey = 0, minRelatedKeyId = -1;
    int64_t count = 0;
    for (int kk = 0; kk < p->num_keyframes; ++kk) {
        const int k = p->keyframe_ids[kk];
        int currOverlap = 0;
        for (int64_t j = p->frame_offset[kk]; j < p->frame_offset[kk + 1]; ++j) {
            const float* point = p->key_xyz + 4 * j;
            if (kdtree.within(point) && is_visible(p->cur_pos, point, p->key_normal + 4 * j)) {
                if (count < capacity) {
                    if (static_xyz_out) static_xyz_out[4 * count] = point[0], static_xyz_out[4 * count + 1] = point[1], static_xyz_out[4 * count + 2] = point[2], static_xyz_out[4 * count + 3] = 1.0f;
                    if (static_id_out) static_id_out[count] = p->key_ring[j];
                }
                ++count;
                ++currOverlap;
                if (minRelatedKeyId < 0 || k < minRelatedKeyId) minRelatedKeyId = k;
            }
            if (currOverlap > maxOverlapKey) maxOverlapKey = currOverlap, keyframeId = k;
        }
        if (overlap_per_keyframe) overlap_per_keyframe[kk] = currOverlap;
    }
    if (res) res->num_static = count, res->keyframe_id = keyframeId, res->min_related_key_id = minRelatedKeyId, res->max_overlap = maxOverlapKey, res->pad = 0;
    return count <= capacity ? DMSA_OK : DMSA_ERR_INVALID;
}

// DmsaSlam.h:377-414
int orc_get_overlap(const float* pc1, int64_t n1, const float* pc2, int64_t n2, float maxDistOverlap, float* overlap_out, int64_t* num_corresp_out) {
    int64_t nCorresp = 0;
    float overlap = 0.0f;
    if (n1 > 0 && n2 > 0) {
        RadiusGrid kdtree;
        const int rc = kdtree.build(pc1, n1, maxDistOverlap);
        if (rc != DMSA_OK) return rc;
        kdtree.r2 = maxDistOverlap * maxDistOverlap;
        for (int64_t i = 0; i < n2; ++i)
            if (kdtree.within(pc2 + 4 * i)) ++nCorresp;
        overlap = static_cast<float>(nCorresp) / static_cast<float>(n2);
    }
    if (overlap_out) *overlap_out = overlap;
    if (num_corresp_out) *num_corresp_out = nCorresp;
    return DMSA_OK;
}

void orc_glibc_rand(uint32_t seed, int32_t count, int32_t* out) {
    GlibcRand g(seed);
    for (int32_t i = 0; i < count; ++i) out[i] = g.next();
}

// helpers.h:67-182 with srand(seed)
int orc_random_grid_downsampling(const float* xyz, int64_t n, float grid_size, uint32_t seed, int32_t* picked_index_out, int64_t capacity,
                                 int64_t* num_out) {
    VoxelResult v;
    const int rc = voxelize(xyz, n, (double)grid_size, v);  // OctreePointCloud(gridSize): float -> double resolution
    if (rc != DMSA_OK) return rc;
    GlibcRand gen(seed);
    int64_t filId = 0;
    const int64_t nv = (int64_t)v.order.size();
    for (int64_t b = 0; b < nv;) {  // leaves in depth-first order; indices of a leaf ascend
        int64_t e = b + 1;
        while (e < nv && v.code[(size_t)v.order[(size_t)e]] == v.code[(size_t)v.order[(size_t)b]]) ++e;
        const double r = (double)gen.next() / 2147483647.0;
        const int id = static_cast<int>(r * (double)((e - b) - 1));
        if (filId < capacity && picked_index_out) picked_index_out[filId] = v.order[(size_t)(b + id)];
        ++filId;
        b = e;
    }
    if (num_out) *num_out = filId;
    return filId <= capacity ? DMSA_OK : DMSA_ERR_INVALID;
}

// DmsaSlam::preProcess (DmsaSlam.h:569-634) on the xyz part of a scan: adaptive random grid filter (0.4 / 0.3 / 0.2 / 0.15 m until
// max_num_points_per_scan leaves are reached), range sort + threshold, strict range gates, lidar->IMU transform, w = 1.
// srand(time(0)) of every filter pass becomes srand(seed) (the passes of one scan fall into the same second).  src_index_out[i] =
// index into the raw scan of output point i (stamp / id / isStatic travel with it).  pcl::transformPointCloud(Matrix4f) of
// PCL >= 1.10 (pcl::detail::Transformer<float>, SSE2 build): x*c0 + (y*c1 + (z*c2 + c3)) per component, no FMA -- recalled, the
// PCL source is not in this container.  `tform` is the Eigen (column-major) storage of lidarToImuTform.
int orc_preprocess_scan(const float* raw_xyz, int64_t n, int32_t max_num_points_per_scan, float min_dist_ds, float min_dist, uint32_t seed,
                        const float* tform, float* xyz_out, int32_t* src_index_out, int64_t capacity, int64_t* num_out, float* grid_size_out) {
    if (num_out) *num_out = 0;
    if (n < 0 || max_num_points_per_scan < 0 || !tform) return DMSA_ERR_INVALID;
    const float grids[4] = {0.4f, 0.3f, 0.2f, 0.15f};
    std::vector<int32_t> pick((size_t)std::max<int64_t>(n, 1));
    int64_t m = 0;
    float grid = grids[0];
    for (int pass = 0; pass < 4; ++pass) {  // :572-592
        if (pass > 0 && !(m < (int64_t)max_num_points_per_scan)) break;
        grid = grids[pass];
        const int rc = orc_random_grid_downsampling(raw_xyz, n, grid, seed, pick.data(), n, &m);
        if (rc != DMSA_OK) return rc;
    }
    if (grid_size_out) *grid_size_out = grid;
    if (m == 0) return DMSA_OK;  // (the reference would index rangesSorted[-1] here)
    std::vector<float> ranges((size_t)m), sorted((size_t)m);
    for (int64_t k = 0; k < m; ++k) {  // :601 Vector3f::norm(): sqrt(x0^2 + (x1^2 + x2^2)), Eigen's unrolled 3-term redux
        const float* p = raw_xyz + 4 * (size_t)pick[(size_t)k];
        const float xx = p[0] * p[0], yy = p[1] * p[1], zz = p[2] * p[2];
        const float t = yy + zz;
        ranges[(size_t)k] = std::sqrt(xx + t);
        sorted[(size_t)k] = ranges[(size_t)k];
    }
    std::sort(sorted.begin(), sorted.end());
    const float thresRange = std::max(sorted[(size_t)std::min((int)max_num_points_per_scan, (int)(m - 1))], min_dist_ds);  // :609
    int64_t out = 0;
    for (int64_t i = 0; i < m; ++i) {
        if (!(ranges[(size_t)i] < thresRange && ranges[(size_t)i] > min_dist)) continue;  // :616
        if (out < capacity) {
            const float* p = raw_xyz + 4 * (size_t)pick[(size_t)i];
            if (xyz_out) {
                for (int c = 0; c < 3; ++c) {
                    const float a = p[0] * tform[0 + c], b = p[1] * tform[4 + c], d = p[2] * tform[8 + c];
                    const float t2 = d + tform[12 + c];
                    const float t1 = b + t2;
                    xyz_out[4 * (size_t)out + c] = a + t1;
                }
                xyz_out[4 * (size_t)out + 3] = 1.0f;  // :629-630
            }
            if (src_index_out) src_index_out[(size_t)out] = pick[(size_t)i];
        }
        ++out;
    }
    if (num_out) *num_out = out;
    return out <= capacity ? DMSA_OK : DMSA_ERR_INVALID;
}

}  // extern "C"

// ================================================================================================================================
// the producers of the hot path's inputs (DmsaSlam::prepareTrajectoryForOptimization, DmsaSlam.h:416-461)
// ================================================================================================================================
namespace {

static inline M3 skewm(const double* v) { return M3{{{0.0, -v[2], v[1]}, {v[2], 0.0, -v[0]}, {-v[1], v[0], 0.0}}}; }  // helpers.h:39-49
static inline M3 smul(double s, const M3& a) {
    M3 c;
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) c.m[i][j] = s * a.m[i][j];
    return c;
}
static inline M3 muls(const M3& a, double s) {
    M3 c;
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) c.m[i][j] = a.m[i][j] * s;
    return c;
}
static inline M3 addm(const M3& a, const M3& b) {
    M3 c;
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) c.m[i][j] = a.m[i][j] + b.m[i][j];
    return c;
}
static inline M3 subm(const M3& a, const M3& b) {
    M3 c;
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) c.m[i][j] = a.m[i][j] - b.m[i][j];
    return c;
}

// VectorXd::LinSpaced(n, 0, high): Eigen 3.4 linspaced_op_impl<double> (not flipped since |high| >= |low| = 0)
static void linSpaced(int n, double high, std::vector<double>& out) {
    out.resize((size_t)n);
    const double step = n == 1 ? 0.0 : (high - 0.0) / (double)(n - 1);
    for (int i = 0; i < n; ++i) out[(size_t)i] = (i == n - 1 && n > 1) ? high : 0.0 + (double)i * step;
}

// ImuBuffer.h:14-175
struct ImuBufferO {
    std::vector<double> AccMeas, AngVelMeas, Stamps;
    double bias_gyr[3] = {0, 0, 0};
    int oldestIndex = 0, maxNumMeas = 10000, numUpdates = 0;
    explicit ImuBufferO(int maxNumMeasIn) : maxNumMeas(maxNumMeasIn) {
        AccMeas.assign(3 * (size_t)maxNumMeas, 0.0), AngVelMeas.assign(3 * (size_t)maxNumMeas, 0.0), Stamps.assign((size_t)maxNumMeas, 0.0);
    }
    void addMeasurement(const double* AccVec, const double* AngVelVec, double stamp) {  // :46-66
        for (int c = 0; c < 3; ++c) AccMeas[3 * (size_t)oldestIndex + c] = AccVec[c], AngVelMeas[3 * (size_t)oldestIndex + c] = AngVelVec[c] - bias_gyr[c];
        Stamps[(size_t)oldestIndex] = stamp;
        ++oldestIndex;
        if (oldestIndex == maxNumMeas) oldestIndex = 0;
        ++numUpdates;
        if (numUpdates == 50) {
            const int n = std::min(numUpdates, maxNumMeas);
            for (int c = 0; c < 3; ++c) {
                double sum = 0.0;
                for (int k = 0; k < n; ++k) sum += AngVelMeas[3 * (size_t)k + c];
                bias_gyr[c] = sum / (double)n;
            }
        }
    }
    double getClosestMeasurement(double t, double* AccVec, double* AngVelVec) const {  // :68-125
        const double* S = Stamps.data();
        double measurementDiff = 0.0;
        long index;
        if (numUpdates <= maxNumMeas || oldestIndex == 0) {
            const double* pointerToVal = std::lower_bound(S, S + std::min(maxNumMeas - 1, numUpdates - 1), t);
            index = pointerToVal - S;
            measurementDiff = std::abs(t - *pointerToVal);
        } else {
            const double* pointerToValRight = std::lower_bound(S + oldestIndex, S + maxNumMeas - 1, t);
            const double* pointerToValLeft = std::lower_bound(S, S + oldestIndex - 1, t);
            if (std::abs(t - *pointerToValRight) < std::abs(t - *pointerToValLeft)) {
                index = pointerToValRight - S;
                measurementDiff = t - *pointerToValRight;
            } else {
                index = pointerToValLeft - S;
                measurementDiff = t - *pointerToValLeft;
            }
        }
        for (int c = 0; c < 3; ++c) AccVec[c] = AccMeas[3 * (size_t)index + c], AngVelVec[c] = AngVelMeas[3 * (size_t)index + c];
        return measurementDiff;
    }
};

// ImuPreintegration.h:23-139 (matrices row-major here; 9 x 9 order rot, vel, pos)
struct ImuPreintegrationO {
    double deltaPos[3], deltaVel[3];
    M3 deltaRot;
    double cov[9][9];
    ImuPreintegrationO() { reset(); }
    void reset() {
        for (int c = 0; c < 3; ++c) deltaPos[c] = deltaVel[c] = 0.0;
        deltaRot = eye3();
        for (auto& r : cov)
            for (double& v : r) v = 0.0;
    }
    static M3 getJacobianR(const double* rot) {  // :35-47
        const double rotNorm = norm3(rot);
        const M3 skewRot = skewm(rot);
        if (rotNorm < 0.00001) return eye3();
        return addm(subm(eye3(), smul((1.0 - std::cos(rotNorm)) / std::pow(rotNorm, 2), skewRot)),
                    mul(smul((rotNorm - std::sin(rotNorm)) / std::pow(rotNorm, 3), skewRot), skewRot));
    }
    void addMeasurement(const double* omega, const double* acc, double dt, const double* gyr_cov, const double* acc_cov) {  // :55-107
        const double dt2 = dt * dt;
        const double w[3] = {dt * omega[0], dt * omega[1], dt * omega[2]};
        const M3 rotIncr = axang2rotm(w);
        double A[9][9] = {}, B[9][6] = {}, Noise[6][6] = {};
        for (int i = 0; i < 9; ++i) A[i][i] = 1.0;
        auto blockA = [&](int r0, int c0, const M3& M) {
            for (int r = 0; r < 3; ++r)
                for (int c = 0; c < 3; ++c) A[r0 + r][c0 + c] = M.m[r][c];
        };
        auto blockB = [&](int r0, int c0, const M3& M) {
            for (int r = 0; r < 3; ++r)
                for (int c = 0; c < 3; ++c) B[r0 + r][c0 + c] = M.m[r][c];
        };
        blockA(0, 0, transpose(rotIncr));
        blockA(3, 0, muls(mul(smul(-1.0, deltaRot), skewm(acc)), dt));
        blockA(6, 0, muls(mul(smul(-0.5, deltaRot), skewm(acc)), dt2));
        blockA(6, 3, smul(dt, eye3()));
        double aa[3];
        rotm2axang(deltaRot, aa);
        blockB(0, 0, muls(getJacobianR(aa), dt));
        blockB(3, 3, muls(deltaRot, dt));
        blockB(6, 3, muls(smul(0.5, deltaRot), dt2));
        for (int r = 0; r < 3; ++r)
            for (int c = 0; c < 3; ++c) Noise[r][c] = gyr_cov[3 * c + r], Noise[3 + r][3 + c] = acc_cov[3 * c + r];
        double AC[9][9], BN[9][6], next[9][9];
        for (int r = 0; r < 9; ++r)
            for (int c = 0; c < 9; ++c) {
                double sum = 0.0;
                for (int k = 0; k < 9; ++k) sum += A[r][k] * cov[k][c];
                AC[r][c] = sum;
            }
        for (int r = 0; r < 9; ++r)
            for (int c = 0; c < 6; ++c) {
                double sum = 0.0;
                for (int k = 0; k < 6; ++k) sum += B[r][k] * Noise[k][c];
                BN[r][c] = sum;
            }
        for (int r = 0; r < 9; ++r)
            for (int c = 0; c < 9; ++c) {
                double s1 = 0.0, s2 = 0.0;
                for (int k = 0; k < 9; ++k) s1 += AC[r][k] * A[c][k];
                for (int k = 0; k < 6; ++k) s2 += BN[r][k] * B[c][k];
                next[r][c] = s1 + s2;
            }
        std::memcpy(cov, next, sizeof(next));
        double ra[3], hra[3];
        matvec(smul(0.5, deltaRot), acc, hra);
        matvec(deltaRot, acc, ra);
        for (int c = 0; c < 3; ++c) {
            deltaPos[c] = deltaPos[c] + (deltaVel[c] * dt + hra[c] * dt2);
            deltaVel[c] = deltaVel[c] + ra[c] * dt;
        }
        deltaRot = mul(deltaRot, rotIncr);
    }
};

// Eigen::AngleAxisd(Matrix3d): via Quaterniond(mat) and AngleAxis(q); returns angle() * axis()
static void angleAxisFromMatrix(const M3& mat, double* out) {
    double q[4];  // x y z w
    double t = mat.m[0][0] + mat.m[1][1] + mat.m[2][2];
    if (t > 0.0) {
        t = std::sqrt(t + 1.0);
        q[3] = 0.5 * t;
        t = 0.5 / t;
        q[0] = (mat.m[2][1] - mat.m[1][2]) * t;
        q[1] = (mat.m[0][2] - mat.m[2][0]) * t;
        q[2] = (mat.m[1][0] - mat.m[0][1]) * t;
    } else {
        int i = 0;
        if (mat.m[1][1] > mat.m[0][0]) i = 1;
        if (mat.m[2][2] > mat.m[i][i]) i = 2;
        const int j = (i + 1) % 3, k = (j + 1) % 3;
        t = std::sqrt(mat.m[i][i] - mat.m[j][j] - mat.m[k][k] + 1.0);
        q[i] = 0.5 * t;
        t = 0.5 / t;
        q[3] = (mat.m[k][j] - mat.m[j][k]) * t;
        q[j] = (mat.m[j][i] + mat.m[i][j]) * t;
        q[k] = (mat.m[k][i] + mat.m[i][k]) * t;
    }
    double n = std::sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2]);
    if (n != 0.0) {
        const double angle = 2.0 * std::atan2(n, std::fabs(q[3]));
        if (q[3] < 0.0) n = -n;
        for (int c = 0; c < 3; ++c) out[c] = angle * (q[c] / n);
    } else {
        out[0] = out[1] = out[2] = 0.0;
    }
}

// The setup half of ContinuousTrajectory (ContinuousTrajectory.h:228-568), on the caller's arrays
struct TrajSetupO {
    dmsa_traj_state* s;
    ConsecutivePoses controlPoses;
    explicit TrajSetupO(dmsa_traj_state* st) : s(st) {
        const int C = s->num_control_poses;
        controlPoses.resize(C);
        std::copy(s->rel_orient, s->rel_orient + 3 * C, controlPoses.rel.O.begin()), std::copy(s->rel_transl, s->rel_transl + 3 * C, controlPoses.rel.T.begin());
        std::copy(s->glob_orient, s->glob_orient + 3 * C, controlPoses.glob.O.begin()), std::copy(s->glob_transl, s->glob_transl + 3 * C, controlPoses.glob.T.begin());
    }
    void store() {
        std::copy(controlPoses.rel.O.begin(), controlPoses.rel.O.end(), s->rel_orient), std::copy(controlPoses.rel.T.begin(), controlPoses.rel.T.end(), s->rel_transl);
        std::copy(controlPoses.glob.O.begin(), controlPoses.glob.O.end(), s->glob_orient), std::copy(controlPoses.glob.T.begin(), controlPoses.glob.T.end(), s->glob_transl);
    }
    void initGravityDir() {  // :263-299
        const double* measuredGravity = s->acc_meas;  // accMeas.col(0)
        const double v1[3] = {s->gravity[0], s->gravity[1], s->gravity[2]};
        const double v2[3] = {-1.0 * measuredGravity[0], -1.0 * measuredGravity[1], -1.0 * measuredGravity[2]};
        double axis[3] = {v1[1] * v2[2] - v1[2] * v2[1], v1[2] * v2[0] - v1[0] * v2[2], v1[0] * v2[1] - v1[1] * v2[0]};
        const double z = axis[0] * axis[0] + axis[1] * axis[1] + axis[2] * axis[2];
        if (z > 0.0) {
            const double nn = std::sqrt(z);
            for (double& a : axis) a = a / nn;
        }
        const double angle = std::acos((v1[0] * v2[0] + v1[1] * v2[1] + v1[2] * v2[2]) / (norm3(v1) * norm3(v2)));
        const M3 K = skewm(axis);
        const M3 R_to_grav = addm(addm(eye3(), smul(std::sin(angle), K)), mul(smul(1 - std::cos(angle), K), K));
        angleAxisFromMatrix(transpose(R_to_grav), &controlPoses.rel.O[0]);
        controlPoses.relative2global();
    }
    static void getInterpRotation(const Poses& posesGlobal, const double* stamps, int n, double t, double* axangNew) {  // :570-591
        const long rightIndex = std::lower_bound(stamps, stamps + n - 1, t) - stamps;
        if (rightIndex > 0) {
            const double t_rel = (t - stamps[rightIndex - 1]) / (stamps[rightIndex] - stamps[rightIndex - 1]);
            slerp(&posesGlobal.O[3 * (size_t)(rightIndex - 1)], &posesGlobal.O[3 * (size_t)rightIndex], t_rel, axangNew);
        } else {
            for (int c = 0; c < 3; ++c) axangNew[c] = posesGlobal.O[(size_t)c];
        }
    }
    void getImuIntegratedParams(double t0, const double* axang0, const double* pos0, const double* v0, double tend, double* axang_end, double* pos_end,
                                double* v_end) const {  // :470-516
        const double* tt = s->traj_time;
        long index = std::lower_bound(tt, tt + s->n_total - 1, t0) - tt;
        // *(pointerToVal - 1) is read even at index 0 in the reference; t0 <= trajTime[0] there, so `next` always wins
        const double prev = index > 0 ? tt[index - 1] : -std::numeric_limits<double>::infinity();
        const double next = tt[index];
        if (std::abs(t0 - prev) < std::abs(t0 - next)) index = index - 1;
        M3 R_imu2w = axang2rotm(axang0);
        double pos_w[3] = {pos0[0], pos0[1], pos0[2]}, vel_w[3] = {v0[0], v0[1], v0[2]};
        const double dt_res = s->dt_res, dt_res2 = dt_res * dt_res;
        double currTime = t0;
        while (std::abs(currTime + dt_res - tend) < std::abs(currTime - tend) && index < s->n_total) {
            const double* acc = s->acc_meas + 3 * (size_t)index;
            double hra[3], ra[3];
            matvec(smul(0.5, R_imu2w), acc, hra);
            matvec(R_imu2w, acc, ra);
            for (int c = 0; c < 3; ++c) {
                pos_w[c] = ((pos_w[c] + vel_w[c] * dt_res) + (0.5 * s->gravity[c]) * dt_res2) + hra[c] * dt_res2;
                vel_w[c] = (vel_w[c] + s->gravity[c] * dt_res) + ra[c] * dt_res;
            }
            const double* av = s->ang_vel_meas + 3 * (size_t)index;
            const double w[3] = {dt_res * av[0], dt_res * av[1], dt_res * av[2]};
            R_imu2w = mul(R_imu2w, axang2rotm(w));
            index += 1;
            currTime += dt_res;
        }
        rotm2axang(R_imu2w, axang_end);
        for (int c = 0; c < 3; ++c) pos_end[c] = pos_w[c], v_end[c] = vel_w[c];
    }
    void updateInitialGuess(int32_t& isInitialized, TrajSetupO& oldTraj, bool useImu) {  // :366-468
        int lastKnownParamId = 0;
        if (!isInitialized) {
            if (useImu) initGravityDir();
            isInitialized = 1;
            return;
        }
        oldTraj.controlPoses.relative2global();
        const int C = s->num_control_poses, Co = oldTraj.s->num_control_poses;
        for (int k = 0; k < C; ++k)
            if (s->t0 + s->stamps[k] < oldTraj.s->t0 + oldTraj.s->horizon) lastKnownParamId = k;
        for (int k = 0; k <= lastKnownParamId; ++k)
            getInterpRotation(oldTraj.controlPoses.glob, oldTraj.s->stamps, Co, s->stamps[k] + s->t0 - oldTraj.s->t0, &controlPoses.glob.O[3 * (size_t)k]);
        double v0[3];
        for (int k = 0; k < 3; ++k) {
            std::vector<double> vec_translations((size_t)Co);
            for (int j = 0; j < Co; ++j) vec_translations[(size_t)j] = oldTraj.controlPoses.glob.T[3 * (size_t)j + k];
            BarycentricRational spline(oldTraj.s->stamps, vec_translations.data(), Co, 2);
            for (int j = 0; j <= lastKnownParamId; ++j) controlPoses.glob.T[3 * (size_t)j + k] = spline(s->stamps[j] + s->t0 - oldTraj.s->t0);
            v0[k] = spline.prime(s->stamps[lastKnownParamId] + s->t0 - oldTraj.s->t0);
        }
        controlPoses.global2relative();
        if (useImu) {
            double pos0[3], axang0[3];
            for (int c = 0; c < 3; ++c) pos0[c] = controlPoses.glob.T[3 * (size_t)lastKnownParamId + c], axang0[c] = controlPoses.glob.O[3 * (size_t)lastKnownParamId + c];
            for (int k = lastKnownParamId; k < C - 1; ++k) {
                double axang_end[3], pos_end[3], v_end[3];
                getImuIntegratedParams(s->stamps[k], axang0, pos0, v0, s->stamps[k + 1], axang_end, pos_end, v_end);
                for (int c = 0; c < 3; ++c) {
                    controlPoses.glob.O[3 * (size_t)(k + 1) + c] = axang_end[c], controlPoses.glob.T[3 * (size_t)(k + 1) + c] = pos_end[c];
                    axang0[c] = axang_end[c], pos0[c] = pos_end[c], v0[c] = v_end[c];
                }
            }
            controlPoses.global2relative();
        } else {
            for (int k = lastKnownParamId; k < C - 1; ++k)
                for (int c = 0; c < 3; ++c) {
                    controlPoses.rel.O[3 * (size_t)(k + 1) + c] = controlPoses.rel.O[3 * (size_t)lastKnownParamId + c];
                    controlPoses.rel.T[3 * (size_t)(k + 1) + c] = controlPoses.rel.T[3 * (size_t)lastKnownParamId + c];
                }
            controlPoses.relative2global();
        }
    }
};

}  // namespace

extern "C" {

void* orc_imu_buffer_create(int32_t max_num_meas) { return max_num_meas >= 2 ? new ImuBufferO(max_num_meas) : nullptr; }
void orc_imu_buffer_destroy(void* b) { delete static_cast<ImuBufferO*>(b); }
void orc_imu_buffer_add(void* b, const double* acc, const double* ang_vel, double stamp) { static_cast<ImuBufferO*>(b)->addMeasurement(acc, ang_vel, stamp); }
int orc_imu_buffer_closest(const void* b, double t, double* acc_out, double* ang_vel_out, double* timediff_out) {
    const ImuBufferO* B = static_cast<const ImuBufferO*>(b);
    if (B->numUpdates <= 0) return DMSA_ERR_INVALID;
    *timediff_out = B->getClosestMeasurement(t, acc_out, ang_vel_out);
    return DMSA_OK;
}
void orc_imu_buffer_state(const void* b, int32_t* num_updates, int32_t* oldest_index, double* bias_gyr) {
    const ImuBufferO* B = static_cast<const ImuBufferO*>(b);
    *num_updates = B->numUpdates, *oldest_index = B->oldestIndex;
    for (int c = 0; c < 3; ++c) bias_gyr[c] = B->bias_gyr[c];
}

// initTraj :301-346
int orc_traj_dims(double t_min, double t_max, double dt_res, double* horizon_out, int32_t* n_total_out) {
    const double horizon = t_max - t_min + dt_res;
    *horizon_out = horizon;
    *n_total_out = (int32_t)(std::round(horizon / dt_res) + 1);
    return DMSA_OK;
}
int orc_traj_grids(double horizon, double dt_res, int32_t n_total, int32_t C, double* traj_time_out, double* stamps_out, int32_t* param_indices_out) {
    std::vector<double> v;
    linSpaced(n_total, horizon, v);
    std::copy(v.begin(), v.end(), traj_time_out);
    linSpaced(C, horizon, v);
    std::copy(v.begin(), v.end(), stamps_out);
    for (int k = 0; k < C; ++k) param_indices_out[k] = (int32_t)std::round(stamps_out[k] / dt_res);
    return DMSA_OK;
}
// registerPcBuffer :240-260
int orc_traj_tform_indices(const double* point_stamps, int64_t n, double t0, const double* traj_time, int32_t n_total, int32_t* out) {
    for (int64_t k = 0; k < n; ++k) {
        const double* pointerToVal = std::lower_bound(traj_time, traj_time + n_total, point_stamps[k] - t0);
        out[k] = std::min((int)(pointerToVal - traj_time), (int)(n_total - 1));
    }
    return DMSA_OK;
}
// transferImuMeasurements :348-364
int orc_traj_transfer_imu(const void* b, double t0, const double* traj_time, int32_t n_total, double* acc_meas_out, double* ang_vel_meas_out, double* worst) {
    const ImuBufferO* B = static_cast<const ImuBufferO*>(b);
    if (B->numUpdates <= 0) return DMSA_ERR_INVALID;
    double w = 0.0;
    for (int k = 0; k < n_total; ++k) {
        const double currGlobalTime = t0 + traj_time[k];
        const double timediff = B->getClosestMeasurement(currGlobalTime, acc_meas_out + 3 * (size_t)k, ang_vel_meas_out + 3 * (size_t)k);
        w = std::max(w, std::abs(timediff));
    }
    if (worst) *worst = w;
    return DMSA_OK;
}
// updatePreintFactors :518-568
int orc_traj_preint_factors(int32_t n_total, int32_t C, const int32_t* paramIndices, double dt_res, const double* accMeas, const double* angVelMeas,
                            const double* gyr_cov, const double* acc_cov, double* preintImuRots, double* preintRelPositions, double* preintRelVelocity,
                            double* CovPVRot_inv, double* preintPosComplHor) {
    ImuPreintegrationO imuPreintegration;
    for (int i = 0; i < 9; ++i) preintImuRots[i] = (i % 4 == 0) ? 1.0 : 0.0;
    for (int c = 0; c < 3; ++c) preintRelPositions[c] = preintRelVelocity[c] = 0.0;
    std::fill(CovPVRot_inv, CovPVRot_inv + 81, 0.0);
    for (int k = 1; k < C; ++k) {
        const int fromId = paramIndices[k - 1], toId = paramIndices[k];
        imuPreintegration.reset();
        for (int t = fromId; t < toId; ++t) imuPreintegration.addMeasurement(angVelMeas + 3 * (size_t)t, accMeas + 3 * (size_t)t, dt_res, gyr_cov, acc_cov);
        for (int r = 0; r < 3; ++r)
            for (int c = 0; c < 3; ++c) preintImuRots[9 * (size_t)k + 3 * c + r] = imuPreintegration.deltaRot.m[r][c];
        for (int c = 0; c < 3; ++c) preintRelPositions[3 * (size_t)k + c] = imuPreintegration.deltaPos[c], preintRelVelocity[3 * (size_t)k + c] = imuPreintegration.deltaVel[c];
        std::vector<double> covMat(81), inv;
        for (int r = 0; r < 9; ++r)
            for (int c = 0; c < 9; ++c) covMat[(size_t)c * 9 + r] = imuPreintegration.cov[r][c];
        invert_dense(covMat, 9, inv);  // Matrix<double,9,9>::inverse(): partial-pivot LU
        std::copy(inv.begin(), inv.end(), CovPVRot_inv + 81 * (size_t)k);
    }
    imuPreintegration.reset();
    for (int t = 0; t < n_total; ++t) imuPreintegration.addMeasurement(angVelMeas + 3 * (size_t)t, accMeas + 3 * (size_t)t, dt_res, gyr_cov, acc_cov);
    for (int c = 0; c < 3; ++c) preintPosComplHor[c] = imuPreintegration.deltaPos[c];
    return DMSA_OK;
}
// getSubmapGravityEstimate :593-601
int orc_traj_submap_gravity_estimate(const dmsa_traj_state* s, const double* preintPosComplHor, double* gravity_imu) {
    const int C = s->num_control_poses;
    double dense0[3], dense1[3];
    for (int k = 0; k < 3; ++k) {
        std::vector<double> tr((size_t)C);
        for (int j = 0; j < C; ++j) tr[(size_t)j] = s->glob_transl[3 * (size_t)j + k];
        BarycentricRational spline(s->stamps, tr.data(), C, 2);
        dense0[k] = spline(s->traj_time[0]), dense1[k] = spline(s->traj_time[1]);
    }
    const double one_div_t_res = 1.0 / s->dt_res;
    double v_start_w[3], inner[3], rot[3];
    for (int c = 0; c < 3; ++c) v_start_w[c] = one_div_t_res * (dense1[c] - dense0[c]);
    const M3 R_imu2w_start = axang2rotm(s->glob_orient);
    for (int c = 0; c < 3; ++c) inner[c] = s->glob_transl[3 * (size_t)(C - 1) + c] - s->glob_transl[c] - v_start_w[c] * s->horizon;
    matvec(transpose(R_imu2w_start), inner, rot);
    for (int c = 0; c < 3; ++c) gravity_imu[c] = (rot[c] - preintPosComplHor[c]) / (0.5 * std::pow(s->horizon, 2));
    return DMSA_OK;
}
// updateInitialGuess :366-468
int orc_traj_update_initial_guess(int32_t* is_initialized, dmsa_traj_state* cur, dmsa_traj_state* old_traj, int32_t use_imu) {
    TrajSetupO c(cur);
    if (!*is_initialized) {
        TrajSetupO none(cur);
        c.updateInitialGuess(*is_initialized, none, use_imu != 0);
        c.store();
        return DMSA_OK;
    }
    TrajSetupO o(old_traj);
    try {
        c.updateInitialGuess(*is_initialized, o, use_imu != 0);
    } catch (const std::logic_error&) {
        return DMSA_ERR_INVALID;
    }
    c.store(), o.store();
    return DMSA_OK;
}

}  // extern "C"

// ================================================================================================================================
// wire formats (src/dmsa_slam_ros.cpp:374-486, OutputManagement.h:80-182)
// ================================================================================================================================
#include <iomanip>
#include <sstream>

// callbackPointCloud :399-486 restated as a table: which message field carries the stamp / the ring for each config.sensor, how it
// is encoded, and how the point stamp follows from it.  Every value is fetched with memcpy at k * point_step + fields[i].offset,
// like the node does.
namespace {
enum class StampKind { AbsF64, RelU32Nanos, RelF32, AbsF64Nanos, Heuristic };
enum class RingKind { U16, U8, I8, IndexMod1000 };
struct SensorLayout {
    int stamp_field;
    StampKind stamp;
    int ring_field;
    RingKind ring;
};
const SensorLayout kSensorLayouts[8] = {
    {4, StampKind::AbsF64, 5, RingKind::U16},              // hesai      :411-419
    {4, StampKind::RelU32Nanos, 6, RingKind::U8},          // ouster     :420-430
    {5, StampKind::AbsF64, 4, RingKind::U16},              // robosense  :431-439
    {5, StampKind::RelF32, 4, RingKind::U16},              // velodyne   :440-448
    {6, StampKind::AbsF64, -1, RingKind::IndexMod1000},    // livox s    :449-458
    {6, StampKind::AbsF64Nanos, -1, RingKind::IndexMod1000},  // livox ns :459-469
    {8, StampKind::RelF32, 11, RingKind::I8},              // sick       :470-478
    {-1, StampKind::Heuristic, -1, RingKind::IndexMod1000},   // unknown :479-486
};
template <typename T>
T fetch(const uint8_t* at) {
    T v;
    std::memcpy(&v, at, sizeof(T));
    return v;
}
}  // namespace

extern "C" int orc_decode_pointcloud2(const dmsa_pointcloud2* msg, int32_t sensor, float* xyz_out, double* stamp_out, int32_t* id_out) {
    if (sensor < 0 || sensor > 7) return DMSA_ERR_INVALID;
    const SensorLayout& L = kSensorLayouts[sensor];
    const uint32_t count = msg->height * msg->width;
    const uint32_t* off = msg->field_offsets;
    for (uint32_t k = 0; k < count; ++k) {
        const uint8_t* pt = msg->data + (uint32_t)(k * msg->point_step);
        float* o = xyz_out + 4 * (size_t)k;
        o[0] = fetch<float>(pt + off[0]), o[1] = fetch<float>(pt + off[1]), o[2] = fetch<float>(pt + off[2]);
        o[3] = 0.0f;  // PointStampId is value-initialised by PointCloud::resize
        const uint8_t* sp = L.stamp_field >= 0 ? pt + off[L.stamp_field] : nullptr;
        double st = 0.0;
        switch (L.stamp) {
            case StampKind::AbsF64: st = fetch<double>(sp); break;
            case StampKind::RelU32Nanos: st = msg->stamp_msg + 1e-9 * (double)fetch<uint32_t>(sp); break;
            case StampKind::RelF32: st = msg->stamp_msg + static_cast<double>(fetch<float>(sp)); break;
            case StampKind::AbsF64Nanos: st = 1e-9 * fetch<double>(sp); break;
            case StampKind::Heuristic: st = msg->stamp_msg + msg->delta_t_pcs * (double)k / (double)count; break;
        }
        const uint8_t* rp = L.ring_field >= 0 ? pt + off[L.ring_field] : nullptr;
        int ring = 0;
        switch (L.ring) {
            case RingKind::U16: ring = (int)fetch<uint16_t>(rp); break;
            case RingKind::U8: ring = (int)fetch<uint8_t>(rp); break;
            case RingKind::I8: ring = static_cast<int>(fetch<int8_t>(rp)); break;
            case RingKind::IndexMod1000: ring = (int)(k % 1000); break;
        }
        stamp_out[k] = st, id_out[k] = ring;
    }
    return DMSA_OK;
}

extern "C" {

// addPoseToFile (OutputManagement.h:80-96) through the same iostream manipulators
int orc_format_tum_pose(double stamp, const double* pos, const double* orient, char* out, int32_t cap) {
    std::ostringstream file;
    file << std::setprecision(6) << std::fixed << stamp << " ";
    file << std::setprecision(5) << std::fixed << pos[0] << " " << pos[1] << " " << pos[2] << " ";
    const M3 R = axang2rotm(orient);
    // Quaterniond q(R)
    double q[4];
    double t = R.m[0][0] + R.m[1][1] + R.m[2][2];
    if (t > 0.0) {
        t = std::sqrt(t + 1.0);
        q[3] = 0.5 * t;
        t = 0.5 / t;
        q[0] = (R.m[2][1] - R.m[1][2]) * t, q[1] = (R.m[0][2] - R.m[2][0]) * t, q[2] = (R.m[1][0] - R.m[0][1]) * t;
    } else {
        int i = 0;
        if (R.m[1][1] > R.m[0][0]) i = 1;
        if (R.m[2][2] > R.m[i][i]) i = 2;
        const int j = (i + 1) % 3, k = (j + 1) % 3;
        t = std::sqrt(R.m[i][i] - R.m[j][j] - R.m[k][k] + 1.0);
        q[i] = 0.5 * t;
        t = 0.5 / t;
        q[3] = (R.m[k][j] - R.m[j][k]) * t;
        q[j] = (R.m[j][i] + R.m[i][j]) * t;
        q[k] = (R.m[k][i] + R.m[i][k]) * t;
    }
    file << std::setprecision(6) << std::fixed << q[0] << " " << q[1] << " " << q[2] << " " << q[3];
    file << "\n";
    const std::string line = file.str();
    if ((int)line.size() >= cap) return DMSA_ERR_INVALID;
    std::memcpy(out, line.c_str(), line.size() + 1);
    return (int)line.size();
}

// saveDensePoses :148-153 / makeNonKeyframePoseGlobal :176-182
int orc_compose_nonkeyframe_pose(const double* keyframePos, const double* keyframeOrient, const double* Translation, const double* Orientation, double* globalPos,
                                 double* globalOrient) {
    const M3 keyRot = axang2rotm(keyframeOrient);
    double rt[3];
    matvec(keyRot, Translation, rt);
    for (int c = 0; c < 3; ++c) globalPos[c] = rt[c] + keyframePos[c];
    rotm2axang(mul(keyRot, axang2rotm(Orientation)), globalOrient);
    return DMSA_OK;
}

}  // extern "C"

// ================================================================================================================================
// keyframe creation (DmsaSlam.h:469-567) -- pcl::NormalEstimationOMP restated, brute-force neighbours
// ================================================================================================================================
namespace {

// pcl/common/impl/eigen.hpp (PCL 1.10): computeRoots2, computeRoots, eigen33 (smallest eigenvalue / eigenvector), float
static void pclComputeRoots2(float b, float c, float* roots) {
    roots[0] = 0.0f;
    float d = float(b * b - 4.0 * c);
    if (d < 0.0) d = 0.0;
    const float sd = std::sqrt(d);
    roots[2] = 0.5f * (b + sd);
    roots[1] = 0.5f * (b - sd);
}
static void pclComputeRoots(const float m[3][3], float* roots) {
    const float c0 = m[0][0] * m[1][1] * m[2][2] + 2.0f * m[0][1] * m[0][2] * m[1][2] - m[0][0] * m[1][2] * m[1][2] - m[1][1] * m[0][2] * m[0][2] -
                     m[2][2] * m[0][1] * m[0][1];
    const float c1 = m[0][0] * m[1][1] - m[0][1] * m[0][1] + m[0][0] * m[2][2] - m[0][2] * m[0][2] + m[1][1] * m[2][2] - m[1][2] * m[1][2];
    const float c2 = m[0][0] + m[1][1] + m[2][2];
    if (std::abs(c0) < std::numeric_limits<float>::epsilon()) {
        pclComputeRoots2(c2, c1, roots);
        return;
    }
    const float s_inv3 = float(1.0 / 3.0);
    const float s_sqrt3 = std::sqrt(float(3.0));
    const float c2_over_3 = c2 * s_inv3;
    float a_over_3 = (c1 - c2 * c2_over_3) * s_inv3;
    if (a_over_3 > 0.0f) a_over_3 = 0.0f;
    const float half_b = 0.5f * (c0 + c2_over_3 * (2.0f * c2_over_3 * c2_over_3 - c1));
    float q = half_b * half_b + a_over_3 * a_over_3 * a_over_3;
    if (q > 0.0f) q = 0.0f;
    const float rho = std::sqrt(-a_over_3);
    // std::atan2 / cos / sin on floats, stated as their correctly rounded values (double evaluation, one rounding)
    const float theta = (float)dmsa_det::det_atan2((double)std::sqrt(-q), (double)half_b) * s_inv3;
    const float cos_theta = (float)dmsa_det::det_cos((double)theta);
    const float sin_theta = (float)dmsa_det::det_sin((double)theta);
    roots[0] = c2_over_3 + 2.0f * rho * cos_theta;
    roots[1] = c2_over_3 - rho * (cos_theta + s_sqrt3 * sin_theta);
    roots[2] = c2_over_3 - rho * (cos_theta - s_sqrt3 * sin_theta);
    if (roots[0] >= roots[1]) std::swap(roots[0], roots[1]);
    if (roots[1] >= roots[2]) {
        std::swap(roots[1], roots[2]);
        if (roots[0] >= roots[1]) std::swap(roots[0], roots[1]);
    }
    if (roots[0] <= 0) pclComputeRoots2(c2, c1, roots);
}

// NormalEstimation::computeFeature for one point given its neighbour list (pcl/features/normal_3d.h)
static void pclPointNormal(const float* cloud, const int* nn, int count, const float* point, const float* vp, float* out) {
    const float nanv = std::numeric_limits<float>::quiet_NaN();
    if (count < 3) {
        out[0] = out[1] = out[2] = out[3] = nanv;
        return;
    }
    float accu[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};  // computeMeanAndCovarianceMatrix
    for (int m = 0; m < count; ++m) {
        const float* p = cloud + 4 * (size_t)nn[m];
        accu[0] += p[0] * p[0], accu[1] += p[0] * p[1], accu[2] += p[0] * p[2], accu[3] += p[1] * p[1], accu[4] += p[1] * p[2], accu[5] += p[2] * p[2];
        accu[6] += p[0], accu[7] += p[1], accu[8] += p[2];
    }
    for (float& a : accu) a /= static_cast<float>(count);
    float cov[3][3];
    cov[0][0] = accu[0] - accu[6] * accu[6], cov[0][1] = accu[1] - accu[6] * accu[7], cov[0][2] = accu[2] - accu[6] * accu[8];
    cov[1][1] = accu[3] - accu[7] * accu[7], cov[1][2] = accu[4] - accu[7] * accu[8], cov[2][2] = accu[5] - accu[8] * accu[8];
    cov[1][0] = cov[0][1], cov[2][0] = cov[0][2], cov[2][1] = cov[1][2];
    // solvePlaneParameters -> eigen33
    float scale = 0.0f;
    for (auto& r : cov)
        for (float v : r) scale = std::max(scale, std::abs(v));
    if (scale <= std::numeric_limits<float>::min()) scale = 1.0f;
    float sm[3][3];
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c) sm[r][c] = cov[r][c] / scale;
    float roots[3];
    pclComputeRoots(sm, roots);
    const float eigenvalue = roots[0] * scale;
    for (int d = 0; d < 3; ++d) sm[d][d] -= roots[0];
    auto cross = [](const float* a, const float* b, float* o) { o[0] = a[1] * b[2] - a[2] * b[1], o[1] = a[2] * b[0] - a[0] * b[2], o[2] = a[0] * b[1] - a[1] * b[0]; };
    float vec1[3], vec2[3], vec3[3];
    cross(sm[0], sm[1], vec1), cross(sm[0], sm[2], vec2), cross(sm[1], sm[2], vec3);
    auto sq = [](const float* v) { const float t = v[1] * v[1] + v[2] * v[2]; return v[0] * v[0] + t; };  // Eigen's 3-term redux
    const float len1 = sq(vec1), len2 = sq(vec2), len3 = sq(vec3);
    const float* best = vec3;
    float len = len3;
    if (len1 >= len2 && len1 >= len3)
        best = vec1, len = len1;
    else if (len2 >= len1 && len2 >= len3)
        best = vec2, len = len2;
    const float s = std::sqrt(len);
    float nx = best[0] / s, ny = best[1] / s, nz = best[2] / s;
    const float eig_sum = cov[0][0] + cov[1][1] + cov[2][2];
    const float curvature = eig_sum != 0 ? std::abs(eigenvalue / eig_sum) : 0.0f;
    // flipNormalTowardsViewpoint
    const float vx = vp[0] - point[0], vy = vp[1] - point[1], vz = vp[2] - point[2];
    const float cos_theta = (vx * nx + vy * ny + vz * nz);
    if (cos_theta < 0) nx *= -1, ny *= -1, nz *= -1;
    out[0] = nx, out[1] = ny, out[2] = nz, out[3] = curvature;
}

}  // namespace

extern "C" {

// DmsaSlam::updateNormals (DmsaSlam.h:553-567).  Neighbours: exhaustive search, ascending (L2_Simple float distance, index).
int orc_update_normals(const float* xyz, int64_t n, int32_t k, const float* viewpoint, float* normal_out, int32_t* nn_index_out) {
    if (k < 1 || k > 8) return DMSA_ERR_INVALID;
#pragma omp parallel for schedule(dynamic, 64)
    for (int64_t i = 0; i < n; ++i) {
        const float* q = xyz + 4 * (size_t)i;
        int nn[8];
        float nd[8];
        int count = 0;
        if (std::isfinite(q[0]) && std::isfinite(q[1]) && std::isfinite(q[2])) {
            for (int64_t j = 0; j < n; ++j) {
                const float* p = xyz + 4 * (size_t)j;
                if (!(std::isfinite(p[0]) && std::isfinite(p[1]) && std::isfinite(p[2]))) continue;
                const float dx = q[0] - p[0], dy = q[1] - p[1], dz = q[2] - p[2];
                float d = 0.0f;
                d += dx * dx;
                d += dy * dy;
                d += dz * dz;
                if (count == k && !(d < nd[k - 1])) continue;  // ascending j: a later equal distance never displaces an earlier one
                int at = count < k ? count : k - 1;
                while (at > 0 && d < nd[at - 1]) nd[at] = nd[at - 1], nn[at] = nn[at - 1], --at;
                nd[at] = d, nn[at] = (int)j;
                if (count < k) ++count;
            }
        }
        if (nn_index_out)
            for (int m = 0; m < k; ++m) nn_index_out[(size_t)i * k + m] = m < count ? nn[m] : -1;
        pclPointNormal(xyz, nn, count, q, viewpoint, normal_out + 4 * (size_t)i);
    }
    return DMSA_OK;
}

// the cloud part of DmsaSlam::addNewKeyframeToMap (DmsaSlam.h:497-531)
int orc_make_keyframe_cloud(const float* global_xyz, const int32_t* ids, int64_t n, float min_grid_size, uint32_t seed, const double* pos0, const double* orient0,
                            float* xyz_local_out, float* normal_out, int32_t* ring_out, int32_t* src_index_out, int64_t capacity, int64_t* num_out) {
    std::vector<int32_t> pick((size_t)std::max<int64_t>(n, 1));
    int64_t m = 0;
    const int rc = orc_random_grid_downsampling(global_xyz, n, min_grid_size, seed, pick.data(), n, &m);
    if (rc != DMSA_OK) return rc;
    if (num_out) *num_out = m;
    if (m > capacity) return DMSA_ERR_INVALID;
    const M3 R = axang2rotm(orient0);
    float currRotInv[3][3];
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c) currRotInv[r][c] = (float)R.m[c][r];
    const float currWorldPose[3] = {(float)pos0[0], (float)pos0[1], (float)pos0[2]};
    for (int64_t k = 0; k < m; ++k) {
        const float* p = global_xyz + 4 * (size_t)pick[(size_t)k];
        const float d[3] = {p[0] - currWorldPose[0], p[1] - currWorldPose[1], p[2] - currWorldPose[2]};
        for (int r = 0; r < 3; ++r) {
            const float t = currRotInv[r][1] * d[1] + currRotInv[r][2] * d[2];
            xyz_local_out[4 * (size_t)k + r] = currRotInv[r][0] * d[0] + t;
        }
        xyz_local_out[4 * (size_t)k + 3] = 1.0f;
        ring_out[(size_t)k] = ids[(size_t)pick[(size_t)k]];
        if (src_index_out) src_index_out[(size_t)k] = pick[(size_t)k];
    }
    const float origin[3] = {0.0f, 0.0f, 0.0f};
    return orc_update_normals(xyz_local_out, m, 6, origin, normal_out, nullptr);
}

}  // extern "C"

