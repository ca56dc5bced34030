// outliers_text_check.cpp — a stand-alone host program around the host-only calls of include/dmsa_dense_outliers.h
// (csrc/dense_outliers_text.cpp), meant for a sanitizer build:
//
//   c++ -std=c++17 -g -O1 -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all -Iinclude scripts/outliers_text_check.cpp \
//       dmsa_lidar_slam_amd/csrc/dense_outliers_text.cpp -o /tmp/outliers_text_check && /tmp/outliers_text_check
//
// dmsa_dense_outlier_threshold gets the sums at the edges of its arithmetic -- no row, one row, two rows, equal values whose rounded variance
// falls below zero, the largest sums O1 admits (2^26 rows of q = 2^18: S2 = 2^62, where a signed overflow in an integer product would show),
// each output pointer alone and none at all (the results go into heap blocks of exactly their size) -- and the arguments it has to
// refuse.  The header itself is compiled as C++ here; the structs' sizes are the ones the Python mirror assumes.  Needs no device and nothing
// else of the library.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>

#include "dmsa_dense_outliers.h"

static int failures = 0;

static void expect(bool ok, const char* what) {
    if (!ok) {
        std::fprintf(stderr, "FAILED: %s\n", what);
        ++failures;
    }
}

// O5 restated: the check is against an independent statement of the rule, one operation per line
static double model(int64_t n_s, int64_t s1, int64_t s2, float mul, double* mean_out, double* sd_out) {
    *mean_out = *sd_out = 0.0;
    if (n_s == 0) return 0.0;
    const double n = (double)n_s, a = (double)s1, b = (double)s2;
    const double mean = a / n;
    double var = 0.0;
    if (n_s >= 2) {
        volatile double sq = a * a;
        volatile double part = sq / n;
        volatile double diff = b - part;
        var = diff / (double)(n_s - 1);
        if (var < 0.0) var = 0.0;
    }
    *mean_out = mean, *sd_out = std::sqrt(var);
    return mean + (double)mul * *sd_out;
}

int main() {
    static_assert(sizeof(dmsa_dense_outlier_config) == 16, "config layout");
    static_assert(sizeof(dmsa_dense_outlier_stats) == 80, "stats layout");
    dmsa_dense_outlier_config cfg;
    std::memset(&cfg, 0x5A, sizeof(cfg));
    dmsa_default_dense_outlier_config(&cfg);
    dmsa_default_dense_outlier_config(nullptr);
    expect(cfg.radius == 0.3f && cfg.k == 8 && cfg.stddev_mul == 1.0f && cfg.pad == 0, "defaults");

    const int64_t rows_max = (int64_t)1 << 26, q_max = (int64_t)1 << 18;
    const int64_t cases[][3] = {
        {0, 0, 0},
        {1, 7, 49},
        {1, q_max, q_max * q_max},
        {2, 10, 52},
        {2, 3, 5},
        {3, 30, 302},
        {3, 3 * 144523ll, 3 * 144523ll * 144523ll},
        {123457, 123457ll * 77777, 123457ll * 77777 * 77777},
        {rows_max - 3, (rows_max - 3) * 181817, (rows_max - 3) * 181817 * 181817},
        {rows_max, rows_max * q_max, rows_max * q_max * q_max},  // S2 = 2^62
        {rows_max, rows_max * q_max - (1 << 20), rows_max * q_max * q_max - ((int64_t)1 << 39)},
        {std::numeric_limits<int64_t>::max(), std::numeric_limits<int64_t>::max(), std::numeric_limits<int64_t>::max()},  // beyond O1: still no overflow
    };
    const float muls[] = {0.0f, 1.0f, 2.5f, 1e6f};
    int negative = 0;
    for (const auto& c : cases) {
        for (const float mul : muls) {
            double* out = static_cast<double*>(std::malloc(3 * sizeof(double)));  // exactly the three results; `lone`: exactly one
            double* lone = static_cast<double*>(std::malloc(sizeof(double)));
            expect(dmsa_dense_outlier_threshold(c[0], c[1], c[2], mul, out, out + 1, out + 2) == DMSA_OK, "status");
            double mean = 0.0, sd = 0.0;
            const double t = model(c[0], c[1], c[2], mul, &mean, &sd);
            expect(std::memcmp(&out[0], &mean, 8) == 0 && std::memcmp(&out[1], &sd, 8) == 0 && std::memcmp(&out[2], &t, 8) == 0, "O5, bit for bit");
            expect(out[1] >= 0.0 && out[2] >= out[0], "stddev >= 0 and T >= mean");
            expect(dmsa_dense_outlier_threshold(c[0], c[1], c[2], mul, nullptr, nullptr, lone) == DMSA_OK && std::memcmp(lone, &t, 8) == 0, "threshold alone");
            expect(dmsa_dense_outlier_threshold(c[0], c[1], c[2], mul, lone, nullptr, nullptr) == DMSA_OK && std::memcmp(lone, &mean, 8) == 0, "mean alone");
            expect(dmsa_dense_outlier_threshold(c[0], c[1], c[2], mul, nullptr, lone, nullptr) == DMSA_OK && std::memcmp(lone, &sd, 8) == 0, "stddev alone");
            expect(dmsa_dense_outlier_threshold(c[0], c[1], c[2], mul, nullptr, nullptr, nullptr) == DMSA_OK, "no output at all");
            std::free(out);
            std::free(lone);
        }
        if (c[0] >= 2 && (double)c[2] - ((double)c[1] * (double)c[1]) / (double)c[0] < 0.0) ++negative;
    }
    expect(negative > 0, "a case whose rounded variance is negative");
    double a = 1.0, b = 1.0, t = 1.0;
    expect(dmsa_dense_outlier_threshold(0, 0, 0, 3.0f, &a, &b, &t) == DMSA_OK && a == 0.0 && b == 0.0 && t == 0.0, "no row: T = 0");
    expect(dmsa_dense_outlier_threshold(3, 30, 302, 1.0f, &a, &b, &t) == DMSA_OK && a == 10.0 && b == 1.0 && t == 11.0, "10 +- 1");
    const float bad_mul[] = {-1.0f, -0.0f - 1e-30f, std::numeric_limits<float>::quiet_NaN(), std::numeric_limits<float>::infinity()};
    for (const float mul : bad_mul) {
        a = b = t = 5.0;
        expect(dmsa_dense_outlier_threshold(3, 30, 302, mul, &a, &b, &t) == DMSA_ERR_INVALID && a == 0.0 && b == 0.0 && t == 0.0, "stddev_mul refused");
    }
    expect(dmsa_dense_outlier_threshold(-1, 0, 0, 1.0f, &a, &b, &t) == DMSA_ERR_INVALID && dmsa_dense_outlier_threshold(3, -30, 302, 1.0f, &a, &b, &t) == DMSA_ERR_INVALID &&
               dmsa_dense_outlier_threshold(3, 30, -302, 1.0f, &a, &b, &t) == DMSA_ERR_INVALID, "negative sums refused");
    expect(dmsa_dense_outlier_threshold(3, 30, 302, -0.0f, &a, &b, &t) == DMSA_OK && t == 10.0, "minus zero is zero");
    std::printf("%s\n", failures ? "FAILED" : "ok");
    return failures ? 1 : 0;
}
