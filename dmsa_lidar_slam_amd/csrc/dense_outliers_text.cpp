// dense_outliers_text.cpp — the host-only side of include/dmsa_dense_outliers.h: the defaults and O5, the threshold from the three exact sums.
// No device, no context.  Built with -ffp-contract=off: every operation of O5 is rounded on its own.
#include "../../include/dmsa_dense_outliers.h"

#include <cmath>

extern "C" {

void dmsa_default_dense_outlier_config(dmsa_dense_outlier_config* cfg) {
    if (!cfg) return;
    cfg->radius = 0.3f, cfg->k = 8, cfg->stddev_mul = 1.0f, cfg->pad = 0;
}

int dmsa_dense_outlier_threshold(int64_t n_s, int64_t s1, int64_t s2, float stddev_mul, double* mean_q, double* stddev_q, double* threshold_q) {
    if (mean_q) *mean_q = 0.0;
    if (stddev_q) *stddev_q = 0.0;
    if (threshold_q) *threshold_q = 0.0;
    if (n_s < 0 || s1 < 0 || s2 < 0 || !std::isfinite(stddev_mul) || stddev_mul < 0.0f) return DMSA_ERR_INVALID;
    if (n_s == 0) return DMSA_OK;  // every row is isolated: T = 0
    const double n = (double)n_s, a = (double)s1, b = (double)s2;
    const double mean = a / n;
    double var = 0.0;
    if (n_s >= 2) {
        const double sq = a * a;
        const double part = sq / n;
        const double diff = b - part;
        var = diff / (double)(n_s - 1);
        if (var < 0.0) var = 0.0;
    }
    const double sd = std::sqrt(var);
    const double spread = (double)stddev_mul * sd;
    if (mean_q) *mean_q = mean;
    if (stddev_q) *stddev_q = sd;
    if (threshold_q) *threshold_q = mean + spread;
    return DMSA_OK;
}

}  // extern "C"
