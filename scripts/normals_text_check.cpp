// normals_text_check.cpp — a stand-alone host program around the host-only calls of include/dmsa_dense_normals.h
// (csrc/dense_normals_text.cpp), meant for a sanitizer build:
//
//   c++ -std=c++17 -g -O1 -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all -Iinclude scripts/normals_text_check.cpp \
//       dmsa_lidar_slam_amd/csrc/dense_normals_text.cpp -o /tmp/normals_text_check && /tmp/normals_text_check
//
// The header is written into heap blocks of exactly `cap` bytes at every capacity around its length (a write past the end is a heap overflow
// the sanitizer sees); dmsa_dense_normal_from_moments gets moment sets at the edges of its arithmetic: too few neighbours, one point three
// times, three points on a line, the largest sums N1 admits, zeros.  Needs no device and nothing else of the library.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "dmsa_dense_normals.h"

static int failures = 0;

static void expect(bool ok, const char* what) {
    if (!ok) {
        std::fprintf(stderr, "FAILED: %s\n", what);
        ++failures;
    }
}

int main() {
    char big[512];
    const int len = dmsa_pcd_header_normals_binary(123456789012ll, big, (int32_t)sizeof(big));
    expect(len > 0 && (int)std::strlen(big) == len, "header length");
    for (int cap = 0; cap <= len + 2; ++cap) {
        char* block = static_cast<char*>(std::malloc(cap > 0 ? (size_t)cap : 1));
        const int rc = dmsa_pcd_header_normals_binary(42, cap > 0 ? block : nullptr, cap);
        expect(cap > len ? rc == len : rc == DMSA_ERR_INVALID, "header capacity");
        std::free(block);
    }
    expect(dmsa_pcd_header_normals_binary(-1, big, 512) == DMSA_ERR_INVALID && dmsa_pcd_header_normals_binary(1000000000000ll, big, 512) == DMSA_ERR_INVALID, "header range");

    dmsa_dense_normals_config cfg;
    dmsa_default_dense_normals_config(&cfg);
    dmsa_default_dense_normals_config(nullptr);
    expect(cfg.radius == 0.3f && cfg.min_neighbours == 5, "defaults");

    const float view[3] = {0.0f, 0.0f, 1.0f};
    const int64_t big_q = (int64_t)1 << 20, n_max = (int64_t)1 << 22;
    const int64_t cases[][10] = {
        {0, 0, 0, 0, 0, 0, 0, 0, 0, 0},
        {2, 3, 3, 3, 9, 9, 9, 9, 9, 9},
        {3, 0, 0, 0, 0, 0, 0, 0, 0, 0},                                                               // one point three times
        {3, 0, 0, 0, 2, 2, 2, 2, 2, 2},                                                               // three points on a line
        {4, 0, 0, 0, 2, 0, 0, 2, 0, 0},                                                               // a plane
        {n_max, n_max * big_q, -n_max * big_q, 0, n_max * big_q * big_q, -n_max * big_q * big_q, 0, n_max * big_q * big_q, 0, 1},  // the largest sums
    };
    for (const auto& m : cases) {
        float out[4], again[4];
        expect(dmsa_dense_normal_from_moments(m, view, 3, out) == DMSA_OK && dmsa_dense_normal_from_moments(m, view, 3, again) == DMSA_OK, "status");
        expect(std::memcmp(out, again, sizeof(out)) == 0, "repeatable");
        if (m[0] < 3) expect(std::isnan(out[0]) && std::isnan(out[3]), "too few neighbours give NaNs");
    }
    float out[4];
    expect(dmsa_dense_normal_from_moments(nullptr, view, 3, out) == DMSA_ERR_INVALID && dmsa_dense_normal_from_moments(cases[4], nullptr, 3, out) == DMSA_ERR_INVALID &&
               dmsa_dense_normal_from_moments(cases[4], view, 3, nullptr) == DMSA_ERR_INVALID, "null arguments");
    expect(dmsa_dense_normal_from_moments(cases[4], view, 3, out) == DMSA_OK && out[0] == 0.0f && out[1] == 0.0f && out[2] == 1.0f && out[3] == 0.0f, "the plane z = 0");
    std::printf("%s\n", failures ? "FAILED" : "ok");
    return failures ? 1 : 0;
}
