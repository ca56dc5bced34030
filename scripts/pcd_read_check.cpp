// pcd_read_check.cpp — a stand-alone host program around dmsa_pcd_xyz_info / dmsa_pcd_xyz_read (csrc/dense_compare_text.cpp), meant for a
// sanitizer build:
//
//   c++ -std=c++17 -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=all -Iinclude scripts/pcd_read_check.cpp \
//       dmsa_lidar_slam_amd/csrc/dense_compare_text.cpp dmsa_lidar_slam_amd/csrc/dense_clusters_text.cpp dmsa_lidar_slam_amd/csrc/dense_intensity_text.cpp \
//       dmsa_lidar_slam_amd/csrc/dense_normals_text.cpp dmsa_lidar_slam_amd/csrc/dense_cloud_text.cpp -o /tmp/pcd_read_check && /tmp/pcd_read_check [file.pcd ...]
//
// The reader takes files from outside (include/dmsa_dense_compare.h, D8).  Every file below is one of the library's own layouts, assembled
// from its host-only header functions, and is handed to the reader whole and at EVERY prefix length, with an output array of exactly the
// rows it may write (a write past it is a heap overflow the sanitizer sees); then a handful of hostile headers.  A prefix is either read
// whole (the rows were all there) or refused; nothing else is a pass.  Files named on the command line are read the same way.  Needs no
// device and nothing else of the library.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <unistd.h>
#include <vector>

#include "dmsa_dense_compare.h"
#include "dmsa_dense_intensity.h"

static int failures = 0;

static void expect(bool ok, const std::string& what) {
    if (!ok) {
        std::fprintf(stderr, "FAILED: %s\n", what.c_str());
        ++failures;
    }
}

static std::string g_path;

static void write_file(const std::string& bytes) {
    std::FILE* f = std::fopen(g_path.c_str(), "wb");
    if (!f || std::fwrite(bytes.data(), 1, bytes.size(), f) != bytes.size()) {
        std::fprintf(stderr, "cannot write %s\n", g_path.c_str());
        std::exit(2);
    }
    std::fclose(f);
}

// the file at g_path through info and read, the output an exact-size heap block; returns read's status, *rows = the file's rows
static int read_exact(int64_t* rows, std::vector<float>* xyz = nullptr) {
    int64_t n = -1;
    const int info = dmsa_pcd_xyz_info(g_path.c_str(), &n);
    expect((info == DMSA_OK) == (dmsa_pcd_xyz_last_error()[0] == 0), "a refusal has a reason, a success none");
    if (info != DMSA_OK) {
        expect(n == 0, "a refused info reports no rows");
        float sentinel[3] = {7.0f, 7.0f, 7.0f};
        expect(dmsa_pcd_xyz_read(g_path.c_str(), sentinel, 1, &n) != DMSA_OK && sentinel[0] == 7.0f, "read refuses what info refused, and writes nothing");
        return *rows = 0, info;
    }
    float* block = static_cast<float*>(std::malloc(n ? (size_t)n * 12 : 1));
    int64_t m = -1;
    const int rc = dmsa_pcd_xyz_read(g_path.c_str(), block, n, &m);
    expect(rc == DMSA_OK && m == n, "read follows info");
    if (n > 0) {
        int64_t k = -1;
        float* small = static_cast<float*>(std::malloc((size_t)(n - 1) * 12 + 1));
        expect(dmsa_pcd_xyz_read(g_path.c_str(), small, n - 1, &k) == DMSA_ERR_INVALID && k == n, "room for one row less is refused");
        std::free(small);
    }
    if (xyz) xyz->assign(block, block + 3 * n);
    std::free(block);
    return *rows = n, rc;
}

// rows of `floats` floats each with x y z first, as the library's files have them
static std::string body_of(int64_t n, int floats) {
    std::vector<float> v((size_t)n * (size_t)floats);
    for (size_t i = 0; i < v.size(); ++i) v[i] = (float)i * 0.25f - 3.0f;
    return std::string(reinterpret_cast<const char*>(v.data()), v.size() * 4);
}

int main(int argc, char** argv) {
    char name[] = "/tmp/pcd_read_check_XXXXXX";
    const int fd = mkstemp(name);
    if (fd < 0) return 2;
    close(fd);
    g_path = name;
    struct Layout {
        const char* what;
        int floats;
        int (*header)(int64_t, char*, int32_t);
        int (*header_i)(int64_t, int32_t, char*, int32_t);
        int32_t intensity;
    };
    const Layout layouts[] = {{"x y z", 3, dmsa_pcd_header_xyz_binary, nullptr, 0},
                              {"x y z intensity", 4, dmsa_pcd_header_xyzi_binary, nullptr, 0},
                              {"x y z and normals", 7, dmsa_pcd_header_normals_binary, nullptr, 0},
                              {"x y z intensity and normals", 8, dmsa_pcd_header_xyzi_normals_binary, nullptr, 0},
                              {"x y z label", 4, nullptr, dmsa_pcd_header_xyz_label_binary, 0},
                              {"x y z intensity label", 5, nullptr, dmsa_pcd_header_xyz_label_binary, 1},
                              {"x y z distance", 4, nullptr, dmsa_pcd_header_xyz_distance_binary, 0},
                              {"x y z intensity distance", 5, nullptr, dmsa_pcd_header_xyz_distance_binary, 1}};
    const int64_t n = 5;
    for (const Layout& l : layouts) {
        char head[512];
        const int hn = l.header ? l.header(n, head, 512) : l.header_i(n, l.intensity, head, 512);
        expect(hn > 0, std::string("header of ") + l.what);
        const std::string whole = std::string(head, (size_t)hn) + body_of(n, l.floats);
        int64_t rows = -1;
        std::vector<float> xyz;
        write_file(whole);
        expect(read_exact(&rows, &xyz) == DMSA_OK && rows == n, std::string("whole file: ") + l.what);
        for (int64_t i = 0; i < rows; ++i)
            for (int a = 0; a < 3; ++a) expect(xyz[(size_t)(3 * i + a)] == (float)(i * l.floats + a) * 0.25f - 3.0f, std::string("coordinates of ") + l.what);
        for (size_t len = 0; len < whole.size(); ++len) {  // every proper prefix lacks at least one byte of the last row
            write_file(whole.substr(0, len));
            expect(read_exact(&rows) == DMSA_ERR_INVALID, std::string("prefix of ") + l.what);
        }
        write_file(whole + "more bytes behind the rows");
        expect(read_exact(&rows) == DMSA_OK && rows == n, std::string("bytes behind the rows: ") + l.what);
    }
    // hostile headers: each is refused (or read, where it is legal after all) without a read or a write out of bounds
    char good_head[512];
    const std::string good(good_head, (size_t)dmsa_pcd_header_xyz_binary(2, good_head, 512));
    const auto with = [&](const char* from, const std::string& to) {
        std::string s = good;
        const size_t at = s.find(from);
        if (at != std::string::npos) s.replace(at, std::strlen(from), to);
        return s;
    };
    const std::string rows24 = body_of(2, 3);
    const std::string hostile[] = {
        with("DATA binary", "DATA ascii"),
        with("DATA binary", "DATA binary_compressed"),
        with("DATA binary\n", "DATA"),
        with("DATA binary\n", "DATA binary"),
        with("FIELDS x y z", "FIELDS x y"),
        with("FIELDS x y z", "FIELDS"),
        with("FIELDS x y z", "FIELDS x x x"),
        with("SIZE 4 4 4", "SIZE 4 4 40000000000000000000"),
        with("SIZE 4 4 4", "SIZE 4 4 -4"),
        with("SIZE 4 4 4", "SIZE 8 8 8"),
        with("TYPE F F F", "TYPE F F"),
        with("COUNT 1 1 1", "COUNT 1 1 0"),
        with("COUNT 1 1 1", "COUNT 1 1 99999999999"),
        with("000000000002", "999999999999"),
        with("000000000002", "9999999999999999999999999999999999999999"),
        with("000000000002", "-2"),
        with("000000000002", "2 2"),
        with("000000000002", ""),
        with("HEIGHT 1", "HEIGHT 4611686018427387904"),
        with("HEIGHT 1", "HEIGHT 999999999999"),
        with("VERSION 0.7", "VERSION"),
        with("# .PCD", std::string(511, '#')),
        with("# .PCD", std::string(512, '#')),
        with("# .PCD", std::string(100000, '#')),
        with("FIELDS x y z", "FIELDS x y z" + std::string(300, ' ') + std::string(300, 'q')),
        with("VIEWPOINT 0 0 0 1 0 0 0\n", ""),
        with("VIEWPOINT", std::string("VIEW\0POINT", 10)),
        std::string("\0\0\0\0", 4),
        std::string(600, '\n'),
        std::string(600, ' '),
        std::string("FIELDS x y z\nSIZE 4 4 4\nTYPE F F F\nWIDTH 2\nHEIGHT 1\nPOINTS 2\nDATA binary\n"),  // (legal: no version, no count, no viewpoint)
    };
    for (const std::string& h : hostile) {
        int64_t rows = -1;
        write_file(h + rows24);
        const int rc = read_exact(&rows);
        expect(rc == DMSA_OK || rc == DMSA_ERR_INVALID, "a hostile header");
        write_file(h);
        read_exact(&rows);
    }
    // a field of 2^20 counts of 8 bytes: the row is too long to be read, whatever the file holds
    {
        int64_t rows = -1;
        std::string s = with("FIELDS x y z", "FIELDS x y z w");
        s.replace(s.find("SIZE 4 4 4"), 10, "SIZE 4 4 4 8"), s.replace(s.find("TYPE F F F"), 10, "TYPE F F F F"), s.replace(s.find("COUNT 1 1 1"), 11, "COUNT 1 1 1 1048576");
        write_file(s + rows24);
        expect(read_exact(&rows) == DMSA_ERR_INVALID && std::strstr(dmsa_pcd_xyz_last_error(), "a row of 8388620 bytes"), "an over-long row");
    }
    int64_t rows = -1;
    expect(dmsa_pcd_xyz_info("/nonexistent/dir/file.pcd", &rows) == DMSA_ERR_INVALID && rows == 0, "a file that is not there");
    expect(dmsa_pcd_xyz_info(nullptr, &rows) == DMSA_ERR_INVALID && dmsa_pcd_xyz_info(g_path.c_str(), nullptr) == DMSA_ERR_INVALID, "null arguments");
    expect(dmsa_pcd_xyz_read(g_path.c_str(), nullptr, 1, &rows) == DMSA_ERR_INVALID && dmsa_pcd_xyz_read(g_path.c_str(), nullptr, -1, nullptr) == DMSA_ERR_INVALID, "null output");
    std::remove(g_path.c_str());
    for (int a = 1; a < argc; ++a) {
        g_path = argv[a];
        const int rc = read_exact(&rows);
        std::printf("%s: status %d, %lld rows%s%s\n", argv[a], rc, (long long)rows, rc == DMSA_OK ? "" : ", ", dmsa_pcd_xyz_last_error());
    }
    std::printf("pcd_read_check: %d failure(s)\n", failures);
    return failures ? 1 : 0;
}
