// tum_parse_check.cpp — a stand-alone host program around dmsa_parse_tum_poses (csrc/dense_cloud_text.cpp), meant for a sanitizer build:
//
//   c++ -std=c++17 -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=all -Iinclude scripts/tum_parse_check.cpp \
//       dmsa_lidar_slam_amd/csrc/dense_cloud_text.cpp -o /tmp/tum_parse_check && /tmp/tum_parse_check [Poses.txt ...]
//
// The parser reads files from outside.  Every text below is handed over in a heap block of exactly its length (no terminating zero, so a read
// past the end is a heap overflow the sanitizer sees), with output arrays of exactly `cap` entries, and at every prefix length.  Files named
// on the command line are parsed the same way.  Needs no device and nothing else of the library.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "dmsa_dense_cloud.h"

static int failures = 0;

static void expect(bool ok, const char* what) {
    if (!ok) {
        std::fprintf(stderr, "FAILED: %s\n", what);
        ++failures;
    }
}

// parse `text` from an exact-size heap copy into exact-size outputs
static int parse_exact(const std::string& text, int64_t cap, int64_t* n, std::string* err, int32_t err_cap = 64) {
    char* block = static_cast<char*>(std::malloc(text.size() ? text.size() : 1));
    std::memcpy(block, text.data(), text.size());
    std::vector<double> st((size_t)cap), ps((size_t)cap * 3), qs((size_t)cap * 4);
    char* e = err_cap > 0 ? static_cast<char*>(std::malloc((size_t)err_cap)) : nullptr;
    const int rc = dmsa_parse_tum_poses(block, (int64_t)text.size(), cap ? st.data() : nullptr, cap ? ps.data() : nullptr, cap ? qs.data() : nullptr, cap, n, e, err_cap);
    if (err) *err = e ? e : "";
    std::free(e);
    std::free(block);
    return rc;
}

int main(int argc, char** argv) {
    const std::string good = "# stamp tx ty tz qx qy qz qw\n1600000000.100000 1.00000 -2.00000 3.00000 0.000000 0.000000 0.000000 1.000000\n\n"
                             "1600000000.200000 1.10000 -2.10000 3.10000 0.100000 0.000000 0.000000 0.994987\r\n   \t\n"
                             "1600000000.300000 1e0 -2.2 +3.2 .1 0 0 0.994987";
    int64_t n = -1;
    std::string err;
    expect(parse_exact(good, 3, &n, &err) == DMSA_OK && n == 3, "three poses");
    expect(parse_exact(good, 2, &n, &err) == DMSA_ERR_INVALID && n == 3, "capacity 2 of 3");
    expect(parse_exact(good, 0, &n, &err) == DMSA_ERR_INVALID && n == 3, "counting pass");
    expect(parse_exact("", 0, &n, &err) == DMSA_OK && n == 0, "empty text");
    // every prefix: a text cut anywhere is either fewer poses or a malformed last line, never a read past the end
    for (size_t len = 0; len <= good.size(); ++len) {
        const int rc = parse_exact(good.substr(0, len), 3, &n, &err, len % 3 == 0 ? 8 : 64);
        expect(rc == DMSA_OK || (rc == DMSA_ERR_INVALID && err.rfind("line ", 0) == 0), "prefix");
    }
    const char* bad[] = {"1 2 3 4 5 6 7", "1 2 3 4 5 6 7 8 9", "1 2 3 4 x 6 7 8", "1 2 3 4 5 6 7 8x", "1,2,3,4,5,6,7,8", "nan inf -inf 0x1p3 1e999 1e-999 0 1",
                         "\n\n\n#\n#", "\r\r\r", "1 2 3 4 5 6 7 8\n-", "1 2 3 4 5 6 7 8\n+", "1 2 3 4 5 6 7 8\n1e", "1 2 3 4 5 6 7 .", "\0 1 2 3"};
    for (const char* b : bad) {
        const int rc = parse_exact(b, 4, &n, &err);
        expect(rc == DMSA_OK || rc == DMSA_ERR_INVALID, b);
    }
    expect(parse_exact(std::string("1 2 3 4 5 6 7 8\n1 2 3 \0 5 6 7 8\n", 32), 4, &n, &err) == DMSA_ERR_INVALID && err.rfind("line 2:", 0) == 0, "a zero byte in a line");
    expect(parse_exact("1 2 3 4 5 6 7 8\n" + std::string(5000, '7') + "\n", 4, &n, &err) == DMSA_ERR_INVALID && n == 1 && err.rfind("line 2:", 0) == 0, "an over-long line");
    expect(parse_exact(std::string(1024, ' ') + "1 2 3 4 5 6 7 8", 4, &n, &err) == DMSA_OK && n == 1, "blanks do not count towards the line limit");
    expect(parse_exact("1 2 3 4 5 6 7 8", 1, &n, &err, 0) == DMSA_OK && n == 1, "no error buffer");
    expect(parse_exact("x", 1, &n, &err, 1) == DMSA_ERR_INVALID && err.empty(), "an error buffer of one byte");
    for (int a = 1; a < argc; ++a) {
        std::FILE* f = std::fopen(argv[a], "rb");
        if (!f) {
            std::fprintf(stderr, "cannot open %s\n", argv[a]);
            return 2;
        }
        std::string text;
        char chunk[4096];
        for (size_t got; (got = std::fread(chunk, 1, sizeof(chunk), f)) > 0;) text.append(chunk, got);
        std::fclose(f);
        parse_exact(text, 0, &n, &err);
        const int64_t count = n;
        const int rc = parse_exact(text, count, &n, &err);
        std::printf("%s: status %d, %lld poses%s%s\n", argv[a], rc, (long long)n, err.empty() ? "" : ", ", err.c_str());
    }
    std::printf("tum_parse_check: %d failure(s)\n", failures);
    return failures ? 1 : 0;
}
