// dense_cloud_text.cpp — the host-only text side of include/dmsa_dense_cloud.h: the parser of Poses.txt (the inverse of dmsa_format_tum_pose)
// and the header of the binary PCD.  No device, no context, no other file of the library: the parser reads files from outside and is
// compiled on its own into a sanitizer build (scripts/tum_parse_check.cpp).
#include "../../include/dmsa_dense_cloud.h"

#include <cerrno>
#include <cstdio>
#include <cstdlib>
#include <cstring>

namespace {

constexpr int kMaxLine = 1024;  // a pose line has some 100 characters

int line_error(char* err, int32_t err_cap, long long line, const char* what) {
    if (err && err_cap > 0) std::snprintf(err, (size_t)err_cap, "line %lld: %s", line, what);
    return DMSA_ERR_INVALID;
}

bool blank(char c) { return c == ' ' || c == '\t' || c == '\r' || c == '\v' || c == '\f'; }

}  // namespace

extern "C" {

int dmsa_parse_tum_poses(const char* text, int64_t bytes, double* stamps, double* pos, double* quat_xyzw, int64_t cap, int64_t* n_out, char* err, int32_t err_cap) {
    if (n_out) *n_out = 0;
    if (err && err_cap > 0) err[0] = 0;
    if (!n_out || bytes < 0 || (bytes > 0 && !text) || cap < 0 || (cap > 0 && (!stamps || !pos || !quat_xyzw))) return DMSA_ERR_INVALID;
    int64_t count = 0;
    long long line_no = 0;
    char buf[kMaxLine + 1];
    for (int64_t at = 0; at < bytes;) {
        int64_t end = at;
        while (end < bytes && text[end] != '\n') ++end;
        ++line_no;
        const char* line = text + at;
        int64_t len = end - at;
        at = end + 1;
        while (len > 0 && blank(line[0])) ++line, --len;
        while (len > 0 && blank(line[len - 1])) --len;
        if (len == 0 || line[0] == '#') continue;
        if (len > kMaxLine) return line_error(err, err_cap, line_no, "longer than 1024 characters");
        if (std::memchr(line, 0, (size_t)len)) return line_error(err, err_cap, line_no, "holds a zero byte");
        std::memcpy(buf, line, (size_t)len);
        buf[len] = 0;
        double v[8];
        char* p = buf;
        for (int k = 0; k < 8; ++k) {
            char* stop = nullptr;
            errno = 0;
            v[k] = std::strtod(p, &stop);
            if (stop == p) return line_error(err, err_cap, line_no, "does not hold eight numbers");
            if (*stop != 0 && !blank(*stop)) return line_error(err, err_cap, line_no, "holds something that is not a number");
            p = stop;
        }
        while (blank(*p)) ++p;
        if (*p != 0) return line_error(err, err_cap, line_no, "holds more than eight numbers");
        if (count < cap) {
            stamps[count] = v[0];
            for (int k = 0; k < 3; ++k) pos[3 * count + k] = v[1 + k];
            for (int k = 0; k < 4; ++k) quat_xyzw[4 * count + k] = v[4 + k];
        }
        *n_out = ++count;
    }
    if (count > cap) {
        if (err && err_cap > 0) std::snprintf(err, (size_t)err_cap, "%lld poses, capacity %lld", (long long)count, (long long)cap);
        return DMSA_ERR_INVALID;
    }
    return DMSA_OK;
}

// the header of a binary PCD of x y z (PCD v0.7 as PCL describes the format; recalled, include/dmsa_dense_cloud.h): width = n, height = 1, the
// identity viewpoint; the two counts twelve digits wide
int dmsa_pcd_header_xyz_binary(int64_t n, char* out, int32_t cap) {
    if (n < 0 || n >= 1000000000000ll || !out || cap < 1) return DMSA_ERR_INVALID;
    const int len = std::snprintf(out, (size_t)cap,
                                  "# .PCD v0.7 - Point Cloud Data file format\nVERSION 0.7\nFIELDS x y z\nSIZE 4 4 4\nTYPE F F F\nCOUNT 1 1 1\nWIDTH %012lld\n"
                                  "HEIGHT 1\nVIEWPOINT 0 0 0 1 0 0 0\nPOINTS %012lld\nDATA binary\n",
                                  (long long)n, (long long)n);
    if (len < 0 || len >= cap) return DMSA_ERR_INVALID;
    return len;
}

}  // extern "C"
