// dense_compare_text.cpp — the host-only side of include/dmsa_dense_compare.h: the defaults, what D1 asks of the tolerance, D5's summary, the
// header of D7 and the reader of D8.  No device, no context.  The reader takes files from outside: every length it uses is checked against
// the buffer or the file it indexes, every product for overflow (scripts/pcd_read_check.cpp runs it under the sanitizers).
#include "../../include/dmsa_dense_compare.h"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

const char* dense_compare_config_refusal(const dmsa_dense_compare_config* cfg);

// D1, the tolerance and the switch alone: the reason of the first breach, or nullptr
const char* dense_compare_config_refusal(const dmsa_dense_compare_config* cfg) {
    if (!std::isfinite(cfg->tolerance)) return "tolerance is not finite";
    if (!(cfg->tolerance > 0.0f && cfg->tolerance <= cfg->max_distance)) return "tolerance must lie in (0, max_distance]";
    if (cfg->keep != DMSA_COMPARE_KEEP_NEAR && cfg->keep != DMSA_COMPARE_KEEP_FAR) return "keep must be DMSA_COMPARE_KEEP_NEAR or DMSA_COMPARE_KEEP_FAR";
    return nullptr;
}

namespace {

constexpr int kLineCap = 512;   // a header line, its newline and the terminating 0
constexpr int kMaxFields = 256;
constexpr int64_t kMaxCount = 1000000000000ll;  // what twelve digits hold

thread_local std::string g_why;

int refuse(const std::string& why) { return g_why = "pcd read: " + why, DMSA_ERR_INVALID; }

// a decimal count without sign, leading zeros legal, at most kMaxCount - 1
bool parse_count(const std::string& tok, int64_t* out) {
    if (tok.empty() || tok.size() > 32) return false;
    int64_t v = 0;
    for (const char ch : tok) {
        if (ch < '0' || ch > '9') return false;
        v = v * 10 + (ch - '0');
        if (v >= kMaxCount) return false;
    }
    return *out = v, true;
}

std::vector<std::string> words_of(const char* line) {
    std::vector<std::string> w;
    const char* p = line;
    while (*p) {
        while (*p == ' ' || *p == '\t' || *p == '\r' || *p == '\n') ++p;
        const char* b = p;
        while (*p && *p != ' ' && *p != '\t' && *p != '\r' && *p != '\n') ++p;
        if (p > b) w.emplace_back(b, (size_t)(p - b));
    }
    return w;
}

struct PcdLayout {
    int64_t points = 0, stride = 0, data_at = 0;
    int64_t at[3] = {-1, -1, -1};  // the byte offsets of x, y and z in a row
};

// D8: the header of `f` (positioned at its start) into `lay`; the file's length is checked against the rows
int read_layout(std::FILE* f, PcdLayout* lay) {
    std::vector<std::string> fields, sizes, types, counts;
    int64_t width = -1, height = -1, points = -1;
    bool data = false;
    char line[kLineCap];
    while (!data) {
        if (!std::fgets(line, kLineCap, f)) return refuse("the file ends inside the header (no DATA line)");
        const size_t len = std::strlen(line);
        if (len == 0 || line[len - 1] != '\n') {
            if (len + 1 >= (size_t)kLineCap) return refuse("a header line longer than " + std::to_string(kLineCap - 2) + " bytes");
            return refuse("the file ends inside the header (no DATA line)");  // (a last line without its newline, or a 0 byte in the header)
        }
        const std::vector<std::string> w = words_of(line);
        if (w.empty() || w[0][0] == '#') continue;
        const std::vector<std::string> rest(w.begin() + 1, w.end());
        if (w[0] == "VERSION") {
            if (rest.size() != 1 || (rest[0] != "0.7" && rest[0] != ".7")) return refuse("VERSION '" + (rest.empty() ? std::string() : rest[0]) + "' (0.7 is read)");
        } else if (w[0] == "FIELDS") {
            fields = rest;
        } else if (w[0] == "SIZE") {
            sizes = rest;
        } else if (w[0] == "TYPE") {
            types = rest;
        } else if (w[0] == "COUNT") {
            counts = rest;
        } else if (w[0] == "WIDTH" || w[0] == "HEIGHT" || w[0] == "POINTS") {
            int64_t v = 0;
            if (rest.size() != 1 || !parse_count(rest[0], &v)) return refuse(w[0] + " is no count below 10^12");
            (w[0] == "WIDTH" ? width : w[0] == "HEIGHT" ? height : points) = v;
        } else if (w[0] == "VIEWPOINT") {
        } else if (w[0] == "DATA") {
            if (rest.size() != 1 || rest[0] != "binary") return refuse("DATA " + (rest.empty() ? std::string("(nothing)") : rest[0]) + " (binary is read)");
            data = true;
        } else {
            return refuse("the header line '" + w[0].substr(0, 32) + "'");
        }
    }
    const size_t nf = fields.size();
    if (nf == 0) return refuse("no FIELDS line");
    if (nf > (size_t)kMaxFields) return refuse("more than " + std::to_string(kMaxFields) + " fields");
    if (sizes.size() != nf || types.size() != nf || (!counts.empty() && counts.size() != nf)) return refuse("FIELDS, SIZE, TYPE and COUNT differ in length");
    if (width < 0 || height < 0 || points < 0) return refuse("WIDTH, HEIGHT or POINTS is missing");
    int64_t wh = 0;
    if (__builtin_mul_overflow(width, height, &wh) || wh != points) return refuse("WIDTH x HEIGHT is not POINTS");
    int64_t stride = 0;
    for (size_t i = 0; i < nf; ++i) {
        int64_t size = 0, count = 1;
        if (!parse_count(sizes[i], &size) || (size != 1 && size != 2 && size != 4 && size != 8)) return refuse("SIZE " + sizes[i].substr(0, 32) + " of field " + fields[i].substr(0, 32));
        if (!counts.empty() && (!parse_count(counts[i], &count) || count > (1 << 20))) return refuse("COUNT " + counts[i].substr(0, 32) + " of field " + fields[i].substr(0, 32));
        const int axis = fields[i] == "x" ? 0 : fields[i] == "y" ? 1 : fields[i] == "z" ? 2 : -1;
        if (axis >= 0) {
            if (lay->at[axis] >= 0) return refuse("field " + fields[i] + " twice");
            if (size != 4 || types[i] != "F" || count != 1) return refuse("field " + fields[i] + " is not SIZE 4, TYPE F, COUNT 1");
            lay->at[axis] = stride;
        }
        stride += size * count;  // (at most 256 * 8 * 2^20)
    }
    if (stride > (1 << 20)) return refuse("a row of " + std::to_string(stride) + " bytes (at most 2^20 are read)");
    for (int a = 0; a < 3; ++a)
        if (lay->at[a] < 0) return refuse(std::string("no field ") + "xyz"[a]);
    const long here = std::ftell(f);
    if (here < 0 || std::fseek(f, 0, SEEK_END) != 0) return refuse("the file cannot be measured");
    const long end = std::ftell(f);
    int64_t bytes = 0;
    if (end < here || __builtin_mul_overflow(points, stride, &bytes)) return refuse("POINTS x the row's bytes overflows");
    if ((int64_t)end - (int64_t)here < bytes)
        return refuse("a short file: " + std::to_string((int64_t)end - (int64_t)here) + " bytes after the header, " + std::to_string(bytes) + " needed");
    lay->points = points, lay->stride = stride, lay->data_at = here;
    return DMSA_OK;
}

struct File {
    std::FILE* f = nullptr;
    ~File() {
        if (f) std::fclose(f);
    }
};

}  // namespace

extern "C" {

// max_distance and tolerance come from no recorded data: ten voxels and one voxel of the demo's 0.1 m, placeholders for a caller who names none
void dmsa_default_dense_compare_config(dmsa_dense_compare_config* cfg) {
    if (!cfg) return;
    cfg->max_distance = 1.0f, cfg->tolerance = 0.1f, cfg->keep = DMSA_COMPARE_KEEP_NEAR, cfg->pad = 0;
}

// D5 of one direction
int dmsa_dense_compare_summary(int64_t matched, int64_t s1, int64_t s2, int64_t within, int64_t queries, double scale, double* mean_m, double* rms_m,
                               double* fraction_within) {
    if (matched < 0 || s1 < 0 || s2 < 0 || within < 0 || queries < 0 || !std::isfinite(scale) || !(scale > 0.0)) return DMSA_ERR_INVALID;
    double mean = 0.0, rms = 0.0, fraction = 0.0;
    if (matched > 0) {
        mean = (double)s1 / (double)matched;
        mean = mean / scale;
        rms = std::sqrt((double)s2 / (double)matched);
        rms = rms / scale;
    }
    if (queries > 0) fraction = (double)within / (double)queries;
    if (mean_m) *mean_m = mean;
    if (rms_m) *rms_m = rms;
    if (fraction_within) *fraction_within = fraction;
    return DMSA_OK;
}

// decided here (D7): the x y z header with the distance, a float, as its last field; width = n, height = 1, the identity viewpoint, the counts
// twelve digits wide
int dmsa_pcd_header_xyz_distance_binary(int64_t n, int32_t intensity, char* out, int32_t cap) {
    if (n < 0 || n >= kMaxCount || !out || cap < 1) return DMSA_ERR_INVALID;
    const int len = std::snprintf(out, (size_t)cap,
                                  "# .PCD v0.7 - Point Cloud Data file format\nVERSION 0.7\nFIELDS x y z %sdistance\nSIZE 4 4 4 %s4\nTYPE F F F %sF\nCOUNT 1 1 1 %s1\n"
                                  "WIDTH %012lld\nHEIGHT 1\nVIEWPOINT 0 0 0 1 0 0 0\nPOINTS %012lld\nDATA binary\n",
                                  intensity ? "intensity " : "", intensity ? "4 " : "", intensity ? "F " : "", intensity ? "1 " : "", (long long)n, (long long)n);
    if (len < 0 || len >= cap) return DMSA_ERR_INVALID;
    return len;
}

const char* dmsa_pcd_xyz_last_error(void) { return g_why.c_str(); }

int dmsa_pcd_xyz_info(const char* path, int64_t* points) {
    if (points) *points = 0;
    if (!path || !points) return refuse("a null argument");
    File file;
    file.f = std::fopen(path, "rb");
    if (!file.f) return refuse(std::string("cannot open ") + path);
    PcdLayout lay;
    if (const int rc = read_layout(file.f, &lay); rc != DMSA_OK) return rc;
    *points = lay.points;
    return g_why.clear(), DMSA_OK;
}

int dmsa_pcd_xyz_read(const char* path, float* xyz_out, int64_t cap, int64_t* points) {
    if (points) *points = 0;
    if (!path || cap < 0 || (cap > 0 && !xyz_out)) return refuse("a null argument or a negative capacity");
    File file;
    file.f = std::fopen(path, "rb");
    if (!file.f) return refuse(std::string("cannot open ") + path);
    PcdLayout lay;
    if (const int rc = read_layout(file.f, &lay); rc != DMSA_OK) return rc;
    if (points) *points = lay.points;
    if (lay.points > cap) return refuse("room for " + std::to_string(cap) + " rows, the file holds " + std::to_string(lay.points));
    if (std::fseek(file.f, (long)lay.data_at, SEEK_SET) != 0) return refuse("the file cannot be positioned");
    const int64_t chunk_rows = std::max<int64_t>(1, ((int64_t)1 << 20) / lay.stride);  // 1 MiB at a time (12 <= stride <= 2^20)
    std::vector<unsigned char> buf((size_t)(chunk_rows * lay.stride));
    for (int64_t r = 0; r < lay.points; r += chunk_rows) {
        const int64_t m = std::min(chunk_rows, lay.points - r);
        if (std::fread(buf.data(), (size_t)lay.stride, (size_t)m, file.f) != (size_t)m) return refuse("the rows cannot be read");
        for (int64_t i = 0; i < m; ++i)
            for (int a = 0; a < 3; ++a) std::memcpy(xyz_out + 3 * (r + i) + a, buf.data() + i * lay.stride + lay.at[a], 4);
    }
    return g_why.clear(), DMSA_OK;
}

}  // extern "C"
