// pcd_file_check.cpp — a stand-alone host program around PcdFile (csrc/pcd_file.h), the file behind every PCD writer of the library, meant for a
// sanitizer build:
//
//   c++ -std=c++17 -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=all scripts/pcd_file_check.cpp \
//       dmsa_lidar_slam_amd/csrc/pcd_file.cpp -o /tmp/pcd_file_check && /tmp/pcd_file_check
//
// What the writers do with it, in a directory of its own under $TMPDIR (/tmp): a header, rows from heap blocks of exactly their size, the header
// rewritten, the bytes read back; the three paths that cannot be written (a missing directory, a directory, /dev/full), where the open, the
// write or the close fails with a reason that names the path; discard(), which removes a regular file and leaves /dev/null alone; and the
// calls out of order (close twice, close and write without open, open over an open file).  Needs no device and nothing else of the library.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include <sys/stat.h>
#include <unistd.h>

#include "../dmsa_lidar_slam_amd/csrc/pcd_file.h"

static int failures = 0;

static void expect(bool ok, const char* what) {
    if (!ok) {
        std::fprintf(stderr, "FAILED: %s\n", what);
        ++failures;
    }
}

static bool exists(const std::string& path) {
    struct stat sb;
    return ::stat(path.c_str(), &sb) == 0;
}

static std::string slurp(const std::string& path) {
    std::string out;
    if (std::FILE* f = std::fopen(path.c_str(), "rb")) {
        char buf[4096];
        for (size_t k; (k = std::fread(buf, 1, sizeof(buf), f)) > 0;) out.append(buf, k);
        std::fclose(f);
    }
    return out;
}

static bool names(const PcdFile& f, const std::string& path, const char* what, const char* did) {
    const std::string& w = f.why();
    return w.rfind(std::string(what) + ": ", 0) == 0 && w.find(path) != std::string::npos && w.find(did) != std::string::npos;
}

int main() {
    const char* tmp = std::getenv("TMPDIR");
    std::string dir = std::string(tmp && *tmp ? tmp : "/tmp") + "/pcd_file_check.XXXXXX";
    if (!::mkdtemp(&dir[0])) {
        std::perror("mkdtemp");
        return 2;
    }
    const std::string path = dir + "/cloud.pcd";

    // ---- write, patch the header, compare the bytes ----
    {
        PcdFile f;
        expect(!f.is_open() && f.bytes() == 0 && f.why().empty(), "a fresh object");
        expect(f.open(path.c_str(), "check") && f.is_open() && f.path() == path, "open");
        const char head0[] = "POINTS 0000000000\nDATA binary\n", head1[] = "POINTS 0000000003\nDATA binary\n";
        const size_t hn = sizeof(head0) - 1;
        expect(f.write(head0, hn) && f.bytes() == (int64_t)hn, "the header");
        std::string want(head1, hn);
        for (int chunk = 0; chunk < 3; ++chunk) {  // rows in heap blocks of exactly their size: a read past the end would show
            const size_t bytes = chunk == 2 ? 1 : 12 * 1000 + 7;
            char* rows = static_cast<char*>(std::malloc(bytes));
            for (size_t i = 0; i < bytes; ++i) rows[i] = (char)(i * 31 + chunk);
            expect(f.write(rows, bytes), "rows");
            want.append(rows, bytes);
            std::free(rows);
        }
        expect(f.write(nullptr, 0) && f.bytes() == (int64_t)want.size(), "no bytes; every byte counted");
        expect(f.rewrite_head(head1, hn) && f.bytes() == (int64_t)want.size(), "the header rewritten, not counted");
        expect(f.close() && !f.is_open() && f.close(), "close, and close again");
        expect(slurp(path) == want, "the file's bytes");
        expect(f.bytes() == (int64_t)want.size() && f.path() == path, "count and path outlive the close");
        expect(!f.write("x", 1) && names(f, path, "check", "write to ") && !f.rewrite_head("x", 1) && names(f, path, "check", "patching the header of "), "closed: no write");
        expect(slurp(path) == want, "... and the file is what it was");
        // an object that is opened again starts over; an open over an open file closes the first
        const std::string second = dir + "/second.pcd";
        expect(f.open(second.c_str(), "again") && f.bytes() == 0 && f.write("abc", 3) && f.open(path.c_str(), "again") && f.write("de", 2) && f.close(), "open over an open file");
        expect(slurp(second) == "abc" && slurp(path) == "de" && f.bytes() == 2, "both files");
        // discard: open or closed, the regular file goes
        expect(f.open(second.c_str(), "again") && f.write("abc", 3), "open for discard");
        f.discard();
        expect(!f.is_open() && !exists(second), "discard of an open file");
        f.discard();
        expect(f.close(), "discard twice, then close");
    }
    {
        PcdFile f;  // destroyed while open: closed, the bytes are there
        expect(f.open(path.c_str(), "check") && f.write("left open", 9), "left open");
    }
    expect(slurp(path) == "left open", "the destructor closes");
    {
        PcdFile f;
        expect(f.close() && !f.write("x", 1) && !f.rewrite_head("x", 1), "close, write and rewrite without open");
        f.discard();  // no path: nothing
        expect(exists(path), "discard without open touches nothing");
        expect(f.open(path.c_str(), "check") && f.close(), "open and close");
        f.discard();
        expect(!exists(path), "discard after close removes the file");
    }

    // ---- paths that cannot be written ----
    {
        PcdFile f;
        const std::string missing = dir + "/no/such/dir.pcd";
        expect(!f.open(missing.c_str(), "dense cloud") && !f.is_open() && names(f, missing, "dense cloud", "cannot open "), "a missing directory");
        expect(f.why().find("No such file") != std::string::npos, "... with the reason");
        expect(!f.open(dir.c_str(), "pcd") && names(f, dir, "pcd", "cannot open ") && exists(dir), "a directory");
        expect(f.close(), "nothing to close after a failed open");
        // /dev/full: a write larger than the stream's buffer fails at once, a small one when the buffer is flushed at close
        if (exists("/dev/full")) {
            std::vector<char> big(1 << 20, 'x');
            expect(f.open("/dev/full", "dense normals") && !f.write(big.data(), big.size()) && names(f, "/dev/full", "dense normals", "write to "), "/dev/full: a large write");
            expect(f.why().find("No space") != std::string::npos && f.bytes() == 0, "... with the reason, nothing counted");
            f.discard();
            expect(f.open("/dev/full", "dense normals") && f.write("abc", 3) && !f.close() && names(f, "/dev/full", "dense normals", "closing "), "/dev/full: the close");
            expect(!f.is_open() && f.close(), "... and it is closed all the same");
            f.discard();
            expect(exists("/dev/full"), "/dev/full survives discard");
        }
        expect(f.open("/dev/null", "pcd") && f.write("abc", 3) && f.close(), "/dev/null");
        f.discard();
        expect(f.open("/dev/null", "pcd"), "/dev/null again");
        f.discard();
        expect(exists("/dev/null"), "/dev/null survives discard, open or closed");
    }
    expect(::rmdir(dir.c_str()) == 0, "the directory is empty again");
    std::printf("%s\n", failures ? "FAILED" : "ok");
    return failures ? 1 : 0;
}
