// pcd_file.cpp — csrc/pcd_file.h (checked on its own under the sanitizers: scripts/pcd_file_check.cpp).
#include "pcd_file.h"

#include <cerrno>
#include <cstring>

#include <sys/stat.h>

bool PcdFile::failed(const char* did, const char* tail, bool reason) {
    const int e = errno;
    why_ = what_ + ": " + did + path_ + tail + (reason ? std::string(": ") + std::strerror(e) : std::string());
    return false;
}

bool PcdFile::open(const char* path, const char* what) {
    (void)close();
    path_ = path, what_ = what, bytes_ = 0;
    file_ = std::fopen(path, "wb");
    return file_ || failed("cannot open ", "");
}

bool PcdFile::write(const void* p, size_t bytes) {
    if (!file_ || (bytes > 0 && std::fwrite(p, 1, bytes, file_) != bytes)) return failed("write to ", " failed");
    bytes_ += (int64_t)bytes;
    return true;
}

bool PcdFile::rewrite_head(const void* p, size_t bytes) {
    return (file_ && std::fseek(file_, 0, SEEK_SET) == 0 && std::fwrite(p, 1, bytes, file_) == bytes) || failed("patching the header of ", " failed", false);
}

bool PcdFile::close() {
    std::FILE* f = file_;
    file_ = nullptr;
    return !f || std::fclose(f) == 0 || failed("closing ", " failed");
}

void PcdFile::discard() {
    if (file_) std::fclose(file_), file_ = nullptr;
    struct stat sb;
    if (::stat(path_.c_str(), &sb) == 0 && S_ISREG(sb.st_mode)) std::remove(path_.c_str());
}
