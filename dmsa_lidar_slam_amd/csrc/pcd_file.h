// pcd_file.h — the host file behind every PCD writer of the library (pcd_export.cpp, dense_cloud_api.cpp, dense_store.cpp): opened for
// writing, written front to back with its bytes counted, its first bytes rewritten once (the header of a file whose counts are known at the
// end), closed -- or discarded.  Host only.  Every operation returns false on failure and leaves "<what>: ... <path> ...: <reason>" in why().
#pragma once
#include <cstdint>
#include <cstdio>
#include <string>

class PcdFile {
public:
    PcdFile() = default;
    PcdFile(const PcdFile&) = delete;
    PcdFile& operator=(const PcdFile&) = delete;
    ~PcdFile() { (void)close(); }
    bool open(const char* path, const char* what);   // "wb"; `what` ("pcd", "dense cloud", ...) opens every reason; a file still open is closed first
    bool write(const void* p, size_t bytes);         // appended and counted
    bool rewrite_head(const void* p, size_t bytes);  // over the first bytes of the file; not counted
    bool close();                                    // true where nothing is open
    void discard();  // closes, then removes the path if it names a regular file: what a failed export leaves behind, never /dev/null (why() stays)
    bool is_open() const { return file_ != nullptr; }
    const std::string& path() const { return path_; }
    int64_t bytes() const { return bytes_; }
    const std::string& why() const { return why_; }

private:
    bool failed(const char* did, const char* tail, bool reason = true);
    std::FILE* file_ = nullptr;
    std::string path_, what_, why_;
    int64_t bytes_ = 0;
};
