// entry_util.hpp -- the host-only pieces the standalone entry points (sbx_sort_bam, sbx_markdup, sbx_merge_bam, sbx_view_*, ...)
// share and that need neither the HIP runtime nor a context: the error type, the decimal environment hook, the output guard and
// the output file.  tests/native/entry_host.cpp compiles them alone.
#pragma once
#include <sys/stat.h>
#include <unistd.h>

#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <optional>
#include <stdexcept>
#include <string>

#include "../../include/sbx_depth.h"

namespace sbx {

struct Error : std::runtime_error {
    int code;
    Error(int c, const std::string& m) : std::runtime_error(m), code(c) {}
};

// the empty BGZF block that ends a BAM file
constexpr uint8_t kEofBlock[28] = {0x1f, 0x8b, 0x08, 0x04, 0, 0, 0, 0, 0, 0xff, 0x06, 0, 0x42, 0x43, 0x02, 0, 0x1b, 0, 0x03, 0, 0, 0, 0, 0, 0, 0, 0, 0};

// A hook of the tests and measurements: the decimal number in environment variable `name`.  Nothing when the variable is missing,
// does not start with a digit or goes on behind the number: anything but a plain number counts as unset.
inline std::optional<uint64_t> env_u64(const char* name) {
    const char* e = getenv(name);
    if (!e || *e < '0' || *e > '9') return std::nullopt;
    char* end = nullptr;
    const unsigned long long v = strtoull(e, &end, 10);
    if (*end) return std::nullopt;
    return (uint64_t)v;
}
// the same for a size that has a default: `dflt` when the variable is unset or its number is below `least`
inline uint64_t env_size(const char* name, uint64_t dflt, uint64_t least = 1) {
    const std::optional<uint64_t> v = env_u64(name);
    return v && *v >= least ? *v : dflt;
}

inline bool same_file(const char* a, const char* b) {
    struct stat sa, sb;
    if (stat(a, &sa) != 0 || stat(b, &sb) != 0) return false;
    return sa.st_dev == sb.st_dev && sa.st_ino == sb.st_ino;
}

// A text into the caller's buffer (out, cap), NUL-terminated; *out_len (optional) always receives its length.  Returns `code` --
// for a call that hands out its error message this way -- or, when the text and its NUL do not fit, SBX_ENOMEM unless `code`
// already names an error.
inline int copy_to_caller(const std::string& t, char* out, size_t cap, size_t* out_len, int code = SBX_OK) {
    if (out_len) *out_len = t.size();
    if (!out || t.size() + 1 > cap) return code != SBX_OK ? code : SBX_ENOMEM;
    memcpy(out, t.data(), t.size());
    out[t.size()] = 0;
    return code;
}

// what a command says about n records its kernels refused; in_path (optional): the input that holds them
inline std::string malformed_records_message(unsigned long long n, const char* in_path = nullptr) {
    return std::string("malformed BAM record") + (in_path ? std::string(" in ") + in_path : std::string()) + " (" + std::to_string(n) +
           " records whose reference id is out of range or whose lengths are inconsistent)";
}

// The output file of a command: removed when the command fails after creating it.  arm() once the file exists, disarm() when it is
// complete; the destructor unlinks while armed.  What is written to stdout is never removed.
struct OutputGuard {
    std::string path;
    bool to_stdout, armed = false;
    explicit OutputGuard(const char* p, bool is_stdout = false) : path(p ? p : ""), to_stdout(is_stdout) {}
    OutputGuard(const OutputGuard&) = delete;
    OutputGuard& operator=(const OutputGuard&) = delete;
    ~OutputGuard() { if (armed) unlink(path.c_str()); }
    void arm() { armed = !to_stdout; }
    void disarm() { armed = false; }
    const char* c_str() const { return path.c_str(); }
};

// The file a command writes piece by piece: opened "wb" (SBX_EIO "cannot write <path>"), and `guard`, when there is one, armed as
// soon as the file exists.  write() latches a failure; finish() appends the BGZF EOF block when asked, closes, and throws SBX_EIO
// "error writing <path>" when anything failed.  A file that is not finished (an exception passes by) is closed by the destructor;
// the guard is never disarmed here: the caller does that when nothing can fail any more.
class OutputFile {
    std::string path_;
    FILE* f_;
    bool ok_ = true;

public:
    explicit OutputFile(const std::string& path, OutputGuard* guard = nullptr) : path_(path), f_(fopen(path.c_str(), "wb")) {
        if (!f_) throw Error(SBX_EIO, "cannot write " + path_);
        if (guard) guard->arm();
    }
    explicit OutputFile(OutputGuard& guard) : OutputFile(guard.path, &guard) {}
    OutputFile(const OutputFile&) = delete;
    OutputFile& operator=(const OutputFile&) = delete;
    ~OutputFile() { if (f_) fclose(f_); }
    bool ok() const { return ok_; }
    void write(const void* p, size_t k) { ok_ = ok_ && fwrite(p, 1, k, f_) == k; }
    void finish(bool with_eof_block) {
        if (with_eof_block) write(kEofBlock, sizeof kEofBlock);
        const bool closed = fclose(f_) == 0;
        f_ = nullptr;
        if (!closed || !ok_) throw Error(SBX_EIO, "error writing " + path_);
    }
};

}  // namespace sbx
