// entry_util.hpp -- the host-only pieces the standalone entry points (sbx_sort_bam, sbx_markdup, sbx_merge_bam, sbx_view_*, ...)
// share and that need neither the HIP runtime nor a context: tests/native/entry_host.cpp compiles them alone.
#pragma once
#include <sys/stat.h>
#include <unistd.h>

#include <cstring>
#include <string>

#include "../../include/sbx_depth.h"

namespace sbx {

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

}  // namespace sbx
