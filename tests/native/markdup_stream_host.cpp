// markdup_stream_host.cpp -- what the streamed path of sbx_markdup adds to sambamba_amd/csrc/markdup_core.hpp, on the CPU
// (tests/test_markdup_stream_cpu.py): the flag rule K10d, the output plan and K10f share, and the entries of the key store, through
// the very functions the kernels compile.  Every buffer has exactly the size of what it holds, so that the sanitizer build sees a
// read behind a record or an entry.
//   markdup_stream_host flags   -> for flag in [0, 2^16), dup in {0, 1}, remove in {0, 1} (innermost): three bytes on stdout, the
//                                  flag written (little-endian) and 1 / 0 for kept
//   markdup_stream_host keys    lines "hex-of-record rg_at rg_len" on stdin -> "pair_key_len hex-of-entry" per line; the entry is
//                                  built byte by byte with pair_key_byte
//   markdup_stream_host equal   lines "hex-of-entry hex-of-entry" -> 1 / 0 per line (pair_keys_equal)
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../sambamba_amd/csrc/markdup_core.hpp"

static std::vector<uint8_t> unhex(const std::string& s) {
    std::vector<uint8_t> out(s.size() / 2);
    for (size_t k = 0; k < out.size(); ++k) out[k] = (uint8_t)strtoul(s.substr(2 * k, 2).c_str(), nullptr, 16);
    return out;
}

static std::string read_word() {
    std::string w;
    int ch;
    while ((ch = getchar()) != EOF && (ch == ' ' || ch == '\n')) {}
    for (; ch != EOF && ch != ' ' && ch != '\n'; ch = getchar()) w.push_back((char)ch);
    return w;
}

int main(int argc, char** argv) {
    using namespace sbx::mdc;
    if (argc < 2) return 2;
    const std::string mode = argv[1];
    if (mode == "flags") {
        std::vector<uint8_t> out;
        out.reserve(3u << 18);
        for (uint32_t flag = 0; flag < 65536u; ++flag)
            for (int dup = 0; dup < 2; ++dup)
                for (int remove = 0; remove < 2; ++remove) {
                    const uint32_t f = flag_after(flag, dup != 0);
                    out.push_back((uint8_t)f);
                    out.push_back((uint8_t)(f >> 8));
                    out.push_back(kept(f, remove != 0) ? 1 : 0);
                }
        return fwrite(out.data(), 1, out.size(), stdout) == out.size() ? 0 : 1;
    }
    if (mode == "keys") {
        for (;;) {
            const std::string hex = read_word();
            if (hex.empty()) return 0;
            const std::vector<uint8_t> rec = unhex(hex);
            const uint32_t rg_at = (uint32_t)strtoul(read_word().c_str(), nullptr, 10), rg_len = (uint32_t)strtoul(read_word().c_str(), nullptr, 10);
            if (rec.size() < 36) return 2;
            const uint32_t l_name = rec[12], len = pair_key_len(l_name, rg_len);
            std::vector<uint8_t> entry(len);
            for (uint32_t k = 0; k < len; ++k) entry[k] = pair_key_byte(rec.data(), l_name, rg_at, rg_len, k);
            printf("%u ", len);
            for (uint8_t b : entry) printf("%02x", b);
            printf("\n");
        }
    }
    if (mode == "equal") {
        for (;;) {
            const std::string a = read_word();
            if (a.empty()) return 0;
            const std::vector<uint8_t> p = unhex(a), q = unhex(read_word());
            if (p.empty() || q.empty()) return 2;
            printf("%d\n", pair_keys_equal(p.data(), q.data()) ? 1 : 0);
        }
    }
    return 2;
}
