// fai_cpu.cpp -- CPU yardstick of `sbx-index -F`: the .fai of a FASTA file from one thread and a memchr loop over
// the file read in 64 MiB pieces, with the semantics of sbx_index_fasta (sbx_depth.h).  Not part of the product: `make fai_cpu`.
//
//   fai_cpu <in.fasta> [out.fai]     prints "fai_cpu: S sequences, L lines, B bytes, W ms" on stderr; the index goes to out.fai or stdout
#include <chrono>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

struct Rec { std::string name; uint64_t seq_len = 0, offset = 0, line_len = 0; };

int main(int argc, char** argv) {
    if (argc < 2 || argc > 3) { fprintf(stderr, "usage: fai_cpu <in.fasta> [out.fai]\n"); return 2; }
    const auto t0 = std::chrono::steady_clock::now();
    FILE* f = fopen(argv[1], "rb");
    if (!f) { fprintf(stderr, "fai_cpu: cannot read %s\n", argv[1]); return 1; }
    std::vector<uint8_t> buf(64u << 20);
    std::vector<Rec> recs;
    bool crlf = false, know_term = false, open = false, header = false, name_done = false, last_cr = false;
    uint64_t open_len = 0, pos = 0, n_lines = 0, n_bare = 0, first_bare = 0;
    std::string name;
    auto piece = [&](const uint8_t* p, size_t n) {          // bytes of the open line
        if (!n) return;
        size_t skip = 0;
        if (!open) { open = true; header = p[0] == '>'; skip = 1; }
        if (header && !name_done && n > skip) {
            const void* sp = memchr(p + skip, ' ', n - skip);
            name.append((const char*)p + skip, sp ? (size_t)((const uint8_t*)sp - p) - skip : n - skip);
            name_done = sp != nullptr;
        }
        open_len += n;
        last_cr = p[n - 1] == '\r';
    };
    auto close = [&](bool terminated, uint64_t behind) -> bool {
        ++n_lines;
        if (!know_term) { crlf = terminated && open && last_cr; know_term = true; }
        const bool cr = terminated && crlf && open && last_cr;
        if (terminated && crlf && !cr && !n_bare++) first_bare = n_lines;
        const uint64_t len = open_len - (cr ? 1 : 0);
        if (open && header) {
            if (cr && !name_done && !name.empty()) name.pop_back();
            Rec r;
            r.name = name;
            r.offset = terminated ? behind : behind + (crlf ? 2 : 1);
            recs.push_back(r);
        } else {
            if (recs.empty()) return false;
            recs.back().seq_len += len;
            if (!recs.back().line_len) recs.back().line_len = len;
        }
        open = header = name_done = last_cr = false;
        open_len = 0;
        name.clear();
        return true;
    };
    bool ok = true;
    for (size_t n; ok && (n = fread(buf.data(), 1, buf.size(), f)) > 0; pos += n) {
        size_t at = 0;
        while (ok) {
            const uint8_t* nl = (const uint8_t*)memchr(buf.data() + at, '\n', n - at);
            if (!nl) { piece(buf.data() + at, n - at); break; }
            const size_t k = (size_t)(nl - buf.data());
            piece(buf.data() + at, k - at);
            ok = close(true, pos + k + 1);
            at = k + 1;
        }
    }
    fclose(f);
    if (ok && open) ok = close(false, pos);
    if (!ok) { fprintf(stderr, "fai_cpu: line 1 does not start with '>'\n"); return 1; }
    if (n_bare) { fprintf(stderr, "fai_cpu: %llu line ends without '\\r', the first is line %llu\n", (unsigned long long)n_bare, (unsigned long long)first_bare); return 1; }
    FILE* out = argc == 3 ? fopen(argv[2], "wb") : stdout;
    if (!out) { fprintf(stderr, "fai_cpu: cannot write %s\n", argv[2]); return 1; }
    for (const Rec& r : recs)
        fprintf(out, "%s\t%llu\t%llu\t%llu\t%llu\n", r.name.c_str(), (unsigned long long)r.seq_len, (unsigned long long)r.offset,
                (unsigned long long)r.line_len, (unsigned long long)(r.line_len + (crlf ? 2 : 1)));
    if (out != stdout) fclose(out);
    const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    fprintf(stderr, "fai_cpu: %zu sequences, %llu lines, %llu bytes, %.1f ms\n", recs.size(), (unsigned long long)n_lines, (unsigned long long)pos, ms);
    return 0;
}
