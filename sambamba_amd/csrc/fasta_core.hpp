// fasta_core.hpp -- the index of a FASTA file (`sambamba index -F`: buildFai, BioD bio/std/file/fai.d:78-101) from chunks of its text
// that are cut anywhere, not at line ends.  Compiled for the device (K17, fasta.hip) and for the host (engine_fasta.cpp; tests/native/
// fasta_host.cpp runs all of it on the CPU).
//
// A chunk is split at its '\n' bytes (K15a gives line_start[0] = 0 and line_start[k] = the byte behind the k-th '\n').  The lines that
// begin AND end inside the chunk -- the INNER lines k = 1 .. n_newlines - 1 -- are the device's: inner_line() says what one is, the
// header lines among them number the SEGMENTS of the chunk (segment 0: the inner lines in front of the first inner header, which belong
// to the sequence that was open when the chunk began), and per segment four numbers come back (FastaSeg).  What crosses a chunk's
// ends is the host's: the HEAD piece [0, first '\n') continues the line the carry holds open, the TAIL piece behind the last '\n'
// opens one.  FastaCarry keeps that line (its kind, its length so far, whether its last byte was '\r', for a header its name so far),
// the open sequence and the counts, and consume() folds a chunk's results into it in file order: head, segment 0, the segments, tail.
// A line may span any number of chunks (an unwrapped chromosome is one line); only the bytes of header lines are looked at on the host.
//
// The terminator is "\r\n" when the first line of the file ends in it, else "\n".  With "\r\n" every '\n' must follow a '\r': then the
// lines and their terminators tile the file, and the running offset of fai.d is the file position behind a line's '\n'.
#pragma once
#include <cstdint>
#include <cstring>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define SBX_FASTA_HD __host__ __device__ __forceinline__
#else
#define SBX_FASTA_HD inline
#endif

#include <string>
#include <vector>

namespace sbx {
namespace fastac {

constexpr uint64_t kNoLine = ~0ull;
constexpr uint64_t kChunkLimit = 1ull << 30;

// what the device hands back per segment (32 bytes)
struct FastaSeg {
    uint64_t seq_bytes;         // bytes of the segment's sequence lines, terminators excluded
    uint64_t first_line;        // (inner line number << 32 | its length) of the first sequence line that is not empty; kNoLine: none
    uint64_t hdr_off;           // segments >= 1: offset of the header line in the chunk ...
    uint64_t hdr_len;           // ... and its length, terminator excluded
};

struct InnerLine {
    uint64_t len;               // without the terminator
    bool header, bare;          // bare: "\r\n" mode and no '\r' in front of the '\n'
};
// the line text[a, e), text[e] being its '\n'
SBX_FASTA_HD InnerLine inner_line(const uint8_t* text, uint64_t a, uint64_t e, bool crlf) {
    InnerLine l;
    const uint64_t raw = e - a;
    l.header = raw != 0 && text[a] == '>';
    const bool cr = raw != 0 && text[e - 1] == '\r';
    l.bare = crlf && !cr;
    l.len = crlf && cr ? raw - 1 : raw;
    return l;
}
// (a chunk holds at most kChunkLimit bytes: line numbers and lengths inside it fit 32 bits)
SBX_FASTA_HD uint64_t first_line_key(uint64_t k, uint64_t len) { return len ? (k << 32 | len) : kNoLine; }

// ---- host ----------------------------------------------------------------------------------------------------------------
struct FaiRecord {
    std::string name;
    uint64_t seq_len = 0, offset = 0, line_len = 0;
};

// what the host needs of a chunk besides its bytes
struct ChunkResult {
    uint64_t size = 0, n_newlines = 0;
    uint64_t first_start = 0;           // line_start[1] (n_newlines >= 1)
    uint64_t last_start = 0;            // line_start[n_newlines]
    uint64_t n_bare = 0, first_bare = kNoLine;      // inner lines that end in a bare '\n'; the lowest inner line number among them
    std::vector<FastaSeg> seg;          // n_headers + 1 (n_newlines >= 2; else empty)
};

struct FastaCarry {
    bool crlf = false;
    uint64_t file_pos = 0;              // bytes consumed
    uint64_t n_lines = 0;               // lines closed
    // the open line
    bool open = false, open_header = false, open_last_cr = false, name_done = false;
    uint64_t open_len = 0;
    std::string open_name;
    std::vector<FaiRecord> recs;
    bool seq_before_header = false;
    uint64_t n_bare = 0, first_bare_line = kNoLine;     // 1-based line number

    uint32_t term() const { return crlf ? 2u : 1u; }

    // the bytes of a header line behind its '>' up to the first space
    void name_bytes(const uint8_t* p, uint64_t n) {
        if (name_done || !n) return;
        const void* sp = memchr(p, ' ', (size_t)n);
        const uint64_t k = sp ? (uint64_t)((const uint8_t*)sp - p) : n;
        open_name.append((const char*)p, (size_t)k);
        name_done = sp != nullptr;
    }
    void append_open(const uint8_t* p, uint64_t n) {
        if (!n) return;
        uint64_t skip = 0;
        if (!open) { open = true; open_header = p[0] == '>'; skip = 1; }
        if (open_header) name_bytes(p + skip, n - skip);
        open_len += n;
        open_last_cr = p[n - 1] == '\r';
    }
    void add_sequence(uint64_t bytes, uint64_t first_len) {
        if (recs.empty()) { seq_before_header = true; return; }
        FaiRecord& r = recs.back();
        r.seq_len += bytes;
        if (r.line_len == 0) r.line_len = first_len;
    }
    void note_bare(uint64_t line_number) {
        ++n_bare;
        if (line_number < first_bare_line) first_bare_line = line_number;
    }
    // the open line (none: an empty line) ends; terminated: by a '\n' whose successor is byte `behind` of the file
    void close_line(bool terminated, uint64_t behind) {
        ++n_lines;
        const bool cr = terminated && crlf && open && open_last_cr;
        if (terminated && crlf && !cr) note_bare(n_lines);
        const uint64_t len = open_len - (cr ? 1u : 0u);
        if (open && open_header) {
            if (cr && !name_done && !open_name.empty()) open_name.pop_back();      // (the '\r' of the terminator)
            FaiRecord r;
            r.name = open_name;
            r.offset = terminated ? behind : behind + term();
            recs.push_back(r);
        } else {
            add_sequence(len, len);
        }
        open = open_header = open_last_cr = name_done = false;
        open_len = 0;
        open_name.clear();
    }

    // a chunk, in file order
    void consume(const uint8_t* text, const ChunkResult& c) {
        const uint64_t base = file_pos;
        file_pos += c.size;
        if (c.n_newlines == 0) { append_open(text, c.size); return; }
        append_open(text, c.first_start - 1);
        close_line(true, base + c.first_start);
        const uint64_t line0 = n_lines;                 // inner line k is line line0 + k of the file
        if (c.n_newlines >= 2) {
            for (size_t s = 0; s < c.seg.size(); ++s) {
                const FastaSeg& g = c.seg[s];
                if (s) {
                    FaiRecord r;
                    const uint8_t* h = text + g.hdr_off + 1;
                    const uint64_t hn = g.hdr_len - 1;
                    const void* sp = memchr(h, ' ', (size_t)hn);
                    r.name.assign((const char*)h, sp ? (size_t)((const uint8_t*)sp - h) : (size_t)hn);
                    r.offset = base + g.hdr_off + g.hdr_len + term();
                    recs.push_back(r);
                }
                // (segment 0 may hold no line at all; line 1 of the file is always the carry's, so a sequence is open here unless
                // that line was already refused)
                add_sequence(g.seq_bytes, g.first_line == kNoLine ? 0 : g.first_line & 0xFFFFFFFFull);
            }
            n_lines += c.n_newlines - 1;
            if (c.n_bare) {
                n_bare += c.n_bare;
                if (line0 + c.first_bare < first_bare_line) first_bare_line = line0 + c.first_bare;
            }
        }
        append_open(text + c.last_start, c.size - c.last_start);
    }
    void finish() {
        if (open) close_line(false, file_pos);
    }
    bool failed() const { return seq_before_header || n_bare; }
    // the refusal, in the project's manner: what, how many, the first
    std::string complaint(const std::string& path) const {
        if (seq_before_header) return "malformed FASTA text in " + path + ": line 1 does not start with '>' (sequence in front of the first header)";
        return "malformed FASTA text in " + path + ": " + std::to_string(n_bare) + (n_bare == 1 ? " line ends" : " lines end") +
               " in '\\n' without '\\r' though the first line ends in \"\\r\\n\", the first is line " + std::to_string(first_bare_line);
    }
    std::string fai_text() const {
        std::string out;
        for (const FaiRecord& r : recs)
            out += r.name + "\t" + std::to_string(r.seq_len) + "\t" + std::to_string(r.offset) + "\t" + std::to_string(r.line_len) + "\t" +
                   std::to_string(r.line_len + term()) + "\n";
        return out;
    }
};

// "\r\n" iff the first '\n' of the file follows a '\r'; feed() the file from its start until it returns true (or the file ends)
struct TerminatorProbe {
    bool crlf = false, last_cr = false;
    bool feed(const uint8_t* p, size_t n) {
        const void* nl = memchr(p, '\n', n);
        if (!nl) { if (n) last_cr = p[n - 1] == '\r'; return false; }
        const size_t k = (size_t)((const uint8_t*)nl - p);
        crlf = k ? p[k - 1] == '\r' : last_cr;
        return true;
    }
};

// What K15a and K17 compute for a chunk, restated serially with the same inner_line / first_line_key (tests/native/fasta_host.cpp;
// the library runs the kernels).
inline ChunkResult chunk_result_serial(const uint8_t* text, uint64_t size, bool crlf) {
    ChunkResult c;
    c.size = size;
    std::vector<uint64_t> line_start{0};
    for (uint64_t i = 0; i < size; ++i) if (text[i] == '\n') line_start.push_back(i + 1);
    c.n_newlines = line_start.size() - 1;
    c.last_start = line_start.back();
    if (c.n_newlines >= 1) c.first_start = line_start[1];
    if (c.n_newlines >= 2) {
        c.seg.push_back(FastaSeg{0, kNoLine, 0, 0});
        for (uint64_t k = 1; k < c.n_newlines; ++k) {
            const uint64_t a = line_start[k], e = line_start[k + 1] - 1;
            const InnerLine l = inner_line(text, a, e, crlf);
            if (l.bare) { ++c.n_bare; if (k < c.first_bare) c.first_bare = k; }
            if (l.header) { c.seg.push_back(FastaSeg{0, kNoLine, a, l.len}); continue; }
            FastaSeg& g = c.seg.back();
            g.seq_bytes += l.len;
            const uint64_t key = first_line_key(k, l.len);
            if (key < g.first_line) g.first_line = key;
        }
    }
    return c;
}

}  // namespace fastac
}  // namespace sbx
