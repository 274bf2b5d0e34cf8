// sort_core.hpp -- what `sambamba sort` (coordinate order) needs besides the kernels: the 64-bit sort key of a record, the digits a
// radix sort has to look at, the arithmetic of the pieces the output stream is produced in and of the windows a file larger than the
// device is written in, and the header text of the output.  The key, piece and window functions are `__host__ __device__` (K9a,
// k_piece_bounds, K9c and K9d of sort.hip run the very statements the CPU tests check: tests/native/sort_host.cpp and
// tests/native/sortwin_host.cpp); the header text, plan_windows and the refusals of the windowed writer (engine_windows.hpp), worded
// for sort or for markdup by a WindowWords, are host code.
//
// Order (compareCoordinatesAndStrand, BioD bio/std/hts/bam/read.d:1632-1642, applied by a stable merge sort): ref_id -1 last, ascending
// ref_id, ascending position as a signed number, forward strand in front of reverse strand, ties in file order.  Records with ref_id -1
// compare equal to one another whatever their position and strand say.  All of it is the unsigned order of
//     key = ref_id << 33 | (uint32)(position + 1) << 1 | strand,          key = n_ref << 33 for ref_id == -1
// for every position >= -1 (what the format allows; a position below -1 wraps and sorts behind the others of its contig).
#pragma once
#include <cstddef>
#include <cstdint>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define SBX_SORT_HD __host__ __device__ __forceinline__
#else
#define SBX_SORT_HD inline
#endif

namespace sbx {
namespace sortc {

constexpr uint32_t kStrandBits = 1, kPosBits = 32, kRefShift = kStrandBits + kPosBits;
constexpr uint32_t kDigitBits = 8;        // one pass of the radix sort (K9b)

SBX_SORT_HD uint64_t sort_key(int32_t ref_id, int32_t pos, uint32_t flag, int32_t n_ref) {
    if (ref_id < 0) return (uint64_t)(uint32_t)n_ref << kRefShift;       // all of them compare equal: they keep their file order
    return (uint64_t)(uint32_t)ref_id << kRefShift | (uint64_t)(uint32_t)(pos + 1) << kStrandBits | ((flag >> 4) & 1u);
}

SBX_SORT_HD uint32_t bit_width64(uint64_t v) {
    uint32_t n = 0;
    while (v) { ++n; v >>= 1; }
    return n;
}

// bits of the largest key a file with n_ref references whose records start at or below position max_pos can hold: the strand bit,
// max_pos + 1, and n_ref (the id that stands for -1).  An upper bound from the header alone; the sort itself looks at the keys.
SBX_SORT_HD uint32_t key_bits(int32_t n_ref, int64_t max_pos) {
    if (n_ref > 0) return kRefShift + bit_width64((uint64_t)n_ref);
    const uint64_t p = max_pos < -1 ? 0 : (uint64_t)(max_pos + 1);
    return kStrandBits + bit_width64(p > 0xFFFFFFFFull ? 0xFFFFFFFFull : p);
}

// The passes of the LSD radix sort: `varying` has a bit set where two keys of the file differ (OR of the keys ^ AND of the keys).
// Digits start at the lowest varying bit; a digit none of whose bits vary is skipped.  Returns the number of passes, their shifts
// in shift[] (ascending; room for 8), and through *bits the width of the varying stretch.
SBX_SORT_HD uint32_t plan_passes(uint64_t varying, uint32_t* shift, uint32_t* bits) {
    *bits = 0;
    if (!varying) return 0;
    uint32_t lo = 0;
    while (!((varying >> lo) & 1)) ++lo;
    const uint32_t hi = bit_width64(varying);
    *bits = hi - lo;
    uint32_t n = 0;
    for (uint32_t s = lo; s < hi; s += kDigitBits)
        if ((varying >> s) & ((1u << kDigitBits) - 1)) shift[n++] = s;
    return n;
}

// ---- the pieces of the output stream (engine_store.hpp; k_piece_bounds and K9c, sort.hip) ----
// The stream is header + records; record i holds the bytes [out_off[i], out_off[i + 1]) of it, out_off[n] is its length.  It is
// produced in pieces [k * cap, min((k + 1) * cap, total)).

// the first i in [0, n) with out_off[i + 1] > target, n when there is none: the record that holds byte `target` of the stream, or
// the first record when `target` lies in the header
SBX_SORT_HD uint64_t first_record_ending_behind(const uint64_t* out_off, uint64_t n, uint64_t target) {
    uint64_t lo = 0, hi = n;
    while (lo < hi) {
        const uint64_t mid = (lo + hi) >> 1;
        if (out_off[mid + 1] > target) hi = mid; else lo = mid + 1;
    }
    return lo;
}

// The records a piece has bytes of: bounds[k] = first_record_ending_behind(k * cap), for every k up to and including the one behind
// the last piece.  Piece k takes [r0, r1): from the record that holds its first byte to the one that holds the first byte of the
// next piece -- which starts there, and has nothing in this piece, when the boundary is a record's edge (clip_to_piece says so).
SBX_SORT_HD void piece_records(const uint32_t* bounds, size_t k, uint64_t n, uint64_t* r0, uint64_t* r1) {
    *r0 = bounds[k];
    const uint64_t e = (uint64_t)bounds[k + 1] + 1;
    *r1 = e < n ? e : n;
}

// What the piece [p0, p1) holds of a record at [o, e) of the stream: `len` bytes from byte `src` of the record to byte `dst` of the
// piece; false when it holds none.
struct PieceClip { uint64_t dst, src, len; };
SBX_SORT_HD bool clip_to_piece(uint64_t o, uint64_t e, uint64_t p0, uint64_t p1, PieceClip* c) {
    const uint64_t lo = o > p0 ? o : p0, hi = e < p1 ? e : p1;
    if (lo >= hi) return false;
    c->dst = lo - p0;
    c->src = lo - o;
    c->len = hi - lo;
    return true;
}

// ---- the windows of the output stream (engine_windows.hpp: the windowed sort and the streamed markdup; K9d, sort.hip; K10f, markdup.hip) ----
// A file whose records do not fit the device is written window by window: a window is a run of whole pieces [w0, w1) of the stream
// that fits the device, filled by passing the file through the read pass again and putting every record that has bytes in it at
// dest - w0 (the clip of a record to a window is clip_to_piece).  window_bytes is rounded UP to whole pieces, at least one; the last
// window ends at total; no window is empty.
SBX_SORT_HD uint64_t window_span(uint64_t piece_bytes, uint64_t window_bytes) {
    const uint64_t pieces = window_bytes ? (window_bytes - 1) / piece_bytes + 1 : 1;
    return pieces * piece_bytes;
}
SBX_SORT_HD uint64_t window_count(uint64_t total, uint64_t piece_bytes, uint64_t window_bytes) {
    const uint64_t span = window_span(piece_bytes, window_bytes);
    return total ? (total - 1) / span + 1 : 0;
}
// window k of window_count(): [*w0, *w1)
SBX_SORT_HD void window_at(uint64_t k, uint64_t total, uint64_t piece_bytes, uint64_t window_bytes, uint64_t* w0, uint64_t* w1) {
    const uint64_t span = window_span(piece_bytes, window_bytes);
    *w0 = k * span;
    *w1 = total - *w0 > span ? *w0 + span : total;
}
// Does a batch of the read pass whose records go to [lo, hi) of the stream (K9d-2: the minimum of dest, the maximum of dest + len;
// a batch without records has lo >= hi) hold a byte of the window [w0, w1)?
SBX_SORT_HD bool span_meets_window(uint64_t lo, uint64_t hi, uint64_t w0, uint64_t w1) {
    return lo < hi && lo < w1 && hi > w0;
}

}  // namespace sortc
}  // namespace sbx

// ---- host only ----
#include <cstdlib>
#include <string>
#include <vector>

namespace sbx {
namespace sortc {

// the windows [w0, w1) of a stream of total_stream_bytes, in order (window_count / window_at)
struct Window { uint64_t w0, w1; };
inline std::vector<Window> plan_windows(uint64_t total_stream_bytes, uint64_t piece_bytes, uint64_t window_bytes) {
    std::vector<Window> w((size_t)window_count(total_stream_bytes, piece_bytes, window_bytes));
    for (size_t k = 0; k < w.size(); ++k) window_at(k, total_stream_bytes, piece_bytes, window_bytes, &w[k].w0, &w[k].w1);
    return w;
}

// The windowed writer (engine_windows.hpp) serves three commands; the phrases of its refusals that differ between them:
struct WindowWords {
    const char* task;           // "... does not fit the device: <task> in windows needs ..."
    const char* window_needs;   // what the window itself needs, for that refusal
    const char* doing;          // "the input changed while <doing>"
    const char* stream;         // "bytes [w0, w1) of the <stream>"
    const char* source;         // "record(s) are not the ones <source>"
    const char* what = "the file does";         // "<what> not fit the device"
};
constexpr WindowWords kSortWindowWords{"sorting it", "one window of one piece and the encoder, next to the read batch and 12 bytes per record",
                                       "it was being sorted", "sorted stream", "the keys were taken from"};
constexpr WindowWords kMarkdupWindowWords{"marking its duplicates", "a window of one piece and the encoder, next to the read batch and 17 bytes per record",
                                          "its duplicates were being marked", "output stream", "the key pass read"};

constexpr WindowWords kMergeWindowWords{"merging them", "a window of one piece and the encoder, next to the read batch and 12 bytes per record",
                                        "it was being merged", "merged stream", "the key pass read", "the files do"};

// the SBX_ENOMEM refusal of a file that does not even go through in windows; parts: what the `need` bytes are for
inline std::string windows_do_not_fit(const WindowWords& words, uint64_t need, uint64_t free_bytes, const std::string& parts) {
    return std::string(words.what) + " not fit the device: " + words.task + " in windows needs " + std::to_string(need) +
           " bytes of device memory (" + parts + "), " + std::to_string(free_bytes) + " are free";
}
// the SBX_EIO refusal of a batch that came out of the read pass differently the second time
inline std::string batch_refusal(const WindowWords& words) {
    return std::string("the input changed while ") + words.doing + " (a batch of the read pass holds other records than before)";
}
// The two checks on a window before it is compressed (the accumulator of K9d-3 / K10f): the record bytes written must be the window
// less the header bytes that lie in it (header: [0, hlen) of the stream), and no record may have had another length than the key pass
// saw.  Empty: the window is whole; otherwise the text of the SBX_EIO refusal.
inline std::string window_refusal(uint64_t w0, uint64_t w1, uint64_t hlen, uint64_t bytes_written, uint64_t mismatches, const WindowWords& words = kSortWindowWords) {
    PieceClip h;
    const uint64_t header_bytes = clip_to_piece(0, hlen, w0, w1, &h) ? h.len : 0;
    if (!mismatches && bytes_written == w1 - w0 - header_bytes) return std::string();
    return std::string("the input changed while ") + words.doing + " (bytes [" + std::to_string(w0) + ", " + std::to_string(w1) + ") of the " +
           words.stream + ": " + std::to_string(bytes_written) + " record bytes arrived where " + std::to_string(w1 - w0 - header_bytes) +
           " belong, " + std::to_string(mismatches) + " record(s) are not the ones " + words.source + ")";
}

// A SAM header text as SamHeader's constructor reads it (BioD bio/std/hts/sam/header.d:473-545) and SamHeader.toSam prints it back
// (header.d:626-656): the version and sorting order of an @HD line that is the first line of the input (1.3 and none otherwise);
// the @SQ, @RG and @PG lines in order of first appearance -- a later line with the same SN / ID is dropped -- each with only the
// fields header.d:216-254 declares, in the declared order, empty strings and zero numbers left out; the @CO lines.  Lines shorter
// than three characters are skipped.  Shared by `sort` (below) and `markdup` (markdup_core.hpp).
struct HeaderLine { std::string id, text; };
struct ParsedHeader {
    std::string version = "1.3", sorting_order;      // sorting_order: the SO field as written ("" when there is none)
    std::vector<HeaderLine> sq, rg, pg;
    std::vector<std::string> rg_library;             // LB of every line of rg ("" when absent)
    std::vector<std::string> comments;
};

// value of field `key` of a header line: the last occurrence wins (parse assigns field by field)
inline std::string header_field(const std::string& line, const char* key) {
    std::string v;
    size_t p = 3;
    while (p <= line.size()) {
        size_t e = line.find('\t', p);
        if (e == std::string::npos) e = line.size();
        if (e - p >= 3 && line[p + 2] == ':' && line[p] == key[0] && line[p + 1] == key[1]) v = line.substr(p + 3, e - p - 3);
        p = e + 1;
    }
    return v;
}

// false: a line does not start with '@', is of no known type, or has a number field (LN, PI) that is not a number (the reference throws).
inline bool parse_header(const char* text, size_t n, ParsedHeader* out, std::string* why) {
    struct Decl { const char* prefix; std::vector<const char*> fields; const char* numeric; };
    static const Decl kSq{"@SQ", {"SN", "LN", "AN", "AS", "DS", "M5", "SP", "UR", "AH"}, "LN"};
    static const Decl kRg{"@RG", {"ID", "BC", "CN", "DS", "DT", "FO", "KS", "LB", "PG", "PI", "PL", "PU", "SM", "PM"}, "PI"};
    static const Decl kPg{"@PG", {"ID", "PN", "CL", "PP", "VN"}, ""};
    ParsedHeader& h = *out;
    h = ParsedHeader();
    bool first = true;
    // (a header text may be padded with zero bytes: the text ends at the first one)
    for (size_t k = 0; k < n; ++k) if (!text[k]) { n = k; break; }
    auto fail = [&](const std::string& m) { if (why) *why = m; return false; };
    // 0: malformed number, 1: added, 2: duplicate (the first line stays)
    auto add = [&](std::vector<HeaderLine>& to, const Decl& d, const std::string& line) -> int {
        HeaderLine l;
        l.text = d.prefix;
        for (size_t k = 0; k < d.fields.size(); ++k) {
            std::string v = header_field(line, d.fields[k]);
            const bool numeric = d.fields[k][0] == d.numeric[0] && d.fields[k][1] == d.numeric[1];
            if (numeric && !v.empty()) {
                // to!uint / to!int: digits only (a sign for PI), printed back as a number
                size_t i = (d.numeric[0] == 'P' && (v[0] == '-' || v[0] == '+')) ? 1 : 0;
                if (i == v.size()) return 0;
                for (size_t j = i; j < v.size(); ++j) if (v[j] < '0' || v[j] > '9') return 0;
                const long long x = strtoll(v.c_str(), nullptr, 10);
                v = x == 0 ? std::string() : std::to_string(x);
            }
            if (k == 0) l.id = v;
            if (!v.empty()) { l.text += '\t'; l.text += d.fields[k]; l.text += ':'; l.text += v; }
        }
        for (const HeaderLine& o : to) if (o.id == l.id) return 2;
        to.push_back(l);
        return 1;
    };
    for (size_t p = 0; p <= n;) {
        size_t e = p;
        while (e < n && text[e] != '\n') ++e;
        const std::string line(text + p, e - p);
        p = e + 1;
        if (line.size() < 3) continue;
        if (first && line.compare(0, 3, "@HD") == 0) { h.version = header_field(line, "VN"); h.sorting_order = header_field(line, "SO"); }
        if (line[0] != '@') return fail("Header lines must start with @");
        const std::string ty = line.substr(1, 2);
        int ok = 1;
        if (ty == "SQ") ok = add(h.sq, kSq, line);
        else if (ty == "RG") { ok = add(h.rg, kRg, line); if (ok == 1) h.rg_library.push_back(header_field(line, "LB")); }
        else if (ty == "PG") ok = add(h.pg, kPg, line);
        else if (ty == "HD") {}
        else if (ty == "CO") h.comments.push_back(line.size() > 4 ? line.substr(4) : std::string());
        else return fail("unknown header line type " + line.substr(0, 3));
        if (!ok) return fail("malformed number in header line " + line);
        first = false;
    }
    return true;
}

// toSam with the sorting order `so` ("": no SO field)
inline std::string serialise_header(const ParsedHeader& h, const std::string& so) {
    std::string out = "@HD\tVN:" + h.version + (so.empty() ? std::string() : "\tSO:" + so) + "\n";
    for (const auto* v : {&h.sq, &h.rg, &h.pg})
        for (const HeaderLine& l : *v) { out += l.text; out += '\n'; }
    for (const std::string& c : h.comments) { out += "@CO\t"; out += c; out += '\n'; }
    return out;
}

// The header of the sorted file: the sorting order was set to `so` (sambamba/sort.d:294-298: coordinate, or queryname for the name orders).
inline bool sort_header_text(const char* text, size_t n, std::string* out, std::string* why, const char* so = "coordinate") {
    ParsedHeader h;
    if (!parse_header(text, n, &h, why)) return false;
    *out = serialise_header(h, so);
    return true;
}

}  // namespace sortc
}  // namespace sbx
