// merge_core.hpp -- the header side of `sambamba merge`: SamHeaderMerger (BioD bio/std/hts/utils/samheadermerger.d:51-301) restated
// over sortc::ParsedHeader.  Host code only (tests/native/merge_host.cpp compiles it with g++).
//
// Input: the header texts of the files, in input order.  Output: the merged header text, the merged reference list, and per input
// three maps -- old reference id -> new reference id, old @RG id -> new id, old @PG id -> new id.
//
//   SO     the first header must say coordinate or queryname, every other header the same (samheadermerger.d:70-79, messages verbatim);
//          queryname is refused with SBX_EUNSUPPORTED: the name orders are not built, as in sbx-sort.
//   @SQ    merge_dictionaries (host_io.hpp): the topological order of "line k comes before line k + 1 of the same file".  When the
//          files contradict one another (a cycle) the reference falls back to all lines sorted by name in byte order (lines 155-160)
//          and then needs a .bai per input; here the records are sorted, so the fallback order is all that is taken from it.  A name
//          keeps the @SQ line of its first appearance; one name with two lengths is an error.
//   @RG,   mergeHeaderLines (lines 185-238): lines with one id and the same fields are one line; a line whose id a DIFFERENT line has
//   @PG    taken becomes id.1, id.2, ... (the first suffix that is free).  The reference walks D associative arrays, so which of two
//          colliding lines keeps the id, and the order of the output, is hash order.  Defined here: inputs in order, lines in order of
//          appearance; the first line to claim an id keeps it; the output is in order of first appearance.
//   @PG    level by level (lines 254-296): first the lines without PP, then the lines whose PP names a line of the level before IN
//          THEIR FILE, their PP rewritten through that file's map before they are merged.  A line whose PP names an id its file does
//          not have (or that sits on a PP cycle) is never reached: it is absent from the merged header and from the map, and the PG
//          tags that name it stay as they are.
//   @CO    concatenated in input order.  @HD is what a fresh SamHeader prints: VN:1.3 (header.d:461-470) and SO:coordinate.
#pragma once
#include <set>
#include <utility>

#include "host_io.hpp"
#include "sort_core.hpp"

namespace sbx {
namespace mergec {

using IdMap = std::vector<std::pair<std::string, std::string>>;      // (old id, new id) of every line that was merged, in line order

struct InputMaps {
    std::vector<int32_t> ref;        // [old reference id] -> id in the merged list
    IdMap rg, pg;
    bool identity() const {
        for (size_t k = 0; k < ref.size(); ++k) if (ref[k] != (int32_t)k) return false;
        for (const IdMap* m : {&rg, &pg}) for (const auto& e : *m) if (e.first != e.second) return false;
        return true;
    }
};

struct MergedHeader {
    std::string text;
    std::vector<RefSeq> refs;
    std::vector<InputMaps> maps;     // one per input
};

// `line` ("@XX\tAA:v\t...") with field `key` set to `value`: replaced where it stands, put first when the line has none
inline std::string with_field(const std::string& line, const char* key, const std::string& value) {
    size_t p = 3;
    while (p < line.size()) {
        size_t e = line.find('\t', p + 1);
        if (e == std::string::npos) e = line.size();
        // the field is [p + 1, e)
        if (e - p >= 4 && line[p + 1] == key[0] && line[p + 2] == key[1] && line[p + 3] == ':')
            return line.substr(0, p + 4) + value + line.substr(e);
        p = e;
    }
    return line.substr(0, 3) + "\t" + key + ":" + value + line.substr(3);
}

namespace detail {

struct Line { size_t file; std::string id, text; };

// mergeHeaderLines over `lines` (in the defined order): `taken` holds the ids of the merged lines so far, `out` the merged lines,
// maps[file] receives (old id, new id).  Lines with the same id and text in this call are one line.
inline void merge_lines(const std::vector<Line>& lines, std::set<std::string>* taken, std::vector<sortc::HeaderLine>* out,
                        std::vector<IdMap>* maps) {
    struct Seen { std::string id, text, new_id; };
    std::vector<Seen> seen;
    for (const Line& l : lines) {
        std::string new_id;
        bool found = false;
        for (const Seen& s : seen)
            if (s.id == l.id && s.text == l.text) { new_id = s.new_id; found = true; break; }
        if (!found) {
            new_id = l.id;
            for (int k = 1; taken->count(new_id); ++k) new_id = l.id + "." + std::to_string(k);
            taken->insert(new_id);
            out->push_back(sortc::HeaderLine{new_id, new_id == l.id ? l.text : with_field(l.text, "ID", new_id)});
            seen.push_back(Seen{l.id, l.text, new_id});
        }
        bool have = false;
        for (const auto& e : (*maps)[l.file]) have = have || e.first == l.id;
        if (!have) (*maps)[l.file].emplace_back(l.id, new_id);
    }
}

inline const std::string* lookup(const IdMap& m, const std::string& id) {
    for (const auto& e : m) if (e.first == id) return &e.second;
    return nullptr;
}

}  // namespace detail

// SBX_OK, or the code of the refusal with its message in *why (SBX_EFORMAT: a header text does not parse; SBX_EINVAL: the sorting
// orders, one name with two lengths; SBX_EUNSUPPORTED: queryname).
inline int merge_headers(const std::vector<std::string>& texts, MergedHeader* out, std::string* why) {
    auto fail = [&](int code, const std::string& m) { if (why) *why = m; return code; };
    const size_t n = texts.size();
    if (!n) return fail(SBX_EINVAL, "no headers to merge");
    std::vector<sortc::ParsedHeader> h(n);
    for (size_t f = 0; f < n; ++f) {
        std::string w;
        if (!sortc::parse_header(texts[f].data(), texts[f].size(), &h[f], &w)) return fail(SBX_EFORMAT, "SAM header of input " + std::to_string(f + 1) + ": " + w);
    }
    const std::string& expected = h[0].sorting_order;
    if (expected != "coordinate" && expected != "queryname") return fail(SBX_EINVAL, "file headers indicate that some files are not sorted");
    for (size_t f = 0; f < n; ++f)
        if (h[f].sorting_order != expected) return fail(SBX_EINVAL, "sorting orders of files don't agree, can't merge");
    if (expected == "queryname") return fail(SBX_EUNSUPPORTED, "the files are sorted by read name: sbx-merge merges by coordinate only");

    *out = MergedHeader();
    out->maps.resize(n);
    sortc::ParsedHeader m;                         // version 1.3, as a fresh SamHeader

    // ---- @SQ ----
    std::vector<std::vector<RefSeq>> dicts(n);
    std::map<std::string, std::string> first_line;
    for (size_t f = 0; f < n; ++f)
        for (const sortc::HeaderLine& l : h[f].sq) {
            RefSeq r;
            r.name = l.id;
            r.length = (int32_t)strtoll(sortc::header_field(l.text, "LN").c_str(), nullptr, 10);
            dicts[f].push_back(r);
            first_line.emplace(l.id, l.text);
        }
    std::vector<const std::vector<RefSeq>*> ptrs;
    for (auto& d : dicts) ptrs.push_back(&d);
    try {
        std::vector<std::vector<int32_t>> maps;
        merge_dictionaries(ptrs, &out->refs, &maps);
        for (size_t f = 0; f < n; ++f) out->maps[f].ref = maps[f];
    } catch (const Error& e) {
        if (e.code != SBX_EUNSUPPORTED) return fail(e.code, e.what());          // one name, two lengths
        // the cycle: every line, sorted by name in byte order
        std::map<std::string, int32_t> by_name;
        for (auto& d : dicts) for (const RefSeq& r : d) by_name.emplace(r.name, r.length);
        std::map<std::string, int32_t> id_of;
        out->refs.clear();
        for (const auto& kv : by_name) {
            id_of[kv.first] = (int32_t)out->refs.size();
            RefSeq r;
            r.name = kv.first;
            r.length = kv.second;
            out->refs.push_back(r);
        }
        for (size_t f = 0; f < n; ++f) {
            out->maps[f].ref.clear();
            for (const RefSeq& r : dicts[f]) out->maps[f].ref.push_back(id_of[r.name]);
        }
    }
    for (const RefSeq& r : out->refs) m.sq.push_back(sortc::HeaderLine{r.name, first_line[r.name]});

    // ---- @RG ----
    {
        std::vector<detail::Line> lines;
        for (size_t f = 0; f < n; ++f) for (const sortc::HeaderLine& l : h[f].rg) lines.push_back(detail::Line{f, l.id, l.text});
        std::set<std::string> taken;
        std::vector<IdMap> maps(n);
        detail::merge_lines(lines, &taken, &m.rg, &maps);
        for (size_t f = 0; f < n; ++f) out->maps[f].rg = maps[f];
    }

    // ---- @PG, level by level ----
    {
        struct Pg { size_t file; std::string id, pp, text; bool done; };
        std::vector<Pg> all;
        for (size_t f = 0; f < n; ++f)
            for (const sortc::HeaderLine& l : h[f].pg) all.push_back(Pg{f, l.id, sortc::header_field(l.text, "PP"), l.text, false});
        std::set<std::string> taken;
        std::vector<IdMap> maps(n);
        std::vector<size_t> level;
        for (size_t k = 0; k < all.size(); ++k) if (all[k].pp.empty()) level.push_back(k);
        while (!level.empty()) {
            std::vector<detail::Line> lines;
            for (size_t k : level) {
                Pg& p = all[k];
                p.done = true;
                std::string text = p.text;
                if (!p.pp.empty())
                    if (const std::string* np = detail::lookup(maps[p.file], p.pp)) if (*np != p.pp) text = with_field(text, "PP", *np);
                lines.push_back(detail::Line{p.file, p.id, text});
            }
            detail::merge_lines(lines, &taken, &m.pg, &maps);
            // the children of this level: PP names one of its lines in the same file
            std::vector<size_t> next;
            for (size_t k = 0; k < all.size(); ++k) {
                if (all[k].done || all[k].pp.empty()) continue;
                for (size_t j : level)
                    if (all[j].file == all[k].file && all[j].id == all[k].pp) { next.push_back(k); break; }
            }
            level.swap(next);
        }
        for (size_t f = 0; f < n; ++f) out->maps[f].pg = maps[f];
    }

    for (size_t f = 0; f < n; ++f) m.comments.insert(m.comments.end(), h[f].comments.begin(), h[f].comments.end());
    out->text = sortc::serialise_header(m, "coordinate");
    return SBX_OK;
}

}  // namespace mergec
}  // namespace sbx
