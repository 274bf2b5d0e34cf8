// index_starts.hpp -- what a .bai says about where records start, beyond the chunks of a query: the first record behind a 16 KiB
// window, the first record of the contigs behind a contig, and where the records without a reference start.  sbx_slice_bam
// (engine_slice.cpp) finds its edge records with it, the indexed view (engine_view.cpp) the stretch the region `*` stands for.
#pragma once
#include <map>

#include "engine_ctx.hpp"

namespace sbx {

// ---- what the index says about the first record behind a window -------------------------------------------------------------------
// first position of a bin of the UCSC scheme (levels of 2^29 .. 2^14 positions)
inline uint64_t bin_first_pos(uint32_t id) {
    static const uint32_t first[6] = {0, 1, 9, 73, 585, 4681}, shift[6] = {29, 26, 23, 20, 17, 14};
    for (int l = 5; l >= 0; --l)
        if (id >= first[l]) return (uint64_t)(id - first[l]) << shift[l];
    return 0;
}

struct IndexStarts {
    // per contig: (first position of a bin, lowest chunk start of the bins that begin there or behind), ascending by position
    std::map<uint32_t, std::vector<std::pair<uint64_t, uint64_t>>> bins_behind;
    std::vector<uint64_t> contigs_behind;       // [r]: lowest chunk start of the contigs behind r, or where the records without reference start
    uint64_t v_unmapped = 0;                    // the highest chunk end of the index: the first record without a reference, or the end
    bool any_chunk = false;
};

inline IndexStarts index_starts(const sbx_ctx* c) {
    IndexStarts s;
    const size_t n = c->bai.refs.size();
    std::vector<uint64_t> first(n, ~0ull);
    for (size_t r = 0; r < n; ++r)
        for (const BaiBin& b : c->bai.refs[r].bins) {
            if (b.id > 37448) continue;
            for (const BaiChunk& ch : b.chunks) {
                if (ch.beg >= ch.end) continue;
                first[r] = std::min(first[r], ch.beg);
                s.v_unmapped = std::max(s.v_unmapped, ch.end);
                s.any_chunk = true;
            }
        }
    s.contigs_behind.assign(n + 1, ~0ull);
    for (size_t r = n; r-- > 0;) s.contigs_behind[r] = r + 1 < n ? std::min(s.contigs_behind[r + 1], first[r + 1]) : ~0ull;
    return s;
}

inline const std::vector<std::pair<uint64_t, uint64_t>>& bins_of(const sbx_ctx* c, IndexStarts* s, uint32_t own) {
    auto it = s->bins_behind.find(own);
    if (it != s->bins_behind.end()) return it->second;
    std::vector<std::pair<uint64_t, uint64_t>> v;
    if (own < c->bai.refs.size())
        for (const BaiBin& b : c->bai.refs[own].bins) {
            if (b.id > 37448) continue;
            uint64_t lo = ~0ull;
            for (const BaiChunk& ch : b.chunks) if (ch.beg < ch.end) lo = std::min(lo, ch.beg);
            if (lo != ~0ull) v.push_back({bin_first_pos(b.id), lo});
        }
    std::sort(v.begin(), v.end());
    for (size_t k = v.size(); k-- > 1;) v[k - 1].second = std::min(v[k - 1].second, v[k].second);
    return s->bins_behind[own] = std::move(v);
}

// Stream offset of the first record behind the 16 KiB window of x that lies in no bin containing the window: the first record of a
// bin that begins behind the window, else of a later contig, else the first record without a reference (the end of the stream when
// there is none).
inline uint64_t first_behind_window(const sbx_ctx* c, IndexStarts* s, uint32_t ref_id, uint32_t x, uint64_t u_unmapped) {
    const uint64_t window_end = (((uint64_t)x >> 14) + 1) << 14;
    uint64_t v = ~0ull;
    if (ref_id < c->bai.refs.size()) {
        const auto& bins = bins_of(c, s, ref_id);
        auto it = std::lower_bound(bins.begin(), bins.end(), std::make_pair(window_end, (uint64_t)0));
        if (it != bins.end()) v = it->second;
        v = std::min(v, s->contigs_behind[ref_id]);
    }
    if (v == ~0ull) return u_unmapped;
    uint32_t blk = 0;
    return std::min(voffset_to_stream(c, v, &blk), u_unmapped);
}

// Stream offset of the first record without a reference -- the highest chunk end of the index --, the end of the stream when there
// is none, the first record when the index names no chunk at all.
inline uint64_t unmapped_start(const sbx_ctx* c, const IndexStarts& s) {
    const uint64_t total = c->blocks.out_off.back(), first_rec = std::min<uint64_t>(c->hdr.first_record_off, total);
    if (!s.any_chunk) return first_rec;
    uint32_t blk = 0;
    return std::max(first_rec, voffset_to_stream(c, s.v_unmapped, &blk));
}

}  // namespace sbx
