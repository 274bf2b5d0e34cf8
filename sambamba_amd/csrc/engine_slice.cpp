// engine_slice.cpp -- sbx_slice_bam: `sambamba slice` (sambamba/slice.d), the indexed copy of regions that reuses the BGZF blocks of
// the input.  Per region (r, beg, end) the output holds the records of R1 (they start in front of beg and reach it) and the stretch
// [a, b) of the inflated stream from the first record at or behind beg to the first at or behind end (slice_core.hpp).
//
// Edge runs.  Only the surroundings of the two edge positions are read.  The point queries (r, beg, beg + 1) and (r, end, end + 1) of
// all regions of the call go through build_runs together: the chunks of the bins that contain the position, cut by the linear index.
// Every record that covers the position lies in them (its bin contains the position, however far in front it starts), and so does the
// first record at or behind it when that record starts in the position's 16 KiB window.  When no record starts in the rest of the
// window, the first one at or behind x is the first record of a bin that begins behind the window, of a later contig, or the first
// record without a reference: the lowest chunk start among those bins -- read from the index on the host -- names it exactly, and
// the one block it points into is added as a run of its own, so that head and tail can be cut out of it.  K1 and K2 run once over
// all of these; K18 (slice.hip) finds R1 and the candidates for a and b among the described records.
//
// Splice writer.  The output is a sequence of segments: BGZF streams compressed on the device -- the header, then per region its R1
// records, the head [a, next block start) and the tail [start of b's block, b), gathered by K9c from the inflated edge runs -- and
// between head and tail the blocks that lie wholly inside [a, b), written from the file as they are.  One BgzfPieceCompressor serves
// every compressed segment of the call (SBX_BGZF_PIECE_BLOCKS honoured); each segment is a launch sequence of its own, and the host
// copies a file range only after the segment in front of it has arrived: neither batching the segments of many regions into one
// deflate launch nor overlapping the copy with the device is built.
#include "engine_store.hpp"
#include "index_starts.hpp"
#include "slice.hpp"
#include "slice_core.hpp"

namespace {

constexpr uint32_t kMaxPos = 0x7FFFFFFFu;        // no record starts behind it: an edge position beyond counts as this one

struct SliceRegions {
    std::vector<sbx_region> list;
    bool unmapped = false;          // "*" alone
};

SliceRegions resolve_regions(const sbx_ctx* c, const char* const* regions, size_t n_regions, const char* bed_path) {
    SliceRegions out;
    const bool have_bed = bed_path && *bed_path;
    if (have_bed && n_regions) throw Error(SBX_EINVAL, "specifying both region and BED filename is disallowed");      // slice.d:321-323
    if (!have_bed && !n_regions) throw Error(SBX_EINVAL, "Must provide either a bed file or list of regions.");       // slice.d:316-318
    if (n_regions && !regions) throw Error(SBX_EINVAL, "null argument");
    if (n_regions > SBX_VIEW_MAX_REGIONS)
        throw Error(SBX_EINVAL, "too many regions (" + std::to_string(n_regions) + "): at most " + std::to_string(SBX_VIEW_MAX_REGIONS) +
                                    " may be listed; use -L with a BED file");
    if (have_bed) {
        std::vector<BedInterval> ivs;
        std::vector<std::string> lines;
        if (!read_bed_file(bed_path, &ivs, &lines)) throw Error(SBX_EIO, std::string("cannot read the BED file ") + bed_path);
        out.list = bed_merged(ivs, c->hdr);
        return out;
    }
    for (size_t k = 0; k < n_regions; ++k) {
        if (!regions[k]) throw Error(SBX_EINVAL, "null argument");
        const std::string arg = regions[k];
        if (arg == "*") {
            if (n_regions != 1) throw Error(SBX_EINVAL, "the region * cannot be combined with other regions");
            out.unmapped = true;
            return out;
        }
        const RegionString rs = parse_region_string(arg);
        const int id = c->hdr.find_ref(rs.reference);
        if (id < 0) throw Error(SBX_EINVAL, "Reference with name " + rs.reference + " does not exist");
        sbx_region g{(uint32_t)id, rs.beg, rs.end};
        if (g.end == 0xFFFFFFFFu) g.end = (uint32_t)c->hdr.refs[(size_t)id].length;
        if (!(g.start < g.end)) throw Error(SBX_EINVAL, "region " + arg + " is empty");
        out.list.push_back(g);
    }
    return out;
}

void print_timing(const sbx_slice_stats& st) {
    if (!getenv("SBX_TIMING")) return;
    fprintf(stderr, "[sbx] slice: n_regions=%llu records_r1=%llu blocks_inflated=%llu blocks_copied=%llu bytes_copied=%llu stream_bytes=%llu "
                    "compressed_bytes=%llu ms_read=%.2f ms_select=%.3f ms_write=%.2f ms_total_wall=%.1f\n",
            (unsigned long long)st.n_regions, (unsigned long long)st.records_r1, (unsigned long long)st.blocks_inflated,
            (unsigned long long)st.blocks_copied, (unsigned long long)st.bytes_copied, (unsigned long long)st.stream_bytes,
            (unsigned long long)st.compressed_bytes, st.ms_read, st.ms_select, st.ms_write, st.ms_total_wall);
}

}  // namespace

extern "C" {

int sbx_slice_bam(const char* in_path, const char* out_path, const char* const* regions, size_t n_regions, const char* bed_path, int device,
                  sbx_slice_stats* stats, char* err, size_t errlen) {
    const bool to_stdout = !out_path || !strcmp(out_path, "-");
    const char* const path = to_stdout ? "/dev/stdout" : out_path;
    return run_entry(err, errlen, [&] {
        if (!in_path) throw Error(SBX_EINVAL, "null argument");
        if (!to_stdout) refuse_overwrite(in_path, path);
        const double w0 = wall_now();
        Standalone c = open_record_pass(in_path, device, nullptr, true);
        if (!c->has_index) throw Error(SBX_ENOINDEX, std::string("the input has no index: ") + in_path + ".bai is needed");
        OutputGuard out_file(path, to_stdout);
        const SliceRegions sel = resolve_regions(c.get(), regions, n_regions, bed_path);
        const BlockTable& bt = c->blocks;
        const uint32_t nbk = (uint32_t)bt.size();
        const uint64_t total = bt.out_off.back(), first_rec = std::min<uint64_t>(c->hdr.first_record_off, total);
        hipStream_t s = c->stream.get();
        sbx_slice_stats st{};
        st.n_regions = sel.unmapped ? 1 : sel.list.size();

        // ---- the index: where the records without a reference start; per edge the first record behind its window ----
        IndexStarts starts = index_starts(c.get());
        const uint64_t u_unmapped = unmapped_start(c.get(), starts);
        const size_t n = sel.list.size();
        auto own_ref = [&](uint32_t r) { return r; };       // (one file: the index speaks the ids of the header)
        std::vector<SliceEdge> edges;
        std::vector<SliceBeg> begs;
        for (size_t g = 0; g < n; ++g) {
            const sbx_region& q = sel.list[g];
            edges.push_back({own_ref(q.ref_id), std::min(q.start, kMaxPos)});
            edges.push_back({own_ref(q.ref_id), std::min(q.end, kMaxPos)});
            begs.push_back({q.ref_id, std::min(q.start, kMaxPos), (uint32_t)g, 0u});
        }
        auto edge_less = [](const SliceEdge& a, const SliceEdge& b) { return a.ref_id != b.ref_id ? a.ref_id < b.ref_id : a.x < b.x; };
        std::sort(edges.begin(), edges.end(), edge_less);
        edges.erase(std::unique(edges.begin(), edges.end(), [](const SliceEdge& a, const SliceEdge& b) { return a.ref_id == b.ref_id && a.x == b.x; }),
                    edges.end());
        std::stable_sort(begs.begin(), begs.end(), [](const SliceBeg& a, const SliceBeg& b) { return a.ref_id != b.ref_id ? a.ref_id < b.ref_id : a.beg < b.beg; });
        std::vector<uint64_t> behind(edges.size());         // per edge: first_behind_window
        for (size_t k = 0; k < edges.size(); ++k) behind[k] = first_behind_window(c.get(), &starts, edges[k].ref_id, edges[k].x, u_unmapped);

        // ---- the edge runs ----
        std::vector<FileRun> runs;
        {
            std::vector<sbx_region> points;
            for (const SliceEdge& e : edges) points.push_back({e.ref_id, e.x, e.x + 1u});
            if (!points.empty()) runs = build_runs(c.get(), points, true);
        }
        auto touch = [&](uint64_t u) {          // the block a record boundary lies inside of, from that record on
            if (u >= total || u < first_rec) return;
            const uint32_t b = slicec::block_of(bt.out_off.data(), nbk, u);
            if (bt.out_off[b] == u) return;     // (a block start: neither a head nor a tail is cut there)
            const bool last = b + 1 >= nbk || bt.out_off[b + 1] >= total;
            runs.push_back(FileRun{b, b + 1, u, last ? total : bt.out_off[b + 1], !last});
        };
        for (uint64_t u : behind) touch(u);
        if (sel.unmapped) touch(u_unmapped);
        runs = join_runs(std::move(runs));

        // ---- K1, K2 over all of them; K18 ----
        uint64_t nrec = 0;
        if (!runs.empty()) {
            run_impl(c.get(), {}, false, &runs);
            nrec = c->primary_records;
            st.blocks_inflated = c->wl.n_blocks();
            st.ms_read = c->stats.ms_inflate + c->stats.ms_index;
        }
        const WorkList& wl = c->wl;
        const uint32_t groups = slice_groups(nrec);
        DevBuf<SliceEdge> d_edges(edges.size() + 1);
        DevBuf<SliceBeg> d_begs(begs.size() + 1);
        DevBuf<unsigned long long> d_edge_min(edges.size() + 1), d_region_bytes(n + 1), d_acc(kSliceAccWords);
        DevBuf<uint32_t> d_region_count(n + 1), d_count((size_t)nrec + 2), d_group_entries(groups + 4);
        DevBuf<uint64_t> d_group_base(groups + 4);
        if (!edges.empty()) SBX_HIP(hipMemcpyAsync(d_edges.p, edges.data(), edges.size() * sizeof(SliceEdge), hipMemcpyHostToDevice, s));
        if (!begs.empty()) SBX_HIP(hipMemcpyAsync(d_begs.p, begs.data(), begs.size() * sizeof(SliceBeg), hipMemcpyHostToDevice, s));
        SBX_HIP(hipMemsetAsync(d_edge_min.p, 0xFF, d_edge_min.bytes(), s));
        SBX_HIP(hipMemsetAsync(d_region_bytes.p, 0, d_region_bytes.bytes(), s));
        SBX_HIP(hipMemsetAsync(d_region_count.p, 0, d_region_count.bytes(), s));
        SBX_HIP(hipMemsetAsync(d_acc.p, 0, d_acc.bytes(), s));
        SliceSelectArgs a{};
        a.U = c->U(); a.desc = c->d_desc.p; a.rec_ref = c->d_rec_ref.p; a.n = nrec; a.u_end = runs.empty() ? 0 : wl.u_bytes;
        a.edges = d_edges.p; a.n_edges = (uint32_t)edges.size(); a.begs = d_begs.p; a.n_begs = (uint32_t)begs.size();
        a.edge_min = d_edge_min.p; a.region_count = d_region_count.p; a.region_bytes = d_region_bytes.p;
        a.count = d_count.p; a.group_entries = d_group_entries.p; a.acc = d_acc.p;
        EventTimer t_a, t_b;
        t_a.start(s);
        launch_slice_select(a, s);
        if (nrec) launch_count_scan(d_group_entries.p, groups, d_group_base.p, s);
        t_a.stop(s);
        unsigned long long acc[kSliceAccWords] = {0};
        std::vector<unsigned long long> edge_min(edges.size(), ~0ull), region_bytes(n, 0);
        std::vector<uint32_t> region_count(n, 0);
        SBX_HIP(hipMemcpyAsync(acc, d_acc.p, sizeof acc, hipMemcpyDeviceToHost, s));
        if (!edges.empty()) SBX_HIP(hipMemcpyAsync(edge_min.data(), d_edge_min.p, edges.size() * 8, hipMemcpyDeviceToHost, s));
        if (n) {
            SBX_HIP(hipMemcpyAsync(region_bytes.data(), d_region_bytes.p, n * 8, hipMemcpyDeviceToHost, s));
            SBX_HIP(hipMemcpyAsync(region_count.data(), d_region_count.p, n * 4, hipMemcpyDeviceToHost, s));
        }
        SBX_HIP(hipStreamSynchronize(s));
        if (nrec) st.ms_select += t_a.ms();
        if (acc[kSliceAccBad]) throw Error(SBX_EFORMAT, malformed_records_message(acc[kSliceAccBad]));
        const uint64_t n_r1 = acc[kSliceAccEntries];
        if (n_r1 + 2 * (uint64_t)n + 2 > 0xFFFFFFF0ull) throw Error(SBX_EUNSUPPORTED, "more than 2^32 records in front of the regions (R1)");
        st.records_r1 = n_r1;

        // ---- the entries: R1 records from K18b, then head and tail of every region from the splice arithmetic ----
        const uint64_t n_ent = n_r1 + 2 * (uint64_t)(sel.unmapped ? 1 : n);
        DevBuf<uint64_t> d_key((size_t)n_ent + 2), d_off((size_t)n_ent + 2), d_out_off((size_t)n_ent + 2);
        DevBuf<uint32_t> d_len((size_t)n_ent + 2);
        if (n_r1) {
            SliceEmitArgs b{};
            b.s = a; b.group_entry_base = d_group_base.p; b.key = d_key.p; b.off = d_off.p; b.len = d_len.p;
            t_b.start(s);
            launch_slice_emit(b, s);
            t_b.stop(s);
        }
        // work-list offset <-> offset of the file's inflated stream (the blocks of the work list ascend in the file)
        auto to_file = [&](uint64_t w) {
            const size_t i = (size_t)(std::upper_bound(wl.out_off.begin(), wl.out_off.end(), w) - wl.out_off.begin()) - 1;
            return bt.out_off[wl.file_blk[i]] + (w - wl.out_off[i]);
        };
        auto to_worklist = [&](uint64_t u) -> uint64_t {
            const uint32_t b = slicec::block_of(bt.out_off.data(), nbk, u);
            const auto it = std::lower_bound(wl.file_blk.begin(), wl.file_blk.end(), b);
            if (runs.empty() || it == wl.file_blk.end() || *it != b)
                throw Error(SBX_EFORMAT, "internal error: the block of an edge of a region was not read (a .bai that does not belong to the file?)");
            return wl.out_off[(size_t)(it - wl.file_blk.begin())] + (u - bt.out_off[b]);
        };
        // first_ge per edge: the suffix minimum of K18a's candidates over the edges of a contig, and what the index says
        std::vector<uint64_t> first_ge(edges.size());
        for (size_t k = edges.size(); k-- > 0;) {
            uint64_t m = edge_min[k] == ~0ull ? ~0ull : to_file(edge_min[k]);
            if (k + 1 < edges.size() && edges[k + 1].ref_id == edges[k].ref_id) m = std::min(m, first_ge[k + 1]);
            first_ge[k] = m;
        }
        for (size_t k = 0; k < edges.size(); ++k) first_ge[k] = std::min(first_ge[k], behind[k]);
        auto edge_value = [&](uint32_t ref_id, uint32_t x) {
            const SliceEdge e{ref_id, std::min(x, kMaxPos)};
            return first_ge[(size_t)(std::lower_bound(edges.begin(), edges.end(), e, edge_less) - edges.begin())];
        };
        struct Segment { slicec::Splice sp; uint64_t r1_count, r1_bytes; };
        std::vector<Segment> segs;
        if (sel.unmapped) segs.push_back({slicec::splice(u_unmapped, total, bt.out_off.data(), nbk), 0, 0});
        for (size_t g = 0; g < n; ++g) {
            const uint64_t ua = edge_value(sel.list[g].ref_id, sel.list[g].start), ub = edge_value(sel.list[g].ref_id, sel.list[g].end);
            if (ua > ub) throw Error(SBX_ENOTSORTED, "the records around a region are not in coordinate order");
            segs.push_back({slicec::splice(ua, ub, bt.out_off.data(), nbk), region_count[g], region_bytes[g]});
        }
        std::vector<uint64_t> h_key(2 * segs.size()), h_off(2 * segs.size());
        std::vector<uint32_t> h_len(2 * segs.size());
        for (size_t g = 0; g < segs.size(); ++g) {
            const slicec::Splice& sp = segs[g].sp;
            h_key[2 * g] = 4ull * g + 1; h_key[2 * g + 1] = 4ull * g + 2;
            h_len[2 * g] = (uint32_t)(sp.head_end - sp.head_beg); h_len[2 * g + 1] = (uint32_t)(sp.tail_end - sp.tail_beg);
            h_off[2 * g] = h_len[2 * g] ? to_worklist(sp.head_beg) : 0;
            h_off[2 * g + 1] = h_len[2 * g + 1] ? to_worklist(sp.tail_beg) : 0;
        }
        if (!segs.empty()) {
            SBX_HIP(hipMemcpyAsync(d_key.p + n_r1, h_key.data(), h_key.size() * 8, hipMemcpyHostToDevice, s));
            SBX_HIP(hipMemcpyAsync(d_off.p + n_r1, h_off.data(), h_off.size() * 8, hipMemcpyHostToDevice, s));
            SBX_HIP(hipMemcpyAsync(d_len.p + n_r1, h_len.data(), h_len.size() * 4, hipMemcpyHostToDevice, s));
        }
        SBX_HIP(hipStreamSynchronize(s));
        if (n_r1) st.ms_select += t_b.ms();

        // ---- the order of the entries (region, then R1 in file order, head, tail) and their offsets in the compressed segments ----
        const std::vector<uint8_t> header = inflate_stream_prefix(c.get(), first_rec);
        const uint64_t hlen = header.size();
        ResidentOrder order;
        const uint64_t varying = (1ull << sortc::bit_width64(4ull * std::max<size_t>(segs.size(), 1) + 3)) - 1ull;
        sort_resident(d_key.p, n_ent, varying, s, &order);
        uint64_t v_total = hlen;
        {
            DevBuf<uint64_t> d_tile_sum(len_tiles(n_ent) + 2);
            launch_sorted_offsets(d_len.p, order.perm, n_ent, hlen, d_tile_sum.p, d_out_off.p, s);
            if (n_ent) SBX_HIP(hipMemcpyAsync(&v_total, d_out_off.p + n_ent, 8, hipMemcpyDeviceToHost, s));
            SBX_HIP(hipStreamSynchronize(s));
        }
        uint64_t want = hlen;
        for (size_t g = 0; g < segs.size(); ++g) want += segs[g].r1_bytes + h_len[2 * g] + h_len[2 * g + 1];
        if (want != v_total) throw Error(SBX_EFORMAT, "internal error: the offsets of the pieces of the slice do not add up");

        // ---- the splice writer ----
        const double w_write = wall_now();
        OutputFile f(out_file);
        BgzfPieceTimes bt_times;
        // the longest compressed segment sizes the buffers
        uint64_t longest = hlen, cur = hlen;
        for (size_t g = 0; g < segs.size(); ++g) {
            cur += segs[g].r1_bytes + h_len[2 * g];
            if (segs[g].sp.blk1 > segs[g].sp.blk0) { longest = std::max(longest, cur); cur = 0; }
            cur += h_len[2 * g + 1];
        }
        longest = std::max(longest, cur);
        {
            const size_t piece_blocks = bgzf_piece_blocks();
            const uint32_t cap_blocks = (uint32_t)std::min<uint64_t>(piece_blocks, std::max<uint64_t>(1, (longest + kBgzfPayload - 1) / kBgzfPayload));
            BgzfPieceCompressor comp(cap_blocks, -1, true);
            auto compress = [&](uint64_t e0, uint64_t e1, uint64_t v0, uint64_t v1) {        // entries [e0, e1) hold bytes [v0, v1)
                if (v1 <= v0) return;
                comp.run((size_t)(v1 - v0), false, &bt_times,
                         [&](uint8_t* d_in, size_t done, size_t bytes, hipStream_t ps) {
                             const uint64_t p0 = v0 + done, p1 = p0 + bytes;
                             if (p0 < hlen) SBX_HIP(hipMemcpyAsync(d_in, header.data() + p0, std::min<uint64_t>(hlen, p1) - p0, hipMemcpyHostToDevice, ps));
                             launch_gather_records(c->U(), d_off.p, order.perm, d_out_off.p, e0, e1, p0, p1, d_in, ps);
                         },
                         [&](const uint8_t* p, size_t k) { f.write(p, k); });
                st.stream_bytes += v1 - v0;
            };
            uint64_t e0 = 0, v0 = 0, e = 0, v = hlen;
            for (size_t g = 0; g < segs.size(); ++g) {
                const slicec::Splice& sp = segs[g].sp;
                e += segs[g].r1_count + 1;
                v += segs[g].r1_bytes + h_len[2 * g];
                if (sp.blk1 > sp.blk0) {
                    compress(e0, e, v0, v);
                    const uint64_t f0 = bt.coffset[sp.blk0];
                    const uint64_t f1 = sp.blk1 < nbk ? bt.coffset[sp.blk1] : bt.comp_off[nbk - 1] + bt.comp_len[nbk - 1] + 8;
                    constexpr uint64_t kCopy = 8ull << 20;      // (the mapping of the input, written in bounded pieces)
                    for (uint64_t o = f0; o < f1 && f.ok(); o += kCopy) f.write(c->file.data + o, (size_t)std::min<uint64_t>(kCopy, f1 - o));
                    st.blocks_copied += sp.blk1 - sp.blk0;
                    st.bytes_copied += f1 - f0;
                    e0 = e; v0 = v;
                }
                e += 1;
                v += h_len[2 * g + 1];
            }
            compress(e0, e, v0, v);
        }                                                   // (the encoder's buffers are freed inside ms_write)
        f.finish(true);
        out_file.disarm();
        st.compressed_bytes = bt_times.out_bytes;
        st.ms_write = (wall_now() - w_write) * 1e3;
        st.ms_total_wall = (wall_now() - w0) * 1e3;
        print_timing(st);
        if (stats) *stats = st;
    });
}

}  // extern "C"
