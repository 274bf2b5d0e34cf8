// engine_worklist.cpp -- from a selection to bytes on the device: the BAI query and its grouping into chain runs (build_runs), the
// per-block tables of a launch (build_worklist), the upload of the file bytes through the pinned staging ring (upload_ranges,
// make_resident, sbx_preload, sbx_prefetch_interval), K1 over the resident work list, and the BAM header at open.
#include <algorithm>
#include <condition_variable>
#include <cstdlib>
#include <thread>

#include "engine_ctx.hpp"

namespace sbx {

// ---- work list ---------------------------------------------------------------------------------------
// virtual offset -> (file block, offset in the inflated stream of the file)
uint64_t voffset_to_stream(const sbx_ctx* c, uint64_t v, uint32_t* blk) {
    const uint32_t nb = (uint32_t)c->blocks.size();
    const uint64_t co = v >> 16, uo = v & 0xFFFF;
    const size_t bi = (size_t)(std::lower_bound(c->blocks.coffset.begin(), c->blocks.coffset.end(), co) - c->blocks.coffset.begin());
    if (bi >= nb) { *blk = nb; return c->blocks.out_off.back(); }     // at / beyond the EOF block
    if (c->blocks.coffset[bi] != co) throw Error(SBX_EFORMAT, "BAI virtual offset does not point at a BGZF block");
    *blk = (uint32_t)bi;
    return c->blocks.out_off[bi] + uo;
}

std::vector<sbx_region> sorted_regions(const std::vector<sbx_region>& sel) {
    std::vector<sbx_region> regs = sel;
    std::sort(regs.begin(), regs.end(), [](const sbx_region& a, const sbx_region& b) {
        if (a.ref_id != b.ref_id) return a.ref_id < b.ref_id;
        if (a.start != b.start) return a.start < b.start;
        return a.end < b.end;
    });
    return regs;
}

// The runs of a pass.  restricted == false: every record of the file.  Otherwise: per contig, the merged BAI chunks
// of its merged regions (getGroupChunks, randomaccessmanager.d:247-294); chunks that share a BGZF block or are at
// most one block apart are joined into one run (what lies between two chunks is a whole number of records, which the
// read selection of K2 drops again), everything else stays a run of its own -- so a sparse BED touches only the
// blocks its chunks live in.
std::vector<FileRun> build_runs(const sbx_ctx* c, const std::vector<sbx_region>& sel, bool restricted) {
    std::vector<FileRun> runs;
    const uint32_t nb = (uint32_t)c->blocks.size();
    const uint64_t total = c->blocks.out_off.back(), first = c->hdr.first_record_off;
    if (!restricted) {
        if (first < total) {
            const uint32_t b0 = (uint32_t)(std::upper_bound(c->blocks.out_off.begin(), c->blocks.out_off.end(), first) - c->blocks.out_off.begin()) - 1;
            runs.push_back({b0, nb, first, total});
        }
        return runs;
    }
    const std::vector<sbx_region> regs = sorted_regions(sel);
    for (size_t i = 0; i < regs.size();) {
        size_t j = i;
        std::vector<sbx_region> group;
        while (j < regs.size() && regs[j].ref_id == regs[i].ref_id) {
            if (!group.empty() && group.back().end >= regs[j].start) group.back().end = std::max(group.back().end, regs[j].end);
            else group.push_back(regs[j]);
            ++j;
        }
        // (the index of a file speaks the file's own reference ids)
        int64_t own = regs[i].ref_id;
        if (!c->merged_to_own.empty()) own = regs[i].ref_id < c->merged_to_own.size() ? c->merged_to_own[regs[i].ref_id] : -1;
        for (auto& g : group) g.ref_id = (uint32_t)std::max<int64_t>(own, 0);
        if (own >= 0 && (size_t)own < c->bai.refs.size())
            for (auto& ch : group_chunks(c->bai, group)) {
                if (ch.beg >= ch.end) continue;
                uint32_t bb = 0, be = 0;
                uint64_t ub = voffset_to_stream(c, ch.beg, &bb), ue = voffset_to_stream(c, ch.end, &be);
                ub = std::max(ub, first);
                ue = std::min(ue, total);
                if (ub >= ue || bb >= nb) continue;
                while (bb + 1 < nb && c->blocks.out_off[bb + 1] <= ub) ++bb;      // (a chunk start at the very end of a block)
                const uint32_t b1 = (be < nb && ue > c->blocks.out_off[be]) ? be + 1 : be;
                runs.push_back({bb, std::max(b1, bb + 1), ub, ue});
            }
        i = j;
    }
    std::sort(runs.begin(), runs.end(), [](const FileRun& a, const FileRun& b) { return a.ub != b.ub ? a.ub < b.ub : a.ue < b.ue; });
    std::vector<FileRun> merged;
    for (auto& r : runs) {
        if (!merged.empty() && r.blk0 <= merged.back().blk1 + 1 && r.ub >= merged.back().ub) {
            FileRun& m = merged.back();
            m.ue = std::max(m.ue, r.ue);
            m.blk1 = std::max(m.blk1, r.blk1);
        } else merged.push_back(r);
    }
    return merged;
}

static void build_worklist(const sbx_ctx* c, std::vector<FileRun> runs, bool file_resident, WorkList* w) {
    *w = WorkList();
    w->runs = std::move(runs);
    uint64_t uo = 0, co = 0;
    for (size_t ri = 0; ri < w->runs.size(); ++ri) {
        const FileRun& r = w->runs[ri];
        const uint32_t first_local = (uint32_t)w->file_blk.size();
        const uint64_t cbase = c->blocks.coffset[r.blk0];
        const uint64_t cend = c->blocks.comp_off[r.blk1 - 1] + c->blocks.comp_len[r.blk1 - 1] + 8;     // + CRC32, ISIZE
        if (!file_resident) w->ranges.push_back({cbase, cend - cbase, co});
        for (uint32_t b = r.blk0; b < r.blk1; ++b) {
            w->file_blk.push_back(b);
            w->comp_off.push_back(file_resident ? c->blocks.comp_off[b] : co + (c->blocks.comp_off[b] - cbase));
            w->comp_len.push_back(c->blocks.comp_len[b]);
            w->isize.push_back(c->blocks.isize[b]);
            w->run_of.push_back((uint32_t)ri);
            w->out_off.push_back(uo + (c->blocks.out_off[b] - c->blocks.out_off[r.blk0]));
        }
        const uint64_t ubase = c->blocks.out_off[r.blk0];
        w->chain.push_back({uo + (r.ub - ubase), uo + (r.ue - ubase), first_local, (uint32_t)w->file_blk.size() - 1, r.open_end ? 1u : 0u, 0u});
        uo += c->blocks.out_off[r.blk1] - ubase;
        co += (cend - cbase + 15) & ~15ull;
    }
    w->out_off.push_back(uo);
    w->u_bytes = uo;
    w->comp_bytes = file_resident ? c->file.size : co;
}

// ---- host -> device copies of file bytes: a pool of threads preads 2 MiB pieces into a ring of pinned staging buffers, the
// calling thread sends every buffer that is complete with an asynchronous DMA on the copy stream (two DMAs in flight while the
// other two buffers are being filled).  The page cache -> pinned copy is what bounds the upload (PCIe takes 57 GB/s, one
// thread copies ~3 GB/s), so the pieces are small and claimed in order: all threads work on the oldest incomplete buffer.
static void read_file_piece(const sbx_ctx* c, uint64_t off, size_t n, uint8_t* dst) {
    size_t lo = 0;
    while (lo < n) {
        ssize_t k = pread(c->file.fd, dst + lo, n - lo, (off_t)(off + lo));
        if (k <= 0) { memcpy(dst + lo, c->file.data + off + lo, n - lo); break; }     // (the mapping always works)
        lo += (size_t)k;
    }
}

static unsigned upload_threads() {
    static const unsigned n = [] {
        if (const char* e = getenv("SBX_UPLOAD_THREADS")) return (unsigned)std::max(1, atoi(e));
        return std::min(8u, std::max(1u, std::thread::hardware_concurrency()));      // (4 .. 16 measured: 8 is the best by a little)
    }();
    return n;
}

// copies the ranges into d_comp; the compute stream waits for the last DMA (no host synchronisation here)
static void upload_ranges(sbx_ctx* c, const std::vector<WorkList::Range>& ranges) {
    for (auto& b : c->stage) b.ensure(kStageBytes);
    hipStream_t cs = c->copy_stream.get();
    struct Chunk { uint64_t file_off, dst; size_t n; };
    struct Piece { uint32_t chunk; uint32_t off, n; };
    constexpr size_t kPiece = 2u << 20;
    std::vector<Chunk> chunks;
    std::vector<Piece> pieces;
    for (auto& r : ranges)
        for (uint64_t done = 0; done < r.len;) {
            const size_t n = (size_t)std::min<uint64_t>(kStageBytes, r.len - done);
            for (size_t o = 0; o < n; o += kPiece) pieces.push_back({(uint32_t)chunks.size(), (uint32_t)o, (uint32_t)std::min(kPiece, n - o)});
            chunks.push_back({r.file_off + done, r.dst + done, n});
            done += n;
        }
    if (chunks.size() == 1 && pieces.size() <= 2) {       // a small transfer: no pool
        read_file_piece(c, chunks[0].file_off, chunks[0].n, c->stage[0].p);
        SBX_HIP(hipMemcpyAsync(c->d_comp.p + chunks[0].dst, c->stage[0].p, chunks[0].n, hipMemcpyHostToDevice, cs));
        SBX_HIP(hipEventRecord(c->stage_ev[0].get(), cs));
        SBX_HIP(hipEventSynchronize(c->stage_ev[0].get()));      // (the buffer may be refilled by the next call)
        SBX_HIP(hipEventRecord(c->upload_done.get(), cs));
        return;
    }
    std::mutex mu;
    std::condition_variable cv;
    std::vector<uint32_t> left(chunks.size(), 0);
    for (auto& p : pieces) ++left[p.chunk];
    size_t avail = kStages;                 // chunks [0, avail) may be filled: the buffer of chunk x is free once chunk x - kStages has left it
    std::atomic<size_t> next{0};
    bool abort_all = false;
    auto worker = [&] {
        for (;;) {
            const size_t p = next.fetch_add(1);
            if (p >= pieces.size()) return;
            const Piece& pc = pieces[p];
            {
                std::unique_lock<std::mutex> g(mu);
                cv.wait(g, [&] { return abort_all || pc.chunk < avail; });
                if (abort_all) return;
            }
            read_file_piece(c, chunks[pc.chunk].file_off + pc.off, pc.n, c->stage[pc.chunk % kStages].p + pc.off);
            std::lock_guard<std::mutex> g(mu);
            if (--left[pc.chunk] == 0) cv.notify_all();
        }
    };
    std::vector<std::thread> pool;
    const size_t n_thr = std::min<size_t>(upload_threads(), pieces.size());
    for (size_t t = 0; t < n_thr; ++t) pool.emplace_back(worker);
    struct Stop {       // an error on the way out must not leave the pool waiting
        std::mutex& mu; std::condition_variable& cv; bool& abort_all; std::vector<std::thread>& pool;
        ~Stop() { { std::lock_guard<std::mutex> g(mu); abort_all = true; } cv.notify_all(); for (auto& t : pool) t.join(); }
    } stop{mu, cv, abort_all, pool};
    for (size_t ci = 0; ci < chunks.size(); ++ci) {
        { std::unique_lock<std::mutex> g(mu); cv.wait(g, [&] { return left[ci] == 0; }); }
        const int slot = (int)(ci % kStages);
        SBX_HIP(hipMemcpyAsync(c->d_comp.p + chunks[ci].dst, c->stage[slot].p, chunks[ci].n, hipMemcpyHostToDevice, cs));
        SBX_HIP(hipEventRecord(c->stage_ev[slot].get(), cs));
        if (ci + 2 >= (size_t)kStages) {       // two DMAs stay in flight; the buffer of the one before them is free again
            const size_t j = ci + 2 - kStages;
            SBX_HIP(hipEventSynchronize(c->stage_ev[j % kStages].get()));
            std::lock_guard<std::mutex> g(mu);
            avail = j + kStages + 1;
            cv.notify_all();
        }
    }
    // the buffers must be free when the next call starts to fill them
    for (int i = 0; i < kStages; ++i) SBX_HIP(hipEventSynchronize(c->stage_ev[i].get()));
    SBX_HIP(hipEventRecord(c->upload_done.get(), cs));      // (the callers wait for the copy stream on the host)
}

// makes `runs` the resident work list: per-block tables on the device and (unless the file is preloaded) the payload bytes
void make_resident(sbx_ctx* c, std::vector<FileRun> runs) {
    if (c->wl_resident && c->wl.runs == runs) return;
    c->wl_resident = false;
    build_worklist(c, std::move(runs), c->preloaded, &c->wl);
    const WorkList& w = c->wl;
    const size_t n = w.n_blocks();
    const double t0 = wall_now();
    c->d_comp_off.ensure(n + 1);
    c->d_comp_len.ensure(n + 1);
    c->d_isize.ensure(n + 1);
    c->d_run_of.ensure(n + 1);
    c->d_out_off.ensure(n + 1);
    c->d_runs.ensure(w.chain.size() + 1);
    hipStream_t s = c->stream.get();
    if (n) {
        SBX_HIP(hipMemcpyAsync(c->d_comp_off.p, w.comp_off.data(), n * 8, hipMemcpyHostToDevice, s));
        SBX_HIP(hipMemcpyAsync(c->d_comp_len.p, w.comp_len.data(), n * 4, hipMemcpyHostToDevice, s));
        SBX_HIP(hipMemcpyAsync(c->d_isize.p, w.isize.data(), n * 4, hipMemcpyHostToDevice, s));
        SBX_HIP(hipMemcpyAsync(c->d_run_of.p, w.run_of.data(), n * 4, hipMemcpyHostToDevice, s));
        SBX_HIP(hipMemcpyAsync(c->d_runs.p, w.chain.data(), w.chain.size() * sizeof(ChainRun), hipMemcpyHostToDevice, s));
    }
    SBX_HIP(hipMemcpyAsync(c->d_out_off.p, w.out_off.data(), (n + 1) * 8, hipMemcpyHostToDevice, s));
    if (!c->preloaded) {
        c->d_comp.ensure((size_t)w.comp_bytes + kCompPad);
        upload_ranges(c, w.ranges);
        SBX_HIP(hipStreamSynchronize(c->copy_stream.get()));
        c->upload_ms.store((wall_now() - t0) * 1e3, std::memory_order_relaxed);
    }
    c->wl_resident = true;
}

// Inflate the blocks of the resident work list into d_U.
void inflate_worklist(sbx_ctx* c, hipEvent_t ev_mid) {
    const WorkList& w = c->wl;
    const uint32_t n = (uint32_t)w.n_blocks();
    c->d_U.ensure((size_t)w.u_bytes + 128);
    c->d_status.ensure(n + 1);
    c->d_nent.ensure(n + 1);
    c->d_scratch.ensure(inflate_scratch_bytes(n));
    c->d_lit.ensure(inflate_lit_bytes(w.u_bytes, n));
    c->d_ent.ensure(inflate_ent_words(w.u_bytes, n));
    c->d_tok.ensure(64);
    SBX_HIP(hipMemsetAsync(c->d_tok.p, 0, 64 * 8, c->stream.get()));
    launch_bgzf_inflate(c->d_comp.p, c->d_comp_off.p, c->d_comp_len.p, c->d_isize.p, c->d_out_off.p, c->d_U.p, n, 0, c->d_scratch.p,
                        c->d_lit.p, c->d_ent.p, c->d_nent.p, c->d_status.p, c->stream.get(), ev_mid, c->d_tok.p);
}

// inflates the first k BGZF blocks of the file into host memory (BAM header at open)
static void inflate_prefix(sbx_ctx* c, uint32_t k, std::vector<uint8_t>* host) {
    const BlockTable& bt = c->blocks;
    const uint64_t in_end = bt.comp_off[k - 1] + bt.comp_len[k - 1], out_end = bt.out_off[k];
    DevBuf<uint8_t> d_in(in_end + kCompPad), d_out(out_end + 128), d_scr(inflate_scratch_bytes(k)), d_lit(inflate_lit_bytes(out_end, k));
    DevBuf<uint32_t> d_ent(inflate_ent_words(out_end, k)), d_nent(k), d_clen(k), d_isz(k), d_st(k);
    DevBuf<uint64_t> d_coff(k), d_ooff(k);
    SBX_HIP(hipMemset(d_in.p + in_end, 0, 64));
    SBX_HIP(hipMemcpy(d_in.p, c->file.data, in_end, hipMemcpyHostToDevice));
    SBX_HIP(hipMemcpy(d_coff.p, bt.comp_off.data(), k * 8ull, hipMemcpyHostToDevice));
    SBX_HIP(hipMemcpy(d_ooff.p, bt.out_off.data(), k * 8ull, hipMemcpyHostToDevice));
    SBX_HIP(hipMemcpy(d_clen.p, bt.comp_len.data(), k * 4ull, hipMemcpyHostToDevice));
    SBX_HIP(hipMemcpy(d_isz.p, bt.isize.data(), k * 4ull, hipMemcpyHostToDevice));
    launch_bgzf_inflate(d_in.p, d_coff.p, d_clen.p, d_isz.p, d_ooff.p, d_out.p, k, 0, d_scr.p, d_lit.p, d_ent.p, d_nent.p, d_st.p, c->stream.get());
    std::vector<uint32_t> st(k);
    SBX_HIP(hipStreamSynchronize(c->stream.get()));
    SBX_HIP(hipMemcpy(st.data(), d_st.p, k * 4ull, hipMemcpyDeviceToHost));
    for (uint32_t i = 0; i < k; ++i)
        if (st[i] != 0)
            throw Error(SBX_EFORMAT, "Error inflating BGZF block starting from offset " + std::to_string(bt.coffset[i]) + ": " +
                                         inflate_status_string(st[i]));
    host->resize(out_end);
    SBX_HIP(hipMemcpy(host->data(), d_out.p, out_end, hipMemcpyDeviceToHost));
}

// the first n_bytes of the inflated stream (sbx_slice_bam: the header bytes as the file has them)
std::vector<uint8_t> inflate_stream_prefix(sbx_ctx* c, uint64_t n_bytes) {
    std::vector<uint8_t> host;
    if (!n_bytes) return host;
    if (n_bytes > c->blocks.out_off.back()) throw Error(SBX_EFORMAT, "BAM header is truncated");
    const uint32_t k = (uint32_t)(std::lower_bound(c->blocks.out_off.begin(), c->blocks.out_off.end(), n_bytes) - c->blocks.out_off.begin());
    inflate_prefix(c, k, &host);
    host.resize((size_t)n_bytes);
    return host;
}

void parse_header_on_device(sbx_ctx* c) {
    uint64_t total = c->blocks.out_off.back();
    if (total < 12) throw Error(SBX_EFORMAT, "BAM header is truncated");
    uint32_t nb = (uint32_t)c->blocks.size();
    uint32_t k = std::min<uint32_t>(nb, 4);
    std::vector<uint8_t> host;
    for (;;) {
        inflate_prefix(c, k, &host);
        if (parse_bam_header(host.data(), host.size(), total, &c->hdr)) break;
        if (k == nb) throw Error(SBX_EFORMAT, "BAM header is truncated");
        k = std::min<uint32_t>(nb, k * 4);
    }
}
}  // namespace sbx

extern "C" {

int sbx_preload(sbx_ctx* c) {
    return guarded(c, [&] {
        if (!c) throw Error(SBX_EINVAL, "null context");
        SBX_HIP(hipSetDevice(c->device));
        for (sbx_ctx* m : files_of(c)) {
            if (m->preloaded) continue;
            const double t0 = wall_now();
            m->d_comp.alloc(m->file.size + kCompPad);
            SBX_HIP(hipMemsetAsync(m->d_comp.p + m->file.size, 0, 64, m->copy_stream.get()));
            upload_ranges(m, {{0, m->file.size, 0}});
            SBX_HIP(hipStreamSynchronize(m->copy_stream.get()));
            m->upload_ms.store((wall_now() - t0) * 1e3, std::memory_order_relaxed);
            m->preloaded = true;
            m->wl_resident = false;
        }
    });
}

int sbx_prefetch_interval(sbx_ctx* c, uint32_t ref_id, uint32_t beg, uint32_t end) {
    return guarded(c, [&] {
        if (!c) throw Error(SBX_EINVAL, "null context");
        if (ref_id >= c->hdr.refs.size()) throw Error(SBX_EINVAL, "Invalid reference sequence index");
        if (!(beg < end)) throw Error(SBX_EINVAL, "empty interval");
        if (!c->has_index) throw Error(SBX_ENOINDEX, "All files must be indexed");
        {   // slices of similar size follow: no buffer should have to grow twice
            int cur = devbuf_slack_pct().load(std::memory_order_relaxed);
            while (cur < 8 && !devbuf_slack_pct().compare_exchange_weak(cur, 8, std::memory_order_relaxed)) {}
        }
        std::vector<sbx_region> sel;
        if (c->regions.empty()) sel.push_back({ref_id, beg, end});
        else
            for (auto& g : c->regions)
                if (g.ref_id == ref_id && g.start < end && g.end > beg) sel.push_back({ref_id, std::max(g.start, beg), std::min(g.end, end)});
        for (sbx_ctx* m : files_of(c)) {
            SBX_HIP(hipSetDevice(m->device));
            make_resident(m, build_runs(m, sel, true));
        }
    });
}

}  // extern "C"
