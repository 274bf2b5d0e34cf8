// engine_chunks.hpp -- what the commands that read text share (sbx_import_sam, sbx_index_fasta): the reader thread that fills two
// pinned buffers in turn, and K15a on a chunk that has been uploaded.
#pragma once
#include "cli_common.hpp"
#include "engine_ctx.hpp"
#include "lines.hpp"

namespace sbx {

// one of the two pinned buffers between the reader thread and the device thread
struct ChunkSlot {
    PinnedBuf<uint8_t> text;
    size_t bytes = 0;
    bool full = false, last = false;        // last: the input is used up, this slot holds nothing
};

// The input in chunks: a reader thread (StageSync / StageThreads, cli_common.hpp) calls fill(slot.text) -- the bytes it put there,
// 0 at the end of the input; it may throw -- for the two slots in turn, each as soon as the consumer has released it, so that reading
// chunk k + 1 overlaps the work on chunk k.  The consumer takes the chunks in order with next() and says with release() when it has no
// more use for a slot's bytes.
template <class Fill>
struct ChunkReader {
    ChunkReader(int device, const char* failure, Fill fill) : sync_(failure), threads_(sync_) {
        threads_.start([this, device, fill = std::move(fill)]() mutable {
            try {
                SBX_HIP(hipSetDevice(device));
                for (uint32_t k = 0;; ++k) {
                    ChunkSlot& c = slot_[k & 1u];
                    if (!sync_.wait_for([&] { return !c.full; })) return;
                    const size_t bytes = fill(c.text);
                    sync_.mark([&] { c.bytes = bytes; c.last = bytes == 0; c.full = true; });
                    if (!bytes) return;
                }
            } catch (const Error& e) { sync_.fail(e.what(), e.code); }
            catch (const std::exception& e) { sync_.fail(e.what()); }
        });
    }
    // the next chunk, or null behind the last one; throws what the reader failed with
    ChunkSlot* next() {
        ChunkSlot& c = slot_[taken_++ & 1u];
        if (!sync_.wait_for([&] { return c.full; })) throw Error(sync_.failure_code, sync_.failure);
        if (!c.last) return &c;
        threads_.regular = true;            // (the reader has left its loop)
        return nullptr;
    }
    void release(ChunkSlot* c) { sync_.mark([&] { c->full = false; }); }

private:
    ChunkSlot slot_[2];
    StageSync sync_;
    StageThreads threads_;                  // (declared last: joined before the slots and the sync go)
    uint32_t taken_ = 0;
};

// K15a on the chunk t, whose upload is queued on s: d_tile receives the tile bases (text_tiles + 1 words), d_line_start the line starts,
// and the number of '\n' bytes is returned.  uploaded() is called as soon as the upload is known to be done.  `timer` covers the launches.
template <class Uploaded>
uint64_t index_lines(const TextChunk& t, DevBuf<uint64_t>& d_tile, DevBuf<uint64_t>& d_line_start, EventTimer& timer, hipStream_t s,
                     Uploaded&& uploaded) {
    const uint32_t tiles = text_tiles(t.size);
    d_tile.ensure(tiles + 2);
    timer.start(s);
    launch_count_newlines(t, d_tile.p, s);
    launch_scan64(d_tile.p, tiles, 0, s);
    uint64_t n_newlines = 0;
    SBX_HIP(hipMemcpyAsync(&n_newlines, d_tile.p + tiles, 8, hipMemcpyDeviceToHost, s));
    SBX_HIP(hipStreamSynchronize(s));
    uploaded();
    if (n_newlines > t.size) throw Error(SBX_EFORMAT, "internal error: more line ends than bytes");
    d_line_start.ensure((size_t)n_newlines + 2);
    launch_line_starts(t, d_tile.p, d_line_start.p, s);
    timer.stop(s);
    return n_newlines;
}

}  // namespace sbx
