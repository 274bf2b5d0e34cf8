// engine_import.cpp -- sbx_import_sam: `sambamba view -S -f bam` (sambamba/view.d:216-218, 292-311; the reader is BioD's
// bio/std/hts/sam/reader.d, the line parser parseAlignmentLine of sam_alignment.rl) with the lines parsed on the device.
//
// The host reads the input sequentially (a pipe works): the header lines, then the record text in chunks cut at line ends.  A reader
// thread fills two pinned buffers in turn (ChunkReader, engine_chunks.hpp), so that reading chunk k + 1 overlaps the device's
// work on chunk k: upload into one of two device buffers, K15a (index_lines), K15b (record lengths, the bad lines counted), a 64-bit
// scan, K15c (records into the resident store of engine_store.hpp, which grows with grow_keeping).  Every chunk is measured even after
// a bad line was met, so that the refusal names how many there are; nothing is emitted from then on.  The output tail is the one of
// the other resident-store commands: the identity permutation through write_store_output, then index_written_bam.
//
// Records that do not fit the device -- on a pipe nobody knows in advance -- leave as a stream (StreamedOutput, engine_streamout.hpp):
// before the store grows, the grown store must fit next to the old one and must leave room for what the streamed path allocates
// (stream_floor below).  If not, the writer is created, the header and the store's records go through its window, the store and
// the per-file arrays are freed, and from this chunk on K15d writes every chunk's records straight into the window, one launch per
// window the chunk touches; d_len and d_off then hold one chunk.  Nothing was written before the switch, so an input that fits
// still fails on a bad line before a byte is out; behind the switch a bad line is met after windows were written: the remaining
// chunks are measured as ever, the refusal is the same, an output file is removed and a pipe has received bytes.
// SBX_STREAM_WINDOW_BYTES takes the streamed path from the first chunk, SBX_IMPORT_STORE_BYTES forces the switch (tests).
#include <memory>

#include "engine_chunks.hpp"
#include "engine_store.hpp"
#include "engine_streamout.hpp"
#include "markdup_core.hpp"
#include "samparse.hpp"

namespace {

// Text bytes per chunk: 64 MiB (not tuned), or SBX_IMPORT_CHUNK_BYTES (tests: a decimal number of at least 1; anything else counts
// as unset).  Chunks are cut at line ends and their records land in the store in order, so the value does not change a byte of the output.
uint64_t import_chunk_bytes() { return env_size("SBX_IMPORT_CHUNK_BYTES", 64ull << 20); }

// The input, read front to back: the bytes between `head` and the end of `buf` are read and not yet handed out.
struct TextInput {
    FILE* f = nullptr;
    bool close_it = false, eof = false;
    std::vector<uint8_t> buf;
    size_t head = 0;
    ~TextInput() { if (f && close_it) fclose(f); }
    size_t have() const { return buf.size() - head; }
    const uint8_t* at() const { return buf.data() + head; }
    // reads at least `more` further bytes unless the input ends first; false: a read error
    bool read_more(size_t more) {
        if (head > (64u << 10) && head >= buf.size() / 2) { buf.erase(buf.begin(), buf.begin() + (ptrdiff_t)head); head = 0; }
        const size_t want = std::max<size_t>(more, 256u << 10), old = buf.size();
        buf.resize(old + want);
        size_t got = 0;
        while (got < more && !eof) {
            const size_t k = fread(buf.data() + old + got, 1, want - got, f);
            got += k;
            if (k == 0) {
                if (ferror(f)) { buf.resize(old + got); return false; }
                eof = true;
            }
        }
        buf.resize(old + got);
        return true;
    }
    // The header: the lines that start with '@' at the top of the input, each ending in '\n' in *text.
    bool read_header(std::string* text, uint64_t* n_lines) {
        for (;;) {
            if (!have() && !eof && !read_more(1)) return false;
            if (!have() || *at() != '@') return true;
            const uint8_t* nl;
            while (!(nl = (const uint8_t*)memchr(at(), '\n', have())) && !eof)
                if (!read_more(have() + 1)) return false;
            const size_t len = nl ? (size_t)(nl - at()) : have();
            text->append((const char*)at(), len);
            text->push_back('\n');
            ++*n_lines;
            head += nl ? len + 1 : len;
        }
    }
    // The next chunk: as many whole lines as fit `budget` bytes, at least one; the last line of the input need not end in '\n'.
    // Returns its bytes (0: the input is used up) at at(); consume() drops them.
    bool next_chunk(uint64_t budget, size_t* bytes) {
        while (have() < budget && !eof) if (!read_more((size_t)std::min<uint64_t>(budget - have(), 1ull << 30))) return false;
        if (have() <= budget && eof) { *bytes = have(); return true; }
        const size_t in_budget = (size_t)std::min<uint64_t>(have(), budget);
        for (size_t k = in_budget; k-- > 0;)
            if (at()[k] == '\n') { *bytes = k + 1; return true; }
        // the first line is longer than the budget: it is the chunk
        size_t from = in_budget;
        for (;;) {
            const uint8_t* nl = (const uint8_t*)memchr(at() + from, '\n', have() - from);
            if (nl) { *bytes = (size_t)(nl - at()) + 1; return true; }
            from = have();
            if (eof) { *bytes = have(); return true; }
            if (!read_more(1)) return false;
        }
    }
    void consume(size_t bytes) { head += bytes; }
};

// name and length of every @SQ line, in file order
std::vector<RefSeq> header_references(const std::string& text) {
    std::vector<RefSeq> refs;
    size_t p = 0;
    while (p < text.size()) {
        size_t e = text.find('\n', p);
        if (e == std::string::npos) e = text.size();
        if (e - p >= 4 && !text.compare(p, 4, "@SQ\t")) {
            RefSeq r;
            bool have_name = false, have_len = false;
            size_t a = p + 4;
            while (a <= e) {
                size_t b = text.find('\t', a);
                if (b == std::string::npos || b > e) b = e;
                if (b - a >= 3 && !text.compare(a, 3, "SN:")) { r.name = text.substr(a + 3, b - a - 3); have_name = true; }
                if (b - a >= 3 && !text.compare(a, 3, "LN:")) {
                    const std::string v = text.substr(a + 3, b - a - 3);
                    char* end = nullptr;
                    const long long len = strtoll(v.c_str(), &end, 10);
                    if (!v.empty() && !*end && len >= 0 && len <= 0x7FFFFFFFll) { r.length = (int32_t)len; have_len = true; }
                }
                a = b + 1;
            }
            if (!have_name || !have_len || r.name.empty()) throw Error(SBX_EFORMAT, "SAM header: an @SQ line without a valid SN and LN");
            refs.push_back(r);
        }
        p = e + 1;
    }
    return refs;
}

// SBX_IMPORT_STORE_BYTES (tests): the record store may hold no more than this many record bytes; the chunk whose records would
// pass it starts the streamed path.  Anything that is not a positive decimal counts as unset (0: no limit but the device's).
uint64_t import_store_limit() { return env_size("SBX_IMPORT_STORE_BYTES", 0); }

// What the streamed path holds on the device, in bytes: a window of one piece, the encoder's buffers (as StreamBudget reserves
// them), two text chunks, and the arrays of a chunk -- line start, length and offset, 20 bytes per line, and no line of the grammar
// has fewer than 22 bytes.
struct StreamFloor {
    uint64_t piece_blocks, piece_bytes;
    uint64_t window, encoder, text, arrays;
    uint64_t total() const { return window + encoder + text + arrays; }
    // ... of which text_held bytes of text buffers exist already
    uint64_t to_allocate(uint64_t text_held) const { return total() - std::min(text, text_held); }
};
StreamFloor stream_floor(uint64_t chunk_bytes) {
    StreamFloor f{};
    f.piece_blocks = bgzf_piece_blocks();
    f.piece_bytes = f.piece_blocks * (uint64_t)kBgzfPayload;
    f.window = f.piece_bytes + 64;
    f.encoder = f.piece_bytes * 3 + (8ull << 20);
    f.text = 2 * (chunk_bytes + 64);
    f.arrays = (chunk_bytes / 22 + 4096) * 20;
    return f;
}

void print_timing(const sbx_import_stats& st, uint64_t chunk_bytes) {
    if (!getenv("SBX_TIMING")) return;
    fprintf(stderr, "[sbx] import: n_lines=%llu n_records=%llu text_bytes=%llu stream_bytes=%llu compressed_bytes=%llu n_chunks=%u chunk_bytes=%llu "
                    "ms_index=%.3f ms_measure=%.3f ms_emit=%.3f ms_deflate=%.2f ms_total_wall=%.1f\n",
            (unsigned long long)st.n_lines, (unsigned long long)st.n_records, (unsigned long long)st.text_bytes, (unsigned long long)st.stream_bytes,
            (unsigned long long)st.compressed_bytes, st.n_chunks, (unsigned long long)chunk_bytes, st.ms_index, st.ms_measure, st.ms_emit,
            st.ms_deflate, st.ms_total_wall);
}

}  // namespace

extern "C" {

int sbx_import_sam_run(const char* in_path, const char* out_path, const char* pg_command_line, int level, int with_index, int device,
                       sbx_import_stats* stats, sbx_stream_stats* stream_stats, char* err, size_t errlen) {
    const bool to_stdout = !out_path || !strcmp(out_path, "-");
    const char* const path = to_stdout ? "/dev/stdout" : out_path;
    const int rc = run_entry(err, errlen, [&] {
        if (!in_path) throw Error(SBX_EINVAL, "null argument");
        check_level(level);
        if (to_stdout && with_index) throw Error(SBX_EINVAL, "an output on stdout cannot be indexed");
        const bool from_stdin = !strcmp(in_path, "-");
        if (!to_stdout && !from_stdin) refuse_overwrite(in_path, path);
        if (stream_stats) *stream_stats = sbx_stream_stats{};
        const double w0 = wall_now();
        require_device(device);
        int dev = 0;
        SBX_HIP(hipGetDevice(&dev));

        TextInput in;
        in.f = from_stdin ? stdin : fopen(in_path, "rb");
        in.close_it = !from_stdin;
        if (!in.f) throw Error(SBX_EIO, std::string("cannot read ") + in_path);
        std::string sam_header;
        uint64_t n_header_lines = 0;
        if (!in.read_header(&sam_header, &n_header_lines)) throw Error(SBX_EIO, std::string("error reading ") + in_path);
        const std::vector<RefSeq> refs = header_references(sam_header);
        std::string text, why;
        if (!mdc::markdup_header_text(sam_header.data(), sam_header.size(), pg_command_line, &text, &why)) throw Error(SBX_EFORMAT, "SAM header: " + why);
        const std::vector<uint8_t> header = bam_header_bytes(text, refs);
        OutputGuard out_file(path, to_stdout);

        // the reference names on the device, and their hash slots
        std::vector<std::string> names;
        for (const RefSeq& q : refs) names.push_back(q.name);
        const std::vector<uint32_t> slots = sampc::ref_table_slots(names);
        Stream stream;
        stream.create();
        hipStream_t s = stream.get();
        DeviceRefNames d_names;
        upload_ref_names(refs, s, &d_names);
        DevBuf<uint32_t> d_slots(slots.size() + 1);
        if (!slots.empty()) SBX_HIP(hipMemcpyAsync(d_slots.p, slots.data(), slots.size() * 4, hipMemcpyHostToDevice, s));
        const sampc::RefTable table{d_slots.p, (uint32_t)slots.size(), d_names.off.p, d_names.bytes.p};
        DevBuf<unsigned long long> d_acc(kImportAccWords);
        {
            const unsigned long long acc0[kImportAccWords] = {0, kImportNoBadLine, 0, 0};
            SBX_HIP(hipMemcpyAsync(d_acc.p, acc0, sizeof acc0, hipMemcpyHostToDevice, s));
            SBX_HIP(hipStreamSynchronize(s));
        }

        // ---- the chunks: the reader thread fills the slots, this thread parses them ----
        const uint64_t budget = import_chunk_bytes(), window_hook = stream_window_hook(), store_limit = import_store_limit();
        sbx_import_stats st{};
        DevBuf<uint8_t> d_store(64), d_text[2];
        DevBuf<uint64_t> d_off(2), d_tile, d_line_start, d_group;
        DevBuf<uint32_t> d_len(2);
        uint64_t store_used = 0, n_rec = 0;
        std::unique_ptr<StreamedOutput> out;            // the streamed path, from the chunk on that did not fit the store (or the first)
        unsigned long long acc[kImportAccWords] = {0, kImportNoBadLine, 0, 0};

        // Room for `more` further record bytes in the store?  Grows it when it has to and may; false: the records go on as a stream.
        auto store_takes = [&](uint64_t more) {
            if (window_hook || (store_limit && store_used + more > store_limit)) return false;
            const uint64_t need = store_used + more + 64;
            if (need <= d_store.n) return true;
            const uint64_t cap = need + need / 2 + 1024;            // (what grow_keeping allocates, next to the store as it is)
            size_t free_b = 0, total_b = 0;
            SBX_HIP(hipMemGetInfo(&free_b, &total_b));
            // behind the growth the switch must still be possible: what the streamed path allocates, next to the grown store
            if (cap > free_b || free_b - cap + d_store.n < stream_floor(budget).to_allocate(d_text[0].n + d_text[1].n)) return false;
            grow_keeping(d_store, (size_t)store_used, (size_t)need, s);
            return true;
        };
        // The switch: the writer, the header, the store's records through the window; the store and the per-file arrays go.  Lines
        // [0, n_lines) of the current chunk have their lengths at d_len[n_rec ...): they move to the front of arrays of their own.
        auto start_stream = [&](uint64_t chunk_text_bytes, uint64_t n_lines) {
            DevBuf<uint32_t> len_now((size_t)n_lines + 2);
            SBX_HIP(hipMemcpyAsync(len_now.p, d_len.p + n_rec, (size_t)n_lines * 4, hipMemcpyDeviceToDevice, s));
            SBX_HIP(hipStreamSynchronize(s));
            d_len = std::move(len_now);
            d_off.alloc((size_t)n_lines + 2);
            const StreamFloor f = stream_floor(std::max<uint64_t>(budget, chunk_text_bytes));
            const uint64_t to_allocate = f.to_allocate(d_text[0].n + d_text[1].n);
            size_t free_b = 0, total_b = 0;
            SBX_HIP(hipMemGetInfo(&free_b, &total_b));
            if (to_allocate > free_b)
                throw Error(SBX_ENOMEM, "the records do not fit the device: importing them in a stream needs " + std::to_string(f.total()) +
                                            " bytes of device memory (a window of one piece " + std::to_string(f.window) + ", the encoder " +
                                            std::to_string(f.encoder) + ", two text chunks " + std::to_string(f.text) + ", the arrays of a chunk " +
                                            std::to_string(f.arrays) + "), " + std::to_string(to_allocate) + " of them are not allocated yet and " +
                                            std::to_string(free_b) + " are free next to a record store of " + std::to_string(d_store.n) + " bytes");
            // The window: the hook's; else the whole pieces that hold four chunks of text, at most half of what is left and at least
            // the one piece of the floor.  A pipe's stream has no bound to cut the window to, and a chunk's records are fewer bytes
            // than its text: a wider window would save no launch of K15d worth its memory.
            const uint64_t spare_pieces = (free_b - to_allocate) / 2 / f.piece_bytes;
            const uint64_t window = window_hook ? sortc::window_span(f.piece_bytes, window_hook)
                                                : std::min(sortc::window_span(f.piece_bytes, 4 * budget), (1 + spare_pieces) * f.piece_bytes);
            out.reset(new StreamedOutput(out_file, header, window, (uint32_t)f.piece_blocks, level, s));
            out->take_device(d_store.p, store_used);
            d_store.release();
        };
        {
            ChunkReader reader(dev, "reading the SAM text failed", [&](PinnedBuf<uint8_t>& text) {
                size_t bytes = 0;
                if (!in.next_chunk(budget, &bytes)) throw Error(SBX_EIO, std::string("error reading ") + in_path);
                if (bytes) {
                    text.ensure(bytes + 64);
                    memcpy(text.p, in.at(), bytes);
                    in.consume(bytes);
                }
                return bytes;
            });
            EventTimer t_index, t_measure, t_emit;
            uint32_t k = 0;
            while (ChunkSlot* c = reader.next()) {
                const uint64_t size = c->bytes;
                const bool open_end = c->text.p[size - 1] != '\n';
                DevBuf<uint8_t>& d_t = d_text[k++ & 1u];
                d_t.ensure((size_t)size + 64);
                SBX_HIP(hipMemcpyAsync(d_t.p, c->text.p, size, hipMemcpyHostToDevice, s));
                const TextChunk t{d_t.p, size};
                // K15a; the reader may fill the slot again as soon as the upload is done
                const uint64_t n_newlines = index_lines(t, d_tile, d_line_start, t_index, s, [&] { reader.release(c); });
                const uint64_t n_lines = n_newlines + (open_end ? 1u : 0u);
                if (n_rec + n_lines > 0xFFFFFFF0ull) throw Error(SBX_EUNSUPPORTED, "more than 2^32 records");
                // K15b and the offsets; the arrays are the file's while the store is kept and the chunk's on the streamed path
                if (out) {
                    d_len.ensure((size_t)n_lines + 2);
                    d_off.ensure((size_t)n_lines + 2);
                } else {
                    grow_keeping(d_len, (size_t)n_rec, (size_t)(n_rec + n_lines) + 2, s);
                    grow_keeping(d_off, (size_t)n_rec, (size_t)(n_rec + n_lines) + 2, s);
                }
                const uint32_t groups = group_count(n_lines);
                d_group.ensure(groups + 2);
                const ImportLines lines{t, d_line_start.p, n_newlines, n_lines, n_header_lines + st.n_lines + 1, table};
                t_measure.start(s);
                launch_import_measure(lines, d_len.p + (out ? 0 : n_rec), d_group.p, d_acc.p, s);
                launch_scan64(d_group.p, groups, 0, s);
                t_measure.stop(s);
                uint64_t chunk_record_bytes = 0;
                SBX_HIP(hipMemcpyAsync(&chunk_record_bytes, d_group.p + groups, 8, hipMemcpyDeviceToHost, s));
                SBX_HIP(hipMemcpyAsync(acc, d_acc.p, sizeof acc, hipMemcpyDeviceToHost, s));
                SBX_HIP(hipStreamSynchronize(s));
                st.ms_index += t_index.ms();
                st.ms_measure += t_measure.ms();
                st.n_lines += n_lines;
                st.text_bytes += size;
                ++st.n_chunks;
                if (acc[kImportAccBad]) continue;               // (the remaining chunks are still measured, for the count)
                if (!out && !store_takes(chunk_record_bytes)) start_stream(size, n_lines);
                if (out) {
                    // K15d: the chunk's records are the next bytes of the stream, one launch per window they touch
                    launch_group_offsets(d_len.p, d_group.p, n_lines, out->stream_bytes(), d_off.p, s);
                    const double ms_before = out->stats().ms_pack;
                    out->take(chunk_record_bytes, [&](uint8_t* window, uint64_t w_from, uint64_t w_to, unsigned long long* counter) {
                        launch_import_emit_window(lines, d_len.p, d_off.p, window, w_from, w_to, d_acc.p, counter, s);
                    });
                    st.ms_emit += out->stats().ms_pack - ms_before;
                } else {
                    // K15c into the store
                    t_emit.start(s);
                    launch_group_offsets(d_len.p + n_rec, d_group.p, n_lines, store_used, d_off.p + n_rec, s);
                    launch_import_emit(lines, d_len.p + n_rec, d_off.p + n_rec, d_store.p, d_acc.p, s);
                    t_emit.stop(s);
                }
                SBX_HIP(hipMemcpyAsync(acc, d_acc.p, sizeof acc, hipMemcpyDeviceToHost, s));
                SBX_HIP(hipStreamSynchronize(s));
                if (!out) st.ms_emit += t_emit.ms();
                if (acc[kImportAccOverrun]) throw Error(SBX_EFORMAT, "internal error: a record did not have the length it was measured with");
                if (!out) store_used += chunk_record_bytes;
                n_rec += n_lines;
            }
        }
        if (acc[kImportAccBad])
            throw Error(SBX_EFORMAT, "malformed SAM text in " + std::string(in_path) + ": " + std::to_string(acc[kImportAccBad]) +
                                         (acc[kImportAccBad] == 1 ? " line is" : " lines are") + " outside the grammar, the first is line " +
                                         std::to_string(acc[kImportAccFirstBad]));
        d_text[0].release(); d_text[1].release();
        d_tile.release(); d_line_start.release(); d_group.release();

        const uint64_t n = n_rec;
        st.n_records = n;
        if (out) {
            // ---- the streamed path: the last window, short ----
            out->finish();
            out_file.disarm();
            st.stream_bytes = out->stream_bytes(); st.compressed_bytes = out->compressed_bytes();
            st.ms_deflate = out->ms_deflate();
            if (stream_stats) *stream_stats = out->stats();
        } else {
            // ---- the output: the records of the store in their order ----
            DevBuf<uint32_t> d_perm((size_t)n + 2);
            launch_iota(d_perm.p, n, s);
            DevBuf<uint64_t> d_out_off((size_t)n + 2);
            double ms_gather = 0;
            const unsigned long long record_bytes = store_used;
            const WrittenBam w = write_store_output(out_file, header, d_store.p, d_off.p, d_len, d_perm.p, n, d_out_off.p, level, &record_bytes,
                                                    "imported records", s, &ms_gather);
            out_file.disarm();
            st.stream_bytes = w.stream_bytes; st.compressed_bytes = w.compressed_bytes;
            st.ms_deflate = w.ms_deflate;
        }
        st.ms_total_wall = (wall_now() - w0) * 1e3;
        print_timing(st, budget);
        if (stats) *stats = st;
    });
    // (the index is a pass of its own and not part of the figures)
    return rc != SBX_OK ? rc : index_written_bam(path, with_index, device, err, errlen);
}

int sbx_import_sam(const char* in_path, const char* out_path, const char* pg_command_line, int level, int with_index, int device,
                   sbx_import_stats* stats, char* err, size_t errlen) {
    return sbx_import_sam_run(in_path, out_path, pg_command_line, level, with_index, device, stats, nullptr, err, errlen);
}

}  // extern "C"
