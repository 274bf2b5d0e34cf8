// engine_fasta.cpp -- sbx_index_fasta: `sambamba index -F` (sambamba/index.d:115-131; buildFai, BioD bio/std/file/fai.d:78-101) with
// the lines found and added up on the device.
//
// The host probes the first line for its terminator, then reads the file front to back in chunks of a fixed size -- cut at multiples
// of 16 bytes, not at line ends: an unwrapped chromosome is one line of hundreds of megabytes.  A reader thread fills two pinned
// buffers in turn (ChunkReader, engine_chunks.hpp) while the device works on the chunk before: upload into one of two device
// buffers, K15a (index_lines), K17a (header lines counted), K17b (one FastaSeg per header line).  Back come the segments -- 32 bytes
// per header line of the chunk --, two line starts and two counters; fastac::FastaCarry (fasta_core.hpp) folds them into the records
// and keeps what crosses the chunk's ends.  The names are cut on the host from the pinned text.  Every chunk is looked at even after a
// bad line end was met, so that the refusal names how many there are.
#include <sys/stat.h>

#include "engine_chunks.hpp"
#include "fasta.hpp"

namespace {

// Text bytes per chunk: 64 MiB (import's value; NOT tuned), or SBX_FASTA_CHUNK_BYTES (tests: a decimal number of at least 16, rounded
// down to a multiple of 16 and capped at fastac::kChunkLimit; anything else counts as unset).  The output does not depend on it.
uint64_t fasta_chunk_bytes() { return std::min<uint64_t>(env_size("SBX_FASTA_CHUNK_BYTES", 64ull << 20, 16) & ~15ull, fastac::kChunkLimit); }

struct FileCloser {
    FILE* f;
    ~FileCloser() { if (f) fclose(f); }
};

}  // namespace

extern "C" {

int sbx_index_fasta(const char* fasta_path, const char* fai_path, int device, sbx_fasta_stats* stats, char* err, size_t errlen) {
    return run_entry(err, errlen, [&] {
        if (!fasta_path || !fai_path) throw Error(SBX_EINVAL, "null argument");
        refuse_overwrite(fasta_path, fai_path);
        const double w0 = wall_now();
        require_device(device);
        int dev = 0;
        SBX_HIP(hipGetDevice(&dev));
        FileCloser in{fopen(fasta_path, "rb")};
        if (!in.f) throw Error(SBX_EIO, std::string("cannot read ") + fasta_path);

        // the terminator of the first line, and whether that line is a header
        fastac::FastaCarry carry;
        {
            fastac::TerminatorProbe probe;
            std::vector<uint8_t> buf(64u << 10);
            bool first = true;
            for (;;) {
                const size_t k = fread(buf.data(), 1, buf.size(), in.f);
                if (!k) {
                    if (ferror(in.f)) throw Error(SBX_EIO, std::string("error reading ") + fasta_path);
                    break;
                }
                if (first && buf[0] != '>') { carry.seq_before_header = true; throw Error(SBX_EFORMAT, carry.complaint(fasta_path)); }
                first = false;
                if (probe.feed(buf.data(), k)) break;
            }
            carry.crlf = probe.crlf;
            if (fseek(in.f, 0, SEEK_SET) != 0) throw Error(SBX_EIO, std::string("cannot rewind ") + fasta_path);
        }

        Stream stream;
        stream.create();
        hipStream_t s = stream.get();
        // (a file shorter than a chunk does not need the pinned and device buffers of a whole one)
        uint64_t chunk = fasta_chunk_bytes();
        struct stat sb;
        if (fstat(fileno(in.f), &sb) == 0 && S_ISREG(sb.st_mode) && sb.st_size > 0) chunk = std::min<uint64_t>(chunk, ((uint64_t)sb.st_size + 15u) & ~15ull);
        sbx_fasta_stats st{};
        DevBuf<uint8_t> d_text[2];
        DevBuf<uint64_t> d_tile, d_line_start, d_group;
        DevBuf<fastac::FastaSeg> d_seg;
        DevBuf<unsigned long long> d_acc(kFastaAccWords);
        {
            ChunkReader reader(dev, "reading the FASTA text failed", [&](PinnedBuf<uint8_t>& text) {
                text.ensure((size_t)chunk + 64);
                size_t bytes = 0;
                while (bytes < chunk) {
                    const size_t got = fread(text.p + bytes, 1, (size_t)chunk - bytes, in.f);
                    if (!got) {
                        if (ferror(in.f)) throw Error(SBX_EIO, std::string("error reading ") + fasta_path);
                        break;
                    }
                    bytes += got;
                }
                return bytes;
            });
            EventTimer t_lines, t_segments;
            uint32_t k = 0;
            while (ChunkSlot* c = reader.next()) {
                const uint64_t size = c->bytes;
                DevBuf<uint8_t>& d_t = d_text[k++ & 1u];
                d_t.ensure((size_t)size + 64);
                SBX_HIP(hipMemcpyAsync(d_t.p, c->text.p, size, hipMemcpyHostToDevice, s));
                const TextChunk t{d_t.p, size};
                fastac::ChunkResult r;
                r.size = size;
                r.n_newlines = index_lines(t, d_tile, d_line_start, t_lines, s, [] {});       // K15a
                if (r.n_newlines) {
                    SBX_HIP(hipMemcpyAsync(&r.first_start, d_line_start.p + 1, 8, hipMemcpyDeviceToHost, s));
                    SBX_HIP(hipMemcpyAsync(&r.last_start, d_line_start.p + r.n_newlines, 8, hipMemcpyDeviceToHost, s));
                }
                // K17
                const uint64_t n_inner = fasta_inner_lines(r.n_newlines);
                double ms_segments = 0;
                if (n_inner) {
                    const FastaLines lines{t, d_line_start.p, r.n_newlines, carry.crlf ? 1u : 0u};
                    const uint32_t groups = group_count(n_inner);
                    d_group.ensure(groups + 2);
                    const unsigned long long acc0[kFastaAccWords] = {0, fastac::kNoLine};
                    SBX_HIP(hipMemcpyAsync(d_acc.p, acc0, sizeof acc0, hipMemcpyHostToDevice, s));
                    t_segments.start(s);
                    launch_fasta_count_headers(lines, d_group.p, s);
                    launch_scan64(d_group.p, groups, 0, s);
                    uint64_t n_headers = 0;
                    SBX_HIP(hipMemcpyAsync(&n_headers, d_group.p + groups, 8, hipMemcpyDeviceToHost, s));
                    SBX_HIP(hipStreamSynchronize(s));
                    if (n_headers > n_inner) throw Error(SBX_EFORMAT, "internal error: more header lines than lines");
                    d_seg.ensure((size_t)n_headers + 1);
                    launch_fasta_clear_segments(d_seg.p, n_headers + 1, s);
                    launch_fasta_segments(lines, d_group.p, d_seg.p, d_acc.p, s);
                    t_segments.stop(s);
                    r.seg.resize((size_t)n_headers + 1);
                    unsigned long long acc[kFastaAccWords];
                    SBX_HIP(hipMemcpyAsync(r.seg.data(), d_seg.p, r.seg.size() * sizeof(fastac::FastaSeg), hipMemcpyDeviceToHost, s));
                    SBX_HIP(hipMemcpyAsync(acc, d_acc.p, sizeof acc, hipMemcpyDeviceToHost, s));
                    SBX_HIP(hipStreamSynchronize(s));
                    r.n_bare = acc[kFastaAccBare];
                    r.first_bare = acc[kFastaAccFirstBare];
                    ms_segments = t_segments.ms();
                    for (size_t g = 1; g < r.seg.size(); ++g)
                        if (r.seg[g].hdr_off >= size || r.seg[g].hdr_len == 0 || r.seg[g].hdr_len > size - r.seg[g].hdr_off)
                            throw Error(SBX_EFORMAT, "internal error: a header line outside its chunk");
                } else {
                    SBX_HIP(hipStreamSynchronize(s));
                }
                if (r.n_newlines && (r.first_start == 0 || r.first_start > size || r.last_start > size || r.last_start < r.first_start))
                    throw Error(SBX_EFORMAT, "internal error: line starts outside their chunk");
                carry.consume(c->text.p, r);
                reader.release(c);                              // the names are cut: the reader may fill this slot again
                st.ms_lines += t_lines.ms();
                st.ms_segments += ms_segments;
                ++st.n_chunks;
            }
        }
        carry.finish();
        if (carry.failed()) throw Error(SBX_EFORMAT, carry.complaint(fasta_path));
        const std::string text = carry.fai_text();
        OutputGuard out_file(fai_path);
        OutputFile f(out_file);
        f.write(text.data(), text.size());
        f.finish(false);
        out_file.disarm();
        st.n_sequences = carry.recs.size();
        st.n_lines = carry.n_lines;
        st.n_bytes = carry.file_pos;
        st.ms_total_wall = (wall_now() - w0) * 1e3;
        if (getenv("SBX_TIMING"))
            fprintf(stderr, "[sbx] fasta: n_sequences=%llu n_lines=%llu n_bytes=%llu n_chunks=%u chunk_bytes=%llu terminator=%s ms_lines=%.3f "
                            "ms_segments=%.3f ms_total_wall=%.1f\n",
                    (unsigned long long)st.n_sequences, (unsigned long long)st.n_lines, (unsigned long long)st.n_bytes, st.n_chunks,
                    (unsigned long long)chunk, carry.crlf ? "crlf" : "lf", st.ms_lines, st.ms_segments, st.ms_total_wall);
        if (stats) *stats = st;
    });
}

}  // extern "C"
