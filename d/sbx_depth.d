/**
 * d/sbx_depth.d -- D binding of libsbx_depth.so for sambamba, and the replacement of the body of
 * depth_main (sambamba/depth.d:1163-1234) that drives it.
 *
 * Source only: the build image has no D compiler (SURVEY.md F1).  The declarations below are kept in
 * lock-step with include/sbx_depth.h by tests/test_d_binding.py, which parses the struct and function
 * declarations of this file, lays the structs out with the C ABI's rules and compares every size with
 * sbx_abi_sizeof() of the built library, and every function name with the header's.
 *
 * It follows the one FFI precedent in the reference, BioD/bio/core/utils/zlib.d:6,139-163
 * (extern(C) prototypes, caller-owned buffers, int status turned into an exception).
 * Link with:  -L-lsbx_depth  (plus -L-L<dir of libsbx_depth.so>).
 */
module sbx_depth;

import std.algorithm : map, max, min, sort;
import std.array : array, split;
import std.conv : to;
import std.exception : enforce;
import std.format : format;
import std.stdio : File, stderr, stdout;
import std.string : fromStringz, stripRight, toStringz;

enum SBX_OK = 0;
enum SBX_ENOMEM = -8;
enum SBX_NCOUNTERS = 7;
enum SBX_MODE_BASE = 0;
enum SBX_MODE_REGION = 1;
enum SBX_MODE_WINDOW = 2;
enum SBX_FILTER_MAX_OPS = 64;
enum SBX_FILTER_STRINGS = 512;
enum SBX_FILTER_REGEXES = 2;
enum SBX_REGEX_STATES = 64;
enum SBX_REGEX_CLASSES = 8;

/// The writer handed to sbx_stream_base_rows: C linkage, but neither nothrow nor @nogc -- the D side writes to a File.
alias sbx_write_fn = extern (C) int function(void* user, const(char)* data, size_t n);

extern (C) nothrow @nogc {
    struct sbx_ctx;
    struct sbx_region { uint ref_id; uint start; uint end; }
    struct sbx_region_stats { uint n_reads; uint n_bases; }
    struct sbx_header_info {
        int n_ref; int n_samples; int n_read_groups; int sorted_by_coordinate; int has_index; int reserved;
        ulong n_bgzf_blocks; ulong compressed_bytes; ulong uncompressed_bytes;
    }
    struct sbx_regex_state { ubyte type; ubyte a; ubyte b; ubyte c; }
    struct sbx_regex {
        ubyte n_states; ubyte n_classes; ubyte start; ubyte reserved;
        sbx_regex_state[SBX_REGEX_STATES] states;
        ubyte[32][SBX_REGEX_CLASSES] classes;      // C: uint8_t classes[SBX_REGEX_CLASSES][32]
    }
    struct sbx_filter_op { ubyte kind; ubyte field; ubyte cmp; ubyte pad; uint mask; long value; }
    struct sbx_filter {
        int n_ops; int reserved;
        sbx_filter_op[SBX_FILTER_MAX_OPS] ops;
        char[SBX_FILTER_STRINGS] strings;
        int n_regex; int reserved2;
        sbx_regex[SBX_FILTER_REGEXES] regex;
    }
    struct sbx_batch { uint first_ref; uint n_refs; ulong est_bytes; }
    struct sbx_run_stats {
        double ms_inflate; double ms_index; double ms_accumulate; double ms_reduce; double ms_total; double ms_h2d;
        ulong n_records; ulong n_admitted; ulong n_bgzf_blocks;
        ulong compressed_bytes; ulong uncompressed_bytes; ulong counter_bytes; ulong covered_positions;
        ulong launches_inflate; ulong launches_index; ulong launches_accumulate;
        double ms_huffman; double ms_lz77;
        ulong n_malformed; ulong n_runs; ulong uploaded_bytes; ulong accumulate_read_bytes;
        ulong token_bytes; ulong max_alignment_span; ulong reserved2; ulong reserved3;
    }

    size_t sbx_abi_sizeof(const(char)* type_name);
    int sbx_bgzf_compress(const(ubyte)* input, size_t n, int level, int with_eof, int device, ubyte* output, size_t cap, size_t* out_len,
                          char* err, size_t errlen);
    int sbx_write_bam(const(char)* path, const(ubyte)* stream, size_t n, int level, int with_index, int device, char* err, size_t errlen);
    int sbx_build_index(const(char)* bam_path, const(char)* bai_path, int device, char* err, size_t errlen);
    struct sbx_flagstat_counts {
        ulong[2] reads; ulong[2] secondary; ulong[2] supplementary; ulong[2] dup; ulong[2] mapped; ulong[2] pair_all;
        ulong[2] first; ulong[2] second; ulong[2] pair_good; ulong[2] pair_map; ulong[2] single; ulong[2] diff_chr;
        ulong[2] diff_high;
    }
    int sbx_flagstat(const(char)* bam_path, int device, sbx_flagstat_counts* out_, char* err, size_t errlen);
    int sbx_format_flagstat(const(sbx_flagstat_counts)* f, int tabular, char* buf, size_t cap, size_t* len);
    // n_windows: 0 when the records stayed on the device; otherwise the windows the sorted stream was written in (a file larger
    // than the device, or SBX_SORT_WINDOW_BYTES): sbx_sort_bam then passes the file through the device once per window
    struct sbx_sort_stats {
        ulong n_records_in; ulong n_records_out; ulong inflated_bytes; ulong sorted_stream_bytes; ulong compressed_bytes;
        uint key_bits; uint n_sort_passes; uint n_batches; uint n_windows;
        double ms_inflate; double ms_index; double ms_keys; double ms_sort; double ms_gather; double ms_deflate; double ms_total_wall;
    }
    int sbx_sort_bam(const(char)* in_path, const(char)* out_path, const(sbx_filter)* filter, int level, int with_index, int device,
                     sbx_sort_stats* stats, char* err, size_t errlen);
    int sbx_sort_header_text(const(char)* text, size_t n, char* out_, size_t cap, size_t* out_len);
    // order: 1 sort -n, 2 sort -N; match_mates: -M
    int sbx_sort_bam_by_name(const(char)* in_path, const(char)* out_path, const(sbx_filter)* filter, int level, int order, int match_mates,
                             int device, sbx_sort_stats* stats, char* err, size_t errlen);
    struct sbx_markdup_stats {
        ulong n_records_in; ulong n_records_out; ulong n_end_pairs; ulong n_single_ends; ulong n_unmatched_pairs; ulong n_duplicates;
        ulong inflated_bytes; ulong stream_bytes; ulong compressed_bytes;
        uint n_sort_passes; uint n_batches;
        double ms_inflate; double ms_index; double ms_ends; double ms_pairing; double ms_groups; double ms_gather; double ms_deflate;
        double ms_total_wall;
    }
    int sbx_markdup(const(char)* in_path, const(char)* out_path, int remove_duplicates, int level, const(char)* pg_command_line, int device,
                    sbx_markdup_stats* stats, char* err, size_t errlen);
    // the streamed path of sbx_markdup (a file larger than the device, or SBX_MARKDUP_WINDOW_BYTES); n_windows == 0: the resident path.
    // struct_size: sbx_markdup_stream_stats.sizeof, set by the caller
    struct sbx_markdup_stream_stats {
        uint struct_size; uint n_windows; uint n_batch_runs; uint n_batches_skipped;
        ulong window_bytes; ulong key_store_bytes; ulong n_key_records;
        double ms_keys; double ms_plan; double ms_scatter; double ms_inflate_replay; double ms_index_replay;
    }
    int sbx_markdup_run(const(char)* in_path, const(char)* out_path, int remove_duplicates, int level, const(char)* pg_command_line, int device,
                        sbx_markdup_stats* stats, sbx_markdup_stream_stats* stream_stats, char* err, size_t errlen);
    int sbx_markdup_header_text(const(char)* text, size_t n, const(char)* pg_command_line, char* out_, size_t cap, size_t* out_len);
    struct sbx_merge_stats {
        ulong n_records_in; ulong n_records_out; ulong n_records_rewritten; long bytes_grown;
        ulong inflated_bytes; ulong merged_stream_bytes; ulong compressed_bytes;
        uint n_inputs; uint key_bits; uint n_sort_passes; uint n_batches;
        double ms_inflate; double ms_index; double ms_rewrite; double ms_sort; double ms_gather; double ms_deflate; double ms_total_wall;
    }
    int sbx_merge_bam(const(char)* out_path, const(char*)* in_paths, int n_inputs, const(sbx_filter)* filter, int level, int with_index,
                      int device, sbx_merge_stats* stats, char* err, size_t errlen);
    // the windowed path of sbx_merge_bam (inputs larger than the device, or SBX_MERGE_WINDOW_BYTES); n_windows == 0: the resident path.
    // struct_size: sbx_merge_window_stats.sizeof, set by the caller
    struct sbx_merge_window_stats {
        uint struct_size; uint n_windows; uint n_batch_runs; uint n_batches_skipped; uint n_input_opens;
        ulong window_bytes;
        double ms_dest; double ms_scatter; double ms_inflate_replay; double ms_index_replay;
    }
    int sbx_merge_bam_run(const(char)* out_path, const(char*)* in_paths, int n_inputs, const(sbx_filter)* filter, int level, int with_index,
                          int device, sbx_merge_stats* stats, sbx_merge_window_stats* window_stats, char* err, size_t errlen);
    int sbx_merge_header_text(const(char*)* texts, const(size_t)* lens, int n, char* out_, size_t cap, size_t* out_len);
    enum SBX_VIEW_MAX_REGIONS = 1024;
    struct sbx_view_opts {
        ushort flags_set; ushort flags_unset; int subsample; double fraction; ulong seed;
    }
    struct sbx_view_stats {
        ulong n_records_in; ulong n_records_selected; ulong n_entries_out; ulong inflated_bytes; ulong stream_bytes; ulong compressed_bytes;
        uint n_regions; uint n_sort_passes; uint n_batches; uint reserved;
        double ms_inflate; double ms_index; double ms_select; double ms_emit; double ms_sort; double ms_gather; double ms_deflate; double ms_total_wall;
    }
    int sbx_view_count(const(char)* in_path, const(sbx_filter)* filter, const(sbx_view_opts)* opts, const(char*)* regions, size_t n_regions,
                       const(char)* bed_path, int device, ulong* count, sbx_view_stats* stats, char* err, size_t errlen);
    int sbx_view_bam(const(char)* in_path, const(char)* out_path, const(sbx_filter)* filter, const(sbx_view_opts)* opts, const(char*)* regions,
                     size_t n_regions, const(char)* bed_path, const(char)* pg_command_line, int level, int with_index, int device,
                     sbx_view_stats* stats, char* err, size_t errlen);
    int sbx_view_sam(const(char)* in_path, const(char)* out_path, const(sbx_filter)* filter, const(sbx_view_opts)* opts, const(char*)* regions,
                     size_t n_regions, const(char)* bed_path, const(char)* pg_command_line, int with_header, int device,
                     sbx_view_stats* stats, char* err, size_t errlen);
    // one entry point for the three sinks; the request starts with its own size and grows at its end.  valid_only: `view -v`
    enum SBX_VIEW_SINK_COUNT = 0;
    enum SBX_VIEW_SINK_BAM = 1;
    enum SBX_VIEW_SINK_SAM = 2;
    alias sbx_cstr = const(char)*;
    alias sbx_cstr_list = const(char*)*;
    alias sbx_filter_ptr = const(sbx_filter)*;
    alias sbx_view_opts_ptr = const(sbx_view_opts)*;
    struct sbx_view_request {
        uint struct_size; int sink;
        sbx_cstr in_path; sbx_cstr out_path; sbx_filter_ptr filter; sbx_view_opts_ptr opts; sbx_cstr_list regions; size_t n_regions;
        sbx_cstr bed_path; sbx_cstr pg_command_line;
        int level; int with_index; int with_header; int device;
        int valid_only; int reserved;
    }
    int sbx_view_run(const(sbx_view_request)* request, ulong* count, sbx_view_stats* stats, char* err, size_t errlen);
    // the same call reading only the blocks the .bai names for the regions; OFF is sbx_view_run, AUTO falls back to it without a .bai
    struct sbx_view_index_stats {
        ulong blocks_in_file; ulong blocks_read; ulong runs; ulong compressed_bytes_read; ulong inflated_bytes_read;
        double ms_plan;
    }
    enum SBX_VIEW_INDEX_OFF = 0;
    enum SBX_VIEW_INDEX_REQUIRED = 1;
    enum SBX_VIEW_INDEX_AUTO = 2;
    int sbx_view_run_indexed(const(sbx_view_request)* request, int index_mode, ulong* count, sbx_view_stats* stats,
                             sbx_view_index_stats* index, char* err, size_t errlen);
    // the streamed path of the commands whose output order is the input order (a file larger than the device, or
    // SBX_STREAM_WINDOW_BYTES); all zeros: the resident path
    struct sbx_stream_stats {
        ulong window_bytes; ulong n_pack_launches;
        uint n_windows; uint reserved;
        double ms_pack;
    }
    int sbx_view_run_streamed(const(sbx_view_request)* request, int index_mode, ulong* count, sbx_view_stats* stats,
                              sbx_view_index_stats* index, sbx_stream_stats* stream_stats, char* err, size_t errlen);
    // which records are valid (alignment.d's isValid), and why not: class k of the report is bit k of a record's mask
    enum SBX_VALIDATE_CLASSES = 10;
    struct sbx_validate_report {
        ulong n_records; ulong n_invalid;
        ulong[SBX_VALIDATE_CLASSES] class_count;
        ulong first_ordinal;
        uint first_mask; uint first_name_len;
        char[256] first_name;
    }
    struct sbx_validate_stats {
        double ms_inflate; double ms_index; double ms_valid; double ms_total_wall;
        ulong inflated_bytes;
        uint n_batches; uint reserved;
    }
    int sbx_validate_bam(const(char)* in_path, int device, sbx_validate_report* report, sbx_validate_stats* stats, char* err, size_t errlen);
    int sbx_format_validate_report(const(char)* path, const(sbx_validate_report)* report, char* buf, size_t cap, size_t* len);
    /* `sambamba slice`: R1 and [a, b) per region, whole BGZF blocks copied from the file (see sbx_depth.h).  Divergences from slice.d's
       code, following its header comment: a is the first record with pos >= beg; b is the end of the contig's records when none starts
       at or behind end; FASTA input is not provided. */
    struct sbx_slice_stats {
        ulong n_regions; ulong records_r1; ulong blocks_inflated; ulong blocks_copied; ulong bytes_copied; ulong stream_bytes; ulong compressed_bytes;
        double ms_read; double ms_select; double ms_write; double ms_total_wall;
    }
    int sbx_slice_bam(const(char)* in_path, const(char)* out_path, const(char*)* regions, size_t n_regions, const(char)* bed_path, int device,
                      sbx_slice_stats* stats, char* err, size_t errlen);
    int sbx_view_num_filter(const(char)* text, ushort* flags_set, ushort* flags_unset);
    int sbx_view_reference_info(sbx_ctx*, char* out_, size_t cap, size_t* out_len);
    struct sbx_import_stats {
        ulong n_lines; ulong n_records; ulong text_bytes; ulong stream_bytes; ulong compressed_bytes;
        uint n_chunks; uint reserved;
        double ms_index; double ms_measure; double ms_emit; double ms_deflate; double ms_total_wall;
    }
    // `sambamba view -S -f bam`: in_path "-" is stdin, out_path null or "-" stdout
    int sbx_import_sam(const(char)* in_path, const(char)* out_path, const(char)* pg_command_line, int level, int with_index, int device,
                       sbx_import_stats* stats, char* err, size_t errlen);
    int sbx_import_sam_run(const(char)* in_path, const(char)* out_path, const(char)* pg_command_line, int level, int with_index, int device,
                           sbx_import_stats* stats, sbx_stream_stats* stream_stats, char* err, size_t errlen);
    // `sambamba index [-c]`: check_bins == 0 is sbx_build_index
    int sbx_index_bam(const(char)* bam_path, const(char)* bai_path, int check_bins, int device, char* err, size_t errlen);
    struct sbx_fixbins_stats {
        ulong n_records; ulong n_bins_changed; ulong inflated_bytes; ulong stream_bytes; ulong compressed_bytes;
        uint n_batches; uint reserved;
        double ms_inflate; double ms_index; double ms_bins; double ms_gather; double ms_deflate; double ms_total_wall;
    }
    // `sambamba fixbins`
    int sbx_fixbins(const(char)* in_path, const(char)* out_path, int level, int device, sbx_fixbins_stats* stats, char* err, size_t errlen);
    int sbx_fixbins_run(const(char)* in_path, const(char)* out_path, int level, int device, sbx_fixbins_stats* stats,
                        sbx_stream_stats* stream_stats, char* err, size_t errlen);
    /* `sambamba subsample --type fasthash --max-cov N [-r]`, which subsample.d leaves unfinished: the coverage of the whole file, the
       larger of that at a read's first and last position, and a hash of the read name decide (see sbx_depth.h).  remove == 0 marks
       the dropped reads with flag 0x200; level is an addition (the reference hard-codes 9). */
    struct sbx_subsample_stats {
        ulong n_records; ulong n_counted; ulong n_over; ulong n_dropped; ulong n_written;
        ulong max_cov_seen; ulong cov_array_bytes;
        ulong inflated_bytes; ulong stream_bytes; ulong compressed_bytes;
        uint n_batches; uint reserved;
        double ms_inflate; double ms_index; double ms_mark; double ms_scan; double ms_verdict; double ms_deflate; double ms_total_wall;
    }
    int sbx_subsample(const(char)* in_path, const(char)* out_path, int max_cov, int remove, int level, int with_index,
                      const(char)* pg_command_line, int device, sbx_subsample_stats* stats, sbx_stream_stats* stream_stats, char* err,
                      size_t errlen);
    struct sbx_fasta_stats {
        ulong n_sequences; ulong n_lines; ulong n_bytes;
        uint n_chunks; uint reserved;
        double ms_lines; double ms_segments; double ms_total_wall;
    }
    // `sambamba index -F`
    int sbx_index_fasta(const(char)* fasta_path, const(char)* fai_path, int device, sbx_fasta_stats* stats, char* err, size_t errlen);
    int sbx_inflate_blocks(const(ubyte)* comp, const(ulong)* comp_off, const(uint)* comp_len, const(uint)* isize,
                           uint n_blocks, ubyte* out_, const(ulong)* out_off, char* err, size_t errlen);
    sbx_ctx* sbx_open(const(char*)* bam_paths, int n_bams, int device, char* err, size_t errlen);
    void sbx_close(sbx_ctx*);
    const(char)* sbx_last_error(sbx_ctx*);
    int sbx_header(sbx_ctx*, sbx_header_info*);
    const(char)* sbx_ref_name(sbx_ctx*, int);
    long sbx_ref_length(sbx_ctx*, int);
    int sbx_ref_id(sbx_ctx*, const(char)*);
    const(char)* sbx_sample_name(sbx_ctx*, int);
    const(char)* sbx_header_text(sbx_ctx*, size_t* len);
    int sbx_compile_filter(const(char)* query, sbx_filter* out_, char* err, size_t errlen);
    int sbx_set_filter(sbx_ctx*, const(sbx_filter)*);
    int sbx_regex_search(const(char)* pattern, const(char)* options, const(char)* text, size_t n, char* err, size_t errlen);
    int sbx_set_params(sbx_ctx*, int mode, ubyte min_bq, int fix_mate_overlaps, int combined, uint window, uint overlap,
                       const(uint)* thresholds, int n_thresholds);
    int sbx_set_regions(sbx_ctx*, const(sbx_region)*, size_t);
    int sbx_parse_regions(sbx_ctx*, const(char)* bed_path_or_region, size_t* n_merged, size_t* n_raw);
    int sbx_parsed_regions(sbx_ctx*, int merged, sbx_region* out_regions, size_t cap);
    const(char)* sbx_parsed_region_line(sbx_ctx*, size_t raw_index);
    int sbx_run(sbx_ctx*);
    int sbx_plan_batches(sbx_ctx*, ulong budget_bytes, sbx_batch* out_batches, size_t cap, size_t* n_out);
    int sbx_run_batch(sbx_ctx*, uint first_ref, uint n_refs);
    int sbx_run_interval(sbx_ctx*, uint ref_id, uint beg, uint end);
    int sbx_prefetch_interval(sbx_ctx*, uint ref_id, uint beg, uint end);
    int sbx_run_interval_owned(sbx_ctx*, uint ref_id, uint beg, uint end);
    int sbx_depth_base_tile_device(sbx_ctx*, uint ref_id, uint beg, uint end, void* d_counters);
    int sbx_depth_base_tile(sbx_ctx*, uint ref_id, uint beg, uint end, uint* counters, ubyte* covered);
    int sbx_depth_region_stats(sbx_ctx*, const(sbx_region)*, size_t, sbx_region_stats*, uint* cov_counts, ubyte* seen);
    int sbx_depth_region_stats_from(sbx_ctx*, const(sbx_region)*, size_t, const(uint)* min_start, sbx_region_stats*,
                                    uint* cov_counts, ubyte* seen);
    int sbx_depth_window_stats(sbx_ctx*, uint ref_id, ulong first_win, ulong n_win, sbx_region_stats*, uint* cov_counts);
    int sbx_format_base_rows(sbx_ctx*, uint ref_id, uint beg, uint end, double min_cov, double max_cov, int annotate,
                             char* out_buf, size_t cap, size_t* out_len);
    int sbx_format_base_rows_device(sbx_ctx*, uint ref_id, uint beg, uint end, double min_cov, double max_cov, int annotate,
                                    void* d_out, size_t cap, size_t* out_len);
    int sbx_stream_base_rows(sbx_ctx*, uint ref_id, uint beg, uint end, double min_cov, double max_cov, int annotate,
                             sbx_write_fn write, void* user);
    int sbx_last_run_stats(sbx_ctx*, sbx_run_stats*);
    int sbx_next_active_range(sbx_ctx*, uint ref_id, ulong from, ulong* beg, ulong* end);
    int sbx_tile_info(sbx_ctx*, uint* tile_pos, uint* n_samples);
    int sbx_preload(sbx_ctx*);
    struct sbx_shard { uint shard; uint ref_id; uint beg; uint end; }
    int sbx_device_count();
    int sbx_plan_shards(const(long)* ref_lengths, int n_ref, int n_shards, uint alignment, sbx_shard* shards, size_t cap, size_t* n_out);
}

/// Thrown exactly where depth.d would throw; depth_main's catch (depth.d:1237-1244) prints it.
void sbxEnforce(sbx_ctx* ctx, int rc) {
    enforce(rc == SBX_OK, fromStringz(sbx_last_error(ctx)).idup);
}

/// What depth_main has parsed from the command line before it opens the BAM files (depth.d:1093-1158).
struct SbxDepthOptions {
    int mode;                    // SBX_MODE_*
    string query;                // -F, null = the default filter of depth.d:1159
    double min_cov = 0, max_cov = 1e50;
    ubyte min_base_quality;
    bool annotate, combined, fix_mate_overlaps;
    uint window_size, overlap;   // window mode (depth.d:1015-1018)
    uint[] cov_thresholds;       // -T (depth.d:712-715)
    sbx_region[] merged_bed;     // -L, merged and sorted as parseBed(..., true) returns it (bed.d:128-141)
    sbx_region[] raw_bed;        // region mode: the unmerged list in input order (depth.d:1192)
    string[] raw_bed_lines;      // region mode: the input lines that go in front of every row (depth.d:902-906)
}

private string fmtG(float f) { return format("%g", f); }   // write(float), depth.d:859-864

/// printRegionStats (depth.d:847-876): one row of region / window statistics.
private void printRegionRow(File output, ref const SbxDepthOptions o, string prefix, uint length,
                            sbx_region_stats st, const(uint)[] cov, string sample) {
    const float mean = cast(float) st.n_bases / length;
    const bool ok = mean >= o.min_cov && mean <= o.max_cov;
    if (!ok && !o.annotate) return;
    output.write(prefix, st.n_reads, '\t', fmtG(mean));
    foreach (j, thr; o.cov_thresholds) {
        const float pct = thr == 0 ? 100.0f : cast(float) cov[j] * 100 / length;
        output.write('\t', fmtG(pct));
    }
    if (!o.combined) output.write('\t', sample);
    if (o.annotate) output.write('\t', ok ? 'y' : 'n');
    output.write('\n');
}

/// The writer of base rows: the File the caller opened for -o / stdout.
extern (C) int sbxFileSink(void* user, const(char)* data, size_t n) {
    try { (cast(File*) user).rawWrite(data[0 .. n]); return 0; } catch (Exception) { return 1; }
}

/// Position of the first pileup column of contigs [r0, r1) of the resident run (cli.cpp first_column): exact, from the
/// `covered` bytes of sbx_depth_base_tile -- sbx_next_active_range alone is tile granular.
private bool firstColumn(sbx_ctx* ctx, uint r0, uint r1, out uint fref, out ulong fpos) {
    uint T, S;
    sbxEnforce(ctx, sbx_tile_info(ctx, &T, &S));
    foreach (r; r0 .. r1) {
        ulong from = 0, b, e;
        for (;;) {
            sbxEnforce(ctx, sbx_next_active_range(ctx, r, from, &b, &e));
            if (b == ulong.max) break;
            for (ulong p = b; p < e; p += 65536) {
                const ulong q = min(e, p + 65536);
                auto cov = new ubyte[cast(size_t)(q - p)];
                sbxEnforce(ctx, sbx_depth_base_tile(ctx, r, cast(uint) p, cast(uint) q, null, cov.ptr));     // `covered` alone
                foreach (x; 0 .. cov.length) if (cov[x]) { fref = r; fpos = p + x; return true; }
            }
            from = e;
        }
    }
    return false;
}

/// Position of the last pileup column of contig r, which has one (cli.cpp WindowPrinter.last_column).
private ulong lastColumn(sbx_ctx* ctx, uint r) {
    uint T, S;
    sbxEnforce(ctx, sbx_tile_info(ctx, &T, &S));
    ulong from = 0, lb = 0, le = 0, b, e;
    for (;;) {
        sbxEnforce(ctx, sbx_next_active_range(ctx, r, from, &b, &e));
        if (b == ulong.max) break;
        lb = b; le = e; from = e;
    }
    for (ulong q = le; q > lb;) {
        const ulong p = q > lb + 65536 ? q - 65536 : lb;
        auto cov = new ubyte[cast(size_t)(q - p)];
        sbxEnforce(ctx, sbx_depth_base_tile(ctx, r, cast(uint) p, cast(uint) q, null, cov.ptr));             // `covered` alone
        for (ulong x = q; x > p; --x) if (cov[cast(size_t)(x - 1 - p)]) return x - 1;
        q = p;
    }
    return 0;
}

/**
 * `depth base` rows printed on the host from the device's counters, for the option sets whose text is NOT a pure function of the
 * position: `-L` together with `-c 0` (writeEmptyColumns consumes the raw BED as it goes, depth.d:464-486) and `-c 0` when alignments
 * hang over a contig's end (their columns are column rows, not zero rows).  It is PerBasePrinter's push / close / writeEmptyColumns /
 * writeColumn (depth.d:452-606) fed with the columns of the device's tiles instead of pileup columns -- the same statements as
 * sambamba_amd/csrc/cli.cpp `BasePrinter` (the compiled host the test-suite holds against the reference's goldens).
 */
private struct BaseHostPrinter {
    sbx_ctx* ctx;
    const(SbxDepthOptions)* o;
    File output;
    string[] samples;
    uint S;
    int n_ref;
    bool bed_provided;
    sbx_region[] bed;          // NonOverlappingRegionStatsCollector view (depth.d:171-198)
    size_t cur_head;
    sbx_region[] raw;          // raw_bed, consumed by writeEmptyColumns
    size_t raw_head;
    int prev_ref = -2;
    long prev_pos;
    string[] tails;

    static bool fullyLeftOf(sbx_region g, uint r, uint pos) { return g.ref_id < r || (g.ref_id == r && g.end <= pos); }
    static bool overlaps(sbx_region g, uint r, uint pos) { return g.ref_id == r && g.start <= pos && pos < g.end; }

    bool outputRequired(int r, long pos) {                                               // depth.d:558-565
        if (!bed_provided) return true;
        while (cur_head < bed.length && fullyLeftOf(bed[cur_head], cast(uint) r, cast(uint) pos)) ++cur_head;
        return cur_head < bed.length && overlaps(bed[cur_head], cast(uint) r, cast(uint) pos);
    }
    void initTails() {                                                                   // depth.d:436-450
        if (tails.length) return;
        const string flag = o.annotate ? (o.min_cov > 0 ? "\tn" : "\ty") : "";
        if (o.combined) tails ~= "\t0\t0\t0\t0\t0\t0\t0" ~ flag;
        else foreach (sm; samples) tails ~= "\t0\t0\t0\t0\t0\t0\t0\t" ~ sm ~ flag;
    }
    void emitEmpty(string name, long from, long to) {
        foreach (pos; from .. to) foreach (t; tails) output.write(name, '\t', pos, t, '\n');
    }
    void writeEmpty(long ref_id, long start, long end) {                                 // writeEmptyColumns, depth.d:452-487
        if (o.min_cov > 0 && !o.annotate) return;
        const name = fromStringz(sbx_ref_name(ctx, cast(int) ref_id)).idup;
        initTails();
        if (!bed_provided) { emitEmpty(name, start, end); return; }
        if (raw_head >= raw.length || raw[raw_head].ref_id > cast(uint) ref_id) return;
        while (raw_head < raw.length && raw[raw_head].ref_id < cast(uint) ref_id) ++raw_head;
        while (raw_head < raw.length && raw[raw_head].ref_id == cast(uint) ref_id) {
            if (fullyLeftOf(raw[raw_head], cast(uint) ref_id, cast(uint) start)) { ++raw_head; continue; }
            const long from = max(start, cast(long) raw[raw_head].start), to = min(end, cast(long) raw[raw_head].end);
            if (from >= to) break;
            emitEmpty(name, from, to);
            raw[raw_head].start = cast(uint) to;
            if (raw[raw_head].start >= raw[raw_head].end) ++raw_head;
        }
        bed = raw[raw_head .. $].dup;                                                     // the collector is rebuilt from what is left (depth.d:485)
        cur_head = 0;
    }
    void writeColumn(int r, long pos, const(uint)[] cnt) {                               // depth.d:534-555
        const name = fromStringz(sbx_ref_name(ctx, r)).idup;
        foreach (s; 0 .. S) {
            const v = cnt[s * SBX_NCOUNTERS .. (s + 1) * SBX_NCOUNTERS];
            const ulong total = cast(ulong) v[0] + v[1] + v[2] + v[3] + v[4] + v[5] + v[6];
            const bool ok = total >= o.min_cov && total <= o.max_cov;
            if (!ok && !o.annotate) return;                                              // return, not continue (depth.d:540-541)
            output.write(name, '\t', pos, '\t', total, '\t', v[0], '\t', v[1], '\t', v[2], '\t', v[3], '\t', v[5], '\t', v[6]);
            if (!o.combined) output.write('\t', samples[s]);
            if (o.annotate) output.write(ok ? "\ty" : "\tn");
            output.write('\n');
        }
    }
    void push(int r, long pos, const(uint)[] cnt) {                                      // depth.d:567-591
        if (o.min_cov > 0) {
            if (outputRequired(r, pos)) writeColumn(r, pos, cnt);
            return;
        }
        if (prev_ref == -2) {
            foreach (id; 0 .. r) writeEmpty(id, 0, sbx_ref_length(ctx, id));
            writeEmpty(r, 0, pos);
        } else if (prev_ref != r) {
            writeEmpty(prev_ref, prev_pos + 1, sbx_ref_length(ctx, prev_ref));
            writeEmpty(r, 0, pos);
        } else if (prev_pos != pos - 1) {
            writeEmpty(r, prev_pos + 1, pos);
        }
        prev_ref = r;
        prev_pos = pos;
        if (outputRequired(r, pos)) writeColumn(r, pos, cnt);
    }
    void close() {                                                                       // depth.d:593-606
        if (!(o.min_cov == 0)) return;
        if (prev_ref == -2) {
            foreach (id; 0 .. n_ref) writeEmpty(id, 0, sbx_ref_length(ctx, id));
        } else {
            writeEmpty(prev_ref, prev_pos + 1, sbx_ref_length(ctx, prev_ref));
            foreach (id; prev_ref + 1 .. n_ref) writeEmpty(id, 0, sbx_ref_length(ctx, id));
        }
    }
    /// every pileup column of contigs [r0, r1) of the resident run, in order
    void runRefs(uint r0, uint r1) {
        enum ulong CH = 1u << 20;
        foreach (r; r0 .. r1) {
            ulong from = 0, b, e;
            for (;;) {
                sbxEnforce(ctx, sbx_next_active_range(ctx, r, from, &b, &e));
                if (b == ulong.max) break;
                for (ulong p = b; p < e; p += CH) {
                    const ulong q = min(e, p + CH);
                    auto cnt = new uint[cast(size_t)(q - p) * S * SBX_NCOUNTERS];
                    auto cov = new ubyte[cast(size_t)(q - p)];
                    sbxEnforce(ctx, sbx_depth_base_tile(ctx, r, cast(uint) p, cast(uint) q, cnt.ptr, cov.ptr));
                    foreach (x; 0 .. cov.length)
                        if (cov[x]) push(cast(int) r, cast(long)(p + x), cnt[x * S * SBX_NCOUNTERS .. (x + 1) * S * SBX_NCOUNTERS]);
                }
                from = e;
            }
        }
    }
}

/**
 * Replacement of depth.d:1163-1234 ("new MultiBamReader ... printer.close()").  depth_main keeps its option
 * parsing and its BED parsing (parseBed / parseRegion need the reference dictionary: use sbxOpen first and
 * sbx_ref_id / sbx_ref_length in place of bam.hasReference / bam[name]) and calls this with the opened context.
 * The header lines (`REF\tPOS...` / `# chrom\t...`) are printed by the caller exactly as printer.init() does.
 *
 * Text rules are the reference's, and the same as sambamba_amd/csrc/cli.cpp applies (the compiled host that the test-suite
 * compares with the reference's goldens and with the oracle):
 *   base    rows come formatted from the device (K6 reproduces writeColumn / writeEmptyColumns byte for byte).  With -c 0 a
 *           contig WITHOUT pileup columns is zero-filled only before the first and after the last contig that has some
 *           (push() fills from the previous column's contig straight to the current one, depth.d:574-583; close() fills what
 *           follows the last column, depth.d:593-606); columns of alignments hanging over a contig end are printed too.
 *   region  printRegionStats' rules; rows only if some column fell inside some region (lazily created samples, B-12).
 *   window  (overlap 0) nothing before the first pileup column of the run -- the exact column, not its tile --; a contig
 *           with columns prints every window finished by its columns or by its length (alignments hanging over the end finish
 *           windows beyond it); read-less contigs between two contigs with columns print length / w all-zero windows; the
 *           FIRST read-less contig after the last contig with columns continues that contig's window coordinates and its
 *           first row shows what the unfinished window held (close() does not reset the ring, depth.d:1070-1076).
 * `base -L` together with `-c 0`, and `base -c 0` when alignments hang over a contig end, are printed on the host from the device's
 * counters (BaseHostPrinter above: PerBasePrinter's own rules), as cli.cpp does.  ONE corner stays with the reference's own code path
 * (return false -> the caller runs the old body of depth_main): `window --overlap > 0` -- cli.cpp `WindowPrinter::window_stats` shows
 * how the ring's bookkeeping is driven through sbx_depth_region_stats_from.
 */
bool sbxDepthRun(sbx_ctx* ctx, ref const SbxDepthOptions o, File output) {
    if (o.mode == SBX_MODE_WINDOW && o.overlap != 0) return false;

    sbx_header_info hi;
    sbxEnforce(ctx, sbx_header(ctx, &hi));
    enforce(hi.sorted_by_coordinate != 0, "All files must be coordinate-sorted");       // depth.d:1164-1165
    enforce(hi.has_index != 0, "All files must be indexed");                            // depth.d:1166

    char[512] err;
    sbx_filter f;
    enforce(sbx_compile_filter(o.query is null ? null : o.query.toStringz, &f, err.ptr, err.length) == SBX_OK,
            fromStringz(err.ptr).idup);
    sbxEnforce(ctx, sbx_set_filter(ctx, &f));
    sbxEnforce(ctx, sbx_set_params(ctx, o.mode, o.min_base_quality, o.fix_mate_overlaps ? 1 : 0, o.combined ? 1 : 0,
                                   o.window_size, o.overlap, o.cov_thresholds.ptr, cast(int) o.cov_thresholds.length));
    if (o.merged_bed.length)
        sbxEnforce(ctx, sbx_set_regions(ctx, o.merged_bed.ptr, o.merged_bed.length));   // bam.getReadsOverlapping(bed)

    string[] samples;
    foreach (s; 0 .. hi.n_samples) samples ~= fromStringz(sbx_sample_name(ctx, s)).idup;
    const uint S = o.combined ? 1 : cast(uint) samples.length;
    const size_t n_thr = max(1, o.cov_thresholds.length);
    const ulong w = o.window_size;

    // the device takes the file in batches of contigs sized to its free memory (one batch unless whole-genome sized)
    size_t n_batches;
    sbxEnforce(ctx, sbx_plan_batches(ctx, 0, null, 0, &n_batches));
    auto plan = new sbx_batch[n_batches];
    if (n_batches) sbxEnforce(ctx, sbx_plan_batches(ctx, 0, plan.ptr, plan.length, &n_batches));

    // region mode gathers per batch and prints at the end, in input order (PerBedRegionPrinter.close, depth.d:925-930)
    auto r_st = new sbx_region_stats[o.raw_bed.length * S];
    auto r_cov = new uint[o.raw_bed.length * S * n_thr];
    auto r_seen = new ubyte[o.raw_bed.length];

    // base -L with -c 0: the text depends on the order in which the raw BED is consumed -- the host printer, fed batch by batch
    const bool base_host = o.mode == SBX_MODE_BASE && o.merged_bed.length && o.min_cov <= 0;
    BaseHostPrinter hp;
    if (o.mode == SBX_MODE_BASE) {
        hp.ctx = ctx; hp.o = &o; hp.output = output; hp.samples = samples; hp.S = S; hp.n_ref = hi.n_ref;
        if (o.merged_bed.length) { hp.bed_provided = true; hp.bed = o.merged_bed.dup; hp.raw = o.merged_bed.dup; }
    }
    // base -c 0: contigs without columns seen since the last contig that had some (cli.cpp BasePrinter.pending_empty_)
    bool base_seen_columns = false;
    uint[] base_pending_empty;
    // window mode (cli.cpp WindowPrinter): first column of the run, the last contig with columns, what its unfinished window holds
    bool have_first = false;
    uint fref = 0;
    ulong fpos = 0;
    int last_cols_ref = -1;
    ulong last_nl = 0;
    sbx_region_stats[] stale_st;
    uint[] stale_cov;
    uint[] win_pending_empty;

    void emitBase(uint r, ulong p, ulong q, double min_cov) {
        if (q <= p) return;
        sbxEnforce(ctx, sbx_stream_base_rows(ctx, r, cast(uint) p, cast(uint) q, min_cov, o.max_cov, o.annotate ? 1 : 0,
                                             &sbxFileSink, &output));
    }
    void windowRows(string name, ulong start, const(sbx_region_stats)[] st, const(uint)[] cov) {
        const prefix = name ~ "\t" ~ start.to!string ~ "\t" ~ (start + w).to!string ~ "\t";
        foreach (s; 0 .. S) {
            sbx_region_stats z;
            auto zc = new uint[n_thr];
            printRegionRow(output, o, prefix, cast(uint) w, st.length ? st[s] : z, cov.length ? cov[s * n_thr .. (s + 1) * n_thr] : zc, samples[s]);
        }
    }
    void zeroWindows(uint r) {                                                           // printEmptyWindows, depth.d:1039-1044
        const ulong cnt = cast(ulong) max(0L, sbx_ref_length(ctx, cast(int) r)) / w;
        const name = fromStringz(sbx_ref_name(ctx, cast(int) r)).idup;
        foreach (k; 0 .. cnt) windowRows(name, k * w, null, null);
    }
    // statistics of windows [k0, k1) of contig r as [k][S] / [k][S][n_thr]: the engine's window statistics for windows inside the
    // contig, region statistics for windows that end beyond it
    void windowStats(uint r, ulong k0, ulong k1, ref sbx_region_stats[] st, ref uint[] cov) {
        const size_t n = cast(size_t)(k1 - k0);
        st = new sbx_region_stats[n * S];
        cov = new uint[n * S * n_thr];
        if (!n) return;
        const ulong len = cast(ulong) max(0L, sbx_ref_length(ctx, cast(int) r));
        if (k1 * w <= len) { sbxEnforce(ctx, sbx_depth_window_stats(ctx, r, k0, k1 - k0, st.ptr, cov.ptr)); return; }
        auto reg = new sbx_region[n];
        foreach (i; 0 .. n) reg[i] = sbx_region(r, cast(uint)((k0 + i) * w), cast(uint)((k0 + i) * w + w));
        auto seen = new ubyte[n];
        auto cov1 = new uint[n * S * n_thr];
        sbxEnforce(ctx, sbx_depth_region_stats(ctx, reg.ptr, n, st.ptr, cov1.ptr, seen.ptr));
        foreach (i; 0 .. n * S) foreach (t; 0 .. o.cov_thresholds.length) cov[i * n_thr + t] = cov1[i * o.cov_thresholds.length + t];
    }

    foreach (b; plan) {
        if (plan.length == 1) sbxEnforce(ctx, sbx_run(ctx));
        else sbxEnforce(ctx, sbx_run_batch(ctx, b.first_ref, b.n_refs));
        const uint r0 = b.first_ref, r1 = b.first_ref + b.n_refs;
        if (o.mode == SBX_MODE_WINDOW && !have_first) {
            if (!firstColumn(ctx, r0, r1, fref, fpos)) continue;                          // no column yet: windows so far print nothing
            have_first = true;
        }
        if (base_host) { hp.runRefs(r0, r1); continue; }
        foreach (r; r0 .. r1) {
            const name = fromStringz(sbx_ref_name(ctx, cast(int) r)).idup;
            const ulong len = cast(ulong) max(0L, sbx_ref_length(ctx, cast(int) r));
            stderr.writeln("Processing reference #", r + 1, " (", name, ")");           // depth.d:1225-1229
            ulong act_b, act_e;
            sbxEnforce(ctx, sbx_next_active_range(ctx, r, 0, &act_b, &act_e));
            const bool has_columns = act_b != ulong.max;
            final switch (o.mode) {
            case SBX_MODE_BASE:
                if (o.merged_bed.length) {
                    foreach (g; o.merged_bed) if (g.ref_id == r) emitBase(r, g.start, g.end, o.min_cov);     // outputRequired, depth.d:558-565
                } else if (o.min_cov <= 0) {
                    if (!has_columns) {
                        if (!base_seen_columns) emitBase(r, 0, len, o.min_cov);            // before the first contig with columns: zero rows
                        else base_pending_empty ~= r;                                      // decided when the next contig with columns / the end comes
                        break;
                    }
                    base_seen_columns = true;
                    base_pending_empty.length = 0;                                         // skipped: push() jumps to the current contig
                    emitBase(r, 0, len, o.min_cov);
                    // columns beyond the contig end (alignments hanging over it) are column rows, not zero rows: from the counters
                    ulong from2 = len, ob, oe;
                    for (;;) {
                        sbxEnforce(ctx, sbx_next_active_range(ctx, r, from2, &ob, &oe));
                        if (ob == ulong.max) break;
                        ob = max(ob, from2);
                        auto cnt = new uint[cast(size_t)(oe - ob) * S * SBX_NCOUNTERS];
                        auto cov = new ubyte[cast(size_t)(oe - ob)];
                        sbxEnforce(ctx, sbx_depth_base_tile(ctx, r, cast(uint) ob, cast(uint) oe, cnt.ptr, cov.ptr));
                        foreach (x; 0 .. cov.length)
                            if (cov[x]) hp.writeColumn(cast(int) r, cast(long)(ob + x), cnt[x * S * SBX_NCOUNTERS .. (x + 1) * S * SBX_NCOUNTERS]);
                        from2 = oe;
                    }
                } else {
                    ulong from = 0, rb, re;
                    for (;;) {
                        sbxEnforce(ctx, sbx_next_active_range(ctx, r, from, &rb, &re));
                        if (rb == ulong.max) break;
                        emitBase(r, max(rb, from), re, o.min_cov);                         // (tiles beyond `len`: the contig's spare tile)
                        from = re;
                    }
                }
                break;
            case SBX_MODE_REGION:
                size_t[] ids;
                sbx_region[] sub;
                foreach (i, g; o.raw_bed) if (g.ref_id == r) { ids ~= i; sub ~= g; }
                if (!sub.length) break;
                auto st = new sbx_region_stats[sub.length * S];
                auto cv = new uint[sub.length * S * n_thr];
                auto sn = new ubyte[sub.length];
                sbxEnforce(ctx, sbx_depth_region_stats(ctx, sub.ptr, sub.length, st.ptr, cv.ptr, sn.ptr));
                foreach (j, id; ids) {
                    r_seen[id] = sn[j];
                    foreach (s; 0 .. S) {
                        r_st[id * S + s] = st[j * S + s];
                        foreach (t; 0 .. o.cov_thresholds.length)
                            r_cov[(id * S + s) * n_thr + t] = cv[(j * S + s) * o.cov_thresholds.length + t];
                    }
                }
                break;
            case SBX_MODE_WINDOW:
                if (r < fref) break;                                                       // before the first column of the run: nothing
                if (!has_columns) { win_pending_empty ~= r; break; }
                foreach (e; win_pending_empty) zeroWindows(e);                             // read-less contigs between two with columns
                win_pending_empty.length = 0;
                // windows finished by the contig's columns or by its length; alignments hanging over the end finish windows beyond it
                const ulong lastcol = lastColumn(ctx, r);
                const ulong nw = max(len >= w ? (len - w) / w + 1 : 0, lastcol >= w ? (lastcol - w) / w + 1 : 0);
                enum ulong CHW = 1u << 18;
                for (ulong k0 = 0; k0 < nw; k0 += CHW) {
                    const ulong k1 = min(nw, k0 + CHW);
                    sbx_region_stats[] st;
                    uint[] cv;
                    windowStats(r, k0, k1, st, cv);
                    foreach (k; k0 .. k1) {
                        if (r == fref && k * w + w <= fpos) continue;                      // finished before the first column of the run
                        const size_t i = cast(size_t)(k - k0);
                        windowRows(name, k * w, st[i * S .. (i + 1) * S], cv[i * S * n_thr .. (i + 1) * S * n_thr]);
                    }
                }
                last_cols_ref = cast(int) r;
                last_nl = nw;
                windowStats(r, nw, nw + 1, stale_st, stale_cov);                           // what the ring (one slot at overlap 0) still holds
                break;
            }
        }
    }
    if (base_host) hp.close();
    if (o.mode == SBX_MODE_BASE && !o.merged_bed.length && o.min_cov <= 0)
        foreach (r; base_pending_empty)                                                   // close(): everything after the last column
            emitBase(r, 0, cast(ulong) max(0L, sbx_ref_length(ctx, cast(int) r)), o.min_cov);
    if (o.mode == SBX_MODE_WINDOW && have_first) {
        bool first = true;
        foreach (e; win_pending_empty) {
            if (first && last_cols_ref >= 0) {
                // close() does not reset the ring: this contig continues the previous one's window coordinates
                const ulong cnt = cast(ulong) max(0L, sbx_ref_length(ctx, cast(int) e)) / w;
                const name = fromStringz(sbx_ref_name(ctx, cast(int) e)).idup;
                foreach (i; 0 .. cnt) {
                    if (i < 1) windowRows(name, (last_nl + i) * w, stale_st[0 .. S], stale_cov[0 .. S * n_thr]);
                    else windowRows(name, (last_nl + i) * w, null, null);
                }
            } else zeroWindows(e);
            first = false;
        }
    }
    if (o.mode == SBX_MODE_REGION) {
        bool any = false;
        foreach (v; r_seen) any |= v != 0;
        if (any) foreach (id, g; o.raw_bed) {
            const prefix = o.raw_bed_lines[id].stripRight ~ "\t";                        // depth.d:902-906
            foreach (s; 0 .. S)
                printRegionRow(output, o, prefix, g.end - g.start, r_st[id * S + s], r_cov[(id * S + s) * n_thr .. $], samples[s]);
        }
    }
    return true;
}

/// `auto bam = new MultiBamReader(bam_filenames)` (depth.d:1163) -> the device context.
sbx_ctx* sbxOpen(string[] bam_filenames) {
    char[512] err;
    auto paths = bam_filenames.map!toStringz.array;
    auto ctx = sbx_open(paths.ptr, cast(int) paths.length, -1, err.ptr, err.length);
    enforce(ctx !is null, fromStringz(err.ptr).idup);
    return ctx;
}

/**
 * Several devices (`sambamba depth ... --gpus N`; the compiled counterpart is cli.cpp `struct Sharded`, which the test-suite runs --
 * tests/test_gpu_cli_sharded.py): ONE process, one device context per GPU (sbx_open(..., device = k, ...)), each driven by its own
 * thread.  The job shards by POSITION (sbx_plan_shards): the outputs of disjoint position ranges are disjoint, so nothing travels
 * between the devices -- the reference's analogue of the cut is pileupChunks (BioD/bio/std/hts/bam/pileup.d:1011-1015).
 *
 *   base    (no -L, --min-coverage > 0: the text is a pure function of the position) every context runs its slices
 *           (sbx_run_interval: only the BGZF blocks the BAI lists for them are uploaded and inflated) and streams the text of its
 *           positions; the slices are dealt round-robin and written in genome order, so device k + 1 computes while device k prints
 *   region  every context reports on the BED regions whose first position it owns (a region is never split); rows are printed at
 *           the end, in input order, as PerBedRegionPrinter.close does (depth.d:925-930)
 * Window mode and the order-dependent option sets (base -L, base -c 0, window --overlap) go through sbxDepthRun on one device
 * (cli.cpp shards window mode as well: `Sharded::window` collects the statistics the printer's rules are stated in).
 * Returns false when the option set is not one of the above; the caller then calls sbxDepthRun(ctx0, ...).
 * `ctx0` is the context depth_main opened (on devices[0]); the others are opened and closed here.
 */
bool sbxDepthRunSharded(sbx_ctx* ctx0, string[] bam_filenames, const(int)[] devices, ref const SbxDepthOptions o, File output) {
    import core.sync.condition : Condition;
    import core.sync.mutex : Mutex;
    import core.thread : Thread;

    if (devices.length < 2) return false;
    const bool base_ok = o.mode == SBX_MODE_BASE && !o.merged_bed.length && o.min_cov > 0;
    if (!base_ok && o.mode != SBX_MODE_REGION) return false;

    sbx_header_info hi;
    sbxEnforce(ctx0, sbx_header(ctx0, &hi));
    enforce(hi.sorted_by_coordinate != 0, "All files must be coordinate-sorted");
    enforce(hi.has_index != 0, "All files must be indexed");
    char[512] err;
    sbx_filter f;
    enforce(sbx_compile_filter(o.query is null ? null : o.query.toStringz, &f, err.ptr, err.length) == SBX_OK, fromStringz(err.ptr).idup);

    string[] samples;
    foreach (s; 0 .. hi.n_samples) samples ~= fromStringz(sbx_sample_name(ctx0, s)).idup;
    const uint S = o.combined ? 1 : cast(uint) samples.length;
    const size_t n_thr = max(1, o.cov_thresholds.length);
    const size_t N = devices.length;

    // the plan: equal shares of the concatenated reference, cuts inside a contig at multiples of the tile size
    auto lens = new long[hi.n_ref];
    foreach (r; 0 .. hi.n_ref) lens[r] = sbx_ref_length(ctx0, r);
    size_t n_sh;
    auto shards = new sbx_shard[hi.n_ref + N + 1];
    enforce(sbx_plan_shards(lens.ptr, hi.n_ref, cast(int) N, 1024, shards.ptr, shards.length, &n_sh) == SBX_OK, "internal: shard plan");
    shards = shards[0 .. n_sh];

    void configure(sbx_ctx* c) {
        sbxEnforce(c, sbx_set_filter(c, &f));
        sbxEnforce(c, sbx_set_params(c, o.mode, o.min_base_quality, o.fix_mate_overlaps ? 1 : 0, o.combined ? 1 : 0, o.window_size,
                                     o.overlap, o.cov_thresholds.ptr, cast(int) o.cov_thresholds.length));
        if (o.merged_bed.length) sbxEnforce(c, sbx_set_regions(c, o.merged_bed.ptr, o.merged_bed.length));
    }
    auto cx = new sbx_ctx*[N];
    cx[0] = ctx0;
    scope (exit) foreach (k; 1 .. N) if (cx[k] !is null) sbx_close(cx[k]);
    sbx_ctx* context(size_t k) {          // called on worker k's thread: the contexts open side by side
        if (k == 0) { configure(ctx0); return ctx0; }
        char[512] e;
        auto paths = bam_filenames.map!toStringz.array;
        auto c = sbx_open(paths.ptr, cast(int) paths.length, devices[k], e.ptr, e.length);
        enforce(c !is null, fromStringz(e.ptr).idup);
        cx[k] = c;
        configure(c);
        return c;
    }

    auto mu = new Mutex;
    auto cv = new Condition(mu);
    string failure;
    void fail(string m) { synchronized (mu) { if (failure is null) failure = m.length ? m : "a device of the sharded run failed"; cv.notifyAll(); } }
    void runWorkers(void delegate(size_t k, sbx_ctx* c) work) {
        Thread[] th;
        foreach (k; 0 .. N) {
            auto t = new Thread({ const size_t me = k; return { try work(me, context(me)); catch (Exception e) fail(e.msg); }; }());
            t.start();
            th ~= t;
        }
        foreach (t; th) t.join();
        enforce(failure is null, failure);
    }
    // the slack --fix-mate-overlaps needs on both sides of a region hull: a read past the overlap with its mate is counted differently
    // from an unpaired one (status `past`, depth.d:717-845), so the mate must be in the run; raised to the longest alignment the run reports
    void runWithMateSlack(sbx_ctx* c, uint r, ulong beg, ulong end) {
        if (!o.fix_mate_overlaps) { sbxEnforce(c, sbx_run_interval(c, r, cast(uint) beg, cast(uint) end)); return; }
        ulong slack = 16384;
        foreach (attempt; 0 .. 4) {
            sbxEnforce(c, sbx_run_interval(c, r, cast(uint)(beg > slack ? beg - slack : 0), cast(uint) min(end + slack, 0x7FFFFFFFUL)));
            sbx_run_stats st;
            sbxEnforce(c, sbx_last_run_stats(c, &st));
            if (st.max_alignment_span <= slack) return;
            slack = (st.max_alignment_span + 16383) / 16384 * 16384;
        }
        enforce(false, "--fix-mate-overlaps: the alignments of a slice span more than " ~ slack.to!string ~ " positions; run on one device");
    }

    if (o.mode == SBX_MODE_BASE) {
        static struct Slice { uint r; ulong beg, end, printEnd; size_t owner; }
        Slice[] sl;
        ulong total = 0;
        foreach (L; lens) total += max(0L, L);
        ulong want = max(total / (4 * N), 16UL << 20);
        want = (want + 1023) / 1024 * 1024;
        foreach (sh; shards) {
            const ulong len = cast(ulong) lens[sh.ref_id], span = sh.end - sh.beg;
            const ulong n = (span + want - 1) / want, step = ((span + n - 1) / n + 1023) / 1024 * 1024;
            for (ulong b = sh.beg; b < sh.end; b += step) {
                const ulong e = min(cast(ulong) sh.end, b + step);
                sl ~= Slice(sh.ref_id, b, e, e == len ? 0xFFFF_FFFFUL : e, 0);      // (columns of alignments hanging over the contig end)
            }
        }
        foreach (g, ref x; sl) x.owner = g % N;          // one output stream: round-robin, so that the devices compute next to the one that prints
        auto written = new bool[sl.length];
        output.flush();
        runWorkers((size_t k, sbx_ctx* c) {
            foreach (g, x; sl) {
                if (x.owner != k) continue;
                // (the last slice of a contig also takes the reads that START behind its end, up to the index's coordinate limit)
                sbxEnforce(c, sbx_run_interval(c, x.r, cast(uint) x.beg, x.printEnd == 0xFFFF_FFFFUL ? 1u << 29 : cast(uint) x.end));
                synchronized (mu) {
                    while (failure is null) {
                        bool ready = true;
                        foreach (i; 0 .. g) ready &= written[i];
                        if (ready) break;
                        cv.wait();
                    }
                    if (failure !is null) return;
                }
                ulong from = x.beg, b, e;
                for (;;) {
                    sbxEnforce(c, sbx_next_active_range(c, x.r, from, &b, &e));
                    if (b == ulong.max || b >= x.printEnd) break;
                    b = max(b, from);
                    e = min(e, x.printEnd);
                    sbxEnforce(c, sbx_stream_base_rows(c, x.r, cast(uint) b, cast(uint) e, o.min_cov, o.max_cov, o.annotate ? 1 : 0,
                                                       &sbxFileSink, &output));
                    from = e;
                }
                output.flush();
                synchronized (mu) { written[g] = true; cv.notifyAll(); }
            }
        });
        return true;
    }

    // ---- region ----
    auto r_st = new sbx_region_stats[o.raw_bed.length * S];
    auto r_cov = new uint[o.raw_bed.length * S * n_thr];
    auto r_seen = new ubyte[o.raw_bed.length];
    size_t ownerOf(sbx_region g) {
        // the device that owns the region's first position (regions starting at or beyond the end of their contig: the owner of the
        // contig's last position; regions of zero-length contigs: device 0)
        const long len = lens[g.ref_id];
        if (len <= 0) return 0;
        const ulong p = min(cast(ulong) g.start, cast(ulong) len - 1);
        foreach (x; shards) if (x.ref_id == g.ref_id && x.beg <= p && p < x.end) return x.shard;
        return 0;
    }
    auto ids = new size_t[][N];
    foreach (i, g; o.raw_bed) ids[ownerOf(g)] ~= i;
    runWorkers((size_t k, sbx_ctx* c) {
        // reads are selected against ALL merged regions (a mate that reaches the pileup through a neighbour's region must still pair,
        // depth.d:717-758), but fetched only for the hull of the owned regions of a contig, widened by the mate slack
        foreach (r; 0 .. cast(uint) hi.n_ref) {
            size_t[] mine;
            sbx_region[] sub;
            ulong lo = ulong.max, hi_ = 0;
            foreach (i; ids[k]) if (o.raw_bed[i].ref_id == r) {
                mine ~= i; sub ~= o.raw_bed[i];
                lo = min(lo, cast(ulong) o.raw_bed[i].start); hi_ = max(hi_, cast(ulong) o.raw_bed[i].end);
            }
            if (!mine.length) continue;
            if (hi_ <= lo) hi_ = lo + 1;
            runWithMateSlack(c, r, lo, min(hi_, 0x7FFFFFFFUL));
            auto st = new sbx_region_stats[sub.length * S];
            auto cvs = new uint[sub.length * S * n_thr];
            auto sn = new ubyte[sub.length];
            sbxEnforce(c, sbx_depth_region_stats(c, sub.ptr, sub.length, st.ptr, cvs.ptr, sn.ptr));
            foreach (j, id; mine) {          // (rows of different devices are disjoint)
                r_seen[id] = sn[j];
                foreach (s; 0 .. S) {
                    r_st[id * S + s] = st[j * S + s];
                    foreach (t; 0 .. o.cov_thresholds.length) r_cov[(id * S + s) * n_thr + t] = cvs[(j * S + s) * o.cov_thresholds.length + t];
                }
            }
        }
    });
    bool any = false;
    foreach (v; r_seen) any |= v != 0;
    if (any) foreach (id, g; o.raw_bed) {
        const prefix = o.raw_bed_lines[id].stripRight ~ "\t";                            // depth.d:902-906
        foreach (s; 0 .. S)
            printRegionRow(output, o, prefix, g.end - g.start, r_st[id * S + s], r_cov[(id * S + s) * n_thr .. $], samples[s]);
    }
    return true;
}
