/* ============================================================================
 * sbx_depth.h -- C ABI of libsbx_depth.so, the MI355X (gfx950) engine behind
 *                `sambamba depth base|region|window`.
 *
 * The reference (biod/sambamba, D) has no plugin API.  Its only FFI precedent is
 * the zlib binding (BioD/bio/core/utils/zlib.d:6,139-163: extern(C) prototypes,
 * caller-owned buffers, int return codes turned into exceptions).  This header
 * follows the same conventions and plugs into the two seams SURVEY.md 8(b) names:
 *
 *   codec seam   decompressBgzfBlock(BgzfBlock)            BioD/bio/core/bgzf/block.d:127
 *                (called from BgzfInputStream.fillNextBlock, inputstream.d:414-417)
 *                -> sbx_inflate_blocks()
 *
 *   engine seam  everything between "bam opened, filter/regions/mode known"
 *                (sambamba/depth.d:1163-1217) and "printer.push / printer.close"
 *                (depth.d:1218-1234)   -> sbx_open ... sbx_depth_* ... sbx_close
 *
 * Conventions: every function returns 0 on success or a negative SBX_E* code;
 * the message is available from sbx_last_error() (the D shim turns it into the
 * `sambamba-depth: <msg>` line of depth.d:1237-1244).  The caller owns every
 * output buffer; the library owns device memory and file mappings.  One sbx_ctx
 * is used from one host thread at a time; calls are blocking.  The library never
 * falls back to a CPU implementation: without a usable HIP device every compute
 * entry point fails with SBX_ENODEVICE.
 * ========================================================================== */
#ifndef SBX_DEPTH_H
#define SBX_DEPTH_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SBX_OK            0
#define SBX_EINVAL       -1   /* bad argument */
#define SBX_EIO          -2   /* file missing / unreadable / truncated */
#define SBX_EFORMAT      -3   /* not BGZF / BAM / BAI, or corrupt deflate stream */
#define SBX_ENODEVICE    -4   /* no HIP device or HIP runtime failure */
#define SBX_EUNSUPPORTED -5   /* valid request outside the device path (e.g. regex -F filter) */
#define SBX_ENOTSORTED   -6   /* "All files must be coordinate-sorted" (depth.d:1164-1165) */
#define SBX_ENOINDEX     -7   /* "All files must be indexed"           (depth.d:1166)      */
#define SBX_ENOMEM       -8
#define SBX_ERG          -9   /* read group of a read is not in the header (depth.d:246-248) */

typedef struct sbx_ctx sbx_ctx;

/* sizeof() of the named struct of this header as the library was compiled ("sbx_filter", "sbx_regex",
 * "sbx_filter_op", "sbx_region", "sbx_region_stats", "sbx_header_info", "sbx_batch", "sbx_run_stats",
 * "sbx_regex_state", "sbx_shard", "sbx_flagstat_counts", "sbx_sort_stats", "sbx_markdup_stats", "sbx_markdup_stream_stats", "sbx_merge_stats", "sbx_merge_window_stats", "sbx_view_opts", "sbx_view_stats", "sbx_import_stats", "sbx_fixbins_stats", "sbx_fasta_stats", "sbx_slice_stats", "sbx_view_request", "sbx_validate_report", "sbx_validate_stats", "sbx_view_index_stats", "sbx_stream_stats", "sbx_subsample_stats"); 0 for an unknown name.  Lets a foreign-language binding (d/sbx_depth.d, the ctypes
 * binding) verify its struct layouts against the library it loaded. */
size_t sbx_abi_sizeof(const char* type_name);

/* Counter layout of one reference position of one sample, `depth base`
 * (PerBasePrinter.writeColumn, depth.d:495-556): A, C, G, T, other (N/IUPAC/'='),
 * DEL, REFSKIP.  COV = sum of all seven (code 4 counts towards COV but has no column). */
#define SBX_NCOUNTERS 7

enum { SBX_MODE_BASE = 0, SBX_MODE_REGION = 1, SBX_MODE_WINDOW = 2 };   /* depth.d:101-105 */

typedef struct {
    uint32_t ref_id;   /* BamRegion (BioD/bio/std/hts/bam/region.d:28-31) */
    uint32_t start;    /* 0-based, inclusive */
    uint32_t end;      /* 0-based, exclusive */
} sbx_region;

typedef struct {
    int32_t n_ref;             /* reference_sequences.length (reader.d:580-598)            */
    int32_t n_samples;         /* sample_names.length, >= 1 ("*" when there is no @RG)      */
    int32_t n_read_groups;
    int32_t sorted_by_coordinate;  /* header.sorting_order == coordinate (depth.d:1164)     */
    int32_t has_index;         /* bam.has_index (depth.d:1166)                             */
    int32_t reserved;
    uint64_t n_bgzf_blocks;
    uint64_t compressed_bytes;
    uint64_t uncompressed_bytes;
} sbx_header_info;

/* Per region (or window) x sample statistics: PerSampleRegionData (depth.d:609-635).
 * The reference keeps these as 32-bit `uint` (wrap-around is reference behaviour). */
typedef struct {
    uint32_t n_reads;
    uint32_t n_bases;
} sbx_region_stats;

/* The compiled subset of the -F filter language (sambamba/utils/common/filtering.d:86-214,
 * queryparser.d:232-483): a postfix program over flag tests, integer-field comparisons,
 * integer-tag comparisons ([NM] <= 2), tag existence ([XS] == null), string comparisons of tags and of
 * read_name / ref_name / mate_ref_name / strand ([RG] == 'lane1', ref_name != 'chrM') and and / or / not.
 * Built by sbx_compile_filter() from the query string. */
#define SBX_FILTER_MAX_OPS 64
#define SBX_FILTER_STRINGS 512
#define SBX_FILTER_REGEXES 2
#define SBX_REGEX_STATES 64
#define SBX_REGEX_CLASSES 8
/* A regular expression (`read_name =~ /^chr[0-9]+/`) compiled to a Thompson NFA of at most 64 states, so that a
 * state set is one 64-bit mask: type 0 CHAR c, 1 ANY, 2 CLASS classes[c], 3 SPLIT a|b, 4 JMP a, 5 BOL, 6 EOL, 7 MATCH;
 * consuming states continue at a. */
typedef struct { uint8_t type, a, b, c; } sbx_regex_state;
typedef struct {
    uint8_t n_states, n_classes, start, reserved;
    sbx_regex_state states[SBX_REGEX_STATES];
    uint8_t classes[SBX_REGEX_CLASSES][32];
} sbx_regex;
typedef struct {
    uint8_t  kind;     /* 0 FLAG_ANY(mask)  1 CHIMERIC  2 INTCMP  3 AND  4 OR  5 NOT  6 TRUE
                          7 TAGCMP (mask = key chars c0 | c1 << 8; cmp; value)  8 TAGNULL (cmp 4: absent, 5: present)
                          9 TAGSTR (mask = key; cmp; value = string)  10 NAMESTR (read_name; cmp; value = string)
                          11 REFNAME (field 0 ref_name, 1 mate_ref_name; cmp 4 / 5; value = string; resolved against
                             the header when the filter is installed)  12 FALSE  13 SEQSTR / 14 CIGARSTR (sequence / cigar as text)
                          15 REGEX (field 0 read_name 1 sequence 2 cigar 3 tag [mask = key] 4 ref_name 5 mate_ref_name;
                             value = index into sbx_filter.regex)  16 REFSET (internal: 15 on a reference name, resolved
                             against the header when the filter is installed)
                          strings: value = offset into sbx_filter.strings | length << 32 */
    uint8_t  field;    /* INTCMP: 0 ref_id 1 position 2 mapping_quality 3 sequence_length
                                  4 mate_ref_id 5 mate_position 6 template_length 7 avg_base_quality */
    uint8_t  cmp;      /* INTCMP: 0 >  1 <  2 >=  3 <=  4 ==  5 !=                           */
    uint8_t  pad;
    uint32_t mask;
    int64_t  value;
} sbx_filter_op;
typedef struct {
    int32_t n_ops;
    int32_t reserved;
    sbx_filter_op ops[SBX_FILTER_MAX_OPS];
    char strings[SBX_FILTER_STRINGS];
    int32_t n_regex;
    int32_t reserved2;
    sbx_regex regex[SBX_FILTER_REGEXES];
} sbx_filter;

/* ---- codec seam -------------------------------------------------------------
 * Batched replacement of decompressBgzfBlock (block.d:127-216): raw-deflate (RFC 1951,
 * zlib windowBits = -15) payloads comp[comp_off[i] .. +comp_len[i]) are inflated on the
 * device into out[out_off[i] .. +isize[i]); bytes of out[0, max end) outside these ranges
 * are kept (they pass through device memory with the blocks).  All pointers are host memory.  As in the
 * reference's release build the CRC32 is not verified (block.d:187).  Returns
 * SBX_EFORMAT if any payload is not a valid deflate stream of exactly isize[i] bytes. */
int sbx_inflate_blocks(const uint8_t* comp, const uint64_t* comp_off, const uint32_t* comp_len,
                       const uint32_t* isize, uint32_t n_blocks, uint8_t* out, const uint64_t* out_off,
                       char* err, size_t errlen);

/* The write side of the same seam: bgzfCompress (BioD/bio/core/bgzf/compress.d:34-103) for a whole buffer at once.  in[0, n) is
 * cut into 0xFF00-byte pieces (bgzf/constants.d:33), every piece becomes one BGZF block -- 18-byte header with the BC
 * subfield, raw deflate, CRC32, ISIZE -- compressed on the device (one lane per block; any RFC 1951 stream is valid for every
 * BGZF reader, the reference's included).  level is zlib's, as bgzfCompress hands it on: 0 = stored blocks; 1 .. 3 = the fixed
 * Huffman code over greedy hash-table matches; 4 .. 9 and -1 -- Z_DEFAULT_COMPRESSION, the reference's default
 * (bgzfCompress(chunk, level = -1), BamWriter(compression_level = -1)) -- = a dynamic Huffman code per block, from level 7 on over
 * four match candidates per position with lazy evaluation; anything else: SBX_EINVAL.  with_eof != 0 appends the 28-byte EOF
 * block (constants.d:37-49).  All pointers are host
 * memory; *out_len receives the size of the stream (also on SBX_ENOMEM, when cap is too small: n + n / 2048 + 64 is
 * always enough).  device: HIP ordinal or -1. */
int sbx_bgzf_compress(const uint8_t* in, size_t n, int level, int with_eof, int device, uint8_t* out, size_t cap, size_t* out_len,
                      char* err, size_t errlen);
/* BamWriter + BgzfOutputStream (BioD/bio/std/hts/bam/writer.d:67-287, bgzf/outputstream.d): `stream` is the uncompressed BAM
 * byte stream ("BAM\1", header text, references, records); it is written to `path` as BGZF with the EOF block, and -- with_index
 * != 0 -- indexed into path + ".bai" (sbx_build_index). */
int sbx_write_bam(const char* path, const uint8_t* stream, size_t n, int level, int with_index, int device, char* err, size_t errlen);
/* `sambamba index` (createIndex / IndexBuilder, BioD/bio/std/hts/bam/bai/indexing.d:52-366): the BAI of a coordinate-sorted BAM.
 * The file goes through the device pipeline once (inflate, record chain, field decode: position, basesCovered(), stored
 * bin, virtual offsets); chunks per bin, the 16 kbp linear index, the metadata pseudo-bin 37450 and the no-coordinate count
 * are assembled on the host as IndexBuilder.put / finish do.  Bins are written in ascending id order (the reference's order
 * is that of a D associative array).  Like IndexBuilder (one pass over a stream of records, indexing.d:262-316) it does not
 * need the file resident: the blocks go through the device in batches sized by the free device memory, a batch ends in front
 * of the record that straddles its last block boundary, the next one starts with it.
 * SBX_ENOTSORTED when the reads are not coordinate-sorted. */
int sbx_build_index(const char* bam_path, const char* bai_path, int device, char* err, size_t errlen);

/* `sambamba flagstat` (computeFlagStatistics, sambamba/flagstat.d:31-58): per counter [0] the QC-passed and [1] the QC-failed
 * (flag 0x200) records, fields in the order of the printed lines (flagstat.d:131-143). */
typedef struct {
    uint64_t reads[2];
    uint64_t secondary[2];
    uint64_t supplementary[2];
    uint64_t dup[2];
    uint64_t mapped[2];
    uint64_t pair_all[2];
    uint64_t first[2];
    uint64_t second[2];
    uint64_t pair_good[2];
    uint64_t pair_map[2];
    uint64_t single[2];
    uint64_t diff_chr[2];
    uint64_t diff_high[2];
} sbx_flagstat_counts;
/* The counters of every record of a BAM, counted on the device.  Like sbx_build_index it streams the file in batches (the same
 * batch loop) and needs neither a sort order nor a .bai.  SBX_EIO when the file cannot be read, SBX_EFORMAT for a broken BGZF
 * stream, deflate stream or record chain, SBX_ENODEVICE without a device.  device: HIP ordinal or -1. */
int sbx_flagstat(const char* bam_path, int device, sbx_flagstat_counts* out, char* err, size_t errlen);
/* The 13 lines flagstat_main prints for `f` (flagstat.d:131-143; tabular != 0: the -b form), host only.  Percentages are computed
 * as percent() does, in single precision (flagstat.d:66-72).  *len receives the length of the text (without the terminating zero,
 * which is written too); SBX_ENOMEM when buf is null or cap is too small. */
int sbx_format_flagstat(const sbx_flagstat_counts* f, int tabular, char* buf, size_t cap, size_t* len);

/* `sambamba sort` in coordinate order (sambamba/sort.d, default mode): compareCoordinatesAndStrand applied by a stable sort -- ref_id -1
 * last, ascending ref_id, ascending position (signed), forward strand first, ties in file order.  The input needs no sort order and no
 * index.  Records are copied byte for byte; the header text is re-serialised with SO:coordinate (sbx_sort_header_text).  The whole
 * file is sorted on the device, on one of two paths that write the same file byte for byte:
 *   resident  the inflated records fit the device next to one batch of the read pass: they stay there (the record store), the keys
 *             are sorted and the records gathered in order.  n_windows == 0.
 *   windowed  they do not fit (or SBX_SORT_WINDOW_BYTES=<n> is set: tests and measurements, windows of n bytes rounded up to whole
 *             pieces of the output stream): only the keys are sorted -- 36 bytes per record during the sort, 12 afterwards -- the
 *             order becomes one destination per record, and the sorted stream is written window by window, n_windows of them: for
 *             every window the batches of the read pass whose records have a byte in it are inflated and described again (K1 + K2)
 *             and K9d puts each record at its place.  No temporary file, no merge; -m and --tmpdir of sbx-sort stay without
 *             effect.  A file already in order is inflated about twice in all, a shuffled one once per window and once more.  If
 *             the input is not the same in every pass -- the record bytes a window receives do not add up, or a record's length is
 *             not the one its key was taken with -- the call fails with SBX_EIO ("the input changed while it was being sorted") and
 *             the output file is removed.  SBX_ENOMEM only when not even the keys, one minimal read batch and a window of one piece
 *             fit.
 * sbx_sort_bam_by_name and view with two or more listed regions have
 * the resident path only and refuse what does not fit with SBX_ENOMEM (a name order needs the names next to the keys: not built);
 * sbx_markdup and sbx_merge_bam have a windowed path of their own (below); sbx_fixbins, sbx_import_sam and both sinks of view in
 * file order stream such a file (sbx_stream_stats).
 * Milliseconds are device time of the kernels (inflate = K1, index = K2, keys = K9a + the copy into the record store, sort = K9b,
 * gather = output offsets + K9c, deflate = the BGZF encoder + packing), ms_total_wall the wall clock of the call without the index.
 * On the windowed path inflate and index are those of the key pass alone (SBX_TIMING=1 reports the replays in a `[sbx] sort-windows:`
 * line), keys = K9a alone, gather = output offsets + K9d. */
typedef struct {
    uint64_t n_records_in, n_records_out;      /* out < in only with a filter */
    uint64_t inflated_bytes, sorted_stream_bytes, compressed_bytes;
    uint32_t key_bits, n_sort_passes, n_batches, n_windows;   /* key_bits: width of the stretch of key bits in which records differ; n_windows: 0 on the resident path */
    double ms_inflate, ms_index, ms_keys, ms_sort, ms_gather, ms_deflate, ms_total_wall;
} sbx_sort_stats;
/* filter == NULL: every record (not depth's default filter); otherwise only the records the filter admits are written.
 * level as sbx_bgzf_compress.  with_index != 0: out_path + ".bai" too.  stats may be NULL.  SBX_EINVAL when out_path is the input. */
int sbx_sort_bam(const char* in_path, const char* out_path, const sbx_filter* filter, int level, int with_index,
                 int device, sbx_sort_stats* stats, char* err, size_t errlen);
/* The output header text for an input header text (host only; what SamHeader.toSam prints after sort.d:294-298).  *out_len receives
 * the length (without the terminating zero, also with SBX_ENOMEM when cap is too small); SBX_EFORMAT for a text the reference's
 * parser throws on. */
int sbx_sort_header_text(const char* text, size_t n, char* out, size_t cap, size_t* out_len);
/* `sambamba sort -n` (order 1) and `sambamba sort -N` (order 2), with -M when match_mates != 0 (sambamba/sort.d:221-298; the
 * comparators: BioD bio/std/hts/bam/read.d:1493-1621), applied by a stable sort -- whatever compares equal keeps file order.
 *   order 1  compareReadNames: read names as unsigned bytes, a proper prefix first.
 *   order 2  mixedStrCompare: as order 1, but where both names stand at a digit the digit runs compare as numbers, leading zeros
 *            skipped; runs of equal value compare by their number of leading zeros.
 *   match_mates  among equal names: ascending HI tag (absent: 0), then ascending flag.
 * Everything else is sbx_sort_bam: filter, level, the record bytes, the resident store and its SBX_ENOMEM.  The header text is
 * what sbx_sort_header_text gives with SO:queryname in the place of SO:coordinate.  No index is written.
 * Deliberate divergences, both SBX_EFORMAT with the number of such records in err and no output file: a read name that holds a byte
 * outside 0x01..0x7F or is not NUL-terminated (the reference orders such bytes unsigned under -n and signed under -N); with
 * match_mates, an HI tag that is of no integer type (c C s S i I) or does not fit int, or aux fields that run past the record (the
 * reference throws).  SBX_EINVAL for another order.
 * sbx_sort_stats for this call: key_bits is the sum of the widths of the varying bits over the key words sorted (a name's key is
 * a string of 64-bit words; a word in which no two records differ is not sorted at all), n_sort_passes the sum of all K9b passes,
 * ms_keys = K9a + the copy into the record store + K14a (key measure, scan, emit), ms_sort = K14b (the gather of one word) + K9b
 * over all words; the other fields as for sbx_sort_bam. */
int sbx_sort_bam_by_name(const char* in_path, const char* out_path, const sbx_filter* filter, int level, int order, int match_mates,
                         int device, sbx_sort_stats* stats, char* err, size_t errlen);

/* `sambamba markdup` (sambamba/markdup.d): every record is written in input order, byte for byte except flag 0x400, which is set on
 * the duplicates and cleared on every other record that is neither secondary nor supplementary; remove_duplicates != 0 drops the
 * records whose resulting flag has 0x400.  Records with a reference id that are not unmapped, secondary or supplementary take part:
 * pairs (both mates mapped; matched by read name and RG string, 1st with 2nd, 3rd with 4th occurrence in file order) are compared by
 * library, the unclipped 5' coordinates and the strands of both ends, fragments by those of their one end; the best of a group (sum of
 * base qualities >= 15; ties: first in the file) stays unmarked, and a fragment where a paired read lies is always marked.  The header
 * text is re-serialised (sbx_markdup_header_text).  More than 2^32 records are refused with SBX_EUNSUPPORTED.  The duplicates are
 * found on the device, on one of two paths that write the same file byte for byte:
 *   resident  the inflated records fit the device next to one batch of the read pass: they stay there (the record store), the flags
 *             are patched in place and the records gathered into the output.  n_windows == 0.
 *   streamed  they do not fit (or SBX_MARKDUP_WINDOW_BYTES=<n> is set: tests and measurements, windows of n bytes rounded up to whole
 *             pieces of the output stream): no record is kept.  Per record the key pass keeps the figures the decision needs and the
 *             flag, and -- for the records that can pair -- name and RG bytes in a compact key store (K10e), over which the pairing
 *             runs.  The output is the input in input order, so the stream is written window by window, n_windows of them: the
 *             batches of the read pass whose records have a byte in the window are inflated and described again (K1 + K2) and K10f
 *             puts each record at its place with its flag byte patched.  Batches and windows are both consecutive stretches of one
 *             stream: a batch is run again at most once per window it touches, n_batch_runs <= n_batches + n_windows - 1, the file
 *             is inflated about twice in all.  No temporary file.  If the input is not the same in both passes the call fails
 *             with SBX_EIO ("the input changed while its duplicates were being marked") and the output file is removed.  SBX_ENOMEM
 *             only when the per-record arrays (98 bytes per record at the peak), the key store (estimated), one minimal read batch,
 *             the encoder and a window of one piece do not fit together; the message states the bytes needed and free.
 * Milliseconds are device time (inflate = K1, index = K2, ends = K10a + the copy into the record store, pairing = hash sort + K10b,
 * groups = K10c + K10d, gather = output offsets + K9c, deflate = the BGZF encoder + packing), ms_total_wall the wall clock of the
 * call.  On the streamed path inflate and index are those of the key pass alone (the replays: sbx_markdup_stream_stats), ends =
 * K10a + K10e, groups = K10c, gather = the output plan + K10f. */
typedef struct {
    uint64_t n_records_in, n_records_out;
    uint64_t n_end_pairs, n_single_ends, n_unmatched_pairs, n_duplicates;   /* the reference's stderr figures */
    uint64_t inflated_bytes, stream_bytes, compressed_bytes;
    uint32_t n_sort_passes, n_batches;
    double ms_inflate, ms_index, ms_ends, ms_pairing, ms_groups, ms_gather, ms_deflate, ms_total_wall;
} sbx_markdup_stats;
/* level as sbx_bgzf_compress.  pg_command_line: the CL field of the @PG line that is added (NULL: no @PG added).  stats may be NULL.
 * SBX_EINVAL when out_path is the input.  On failure no output file is left behind. */
int sbx_markdup(const char* in_path, const char* out_path, int remove_duplicates, int level,
                const char* pg_command_line, int device, sbx_markdup_stats* stats, char* err, size_t errlen);
/* What the streamed path of sbx_markdup did.  n_windows == 0: the resident path, and every other figure is 0.  struct_size: set by
 * the caller to sizeof(sbx_markdup_stream_stats) and left as it is (a smaller value is SBX_EINVAL).  window_bytes: bytes of the
 * output stream per window; n_batch_runs / n_batches_skipped: batches run again / not run, summed over the windows;
 * key_store_bytes / n_key_records: the key store at its end and the records with an entry in it.  Milliseconds are device time:
 * keys = K10e, plan = output lengths, destinations and the batches' spans, scatter = K10f, inflate_replay / index_replay = K1 / K2
 * of the batches run again.  With SBX_TIMING=1 the same figures are printed in a `[sbx] markdup-stream:` line. */
typedef struct {
    uint32_t struct_size;
    uint32_t n_windows, n_batch_runs, n_batches_skipped;
    uint64_t window_bytes, key_store_bytes, n_key_records;
    double ms_keys, ms_plan, ms_scatter, ms_inflate_replay, ms_index_replay;
} sbx_markdup_stream_stats;
/* sbx_markdup with the figures of the streamed path: stream_stats may be NULL, and sbx_markdup is this call with NULL. */
int sbx_markdup_run(const char* in_path, const char* out_path, int remove_duplicates, int level,
                    const char* pg_command_line, int device, sbx_markdup_stats* stats, sbx_markdup_stream_stats* stream_stats,
                    char* err, size_t errlen);
/* The output header text for an input header text (host only): SamHeader.toSam of the input -- SO kept when it is unsorted, coordinate
 * or queryname -- with "@PG ID:sambamba CL:<pg_command_line> PP:<last @PG> VN:1.0" added unless pg_command_line is NULL or an @PG
 * with ID:sambamba exists.  Lengths and errors as sbx_sort_header_text. */
int sbx_markdup_header_text(const char* text, size_t n, const char* pg_command_line, char* out, size_t cap, size_t* out_len);

/* `sambamba merge` (sambamba/merge.d) for coordinate-sorted inputs: the headers are merged as SamHeaderMerger does (sbx_merge_header_text),
 * every record gets its reference ids renumbered into the merged dictionary -- ref_id AND next_ref_id; the reference renumbers only
 * ref_id -- and the value of its RG:Z / PG:Z tag replaced when the merged header renamed that id, and the records of all inputs are
 * sorted by coordinate with sbx_sort_bam's stable sort: ties (same reference, position and strand) come out lower input first, then
 * in file order.  The inputs are not assumed to BE sorted: the output is sorted whatever the records say.  filter is applied to the
 * records as they are in their input.  More than 2^32 records and inputs sorted by read name are refused with SBX_EUNSUPPORTED,
 * fewer than two inputs, more than SBX_MERGE_MAX_INPUTS, or an output that is one of the inputs with SBX_EINVAL.  The merge runs on
 * one of two paths that write the same file byte for byte:
 *   resident  the inflated records of ALL inputs fit the device next to one batch of the read pass: they stay there (the record
 *             store), the keys are sorted and the records gathered in order.  sbx_merge_window_stats is all zeros.
 *   windowed  they do not fit (or SBX_MERGE_WINDOW_BYTES=<n> is set: tests and measurements, windows of n bytes rounded up to whole
 *             pieces of the output stream; anything but a positive decimal number counts as unset; the file written does not depend
 *             on n): the key pass visits every input in turn and keeps only key and NEW length of every record -- 36 bytes per
 *             record during the sort, 12 afterwards; every malformed-record refusal and the 2^32 cap are met in this pass, before the
 *             output file receives a byte.  The order becomes one destination per record, and the merged stream is written window
 *             by window: per window the inputs that have a batch with a byte in it are opened again in input order, ONE AT A TIME,
 *             those batches are inflated and described again (K1 + K2), and K9d (an input nothing changes in) or K11a + K11c (a
 *             rewritten one: the record's pieces -- fixed part, source stretches, new ids -- each clipped to the window) put the
 *             bytes in place.  Coordinate-sorted inputs go to ascending, disjoint stretches of the output, so a batch is run again
 *             at most once per window it touches, n_batch_runs <= n_batches + n_inputs * (n_windows - 1), and every input is
 *             inflated about twice in all; inputs that are not sorted cost up to one pass per window.  No temporary file.  If an
 *             input is not the same in both passes the call fails with SBX_EIO ("the input changed while it was being merged") and
 *             the output file is removed.  SBX_ENOMEM only when the keys, K11's scratch of one batch, one minimal read batch, the
 *             encoder and a window of one piece do not fit together; the message states the bytes needed, part by part, and free.
 *             No set of inputs larger than the device has been merged: the path is exercised only through the hook.
 * n_records_rewritten: records in which a
 * reference id or a tag value changed; bytes_grown: bytes of the records written minus bytes of the same records as read.
 * Milliseconds are device time (inflate = K1, index = K2, rewrite = K11 or, for an input nothing changes in, K9a + the copy into
 * the record store, sort = K9b, gather = output offsets + K9c, deflate = the BGZF encoder + packing), ms_total_wall the wall clock of
 * the call without the index.  On the windowed path inflate and index are those of the key pass alone (the replays:
 * sbx_merge_window_stats), rewrite = K9a alone or K11a + the key-only emit, gather = output offsets + K9d-1/2 + the scatters.
 * How closely a record is checked depends on whether its input is rewritten.  An input with a renumbered reference or a renamed id
 * goes through K11, which checks the fixed part and every aux field against block_size and refuses the call with SBX_EFORMAT.  An
 * input nothing changes in is copied and checked as sbx_sort_bam checks a record: block_size against the batch, ref_id against the
 * input's dictionary (with a filter: the verdict of the filter pass); a malformed aux field is copied as it is.  Which of the two
 * an input gets depends on the other inputs' headers.  SBX_MERGE_FORCE_REWRITE=1 sends every input through K11. */
#define SBX_MERGE_MAX_INPUTS 1024
typedef struct {
    uint64_t n_records_in, n_records_out;      /* summed over the inputs; out < in only with a filter */
    uint64_t n_records_rewritten;
    int64_t bytes_grown;
    uint64_t inflated_bytes, merged_stream_bytes, compressed_bytes;
    uint32_t n_inputs, key_bits, n_sort_passes, n_batches;
    double ms_inflate, ms_index, ms_rewrite, ms_sort, ms_gather, ms_deflate, ms_total_wall;
} sbx_merge_stats;
/* filter, level, with_index, stats as sbx_sort_bam.  On failure no output file is left behind. */
int sbx_merge_bam(const char* out_path, const char* const* in_paths, int n_inputs, const sbx_filter* filter, int level, int with_index,
                  int device, sbx_merge_stats* stats, char* err, size_t errlen);
/* What the windowed path of sbx_merge_bam did.  n_windows == 0: the resident path, and every other figure is 0.  struct_size: set
 * by the caller to sizeof(sbx_merge_window_stats) and left as it is (a smaller value is SBX_EINVAL).  window_bytes: bytes of the
 * merged stream per window; n_batch_runs / n_batches_skipped: batches run again / not run, summed over the windows and inputs;
 * n_input_opens: times an input was opened again for a window (an input that serves consecutive windows alone stays open).
 * Milliseconds are device time: dest = K9d-1 + K9d-2, scatter = K9d-3 and K11a + K11c, inflate_replay / index_replay = K1 / K2 of the
 * batches run again.  With SBX_TIMING=1 the same figures are printed in a `[sbx] merge-windows:` line. */
typedef struct {
    uint32_t struct_size;
    uint32_t n_windows, n_batch_runs, n_batches_skipped, n_input_opens;
    uint64_t window_bytes;
    double ms_dest, ms_scatter, ms_inflate_replay, ms_index_replay;
} sbx_merge_window_stats;
/* sbx_merge_bam with the figures of the windowed path: window_stats may be NULL, and sbx_merge_bam is this call with NULL. */
int sbx_merge_bam_run(const char* out_path, const char* const* in_paths, int n_inputs, const sbx_filter* filter, int level, int with_index,
                      int device, sbx_merge_stats* stats, sbx_merge_window_stats* window_stats, char* err, size_t errlen);
/* The merged header text for n header texts in input order (host only).  Lengths as sbx_sort_header_text; SBX_EFORMAT for a text the
 * reference's parser throws on, SBX_EINVAL when the sorting orders forbid the merge or one reference name has two lengths,
 * SBX_EUNSUPPORTED for queryname.  The message of a refusal is written to out when it fits. */
int sbx_merge_header_text(const char* const* texts, const size_t* lens, int n, char* out, size_t cap, size_t* out_len);

/* `sambamba view` (sambamba/view.d), the record selection with its two cheapest sinks: a count (-c) and a BAM (-f bam).  A record is
 * selected when ALL of these hold (a part that was not asked for always holds):
 *   filter       the -F program (NULL: every record, not depth's default filter);
 *   num-filter   (flag & flags_set) == flags_set && (flag & flags_unset) == 0            (FlagBitFilter, filtering.d:176-187);
 *   subsample    low 32 bits of the 64-bit FNV-1a over the read name (without its NUL) and the 8 bytes of `seed`, least significant
 *                first, < (uint64)(4294967296.0 * fraction); mates share a name and so a verdict (SubsampleFilter, filtering.d:340-371);
 *   regions      the record overlaps a region: ref_id == r && pos < end && (pos > start || pos + basesCovered > start), the
 *                predicate of the reference's random access (randomaccessmanager.d:397-460) -- a record that covers no bases is
 *                selected strictly inside a region and not at pos == start.
 * Regions are given as the reference gets them: `regions` are the strings of the command line ("chr", "chr:beg-end" with a 1-based
 * beg, and "*", which stands for the records with ref_id < 0), resolved against the header of the input; an unknown name is
 * SBX_EINVAL and named in the message.  The output is then the concatenation, in the listed order, of each region's records in file
 * order: a record that overlaps two listed regions appears -- and is counted -- twice.  At most SBX_VIEW_MAX_REGIONS may be listed
 * (SBX_EINVAL beyond).  `bed_path` (NULL or "": none) names a BED file instead: its regions are sorted and merged as parseBed leaves
 * them and every record that overlaps any of them is output once, in file order.  Both at once are SBX_EINVAL.
 * Deliberate divergences: no .bai is needed and the input need not be sorted -- the result is defined by the predicate over all
 * records in file order, which is what the reference yields for a sorted, indexed file -- and -L uses the same predicate whatever
 * the header's SO says.  These calls read the whole file even for a small region; sbx_view_run_indexed reads what the .bai names.
 * Milliseconds are device time (inflate = K1, index = K2, select = K12a [+ the copy into the record store and the scans of its
 * counts for BAM output], emit = K12b, sort = K9b over the region indices + the composition, gather = output offsets + K9c,
 * deflate = the BGZF encoder + packing), ms_total_wall the wall clock of the call without the index. */
#define SBX_VIEW_MAX_REGIONS 1024
typedef struct {
    uint16_t flags_set, flags_unset;           /* --num-filter=i1/i2 (sbx_view_num_filter); 0, 0: every record */
    int32_t subsample;                         /* != 0: -s fraction with --subsampling-seed=seed */
    double fraction;                           /* negative or NaN: SBX_EINVAL */
    uint64_t seed;
} sbx_view_opts;
typedef struct {
    uint64_t n_records_in, n_records_selected, n_entries_out;    /* entries: selected records, one per listed region they overlap */
    uint64_t inflated_bytes, stream_bytes, compressed_bytes;     /* the last two: BAM output only */
    uint32_t n_regions, n_sort_passes, n_batches, reserved;
    double ms_inflate, ms_index, ms_select, ms_emit, ms_sort, ms_gather, ms_deflate, ms_total_wall;
} sbx_view_stats;
/* -c: *count = the number of entries.  Streams the file in batches like sbx_flagstat; nothing is stored, so a file larger than the
 * device works.  opts may be NULL (no num-filter, no subsampling); stats may be NULL. */
int sbx_view_count(const char* in_path, const sbx_filter* filter, const sbx_view_opts* opts, const char* const* regions, size_t n_regions,
                   const char* bed_path, int device, uint64_t* count, sbx_view_stats* stats, char* err, size_t errlen);
/* -f bam: the header text of sbx_markdup_header_text (SO kept; "@PG ID:sambamba CL:<pg_command_line> ..." added unless
 * pg_command_line is NULL or an @PG ID:sambamba exists), the selected records byte for byte in the order defined above, the EOF
 * block; an empty selection writes header + EOF.  out_path NULL or "-": stdout (never indexed, never removed).  level as
 * sbx_bgzf_compress; with_index != 0: out_path + ".bai" too (the selection of a sorted input through bed_path is sorted).  The
 * records of the file are resident on the device as for sbx_sort_bam: one whose inflated records do not fit is refused with
 * SBX_ENOMEM, more than 2^32 output entries with SBX_EUNSUPPORTED, an out_path that is the input with SBX_EINVAL.  On failure no
 * output file is left behind. */
int sbx_view_bam(const char* in_path, const char* out_path, const sbx_filter* filter, const sbx_view_opts* opts, const char* const* regions,
                 size_t n_regions, const char* bed_path, const char* pg_command_line, int level, int with_index, int device,
                 sbx_view_stats* stats, char* err, size_t errlen);
/* -f sam, the reference's default: one line per entry (BamRead.toSam, BioD bio/std/hts/bam/read.d:695-760; tags as TagValue.toSam,
 * floats as C's "%g" of the value widened to double), in the order sbx_view_bam writes the entries, formatted on the device (K13).
 * with_header != 0 (-h): the header text of sbx_view_bam comes first, with its @PG line, no blank line added; 0: no header.
 * out_path NULL or "-": stdout.  A selected record the reference dies on with a range error -- ref_id or mate_ref_id outside
 * [-1, n_ref), a tag of unknown type, a tag value that runs past the record, a Z / H without NUL -- is counted and the call
 * fails with SBX_EFORMAT before a byte is written; a record that is not selected is not looked at.  The file is resident as for
 * sbx_view_bam (SBX_ENOMEM when it does not fit); an out_path that is the input is SBX_EINVAL; on failure no output file is left.
 * stats: stream_bytes = bytes of record text (header excluded), compressed_bytes = 0, ms_deflate = 0, ms_gather = K13a + K13b. */
int sbx_view_sam(const char* in_path, const char* out_path, const sbx_filter* filter, const sbx_view_opts* opts, const char* const* regions,
                 size_t n_regions, const char* bed_path, const char* pg_command_line, int with_header, int device,
                 sbx_view_stats* stats, char* err, size_t errlen);
/* One entry point for the three sinks, and the way in for options sbx_view_opts (whose size is fixed) cannot take.  The request
 * begins with its own size as the caller compiled it: fields the caller's struct does not have are 0 here, so the struct grows at its
 * end without new functions; a struct_size that ends in front of `device`'s end is SBX_EINVAL.  sink selects sbx_view_count (*count
 * receives the entries; out_path, pg_command_line, level, with_index, with_header unused), sbx_view_bam (with_header unused) or
 * sbx_view_sam (level, with_index unused); those three are this call with valid_only = 0, and every field means what their
 * argument of the same name means.  count may be NULL for the other sinks.
 * valid_only != 0 (`view -v`): K19 (sbx_validate_bam's kernel) runs on every batch in front of the selection and a record whose
 * mask is not 0 is not selected, whatever else it passes -- also a record with a malformed fixed part or malformed tags, which
 * without the option fails the call with SBX_EFORMAT when it is selected.  stats.ms_select includes the time of K19. */
#define SBX_VIEW_SINK_COUNT 0
#define SBX_VIEW_SINK_BAM 1
#define SBX_VIEW_SINK_SAM 2
typedef const char* sbx_cstr;
typedef const char* const* sbx_cstr_list;
typedef const sbx_filter* sbx_filter_ptr;
typedef const sbx_view_opts* sbx_view_opts_ptr;
typedef struct {
    uint32_t struct_size;                      /* sizeof(sbx_view_request) */
    int32_t sink;                              /* SBX_VIEW_SINK_* */
    sbx_cstr in_path;
    sbx_cstr out_path;
    sbx_filter_ptr filter;
    sbx_view_opts_ptr opts;
    sbx_cstr_list regions;
    size_t n_regions;
    sbx_cstr bed_path;
    sbx_cstr pg_command_line;
    int32_t level, with_index, with_header, device;
    int32_t valid_only, reserved;
} sbx_view_request;
int sbx_view_run(const sbx_view_request* request, uint64_t* count, sbx_view_stats* stats, char* err, size_t errlen);
/* sbx_view_run that reads only the blocks the .bai names for the regions of the request.  The calls above keep reading the whole
 * file: they need no .bai and promise n_records_in = the records of the file; this one is the way to a cost that follows the region.
 * index_mode: SBX_VIEW_INDEX_OFF is sbx_view_run; SBX_VIEW_INDEX_REQUIRED fails with SBX_ENOINDEX when the request has a region or a
 * BED file and the input has no .bai; SBX_VIEW_INDEX_AUTO then reads the whole file.  Without region and BED file there is nothing to
 * restrict: every mode is OFF, and blocks_read == blocks_in_file.
 * On the indexed path the merged BAI chunks of all regions of the call (getGroupChunks, randomaccessmanager.d:247-294; for `*` the
 * stretch from the first record without a reference to the end of the stream) are joined where they share a block or lie at most
 * one block apart, and the union is read once, in batches of SBX_INDEX_BATCH_BYTES as for the other passes; the selection over the
 * described records is the one of sbx_view_run, so counts, BAM and SAM bytes are those of the whole-file pass.  stats.n_records_in
 * is then the number of records described and stats.inflated_bytes the bytes inflated (a block at the cut between two batches of one
 * run is inflated twice); every other field means what it means there.  The record store of the BAM and SAM sinks holds the inflated
 * bytes of the runs' blocks (index.inflated_bytes_read), and SBX_ENOMEM names that figure.
 * The result equals the predicate over all records only when the file is in coordinate order, so every batch read is checked: a
 * record with a reference whose (ref_id, pos) lies in front of the record read before it is SBX_ENOTSORTED.  A .bai whose number of
 * references differs from the header's is SBX_EFORMAT, and so is a chunk offset that lands on no record (K2's chain check).  On
 * failure no output file is left.
 * index (may be NULL): blocks_in_file = BGZF blocks of the input in front of the first empty one (the EOF block); blocks_read, runs, compressed_bytes_read,
 * inflated_bytes_read = the distinct blocks of the joined runs, their number, the file bytes from the first to the last block of
 * every run, and what they inflate to; ms_plan = host time from the regions to the run list. */
typedef struct {
    uint64_t blocks_in_file, blocks_read, runs, compressed_bytes_read, inflated_bytes_read;
    double ms_plan;
} sbx_view_index_stats;
#define SBX_VIEW_INDEX_OFF 0
#define SBX_VIEW_INDEX_REQUIRED 1
#define SBX_VIEW_INDEX_AUTO 2
int sbx_view_run_indexed(const sbx_view_request* request, int index_mode, uint64_t* count, sbx_view_stats* stats,
                         sbx_view_index_stats* index, char* err, size_t errlen);
/* What the streamed path of a command whose output order is the input order did (sbx_view_run_streamed, sbx_fixbins_run).  All
 * zeros: the resident path.  The streamed path keeps no record store: while a batch of the read pass is on the device K21 puts its
 * selected records into one staging window of the output stream, and a full window goes through the BGZF encoder into the file, so
 * a file larger than the device works and the file written is the resident path's byte for byte.  It is taken when the resident
 * store would be refused with SBX_ENOMEM, or when SBX_STREAM_WINDOW_BYTES=<n> is set (tests and measurements: a window of n bytes
 * rounded up to whole pieces of the output stream; anything but a positive decimal counts as unset).  n_windows: windows handed to
 * the encoder; window_bytes: bytes of the output stream per window; n_pack_launches: launches of K21's copy kernel (one per batch
 * and window the batch has bytes in); ms_pack: device time of K21.  SBX_ENOMEM is left for one minimal read batch, the encoder and a
 * window of one piece not fitting; the message states the bytes needed and free.  With SBX_TIMING=1 the same figures are printed in
 * a `[sbx] stream:` line. */
typedef struct {
    uint64_t window_bytes, n_pack_launches;
    uint32_t n_windows, reserved;
    double ms_pack;
} sbx_stream_stats;
/* sbx_view_run_indexed with the figures of the streamed path: stream_stats may be NULL, and sbx_view_run_indexed is this call with
 * NULL.  The BAM and the SAM sink stream when the output order is the file order -- no region, exactly one listed region, or a BED
 * file -- with or without filter, num-filter, subsampling and valid_only, on the whole-file and on the indexed pass.  Two or more
 * listed regions order the output by region and keep the resident store and its SBX_ENOMEM.  The SAM sink has no window: per batch
 * K12b, K13a and K13b run over the records where K1 left them, n_windows counts the pieces of text written, window_bytes is the
 * piece size, n_pack_launches and ms_pack stay 0.  On the streamed path a malformed selected record of a later batch is met after
 * earlier windows or pieces were written: the call fails with the same code and message, an output file is removed, an output on
 * stdout has received bytes by then. */
int sbx_view_run_streamed(const sbx_view_request* request, int index_mode, uint64_t* count, sbx_view_stats* stats,
                          sbx_view_index_stats* index, sbx_stream_stats* stream_stats, char* err, size_t errlen);

/* ---- validate: which records of a BAM are valid, and why not (`sambamba view -v`; `sambamba validate` is an empty stub) ----
 * A record is valid when isValid of BioD bio/std/hts/bam/validation/alignment.d says so.  K19 evaluates every class of error on its
 * own, so a record can be counted in several; class k, in this order: name-empty, name-chars (a byte < '!', > '~' or '@'), position
 * (outside [-1, 2^29 - 2]), qualities (neither all 0xFF nor all <= 93), cigar-hard (H strictly inside), cigar-soft (S strictly inside
 * once one H is taken off either end), cigar-length (l_seq > 0 differs from the M I S = X lengths), tag-value (a tag breaks a rule of
 * its type or of its predefined key), tag-duplicate (two tags share a key), malformed.  Deliberate divergence: `malformed` -- a
 * block_size below 32, l_read_name 0, name + CIGAR + sequence + qualities past block_size, a tag of unknown type, a B array of
 * unknown element type, a tag value past the record, a Z / H without NUL -- makes the reference read past the record or throw; here
 * the record is invalid.  A malformed fixed part is counted in `malformed` alone; with malformed tags the other classes cover what
 * lies in front of the break.
 * sbx_validate_bam streams the file in batches like sbx_flagstat (any BAM, sorted or not, indexed or not; nothing is resident;
 * SBX_INDEX_BATCH_BYTES applies); what breaks the record chain is SBX_EFORMAT as there.  first_*: the first invalid record in file
 * order, meaningful when n_invalid > 0 -- its 0-based ordinal, its mask (bit k = class k) and its name without the NUL (at most 254
 * bytes, not terminated; length 0 when l_read_name is 0 or 32 + l_read_name exceeds block_size).  Milliseconds are device time (valid = K19). */
#define SBX_VALIDATE_CLASSES 10
typedef struct {
    uint64_t n_records, n_invalid;
    uint64_t class_count[SBX_VALIDATE_CLASSES];
    uint64_t first_ordinal;
    uint32_t first_mask, first_name_len;
    char first_name[256];
} sbx_validate_report;
typedef struct {
    double ms_inflate, ms_index, ms_valid, ms_total_wall;
    uint64_t inflated_bytes;
    uint32_t n_batches, reserved;
} sbx_validate_stats;
int sbx_validate_bam(const char* in_path, int device, sbx_validate_report* report, sbx_validate_stats* stats, char* err, size_t errlen);
/* The report of `sbx-validate` for one file (host only), tab-separated lines: "file" path, "records" n, "invalid" m, the ten classes
 * by name with their counts, and when m > 0 "first-invalid" with the ordinal, the name (bytes outside [!-~] and '\\' as \xHH) and the
 * comma-joined names of its classes.  buf / cap / len as sbx_format_flagstat. */
int sbx_format_validate_report(const char* path, const sbx_validate_report* report, char* buf, size_t cap, size_t* len);
/* ---- `sambamba slice` (sambamba/slice.d): regions of an indexed BAM copied with their BGZF blocks reused ----
 * The records of in_path in file order are i = 0 .. n-1; record i occupies [u_i, u_{i+1}) of the inflated stream.  For a region
 * (r, beg, end): R1 = the records with ref == r, pos < beg and pos + basesCovered > beg; first_ge(x) = the first record with ref < 0,
 * ref > r, or ref == r and pos >= x (n when there is none); a = u[first_ge(beg)], b = u[first_ge(end)].  The output is the header
 * bytes of the input unchanged (no @PG), then for every region in the order given the records of R1 and the stream bytes [a, b), then
 * the EOF block; two regions that overlap give their common records twice.  Every BGZF block of the input that lies wholly inside
 * [a, b) is written as it is in the file and is neither uploaded nor inflated; the head [a, next block start), the tail [start of b's
 * block, b) and R1 are compressed on the device at the default level (an empty piece writes no block).  Only the blocks the .bai names
 * for the two edge positions of a region are read.  `regions` as for sbx_view_bam ("chr", "chr:beg-end", at most SBX_VIEW_MAX_REGIONS);
 * "*" alone gives the header and everything from the first record without a reference on, "*" next to other regions is SBX_EINVAL.
 * `bed_path` (NULL or "": none) names a BED file instead (merged, in (reference, start) order, unknown contigs dropped); both, or
 * neither, are SBX_EINVAL.  out_path NULL or "-": stdout.  SBX_ENOINDEX without a .bai, SBX_EINVAL for an unknown reference (named), an
 * empty region or an out_path that is the input, SBX_EUNSUPPORTED for more than 2^32 R1 records.  On failure no output file is left.
 * Deliberate divergences from the reference's code, which departs from its own header comment: a is the first record with pos >= beg
 * (the code also copies the records behind the last R1 record that start in front of beg and do not reach it); when reads reach
 * `end` but none of the contig starts at or behind it, b is the end of the contig's records (the code ends the copy in front of the
 * last such read and loses it); FASTA input (-F) is not provided.
 * stats: stream_bytes = inflated bytes that went through the device writer (the header included), compressed_bytes = what it wrote
 * (the EOF block and the copied blocks not included), blocks_inflated = blocks of the edge runs (the header's blocks, inflated at
 * open, not included), ms_read = K1 + K2 of the edge runs, ms_select = K18, ms_write / ms_total_wall = wall clock. */
typedef struct {
    uint64_t n_regions, records_r1, blocks_inflated, blocks_copied, bytes_copied, stream_bytes, compressed_bytes;
    double ms_read, ms_select, ms_write, ms_total_wall;
} sbx_slice_stats;
int sbx_slice_bam(const char* in_path, const char* out_path, const char* const* regions, size_t n_regions, const char* bed_path, int device,
                  sbx_slice_stats* stats, char* err, size_t errlen);
/* "i1/i2" of --num-filter (view.d:271-277; host only): either number may be missing ("4/", "/4", "3", ""), each is an unsigned
 * 16-bit decimal; anything else is SBX_EINVAL. */
int sbx_view_num_filter(const char* text, uint16_t* flags_set, uint16_t* flags_unset);
/* The text of `view -I` for an open file (outputReferenceInfoJson, view.d:98-118; host only), exactly as the reference's code
 * prints it -- the quote in front of the brace included: [{"name":"chr1","length":1000}] is what a correct writer would print,
 * ["{name":"chr1","length":1000}] plus a newline is what comes out.  Lengths as sbx_sort_header_text. */
int sbx_view_reference_info(sbx_ctx*, char* out, size_t cap, size_t* out_len);

/* ---- import: SAM text in, BAM out (`sambamba view -S -f bam in.sam -o out.bam`, view.d:216-218, 292-311) ----
 * The lines are parsed on the device (K15) by the grammar of parseAlignmentLine (BioD bio/etc/ragel/sam_alignment.rl): QNAME, FLAG,
 * RNAME, POS, MAPQ, CIGAR, RNEXT, PNEXT, TLEN, SEQ, QUAL and the tags A i f Z H B; the bin is reg2bin of POS and the reference bases
 * of the CIGAR, integer tags take the smallest type, floats are the correctly rounded binary32 of their text (what glibc's strtof
 * returns).  in_path: a path or "-" (stdin); it is read sequentially, so a pipe works.  The header is the run of lines starting with
 * '@' at the top; the output header is what sbx_view_bam writes for a BAM with this text and these @SQ lines (pg_command_line as there).
 * out_path NULL or "-": stdout (never indexed).  level as sbx_bgzf_compress; with_index != 0: out_path + ".bai" too.
 * Deliberate divergences: the reference recovers silently from an invalid field (it skips to the next tab, drops the tag, fills
 * the qualities with 0xFF); here any line outside the grammar -- a QUAL whose length is not SEQ's (other than a lone '*'), a
 * reference name the header lacks, a '\r', an empty line included -- fails the call with SBX_EFORMAT, the message carrying the
 * number of such lines and the 1-based number of the first, and no output file is left.  Two texts sbx_view_sam writes and the
 * grammar lacks are read: "B:<type>," (an array without elements) and "-nan" (0xFFC00000).
 * The records stay resident on the device while they fit, in a store that grows chunk by chunk.  When it cannot grow -- the grown store
 * does not fit next to the old one, or would leave no room for the streamed path -- the call switches: the header and the records kept
 * so far go through one staging window of the output stream into the file, the store is freed, and from then on K15d writes every
 * chunk's records into the window directly (sbx_stream_stats, sbx_import_sam_run below).  Nothing is written before the switch; the file
 * is the resident path's byte for byte.  A bad line met behind the switch is the same SBX_EFORMAT with the same message; an output file
 * is removed, an output on stdout has received bytes by then.  SBX_STREAM_WINDOW_BYTES takes the streamed path from the first chunk
 * (as for view and fixbins), SBX_IMPORT_STORE_BYTES=<n> switches at the chunk whose records would bring the store past n bytes (both for
 * tests; anything but a positive decimal counts as unset).  SBX_ENOMEM, naming the bytes needed part by part and the bytes free, only
 * when not even a window of one piece, the encoder, two text chunks and the arrays of one chunk fit; more than 2^32 records are
 * SBX_EUNSUPPORTED; an out_path that is the input is SBX_EINVAL.  The text is uploaded in
 * chunks cut at line ends (64 MiB, not tuned; SBX_IMPORT_CHUNK_BYTES overrides it for tests); the output does not depend on the size.
 * n_lines: lines behind the header; text_bytes: their bytes.  Milliseconds are device time (index = K15a, measure = K15b + scan,
 * emit = K15c, deflate = the BGZF encoder + packing), ms_total_wall the wall clock of the call without the index. */
typedef struct {
    uint64_t n_lines, n_records, text_bytes, stream_bytes, compressed_bytes;
    uint32_t n_chunks, reserved;
    double ms_index, ms_measure, ms_emit, ms_deflate, ms_total_wall;
} sbx_import_stats;
int sbx_import_sam(const char* in_path, const char* out_path, const char* pg_command_line, int level, int with_index, int device,
                   sbx_import_stats* stats, char* err, size_t errlen);
/* sbx_import_sam with the figures of the streamed path (sbx_stream_stats above; n_pack_launches counts the launches of K15d, ms_pack
 * their time, which is ms_emit too): stream_stats may be NULL, and sbx_import_sam is this call with NULL.  All zero when the records
 * stayed resident. */
int sbx_import_sam_run(const char* in_path, const char* out_path, const char* pg_command_line, int level, int with_index, int device,
                       sbx_import_stats* stats, sbx_stream_stats* stream_stats, char* err, size_t errlen);

/* ---- index, fixbins (`sambamba index [-c] [-F]`, index.d; `sambamba fixbins`, fixbins.d) ----
 * sbx_index_bam with check_bins == 0 is sbx_build_index: the same file, the same errors.  With check_bins != 0 (`index -c`) the same
 * pass (K16a) also compares the stored bin of every PLACED record (ref_id >= 0 and pos >= 0) with reg2bin(pos, pos + basesCovered())
 * in the reference's int arithmetic (bin.d:82-92; an unmapped read covers nothing).  A mismatch fails the call with SBX_EFORMAT and
 * the reference's message for the first such record in file order -- "Bin in read with name 'NAME' is set incorrectly (B instead of
 * expected E)" -- followed by "; N record(s) of the file have a wrong bin"; no .bai is written.  Deliberate divergences: the
 * reference never checks the first placed read of a file (IndexBuilder.put returns before checkThatBinIsCorrect while _first_read is
 * set), here it is checked; an unsorted file is SBX_ENOTSORTED as without the check, whichever of the two faults comes first. */
int sbx_index_bam(const char* bam_path, const char* bai_path, int check_bins, int device, char* err, size_t errlen);
/* `sambamba fixbins`: every record of in_path, placed or not, mapped or not, gets bin = reg2bin(pos, pos + basesCovered()) (4680 for
 * ref_id -1, pos -1); nothing else changes: header text and reference list are the input's byte for byte (no @PG), the records keep
 * their order, an EOF block ends the file.  level as sbx_bgzf_compress.  The records are resident on the device as for sbx_markdup
 * (K16b patches the two bytes in the store): SBX_ENOMEM when they do not fit, SBX_EINVAL when out_path is the input, SBX_EFORMAT for
 * a record whose name and CIGAR run past its block_size, SBX_EUNSUPPORTED for more than 2^32 records.  On failure no output file is
 * left.  Milliseconds are device time (bins = K16b), ms_total_wall the wall clock of the call. */
typedef struct {
    uint64_t n_records, n_bins_changed, inflated_bytes, stream_bytes, compressed_bytes;
    uint32_t n_batches, reserved;
    double ms_inflate, ms_index, ms_bins, ms_gather, ms_deflate, ms_total_wall;
} sbx_fixbins_stats;
int sbx_fixbins(const char* in_path, const char* out_path, int level, int device, sbx_fixbins_stats* stats, char* err, size_t errlen);
/* sbx_fixbins with the figures of the streamed path (sbx_stream_stats above): stream_stats may be NULL, and sbx_fixbins is this call
 * with NULL.  On the streamed path K16b computes the bin of every record of a batch and K21 writes the two bytes while it copies the
 * record into the window: the patched record never exists in a store.  ms_gather is 0 there (the copy is ms_pack). */
int sbx_fixbins_run(const char* in_path, const char* out_path, int level, int device, sbx_fixbins_stats* stats,
                    sbx_stream_stats* stream_stats, char* err, size_t errlen);

/* ---- subsample: cap the coverage by dropping reads (`sambamba subsample --type fasthash --max-cov N [-r]`, subsample.d) ----
 * The reference's command is unfinished (it prints debug text, never drops a read and ends in "Pileup buffer is full"); its header
 * comment and usage text are the specification, and this is the definition:
 * A record is COUNTED when its flag has none of 0x4, 0x200, 0x400, 0 <= ref_id < n_ref and 0 <= pos < LN[ref_id].  Its span is
 * [pos, e), e = min(pos + max(basesCovered, 1), LN) (basesCovered: the M D N = X lengths added up in 32 bits; a sum past 2^31 is
 * clipped by LN).  c_r(p) is the number of counted records of reference r with pos <= p < e, over the WHOLE file -- so the result
 * does not depend on the order of the records, the input need not be sorted and no .bai is needed.  A counted record has
 * cov = max(c(pos), c(e - 1)) >= 1 and h = the low 32 bits of the 64-bit FNV-1a hash `view -s` uses, over its name without the NUL
 * and a seed of 0; it is KEPT iff cov <= max_cov or (uint64)h * cov < (uint64)max_cov << 32 (exact integer arithmetic).  Mates share
 * h but not cov, so their verdicts may differ (as in VariantBam).  Records that are not counted are always kept.
 * The output is in file order; its header is the input's with the "@PG ID:sambamba CL:<pg_command_line>" line of
 * sbx_markdup_header_text (SO kept; NULL: no @PG line).  remove != 0: dropped records are left out.  remove == 0: every record is
 * written and a dropped one gets flag bit 0x200 (the reference's "mark as bad quality"; depth's default filter and a second
 * subsample then ignore it).  Nothing else changes, bins included.  level as sbx_bgzf_compress (the reference hard-codes 9);
 * with_index != 0: out_path + ".bai" too, a pass of its own.
 * The file is read twice in batches (K22a marks span ends in a coverage array of one uint32 per reference position plus one per
 * reference, K22b scans it, K22c judges) and always written through the streamed writer (sbx_stream_stats above;
 * SBX_INDEX_BATCH_BYTES, SBX_STREAM_WINDOW_BYTES and SBX_BGZF_PIECE_BLOCKS apply and change no byte).  SBX_EINVAL: max_cov <= 0, a
 * bad level, out_path is the input.  SBX_EUNSUPPORTED: more than 2^32 records.  SBX_EFORMAT: a record whose name and CIGAR run
 * past its block_size.  SBX_ENOMEM: the coverage array next to one minimal read batch, the encoder and a window of one piece does
 * not fit; the message states the bytes needed and free and the coverage array's share.  On failure no output file is left.
 * n_over: counted records with cov > max_cov; n_dropped: those of them the hash drops; n_written: records in the output;
 * max_cov_seen: the largest cov; cov_array_bytes: bytes of the coverage array; n_batches and the inflate / index milliseconds are
 * those of both read passes.  Milliseconds are device time (mark = K22a, scan = K22b, verdict = K22c), ms_total_wall the wall clock. */
typedef struct {
    uint64_t n_records, n_counted, n_over, n_dropped, n_written;
    uint64_t max_cov_seen, cov_array_bytes;
    uint64_t inflated_bytes, stream_bytes, compressed_bytes;
    uint32_t n_batches, reserved;
    double ms_inflate, ms_index, ms_mark, ms_scan, ms_verdict, ms_deflate, ms_total_wall;
} sbx_subsample_stats;
int sbx_subsample(const char* in_path, const char* out_path, int max_cov, int remove, int level, int with_index,
                  const char* pg_command_line, int device, sbx_subsample_stats* stats, sbx_stream_stats* stream_stats, char* err,
                  size_t errlen);
/* `sambamba index -F` (buildFai, BioD bio/std/file/fai.d:78-101): the .fai of a FASTA file, its lines found and added up on the
 * device (K17).  The line terminator is "\r\n" when the first line ends in it, "\n" otherwise, for the whole file; the text is split
 * at it only (a last line without terminator is a line; with "\n" a '\r' is a byte of its line).  A line starting with '>' opens a
 * sequence whose name is the bytes between '>' and the first space (a tab does not end it; it may be empty) and whose offset is
 * that of the byte behind the line's terminator; any other line adds its length to the sequence, the first one that is not empty
 * sets the line length.  One row per sequence: name, length, offset, line length, line length + terminator, tab separated.
 * Deliberate divergences: an empty file gives an empty .fai (the reference dies); a first line that is no header is SBX_EFORMAT
 * naming line 1 (the reference indexes an empty array); with "\r\n" a '\n' without '\r' in front of it is SBX_EFORMAT with the number
 * of such line ends and the 1-based number of the first line that ends so (the reference counts it as sequence).  On failure no
 * .fai is left.  The text is uploaded in chunks cut at multiples of 16 bytes, not at line ends (64 MiB, not tuned;
 * SBX_FASTA_CHUNK_BYTES, at least 16, overrides it for tests); the output does not depend on the size.  Milliseconds are device time
 * (lines = K15a's newline count, scan and line starts; segments = K17's header flags, their scan and the reduction). */
typedef struct {
    uint64_t n_sequences, n_lines, n_bytes;
    uint32_t n_chunks, reserved;
    double ms_lines, ms_segments, ms_total_wall;
} sbx_fasta_stats;
int sbx_index_fasta(const char* fasta_path, const char* fai_path, int device, sbx_fasta_stats* stats, char* err, size_t errlen);

/* ---- engine seam ------------------------------------------------------------ */

/* new MultiBamReader(filenames) (multireader.d:244) + BamReader header parse (reader.d:101-125).
 * Several BAMs are processed as the reference's merged stream would be: the pileup of the merge is the union
 * of the files' reads, so every file goes through the device pipeline on its own and the per-position results
 * are added up; samples are the union of the @RG SM values in order of first appearance (depth.d:1170-1181 over
 * the merged header) and every file keeps its own RG-id -> sample table.  Reference dictionaries that differ
 * but are compatible are merged the way SamHeaderMerger does it (samheadermerger.d:127-177: a topological order
 * of the union of the @SQ lists; every context then holds the MERGED dictionary, ref_id arguments and results of
 * this API are ids of the merged dictionary, and the records' own ids are translated when they are read, as
 * adjustTagsInRange does, multireader.d:174-190).  Dictionaries that cannot be merged -- one name with two
 * lengths, contradicting orders -- fail with SBX_EUNSUPPORTED and the reference's message.  With -m, mates
 * are paired within a file only.
 * device = HIP device ordinal (or -1: use LOCAL_RANK / 0). */
sbx_ctx* sbx_open(const char* const* bam_paths, int n_bams, int device, char* err, size_t errlen);
void sbx_close(sbx_ctx*);
const char* sbx_last_error(sbx_ctx*);

int sbx_header(sbx_ctx*, sbx_header_info* out);
/* reference_sequences[i].name / .length (depth.d:455,576,1041,1223) */
const char* sbx_ref_name(sbx_ctx*, int ref_id);
int64_t sbx_ref_length(sbx_ctx*, int ref_id);
int sbx_ref_id(sbx_ctx*, const char* name);           /* bam.hasReference / bam[name].id; -1 if absent */
/* printer.sample_names (depth.d:1170-1181) */
const char* sbx_sample_name(sbx_ctx*, int sample_id);
/* raw SAM header text (for the D shim's SamHeader) */
const char* sbx_header_text(sbx_ctx*, size_t* len);

/* createFilterFromQuery (filtering.d:40-51).  query == NULL compiles the default
 * "mapping_quality > 0 and not duplicate and not failed_quality_control" (depth.d:1159).
 * The whole query language compiles; regular expressions in the common core of D's std.regex and ECMAScript
 * (no back-references, look-around or word boundaries; option i only; at most 2 per filter and 64 NFA states each),
 * anything else returns SBX_EUNSUPPORTED. */
int sbx_compile_filter(const char* query, sbx_filter* out, char* err, size_t errlen);
int sbx_set_filter(sbx_ctx*, const sbx_filter* f);
/* Host-side evaluation of one `=~` condition (the same NFA simulation the device runs): 1 = the pattern matches
 * somewhere in text[0, n), 0 = it does not, < 0 = the pattern is outside the supported subset (message in err). */
int sbx_regex_search(const char* pattern, const char* options, const char* text, size_t n, char* err, size_t errlen);

/* -q, -m, --combined (depth.d:1127-1132); window/overlap and -T (depth.d:712-715,1015-1018). */
int sbx_set_params(sbx_ctx*, int mode, uint8_t min_base_quality, int fix_mate_overlaps, int combined,
                   uint32_t window_size, uint32_t overlap, const uint32_t* cov_thresholds, int n_thresholds);

/* -L: the merged, sorted region list used to fetch reads (getReadsOverlapping, depth.d:1211 ->
 * randomaccessmanager.d:316-338).  n == 0 means "all reads" (bam.reads, depth.d:1214). */
int sbx_set_regions(sbx_ctx*, const sbx_region* regions, size_t n);

/* The -L argument of depth_main turned into regions the way the reference does it (depth.d:1184-1208): a BED file
 * (readIntervals / parseBed, sambamba/utils/common/bed.d:59-152: two-column lines mean [beg, beg+1), empty intervals
 * become one base long, lines naming contigs the BAM does not have are dropped) or, when the argument cannot be read
 * as one, a region string "ref[:beg[-end]]" (BioD/bio/core/region.d:97-246).  Afterwards sbx_parsed_regions copies out
 * the merged, sorted list (merged != 0: what sbx_set_regions wants) or the raw list in input order (what region mode
 * reports on), and sbx_parsed_region_line returns the input line that precedes the rows of raw region i
 * (depth.d:902-906; for a region string the synthetic "ref\tstart\tend", depth.d:1203-1206). */
int sbx_parse_regions(sbx_ctx*, const char* bed_path_or_region, size_t* n_merged, size_t* n_raw);
int sbx_parsed_regions(sbx_ctx*, int merged, sbx_region* out, size_t cap);
const char* sbx_parsed_region_line(sbx_ctx*, size_t raw_index);

/* Run BGZF inflate -> record index -> decode+accumulate on the device for everything the
 * current filter/params/regions select.  Results stay resident in HBM until the next
 * sbx_run()/sbx_close(); the sbx_depth_* getters below copy them out.  */
int sbx_run(sbx_ctx*);

/* Streaming over contigs.  One pass needs ~4.5 bytes of HBM per inflated byte (stream, token streams,
 * descriptors, counter tiles), so a whole-genome BAM is processed as consecutive batches of contigs --
 * the device-side counterpart of the reference's streaming BamReadRange (readrange.d:118-173).
 * sbx_plan_batches splits contigs [0, n_ref) into the fewest consecutive batches whose estimated footprint
 * stays below budget_bytes (0 = 70 % of the free device memory); an over-sized single contig gets a batch of
 * its own.  sbx_run_batch is sbx_run() restricted to the reads of contigs [first_ref, first_ref + n_refs)
 * (and to the regions of sbx_set_regions that lie on them, if any): afterwards the getters below answer for
 * those contigs only.  Results of the previous run / batch are replaced. */
typedef struct {
    uint32_t first_ref, n_refs;
    uint64_t est_bytes;
} sbx_batch;
int sbx_plan_batches(sbx_ctx*, uint64_t budget_bytes, sbx_batch* out, size_t cap, size_t* n_out);
int sbx_run_batch(sbx_ctx*, uint32_t first_ref, uint32_t n_refs);
/* sbx_run() restricted to the reads overlapping [beg, end) of ref_id (intersected with the regions of
 * sbx_set_regions, if any) -- the unit of sub-contig streaming and of position sharding across GPUs
 * (the analogue of one element of pileupChunks, BioD/bio/std/hts/bam/pileup.d:1011-1015; the reads come
 * through the BAI exactly as bam[ref][beg .. end] fetches them, randomaccessmanager.d:247-338).  Afterwards
 * the getters answer for positions in [beg, end) only: counters there are complete (every read overlapping
 * the interval was seen), outside they are partial. */
int sbx_run_interval(sbx_ctx*, uint32_t ref_id, uint32_t beg, uint32_t end);
/* Upload stage of the next sbx_run_interval(ref_id, beg, end) on its own: the BGZF blocks of the interval's work list are read from
 * the file and copied to the device (pinned staging, the context's copy stream); the results of the previous run stay valid and
 * may be read meanwhile -- by sbx_stream_base_rows / sbx_depth_* on ANOTHER host thread (the one exception to "one context, one
 * thread at a time").  A following sbx_run_interval with the same arguments finds the blocks resident and starts with the
 * kernels.  Lets a caller overlap file -> device, the kernels and device -> text of consecutive slices (cli.cpp does). */
int sbx_prefetch_interval(sbx_ctx*, uint32_t ref_id, uint32_t beg, uint32_t end);
/* The same fetch, but the run keeps only the reads whose LEFTMOST position lies in [beg, end) and counts every position
 * they cover, also beyond `end`: reads are partitioned between the intervals instead of clipped to them (what the elements of
 * pileupChunks are, pileup.d:1011-1015: chunks of READS).  Per-position counters of such runs are partial sums; adding them up
 * over a set of intervals that tile the contig (an all-reduce across GPUs, see sambamba_amd.dist_depth --reduce allreduce) gives
 * the counters of the whole.  Only without --fix-mate-overlaps (a pair must be resolved by one owner: SBX_EUNSUPPORTED). */
int sbx_run_interval_owned(sbx_ctx*, uint32_t ref_id, uint32_t beg, uint32_t end);

/* depth base: counters[(pos-beg)*n_samples*7 + s*7 + k] for pos in [beg,end) of ref_id
 * (k = A,C,G,T,other,DEL,REFSKIP; n_samples = 1 when --combined).  Positions no admitted read
 * spans are all-zero.  covered (optional, may be NULL): 1 byte per position, non-zero iff >= 1
 * admitted read spans the position (a pileup column exists there, pileup.d:345-397) -- needed
 * to tell "column with COV 0" from "no column" when min_base_quality > 0.
 * counters may be NULL when only `covered` is wanted.  The seven counters per position exist after a `base` run (and after
 * any run with --fix-mate-overlaps or several files); a region / window run keeps what its statistics are sums of -- the bases
 * counted and the depth of a position -- and answers a request for counters with SBX_EINVAL (`covered` is always available). */
int sbx_depth_base_tile(sbx_ctx*, uint32_t ref_id, uint32_t beg, uint32_t end, uint32_t* counters,
                        uint8_t* covered);

/* The same counters copied into DEVICE memory of the context's GPU (d_counters: (end - beg) * n_samples * 7 uint32, e.g. the
 * storage of a torch tensor handed to an RCCL all-reduce): device-to-device, nothing crosses PCIe. */
int sbx_depth_base_tile_device(sbx_ctx*, uint32_t ref_id, uint32_t beg, uint32_t end, void* d_counters);

/* depth region: stats[r*n_samples + s] and cov_counts[(r*n_samples + s)*n_thresholds + t] for the
 * raw (unmerged, input-order) region list given here (PerBedRegionPrinter, depth.d:879-931).
 * seen[r] != 0 iff at least one column hit region r (is_first_occurrence cleared). */
int sbx_depth_region_stats(sbx_ctx*, const sbx_region* raw_regions, size_t n_regions,
                           sbx_region_stats* stats, uint32_t* cov_counts, uint8_t* seen);

/* The same with a per-region lower bound on the read start (min_start[r] != 0: only reads with position >= min_start[r]
 * are counted for region r, n_bases being the sum over those reads).  This is what the reference's first ring of
 * OVERLAPPING windows computes (is_first_occurrence starts out false, depth.d:1031-1032): the host composes
 * `window --overlap` from this call and plain region statistics (cli.cpp WindowPrinter). */
int sbx_depth_region_stats_from(sbx_ctx*, const sbx_region* raw_regions, size_t n_regions, const uint32_t* min_start,
                                sbx_region_stats* stats, uint32_t* cov_counts, uint8_t* seen);

/* depth window: the same for windows [k*step, k*step + window) of ref_id, k in
 * [first_win, first_win + n_win) (PerWindowPrinter, depth.d:933-1077). */
int sbx_depth_window_stats(sbx_ctx*, uint32_t ref_id, uint64_t first_win, uint64_t n_win,
                           sbx_region_stats* stats, uint32_t* cov_counts);

/* Device-side row formatting of `depth base` (writeColumn's text, depth.d:534-555) for
 * [beg,end) of ref_id into a caller buffer; returns bytes written through *out_len, or
 * SBX_ENOMEM if cap is too small (then *out_len = required size). */
int sbx_format_base_rows(sbx_ctx*, uint32_t ref_id, uint32_t beg, uint32_t end, double min_cov, double max_cov,
                         int annotate, char* out, size_t cap, size_t* out_len);

/* sbx_format_base_rows with the text left in DEVICE memory: d_out is a device pointer on the context's device with room for cap
 * bytes (null with cap 0: measure only; *out_len receives the size either way, SBX_ENOMEM when cap is too small).  For a consumer
 * that keeps working on the device -- and for bench.py's `device_text` figure (the pass including its text, nothing over PCIe). */
int sbx_format_base_rows_device(sbx_ctx*, uint32_t ref_id, uint32_t beg, uint32_t end, double min_cov, double max_cov,
                                int annotate, void* d_out, size_t cap, size_t* out_len);
/* The same rows handed to a writer piece by piece, in output order.  The device formats the next piece while the
 * previous one travels to pinned host memory and the writer consumes the one before; `write` returns 0 on success
 * (anything else aborts with SBX_EIO).  `data` is only valid during the call.  Replaces the per-column
 * output.write(...) calls of writeColumn / writeEmptyColumns (depth.d:452-487,534-555) for a whole interval. */
typedef int (*sbx_write_fn)(void* user, const char* data, size_t n);
int sbx_stream_base_rows(sbx_ctx*, uint32_t ref_id, uint32_t beg, uint32_t end, double min_cov, double max_cov,
                         int annotate, sbx_write_fn write, void* user);

/* Timing / accounting of the last sbx_run() (for bench.py): per-kernel milliseconds measured
 * with HIP events on the engine's stream, record counts, byte counts. */
typedef struct {
    double ms_inflate, ms_index, ms_accumulate, ms_reduce, ms_total, ms_h2d;
    uint64_t n_records, n_admitted, n_bgzf_blocks;
    uint64_t compressed_bytes, uncompressed_bytes, counter_bytes, covered_positions;
    uint64_t launches_inflate, launches_index, launches_accumulate;
    double ms_huffman, ms_lz77;   /* the two kernels of ms_inflate */
    uint64_t n_malformed;         /* records dropped as malformed (always 0 after a successful run: they raise SBX_EFORMAT) */
    uint64_t n_runs;              /* record-chain runs of the device work list (1 for a whole file, one per merged BAI chunk group with -L) */
    uint64_t uploaded_bytes;      /* compressed bytes resident in HBM for this run (the BGZF blocks of the work list only) */
    uint64_t accumulate_read_bytes;   /* bytes the accumulate kernel has to read: 32-byte descriptors of the records + CIGAR and packed
                                         sequence of the admitted ones (+ their base qualities when min_base_quality > 0) */
    uint64_t token_bytes;             /* bytes of the literal + match-entry streams the Huffman kernel wrote and the LZ77 kernel read */
    uint64_t max_alignment_span;      /* longest alignment (reference positions) among the admitted records of the run */
    uint64_t reserved2, reserved3;
} sbx_run_stats;
int sbx_last_run_stats(sbx_ctx*, sbx_run_stats* out);

/* Geometry of the result tiles of the last sbx_run(): positions per tile and the effective
 * number of samples (1 under --combined). */
int sbx_tile_info(sbx_ctx*, uint32_t* tile_pos, uint32_t* n_samples);
/* Next maximal run of tiles of ref_id holding >= 1 admitted read, at or after position `from`:
 * [*beg,*end) in contig coordinates (tile-aligned end), or *beg == *end == UINT64_MAX when there is
 * none.  Lets a caller walk a contig without copying the all-zero stretches. */
int sbx_next_active_range(sbx_ctx*, uint32_t ref_id, uint64_t from, uint64_t* beg, uint64_t* end);

/* ---- several devices -----------------------------------------
 * The path shards by POSITION: the outputs of disjoint position ranges are disjoint, so one process drives N contexts -- one
 * sbx_open(..., device = k, ...) per device, each from its own thread -- and every context runs the slices it was given
 * (sbx_run_interval) and hands over its share of the result; there is no data-path collective (the reference's analogue of the
 * cut is pileupChunks, BioD/bio/std/hts/bam/pileup.d:1011-1015).  `sbx-depth --gpus N` and d/sbx_depth.d (sbxDepthRunSharded)
 * are built on these two calls. */
int sbx_device_count(void);          /* HIP devices visible to the process; 0 when there is none (never negative) */
typedef struct {
    uint32_t shard;    /* 0 .. n_shards - 1, ascending in the array */
    uint32_t ref_id;
    uint32_t beg;      /* [beg, end) of the contig; cuts inside a contig are multiples of `align` */
    uint32_t end;
} sbx_shard;
/* Equal shares of the concatenated reference for n_shards devices: whole contigs and, where a contig is cut, position
 * intervals inside it -- so ONE long contig shards as well as a genome does.  Every position of every contig belongs to
 * exactly one shard; a shard's intervals are in genome order; `align` (the tile size 1024, or the window size) keeps tiles /
 * windows whole.  Host arithmetic only (no device, no context).  *n_out receives the number of intervals (also with
 * SBX_ENOMEM, when cap is too small: n_ref + n_shards is always enough). */
int sbx_plan_shards(const int64_t* ref_lengths, int32_t n_ref, int32_t n_shards, uint32_t align, sbx_shard* out, size_t cap,
                    size_t* n_out);

/* Keep the compressed file resident in HBM across sbx_run() calls (bench: "inputs already
 * resident in HBM when the timed region starts"). */
int sbx_preload(sbx_ctx*);

#ifdef __cplusplus
}
#endif
#endif /* SBX_DEPTH_H */
