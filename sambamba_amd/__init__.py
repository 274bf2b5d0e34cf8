"""sambamba_amd -- Python harness around libsbx_depth.so, the MI355X (gfx950) engine behind
`sambamba depth base|region|window`, `sambamba flagstat`, `sambamba sort`, `sambamba markdup`, `sambamba merge`, `sambamba view` (SAM input included), `sambamba slice`, `sambamba index` (BAM and FASTA) `sambamba fixbins`, `sambamba subsample` and `sambamba view -v` / `sbx-validate`.

The product is the C-ABI library (include/sbx_depth.h) plus the `sbx-depth` CLI, both built
from sambamba_amd/csrc/ by sambamba_amd.build.  This package only binds the C ABI with ctypes
for tests and bench.py; there is no Python or CPU implementation of the hot path, and loading
fails loudly when the library has not been built.
"""
from ._lib import (SbxError, Depth, lib, lib_path, inflate_blocks, compile_filter, regex_search, cli_path,  # noqa: F401
                   bgzf_compress, write_bam, build_index, flagstat, format_flagstat, flagstat_cli_path,
                   sort_bam, sort_header_text, sort_cli_path, nsort_cli_path, markdup, markdup_header_text, markdup_cli_path,
                   merge, merge_header_text, merge_cli_path,
                   view, view_num_filter, view_reference_info, view_cli_path, sam_cli_path, iview_cli_path,
                   slice_bam, slice_cli_path,
                   import_sam, import_cli_path,
                   fixbins, index_fasta, index_cli_path, fixbins_cli_path,
                   subsample, subsample_cli_path,
                   validate, format_validate_report, validate_cli_path, VALIDATE_CLASSES,
                   SBX_MODE_BASE, SBX_MODE_REGION, SBX_MODE_WINDOW)
