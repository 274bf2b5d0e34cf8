"""Build libsbx_depth.so (HIP kernels + C ABI) and the sbx-depth / sbx-flagstat / sbx-sort / sbx-markdup / sbx-merge / sbx-view / sbx-sam / sbx-iview / sbx-nsort / sbx-import / sbx-index / sbx-fixbins / sbx-slice / sbx-validate / sbx-subsample CLIs for gfx950 with hipcc.

Usage: python -m sambamba_amd.build   (or sambamba_amd.build.build())
Outputs are written in-tree (sambamba_amd/csrc/) so they travel with gpurun snapshots.
"""
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
LIB = os.path.join(CSRC, "libsbx_depth.so")
CLI = os.path.join(CSRC, "sbx-depth")
FLAGSTAT_CLI = os.path.join(CSRC, "sbx-flagstat")
SORT_CLI = os.path.join(CSRC, "sbx-sort")
MARKDUP_CLI = os.path.join(CSRC, "sbx-markdup")
MERGE_CLI = os.path.join(CSRC, "sbx-merge")
VIEW_CLI = os.path.join(CSRC, "sbx-view")
SAM_CLI = os.path.join(CSRC, "sbx-sam")        # view_cli.cpp once more, with SAM output (-DSBX_VIEW_SAM=1)
IVIEW_CLI = os.path.join(CSRC, "sbx-iview")    # view_cli.cpp a third time, reading through the .bai (-DSBX_VIEW_INDEXED=1)
NSORT_CLI = os.path.join(CSRC, "sbx-nsort")    # sort_cli.cpp once more, with the name orders (-DSBX_SORT_BY_NAME=1)
IMPORT_CLI = os.path.join(CSRC, "sbx-import")
INDEX_CLI = os.path.join(CSRC, "sbx-index")
FIXBINS_CLI = os.path.join(CSRC, "sbx-fixbins")
SLICE_CLI = os.path.join(CSRC, "sbx-slice")
VALIDATE_CLI = os.path.join(CSRC, "sbx-validate")
SUBSAMPLE_CLI = os.path.join(CSRC, "sbx-subsample")
SOURCES = ["inflate.hip", "index.hip", "scan.hip", "lines.hip", "depth.hip", "reduce.hip", "mates.hip", "format.hip", "deflate.hip", "flagstat.hip", "sort.hip", "markdup.hip", "merge.hip", "view.hip", "sam.hip", "namesort.hip", "samparse.hip", "bins.hip", "fasta.hip", "slice.hip", "valid.hip", "stream.hip", "subsample.hip", "engine.cpp",
           "engine_worklist.cpp", "engine_run.cpp", "engine_stats.cpp", "engine_text.cpp", "engine_writer.cpp", "engine_sort.cpp", "engine_markdup.cpp", "engine_merge.cpp", "engine_view.cpp", "engine_import.cpp", "engine_fixbins.cpp", "engine_fasta.cpp", "engine_slice.cpp", "engine_valid.cpp", "engine_subsample.cpp"]
HEADERS = sorted(f for f in os.listdir(CSRC) if f.endswith(".hpp")) + [os.path.join("..", "..", "include", "sbx_depth.h")]


def _hipcc():
    for cand in (os.environ.get("HIPCC"), "/opt/rocm/bin/hipcc", "hipcc"):
        if cand and (os.path.isabs(cand) and os.path.exists(cand) or not os.path.isabs(cand)):
            return cand
    return "hipcc"


def _stale(target, deps):
    if not os.path.exists(target):
        return True
    t = os.path.getmtime(target)
    return any(os.path.getmtime(d) > t for d in deps if os.path.exists(d))


def build(force=False, verbose=False):
    srcs = [os.path.join(CSRC, s) for s in SOURCES]
    deps = srcs + [os.path.join(CSRC, h) for h in HEADERS]
    flags = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-Wall", "-Wno-unused-function",
             "-Wno-unused-result"]
    if force or _stale(LIB, deps):
        objs, jobs = [], []
        for s in srcs:
            o = s.rsplit(".", 1)[0] + ".o"
            if force or _stale(o, deps):
                cmd = [_hipcc()] + flags + ["-x", "hip", "-c", s, "-o", o]
                if verbose:
                    print(" ".join(cmd))
                jobs.append(cmd)
            objs.append(o)
        # the translation units are independent: compile them side by side
        from concurrent.futures import ThreadPoolExecutor
        with ThreadPoolExecutor(max_workers=max(1, min(len(jobs), os.cpu_count() or 1))) as ex:
            for rc in ex.map(subprocess.call, jobs):
                if rc != 0:
                    raise subprocess.CalledProcessError(rc, "hipcc")
        cmd = [_hipcc(), "--offload-arch=gfx950", "-shared", "-fPIC", "-o", LIB] + objs
        if verbose:
            print(" ".join(cmd))
        subprocess.check_call(cmd)
    for cli, src, defs in ((CLI, "cli.cpp", []), (FLAGSTAT_CLI, "flagstat_cli.cpp", []), (SORT_CLI, "sort_cli.cpp", []),
                           (MARKDUP_CLI, "markdup_cli.cpp", []), (MERGE_CLI, "merge_cli.cpp", []), (VIEW_CLI, "view_cli.cpp", []),
                           (SAM_CLI, "view_cli.cpp", ["-DSBX_VIEW_SAM=1"]), (IVIEW_CLI, "view_cli.cpp", ["-DSBX_VIEW_INDEXED=1"]), (NSORT_CLI, "sort_cli.cpp", ["-DSBX_SORT_BY_NAME=1"]),
                           (IMPORT_CLI, "import_cli.cpp", []), (INDEX_CLI, "index_cli.cpp", []), (FIXBINS_CLI, "fixbins_cli.cpp", []), (SLICE_CLI, "slice_cli.cpp", []),
                           (VALIDATE_CLI, "validate_cli.cpp", []), (SUBSAMPLE_CLI, "subsample_cli.cpp", [])):
        cli_src = os.path.join(CSRC, src)
        if os.path.exists(cli_src) and (force or _stale(cli, [cli_src, LIB] + deps)):
            cmd = [_hipcc(), "-O2", "-std=c++17"] + defs + ["-o", cli, cli_src, "-L" + CSRC, "-lsbx_depth",
                   "-Wl,-rpath,$ORIGIN"]
            if verbose:
                print(" ".join(cmd))
            subprocess.check_call(cmd)
    return LIB


if __name__ == "__main__":
    build(force="--force" in sys.argv, verbose=True)
    print(LIB)
