"""Record validation on the device -- K19 (valid.hip) behind sbx_validate_bam, `sbx-validate`, view(valid=True) and `sbx-sam -v` --
against the Python restatement of alignment.d (tests/valid_ref.py) applied to the records of generated files: the hand-made cases
of tests/valid_cases.py interleaved with valid records, in small BGZF blocks so that records straddle them."""
import ctypes as C
import os
import struct
import subprocess

import pytest

from tests import bamgen
from tests import sam_ref
from tests import valid_cases as cases
from tests import valid_ref as vref
from tests import view_ref
from tests.flagstat_ref import inflate
from tests.markdup_ref import header_text
from tests.sort_ref import split_stream
from tests.test_gpu_sort import check_file

pytestmark = pytest.mark.gpu

REFS = [("c1", 1 << 29), ("c2", 100000)]
N_RECORDS = 3001                    # a multiple of neither 64 nor 256
# valid for alignment.d, whose tag loop does not look at one byte left over, and refused by the SAM sink (K13), which does: the files
# here are also written as SAM, so the case stays with the CPU tests
LEFT_OVER = "one byte left over"
SMALL_BATCH = "40000"               # inflated bytes per batch: the dirty file is some 250 KB


def filler(k):
    """valid record number k: mapq, flag and position vary so that -F, --num-filter and the regions select some"""
    body = cases.rec(name=b"fill%05d" % k, pos=1000 + 7 * k, cigar="%dM" % (20 + k % 50), ref=k % 2, flag=(16 if k % 3 == 0 else 0) | (1024 if k % 5 == 0 else 0),
                     tags=cases.num(b"NM", b"C", k % 7) + cases.z(b"RG", b"g%d" % (k % 3)))
    return body[:13] + bytes([10 + k % 60]) + body[14:]            # mapq


def build(path, special, first_special=0):
    """special records spread evenly among fillers, N_RECORDS in all, none in front of ordinal first_special"""
    recs, k = [], 0
    gap = max(1, (N_RECORDS - first_special) // max(1, len(special)))
    it = iter(special)
    nxt = next(it, None)
    while len(recs) < N_RECORDS:
        if nxt is not None and len(recs) >= first_special and (len(recs) - first_special) % gap == 0:
            recs.append(nxt)
            nxt = next(it, None)
        else:
            recs.append(filler(k))
            k += 1
    assert nxt is None
    bamgen.write_bam(path, REFS, recs, block_size=1531, write_index=False)
    return recs


def report_of(recs):
    masks = [vref.mask(r) for r in recs]
    bad = [i for i, m in enumerate(masks) if m]
    first = None
    if bad:
        first = {"ordinal": bad[0], "mask": masks[bad[0]], "classes": [c for k, c in enumerate(vref.CLASSES) if masks[bad[0]] >> k & 1],
                 "name": vref.name_of(recs[bad[0]])}
    return {"n_records": len(recs), "n_invalid": len(bad),
            "class_count": {c: sum(1 for m in masks if m >> k & 1) for k, c in enumerate(vref.CLASSES)}, "first_invalid": first}


@pytest.fixture(scope="module")
def dirty(tmp_path_factory):
    """every case that can stand in a record chain; the first invalid record lies behind the first small batch"""
    d = tmp_path_factory.mktemp("valid")
    path = str(d / "dirty.bam")
    special = [r for label, r, _ in cases.cases() if cases.stream_safe(r) and label != LEFT_OVER]
    recs = build(path, special, first_special=700)
    assert recs == split_stream(inflate(path))[3]
    want = report_of(recs)
    assert want["n_invalid"] > 80 and all(want["class_count"].values()) and want["first_invalid"]["ordinal"] >= 700
    return path, recs, want


@pytest.fixture(scope="module")
def sane(tmp_path_factory):
    """the invalid records view reads without -v: no malformed fixed part, no malformed tags"""
    d = tmp_path_factory.mktemp("valid_sane")
    path = str(d / "sane.bam")
    recs = build(path, [r for label, r, m in cases.cases() if cases.stream_safe(r) and not m & cases.MALFORMED and label != LEFT_OVER])
    return path, recs


@pytest.fixture(scope="module")
def clean(tmp_path_factory):
    d = tmp_path_factory.mktemp("valid_clean")
    path = str(d / "clean.bam")
    return path, build(path, [])


def env_with(batch):
    return dict(os.environ, SBX_INDEX_BATCH_BYTES=batch) if batch else dict(os.environ)


def in_env(batch, fn):
    old = os.environ.get("SBX_INDEX_BATCH_BYTES")
    try:
        if batch:
            os.environ["SBX_INDEX_BATCH_BYTES"] = batch
        return fn()
    finally:
        if old is None:
            os.environ.pop("SBX_INDEX_BATCH_BYTES", None)
        else:
            os.environ["SBX_INDEX_BATCH_BYTES"] = old


@pytest.mark.parametrize("batch", [None, SMALL_BATCH])
def test_validate_equals_the_restatement(dirty, batch):
    import sambamba_amd
    path, recs, want = dirty
    got = in_env(batch, lambda: sambamba_amd.validate(path))
    st = got.pop("stats")
    print(got["class_count"], got["first_invalid"], st)
    assert got == want
    assert st["inflated_bytes"] == len(inflate(path))
    if batch:
        first_batch_records = next(i for i in range(len(recs)) if sum(len(r) for r in recs[:i + 1]) > int(batch))
        assert st["n_batches"] >= 3 and want["first_invalid"]["ordinal"] > first_batch_records
    else:
        assert st["n_batches"] == 1


def test_validate_a_clean_file(clean):
    import sambamba_amd
    path, recs = clean
    got = sambamba_amd.validate(path)
    assert got["n_records"] == N_RECORDS and got["n_invalid"] == 0 and got["first_invalid"] is None and not any(got["class_count"].values())


SELECTIONS = {
    "alone": dict(),
    "filter": dict(filter="mapping_quality >= 30 and not duplicate"),
    "num_filter": dict(num_filter="/1024"),
    "regions": dict(regions=["c1:1-9000", "c1:5000-12000"]),
}


def expected_records(recs, which, valid_only):
    kept = [r for r in recs if not valid_only or vref.mask(r) == 0]
    kw = {}
    if which == "filter":
        kw["keep"] = lambda r: r[13] >= 30 and not struct.unpack_from("<H", r, 18)[0] & 0x400
    if which == "num_filter":
        kw["bits"] = view_ref.num_filter("/1024")
    if which == "regions":
        kw["regions"] = [view_ref.parse_region(g, REFS) for g in SELECTIONS[which]["regions"]]
    return view_ref.select(kept, **kw)


def expected_bam(path, records, command_line):
    text, refs, _, _ = split_stream(inflate(path))
    new_text = header_text(text.decode(), command_line).encode()
    return b"BAM\1" + struct.pack("<i", len(new_text)) + new_text + refs + b"".join(records)


@pytest.mark.parametrize("batch", [None, SMALL_BATCH])
@pytest.mark.parametrize("which", list(SELECTIONS))
def test_view_valid_only(dirty, tmp_path, which, batch):
    import sambamba_amd
    path, recs, _ = dirty
    want = expected_records(recs, which, True)
    assert 0 < len(want) < len(expected_records(recs, which, False))
    kw = SELECTIONS[which]

    def run():
        assert sambamba_amd.view(path, count=True, valid=True, **kw) == len(want)
        out = str(tmp_path / "v.bam")
        st = sambamba_amd.view(path, out, valid=True, command_line="view -v", **kw)
        check_file(out, expected_bam(path, want, "view -v"))
        assert st["n_entries_out"] == len(want) and st["n_records_in"] == len(recs)
        sam = str(tmp_path / "v.sam")
        sambamba_amd.view(path, sam, valid=True, format="sam", **kw)
        assert open(sam, "rb").read() == sam_ref.sam_text(want, [n for n, _ in REFS])
    in_env(batch, run)


@pytest.mark.parametrize("which", list(SELECTIONS))
def test_without_the_option_run_and_the_old_entry_points_agree(sane, tmp_path, which):
    import sambamba_amd
    from sambamba_amd._lib import ViewOpts, ViewStats, compile_filter
    path, recs = sane
    want = expected_records(recs, which, False)
    assert len(want) > len(expected_records(recs, which, True))
    kw = SELECTIONS[which]
    L = sambamba_amd.lib()
    f = compile_filter(kw["filter"]) if "filter" in kw else None
    fp = C.byref(f) if f is not None else None
    o = ViewOpts()
    if "num_filter" in kw:
        o.flags_set, o.flags_unset = sambamba_amd.view_num_filter(kw["num_filter"])
    regions = kw.get("regions", [])
    arr = (C.c_char_p * max(1, len(regions)))(*[g.encode() for g in regions])
    err = C.create_string_buffer(512)
    st = ViewStats()
    n = C.c_uint64(0)
    assert L.sbx_view_count(path.encode(), fp, C.byref(o), arr, len(regions), None, -1, C.byref(n), C.byref(st), err, 512) == 0, err.value
    assert n.value == len(want) == sambamba_amd.view(path, count=True, **kw)
    old_bam, new_bam = str(tmp_path / "old.bam"), str(tmp_path / "new.bam")
    assert L.sbx_view_bam(path.encode(), old_bam.encode(), fp, C.byref(o), arr, len(regions), None, b"view x", -1, 0, -1, C.byref(st), err, 512) == 0, err.value
    sambamba_amd.view(path, new_bam, command_line="view x", **kw)
    assert open(old_bam, "rb").read() == open(new_bam, "rb").read()
    check_file(new_bam, expected_bam(path, want, "view x"))
    old_sam, new_sam = str(tmp_path / "old.sam"), str(tmp_path / "new.sam")
    assert L.sbx_view_sam(path.encode(), old_sam.encode(), fp, C.byref(o), arr, len(regions), None, None, 0, -1, C.byref(st), err, 512) == 0, err.value
    sambamba_amd.view(path, new_sam, format="sam", **kw)
    assert open(old_sam, "rb").read() == open(new_sam, "rb").read() == sam_ref.sam_text(want, [n for n, _ in REFS])


def test_a_request_from_an_older_caller(sane):
    """struct_size that ends in front of valid_only: the field counts as 0; one that ends in front of `device` is refused"""
    import sambamba_amd
    from sambamba_amd._lib import ViewRequest, ViewStats
    path, recs = sane
    L = sambamba_amd.lib()
    q = ViewRequest()
    q.struct_size, q.sink, q.in_path, q.device, q.valid_only = ViewRequest.valid_only.offset, 0, path.encode(), -1, 1
    n, err = C.c_uint64(0), C.create_string_buffer(512)
    assert L.sbx_view_run(C.byref(q), C.byref(n), None, err, 512) == 0, err.value
    assert n.value == len(recs)
    q.struct_size = C.sizeof(ViewRequest)
    assert L.sbx_view_run(C.byref(q), C.byref(n), None, err, 512) == 0 and n.value == sum(1 for r in recs if vref.mask(r) == 0)
    q.struct_size = ViewRequest.device.offset
    assert L.sbx_view_run(C.byref(q), C.byref(n), None, err, 512) == -1 and b"struct_size" in err.value


def run_cli(exe, args, batch=None):
    return subprocess.run([exe] + args, stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env_with(batch))


def test_sbx_sam_valid(dirty, tmp_path):
    import sambamba_amd
    path, recs, _ = dirty
    want = [r for r in recs if vref.mask(r) == 0]
    r = run_cli(sambamba_amd.sam_cli_path(), ["-v", "-c", path])
    assert (r.returncode, r.stdout) == (0, b"%d\n" % len(want)), r.stderr
    out = str(tmp_path / "o.bam")
    args = ["--valid", "-f", "bam", "-o", out, path]
    r = run_cli(sambamba_amd.sam_cli_path(), args, SMALL_BATCH)
    assert r.returncode == 0 and r.stdout == b"", r.stderr
    check_file(out, expected_bam(path, want, "view " + " ".join(args)))
    r = run_cli(sambamba_amd.sam_cli_path(), ["-v", path, "c2"])
    assert r.returncode == 0, r.stderr
    assert r.stdout == sam_ref.sam_text(view_ref.select(want, regions=[view_ref.parse_region("c2", REFS)]), [n for n, _ in REFS])


def report_text(path, want):
    import sambamba_amd
    return sambamba_amd.format_validate_report(path, want["n_records"], want["n_invalid"], want["class_count"], want["first_invalid"])


def test_sbx_validate(dirty, clean):
    import sambamba_amd
    exe = sambamba_amd.validate_cli_path()
    path, recs, want = dirty
    lines = ["file\t" + path, "records\t%d" % len(recs), "invalid\t%d" % want["n_invalid"]]
    lines += ["%s\t%d" % (c, want["class_count"][c]) for c in vref.CLASSES]
    name = "".join(chr(c) if 33 <= c <= 126 and c != 92 else "\\x%02X" % c for c in want["first_invalid"]["name"])
    lines += ["first-invalid\t%d\t%s\t%s" % (want["first_invalid"]["ordinal"], name, ",".join(want["first_invalid"]["classes"]))]
    text = ("\n".join(lines) + "\n").encode()
    assert text == report_text(path, want)
    r = run_cli(exe, ["-t", "3", path], SMALL_BATCH)
    assert (r.returncode, r.stdout, r.stderr) == (1, text, b"")
    cpath, crecs = clean
    ctext = report_text(cpath, report_of(crecs))
    r = run_cli(exe, [cpath, "-p"])
    assert (r.returncode, r.stdout, r.stderr) == (0, ctext, b"")
    r = run_cli(exe, [cpath, path, cpath])
    assert (r.returncode, r.stdout, r.stderr) == (1, ctext + text + ctext, b"")
    r = run_cli(exe, [cpath, os.path.join(os.path.dirname(cpath), "missing.bam"), path])
    assert r.returncode == 1 and r.stdout == ctext and r.stderr.startswith(b"sbx-validate: ")


def test_a_record_with_malformed_tags_is_dropped_not_fatal(tmp_path):
    import sambamba_amd
    path = str(tmp_path / "one.bam")
    broken = cases.rec(name=b"broken", tags=cases.num(b"XI", b"i") + b"XZZno end")
    assert vref.mask(broken) == vref.MALFORMED
    recs = build(path, [broken], first_special=1500)
    good = [r for r in recs if r is not broken]
    out = str(tmp_path / "o.sam")
    with pytest.raises(sambamba_amd.SbxError) as ei:
        sambamba_amd.view(path, out, format="sam")
    assert ei.value.code == -3 and not os.path.exists(out)          # SBX_EFORMAT, as before
    sambamba_amd.view(path, out, format="sam", valid=True)
    assert open(out, "rb").read() == sam_ref.sam_text(good, [n for n, _ in REFS])
    # and one with a malformed fixed part, which without -v fails every sink
    cut = cases.rec(cigar="5M")[4:-1]
    recs = build(path, [struct.pack("<i", len(cut)) + cut], first_special=10)
    with pytest.raises(sambamba_amd.SbxError) as ei:
        sambamba_amd.view(path, count=True)
    assert ei.value.code == -3
    assert sambamba_amd.view(path, count=True, valid=True) == N_RECORDS - 1
    bam = str(tmp_path / "o.bam")
    sambamba_amd.view(path, bam, valid=True)
    check_file(bam, expected_bam(path, [r for r in recs if vref.mask(r) == 0], None))


def test_abi_sizes_and_bindings_agree():
    import sambamba_amd
    from sambamba_amd._lib import ValidateReport, ValidateStats, ViewRequest
    from tests.test_d_binding import _d_source, _enums, _extern_block, _layout, _structs
    L = sambamba_amd.lib()
    text = _d_source()
    structs = _structs(_extern_block(text), _enums(text))
    for name, ty in (("sbx_view_request", ViewRequest), ("sbx_validate_report", ValidateReport), ("sbx_validate_stats", ValidateStats)):
        want = L.sbx_abi_sizeof(name.encode())
        assert want == C.sizeof(ty) > 0
        fields = [("size_t" if t in ("sbx_cstr", "sbx_cstr_list", "sbx_filter_ptr", "sbx_view_opts_ptr") else t, dims, f) for t, dims, f in structs[name]]
        assert _layout(name, dict(structs, **{name: fields}), {})[0] == want
        assert [f for _, _, f in structs[name]] == [f for f, _ in ty._fields_]
