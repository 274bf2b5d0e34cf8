"""`sambamba sort` (coordinate order) on the device -- sbx_sort_bam: K9a keys, K9b radix sort, K9c gather (sort.hip) between the read
pass and the BGZF encoder -- through the Python API and the `sbx-sort` CLI, against the pure-Python restatement of sort.d
(tests/sort_ref.py).  Every comparison is byte for byte on the INFLATED output; the file itself must end with the EOF block and hold
no block of more than 0xFF00 payload bytes."""
import ctypes as C
import os
import random
import struct
import subprocess

import pytest

from tests import bamgen
from tests import sort_ref as ref
from tests.flagstat_ref import inflate
from tests.util import GOLDEN, gen_bam, run_cli, scan_bgzf

pytestmark = pytest.mark.gpu

REFS = [("c1", 100000), ("c2", 50000)]
UNSORTED = "@HD\tVN:1.6\tSO:unsorted\n@SQ\tSN:c1\tLN:100000\n@SQ\tSN:c2\tLN:50000\n@RG\tID:g1\tSM:s1\n@CO\tmade by the test-suite\n"
FIXTURES = ("issue225", "issue_193", "issue_204", "mate_overlaps_1_3M_4M", "match_mates")


def cli(args, env=None):
    from sambamba_amd import sort_cli_path
    return subprocess.run([sort_cli_path()] + list(args), stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                          env=dict(os.environ, **env) if env else None)


def check_file(path, want):
    """The BGZF file at `path` inflates to `want`, ends with the EOF block and has no payload above 0xFF00 bytes."""
    raw = open(path, "rb").read()
    assert raw[-28:] == bamgen.EOF_BLOCK
    _, _, _, isize, _, _ = scan_bgzf(path)
    assert all(int(x) <= 0xFF00 for x in isize)
    assert int(isize[-1]) == 0 and all(int(x) > 0 for x in isize[:-1])
    got = inflate(path)
    assert len(got) == len(want)
    assert got == want


def check(path, tmp_path, want=None, flt=None, keep=None, level=-1, tag="o"):
    """API and CLI against the restatement; returns the API's stats."""
    import sambamba_amd
    want = want if want is not None else ref.expected(path, keep)
    out_api = str(tmp_path / (tag + ".api.bam"))
    st = sambamba_amd.sort_bam(path, out_api, filter=flt, level=level)
    check_file(out_api, want)
    assert not os.path.exists(out_api + ".bai")
    out_cli = str(tmp_path / (tag + ".cli.bam"))
    args = ["-o", out_cli, path] + (["-F", flt] if flt else []) + (["-l", str(level)] if level != -1 else [])
    r = cli(args)
    assert r.returncode == 0, r.stderr
    check_file(out_cli, want)
    assert os.path.exists(out_cli + ".bai")          # like the reference's BamWriter for a name that ends in .bam
    n_want = len(ref.split_stream(want)[3])
    assert st["n_records_out"] == n_want and st["sorted_stream_bytes"] == len(want)
    assert st["compressed_bytes"] == os.path.getsize(out_api)
    return st


def refs_of(stream):
    _, refs, n_ref, _ = ref.split_stream(stream)
    out, p = [], 4
    for _ in range(n_ref):
        l_name = struct.unpack_from("<i", refs, p)[0]
        out.append((refs[p + 4:p + 4 + l_name - 1].decode(), struct.unpack_from("<i", refs, p + 4 + l_name)[0]))
        p += 8 + l_name
    return out


def shuffled_copy(path, out, seed):
    stream = inflate(path)
    text, _, _, recs = ref.split_stream(stream)
    recs = list(recs)
    random.Random(seed).shuffle(recs)
    bamgen.write_bam(out, refs_of(stream), recs, text=text.decode(), write_index=False)
    return out


@pytest.mark.parametrize("name", FIXTURES)
def test_reference_fixtures(name, tmp_path):
    path = os.path.join(GOLDEN, name + ".bam")
    check(path, tmp_path)
    shuf = shuffled_copy(path, str(tmp_path / "shuffled.bam"), seed=len(name))
    # the shuffle moves ties too: the expected stream is that of the shuffled file
    check(shuf, tmp_path, tag="s")


def test_match_mates_as_it_is(tmp_path):
    path = os.path.join(GOLDEN, "match_mates.bam")
    st = check(path, tmp_path)
    assert st["n_records_in"] == st["n_records_out"] == 22


def _tie_records(n=6000, seed=5):
    rng = random.Random(seed)
    recs = []
    for i in range(n):
        kind = rng.random()
        flag = 0x10 if rng.random() < 0.5 else 0
        if kind < 0.08:
            recs.append(bamgen.make_record(-1, rng.choice((-1, 0, 7)), "", "ACGT", 30, name="u%05d" % i, mapq=0, flag=0x4 | flag))
        elif kind < 0.16:
            recs.append(bamgen.make_record(rng.choice((0, 1)), -1, "", "ACGTA", 30, name="p%05d" % i, mapq=0, flag=0x4 | flag))
        else:
            pos = rng.choice((0, 1, 100, 100, 100, 4999, 49999))
            seq = "ACGTACGTAC"[:rng.randrange(4, 11)]
            recs.append(bamgen.make_record(rng.choice((0, 1)), pos, "%dM" % len(seq), seq, 30, name="t%05d" % i, flag=flag,
                                           tags=bamgen.tag_z("RG", "g1") if i % 3 else b""))
    return recs


def test_ties_keep_file_order(tmp_path):
    path = str(tmp_path / "ties.bam")
    recs = _tie_records()
    bamgen.write_bam(path, REFS, recs, text=UNSORTED, write_index=False)
    want = ref.expected(path)
    out = ref.split_stream(want)[3]
    # the restatement's own stability: records with equal keys appear in file order (names carry the file index)
    by_key = {}
    for r in out:
        by_key.setdefault(ref.record_key(r, 2), []).append(r[36:42])
    assert len(by_key) < 40 and all(v == sorted(v, key=lambda nm: nm[1:]) for v in by_key.values())
    st = check(path, tmp_path, want=want)
    assert st["n_records_out"] == len(recs) and st["n_sort_passes"] >= 1


@pytest.fixture(scope="module")
def layouts(tmp_path_factory):
    d = tmp_path_factory.mktemp("sortlayouts")
    recs = _tie_records(n=12000, seed=11)
    files = {}
    info = bamgen.write_bam(str(d / "all.bam"), REFS, recs, text=UNSORTED, write_index=False)
    files["all"] = str(d / "all.bam")
    starts = [r[3] for r in info["records"]]
    cuts = [s + 3 for s in starts[::97]] + [s + 30 for s in starts[50::211]]
    bamgen.write_bam(str(d / "cuts.bam"), REFS, recs, text=UNSORTED, cuts=cuts, write_index=False)
    files["cuts"] = str(d / "cuts.bam")
    bamgen.write_bam(str(d / "tiny.bam"), REFS, recs, text=UNSORTED, block_size=300, write_index=False)
    files["tiny"] = str(d / "tiny.bam")
    bamgen.write_bam(str(d / "levels.bam"), REFS, recs, text=UNSORTED, block_size=1000, levels=[0, 1, 9, 0, 6], write_index=False)
    files["levels"] = str(d / "levels.bam")
    return files, info, ref.expected(files["all"])


@pytest.mark.parametrize("kind", ["cuts", "tiny", "levels"])
def test_records_straddling_blocks(layouts, kind, tmp_path):
    files, _, want = layouts
    check(files[kind], tmp_path, want=want)


@pytest.mark.parametrize("kind", ["all", "tiny"])
def test_batches_give_the_same_output(layouts, kind, tmp_path, monkeypatch):
    import sambamba_amd
    files, info, want = layouts
    path = files[kind]
    batch = str(min(info["stream_len"] // 12, 60000))          # (at most one whole 0xFF00 block per batch: 12 batches or more)
    out = str(tmp_path / "b.bam")
    r = cli(["-o", out, path], env={"SBX_INDEX_BATCH_BYTES": batch, "SBX_TIMING": "1"})
    assert r.returncode == 0, r.stderr
    line = [x for x in r.stderr.decode().splitlines() if x.startswith("[sbx] sort:")]
    assert len(line) == 1
    fields = dict(kv.split("=") for kv in line[0].split("(")[0].split()[2:])
    assert int(fields["n_batches"]) >= 10, line[0]
    check_file(out, want)
    monkeypatch.setenv("SBX_INDEX_BATCH_BYTES", batch)
    out2 = str(tmp_path / "b2.bam")
    st = sambamba_amd.sort_bam(path, out2)
    assert st["n_batches"] >= 10
    check_file(out2, want)


def test_generated_bam_round_trip(tmp_path):
    import sambamba_amd
    bam = gen_bam(str(tmp_path / "g.bam"), "chrA:200000,chrB:150000", coverage=12, seed=77)
    shuf = shuffled_copy(bam, str(tmp_path / "g.shuffled.bam"), seed=2024)
    want = ref.expected(shuf)
    out = str(tmp_path / "g.sorted.bam")
    st = sambamba_amd.sort_bam(shuf, out, index=True)
    check_file(out, want)
    assert os.path.exists(out + ".bai")
    assert st["n_records_in"] == st["n_records_out"] > 10000
    os.remove(out + ".bai")
    sambamba_amd.build_index(out)
    assert run_cli(["base", out]) == run_cli(["base", bam])
    # the CLI's default output name: the extension replaced by sorted.bam
    r = cli([shuf])
    assert r.returncode == 0, r.stderr
    check_file(str(tmp_path / "g.shuffled.sorted.bam"), want)


def test_sorted_input_and_header_only(tmp_path):
    bam = gen_bam(str(tmp_path / "s.bam"), "chrA:60000", coverage=8, seed=3)
    stream = inflate(bam)
    st = check(bam, tmp_path)
    out = inflate(str(tmp_path / "o.api.bam"))
    assert ref.split_stream(out)[3] == ref.split_stream(ref.expected_stream(stream))[3]
    assert sorted(ref.split_stream(out)[3]) == sorted(ref.split_stream(stream)[3])
    assert st["n_records_in"] == st["n_records_out"]
    empty = str(tmp_path / "empty.bam")
    bamgen.write_bam(empty, REFS, [], text=UNSORTED, write_index=False)
    st = check(empty, tmp_path, tag="e")
    assert st["n_records_out"] == 0 and st["n_sort_passes"] == 0
    want = ref.expected(empty)
    assert ref.split_stream(want)[3] == [] and want[8:].startswith(b"@HD\tVN:1.6\tSO:coordinate\n@SQ\tSN:c1\tLN:100000\n")


def _keep_q30_not_dup(rec):
    bin_mq_nl, flag_nc = struct.unpack_from("<II", rec, 12)
    return ((bin_mq_nl >> 8) & 0xFF) >= 30 and not (flag_nc >> 16) & 0x400


def test_filter(tmp_path):
    bam = gen_bam(str(tmp_path / "f.bam"), "chrA:120000,chrB:80000", coverage=10, seed=9)
    shuf = shuffled_copy(bam, str(tmp_path / "f.shuffled.bam"), seed=7)
    st = check(shuf, tmp_path, flt="mapping_quality >= 30 and not duplicate", keep=_keep_q30_not_dup)
    assert 0 < st["n_records_out"] < st["n_records_in"]
    # unmapped and unplaced records are asked too
    path = str(tmp_path / "ties.bam")
    bamgen.write_bam(path, REFS, _tie_records(n=3000, seed=21), text=UNSORTED, write_index=False)
    st = check(path, tmp_path, flt="unmapped or reverse_strand", tag="u",
               keep=lambda r: bool((struct.unpack_from("<I", r, 16)[0] >> 16) & 0x14))
    assert 0 < st["n_records_out"] < st["n_records_in"]
    st = check(path, tmp_path, flt="[RG] == 'g1'", tag="rg", keep=lambda r: b"RGZg1\0" in r)
    assert 0 < st["n_records_out"] < st["n_records_in"]


def test_levels_inflate_to_the_same_stream(layouts, tmp_path):
    files, _, want = layouts
    sizes = {}
    for level in (0, 1, 6, -1):
        check(files["all"], tmp_path, want=want, level=level, tag="l%d" % level)
        sizes[level] = os.path.getsize(str(tmp_path / ("l%d.api.bam" % level)))
    assert sizes[0] > sizes[1] >= sizes[6]


def _assert_fails(args_path, code, tmp_path):
    import sambamba_amd
    out = str(tmp_path / "fail.bam")
    with pytest.raises(sambamba_amd.SbxError) as ei:
        sambamba_amd.sort_bam(args_path, out)
    assert ei.value.code == code, ei.value
    assert not os.path.exists(out)
    r = cli(["-o", out, args_path])
    assert r.returncode == 1 and r.stdout == b"" and r.stderr.startswith(b"sbx-sort: ")
    assert not os.path.exists(out) and not os.path.exists(out + ".bai")


def test_refused_options(tmp_path):
    path = os.path.join(GOLDEN, "match_mates.bam")
    for opt in (["-n"], ["-N"], ["--sort-picard"], ["-M"], ["-n", "-M"], ["--sort-by-name"], ["--natural-sort"], ["--match-mates"]):
        out = str(tmp_path / "r.bam")
        r = cli(opt + ["-o", out, path])
        assert r.returncode == 1 and r.stdout == b"", opt
        assert r.stderr.startswith(b"sbx-sort: ") and opt[0].lstrip("-").encode() in r.stderr, (opt, r.stderr)
        assert not os.path.exists(out)


def test_missing_truncated_and_corrupt(layouts, tmp_path):
    files, info, _ = layouts
    _assert_fails(str(tmp_path / "no_such.bam"), -2, tmp_path)
    raw = open(files["all"], "rb").read()
    cut = str(tmp_path / "cut.bam")
    open(cut, "wb").write(raw[:len(raw) // 2])
    _assert_fails(cut, -3, tmp_path)
    _, co, _, _, oo, _ = scan_bgzf(files["all"])
    starts = {r[3] for r in info["records"]}
    k = next(k for k in range(len(co) // 2, len(co)) if int(oo[k]) not in starts)
    chopped = str(tmp_path / "chopped.bam")
    open(chopped, "wb").write(raw[:int(co[k]) - 18])
    _assert_fails(chopped, -3, tmp_path)
    bad = str(tmp_path / "bad.bam")
    _, co, _, _, _, _ = scan_bgzf(files["levels"])
    b = bytearray(open(files["levels"], "rb").read())
    b[int(co[len(co) // 2])] = 0xFF
    open(bad, "wb").write(b)
    _assert_fails(bad, -3, tmp_path)


def test_reference_id_out_of_range(tmp_path):
    path = str(tmp_path / "badref.bam")
    recs = [bamgen.make_record(0, 10, "4M", "ACGT", 30, name="a"), bamgen.make_record(2, 10, "4M", "ACGT", 30, name="b")]
    bamgen.write_bam(path, REFS, recs, text=UNSORTED, write_index=False)
    _assert_fails(path, -3, tmp_path)


def test_output_must_not_be_the_input(tmp_path):
    import sambamba_amd
    path = str(tmp_path / "in.bam")
    bamgen.write_bam(path, REFS, _tie_records(n=50), text=UNSORTED, write_index=False)
    before = open(path, "rb").read()
    with pytest.raises(sambamba_amd.SbxError):
        sambamba_amd.sort_bam(path, path)
    for args in (["-o", path, path], ["-o", str(tmp_path / "." / "in.bam"), path]):
        r = cli(args)
        assert r.returncode == 1 and r.stderr.startswith(b"sbx-sort: ")
    assert open(path, "rb").read() == before


def test_cli_arguments(tmp_path):
    r = cli([])
    assert r.returncode == 1 and r.stdout == b"" and b"Usage" in r.stderr
    path = os.path.join(GOLDEN, "match_mates.bam")
    want = ref.expected(path)
    for k, args in enumerate((["-t", "4", "-m", "1G"], ["--tmpdir=/tmp", "-u", "-p"], ["--nthreads=2", "--memory-limit=500M", "-l", "1"],
                              ["--compression-level=0", "--show-progress"])):
        out = str(tmp_path / ("a%d.bam" % k))
        r = cli(args[:2] + [path] + args[2:] + ["--out=" + out])
        assert r.returncode == 0, (args, r.stderr)
        check_file(out, want)
    assert cli(["-l", "12", "-o", str(tmp_path / "x.bam"), path]).returncode == 1
    assert cli(["--no-such-option", path]).returncode == 1
    r = cli(["-F", "mapping_quality >=", "-o", str(tmp_path / "x.bam"), path])
    assert r.returncode == 1 and r.stderr.startswith(b"sbx-sort: ") and not os.path.exists(str(tmp_path / "x.bam"))


def test_abi_sizeof_sort_stats():
    import sambamba_amd
    from sambamba_amd._lib import SortStats
    L = sambamba_amd.lib()
    assert L.sbx_abi_sizeof(b"sbx_sort_stats") == C.sizeof(SortStats) == 5 * 8 + 4 * 4 + 7 * 8
