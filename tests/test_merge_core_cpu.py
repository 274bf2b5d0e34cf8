"""The header merge of `sambamba merge` (sambamba_amd/csrc/merge_core.hpp, a restatement of SamHeaderMerger, BioD
bio/std/hts/utils/samheadermerger.d:51-301) against hand-written answers: through tests/native/merge_host.cpp, compiled for the host
with g++, through sbx_merge_header_text of the library, and through the Python restatement the GPU tests compare with
(tests/merge_ref.py) -- no GPU needed."""
import os
import subprocess

import pytest

from tests import merge_ref
from tests.util import ROOT

SRC = os.path.join(ROOT, "tests", "native", "merge_host.cpp")
HD = "@HD\tVN:1.6\tSO:coordinate\n"


def header(sq=(), rg=(), pg=(), co=(), hd=HD):
    """sq: (name, length); rg: (id, fields text); pg: (id, PN, PP or None)."""
    t = hd + "".join("@SQ\tSN:%s\tLN:%d\n" % s for s in sq)
    t += "".join("@RG\tID:%s%s\n" % (i, "\t" + f if f else "") for i, f in rg)
    t += "".join("@PG\tID:%s\tPN:%s%s\n" % (i, pn, "\tPP:" + pp if pp else "") for i, pn, pp in pg)
    return t + "".join("@CO\t%s\n" % c for c in co)


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    d = tmp_path_factory.mktemp("mergec")
    exe = str(d / "merge_host")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-I/opt/rocm/include", "-D__HIP_PLATFORM_AMD__", "-o", exe, SRC])

    def run(texts):
        paths = []
        for k, t in enumerate(texts):
            paths.append(str(d / ("h%d.txt" % k)))
            with open(paths[-1], "w") as fh:
                fh.write(t)
        out = subprocess.run([exe] + paths, stdout=subprocess.PIPE, check=True).stdout.decode()
        head, _, text = out.partition("text\n")
        res = {"rc": None, "why": None, "sq": [], "ref": {}, "rg": {}, "pg": {}, "text": text}
        for line in head.splitlines():
            kind, _, rest = line.partition(" ")
            if kind == "rc":
                res["rc"] = int(rest)
            elif kind == "why":
                res["why"] = rest
            elif kind == "sq":
                res["sq"] = [(x.rsplit(":", 1)[0], int(x.rsplit(":", 1)[1])) for x in rest.split(",") if x]
            elif kind == "ref":
                f, _, ids = rest.partition(" ")
                res["ref"][int(f)] = [int(x) for x in ids.split(",") if x]
            else:
                f, _, pair = rest.partition(" ")
                old, new = pair.split("\t")
                res[kind].setdefault(int(f), {})[old] = new
        return res
    return run


def check(host, texts, text=None, sq=None, ref=None, rg=None, pg=None):
    """The three implementations against the hand-written answer (every part that is given)."""
    import sambamba_amd
    got = host(texts)
    assert got["rc"] == 0, got["why"]
    r_text, r_sq, r_maps = merge_ref.merge_headers(texts)
    assert got["text"] == r_text == sambamba_amd.merge_header_text(texts)
    assert got["sq"] == r_sq
    for f in range(len(texts)):
        assert got["ref"].get(f, []) == r_maps[f]["ref"]
        assert got["rg"].get(f, {}) == r_maps[f]["rg"] and got["pg"].get(f, {}) == r_maps[f]["pg"]
    if text is not None:
        assert got["text"] == text
    if sq is not None:
        assert got["sq"] == sq
    for name, want in (("ref", ref), ("rg", rg), ("pg", pg)):
        if want is not None:
            assert [got[name].get(f, {} if name != "ref" else []) for f in range(len(texts))] == want
    return got


def refused(host, texts, code, message):
    import sambamba_amd
    got = host(texts)
    assert (got["rc"], got["why"]) == (code, message)
    with pytest.raises(sambamba_amd.SbxError) as e:
        sambamba_amd.merge_header_text(texts)
    assert (e.value.code, e.value.msg) == (code, message)
    with pytest.raises(merge_ref.MergeError) as e2:
        merge_ref.merge_headers(texts)
    assert str(e2.value) == message


def test_the_references_unittest_headers(host):
    """samheadermerger.d:303-400, restated as data; the unittest pins the @SQ order, the comments and the SETS of ids."""
    h1 = header(sq=[("A", 100), ("B", 200), ("C", 300)], rg=[("A", "CN:CN1"), ("C", "CN:CN3")],
                pg=[("A", "X", None), ("B", "Y", "A"), ("C", "Z", "B"), ("D", "T", "B")], co=["abc"])
    h2 = header(sq=[("D", 100), ("B", 200), ("E", 300)], rg=[("B", "CN:CN2"), ("C", "CN:CN4")],
                pg=[("B", "Z", None), ("A", "Y", "B"), ("C", "T", "A")], co=["def", "ghi"])
    h3 = header(sq=[("A", 100), ("E", 300), ("C", 300)], rg=[("B", "CN:CN2"), ("A", "CN:CN4")],
                pg=[("D", "Y", None), ("C", "T", "D"), ("B", "X", "C")])
    got = check(host, [h1, h2, h3], sq=[("A", 100), ("D", 100), ("B", 200), ("E", 300), ("C", 300)],
                ref=[[0, 2, 4], [1, 2, 3], [0, 3, 4]],
                rg=[{"A": "A", "C": "C"}, {"B": "B", "C": "C.1"}, {"B": "B", "A": "A.1"}],
                pg=[{"A": "A", "B": "B.1", "C": "C.1", "D": "D.1"}, {"B": "B", "A": "A.1", "C": "C.2"}, {"D": "D", "C": "C", "B": "B.2"}])
    lines = got["text"].splitlines()
    assert lines[0] == "@HD\tVN:1.3\tSO:coordinate"
    assert sorted(x.split("\t")[1][3:] for x in lines if x.startswith("@PG")) == ["A", "A.1", "B", "B.1", "B.2", "C", "C.1", "C.2", "D", "D.1"]
    assert sorted(x.split("\t")[1][3:] for x in lines if x.startswith("@RG")) == ["A", "A.1", "B", "C", "C.1"]
    assert [x for x in lines if x.startswith("@CO")] == ["@CO\tabc", "@CO\tdef", "@CO\tghi"]
    # the defined order: level by level, inputs in order, and every child's PP follows its parent's new id
    assert [x for x in lines if x.startswith("@PG")] == [
        "@PG\tID:A\tPN:X", "@PG\tID:B\tPN:Z", "@PG\tID:D\tPN:Y",
        "@PG\tID:B.1\tPN:Y\tPP:A", "@PG\tID:A.1\tPN:Y\tPP:B", "@PG\tID:C\tPN:T\tPP:D",
        "@PG\tID:C.1\tPN:Z\tPP:B.1", "@PG\tID:D.1\tPN:T\tPP:B.1", "@PG\tID:C.2\tPN:T\tPP:A.1", "@PG\tID:B.2\tPN:X\tPP:C"]


def test_a_single_header_is_kept(host):
    """sambamba issue 110 (samheadermerger.d:394-403)."""
    check(host, [header(sq=[("A", 100)])], text="@HD\tVN:1.3\tSO:coordinate\n@SQ\tSN:A\tLN:100\n", ref=[[0]])


def test_identical_lines_are_one_line(host):
    h = header(sq=[("c", 5)], rg=[("x", "SM:s\tLB:l")], pg=[("bwa", "bwa", None)])
    check(host, [h, h], text="@HD\tVN:1.3\tSO:coordinate\n@SQ\tSN:c\tLN:5\n@RG\tID:x\tLB:l\tSM:s\n@PG\tID:bwa\tPN:bwa\n",
          rg=[{"x": "x"}, {"x": "x"}], pg=[{"bwa": "bwa"}, {"bwa": "bwa"}])


def test_same_id_with_other_fields_is_renamed(host):
    a, b = header(sq=[("c", 5)], rg=[("x", "SM:s1")]), header(sq=[("c", 5)], rg=[("x", "SM:s2")])
    check(host, [a, b], text="@HD\tVN:1.3\tSO:coordinate\n@SQ\tSN:c\tLN:5\n@RG\tID:x\tSM:s1\n@RG\tID:x.1\tSM:s2\n", rg=[{"x": "x"}, {"x": "x.1"}])


def test_the_first_free_suffix_is_taken(host):
    a = header(sq=[("c", 5)], rg=[("x", "SM:s1"), ("x.1", "SM:other")])
    b = header(sq=[("c", 5)], rg=[("x", "SM:s2")])
    check(host, [a, b], rg=[{"x": "x", "x.1": "x.1"}, {"x": "x.2"}],
          text="@HD\tVN:1.3\tSO:coordinate\n@SQ\tSN:c\tLN:5\n@RG\tID:x\tSM:s1\n@RG\tID:x.1\tSM:other\n@RG\tID:x.2\tSM:s2\n")


def test_three_files_one_id(host):
    hs = [header(sq=[("c", 5)], rg=[("x", "SM:s%d" % k)]) for k in (1, 2, 1, 3)]
    check(host, hs, rg=[{"x": "x"}, {"x": "x.1"}, {"x": "x"}, {"x": "x.2"}])


def test_pg_chain_follows_the_renamed_parent(host):
    a = header(sq=[("c", 5)], pg=[("bwa", "bwa", None), ("sort", "samtools", "bwa")])
    b = header(sq=[("c", 5)], pg=[("sort", "sambamba", "bwa"), ("bwa", "bowtie", None)])
    check(host, [a, b], pg=[{"bwa": "bwa", "sort": "sort"}, {"bwa": "bwa.1", "sort": "sort.1"}],
          text="@HD\tVN:1.3\tSO:coordinate\n@SQ\tSN:c\tLN:5\n@PG\tID:bwa\tPN:bwa\n@PG\tID:bwa.1\tPN:bowtie\n"
               "@PG\tID:sort\tPN:samtools\tPP:bwa\n@PG\tID:sort.1\tPN:sambamba\tPP:bwa.1\n")


def test_pg_whose_parent_is_missing_is_never_reached(host):
    a = header(sq=[("c", 5)], pg=[("bwa", "bwa", None)])
    b = header(sq=[("c", 5)], pg=[("lost", "x", "nowhere"), ("child", "y", "lost"), ("self", "z", "self"), ("bwa", "bwa", None)])
    check(host, [a, b], pg=[{"bwa": "bwa"}, {"bwa": "bwa"}], text="@HD\tVN:1.3\tSO:coordinate\n@SQ\tSN:c\tLN:5\n@PG\tID:bwa\tPN:bwa\n")


def test_interleaved_dictionaries(host):
    a, b = header(sq=[("chr1", 10), ("chr2", 20), ("chr3", 30)]), header(sq=[("chr2", 20), ("chr4", 40)])
    check(host, [a, b], sq=[("chr1", 10), ("chr2", 20), ("chr3", 30), ("chr4", 40)], ref=[[0, 1, 2], [1, 3]])
    # a line keeps the @SQ text of its first appearance
    a2 = HD + "@SQ\tSN:chr1\tLN:10\tAS:first\n"
    b2 = HD + "@SQ\tSN:chr0\tLN:5\n@SQ\tSN:chr1\tLN:10\tAS:second\n"
    check(host, [a2, b2], text="@HD\tVN:1.3\tSO:coordinate\n@SQ\tSN:chr0\tLN:5\n@SQ\tSN:chr1\tLN:10\tAS:first\n", ref=[[1], [0, 1]])


def test_a_cycle_falls_back_to_the_names_in_byte_order(host):
    a, b = header(sq=[("b", 2), ("a", 1), ("Z", 3)]), header(sq=[("a", 1), ("b", 2), ("c", 4)])
    check(host, [a, b], sq=[("Z", 3), ("a", 1), ("b", 2), ("c", 4)], ref=[[2, 1, 0], [1, 2, 3]])


def test_one_name_two_lengths(host):
    a, b = header(sq=[("chr1", 10)]), header(sq=[("chr1", 11)])
    refused(host, [a, b], -1, "can't merge SAM headers: one of references with name chr1 has length 10 while another one with the same "
                               "name has length 11")


def test_sorting_orders(host):
    co, qn, un = header(sq=[("c", 5)]), header(sq=[("c", 5)], hd="@HD\tVN:1.6\tSO:queryname\n"), header(sq=[("c", 5)], hd="@HD\tVN:1.6\tSO:unsorted\n")
    none = header(sq=[("c", 5)], hd="")
    for first in (un, none):
        refused(host, [first, co], -1, "file headers indicate that some files are not sorted")
    for pair in ([co, qn], [qn, co], [co, un], [co, co, none]):
        refused(host, pair, -1, "sorting orders of files don't agree, can't merge")
    import sambamba_amd
    got = host([qn, qn])                             # (the name orders are not built: the library's own refusal, SBX_EUNSUPPORTED)
    assert (got["rc"], got["why"]) == (-5, "the files are sorted by read name: sbx-merge merges by coordinate only")
    with pytest.raises(sambamba_amd.SbxError) as e:
        sambamba_amd.merge_header_text([qn, qn])
    assert (e.value.code, e.value.msg) == (-5, got["why"])


def test_comments_in_input_order(host):
    hs = [header(sq=[("c", 5)], co=c) for c in (["b", "a"], [], ["a", ""])]
    got = check(host, hs)
    assert [x for x in got["text"].split("\n") if x.startswith("@CO")] == ["@CO\tb", "@CO\ta", "@CO\ta", "@CO\t"]


def test_a_text_the_parser_throws_on(host):
    import sambamba_amd
    got = host([header(sq=[("c", 5)]), "junk line\n"])
    assert got["rc"] == -3 and got["why"].startswith("SAM header of input 2: ")
    with pytest.raises(sambamba_amd.SbxError) as e:
        sambamba_amd.merge_header_text([header(sq=[("c", 5)]), "junk line\n"])
    assert e.value.code == -3
