"""The windowed path of `sbx_merge_bam` (K11c, merge.hip; the writer with several sources, engine_windows.hpp): inputs whose records
do not stay on the device are merged through a key pass and written window by window, every window filled by passing the inputs
that meet it through the read pass again.  No set of test files is larger than the device: SBX_MERGE_WINDOW_BYTES forces the path,
with windows of one or a few pieces, and SBX_BGZF_PIECE_BLOCKS=1 makes a piece -- the smallest window -- 65 280 bytes.  Every case
asserts that the output inflates to the restatement's stream (tests/merge_ref.py) and that the FILE is, byte for byte, the one the
same call writes without SBX_MERGE_WINDOW_BYTES, which reports n_windows == 0."""
import os
import random
import struct
import subprocess

import pytest

from tests import bamgen
from tests import merge_ref as ref
from tests import sort_ref
from tests.flagstat_ref import inflate
from tests.test_gpu_merge import POOL, check_file, records, text_of, write
from tests.test_gpu_sort_windows import _filler, _minimal

pytestmark = pytest.mark.gpu

P = 0xFF00                       # one piece with SBX_BGZF_PIECE_BLOCKS=1
WINDOW_KEYS = ("n_windows", "n_batch_runs", "n_batches_skipped", "n_input_opens", "window_bytes", "ms_dest", "ms_scatter", "ms_inflate_replay",
               "ms_index_replay")


def _env(window=None, batch=None, force=False):
    e = {"SBX_BGZF_PIECE_BLOCKS": "1"}
    if window is not None:
        e["SBX_MERGE_WINDOW_BYTES"] = str(window)
    if batch is not None:
        e["SBX_INDEX_BATCH_BYTES"] = str(batch)
    if force:
        e["SBX_MERGE_FORCE_REWRITE"] = "1"
    return e


def api_merge(monkeypatch, out, paths, window=None, batch=None, flt=None, force=False, index=False):
    import sambamba_amd
    with monkeypatch.context() as m:
        for k in ("SBX_MERGE_WINDOW_BYTES", "SBX_INDEX_BATCH_BYTES", "SBX_MERGE_FORCE_REWRITE", "SBX_TIMING"):
            m.delenv(k, raising=False)
        for k, v in _env(window, batch, force).items():
            m.setenv(k, v)
        return sambamba_amd.merge(out, paths, filter=flt, index=index)


def both_paths(monkeypatch, tmp_path, paths, want, window, batch=None, flt=None, force=False, tag="w"):
    """The resident file and the windowed one: the stream is `want`, the two files are the same bytes.  Returns both stats."""
    res, win = str(tmp_path / (tag + ".res.bam")), str(tmp_path / (tag + ".win.bam"))
    st = api_merge(monkeypatch, res, paths, batch=batch, flt=flt, force=force)
    assert all(st[k] == 0 for k in WINDOW_KEYS), st                      # the resident path: every figure of the windows is 0
    check_file(res, want)
    sw = api_merge(monkeypatch, win, paths, window=window, batch=batch, flt=flt, force=force)
    check_file(win, want)
    assert open(win, "rb").read() == open(res, "rb").read()
    span = -(-window // P) * P
    assert sw["n_windows"] == -(-len(want) // span) and sw["window_bytes"] == span
    for k in ("n_records_in", "n_records_out", "n_records_rewritten", "bytes_grown", "merged_stream_bytes", "compressed_bytes", "n_inputs", "n_batches"):
        assert sw[k] == st[k], k
    assert sw["merged_stream_bytes"] == len(want)
    return st, sw


def _three_inputs(tmp_path, n, seed, sort=True):
    """Different dictionaries, colliding @RG / @PG ids: nothing changes in the first input, the two others are rewritten."""
    refs = POOL[:3]
    specs = [(refs, [("x", "s1")], [("p", "bwa", None)]), ([refs[1], POOL[3]], [("x", "s2")], [("p", "bowtie", None)]), (refs, [("x", "s3")], [("p", "bwa", None)])]
    paths = []
    for k, (rf, rg, pg) in enumerate(specs):
        recs = records(n, len(rf), seed + k, rgs=["x"], pgs=["p"], sort=sort)
        paths.append(write(str(tmp_path / ("m%d_%d.bam" % (seed, k))), rf, recs, text=text_of(rf, rg=rg, pg=pg), block_size=9000))
    return paths


# ---- 1. windows x batches x inputs ---------------------------------------------------------------------------------------------------
def test_windows_times_batches_times_inputs(tmp_path, monkeypatch):
    paths = _three_inputs(tmp_path, 3000, 20)
    want = ref.expected(paths)
    st, sw = both_paths(monkeypatch, tmp_path, paths, want, P, batch=40000)
    assert sw["n_windows"] >= 8 and sw["n_windows"] == -(-len(want) // P)
    # at 40 000 inflated bytes per batch every input makes three batches and more
    assert all(len(inflate(p)) // 40000 >= 3 for p in paths) and st["n_batches"] >= 9
    assert 0 < st["n_records_rewritten"] < 9000 and st["bytes_grown"] > 0
    assert sw["n_batch_runs"] >= sw["n_windows"] and sw["n_input_opens"] >= 3
    # K11c for the input nothing changes in too: the same file
    forced = str(tmp_path / "forced.bam")
    sf = api_merge(monkeypatch, forced, paths, window=P, batch=40000, force=True)
    assert sf["n_windows"] == sw["n_windows"]
    assert open(forced, "rb").read() == open(str(tmp_path / "w.res.bam"), "rb").read()


# ---- 2. edges of the clip in a rewritten record ---------------------------------------------------------------------------------------
def _tagged(pos, name, pg=True):
    """38 bytes + RG:Z:x (+ PG:Z:p).  Rewritten, x becomes x.1 and p becomes p.1: 52 bytes, the new ids at [41, 44) and [48, 51)."""
    return _minimal(pos, name, bamgen.tag_z("RG", "x") + (bamgen.tag_z("PG", "p") if pg else b""))


def test_edges_of_the_clip_in_a_rewritten_record(tmp_path, monkeypatch):
    """Window edges (multiples of P) at chosen bytes of rewritten records.  The ids the header merge hands out only ever gain a
    ".N" suffix, so a new id SHORTER than the old one cannot be made through the interface: the record with two patches here has
    two ids that both grow; shorter ids are covered on the CPU (tests/test_merge_window_core_cpu.py)."""
    a_refs, b_refs = [("c1", 1000000), ("c2", 900000)], [("c2", 900000)]
    a_text = text_of(a_refs, rg=[("x", "s1")], pg=[("p", "bwa", None)], co=["padded " + "x" * 211])
    b_text = text_of(b_refs, rg=[("x", "s2")], pg=[("p", "bowtie", None)])
    # the one record of the first input is unplaced: it goes last, and the records of the second input follow the header
    a_recs = [bamgen.make_record(-1, -1, "", "ACGT", 30, name="last", mapq=0, flag=0x4, tags=bamgen.tag_z("RG", "x"))]
    hlen = len(ref.expected_stream([bamgen.bam_header(a_text, a_refs), bamgen.bam_header(b_text, b_refs)]))
    # (offset of the edge in the rewritten record, what lies there)
    edges = [(1, "one byte into block_size"), (6, "inside ref_id"), (26, "inside next_ref_id"), (41, "on the first byte of a new id"),
             (43, "on the last byte of a new id"), (44, "between a new id and the stretch behind it"), (0, "between two records"),
             (46, "between the two patches of a record"), (49, "inside the second new id of a record with two patches")]
    b_recs, special, cur, pos = [], [], hlen, 10
    for off, _ in edges:
        start = cur + 47
        start += -(start + off) % P
        b_recs.append(_filler(pos, start - cur))
        b_recs.append(_tagged(pos + 5, "t"))
        special.append((len(b_recs) - 1, off))
        cur, pos = start + 52, pos + 10
    # one record longer than three windows, its patch at the very end
    b_recs.append(bamgen.make_record(0, pos, "150000M", "ACGTTGCA" * 18750, 30, name="l", tags=bamgen.tag_z("RG", "x")))
    cur, pos = cur + len(b_recs[-1]) + 2, pos + 10
    assert len(b_recs[-1]) > 3 * P
    # ... and the stream ends on a window edge
    tail = 47 + (-(cur + 47 + len(a_recs[0])) % P)
    b_recs.append(_filler(pos, tail))
    a = write(str(tmp_path / "a.bam"), a_refs, a_recs, text=a_text)
    b = write(str(tmp_path / "b.bam"), b_refs, b_recs, text=b_text, block_size=30000)
    want = ref.expected([a, b])
    # the layout is the one intended
    got = sort_ref.split_stream(want)[3]
    assert len(got) == len(b_recs) + 1 and len(want) % P == 0 and len(want) - sum(len(r) for r in got) == hlen
    starts, p = [], hlen
    for r in got:
        starts.append(p)
        p += len(r)
    for i, off in special:
        assert len(got[i]) == 52 and got[i][41:44] == b"x.1" and got[i][48:51] == b"p.1" and (starts[i] + off) % P == 0, (i, off)
        assert struct.unpack_from("<i", got[i], 4)[0] == 1                   # c2 is reference 1 of the merged dictionary
    long_at = len(b_recs) - 2
    assert got[long_at].endswith(b"RGZx.1\0") and len({(starts[long_at] + j) // P for j in range(len(got[long_at]))}) >= 4
    st, sw = both_paths(monkeypatch, tmp_path, [a, b], want, P, batch=40000, tag="p1")
    assert sw["n_windows"] == len(want) // P and st["n_records_rewritten"] == len(b_recs)
    # windows of a piece and a half round up to two
    _, s2 = both_paths(monkeypatch, tmp_path, [a, b], want, P + P // 2, batch=40000, tag="p2")
    assert s2["window_bytes"] == 2 * P
    both_paths(monkeypatch, tmp_path, [a, b], want, P, batch=40000, force=True, tag="pf")


# ---- 3. ties across inputs and batches --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("force", [False, True], ids=["copied", "rewritten"])
def test_ties_across_inputs_and_batches(tmp_path, monkeypatch, force):
    refs = POOL[:1]
    paths = []
    for k in range(3):
        recs = [bamgen.make_record(0, 100, "4M", "ACGT", 30, name="in%d_%04d" % (k, i), flag=0x10 * (i >= 700)) for i in range(1400)]
        paths.append(write(str(tmp_path / ("t%d.bam" % k)), refs, recs, block_size=8000))
    want = ref.expected(paths)
    st, sw = both_paths(monkeypatch, tmp_path, paths, want, P, batch=16000, force=force)
    assert st["n_batches"] >= 9 and sw["n_windows"] >= 3                   # batches of a few hundred records
    names = [r[36:36 + r[12] - 1].decode() for r in sort_ref.split_stream(inflate(str(tmp_path / "w.win.bam")))[3]]
    fwd = ["in%d_%04d" % (k, i) for k in range(3) for i in range(700)]
    assert names == fwd + ["in%d_%04d" % (k, i) for k in range(3) for i in range(700, 1400)]      # lower input first, then file order


# ---- 4. filter ------------------------------------------------------------------------------------------------------------------------
def test_filter(tmp_path, monkeypatch):
    refs = POOL[:2]
    a = write(str(tmp_path / "a.bam"), refs, records(2500, 2, 40, rgs=["x"]), text=text_of(refs, rg=[("x", "s1")]), block_size=9000)
    b = write(str(tmp_path / "b.bam"), [refs[1], refs[0]], records(2500, 2, 41, rgs=["x"]), text=text_of([refs[1], refs[0]], rg=[("x", "s2")]), block_size=9000)
    want = ref.expected([a, b], lambda rec: rec[13] >= 30)
    st, sw = both_paths(monkeypatch, tmp_path, [a, b], want, P, batch=40000, flt="mapping_quality >= 30")
    assert 0 < st["n_records_out"] < st["n_records_in"] == 5000 and sw["n_windows"] >= 2
    # nothing changes in the first input (it is copied), every reference id of the second changes (it is rewritten)
    assert ref.merge_headers([sort_ref.split_stream(inflate(p))[0].decode() for p in (a, b)])[2][0]["ref"] == [0, 1]
    assert 0 < st["n_records_rewritten"] < st["n_records_out"]
    # nothing passes: the header alone
    want = ref.expected([a, b], lambda rec: False)
    st, sw = both_paths(monkeypatch, tmp_path, [a, b], want, P, batch=40000, flt="mapping_quality > 100", tag="none")
    assert st["n_records_out"] == 0 and sort_ref.split_stream(want)[3] == []
    assert sw["n_windows"] == 1 and sw["n_batch_runs"] == 0 and sw["n_input_opens"] == 0


# ---- 5. skipping and opens --------------------------------------------------------------------------------------------------------------
def _placed(n, r, seed):
    rng = random.Random(seed)
    out = [bamgen.make_record(r, rng.randrange(70000), "8M", "ACGTACGT", 30, name="q%d_%04d" % (seed, i), flag=0x10 * rng.randrange(2),
                              tags=bamgen.tag_z("RG", "x")) for i in range(n)]
    return sorted(out, key=lambda b: sort_ref.record_key(b, 2))


def test_batches_and_inputs_outside_a_window_are_skipped(tmp_path, monkeypatch):
    # coordinate-sorted inputs: the spans of an input's batches are disjoint and ascending, so a batch is run once, and once more
    # for every window edge inside its span -- of which an input has at most n_windows - 1
    paths = _three_inputs(tmp_path, 3000, 60)
    want = ref.expected(paths)
    st, sw = both_paths(monkeypatch, tmp_path, paths, want, P, batch=30000)
    n_batches, n_windows = st["n_batches"], sw["n_windows"]
    assert n_windows >= 8 and n_batches >= 15
    assert sw["n_batch_runs"] + sw["n_batches_skipped"] == n_batches * n_windows
    assert sw["n_batch_runs"] <= n_batches + 3 * (n_windows - 1) and sw["n_batches_skipped"] > 0
    # two inputs on disjoint references: one window at most meets both, every other window opens one input (or keeps it open)
    refs = POOL[:2]
    text1, text2 = text_of(refs, rg=[("x", "s1")]), text_of(refs, rg=[("x", "s2")])
    one, two = _placed(4000, 0, 71), _placed(4000, 1, 72)
    figures = {}
    for name, (r1, r2) in (("sorted", (one, two)), ("shuffled", (random.Random(5).sample(one, len(one)), random.Random(6).sample(two, len(two))))):
        pair = [write(str(tmp_path / (name + "1.bam")), refs, r1, text=text1, block_size=9000),
                write(str(tmp_path / (name + "2.bam")), refs, r2, text=text2, block_size=9000)]
        want = ref.expected(pair)
        st, sw = both_paths(monkeypatch, tmp_path, pair, want, P, batch=30000, tag=name)
        assert sw["n_windows"] >= 6 and st["n_batches"] >= 12
        assert sw["n_batch_runs"] + sw["n_batches_skipped"] == st["n_batches"] * sw["n_windows"]
        assert sw["n_input_opens"] <= sw["n_windows"] + 1
        figures[name] = (st["n_batches"], sw["n_windows"], sw["n_batch_runs"])
    n_batches, n_windows, runs = figures["sorted"]
    assert runs <= n_batches + 2 * (n_windows - 1), figures
    n_batches, n_windows, runs = figures["shuffled"]
    assert runs > n_batches + 2 * (n_windows - 1), figures                 # the bound above is not vacuous


# ---- 6. empty inputs, one window ------------------------------------------------------------------------------------------------------------
def test_empty_inputs_and_one_window(tmp_path, monkeypatch):
    refs = POOL[:2]
    full = write(str(tmp_path / "f.bam"), refs, records(1500, 2, 30, rgs=["x"]), text=text_of(refs, rg=[("x", "s1")]))
    empty = write(str(tmp_path / "e.bam"), refs, [], text=text_of(refs, rg=[("x", "s2")]))
    full2 = write(str(tmp_path / "g.bam"), refs, records(1400, 2, 31, rgs=["x"]), text=text_of(refs, rg=[("x", "s3")]))
    paths = [full, empty, full2]
    want = ref.expected(paths)
    st, sw = both_paths(monkeypatch, tmp_path, paths, want, P)
    assert st["n_records_in"] == 2900 and sw["n_windows"] >= 2
    # a hook larger than the stream: one window
    _, s1 = both_paths(monkeypatch, tmp_path, paths, want, 1 << 30, tag="one")
    assert s1["n_windows"] == 1 and s1["n_batch_runs"] == 2 and s1["n_input_opens"] == 2
    # all inputs empty
    empties = [empty, write(str(tmp_path / "e2.bam"), refs, [], text=text_of(refs, rg=[("x", "s1")])), empty]
    want = ref.expected(empties)
    st, sw = both_paths(monkeypatch, tmp_path, empties, want, P, tag="none")
    assert st["n_records_out"] == 0 and sw["n_windows"] == 1 and sw["n_batch_runs"] == 0
    # a hook that is no positive decimal number counts as unset
    import sambamba_amd
    for bad in ("0", "-5", "64k", ""):
        with monkeypatch.context() as m:
            m.setenv("SBX_MERGE_WINDOW_BYTES", bad)
            assert sambamba_amd.merge(str(tmp_path / "unset.bam"), paths)["n_windows"] == 0


# ---- 7. failure leaves nothing --------------------------------------------------------------------------------------------------------------
def test_failure_leaves_nothing(tmp_path, monkeypatch):
    import sambamba_amd
    refs = POOL[:1]
    good = bamgen.make_record(0, 100, "4M", "ACGT", 30, name="ok", tags=bamgen.tag_z("RG", "x"))
    bad = bamgen.make_record(0, 200, "4M", "ACGT", 30, name="bad", tags=bamgen.tag_z("RG", "x") + b"XZZ" + b"abc")     # no NUL before the record ends
    a = write(str(tmp_path / "a.bam"), refs, [good] * 50, text=text_of(refs, rg=[("x", "s1")]))
    b = str(tmp_path / "b.bam")
    stream = bamgen.bam_header(text_of(refs, rg=[("x", "s2")]), refs) + good + bad + good
    open(b, "wb").write(bamgen.bgzf_block(stream) + bamgen.EOF_BLOCK)
    out = str(tmp_path / "fail.bam")
    with pytest.raises(sambamba_amd.SbxError) as ei:
        api_merge(monkeypatch, out, [a, a, b], window=P, index=True)
    assert ei.value.code == -3 and ei.value.msg.startswith("malformed BAM record in ") and "b.bam" in ei.value.msg, ei.value
    assert not os.path.exists(out) and not os.path.exists(out + ".bai")


# ---- 8. the command line ------------------------------------------------------------------------------------------------------------------
def test_cli(tmp_path):
    from sambamba_amd import merge_cli_path
    paths = _three_inputs(tmp_path, 1500, 80)
    want = ref.expected(paths)
    outs = {}
    for name, window in (("res", None), ("win", P)):
        out = str(tmp_path / (name + ".bam"))
        r = subprocess.run([merge_cli_path(), out] + paths, stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                           env=dict(os.environ, SBX_TIMING="1", **_env(window, 40000)))
        assert r.returncode == 0, r.stderr
        lines = r.stderr.decode().splitlines()
        assert len([x for x in lines if x.startswith("[sbx] merge:")]) == 1
        outs[name] = (out, [x for x in lines if x.startswith("[sbx] merge-windows:")])
        check_file(out, want)
    assert outs["res"][1] == [] and len(outs["win"][1]) == 1
    f = dict(kv.split("=") for kv in outs["win"][1][0].split()[2:])
    assert list(f) == list(WINDOW_KEYS[:1] + ("window_bytes",) + WINDOW_KEYS[1:4] + WINDOW_KEYS[5:])
    assert int(f["n_windows"]) == -(-len(want) // P) >= 3 and int(f["window_bytes"]) == P and int(f["n_input_opens"]) >= 3
    assert open(outs["win"][0], "rb").read() == open(outs["res"][0], "rb").read()
    assert open(outs["win"][0] + ".bai", "rb").read() == open(outs["res"][0] + ".bai", "rb").read()
