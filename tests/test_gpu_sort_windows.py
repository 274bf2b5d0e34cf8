"""The windowed path of `sbx_sort_bam` (K9d, sort.hip): a file whose records do not stay on the device is written window by window,
every window filled by passing the file through the read pass again.  No test file is larger than the device: SBX_SORT_WINDOW_BYTES
forces the path, with windows of one or a few pieces, and SBX_BGZF_PIECE_BLOCKS=1 makes a piece -- the smallest window -- 65 280
bytes.  Every case asserts that the output inflates to the restatement's stream (tests/sort_ref.py) and that the FILE is, byte for
byte, the one the same call writes without SBX_SORT_WINDOW_BYTES."""
import os
import random
import struct
import subprocess

import pytest

from tests import bamgen
from tests import sort_ref as ref
from tests.test_gpu_sort import check_file

pytestmark = pytest.mark.gpu

P = 0xFF00                       # one piece with SBX_BGZF_PIECE_BLOCKS=1
REFS = [("c1", 1000000), ("c2", 500000)]
TEXT = "@HD\tVN:1.6\tSO:unsorted\n@SQ\tSN:c1\tLN:1000000\n@SQ\tSN:c2\tLN:500000\n@CO\tmade by the test-suite\n"


def _env(window=None, batch=None):
    e = {"SBX_BGZF_PIECE_BLOCKS": "1", "SBX_TIMING": "1"}
    if window is not None:
        e["SBX_SORT_WINDOW_BYTES"] = str(window)
    if batch is not None:
        e["SBX_INDEX_BATCH_BYTES"] = str(batch)
    return e


def _fields(stderr, prefix):
    lines = [x for x in stderr.decode().splitlines() if x.startswith(prefix)]
    assert len(lines) <= 1
    return dict(kv.split("=") for kv in lines[0].split("(")[0].split()[2:] if "=" in kv) if lines else None


def cli_sort(path, out, window=None, batch=None, flt=None):
    """sbx-sort in a process of its own; returns (fields of the `[sbx] sort:` line, fields of the `[sbx] sort-windows:` line or None)."""
    from sambamba_amd import sort_cli_path
    r = subprocess.run([sort_cli_path(), "-o", out, path] + (["-F", flt] if flt else []), stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                       env=dict(os.environ, **_env(window, batch)))
    assert r.returncode == 0, r.stderr
    sort = _fields(r.stderr, "[sbx] sort:")
    assert sort is not None
    return sort, _fields(r.stderr, "[sbx] sort-windows:")


def api_sort(monkeypatch, path, out, window=None, batch=None, flt=None, index=False):
    import sambamba_amd
    with monkeypatch.context() as m:
        for k in ("SBX_SORT_WINDOW_BYTES", "SBX_INDEX_BATCH_BYTES", "SBX_TIMING"):
            m.delenv(k, raising=False)
        for k, v in _env(window, batch).items():
            if k != "SBX_TIMING":
                m.setenv(k, v)
        return sambamba_amd.sort_bam(path, out, filter=flt, index=index)


def both_paths(monkeypatch, tmp_path, path, want, window, batch=None, flt=None, tag="w"):
    """The resident file (API) and the windowed one (CLI): the stream is `want`, the two files are the same bytes.  Returns the
    resident stats and the fields of the windowed run's two lines."""
    res, win = str(tmp_path / (tag + ".res.bam")), str(tmp_path / (tag + ".win.bam"))
    st = api_sort(monkeypatch, path, res, batch=batch, flt=flt)
    assert st["n_windows"] == 0
    check_file(res, want)
    sort, w = cli_sort(path, win, window=window, batch=batch, flt=flt)
    assert w is not None
    check_file(win, want)
    assert open(win, "rb").read() == open(res, "rb").read()
    assert int(sort["n_records_out"]) == st["n_records_out"] and int(sort["sorted_stream_bytes"]) == len(want)
    assert int(w["n_windows"]) == -(-len(want) // (-(-window // P) * P)) and int(w["window_bytes"]) == -(-window // P) * P
    return st, sort, w


def _records(n, seed, mapq=None, keys=None, unplaced=0.0):
    rng = random.Random(seed)
    recs = []
    for i in range(n):
        seq = "".join(rng.choice("ACGT") for _ in range(rng.randrange(40, 90)))
        flag = 0x10 if rng.random() < 0.5 else 0
        mq = mapq(i, rng) if mapq else 60
        if rng.random() < unplaced:
            recs.append(bamgen.make_record(-1, rng.choice((-1, 5)), "", seq, 30, name="n%05d" % i, mapq=0, flag=0x4 | flag))
            continue
        r, pos, strand = keys[rng.randrange(len(keys))] if keys else (rng.choice((0, 0, 1)), rng.randrange(0, 400000), flag)
        recs.append(bamgen.make_record(r, pos, "%dM" % len(seq), seq, 30, name="n%05d" % i, mapq=mq, flag=0x10 if strand else 0))
    return recs


# ---- 1. windows x batches ------------------------------------------------------------------------------------------------------------
def test_windows_times_batches(tmp_path, monkeypatch):
    path = str(tmp_path / "in.bam")
    info = bamgen.write_bam(path, REFS, _records(4000, 1), text=TEXT, block_size=10000, write_index=False)
    assert 450000 < info["stream_len"] < 800000
    batch = info["stream_len"] // 12
    want = ref.expected(path)
    st_res, sort, w = both_paths(monkeypatch, tmp_path, path, want, P, batch)
    n_windows = int(w["n_windows"])
    assert n_windows >= 8 and int(sort["n_batches"]) >= 10
    assert int(w["n_batch_runs"]) >= 3 * n_windows
    # the API: the same file, and the windows counted in the stats
    out = str(tmp_path / "api.bam")
    st = api_sort(monkeypatch, path, out, window=P, batch=batch, index=True)
    assert st["n_windows"] == n_windows >= 8 and st["n_batches"] >= 10
    assert st["n_records_in"] == st["n_records_out"] == 4000 and st["sorted_stream_bytes"] == len(want)
    assert st["compressed_bytes"] == os.path.getsize(out)
    assert open(out, "rb").read() == open(str(tmp_path / "w.res.bam"), "rb").read()
    # the index is a pass of its own over the file written: the CLI's and the API's are the same
    assert open(out + ".bai", "rb").read() == open(str(tmp_path / "w.win.bam.bai"), "rb").read()


# ---- 2. edges of the clip --------------------------------------------------------------------------------------------------------------
def _minimal(pos, name, tags=b""):
    """The shortest record there is, plus tags: a one-byte name, no CIGAR, no sequence (unmapped, but placed at pos of c1)."""
    return bamgen.make_record(0, pos, "", "", 30, name=name, mapq=0, flag=0x4, tags=tags)


def _filler(pos, length, name="f"):
    """A record of exactly `length` bytes (>= 46 + len(name)): no sequence, one B:C aux array."""
    base = len(_minimal(pos, name, bamgen.tag_bytes("XX", b"")))
    assert length >= base
    r = _minimal(pos, name, bamgen.tag_bytes("XX", bytes((pos + j) % 251 for j in range(length - base))))
    assert len(r) == length
    return r


def _padded_text(hlen_want, refs, sq_text):
    """A header text whose OUTPUT header (text re-serialised + reference list) is exactly hlen_want bytes: an @CO line pads it."""
    def out_len(pad):
        text = "@HD\tVN:1.6\tSO:unsorted\n" + sq_text + "@CO\t" + "x" * pad + "\n"
        return text, len(bamgen.bam_header(ref.header_text(text), refs))
    _, h0 = out_len(0)
    assert hlen_want >= h0
    text, h = out_len(hlen_want - h0)
    assert h == hlen_want
    return text


def test_edges_of_the_clip(tmp_path, monkeypatch):
    refs = [("c1", 1000000)]
    m = len(_minimal(0, "a"))
    assert m == 38
    text = _padded_text(P - 1 - m, refs, "@SQ\tSN:c1\tLN:1000000\n")
    recs = [_minimal(10, "a"),            # [P - 39, P - 1)
            _minimal(20, "b"),            # [P - 1, P + 37): the edge P lies one byte into it
            _filler(30, (2 * P + 1 - m) - (P - 1 + m)),
            _minimal(40, "c"),            # ends at 2 P + 1: the edge 2 P is one byte before its end
            bamgen.make_record(0, 50, "150000M", "ACGTTGCA" * 18750, 30, name="l")]
    at = 2 * P + 1 + len(recs[-1])
    k = -(-(at + 100) // P)
    recs.append(_filler(60, k * P - at))                                # ends at k P: the edge lies exactly between two records
    recs.append(_minimal(70, "d"))
    recs.append(_filler(80, P - m))                                     # ... and the stream ends at (k + 1) P
    total = (k + 1) * P
    order = list(range(len(recs)))
    random.Random(3).shuffle(order)
    path = str(tmp_path / "edges.bam")
    bamgen.write_bam(path, refs, [recs[i] for i in order], text=text, block_size=30000, write_index=False)
    want = ref.expected(path)
    # the layout is the one intended
    assert len(want) == total and ref.split_stream(want)[3] == recs
    starts, p = [], P - 1 - m
    for r in recs:
        starts.append(p)
        p += len(r)
    assert starts[1] == P - 1 and starts[3] + m == 2 * P + 1 and starts[4] == 2 * P + 1 and starts[6] == k * P
    assert len(recs[4]) > 3 * P                                         # three windows and more write a part of the long record
    _, _, w = both_paths(monkeypatch, tmp_path, path, want, P, batch=40000, tag="p1")
    assert int(w["n_windows"]) == k + 1                                 # total is a multiple of the window: no empty last window
    _, _, w = both_paths(monkeypatch, tmp_path, path, want, 2 * P, batch=40000, tag="p2")
    assert int(w["n_windows"]) == -(-(k + 1) // 2)


# ---- 3. header -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["long_header", "header_ends_at_an_edge", "edge_and_no_records", "no_records"])
def test_header(kind, tmp_path, monkeypatch):
    refs = [("s%04d" % i, 1000 + i) for i in range(4200)]
    sq = "".join("@SQ\tSN:%s\tLN:%d\n" % r for r in refs)
    if kind in ("header_ends_at_an_edge", "edge_and_no_records"):
        text = _padded_text(3 * P, refs, sq)
    else:
        text = "@HD\tVN:1.6\tSO:unsorted\n" + sq
    recs = [] if kind.endswith("no_records") else [bamgen.make_record(r, pos, "8M", "ACGTACGT", 30, name="h%d" % i) for i, (r, pos) in
                                                   enumerate(((4199, 5), (0, 900), (2000, 0), (17, 3), (0, 2), (4199, 1)))]
    path = str(tmp_path / "h.bam")
    bamgen.write_bam(path, refs, recs, text=text, write_index=False)
    want = ref.expected(path)
    hlen = len(want) - sum(len(r) for r in recs)
    assert hlen > 2 * P and (hlen == 3 * P) == ("edge" in kind)
    st, sort, w = both_paths(monkeypatch, tmp_path, path, want, P)
    assert int(sort["n_records_out"]) == len(recs)
    assert int(w["n_windows"]) == {"long_header": 3, "header_ends_at_an_edge": 4, "edge_and_no_records": 3, "no_records": 3}[kind]


# ---- 4. filter -------------------------------------------------------------------------------------------------------------------------
def _mapq_of(rec):
    return (struct.unpack_from("<I", rec, 12)[0] >> 8) & 0xFF


@pytest.mark.parametrize("batch", ["small", "whole"])
def test_filter(batch, tmp_path, monkeypatch):
    path = str(tmp_path / "f.bam")
    info = bamgen.write_bam(path, REFS, _records(4000, 8, mapq=lambda i, rng: rng.choice((0, 10, 29, 30, 31, 60))), text=TEXT, block_size=10000,
                            write_index=False)
    b = info["stream_len"] // 12 if batch == "small" else None
    want = ref.expected(path, keep=lambda r: _mapq_of(r) >= 30)
    st, sort, w = both_paths(monkeypatch, tmp_path, path, want, P, b, flt="mapping_quality >= 30")
    assert 0 < st["n_records_out"] < st["n_records_in"] == 4000
    assert batch != "small" or int(sort["n_batches"]) >= 10
    # nothing passes: the header alone
    want = ref.expected(path, keep=lambda r: False)
    st, sort, w = both_paths(monkeypatch, tmp_path, path, want, P, b, flt="mapping_quality > 100", tag="none")
    assert st["n_records_out"] == 0 == int(sort["n_records_out"]) and ref.split_stream(want)[3] == []
    assert int(w["n_windows"]) == 1 and int(w["n_batch_runs"]) == 0


# ---- 5. stability ----------------------------------------------------------------------------------------------------------------------
def test_ties_keep_file_order(tmp_path, monkeypatch):
    rng = random.Random(12)
    keys = [(rng.choice((0, 1)), rng.choice((0, 7, 100, 399999)), s) for s in (0, 1) for _ in range(10)]
    path = str(tmp_path / "ties.bam")
    info = bamgen.write_bam(path, REFS, _records(2000, 13, keys=keys, unplaced=0.1), text=TEXT, block_size=10000, write_index=False)
    want = ref.expected(path)
    out = ref.split_stream(want)[3]
    by_key = {}
    for r in out:
        by_key.setdefault(ref.record_key(r, 2), []).append(r[36:42])
    assert len(by_key) <= 21 and all(v == sorted(v) for v in by_key.values())        # names carry the file index
    assert struct.unpack_from("<i", out[-1], 4)[0] == -1 and len(by_key[(2, 0, 0)]) > 100     # the unplaced records go last
    st, sort, w = both_paths(monkeypatch, tmp_path, path, want, P, info["stream_len"] // 8)
    assert int(sort["n_batches"]) >= 6 and int(w["n_windows"]) >= 3


# ---- 6. skipping -----------------------------------------------------------------------------------------------------------------------
def test_batches_outside_a_window_are_skipped(tmp_path, monkeypatch):
    recs = _records(4000, 21)
    n_ref = len(REFS)
    in_order = sorted(recs, key=lambda r: ref.record_key(r, n_ref))
    shuffled = list(recs)
    random.Random(22).shuffle(shuffled)
    figures = {}
    for name, rs in (("sorted", in_order), ("shuffled", shuffled)):
        path = str(tmp_path / (name + ".bam"))
        info = bamgen.write_bam(path, REFS, rs, text=TEXT, block_size=10000, write_index=False)
        want = ref.expected(path)
        _, sort, w = both_paths(monkeypatch, tmp_path, path, want, P, info["stream_len"] // 16, tag=name)
        figures[name] = (int(sort["n_batches"]), int(w["n_windows"]), int(w["n_batch_runs"]), int(w["n_batches_skipped"]))
        assert int(w["n_windows"]) >= 6 and int(sort["n_batches"]) >= 12
        assert int(w["n_batch_runs"]) + int(w["n_batches_skipped"]) == int(sort["n_batches"]) * int(w["n_windows"])
    n_batches, n_windows, runs, skipped = figures["sorted"]
    assert skipped > 0 and runs <= n_batches + 2 * n_windows, figures        # a batch meets only the windows its span touches
    n_batches, n_windows, runs, skipped = figures["shuffled"]
    assert runs > n_batches + 2 * n_windows, figures


# ---- 7. one window, 8. the resident path ----------------------------------------------------------------------------------------------
def test_one_window_and_the_resident_path(tmp_path, monkeypatch):
    path = str(tmp_path / "one.bam")
    bamgen.write_bam(path, REFS, _records(1500, 31, unplaced=0.05), text=TEXT, write_index=False)
    want = ref.expected(path)
    st, sort, w = both_paths(monkeypatch, tmp_path, path, want, 1 << 30)
    assert int(w["n_windows"]) == 1
    out = str(tmp_path / "api1.bam")
    assert api_sort(monkeypatch, path, out, window=1 << 30)["n_windows"] == 1
    assert open(out, "rb").read() == open(str(tmp_path / "w.res.bam"), "rb").read()
    # without the hook: the resident path, no window, no line
    sort, w = cli_sort(path, str(tmp_path / "r.bam"))
    assert w is None and int(sort["n_records_out"]) == 1500
    assert open(str(tmp_path / "r.bam"), "rb").read() == open(out, "rb").read()
