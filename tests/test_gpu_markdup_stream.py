"""The streamed path of `sbx_markdup` (K10e, K10b over the key store, K10f; markdup.hip): a file whose records do not stay on the
device is marked without a record store and written window by window, the batches of the read pass run again as the windows need
them.  No test file is larger than the device: SBX_MARKDUP_WINDOW_BYTES forces the path, and SBX_BGZF_PIECE_BLOCKS=1 makes a piece
-- the smallest window -- 65 280 bytes.  Every case asserts that the output inflates to the restatement's stream
(tests/markdup_ref.py) and that the FILE is, byte for byte, the one the same call writes without SBX_MARKDUP_WINDOW_BYTES: the
resident call goes through the API, the streamed one through the CLI in a process of its own."""
import ctypes as C
import os
import struct
import subprocess

import pytest

from tests import bamgen
from tests import markdup_cases as mc
from tests import markdup_ref as ref
from tests.flagstat_ref import inflate
from tests.test_gpu_markdup import check_file

pytestmark = pytest.mark.gpu

P = 0xFF00                       # one piece with SBX_BGZF_PIECE_BLOCKS=1
HOOKS = ("SBX_MARKDUP_WINDOW_BYTES", "SBX_INDEX_BATCH_BYTES", "SBX_TIMING", "SBX_MARKDUP_HASH_BITS")


def _env(window=None, batch=None, extra=None):
    e = {"SBX_BGZF_PIECE_BLOCKS": "1", "SBX_TIMING": "1"}
    if window is not None:
        e["SBX_MARKDUP_WINDOW_BYTES"] = str(window)
    if batch is not None:
        e["SBX_INDEX_BATCH_BYTES"] = str(batch)
    e.update(extra or {})
    return e


def _fields(stderr, prefix):
    lines = [x for x in stderr.decode().splitlines() if x.startswith(prefix)]
    assert len(lines) <= 1
    return dict(kv.split("=") for kv in lines[0].split("(")[0].split()[2:] if "=" in kv) if lines else None


def cli_markdup(args, window=None, batch=None, extra=None):
    """sbx-markdup in a process of its own; returns (fields of the `[sbx] markdup:` line, fields of `[sbx] markdup-stream:` or None)."""
    from sambamba_amd import markdup_cli_path
    env = {k: v for k, v in os.environ.items() if k not in HOOKS}
    r = subprocess.run([markdup_cli_path()] + list(args), stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=dict(env, **_env(window, batch, extra)),
                       timeout=300)
    assert r.returncode == 0, r.stderr
    md = _fields(r.stderr, "[sbx] markdup:")
    assert md is not None
    return md, _fields(r.stderr, "[sbx] markdup-stream:")


def api_markdup(monkeypatch, path, out, window=None, batch=None, extra=None, **kw):
    import sambamba_amd
    with monkeypatch.context() as m:
        for k in HOOKS:
            m.delenv(k, raising=False)
        for k, v in _env(window, batch, extra).items():
            if k != "SBX_TIMING":
                m.setenv(k, v)
        return sambamba_amd.markdup(path, out, **kw)


def both_paths(monkeypatch, tmp_path, path, window, batch=None, remove=False, level=-1, tag="w", extra=None, stream=None):
    """The resident file (API) and the streamed one (CLI): both inflate to the restatement's stream, the two files are the same bytes.
    Returns the resident stats, the fields of the streamed run's two lines and the stream."""
    res, win = str(tmp_path / (tag + ".res.bam")), str(tmp_path / (tag + ".win.bam"))
    args = (["-r"] if remove else []) + (["-l", str(level)] if level != -1 else []) + [path, win]
    cl = "markdup " + " ".join(args)
    st = api_markdup(monkeypatch, path, res, batch=batch, extra=extra, remove_duplicates=remove, level=level, command_line=cl)
    assert st["n_windows"] == 0 and st["n_batch_runs"] == 0 and st["window_bytes"] == 0 and st["key_store_bytes"] == 0
    want = ref.expected_stream(stream if stream is not None else inflate(path), remove, cl)
    check_file(res, want)
    md, w = cli_markdup(args, window=window, batch=batch, extra=extra)
    assert w is not None, "no `[sbx] markdup-stream:` line: the streamed path was not taken"
    check_file(win, want)
    assert open(win, "rb").read() == open(res, "rb").read()
    for k in ("n_records_in", "n_records_out", "n_end_pairs", "n_single_ends", "n_unmatched_pairs", "n_duplicates", "stream_bytes", "compressed_bytes"):
        assert int(md[k]) == st[k], k
    assert int(md["stream_bytes"]) == len(want) and int(md["compressed_bytes"]) == os.path.getsize(win)
    span = -(-window // P) * P
    assert int(w["n_windows"]) == -(-len(want) // span) and int(w["window_bytes"]) == span
    n_batches, n_windows = int(md["n_batches"]), int(w["n_windows"])
    assert int(w["n_batch_runs"]) + int(w["n_batches_skipped"]) == n_batches * n_windows
    # batches and windows are both consecutive intervals of one ordered stream: a batch is run again once per window it touches
    assert int(w["n_batch_runs"]) <= n_batches + n_windows - 1, (md, w)
    return st, md, w, want


def write(path, records, text=mc.TEXT, refs=mc.REFS, **kw):
    return bamgen.write_bam(str(path), refs, records, text=text, write_index=False, **kw)


def marked_names(records, stream):
    """name#occurrence of the records of an output stream written without -r that carry 0x400."""
    out = ref.split_stream(stream)[3]
    assert len(out) == len(records)
    return {n for n, r in zip(mc.labels(records), out) if struct.unpack_from("<H", r, 18)[0] & 0x400}


# ---- 1. windows x batches ------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def random_file(tmp_path_factory):
    # (the generator's records are ~80 bytes: 9 000 of them are what >= 8 windows of one piece take, also when -r drops a third)
    records = mc.random_records(9000, 7, True)
    path = str(tmp_path_factory.mktemp("mdstream") / "random.bam")
    info = write(path, records, block_size=10000)
    return path, records, info, inflate(path)


@pytest.mark.parametrize("remove", [False, True])
def test_windows_times_batches(random_file, remove, tmp_path, monkeypatch):
    path, records, info, stream = random_file
    dup = ref.duplicates(records, mc.TEXT)
    assert 0.05 * len(records) <= len(dup) <= 0.95 * len(records)
    batch = info["stream_len"] // 12
    st, md, w, want = both_paths(monkeypatch, tmp_path, path, P, batch, remove=remove, stream=stream)
    n_windows, n_batches = int(w["n_windows"]), int(md["n_batches"])
    assert n_windows >= 8 and n_batches >= 10
    assert n_windows == -(-len(want) // P)
    assert int(w["n_batch_runs"]) <= n_batches + n_windows - 1
    assert int(w["n_batch_runs"]) >= n_batches                              # every batch holds records that are written
    assert int(w["n_key_records"]) == sum(1 for r in records if (struct.unpack_from("<H", r, 18)[0] & 0x90D) == 1)
    assert st["n_duplicates"] == len(dup) and (st["n_records_out"] < st["n_records_in"]) == remove


# ---- 2. mates far apart ---------------------------------------------------------------------------------------------------------------
def _big(pos, length, name="f"):
    """An unmapped record of about `length` bytes placed at pos of c1: it takes no part, it only moves the others apart."""
    return bamgen.make_record(0, pos, "", "", 30, name=name, mapq=0, flag=0x4, tags=bamgen.tag_bytes("XX", bytes((pos + j) % 251 for j in range(length))))


def far_apart_records():
    scen, dups, _, counts = mc.scenarios()
    half = len(scen) // 2
    big = [_big(30000 + k, 15000, "big%d" % k) for k in range(16)]
    records = ([mc.rec("far", 0, 20000, flag=mc.F1, qual=30)] + big[:4] + scen[:half] + big[4:8] +
               [mc.rec("farB", 0, 20000, flag=mc.F1, qual=20), mc.rec("farB", 0, 20200, flag=mc.R2, qual=20)] + big[8:12] + scen[half:] + big[12:] +
               [mc.rec("far", 0, 20200, flag=mc.R2, qual=30)])
    return records, dups | {"farB#0", "farB#1"}, (counts[0] + 2, counts[1], counts[2])


@pytest.mark.parametrize("remove", [False, True])
def test_mates_far_apart(remove, tmp_path, monkeypatch):
    records, dups, counts = far_apart_records()
    path = str(tmp_path / "far.bam")
    info = write(path, records, block_size=5000)
    assert info["stream_len"] > 3 * P
    st, md, w, want = both_paths(monkeypatch, tmp_path, path, P, batch=20000, remove=remove)
    assert int(w["n_windows"]) >= (3 if remove else 4) and int(md["n_batches"]) >= 8         # the two ends of "far": first and last of both
    assert (st["n_end_pairs"], st["n_single_ends"], st["n_unmatched_pairs"], st["n_duplicates"]) == counts + (len(dups),) == (14, 23, 4, 20)
    assert (int(md["n_end_pairs"]), int(md["n_single_ends"]), int(md["n_unmatched_pairs"]), int(md["n_duplicates"])) == (14, 23, 4, 20)
    if not remove:
        assert marked_names(records, inflate(str(tmp_path / "w.win.bam"))) == dups | {"s15s#0", "s15x#0"}
    else:
        assert st["n_records_out"] == len(records) - len(dups) - 2


# ---- 3. the flag byte at window edges -------------------------------------------------------------------------------------------------
EDGE_REFS = [("c1", 1000000)]
EDGE_SQ = "@SQ\tSN:c1\tLN:1000000\n"


def _filler(pos, length, name="f"):
    """A record of exactly `length` bytes (>= 46 + len(name)) that takes no part: unmapped, no sequence, one B:C aux array."""
    base = len(bamgen.make_record(0, pos, "", "", 30, name=name, mapq=0, flag=0x4, tags=bamgen.tag_bytes("XX", b"")))
    assert length >= base, (length, base)
    r = bamgen.make_record(0, pos, "", "", 30, name=name, mapq=0, flag=0x4, tags=bamgen.tag_bytes("XX", bytes((pos + j) % 251 for j in range(length - base))))
    assert len(r) == length
    return r


def _padded_text(hlen_want, refs, sq_text, command_line):
    """A header text whose OUTPUT header (text re-serialised with the @PG line + reference list) is exactly hlen_want bytes."""
    def out_len(pad):
        text = "@HD\tVN:1.6\tSO:unsorted\n" + sq_text + "@CO\t" + "x" * pad + "\n"
        return text, len(bamgen.bam_header(ref.header_text(text, command_line), refs))
    _, h0 = out_len(0)
    assert hlen_want >= h0
    text, h = out_len(hlen_want - h0)
    assert h == hlen_want
    return text


def _frag(name, pos, qual, flag=0):
    return mc.rec(name, 0, pos, flag=flag, qual=qual)


def edge_layout(hlen):
    """Records and the offsets in the OUTPUT stream (no -r) at which the six records under test start.  `m*` get marked (a better
    fragment at their position comes first), `c*` come with 0x400 and lose it.  Offsets relative to a window edge k P:
    0 -- the record starts at the edge;  -19 -- its byte 18 is the last byte of a window and byte 19 the first of the next;
    -20 -- its byte 19 is the last byte of a window."""
    records, at, starts = [], hlen, {}
    for k in range(6):
        records.append(_frag("keep%d" % k, 1000 + 100 * k, 40))
    at += sum(len(r) for r in records)
    edge = 1
    for k, (name, delta) in enumerate((("m0", 0), ("m1", -19), ("m2", -20), ("c0", 0), ("c1", -19), ("c2", -20))):
        rec = _frag(name, 1000 + 100 * k, 20) if name[0] == "m" else _frag(name, 50000 + 100 * k, 30, flag=0x400)
        target = edge * P + delta
        while target - at < 60:
            edge += 1
            target = edge * P + delta
        records.append(_filler(90000 + k, target - at, "fill%d" % k))
        records.append(rec)
        starts[name] = target
        at = target + len(rec)
        edge += 1
    records.append(_filler(99000, 100, "tail"))
    return records, starts


def test_flag_byte_at_window_edges(tmp_path, monkeypatch):
    path = str(tmp_path / "edges.bam")
    win = str(tmp_path / "w.win.bam")
    cl = "markdup " + path + " " + win
    hlen = 700 + len(cl)
    text = _padded_text(hlen, EDGE_REFS, EDGE_SQ, cl)
    records, starts = edge_layout(hlen)
    write(path, records, text=text, refs=EDGE_REFS, block_size=20000)
    st, md, w, want = both_paths(monkeypatch, tmp_path, path, P, batch=30000)
    # the layout is the one intended
    _, _, _, out = ref.split_stream(want)
    off, p = {}, len(want) - sum(len(r) for r in out)
    assert p == hlen
    for r in out:
        off[r[36:36 + r[12] - 1].decode()] = (p, struct.unpack_from("<H", r, 18)[0])
        p += len(r)
    assert {n: off[n][0] for n in starts} == starts
    assert starts["m0"] % P == 0 and (starts["m1"] + 18) % P == P - 1 and (starts["m1"] + 19) % P == 0 and (starts["m2"] + 19) % P == P - 1
    assert starts["c0"] % P == 0 and (starts["c1"] + 18) % P == P - 1 and (starts["c1"] + 19) % P == 0 and (starts["c2"] + 19) % P == P - 1
    assert all(off["m%d" % k][1] == 0x400 and off["c%d" % k][1] == 0 for k in range(3))
    assert st["n_duplicates"] == 3 and int(w["n_windows"]) >= 6 and int(md["n_batches"]) >= 6


def _fill(records, length, tag):
    """Fillers of 1500 bytes and one last of what is left, `length` bytes in all: no record is longer than a batch of the test, so the
    read pass never has to lengthen its batches."""
    k = 0
    while length > 3000:
        records.append(_filler(90000 + k, 1500, "%s%d" % (tag, k)))
        length -= 1500
        k += 1
    records.append(_filler(90000 + k, length, "%s%d" % (tag, k)))


def removed_layout(hlen):
    """For -r.  Output offsets: a removed record `gone` sits at a window edge -- the kept record `next` behind it (0x400 preset, cleared)
    starts at the same destination, the edge -- and a long run of removed records makes whole batches without a byte in the output."""
    records = [_frag("best", 1000, 40), _frag("bestrun", 2000, 40)]
    at = hlen + sum(len(r) for r in records)
    _fill(records, P - at, "fill")
    records += [_frag("gone", 1000, 20), _frag("next", 60000, 30, flag=0x400)]
    run = [_frag("run%04d" % k, 2000, 20) for k in range(700)]
    records += run
    records.append(_frag("after", 61000, 30))
    _fill(records, 70000, "tail")
    return records, sum(len(r) for r in run)


def test_removed_records_at_an_edge_and_empty_batches(tmp_path, monkeypatch):
    path = str(tmp_path / "removed.bam")
    win = str(tmp_path / "w.win.bam")
    cl = "markdup -r " + path + " " + win
    hlen = 700 + len(cl)
    records, run_bytes = removed_layout(hlen)
    write(path, records, text=_padded_text(hlen, EDGE_REFS, EDGE_SQ, cl), refs=EDGE_REFS, block_size=2000)
    batch = 6000
    st, md, w, want = both_paths(monkeypatch, tmp_path, path, P, batch=batch, remove=True)
    out = ref.split_stream(want)[3]
    names = [r[36:36 + r[12] - 1].decode() for r in out]
    kept = [r[36:36 + r[12] - 1].decode() for r in records]
    assert names == [n for n in kept if n != "gone" and not n.startswith("run")] and st["n_duplicates"] == 701
    at = names.index("next")
    assert names[at - 1].startswith("fill") and names[at + 1] == "after"
    assert hlen + sum(len(r) for r in out[:at]) == P                         # `next` starts at the edge, where `gone` would have
    assert struct.unpack_from("<H", out[at], 18)[0] == 0
    # a batch holds at most `batch` bytes and one more block: so many batches lie inside the run of removed records and are never run
    assert int(md["n_batches"]) >= 20
    empty = run_bytes // (batch + 2000) - 1
    assert empty >= 4
    assert int(w["n_batch_runs"]) <= int(md["n_batches"]) - empty + int(w["n_windows"]) - 1, (md, w)
    # without -r the same file: every record is written, `gone` and the run carry 0x400
    st2, md2, w2, want2 = both_paths(monkeypatch, tmp_path, path, P, batch=batch, tag="k")
    assert marked_names(records, want2) == {"gone#0"} | {"run%04d#0" % k for k in range(700)}


# ---- 4. secondary / supplementary records with 0x400 ---------------------------------------------------------------------------------
@pytest.mark.parametrize("remove", [False, True])
def test_secondary_and_supplementary_keep_or_lose_their_bit(remove, tmp_path, monkeypatch):
    records = []
    for k in range(300):
        records += [mc.rec("sec%d" % k, 0, 1000 + k, flag=0x100 | 0x400), mc.rec("sup%d" % k, 0, 1000 + k, flag=0x800 | 0x400),
                    mc.rec("plain%d" % k, 0, 1000 + k, flag=0x100), mc.rec("prim%d" % k, 0, 40000 + k, flag=0x400)]
    path = str(tmp_path / "sec.bam")
    write(path, records, block_size=3000)
    st, md, w, want = both_paths(monkeypatch, tmp_path, path, P, batch=9000, remove=remove)
    out = ref.split_stream(want)[3]
    flags = [struct.unpack_from("<H", r, 18)[0] for r in out]
    assert st["n_duplicates"] == 0 and int(md["n_batches"]) >= 5
    if remove:
        assert flags == [0x100, 0] * 300                                     # dropped by the flag they came with
    else:
        assert flags == [0x500, 0xC00, 0x100, 0] * 300


# ---- 5. key store edges ---------------------------------------------------------------------------------------------------------------
def key_edge_records():
    F1, R2, rec = mc.F1, mc.R2, mc.rec
    long_name = "L" * 254
    rg_i = bamgen.tag_i("RG", 7)

    def typed(name, pos, flag):
        return bamgen.make_record(0, pos, "10M", "ACGTACGTAC", 30, name=name, flag=flag, tags=bamgen.tag_i("NM", 0) + rg_i)
    records = [
        rec("a", 0, 1000, flag=F1), rec("a", 0, 1200, flag=R2),                              # a name of one character
        rec(long_name, 0, 2000, flag=F1, rg="gA"), rec(long_name, 0, 2200, flag=R2, rg="gA"),    # ... and of 254
        rec("e", 0, 3000, flag=F1), rec("e", 0, 3200, flag=R2, rg=""),                       # RG absent against RG:Z: empty: a pair
        rec("d", 0, 4000, flag=F1, rg="gA"), rec("d", 0, 4200, flag=R2, rg="gB"),            # equal names, different RG: no pair
        rec("ab", 0, 5000, flag=F1, rg="c"), rec("a", 0, 5200, flag=R2, rg="bc"),            # the same bytes cut elsewhere: no pair
        typed("t", 6000, F1), typed("t", 6200, R2),                                          # an RG tag that is no string: as if absent
        rec("k3", 0, 7000, flag=F1), rec("k3", 0, 7200, flag=R2), rec("k3", 0, 7000, flag=F1),
        rec("k4", 0, 8000, flag=F1, qual=30), rec("k4", 0, 8200, flag=R2, qual=30), rec("k4", 0, 8000, flag=F1, qual=20), rec("k4", 0, 8200, flag=R2, qual=20),
    ]
    return records, (7, 5, 5), {"k4#2", "k4#3"}


@pytest.mark.parametrize("hash_bits", [None, 4])
def test_key_store_edges(hash_bits, tmp_path, monkeypatch):
    records, counts, dups = key_edge_records()
    # between them a few hundred plain pairs: with 4 hash bits the runs of unequal keys in the key store are long
    plain = []
    for k in range(300):
        plain += [mc.rec("p%03d" % k, 1, 100 + 50 * k, flag=mc.F1), mc.rec("p%03d" % k, 1, 300 + 50 * k, flag=mc.R2)]
    records = plain[:300] + records + plain[300:]
    path = str(tmp_path / "keys.bam")
    write(path, records, block_size=4000)
    extra = {"SBX_MARKDUP_HASH_BITS": str(hash_bits)} if hash_bits is not None else None
    st, md, w, want = both_paths(monkeypatch, tmp_path, path, P, batch=12000, extra=extra)
    assert (st["n_end_pairs"], st["n_single_ends"], st["n_unmatched_pairs"]) == (counts[0] + 300, counts[1], counts[2])
    assert marked_names(records, want) == dups
    assert int(w["n_key_records"]) == len(records)
    # an entry is 2 + l_read_name + the length of the RG value
    def entry(r):
        l_name = r[12]
        tags = r[36 + l_name + 4 + 5 + 10 + 7:]
        return 2 + l_name + (tags.index(b"\0", 3) - 3 if tags[:3] == b"RGZ" else 0)
    assert int(w["key_store_bytes"]) == sum(entry(r) for r in records)


# ---- 6. degenerate ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["header_only", "long_header", "one_record", "unmapped_only"])
def test_degenerate(kind, tmp_path, monkeypatch):
    refs, text = mc.REFS, mc.TEXT
    if kind == "header_only":
        records = []
    elif kind == "long_header":
        refs = [("s%04d" % i, 1000 + i) for i in range(4200)]
        text = "@HD\tVN:1.6\tSO:unsorted\n" + "".join("@SQ\tSN:%s\tLN:%d\n" % r for r in refs)
        records = [bamgen.make_record(r, pos, "8M", "ACGTACGT", 30, name="h%d" % i) for i, (r, pos) in enumerate(((4199, 5), (0, 900), (0, 900)))]
    elif kind == "one_record":
        records = [mc.rec("only", 0, 100, flag=0x400)]
    else:
        records = [bamgen.make_record(-1, -1, "", "ACGT", 30, name="u%d" % i, flag=0x4 | (0x400 if i % 3 == 0 else 0)) for i in range(700)]
    path = str(tmp_path / "d.bam")
    write(path, records, text=text, refs=refs)
    for remove in (False, True):
        st, md, w, want = both_paths(monkeypatch, tmp_path, path, P, remove=remove, tag="r" if remove else "w")
        hlen = len(want) - sum(len(r) for r in ref.split_stream(want)[3])
        assert st["n_records_in"] == len(records)
        if kind == "header_only":
            assert int(w["n_windows"]) == 1 and int(w["n_batch_runs"]) == 0 and st["n_records_out"] == 0
        elif kind == "long_header":
            assert hlen > 2 * P and int(w["n_windows"]) == 3 and st["n_duplicates"] == 1 and st["n_records_out"] == (2 if remove else 3)
        elif kind == "one_record":
            assert st["n_records_out"] == 1 and st["n_duplicates"] == 0 and struct.unpack_from("<H", ref.split_stream(want)[3][0], 18)[0] == 0
        else:
            assert int(w["key_store_bytes"]) == 0 == int(w["n_key_records"]) and st["n_end_pairs"] == 0 == st["n_duplicates"]
            assert st["n_records_out"] == 700


# ---- 7. levels --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("level", [0, 1, 6])
def test_levels(random_file, level, tmp_path, monkeypatch):
    path, records, info, stream = random_file
    both_paths(monkeypatch, tmp_path, path, 3 * P, info["stream_len"] // 5, level=level, stream=stream)


# ---- 8. API and ABI ---------------------------------------------------------------------------------------------------------------------
def test_api_and_abi(random_file, tmp_path, monkeypatch):
    import sambamba_amd
    from sambamba_amd import _lib
    L = sambamba_amd.lib()
    assert L.sbx_abi_sizeof(b"sbx_markdup_stream_stats") == C.sizeof(_lib.MarkdupStreamStats) == 80
    assert "sbx_markdup_run" in _lib.EXPORTS and hasattr(L, "sbx_markdup_run")
    path, records, info, stream = random_file
    want = ref.expected_stream(stream)
    res, win = str(tmp_path / "res.bam"), str(tmp_path / "win.bam")
    st0 = api_markdup(monkeypatch, path, res)
    assert st0["n_windows"] == 0 == st0["n_batch_runs"] == st0["window_bytes"] == st0["key_store_bytes"]
    st = api_markdup(monkeypatch, path, win, window=2 * P, batch=info["stream_len"] // 6)
    assert st["n_windows"] == -(-len(want) // (2 * P)) > 0 and st["window_bytes"] == 2 * P
    assert st["n_batches"] >= 5 and st["n_batches"] <= st["n_batch_runs"] <= st["n_batches"] + st["n_windows"] - 1 and st["key_store_bytes"] > 0
    assert st["compressed_bytes"] == os.path.getsize(win) and st0["compressed_bytes"] == os.path.getsize(res)
    check_file(win, want)
    assert open(win, "rb").read() == open(res, "rb").read()
    for k in ("n_records_in", "n_records_out", "n_end_pairs", "n_single_ends", "n_unmatched_pairs", "n_duplicates", "stream_bytes"):
        assert st[k] == st0[k], k
    # the struct: NULL is sbx_markdup; a struct_size below the struct's is refused before anything is read
    ss = _lib.MarkdupStreamStats()
    ss.struct_size = 16
    err = C.create_string_buffer(512)
    assert L.sbx_markdup_run(path.encode(), str(tmp_path / "no.bam").encode(), 0, -1, None, -1, None, C.byref(ss), err, 512) == -1
    assert b"struct_size" in err.value and not os.path.exists(str(tmp_path / "no.bam"))
    # the CLI without the hook: the resident path, no stream line
    md, w = cli_markdup([path, str(tmp_path / "c.bam")])
    assert w is None and int(md["n_records_in"]) == len(records)
