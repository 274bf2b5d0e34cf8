"""The streamed path of sbx_import_sam (sbx_import_sam_run): records that do not stay in a store.  K15d (samparse.hip) writes the
records of a text chunk into ONE staging window of the output stream (engine_streamout.hpp), clipped at the window's edges; the
records a store held before the switch are drained through the same window.

Every case is written once on the resident path (no hook) and once or more through the hooks -- SBX_STREAM_WINDOW_BYTES=1 with
SBX_BGZF_PIECE_BLOCKS=1: a window of one 65280-byte piece, the smallest there is, from the first chunk on; SBX_IMPORT_STORE_BYTES=n:
the switch at the chunk whose records would bring the store past n bytes -- and the files must be identical.  The resident file is
the reference: tests/test_gpu_import.py ties it to tests/samin_ref.py.  On a library without the feature the hooks are ignored and
no stream stats exist."""
import ctypes as C
import filecmp
import os
import random
import subprocess

import pytest

from tests import samin_cases as cases
from tests import samin_ref as ref

pytestmark = pytest.mark.gpu

PIECE = 0xFF00
STREAM_KEYS = ("n_windows", "window_bytes", "n_pack_launches", "ms_pack")
SAME_KEYS = ("n_lines", "n_records", "text_bytes", "stream_bytes", "compressed_bytes", "n_chunks")
HOOKS = ("SBX_STREAM_WINDOW_BYTES", "SBX_IMPORT_STORE_BYTES", "SBX_IMPORT_CHUNK_BYTES")
SWITCH_CHUNK = 12 << 10     # four such chunks fit one piece: the window the switch chooses by itself is one piece


def windows_of(stream_bytes):
    return -(-stream_bytes // PIECE)


def write_sam(data, tmp_path, tag):
    sam = str(tmp_path / (tag + ".sam"))
    with open(sam, "wb") as f:
        f.write(data)
    return sam


def run_import(monkeypatch, sam, bam, chunk=None, window=None, store=None, **kw):
    """import_sam with one piece per BGZF block and these hooks (None: unset)"""
    import sambamba_amd
    monkeypatch.setenv("SBX_BGZF_PIECE_BLOCKS", "1")
    for name, value in zip(HOOKS, (window, store, chunk)):
        if value is None:
            monkeypatch.delenv(name, raising=False)
        else:
            monkeypatch.setenv(name, str(value))
    try:
        return sambamba_amd.import_sam(sam, bam, **kw)
    finally:
        for name in HOOKS:
            monkeypatch.delenv(name, raising=False)


def streamed_equals_resident(monkeypatch, data, tmp_path, tag, chunk=None, window=1, store=None, **kw):
    """(resident stats, streamed stats, resident file); the two files are identical and the stats that both paths have agree"""
    sam = write_sam(data, tmp_path, tag)
    a, b = str(tmp_path / (tag + ".resident.bam")), str(tmp_path / (tag + ".streamed.bam"))
    st_r = run_import(monkeypatch, sam, a, chunk=chunk, **kw)
    st_s = run_import(monkeypatch, sam, b, chunk=chunk, window=window, store=store, **kw)
    print("%s: stream_bytes %d n_chunks %d n_windows %d n_pack_launches %d ms_emit %.3f / %.3f" % (
        tag, st_s["stream_bytes"], st_s["n_chunks"], st_s["n_windows"], st_s["n_pack_launches"], st_r["ms_emit"], st_s["ms_emit"]))
    assert filecmp.cmp(a, b, shallow=False), tag
    assert tuple(st_r[k] for k in STREAM_KEYS) == (0, 0, 0, 0.0)
    for k in SAME_KEYS:
        assert st_r[k] == st_s[k], (tag, k)
    assert st_s["compressed_bytes"] == os.path.getsize(b)
    return st_r, st_s, a


def mixed_line(rng, k):
    """a mapped line with 1 .. 400 bases and some tags"""
    n = rng.choice((1, 2, 7, 36, 100, 151, 250, 400))
    seq = bytes(rng.choice(b"ACGTN") for _ in range(n))
    qual = bytes(rng.randrange(33, 127) for _ in range(n))
    tags = [b"NM:i:%d" % rng.randrange(-70000, 70000), b"RG:Z:grp%d" % (k % 3), b"XF:f:%d.5" % k, b"XB:B:S,%d,%d" % (k % 65536, n)][:rng.randrange(0, 5)]
    return cases.line(b"m%05d" % k, b"%d" % rng.choice((0, 16, 99, 147)), rng.choice((b"c1", b"c2")), b"%d" % rng.randrange(1, 30000), b"%d" % rng.randrange(0, 61),
                      b"%dM" % n, b"=", b"%d" % rng.randrange(1, 30000), b"%d" % rng.randrange(-500, 500), seq, qual, tags)


# ---- byte identity across chunk sizes -----------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def big_text():
    """the good edge lines, generated lines of mixed lengths, and one record of 100,000 bases -- larger than two windows, so it is
    clipped on both sides -- in the middle"""
    rng = random.Random(20251021)
    lines = list(cases.good_lines().values()) + [mixed_line(rng, k) for k in range(250)]
    n = 100000
    long_line = cases.line(b"long100k", cigar=b"%dM" % n, seq=bytes(b"ACGTNacgtn=."[k % 12] for k in range(n)), qual=bytes(33 + (7 * k) % 94 for k in range(n)),
                           tags=[b"NM:i:0", b"XZ:Z:behind the bases"])
    assert len(ref.record(long_line, cases.REF_NAMES)) > 2 * PIECE
    lines.insert(len(lines) - 100, long_line)
    rng.shuffle(lines)
    data = cases.sam_text(lines)
    assert 400 << 10 <= len(data) <= 800 << 10
    return data, lines


@pytest.mark.parametrize("chunk", [16 << 10, 160 << 10, 1 << 30], ids=["chunk_below_a_window", "chunk_above_two_windows", "one_chunk"])
def test_chunk_sizes_give_the_resident_file(big_text, chunk, tmp_path, monkeypatch):
    data, lines = big_text
    assert chunk < PIECE // 2 or chunk > 2 * PIECE
    st_r, st_s, _ = streamed_equals_resident(monkeypatch, data, tmp_path, "c%d" % chunk, chunk=chunk)
    assert st_s["n_records"] == st_s["n_lines"] == len(lines)
    assert (st_s["n_chunks"] == 1) == (chunk == 1 << 30) and (chunk == 1 << 30 or st_s["n_chunks"] > 3)
    assert st_s["n_windows"] == windows_of(st_s["stream_bytes"]) > 6 and st_s["window_bytes"] == PIECE
    # one launch of K15d per window a chunk touches: at least one per window and one per chunk
    assert st_s["n_pack_launches"] >= max(st_s["n_windows"] - 1, st_s["n_chunks"])


# ---- the first window edge inside every part of a record ----------------------------------------------------------------------------
VICTIM_TAGS = [(b"XA:A:Q", "A"), (b"Xc:i:-100", "c"), (b"XC:i:200", "C"), (b"Xs:i:-30000", "s"), (b"XS:i:60000", "S"), (b"Xi:i:-70000", "i"),
               (b"XI:i:3000000000", "I"), (b"Xf:f:-2.75", "f"), (b"XZ:Z:some text here", "Z"), (b"XH:H:1AE301FF", "H"), (b"XB:B:s,1,-2,3,-4,5", "B")]


def victim_line(l_seq):
    seq = bytes(b"ACGTNRYKM"[k % 9] for k in range(l_seq))
    return cases.line(b"victim_of_the_edge", b"99", b"c2", b"17000", b"60", b"10M2I%dM5S" % (l_seq - 17), b"=", b"17100", b"-150", seq,
                      bytes(33 + (11 * k) % 94 for k in range(l_seq)), [t for t, _ in VICTIM_TAGS])


def victim_parts(l_seq):
    """{part: (first byte, end)} of the victim's record, from the record layout"""
    line = victim_line(l_seq)
    f = line.split(b"\t")
    name_at, cigar_at = 36, 36 + len(f[0]) + 1
    seq_at = cigar_at + 4 * 4
    qual_at = seq_at + (l_seq + 1) // 2
    parts = {"block_size": (0, 4), "fixed": (4, 36), "name": (name_at, cigar_at), "cigar": (cigar_at, seq_at),
             "seq_odd" if l_seq % 2 else "seq_even": (seq_at, qual_at), "qual": (qual_at, qual_at + l_seq)}
    at = qual_at + l_seq
    for k, (_, ty) in enumerate(VICTIM_TAGS):
        end = len(ref.record(b"\t".join(f[:12 + k]), cases.REF_NAMES))
        parts["tag_" + ty] = (at + (8 if ty == "B" else 3), end)       # the value: behind key and type (B: and element type and count)
        at = end
    assert at == len(ref.record(line, cases.REF_NAMES))
    return parts


def pad_line(need):
    """a leading record of exactly `need` bytes: the name's and the SEQ's lengths are chosen from the layout 36 + name + 1 +
    ceil(l / 2) + l (CIGAR '*', QUAL '*': 0xFF for every base)"""
    for l_name in range(8, 12):
        body = need - 36 - l_name - 1
        for l_seq in range(max(2, body * 2 // 3 - 2), body * 2 // 3 + 3):
            if (l_seq + 1) // 2 + l_seq == body:
                line = cases.line(b"p" * l_name, b"4", b"*", b"0", b"0", b"*", b"*", b"0", b"0", bytes(b"ACGT"[k % 4] for k in range(l_seq)), b"*")
                assert len(ref.record(line, cases.REF_NAMES)) == need
                return line, l_seq
    raise AssertionError(need)


def test_first_window_edge_inside_every_field(tmp_path, monkeypatch):
    import sambamba_amd
    hlen = len(ref.bam_stream(sambamba_amd.markdup_header_text(cases.TEXT, None), cases.REFS, []))
    tail = [cases.line(b"after%d" % k) for k in range(3)]
    hit, pad_lengths = set(), set()
    for l_seq in (150, 151):
        parts = victim_parts(l_seq)
        victim = victim_line(l_seq)
        if l_seq == 151:                                  # the second victim for what an odd number of bases changes
            parts = {k: parts[k] for k in ("cigar", "seq_odd", "qual")}
        for part, (a, b) in parts.items():
            # the edge in the middle of the part; a part of one byte as the last byte of window 0 and as the first of window 1
            for e in ([a, b] if b - a == 1 else [a + (b - a) // 2]):
                pad, pad_l_seq = pad_line(PIECE - hlen - e)
                data = cases.sam_text([pad, victim] + tail)
                st_r, st_s, _ = streamed_equals_resident(monkeypatch, data, tmp_path, "%s_%d_%d" % (part, l_seq, e))
                assert st_s["n_windows"] == windows_of(st_s["stream_bytes"]) == 2 and st_s["n_records"] == 5
                # where the first window ends inside the victim, from the offsets computed here
                edge = PIECE - hlen - len(ref.record(pad, cases.REF_NAMES))
                assert edge == e and (a < edge < b or (b - a == 1 and edge in (a, b)))
                hit.add(part)
                pad_lengths.add(pad_l_seq)
    want = {"block_size", "fixed", "name", "cigar", "seq_odd", "seq_even", "qual"} | {"tag_" + ty for ty in "AcCsSiIfZHB"}
    assert hit == want
    assert 20 <= len(pad_lengths) <= 60                   # a few dozen lengths of the pad's SEQ


# ---- the switch ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def switch_text():
    rng = random.Random(7)
    lines = [mixed_line(rng, k) for k in range(900)]
    record_bytes = sum(len(ref.record(l, cases.REF_NAMES)) for l in lines)
    first_chunk = 0
    used = 0
    for l in lines:                                         # the records of the first chunk of text
        if used + len(l) + 1 > SWITCH_CHUNK:
            break
        used += len(l) + 1
        first_chunk += len(ref.record(l, cases.REF_NAMES))
    return cases.sam_text(lines), lines, record_bytes, first_chunk


@pytest.mark.parametrize("where", ["after_several_chunks", "at_the_first_chunk"])
def test_switch_from_the_store(switch_text, where, tmp_path, monkeypatch):
    data, lines, record_bytes, first_chunk = switch_text
    limit = record_bytes // 2 if where == "after_several_chunks" else first_chunk - 1
    assert record_bytes // 2 > 4 * first_chunk > 4 * 1000 and record_bytes > 3 * PIECE
    st_r, st_s, _ = streamed_equals_resident(monkeypatch, data, tmp_path, where, chunk=SWITCH_CHUNK, window=None, store=limit)
    assert st_s["n_chunks"] > 8 and st_s["n_records"] == len(lines)
    assert st_s["window_bytes"] == PIECE and st_s["n_windows"] == windows_of(st_s["stream_bytes"]) > 3
    # K15d ran for the chunks behind the switch only
    assert 0 < st_s["n_pack_launches"] and (where == "at_the_first_chunk") == (st_s["n_pack_launches"] >= st_s["n_chunks"])


@pytest.mark.parametrize("slack", [0, 1 << 20])
def test_no_switch_when_the_store_may_hold_every_record(switch_text, slack, tmp_path, monkeypatch):
    data, lines, record_bytes, _ = switch_text
    sam = write_sam(data, tmp_path, "fits")
    a, b = str(tmp_path / "a.bam"), str(tmp_path / "b.bam")
    st_r = run_import(monkeypatch, sam, a, chunk=SWITCH_CHUNK)
    st_s = run_import(monkeypatch, sam, b, chunk=SWITCH_CHUNK, store=record_bytes + slack)
    assert filecmp.cmp(a, b, shallow=False)
    assert st_s["n_windows"] == 0 and tuple(st_s[k] for k in STREAM_KEYS) == (0, 0, 0, 0.0)
    for k in SAME_KEYS:
        assert st_r[k] == st_s[k], k


# ---- a malformed line behind windows that were written ------------------------------------------------------------------------------
def test_malformed_lines_in_late_chunks(tmp_path, monkeypatch):
    import sambamba_amd
    rng = random.Random(11)
    good = [mixed_line(rng, k) for k in range(900)]
    bad = cases.malformed_lines()
    lines = good[:700] + [bad["qual_short"]] + good[700:] + [bad["tag_i_2_32"]]
    text_before = sum(len(l) + 1 for l in lines[:700])
    assert text_before > 8 * (16 << 10) and sum(len(l) + 1 for l in lines[701:]) > 16 << 10       # chunks apart, windows written before
    assert sum(len(ref.record(l, cases.REF_NAMES)) for l in good[:700]) > 2 * PIECE
    sam = write_sam(cases.sam_text(lines, final_newline=False), tmp_path, "bad")
    messages = []
    for tag, hooks in (("resident", {}), ("window", {"window": 1}), ("store", {"store": 20000})):
        out = str(tmp_path / (tag + ".bam"))
        with pytest.raises(sambamba_amd.SbxError) as ei:
            run_import(monkeypatch, sam, out, chunk=16 << 10, **hooks)
        assert ei.value.code == -3 and not os.path.exists(out), tag
        messages.append(str(ei.value))
    n_header = cases.TEXT.count("\n")
    assert ": 2 lines are outside the grammar" in messages[0] and messages[0].endswith("the first is line %d" % (n_header + 701))
    assert messages[1] == messages[0] and messages[2] == messages[0]


# ---- levels, index, inputs without records ------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def sorted_text():
    rng = random.Random(3)
    lines = []
    for r, (name, length) in enumerate(cases.REFS):
        for p in sorted(rng.randrange(1, length - 200) for _ in range(500)):
            lines.append(cases.line(b"s%d_%d" % (r, p), b"0", name.encode(), b"%d" % p, b"40", b"50M", b"*", b"0", b"0", b"ACGTA" * 10, b"F" * 50, [b"NM:i:%d" % (p % 7)]))
    return cases.TEXT.replace("SO:unsorted", "SO:coordinate").encode() + b"".join(l + b"\n" for l in lines)


@pytest.mark.parametrize("level", [0, 1, 6])
def test_levels(sorted_text, level, tmp_path, monkeypatch):
    st_r, st_s, _ = streamed_equals_resident(monkeypatch, sorted_text, tmp_path, "l%d" % level, chunk=16 << 10, level=level)
    assert st_s["n_windows"] == windows_of(st_s["stream_bytes"]) > 1


def test_index(sorted_text, tmp_path, monkeypatch):
    st_r, st_s, a = streamed_equals_resident(monkeypatch, sorted_text, tmp_path, "ix", chunk=16 << 10, index=True, command_line="view -S x")
    b = a.replace(".resident.", ".streamed.")
    assert st_s["n_windows"] > 1 and os.path.getsize(a + ".bai") > 100
    assert filecmp.cmp(a + ".bai", b + ".bai", shallow=False)


@pytest.mark.parametrize("which", ["header_only", "no_sq"])
def test_inputs_without_records_or_references(which, tmp_path, monkeypatch):
    unmapped = [cases.line(b"u%d" % k, b"4", b"*", b"0", b"0", b"*", b"*", b"0", b"0", b"ACGT", b"IIII") for k in range(3)]
    data = cases.TEXT.encode() if which == "header_only" else b"@HD\tVN:1.6\tSO:unsorted\n" + b"".join(l + b"\n" for l in unmapped)
    for hooks in ({"window": 1}, {"window": None, "store": 1}):
        st_r, st_s, _ = streamed_equals_resident(monkeypatch, data, tmp_path, which + "_" + "_".join(hooks), **hooks)
        assert st_s["n_records"] == (0 if which == "header_only" else 3)
        # (without a record there is no chunk, and nothing to switch for)
        assert st_s["n_windows"] == (0 if which == "header_only" else 1)


# ---- the command line on a pipe -----------------------------------------------------------------------------------------------------
def test_cli_on_a_pipe(big_text, tmp_path):
    import sambamba_amd
    data, _ = big_text
    imp = sambamba_amd.import_cli_path()
    base = {k: v for k, v in os.environ.items() if k not in HOOKS}
    base["SBX_BGZF_PIECE_BLOCKS"] = "1"
    base["SBX_IMPORT_CHUNK_BYTES"] = str(16 << 10)
    files = []
    for tag, hooks in (("resident", {}), ("window", {"SBX_STREAM_WINDOW_BYTES": "1"}), ("store", {"SBX_IMPORT_STORE_BYTES": "100000"})):
        d = tmp_path / tag
        d.mkdir()
        # (a fresh child process; the same relative output name everywhere, so that the @PG line is the same)
        r = subprocess.run([imp, "-o", "out.bam", "-"], input=data, cwd=str(d), env=dict(base, SBX_TIMING="1", **hooks), stdout=subprocess.PIPE,
                           stderr=subprocess.PIPE, timeout=120)
        assert r.returncode == 0, r.stderr.decode()[-2000:]
        assert ("[sbx] stream:" in r.stderr.decode()) == (tag != "resident") and "[sbx] import:" in r.stderr.decode()
        files.append(str(d / "out.bam"))
    assert filecmp.cmp(files[0], files[1], shallow=False) and filecmp.cmp(files[0], files[2], shallow=False)


# ---- the interface ------------------------------------------------------------------------------------------------------------------
def test_stats_and_entry_point(tmp_path, monkeypatch):
    import sambamba_amd
    from sambamba_amd._lib import EXPORTS, ImportStats
    data = cases.sam_text([cases.line(b"r%d" % k) for k in range(5)])
    sam, bam = write_sam(data, tmp_path, "s"), str(tmp_path / "s.bam")
    st = run_import(monkeypatch, sam, bam)
    assert set(STREAM_KEYS) <= set(st) and tuple(st[k] for k in STREAM_KEYS) == (0, 0, 0, 0.0)
    st = run_import(monkeypatch, sam, bam, window=1)
    assert st["n_windows"] == 1 and st["window_bytes"] == PIECE and st["n_pack_launches"] == 1 and st["n_records"] == 5
    # the C entry point with no sbx_stream_stats to fill
    assert "sbx_import_sam_run" in EXPORTS
    L = sambamba_amd.lib()
    raw, err, other = ImportStats(), C.create_string_buffer(512), str(tmp_path / "null.bam")
    monkeypatch.setenv("SBX_STREAM_WINDOW_BYTES", "1")
    rc = L.sbx_import_sam_run(sam.encode(), other.encode(), None, -1, 0, -1, C.byref(raw), None, err, 512)
    monkeypatch.delenv("SBX_STREAM_WINDOW_BYTES")
    assert rc == 0, err.value
    assert raw.n_records == 5 and filecmp.cmp(bam, other, shallow=False)
