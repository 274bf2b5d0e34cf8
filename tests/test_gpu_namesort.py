"""`sambamba sort -n / -N / -M` on the device -- sbx_sort_bam_by_name: K14a name keys, K14b word gather (namesort.hip) around the
radix sort K9b -- through the Python API and the `sbx-nsort` CLI, against the pure-Python restatement of the reference's comparators
(tests/namesort_ref.py).  Every comparison is byte for byte on the INFLATED output; the file itself must end with the EOF block and
hold no block of more than 0xFF00 payload bytes."""
import os
import random
import struct
import subprocess

import pytest

from tests import bamgen
from tests import namesort_ref as ref
from tests import sort_ref
from tests.flagstat_ref import inflate
from tests.test_gpu_sort import FIXTURES, REFS, UNSORTED, check_file, shuffled_copy
from tests.util import GOLDEN

pytestmark = pytest.mark.gpu

ORDER_NAME = {ref.LEX: "queryname", ref.NATURAL: "natural"}
ORDER_FLAG = {ref.LEX: "-n", ref.NATURAL: "-N"}


def cli(args, env=None):
    from sambamba_amd import nsort_cli_path
    return subprocess.run([nsort_cli_path()] + list(args), stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                          env=dict(os.environ, **env) if env else None)


def check(path, tmp_path, order, match_mates=False, want=None, flt=None, keep=None, tag="o", env=None):
    """API and CLI against the restatement; returns the API's stats and the CLI's stderr."""
    import sambamba_amd
    want = want if want is not None else ref.expected(path, order, match_mates, keep)
    out_api = str(tmp_path / (tag + ".api.bam"))
    st = sambamba_amd.sort_bam(path, out_api, filter=flt, order=ORDER_NAME[order], match_mates=match_mates)
    check_file(out_api, want)
    assert not os.path.exists(out_api + ".bai")
    out_cli = str(tmp_path / (tag + ".cli.bam"))
    args = [ORDER_FLAG[order]] + (["-M"] if match_mates else []) + ["-o", out_cli, path] + (["-F", flt] if flt else [])
    r = cli(args, env=env)
    assert r.returncode == 0, r.stderr
    check_file(out_cli, want)
    assert not os.path.exists(out_cli + ".bai")          # a name order has no index
    assert st["n_records_out"] == len(sort_ref.split_stream(want)[3]) and st["sorted_stream_bytes"] == len(want)
    assert st["compressed_bytes"] == os.path.getsize(out_api)
    return st, r.stderr.decode()


# ---- the reference's own fixture ----
@pytest.mark.parametrize("order", [ref.LEX, ref.NATURAL])
@pytest.mark.parametrize("match_mates", [False, True])
def test_match_mates_golden(order, match_mates, tmp_path):
    path = os.path.join(GOLDEN, "match_mates.bam")
    want = ref.expected(path, order, match_mates)
    text, _, _, recs = sort_ref.split_stream(want)
    assert text.startswith(b"@HD\tVN:1.3\tSO:queryname\n") and len(recs) == 22
    if match_mates:
        keys = [(ref.name_of(r), ref.hi_of(r), ref.flag_of(r)) for r in recs]
        assert keys == sorted(keys)
    st, _ = check(path, tmp_path, order, match_mates, want=want)
    assert st["n_records_in"] == st["n_records_out"] == 22


@pytest.mark.parametrize("name", [f for f in FIXTURES if f != "match_mates"])
def test_other_fixtures_by_name(name, tmp_path):
    shuf = shuffled_copy(os.path.join(GOLDEN, name + ".bam"), str(tmp_path / "shuffled.bam"), seed=len(name) + 1)
    check(shuf, tmp_path, ref.LEX)
    # the reference suite's own check: `LC_ALL=C sort -c` on the name column
    names = [ref.name_of(r) for r in sort_ref.split_stream(inflate(str(tmp_path / "o.api.bam")))[3]]
    assert len(names) > 1 and all(a <= b for a, b in zip(names, names[1:]))


# ---- generated names ----
PREFIX = "HWI-ST1234:77:C2A6RACX"[:20]


def _names(rng, n):
    """Names of every length that matters to the 8-byte words of the key, with exact duplicates, prefixes of other names, a shared
    20-byte prefix and digit runs with leading zeros."""
    assert len(PREFIX) == 20
    out = []
    short = [0, 1, 7, 8, 9, 15, 16, 17]
    for i in range(n):
        k = rng.random()
        if k < 0.10:
            ln = rng.choice(short)
            out.append("".join(rng.choice("ab0") for _ in range(ln)))
        elif k < 0.12:
            out.append((PREFIX + ":" + "".join(rng.choice("0123456789x:") for _ in range(254)))[:254])
        elif k < 0.45 and out:
            out.append(rng.choice(out))                                     # an exact duplicate: file order must show
        elif k < 0.55 and out:
            base = rng.choice(out)
            out.append(base[:rng.randrange(len(base) + 1)])                # a prefix of another name
        else:
            lane, tile = rng.randrange(1, 4), rng.choice((1101, 2201))
            x = rng.randrange(0, 300)
            fmt = rng.choice(("%d", "%03d", "%05d", "%d"))
            out.append("%s:%d:%d:%s:%s" % (PREFIX, lane, tile, fmt % x, rng.choice(("7", "07", "007", "70", "9", "10"))))
    return out


def _records(names, rng):
    recs = []
    for i, nm in enumerate(names):
        flag = (0x10 if rng.random() < 0.5 else 0) | rng.choice((0, 0x40, 0x80))
        seq = "ACGTACGTAC"[:rng.randrange(4, 11)]
        # the position carries the file index: records with equal names differ, so a wrong tie order shows in the bytes
        recs.append(bamgen.make_record(rng.choice((0, 1)), i, "%dM" % len(seq), seq, 30, name=nm, flag=flag,
                                       tags=bamgen.tag_z("RG", "g1") if i % 3 else b""))
    return recs


def _reverse(rec):
    return bool(ref.flag_of(rec) & 0x10)


@pytest.fixture(scope="module")
def generated(tmp_path_factory):
    d = tmp_path_factory.mktemp("namesort")
    rng = random.Random(20240917)
    names = _names(rng, 6000)
    assert {len(n) for n in names} >= {0, 1, 7, 8, 9, 15, 16, 17, 254} and len(set(names)) < 4500
    recs = _records(names, rng)
    path = str(d / "names.bam")
    info = bamgen.write_bam(path, REFS, recs, text=UNSORTED, write_index=False)
    stream = inflate(path)
    want = {(o, f): ref.expected_stream(stream, o, False, _reverse if f else None) for o in (ref.LEX, ref.NATURAL) for f in (False, True)}
    return path, info, want


@pytest.mark.parametrize("order", [ref.LEX, ref.NATURAL])
def test_generated_names(generated, order, tmp_path):
    path, _, want = generated
    out = sort_ref.split_stream(want[order, False])[3]
    # the restatement's own stability: records with one name appear in file order (the position is the file index)
    by_name = {}
    for r in out:
        by_name.setdefault(ref.name_of(r), []).append(struct.unpack_from("<i", r, 8)[0])
    assert max(len(v) for v in by_name.values()) > 3 and all(v == sorted(v) for v in by_name.values())
    if order == ref.NATURAL:
        assert want[ref.LEX, False] != want[ref.NATURAL, False]
    st, err = check(path, tmp_path, order, want=want[order, False], env={"SBX_TIMING": "1"})
    assert st["n_records_out"] == 6000 and st["n_sort_passes"] >= 3 and st["n_batches"] == 1
    line = [x for x in err.splitlines() if x.startswith("[sbx] sort:")]
    assert len(line) == 1 and (" order=%s " % ORDER_NAME[order]) in line[0] and " words_sorted=" in line[0]


@pytest.mark.parametrize("order", [ref.LEX, ref.NATURAL])
def test_several_batches_and_a_filter(generated, order, tmp_path, monkeypatch):
    import sambamba_amd
    path, info, want = generated
    # the filter drops about half: the keys are built after the compaction
    n_out = len(sort_ref.split_stream(want[order, True])[3])
    assert 2000 < n_out < 4000
    st, _ = check(path, tmp_path, order, want=want[order, True], flt="reverse_strand", tag="one")
    assert st["n_batches"] == 1 and st["n_records_out"] == n_out
    batch = str(min(info["stream_len"] // 8, 60000))
    monkeypatch.setenv("SBX_INDEX_BATCH_BYTES", batch)
    for flt in (None, "reverse_strand"):
        st, _ = check(path, tmp_path, order, want=want[order, flt is not None], flt=flt, tag="many", env={"SBX_INDEX_BATCH_BYTES": batch})
        assert st["n_batches"] >= 6


def test_shared_prefix_costs_nothing(tmp_path):
    # every name is the 20-byte prefix + six digits: words 0 and 1 of the key hold no varying bit, word 2 only in its low four
    # bytes, word 3 in its two high ones -- at most six radix passes, where a sort of all 26 bytes would take 26
    rng = random.Random(5)
    names = [PREFIX + "%06d" % rng.randrange(10 ** 6) for _ in range(4200)]
    path = str(tmp_path / "prefixed.bam")
    bamgen.write_bam(path, REFS, _records(names, rng), text=UNSORTED, write_index=False)
    st, _ = check(path, tmp_path, ref.LEX)
    assert 1 <= st["n_sort_passes"] <= 6 and st["key_bits"] <= 48


# ---- -M ----
def test_match_mates_orders_hi_then_flag(tmp_path):
    rng = random.Random(9)
    t = bamgen.tag_num
    his = [t("HI", "c", -1), t("HI", "c", -128), t("HI", "C", 1), t("HI", "C", 255), t("HI", "s", -300), t("HI", "S", 65535),
           t("HI", "i", -2 ** 31), t("HI", "i", 70000), t("HI", "I", 2 ** 31 - 1), t("HI", "I", 2), b"", bamgen.tag_z("RG", "g1"),
           t("NH", "C", 4) + t("HI", "C", 0)]
    recs = []
    for nm in ("frag", "frag1", "a", ""):
        for aux in his:
            for flag in (0x41, 0x81, 0x1, 0xC1):
                recs.append(bamgen.make_record(0, len(recs), "4M", "ACGT", 30, name=nm, flag=flag, tags=aux))
    rng.shuffle(recs)
    recs = recs * 2                                                     # every (name, HI, flag) twice: ties in file order
    recs = [r[:8] + struct.pack("<i", i) + r[12:] for i, r in enumerate(recs)]
    path = str(tmp_path / "mates.bam")
    bamgen.write_bam(path, REFS, recs, text=UNSORTED, write_index=False)
    for order in (ref.LEX, ref.NATURAL):
        want = ref.expected(path, order, True)
        out = sort_ref.split_stream(want)[3]
        keys = [(ref.name_of(r), ref.hi_of(r), ref.flag_of(r), struct.unpack_from("<i", r, 8)[0]) for r in out]
        assert keys == sorted(keys)
        # an absent HI counts as 0: between -1 and 1
        frag = [k[1] for k in keys if k[0] == b"frag"]
        assert frag.index(-1) < frag.index(0) < frag.index(1)
        check(path, tmp_path, order, True, want=want, tag="m%d" % order)
    # without -M the same file keeps file order among equal names
    check(path, tmp_path, ref.LEX, False, tag="nm")


# ---- refusals ----
def _assert_refused(path, tmp_path, order, match_mates, needle):
    import sambamba_amd
    out = str(tmp_path / "refused.bam")
    with pytest.raises(sambamba_amd.SbxError) as ei:
        sambamba_amd.sort_bam(path, out, order=ORDER_NAME[order], match_mates=match_mates)
    assert ei.value.code == -3 and needle in str(ei.value), ei.value            # SBX_EFORMAT, with the count
    assert not os.path.exists(out)
    r = cli([ORDER_FLAG[order]] + (["-M"] if match_mates else []) + ["-o", out, path])
    assert r.returncode == 1 and r.stdout == b"" and r.stderr.startswith(b"sbx-nsort: ") and needle.encode() in r.stderr
    assert not os.path.exists(out) and not os.path.exists(out + ".bai")


def test_refusals(tmp_path):
    good = [bamgen.make_record(0, i, "4M", "ACGT", 30, name="r%d" % (i % 7)) for i in range(300)]
    bad = bamgen.make_record(0, 5, "4M", "ACGT", 30, name="rX")
    bad = bad[:37] + b"\x80" + bad[38:]
    path = str(tmp_path / "highbit.bam")
    bamgen.write_bam(path, REFS, good[:150] + [bad, bad] + good[150:], text=UNSORTED, write_index=False)
    for order in (ref.LEX, ref.NATURAL):
        _assert_refused(path, tmp_path, order, False, "2 record(s)")
    hiz = str(tmp_path / "hiz.bam")
    recs = good[:100] + [bamgen.make_record(0, 7, "4M", "ACGT", 30, name="r1", tags=bamgen.tag_z("HI", "2"))] + good[100:]
    bamgen.write_bam(hiz, REFS, recs, text=UNSORTED, write_index=False)
    _assert_refused(hiz, tmp_path, ref.LEX, True, "1 record(s)")
    _assert_refused(hiz, tmp_path, ref.NATURAL, True, "1 record(s)")
    check(hiz, tmp_path, ref.LEX, False, tag="hiz")                       # the same file sorts without -M
    # the coordinate sort takes both files as before
    import sambamba_amd
    for p in (path, hiz):
        out = str(tmp_path / "c.bam")
        sambamba_amd.sort_bam(p, out)
        check_file(out, sort_ref.expected(p))


# ---- small files ----
def test_empty_and_one_record(tmp_path):
    empty = str(tmp_path / "empty.bam")
    bamgen.write_bam(empty, REFS, [], text=UNSORTED, write_index=False)
    one = str(tmp_path / "one.bam")
    bamgen.write_bam(one, REFS, [bamgen.make_record(1, 10, "4M", "ACGT", 30, name="only", tags=bamgen.tag_num("HI", "C", 2))], text=UNSORTED,
                     write_index=False)
    for order in (ref.LEX, ref.NATURAL):
        for mm in (False, True):
            st, _ = check(empty, tmp_path, order, mm, tag="e")
            assert st["n_records_out"] == 0 and st["n_sort_passes"] == 0
            st, _ = check(one, tmp_path, order, mm, tag="1")
            assert st["n_records_out"] == 1 and st["n_sort_passes"] == 0
    want = ref.expected(empty, ref.LEX)
    assert sort_ref.split_stream(want)[3] == [] and want[8:].startswith(b"@HD\tVN:1.6\tSO:queryname\n@SQ\tSN:c1\tLN:100000\n")


# ---- what was there stays as it was ----
def test_coordinate_order_is_unchanged(generated, tmp_path):
    import sambamba_amd
    from sambamba_amd import sort_cli_path
    path, _, _ = generated
    want = sort_ref.expected(path)
    a, b = str(tmp_path / "a.bam"), str(tmp_path / "b.bam")
    sambamba_amd.sort_bam(path, a)
    sambamba_amd.sort_bam(path, b, order="coordinate", match_mates=False, index=True)
    check_file(a, want)
    assert open(a, "rb").read() == open(b, "rb").read() and os.path.exists(b + ".bai") and not os.path.exists(a + ".bai")
    # sbx-nsort without -n / -N is sbx-sort, .bai included
    c, d = str(tmp_path / "c.bam"), str(tmp_path / "d.bam")
    r1 = subprocess.run([sort_cli_path(), "-o", c, path, "-F", "reverse_strand"], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    r2 = cli(["-o", d, path, "-F", "reverse_strand"])
    assert r1.returncode == 0 and r2.returncode == 0, (r1.stderr, r2.stderr)
    assert open(c, "rb").read() == open(d, "rb").read()
    assert open(c + ".bai", "rb").read() == open(d + ".bai", "rb").read()
    check_file(d, sort_ref.expected(path, _reverse))


# ---- the scan of the word counts (launch_count_scan) at the edges of its round of 4096 counts ----
@pytest.fixture(scope="module")
def scan_round_records():
    rng = random.Random(20241019)
    return _records(_names(rng, 8193), rng)


@pytest.mark.parametrize("order", [ref.LEX, ref.NATURAL])
@pytest.mark.parametrize("n", [4095, 4096, 4097, 8193])
def test_record_counts_around_the_scan_round(scan_round_records, n, order, tmp_path):
    path = str(tmp_path / "n.bam")
    bamgen.write_bam(path, REFS, scan_round_records[:n], text=UNSORTED, write_index=False)
    st, _ = check(path, tmp_path, order)
    assert st["n_records_out"] == n and st["n_batches"] == 1
