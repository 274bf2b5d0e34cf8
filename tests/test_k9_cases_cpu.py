"""The premises of tests/test_gpu_k9_edges.py, checked without a GPU: every case of tests/k9_cases.py sits on the limit its docstring
names; the restatement of `sort_key` / `plan_passes` the expected stats come from equals sort_core.hpp (tests/native/sort_host.cpp);
the gather file reaches every alignment of copy_span16; and the cases CAN fail -- a plain model of K9b (tiles, rounds, waves, peer
ranks, [digit][tile] bases, running offsets, two buffers) equals a stable sort on every case, and with one defect switched on gets
a named case wrong."""
import os
import struct
import subprocess

import pytest

from tests import k9_cases as kc
from tests import sort_ref
from tests.util import ROOT

TILE, ROUND, WAVE = kc.TILE, kc.ROUND, kc.WAVE


@pytest.fixture(scope="module")
def sort_host(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("k9") / "sort_host")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-o", exe, os.path.join(ROOT, "tests", "native", "sort_host.cpp")])
    return exe


@pytest.fixture(scope="module")
def namesort_host(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("k9") / "namesort_host")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-o", exe, os.path.join(ROOT, "tests", "native", "namesort_host.cpp")])
    return exe


def out_of(exe, args, data=b""):
    r = subprocess.run([exe] + [str(a) for a in args], input=data, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert r.returncode == 0, r.stderr
    return r.stdout


# ---- the restatement is sort_core.hpp -------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", kc.COORDINATE_NAMES)
def test_keys_and_plan_are_those_of_sort_core(sort_host, name):
    c = kc.case(name)
    kept = [r for r in c.records if c.keep is None or c.keep(r)]
    lines = "".join("%d %d %d\n" % kc.fields_of_record(r) for r in kept)
    assert [int(x) for x in out_of(sort_host, ["keys", len(c.refs)], lines.encode()).split()] == c.keys
    got = [int(x) for x in out_of(sort_host, ["passes", c.varying]).split()]
    assert got[0] == len(c.shifts) == c.expect["n_sort_passes"] and got[1] == c.expect["key_bits"] and got[2:] == c.shifts
    # the restatement orders as the oracle of the device test does
    n_ref = len(c.refs)
    assert sorted(range(len(kept)), key=lambda i: c.keys[i]) == sorted(range(len(kept)), key=lambda i: sort_ref.record_key(kept[i], n_ref))


def test_rules_for_every_case():
    """Names carry the file index; records are short (4 to 10 bases, no tags) except in the gather file; at most about 12,300 records."""
    for name in kc.COORDINATE_NAMES:
        c = kc.case(name)
        assert len(c.records) <= 12300
        if name == "gather":
            continue
        for i, r in enumerate(c.records):
            l_name, n_cig, l_seq = r[12], struct.unpack_from("<H", r, 16)[0], struct.unpack_from("<i", r, 20)[0]
            assert int(r[37:36 + l_name - 1]) == i and 4 <= l_seq <= 10
            assert len(r) == 36 + l_name + 4 * n_cig + (l_seq + 1) // 2 + l_seq            # no tags


# ---- 1 ----
def test_record_counts():
    assert kc.COUNTS == (1, 2, 63, 64, 65, 255, 256, 257, 4095, 4096, 4097, 8191, 8192, 8193, 12289)
    assert {n % 16 for n in kc.COUNTS} >= {0, 1, 15}
    for n in kc.COUNTS:
        c = kc.case("count%d" % n)
        pos = [kc.fields_of_record(r)[1] for r in c.records]
        assert len(pos) == n and all(a > b for a, b in zip(pos, pos[1:])) and pos[-1] == 0
        assert c.expect["n_records_out"] == n and (c.expect["n_sort_passes"] >= 1) == (n > 1)
    assert kc.case("count1").expect["n_sort_passes"] == 0 and kc.case("count1").expect["key_bits"] == 0
    two = kc.case("two_equal")
    assert len(two.records) == 2 and two.keys[0] == two.keys[1] and two.expect["n_sort_passes"] == 0 and two.expect["key_bits"] == 0


# ---- 2 ----
def test_pass_plans():
    for name, (shifts, bits) in kc.PLAN_SHIFTS.items():
        c = kc.case(name)
        if shifts is not None:
            assert (c.shifts, c.expect["key_bits"]) == (shifts, bits), name
        assert len(set(c.keys)) < len(c.keys)                               # ties
        assert c.keys != sorted(c.keys)                                     # and something moves
    assert {len(kc.case(n).shifts) for n in kc.PLAN_SHIFTS} >= {1, 2, 3, 4, 5, 6}
    # unaligned digits: the top digit of `overhang` reaches past the highest varying bit
    c = kc.case("overhang")
    assert c.varying == 0x1FF << 5 and c.shifts[-1] + 8 > c.varying.bit_length()
    assert kc.case("unaligned").varying == 0xFF << 5
    for w in (8, 9, 16, 17, 25):
        assert kc.case("width%d" % w).varying == ((1 << w) - 1) << 1
    assert len(kc.case("width17").records) == TILE + 1
    assert kc.case("skipped").varying == 0xFF | 3 << 33
    c = kc.case("strand")
    assert len(c.records) == 2 * TILE + 1 and len(set(c.keys)) == 2 and c.varying == 1
    c = kc.case("refbit")
    assert c.varying == 1 << 33 and len(set(c.keys)) == 2
    c = kc.case("unmapped")
    mapped = [i for i, r in enumerate(c.records) if kc.fields_of_record(r)[0] >= 0]
    assert mapped == [len(c.records) - 2] and len(set(c.keys)) == 2 and c.expect["n_sort_passes"] >= 1
    c = kc.case("widest")
    assert len(c.refs) == 300 and all(ln == 2 ** 31 - 1 for _, ln in c.refs)
    assert c.varying == ((1 << 42) - 1) & ~(1 << 32)
    assert max(kc.fields_of_record(r)[1] for r in c.records) == 2 ** 31 - 2
    assert any(kc.fields_of_record(r)[0] < 0 for r in c.records)


# ---- 3 ----
def lanes(digits, rnd):
    return digits[rnd * ROUND:(rnd + 1) * ROUND]


def test_digit_layouts():
    lay = kc.layout_digits()
    assert sorted(lay) == sorted(kc.LAYOUT_NAMES)
    for name, digits in lay.items():
        c = kc.case(name)
        # one pass at shift 0: lane i of the pass extracts digits[i]
        assert c.shifts == [0] and [k & 255 for k in c.keys] == digits and all(k < 256 for k in c.keys), name
    d = lay["uniform_rounds"]
    assert len(d) == TILE + 2 * ROUND
    per_round = [set(lanes(d, g)) for g in range(len(d) // ROUND)]
    assert all(len(s) == 1 for s in per_round) and all(a != b for a, b in zip(per_round, per_round[1:]))
    d = lay["everywhere"]
    assert len(d) == 3 * TILE and all(0 < lanes(d, g).count(77) < ROUND for g in range(3 * TILE // ROUND))
    d = lay["descending"]
    assert lanes(d, 0) == lanes(d, 1) == list(range(255, -1, -1)) and lanes(d, 2) == list(range(256))
    d = lay["lanes_0_63"]
    assert [i for i, x in enumerate(d) if x == 253] == [ROUND + WAVE, ROUND + 2 * WAVE - 1]
    d = lay["wave_edge"]
    assert [i for i, x in enumerate(d) if x == 252] == [ROUND + WAVE - 1, ROUND + WAVE]
    d = lay["wave3_alone"]
    waves_with = lambda rnd: {l // WAVE for l, x in enumerate(lanes(d, rnd)) if x == 254}
    assert waves_with(0) == {0, 1, 2} and waves_with(1) == {3} and waves_with(2) == {0}
    d = lay["extremes"]
    r1 = lanes(d, 1)
    assert set(r1[2 * WAVE:3 * WAVE]) == {0, 255} and not {0, 255} & set(r1[:2 * WAVE] + r1[3 * WAVE:])
    d = lay["dead_lanes"]
    assert len(d) == ROUND + 10 and d[ROUND:] == [0] * 10 and 0 in d[:ROUND]
    d = lay["last_lane"]
    assert len(d) == TILE + 257 and d.count(255) == 1 and d[-1] == 255


# ---- 4 ----
def test_filter_placements():
    keeps = kc.filter_keeps()
    G = kc.GROUP
    assert sorted("filter_" + k for k in keeps) == sorted(kc.FILTER_NAMES)
    group = lambda k, g: keeps[k][g * G:(g + 1) * G]
    assert all(len(v) == 2 * G + G // 2 for k, v in keeps.items() if k != "first_group_empty")
    assert not any(group("group_rejected", 1)) and any(group("group_rejected", 0)) and any(group("group_rejected", 2))
    assert [l for l, k in enumerate(group("lane0_only", 1)) if k] == [0]
    assert [l for l, k in enumerate(group("lane255_only", 1)) if k] == [G - 1]
    g = group("wave2_rejected", 1)
    assert not any(g[2 * WAVE:3 * WAVE]) and all(g[:2 * WAVE]) and all(g[3 * WAVE:])
    assert keeps["alternating"] == [False, True] * (G + G // 4)
    assert all(keeps["all_kept"])
    k = keeps["first_group_empty"]
    assert len(k) == G + G // 2 and not any(k[:G]) and any(k[G:]) and not all(k[G:])
    assert sum(keeps["one_kept"]) == 1 and not any(keeps["none_kept"])
    for name in kc.FILTER_NAMES:
        c = kc.case(name)
        assert [c.keep(r) for r in c.records] == keeps[name[7:]]
        assert c.expect["n_records_out"] == sum(keeps[name[7:]])
        # the rejected records carry key bits no kept key has: with them the plan would be another
        all_keys = [kc.key_of_record(r, len(c.refs)) for r in c.records]
        k_or = 0
        k_and = (1 << 64) - 1
        for k in all_keys:
            k_or |= k
            k_and &= k
        if not all(keeps[name[7:]]):
            assert kc.plan_passes(k_or ^ k_and) != (c.shifts, c.expect["key_bits"]), name
    assert kc.case("filter_none_kept").expect == {"n_records_in": 640, "n_records_out": 0, "n_sort_passes": 0, "key_bits": 0}
    assert kc.case("filter_one_kept").expect["n_sort_passes"] == 0
    assert kc.case("filter_alternating").expect["n_sort_passes"] == 1 and kc.case("filter_alternating").expect["key_bits"] == 7


# ---- 5 ----
def test_gather_alignments():
    """src: the record's offset in the record store, which begins with the file's first record (behind the header and the
    reference list); dst: its offset in the sorted stream, behind the re-serialised header (one piece: the piece buffer begins
    with the stream).  Both buffers are device allocations, aligned to more than 16 bytes."""
    c = kc.case("gather")
    n = len(c.records)
    assert n == kc.GATHER_N and len(set(c.keys)) == n
    src, at = [], 0
    for r in c.records:
        src.append(at)
        at += len(r)
    text = "@HD\tVN:1.6\tSO:coordinate\n" + "".join("@SQ\tSN:%s\tLN:%d\n" % r for r in c.refs)
    hlen = len(kc.bg.bam_header(sort_ref.header_text(text), c.refs))
    pairs, heads, tails, chunks = set(), set(), set(), set()
    at = hlen
    for i in sorted(range(n), key=lambda i: c.keys[i]):
        ln = len(c.records[i])
        h, ch, t = kc.copy_span16_parts(at, ln)
        assert h + 16 * ch + t == ln
        pairs.add((at & 15, src[i] & 15))
        heads.add(h)
        tails.add(t)
        chunks.add(ch)
        at += ln
    assert len(pairs) == 256
    assert heads == set(range(16)) and tails == set(range(16))
    assert chunks & {0, 1} and {15, 16, 17} <= chunks and max(chunks) > 32
    lengths = [len(r) for r in c.records]
    assert min(lengths) == 37 == len(kc.bg.make_record(0, 0, "", "", 0, name=""))
    assert any(272 < x <= 4352 for x in lengths) and any(x > 4352 for x in lengths)
    assert {r[12] for r in c.records} >= {1, 2, 254}


# ---- 6 ----
def test_name_case_word_plans(namesort_host, sort_host):
    c = kc.case("names")
    got = [[int(x) for x in ln.split()] for ln in out_of(namesort_host, ["words", 1], "".join(nm + "\n" for nm in c.names).encode()).decode().splitlines()]
    assert got == c.words and all(len(w) == 2 for w in got)
    assert len(set(c.names)) == len(c.names)
    (s1, b1), (s0, b0) = c.per_word
    assert len(s1) % 2 == 1 and len(s0) >= 1            # the second word sorted starts from the second value buffer
    assert (s1, b1, s0, b0) == ([0], 4, [0, 8, 16, 24], 28)
    assert c.expect["n_sort_passes"] == 5 and c.expect["key_bits"] == 32
    varying = []
    for w in (1, 0):
        col = [ws[w] for ws in c.words]
        k_or, k_and = 0, (1 << 64) - 1
        for x in col:
            k_or, k_and = k_or | x, k_and & x
        varying.append(k_or ^ k_and)
    assert varying == [0xF, 0x0F0F0F0F]
    for varying, (shifts, bits) in zip(varying, c.per_word):
        got = [int(x) for x in out_of(sort_host, ["passes", varying]).split()]
        assert got == [len(shifts), bits] + shifts
    assert c.names != sorted(c.names)


# ---- 7. the cases can fail --------------------------------------------------------------------------------------------------
DEFECTS = {
    # defect -> the cases that must come out different from the stable sort
    "dead_lanes_counted": ["dead_lanes", "count257"],
    "no_waves_in_front": ["uniform_rounds", "wave3_alone"],
    "off_not_advanced": ["uniform_rounds", "everywhere", "descending"],
    "base_tile_digit": ["everywhere", "count8193", "strand"],
    "rank_le": ["lanes_0_63", "wave_edge", "last_lane"],
    "other_buffer": ["shift0", "overhang", "width17", "widest"],
    "digits_from_bit_0": ["unaligned", "skipped", "refbit"],
}


def model_pass(keys, vals, shift, defect=None):
    """One pass of K9b as sort.hip runs it; (keys, vals) out, or None when a slot is written twice, never, or outside [0, n)."""
    n = len(keys)
    tiles = (n + TILE - 1) // TILE
    digit = [(k >> shift) & 255 for k in keys]
    hist = [0] * (256 * tiles)                          # k_radix_hist: [digit][tile]
    for i in range(n):
        hist[digit[i] * tiles + i // TILE] += 1
    if defect == "dead_lanes_counted" and n % ROUND:    # the dead lanes of the partial round count as digit 0
        hist[0 * tiles + tiles - 1] += ROUND - n % ROUND
    base, run = [], 0                                   # launch_count_scan
    for h in hist:
        base.append(run)
        run += h
    out_k, out_v = {}, {}
    for t in range(tiles):
        if defect == "base_tile_digit":
            off = [base[t * 256 + d] for d in range(256)]
        else:
            off = [base[d * tiles + t] for d in range(256)]
        for r in range(TILE // ROUND):
            start = t * TILE + r * ROUND
            if start >= n:
                break
            wcount = [dict() for _ in range(ROUND // WAVE)]
            slots = []
            for w in range(ROUND // WAVE):
                peers = {}
                for l in range(WAVE):
                    i = start + w * WAVE + l
                    live = i < n
                    if not live and defect not in ("dead_lanes_counted", "dead_lanes_in_peers"):
                        continue
                    d = digit[i] if live else 0
                    p = peers.setdefault(d, [])
                    rank = len(p) + (1 if defect == "rank_le" else 0)
                    p.append(live)
                    if live:
                        slots.append((i, w, d, rank))
                for d, p in peers.items():
                    if p[0]:                            # the lowest peer publishes, if it is live
                        wcount[w][d] = len(p)
            for i, w, d, rank in slots:
                at = off[d] + rank
                if defect != "no_waves_in_front":
                    at += sum(wcount[x].get(d, 0) for x in range(w))
                if at in out_k or not 0 <= at < n:
                    return None
                out_k[at], out_v[at] = keys[i], vals[i]
            if defect != "off_not_advanced":
                for wc in wcount:
                    for d, cnt in wc.items():
                        off[d] += cnt
    if len(out_k) != n:
        return None
    return [out_k[i] for i in range(n)], [out_v[i] for i in range(n)]


def model_sort(keys, shifts, defect=None):
    """queue_resident_passes: two key and two value buffers; the permutation, or None."""
    n = len(keys)
    kbuf, vbuf = [list(keys), [None] * n], [list(range(n)), [None] * n]
    at = 0
    for p, s in enumerate(shifts):
        got = model_pass(kbuf[at], vbuf[at], 8 * p if defect == "digits_from_bit_0" else s, defect)
        if got is None:
            return None
        kbuf[at ^ 1], vbuf[at ^ 1] = got
        at ^= 1
    return vbuf[at ^ 1] if defect == "other_buffer" else vbuf[at]


def stable(keys):
    return sorted(range(len(keys)), key=lambda i: keys[i])


@pytest.mark.parametrize("name", kc.COORDINATE_NAMES)
def test_model_without_a_defect_is_a_stable_sort(name):
    c = kc.case(name)
    assert model_sort(c.keys, c.shifts) == stable(c.keys)


@pytest.mark.parametrize("defect,name", [(d, n) for d, names in DEFECTS.items() for n in names])
def test_every_defect_gets_a_named_case_wrong(defect, name):
    c = kc.case(name)
    assert name in kc.COORDINATE_NAMES and len(c.shifts) >= 1
    assert model_sort(c.keys, c.shifts, defect) != stable(c.keys)


@pytest.mark.parametrize("name", [n for n in kc.COORDINATE_NAMES if len(kc.case(n).keys) % ROUND and kc.case(n).shifts])
def test_dead_lanes_in_the_peers_alone_cannot_show(name):
    """Why `dead_lanes_counted` counts them in the histogram too.  The dead lanes of K9b are the lanes behind the last record: in
    k_radix_scatter they sit above every live lane of their wave (no rank changes), in front of no live wave and of no later round
    (the inflated count of digit 0 is never read), so no input can show them there -- the model says the same of every case with a
    partial round.  Counted in k_radix_hist they move the base of every digit above 0, which `dead_lanes` and `count257` show."""
    c = kc.case(name)
    assert model_sort(c.keys, c.shifts, "dead_lanes_in_peers") == stable(c.keys)
