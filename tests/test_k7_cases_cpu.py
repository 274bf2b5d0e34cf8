"""The premises of tests/test_gpu_k7_edges.py, checked without a GPU: every builder of tests/k7_cases.py still puts its records on
the limit its docstring names.  The rules of mates.hip that the checks need are restated here in plain Python: who is whose
partner (`link_if_mates`: admitted, same contig, name and sample, overlapping), which records phase 1 of k_accumulate_mates takes
(`eligible_fast` and the 11-block test) and where a record sits in the window of its workgroup of k_find_mates_join."""
import struct

import numpy as np
import pytest

from tests import k7_cases as kc
from tests.test_k3_cases_cpu import classify, n_blocks, parse


def describe(records):
    """The records of a file in file order, with what K2 and K7 know of them."""
    out = []
    for i, b in enumerate(records):
        r = parse(b)
        l_name = b[12]
        r["index"], r["name"] = i, b[36:36 + l_name - 1].decode()
        tail = b[36 + l_name + 4 * len(r["cigar"]) + (r["l_seq"] + 1) // 2 + r["l_seq"]:]
        r["group"] = tail[3:-1].decode() if tail[:3] == b"RGZ" else ""
        r["qual"] = b[len(b) - len(tail) - r["l_seq"]:len(b) - len(tail)]
        r["kind"], r["end"], r["q_lead"] = classify(r)
        out.append(r)
    assert all((a["ref"], a["pos"]) <= (b["ref"], b["pos"]) for a, b in zip(out, out[1:]))
    return out


def link(recs):
    """r["partners"] = the records K7 links r with, for every record."""
    by_key = {}
    for r in recs:
        r["partners"] = []
        if r["kind"]:
            by_key.setdefault((r["ref"], r["name"], r["group"]), []).append(r)
    for group in by_key.values():
        for i, a in enumerate(group):
            for b in group[i + 1:]:
                if b["pos"] < a["end"] and b["end"] > a["pos"]:
                    a["partners"].append(b)
                    b["partners"].append(a)
    return recs


def single_run_ok(r):
    return r["kind"] == 1 and r["q_lead"] + r["end"] - r["pos"] <= r["l_seq"]


def blocks_in_tile(r, ts, te):
    a, b = max(r["pos"], ts), min(r["end"], te)
    return n_blocks(a - ts, b - a) if b > a else 0


def phase1(r, ts, te):
    """Does phase 1 take record r in the tile [ts, te)?  eligible_fast() and the 11-block test of mates.hip."""
    ok = len(r["partners"]) <= 1 and single_run_ok(r) and all(single_run_ok(p) for p in r["partners"])
    return ok and blocks_in_tile(r, ts, te) <= kc.FAST_BLOCKS


def max_depth(refs, recs):
    top = 0
    for ref, (_, ln) in enumerate(refs):
        depth = np.zeros(ln + 1, dtype=int)
        for r in recs:
            if r["ref"] == ref and r["kind"]:
                depth[r["pos"]] += 1
                depth[min(r["end"], ln)] -= 1
        top = max(top, int(np.cumsum(depth).max()))
    return top


def pairs_of(recs):
    """[(first, second)] of the name groups of two records."""
    names = {}
    for r in recs:
        names.setdefault((r["ref"], r["name"]), []).append(r)
    assert all(len(g) == 2 for g in names.values())
    return list(names.values())


@pytest.mark.parametrize("n_samples", [1, 2, 3])
def test_the_sweep_has_every_cell_and_stays_shallow(n_samples):
    T = kc.tile_positions(n_samples)
    refs, records, groups = kc.pair_sweep(n_samples)
    assert len(groups) == (n_samples if n_samples > 1 else 0) and all(ln == T for _, ln in refs)
    recs = link(describe(records))
    assert max_depth(refs, recs) <= 2 * kc.MAX_PAIRS
    grid, ends, lengths_a, lengths_b, shapes, edges, mixed, extremes, used = set(), set(), set(), set(), set(), {}, set(), set(), set()
    for a, b in pairs_of(recs):
        assert a["kind"] == b["kind"] == 1 and a["group"] == b["group"] and b["end"] <= T and a["end"] <= T
        assert single_run_ok(a) and single_run_ok(b)
        used.add(a["group"])
        d, na, nb = b["pos"] - a["pos"], a["end"] - a["pos"], b["end"] - b["pos"]
        off, pa, pb = a["pos"] & 15, a["q_lead"] & 1, b["q_lead"] & 1
        overlap = d < na
        assert (a["partners"] == [b]) == overlap
        if set(a["qual"]) | set(b["qual"]) <= set(kc.EXTREME_QUALS):
            extremes.add(d)
            assert {0, 255} <= set(a["qual"][d:]) and {0, 255} <= set(b["qual"])
            assert any(x == y for x, y in zip(a["qual"][d:], b["qual"]))       # a tie at an extreme
        if na in kc.BLOCK_EDGE_LENGTHS or nb in kc.BLOCK_EDGE_LENGTHS:
            for who, r, n in (("A", a, na), ("B", b, nb)):
                if n in kc.BLOCK_EDGE_LENGTHS:
                    edges[(who, r["pos"] & 15, r["q_lead"] & 1, n)] = blocks_in_tile(r, 0, T)
            if na in kc.BLOCK_EDGE_LENGTHS and nb in kc.BLOCK_EDGE_LENGTHS:
                mixed.add((phase1(a, 0, T), phase1(b, 0, T), off))
            continue
        if overlap:
            grid.add((off, d, pa, pb))
            ends.add((off, min(a["end"], b["end"]) & 15))
            lengths_a.add(na)
            lengths_b.add(nb)
        shapes.add(("same" if (d, na) == (0, nb) else "a_in_b" if d == 0 and nb > na else "b_in_a" if d > 0 and b["end"] < a["end"]
                    else "abut" if d == na else "one_column" if d == na - 1 and nb > 1 else "other", off))
    assert used == {g for g, _ in groups} or n_samples == 1
    assert grid >= {(o, d, pa, pb) for o in range(16) for d in kc.SWEEP_STARTS for pa in (0, 1) for pb in (0, 1)}
    assert ends == {(o, e) for o in range(16) for e in range(16)}
    assert lengths_a >= set(kc.SWEEP_LENGTHS) and lengths_b >= set(kc.SWEEP_LENGTHS)
    assert shapes >= {(s, o) for s in ("same", "a_in_b", "b_in_a", "abut", "one_column") for o in (0, 1, 7, 15)}
    assert set(edges) >= {(w, o, p, n) for w in "AB" for o in kc.BLOCK_EDGE_OFFSETS for p in (0, 1) for n in kc.BLOCK_EDGE_LENGTHS}
    for w in "AB":
        for p in (0, 1):
            assert (edges[(w, 15, p, 161)], edges[(w, 15, p, 162)]) == (kc.FAST_BLOCKS, kc.FAST_BLOCKS + 1)
            assert (edges[(w, 0, p, 176)], edges[(w, 0, p, 177)]) == (kc.FAST_BLOCKS, kc.FAST_BLOCKS + 1)
    # one mate in phase 1 and the other on the per-position path, either one first, at both offsets
    assert mixed == {(True, False, 0), (False, True, 0), (True, False, 15), (False, True, 15)}
    assert extremes == {0, 1, 2, 3}


@pytest.mark.parametrize("n_samples", [1, 2, 3])
def test_the_border_pairs_lie_where_the_docstring_says(n_samples):
    T = kc.tile_positions(n_samples)
    refs, records, _ = kc.pair_borders(n_samples)
    names = [n for n, _ in refs]
    recs = link(describe(records))
    assert max_depth(refs, recs) <= 2 * kc.MAX_PAIRS
    assert all(r["kind"] == 1 and single_run_ok(r) and len(r["partners"]) == 1 for r in recs)
    seen, per_border = set(), {}
    for x, y in pairs_of([r for r in recs if r["ref"] == 0]):
        a, b = (x, y) if x["mapq"] == 60 else (y, x)
        assert (a["mapq"], b["mapq"]) == kc.A_FIRST
        border = (a["pos"] // T + 1) * T
        d, m = border - a["pos"], a["end"] - border
        assert d in kc.BORDER_BEFORE and m in kc.BORDER_BEHIND
        per_border[border] = per_border.get(border, 0) + 1
        o0, o1 = max(a["pos"], b["pos"]), min(a["end"], b["end"])
        assert o1 > o0
        if b["index"] < a["index"]:
            assert b["pos"] < a["pos"]
            seen.add((d, m, "b_first"))
            continue
        if o1 == border:
            seen.add((d, m, "ends_at"))
        if b["pos"] == a["pos"] and (o1 < border or d == 1):        # (d = 1: a B that covers A's first base ends at the border)
            seen.add((d, m, "before"))
        if o0 >= border:
            seen.add((d, m, "behind"))
        if o0 < border < o1:
            seen.add((d, m, "spans"))
    assert seen == {(d, m, w) for d in kc.BORDER_BEFORE for m in kc.BORDER_BEHIND for w in kc.BORDER_WAYS}
    assert max(per_border.values()) <= kc.MAX_PAIRS and refs[0] == ("edge", max(per_border) + T)
    far = set()
    for ref, (name, ln) in enumerate(refs):
        if name.startswith("far"):
            (b, a), = pairs_of([r for r in recs if r["ref"] == ref])
            assert ln == 3 * T and b["pos"] // T == 0 and a["pos"] // T == 1 and not phase1(b, T, 2 * T) and phase1(a, T, 2 * T)
            far.add((2 * T - a["pos"], a["end"] - 2 * T, b["end"] - a["pos"]))
    assert far == {(d, m, x) for d in (1, 16, 17) for m in (1, 17) for x in (1, d, d + m)}
    last = [r for r in recs if r["ref"] == names.index("last")]
    ln = refs[names.index("last")][1]
    assert ln % T and any(r["pos"] < T < r["end"] for r in last) and sum(r["end"] == ln for r in last) == 2
    depth = np.zeros(T, dtype=int)
    for r in recs:
        if r["ref"] == names.index("steps"):
            depth[r["pos"]:r["end"]] += 1
    for q in (1, 2, 3):
        assert depth[q * T // 4 - 1] == depth[q * T // 4] == 2 and depth[q * T // 4 + T // 8] == 0
    assert depth[0] == 2 and depth[T - 1] == 2


def columns(r):
    """position -> 'M', 'D' or 'N' of an admitted record (zero-length operations take one column, the record ends at r["end"])."""
    out, rp = {}, r["pos"]
    for op, n in r["cigar"]:
        if op in "MDN=X":
            for p in range(rp, min(rp + max(n, 1), r["end"])):
                out[p] = "M" if op in "M=X" else op
            rp += max(n, 1)
    return out


def test_the_kinds_meet_the_single_run_read_in_every_way():
    refs, records, groups = kc.pair_kinds()
    recs = link(describe(records))
    assert not groups and max_depth(refs, recs) <= 2
    seen, met = set(), set()
    for a, b in pairs_of(recs):
        assert a["partners"] == [b] and a["index"] < b["index"]
        ca, cb = columns(a), columns(b)
        met.update(ca[p] + cb[p] for p in ca if p in cb)
        text = ["".join("%d%s" % (n, op) for op, n in r["cigar"]) for r in (a, b)]
        order = (a["mapq"] > b["mapq"]) - (a["mapq"] < b["mapq"])
        if "24M" in text:
            first = text[0] == "24M"
            # clips and padding leave one run: those pairs are phase 1's; every other shape sends BOTH mates to the per-position path
            one_run = text[first] in ("3H20M", "20M3H", "10M2P10M", "4S20M", "20M4S")
            assert phase1(a, 0, 1 << 30) == phase1(b, 0, 1 << 30) == one_run
            seen.add((text[first], first, b["pos"] - a["pos"], order))
        else:
            assert sorted(text) == ["10M4D10M", "8M6N10M"]
            seen.add(("DN", order))
    assert seen == ({(s, f, d, o) for s in kc.KIND_SHAPES for f in (False, True) for d in kc.KIND_STARTS for o in (-1, 0, 1)}
                    | {("DN", o) for o in (-1, 0, 1)})
    assert met >= {"MM", "DM", "MD", "NM", "MN", "DN"}
    refs, records, _ = kc.short_sequence()
    recs = link(describe(records))
    short = [r for r in recs if r["l_seq"] == 0]
    assert len(short) == 1 and short[0]["kind"] == 1 and not single_run_ok(short[0]) and len(short[0]["partners"]) == 1
    assert not phase1(short[0], 0, 1024) and not phase1(short[0]["partners"][0], 0, 1024)


def test_the_work_list_is_full_in_one_tile_and_overflows_in_another():
    T = 1024
    refs, records, _ = kc.work_list()
    assert refs == [("list", 3 * T)]
    recs = link(describe(records))
    assert all(r["kind"] and len(r["partners"]) <= 1 and r["pos"] // T == (r["end"] - 1) // T for r in recs)
    listed, fast_pairs, listed_mates = [0, 0, 0], [0, 0, 0], [0, 0, 0]
    for r in recs:
        t = r["pos"] // T
        if phase1(r, t * T, t * T + T):
            fast_pairs[t] += bool(r["partners"] and r["index"] < r["partners"][0]["index"])
        else:
            listed[t] += 1
            listed_mates[t] += bool(r["partners"] and r["partners"][0]["kind"] == 2 and r["kind"] == 2)
    assert listed == [kc.WORK_CAP, 0, kc.WORK_CAP + 1] and kc.WORK_CAP == 382
    assert fast_pairs[0] >= 200 and fast_pairs[2] >= 200 and fast_pairs[1] > 0
    assert listed_mates[0] >= 100 and listed_mates[2] >= 100
    # the records phase 1 takes lie between the listed ones, not behind them
    kinds = [phase1(r, 0, T) for r in recs if r["pos"] < T]
    assert sum(a != b for a, b in zip(kinds, kinds[1:])) > 200


@pytest.mark.parametrize("n", [65535, 65536])
def test_the_tile_holds_exactly_n_records(n):
    refs, records, _ = kc.index_limit(n)
    assert refs == [("tile", 1024)] and len(records) == n
    recs = link(describe(records))
    assert all(r["kind"] and r["end"] <= 1024 and len(r["partners"]) <= 1 for r in recs)       # all admitted, all in the one tile
    listed = [r["index"] for r in recs if not phase1(r, 0, 1024)]
    assert len(listed) == kc.INDEX_GAPPED and listed[-3:] == [n - 3, n - 2, n - 1]
    assert (n > 0xFFFF) == (n == 65536)         # the guard `r_hi - r_lo > 0xFFFF`
    pairs = [r for r in recs if r["partners"]]
    assert len(pairs) == 2 * kc.INDEX_PAIRS and {p["end"] - p["pos"] for p in pairs} == {2}
    assert {min(a["end"], a["partners"][0]["end"]) - max(a["pos"], a["partners"][0]["pos"]) for a in pairs} == {1, 2}
    per_pos = np.bincount([r["pos"] for r in recs if r["cigar"] == [("M", 1)]], minlength=1024)
    assert set(per_pos[:1022]) <= {63, 64} and not per_pos[1022:].any()
    assert max(r["end"] - r["pos"] for r in recs) <= 3


def test_the_join_scenarios_sit_at_their_window_indices():
    refs, records, _ = kc.join_window()
    names = [n for n, _ in refs]
    recs = link(describe(records))
    assert max(len(r["partners"]) for r in recs) == 1
    W, G = kc.JOIN_WINDOW, kc.JOIN_GROUP

    def a_and_mate(contig):
        (a,) = [r for r in recs if r["ref"] == names.index(contig) and r["end"] - r["pos"] == kc.A_LEN]
        (m,) = a["partners"]
        base = a["index"] - a["index"] % G
        return a, m, base

    for w in kc.JOIN_MATE_AT:
        for t in kc.JOIN_LANES:
            a, m, base = a_and_mate("w%d_t%d" % (w, t))
            assert a["index"] % G == t and m["index"] - base == w and a["pos"] <= m["pos"] < a["end"]
            between = recs[a["index"] + 1:m["index"]]
            assert all(r["ref"] == a["ref"] and a["pos"] <= r["pos"] < a["end"] and r["end"] - r["pos"] == 1 for r in between)
            assert len({r["name"] for r in between}) == len(between)
            # the window's last entry lies inside A's span (the scan goes on in global memory) unless the mate is the last entry
            last = recs[base + W - 1]
            assert last["ref"] == a["ref"] and last["pos"] < a["end"]
            behind = [r for r in recs[m["index"] + 1:] if r["ref"] == a["ref"]]
            assert any(r["pos"] < a["end"] for r in behind) and any(r["pos"] >= a["end"] for r in behind)
    assert {1023, 1024, 1025} <= set(kc.JOIN_MATE_AT) and W == 1024 and G == 256
    a, m, base = a_and_mate("next_ref")
    assert m["index"] - base < W - 1 and recs[base + W - 1]["ref"] == a["ref"] + 1
    a, m, base = a_and_mate("filtered_last")
    last = recs[base + W - 1]
    assert last["kind"] == 0 and last["mapq"] == 0 and last["ref"] == a["ref"] and last["pos"] < a["end"] and m["index"] - base > W
    assert sum(r["kind"] == 0 for r in recs) == 1
    a, m, base = a_and_mate("file_end")
    assert m["index"] == len(recs) - 1 < base + W - 1
    # one name on two adjacent contigs, same coordinates, inside one window
    dup = [r for r in recs if r["name"] == "dup"]
    assert [r["ref"] for r in dup] == [names.index("dup_a")] + [names.index("dup_b")] * 2 and dup[2]["index"] - dup[0]["index"] == 2
    assert len({(r["pos"], r["end"]) for r in dup}) == 1 and dup[0]["partners"] == [] and dup[1]["partners"] == [dup[2]]
    assert dup[0]["index"] // G == dup[2]["index"] // G or dup[2]["index"] - (dup[0]["index"] - dup[0]["index"] % G) < W
    # the half-hash collision
    h = [kc.fnv1a(nm) for nm in kc.HALF_COLLISION]
    assert h[0] != h[1] and h[0] & 0xFFFFFFFF == h[1] & 0xFFFFFFFF and h[0] >> 32 != h[1] >> 32
    assert kc.fnv1a("") == 14695981039346656037 and kc.fnv1a("a") == 0xAF63DC4C8601EC8C        # FNV-1a's published vectors
    four = [r for r in recs if r["name"] in kc.HALF_COLLISION]
    assert len(four) == 4 and [r["name"] for r in four] == list(kc.HALF_COLLISION) * 2
    assert max(r["pos"] for r in four) < min(r["end"] for r in four) and all(len(r["partners"]) == 1 for r in four)
    chain = [r for r in recs if r["name"] == kc.CHAIN_NAME]
    assert len(chain) == kc.CHAIN_LENGTH == 300 and not any(r["partners"] for r in chain)
    assert len({r["pos"] for r in chain}) == 300 and {r["end"] - r["pos"] for r in chain} == {1}
    among = [r for r in recs if r["ref"] == names.index("chain") and r["name"] != kc.CHAIN_NAME]
    assert len(among) == 2 and among[0]["partners"] == [among[1]] and chain[0]["index"] < among[0]["index"] < among[1]["index"] < chain[-1]["index"]


def intervals(a):
    cuts = {a["pos"], a["end"]}
    for p in a["partners"]:
        cuts.update(x for x in (p["pos"], p["end"]) if a["pos"] < x < a["end"])
    return len(cuts) - 1


@pytest.mark.parametrize("n_samples", [1, 2])
def test_the_partner_lists_stay_inside_what_is_supported(n_samples):
    T = kc.tile_positions(n_samples)
    refs, records, groups = kc.partner_lists(n_samples)
    recs = link(describe(records))
    assert max(len(r["partners"]) for r in recs) == 3
    by_name = {}
    for r in recs:
        by_name.setdefault(r["name"], []).append(r)
    assert all(len({r["group"] for r in g}) == 1 for g in by_name.values())
    assert n_samples == 1 or {g[0]["group"] for g in by_name.values()} == {g for g, _ in groups}
    for g in by_name.values():      # never four records of a name over one column
        depth = {}
        for r in g:
            for p in range(r["pos"], r["end"]):
                depth[p] = depth.get(p, 0) + 1
        assert max(depth.values()) <= 3
    ordered = list(by_name.values())
    shape = {name: g for (name, _), g in zip(kc.PARTNER_GROUPS, ordered)}
    long_one = lambda g: max(g, key=lambda r: r["end"] - r["pos"])
    for name in ("nested", "touching", "at_start", "at_end", "before"):
        a = long_one(shape[name])
        ps = sorted(a["partners"], key=lambda r: r["pos"])
        assert len(ps) == 3 and all(x["end"] <= y["pos"] for x, y in zip(ps, ps[1:])) and all(len(p["partners"]) == 1 for p in ps)
    assert intervals(long_one(shape["nested"])) == 7
    a = long_one(shape["touching"])
    assert intervals(a) == 6 and any(x["end"] == y["pos"] for x in a["partners"] for y in a["partners"])
    a = long_one(shape["at_start"])
    assert any(p["pos"] == a["pos"] and p["index"] > a["index"] for p in a["partners"])
    a = long_one(shape["at_end"])
    assert any(p["end"] == a["end"] for p in a["partners"])
    a = long_one(shape["before"])
    assert any(p["pos"] == a["pos"] and p["index"] < a["index"] for p in a["partners"]) and sum(p["index"] > a["index"] for p in a["partners"]) == 2
    a = long_one(shape["before_two"])
    assert sum(p["index"] < a["index"] for p in a["partners"]) == 2 and sum(p["index"] > a["index"] for p in a["partners"]) == 1
    trio = ordered[len(kc.PARTNER_GROUPS)]
    assert len(trio) == 3 and all(len(r["partners"]) == 2 for r in trio) and all(r["pos"] < trio[0]["pos"] // T * T + T < r["end"] for r in trio)
    refused = {k: link(describe(v[1])) for k, v in kc.partner_refusals().items()}
    a = max(refused["four_partners"], key=lambda r: len(r["partners"]))
    assert len(a["partners"]) == 4 and max_depth([("c", 1024)], refused["four_partners"]) == 2
    assert max_depth([("c", 1024)], refused["four_over_one_column"]) == 4


def test_one_name_in_two_samples():
    files = kc.same_name_two_samples()
    want = {"xyz": ["g0", "g1", "g0"], "xyzw": ["g0", "g1", "g0", "g1"], "xzy": ["g0", "g0", "g1"], "two": ["g0", "g1"]}
    for key, (refs, records, groups) in files.items():
        recs = link(describe(records))
        same = [r for r in recs if r["name"] == recs[0]["name"]]
        assert [r["group"] for r in same] == want[key] and [sm for _, sm in groups] == ["s0", "s1"]
        assert max(r["pos"] for r in same) < min(r["end"] for r in same)            # some column holds them all
        # a record with a partner of its own sample and an overlapping same-name record of the other one: what K7 refuses
        mixed = any(r["partners"] and any(o["group"] != r["group"] and o["pos"] < r["end"] and o["end"] > r["pos"] for o in same) for r in same)
        assert mixed == (key != "two")
        assert sum(bool(r["partners"]) for r in recs if r["name"] != same[0]["name"]) == 2      # the ordinary pair next to them


@pytest.mark.parametrize("builder,args", [(kc.pair_sweep, (2,)), (kc.pair_kinds, ()), (kc.work_list, ()), (kc.partner_lists, (2,))])
def test_written_files_inflate_to_the_records(tmp_path, builder, args):
    from tests import bamgen as bg
    from tests.util import oracle_inflate_all
    refs, records, groups = builder(*args)
    path = str(tmp_path / "x.bam")
    info = bg.write_bam(path, refs, records, read_groups=groups)
    u = bytes(oracle_inflate_all(path))
    assert len(u) == info["stream_len"] and u[info["header_len"]:] == b"".join(records)
    assert struct.unpack_from("<i", u, 4)[0] > 0
