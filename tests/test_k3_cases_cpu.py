"""The premises of tests/test_gpu_k3_edges.py, checked without a GPU: every builder of tests/k3_cases.py still puts its reads on the
boundary its docstring names.  K2's classification of a record (index.hip: `runs == 1 && !other_ref && !zero_ref`) and the rule by
which the second stage of k_accumulate16c queues an item (a run or gap that touches the tile, of a general CIGAR of at most 8
operations) are restated here in plain Python."""
import struct

import numpy as np
import pytest

from tests import bamgen as bg
from tests import k3_cases as kc
from tests.util import oracle_base_counters, oracle_inflate_all

LANE_OPS, RUN_ITEMS, GAP_ITEMS, RUN_BLOCKS, FAST_BLOCKS = 8, 22, 8, 352, 11


def parse(b):
    ref, pos, l_name, mapq, _bin, n_cig, flag, l_seq = struct.unpack_from("<iiBBHHHi", b, 4)
    cig = [struct.unpack_from("<I", b, 36 + l_name + 4 * i)[0] for i in range(n_cig)]
    return {"ref": ref, "pos": pos, "mapq": mapq, "flag": flag, "l_seq": l_seq, "cigar": [(bg.CIGAR_OPS[c & 15], c >> 4) for c in cig]}


def classify(r):
    """(kind, end, q_lead) as K2 describes the record under the default filter: kind 0 dropped, 1 one run of aligned bases, 2 general."""
    if r["flag"] & (0x4 | 0x400 | 0x200) or r["mapq"] == 0:
        return 0, r["pos"], 0
    span = q_lead = runs = 0
    in_run = other_ref = seen_ref = zero_ref = False
    for op, n in r["cigar"]:
        if n == 0 and op in "MDN=X":
            zero_ref = True
        if op in "M=X":
            if not in_run:
                runs, in_run = runs + 1, True
            span += n
            seen_ref = True
        elif op in "DN":
            other_ref, seen_ref, in_run = True, True, False
            span += n
        elif op in "IS":
            if not seen_ref:
                q_lead += n
            else:
                in_run = False
    if span <= 0:
        return 0, r["pos"], 0
    return (1 if runs == 1 and not other_ref and not zero_ref else 2), r["pos"] + span, q_lead


def n_blocks(t0, n):
    return ((t0 + n - 1) >> 4) - (t0 >> 4) + 1


def lane_items(r, ts, te):
    """Run items [(tile offset, bases)] and gap items a lane queues for a kind-2 record of at most LANE_OPS operations."""
    kind, end, _ = classify(r)
    if kind != 2 or len(r["cigar"]) > LANE_OPS or not (r["pos"] < te and end > ts):
        return [], []
    runs, gaps, rp = [], [], r["pos"]
    for op, n in r["cigar"]:
        if op in "MDN=X":
            n = min(max(n, 1), max(end - rp, 0))
            c0, c1 = max(ts - rp, 0), min(n, max(te - rp, 0))
            if c1 > c0:
                (runs if op in "M=X" else gaps).append((rp + c0 - ts, c1 - c0))
            rp += n
            if rp >= te or rp >= end:
                break
    return runs, gaps


def by_contig(records, ref):
    return [r for r in map(parse, records) if r["ref"] == ref]


def tile_range(recs, ts, te):
    hit = [i for i, r in enumerate(recs) if classify(r)[0] and r["pos"] < te and classify(r)[1] > ts]
    return (hit[0], hit[-1] + 1) if hit else (0, 0)


def window_counts(recs, ts, te):
    """(run items, gap items, run blocks) of every window of 64 consecutive records, any phase."""
    per = [lane_items(r, ts, te) for r in recs]
    out = set()
    for a in range(len(recs) - 63):
        runs = [x for p in per[a:a + 64] for x in p[0]]
        out.add((len(runs), sum(len(p[1]) for p in per[a:a + 64]), sum(n_blocks(*x) for x in runs)))
    return out


@pytest.mark.parametrize("n_samples", [1, 2, 3])
def test_every_window_of_64_records_fills_the_queues_as_designed(n_samples):
    T = kc.tile_positions(n_samples)
    refs, records, groups = kc.queue_periods(n_samples)
    assert len(groups) == (n_samples if n_samples > 1 else 0)
    names = [n for n, _ in refs]
    assert all(ln == T for _, ln in refs)
    for name, (_, want_runs, want_gaps) in kc.PERIODS.items():
        recs = by_contig(records, names.index(name))
        assert len(recs) % 256 == 0 and tile_range(recs, 0, T)[0] == 0 and max(classify(r)[1] for r in recs) <= T
        assert all(a["pos"] <= b["pos"] for a, b in zip(recs, recs[1:]))
        got = window_counts(recs, 0, T)
        assert {g[:2] for g in got} == {(want_runs, want_gaps)}, name
        assert all(g[2] <= RUN_BLOCKS for g in got)
        kinds = [classify(r)[0] for r in recs[:64]]
        assert kinds.count(0) >= 8 and kinds.count(1) >= 8          # dropped and single-run lanes between the others
    assert kc.PERIODS["a_full"][1:] == (RUN_ITEMS, GAP_ITEMS) and kc.PERIODS["b_runs23"][1:] == (RUN_ITEMS + 1, GAP_ITEMS)
    assert kc.PERIODS["c_gaps9"][1:] == (RUN_ITEMS, GAP_ITEMS + 1)
    if n_samples > 1:
        return
    for name, want in (("d_blocks352", (RUN_ITEMS, GAP_ITEMS, RUN_BLOCKS)), ("e_blocks353", (RUN_ITEMS, GAP_ITEMS, RUN_BLOCKS + 1))):
        recs = by_contig(records, names.index(name))
        assert len(recs) % 256 == 0 and max(classify(r)[1] for r in recs) <= T
        assert window_counts(recs, 0, T) == {want}, name
        blocks = [n_blocks(*x) for r in recs[:64] for x in lane_items(r, 0, T)[0]]
        assert sorted(blocks) == [16] * 21 + [16 if name[0] == "d" else 17]
    for name, n_items, n_gaps, n_runs in (("g_outside", RUN_ITEMS, 4, 35), ("g_outside23", RUN_ITEMS + 1, 5, 37)):
        recs = by_contig(records, names.index(name))
        for ts in (0, T):           # the contig's tile and the spare tile behind it
            assert {g[:2] for g in window_counts(recs, ts, ts + T)} == {(n_items, n_gaps)}, (name, ts)
        all_runs = sum(1 for r in recs[:64] if classify(r)[0] == 2 for k, (op, n) in enumerate(r["cigar"]) if op == "M")
        assert all_runs == n_runs > n_items


def test_cigars_of_eight_and_nine_operations_share_a_batch():
    refs, records, _ = kc.queue_periods(1)
    recs = by_contig(records, [n for n, _ in refs].index("f_ops8_9"))
    for a in range(len(recs) - 63):
        ops = [len(r["cigar"]) for r in recs[a:a + 64] if classify(r)[0] == 2]
        assert ops.count(LANE_OPS) == 4 and ops.count(LANE_OPS + 1) == 4
    for name in ("b_runs23", "c_gaps9"):
        recs = by_contig(records, [n for n, _ in refs].index(name))
        assert sum(1 for r in recs[:64] if len(r["cigar"]) == LANE_OPS + 1) == 2


@pytest.mark.parametrize("n_samples", [1, 2, 3])
def test_the_sweep_has_every_cell_and_stays_shallow(n_samples):
    T = kc.tile_positions(n_samples)
    refs, records, _ = kc.alignment_sweep(n_samples)
    names = [n for n, _ in refs]
    cells, edges, codes = set(), {}, set()
    for ref, (name, ln) in enumerate(refs):
        if not name.startswith("in"):
            continue
        assert ln == T
        depth = np.zeros(T, dtype=int)
        for r in by_contig(records, ref):
            kind, end, q_lead = classify(r)
            assert kind == 1 and end <= T
            n = end - r["pos"]
            depth[r["pos"]:end] += 1
            if n in kc.SWEEP_LENGTHS:
                cells.add((r["pos"] & 15, q_lead & 1, n))
            else:
                edges[(r["pos"] & 15, q_lead & 1, n)] = n_blocks(r["pos"], n)
        assert depth.max() <= kc.SWEEP_MAX_DEPTH
    assert cells == {(o, p, n) for o in range(16) for p in (0, 1) for n in kc.SWEEP_LENGTHS}
    assert {(o, p, n % 16) for o, p, n in cells} == {(o, p, m) for o in range(16) for p in (0, 1) for m in range(16)}
    assert set(edges) == {(o, p, n) for o in kc.BLOCK_EDGE_OFFSETS for p in (0, 1) for n in kc.BLOCK_EDGE_LENGTHS}
    for p in (0, 1):
        assert (edges[(15, p, 161)], edges[(15, p, 162)]) == (FAST_BLOCKS, FAST_BLOCKS + 1)
        assert (edges[(0, p, 176)], edges[(0, p, 177)]) == (FAST_BLOCKS, FAST_BLOCKS + 1)
    # tile borders: the part in the tile behind the border starts at query base q_lead + d, the part before it ends the tile
    recs = by_contig(records, names.index("edge"))
    starts, ends = set(), set()
    per_border = {}
    for r in recs:
        kind, end, q_lead = classify(r)
        b = (r["pos"] // T + 1) * T
        assert kind == 1 and r["pos"] < b < end <= b + T
        d, m = b - r["pos"], end - b
        per_border[b] = per_border.get(b, 0) + 1
        starts.add((d, (q_lead + d) & 1, m))
        ends.add(((T - d) & 15, q_lead & 1, d))
    assert max(per_border.values()) <= kc.SWEEP_MAX_DEPTH and refs[names.index("edge")][1] == max(per_border) + T
    assert starts >= {(d, p, m) for d in range(1, 18) for p in (0, 1) for m in kc.SWEEP_LENGTHS}
    assert {(o, p, d % 16) for o, p, d in ends} >= {((T - d) & 15, p, d % 16) for d in range(1, 34) for p in (0, 1)}
    # the span steps: a read over every quarter border of the tile, uncovered positions behind each
    depth = np.zeros(T, dtype=int)
    for r in by_contig(records, names.index("steps")):
        depth[r["pos"]:classify(r)[1]] += 1
    for q in (1, 2, 3):
        assert depth[q * T // 4 - 1] == depth[q * T // 4] == 1 and depth[q * T // 4 + T // 8] == 0
    assert depth[0] == depth[T - 1] == 1
    full = by_contig(records, names.index("full"))
    assert [(r["pos"], classify(r)[1]) for r in full] == [(0, T)]
    for b in records:
        r = parse(b)
        o = 36 + b[12] + 4 * len(r["cigar"])
        codes.update(x >> 4 for x in b[o:o + r["l_seq"] // 2])
    assert codes == set(range(16))


def test_the_zoo_reads_are_walked_where_the_docstring_says():
    refs, records, _ = kc.zero_length_zoo()
    want_short = {s for s in kc.ZERO_SHAPES}
    want_long = {kc.zero_ninth(s) for s in kc.ZERO_SHAPES}
    for ref, (name, ln) in enumerate(refs):
        recs = by_contig(records, ref)
        assert all(a["pos"] <= b["pos"] for a, b in zip(recs, recs[1:]))
        seen = set()
        for r in recs:
            text = "".join("%d%s" % (n, op) for op, n in r["cigar"])
            zero = [k for k, (op, n) in enumerate(r["cigar"]) if n == 0]
            if zero:
                assert classify(r)[0] == 2 and r["cigar"][zero[0]][0] in "MDN="
                assert (len(r["cigar"]) <= LANE_OPS) if text in want_short else (zero[0] == LANE_OPS and text in want_long)
                seen.add(text)
            else:
                assert classify(r)[0] == 1
        assert seen == want_short | want_long
        for ts in range(0, ln, 1024):
            assert all(g[0] <= RUN_ITEMS and g[1] <= GAP_ITEMS and g[2] <= RUN_BLOCKS for g in window_counts(recs, ts, ts + 1024))
    edge = [r for r in by_contig(records, 1) if any(n == 0 for _, n in r["cigar"])]
    assert {r["pos"] for r in edge} == {1013, 1014, 1015, 1024}


@pytest.fixture(scope="module")
def stack_files(tmp_path_factory):
    d = tmp_path_factory.mktemp("k3stacks")
    out = {}
    for name, builder in (("stacks", kc.stacks), ("deep", kc.stacks_deep)):
        refs, records, groups = builder()
        path = str(d / (name + ".bam"))
        bg.write_bam(path, refs, records, read_groups=groups)
        out[name] = (path, refs, records)
    return out


def _records_per_tile(refs, records):
    n = {}
    for b in set(records):
        r = parse(b)
        kind, end, _ = classify(r)
        assert kind != 0
        for t in range(r["pos"] // 1024, (end - 1) // 1024 + 1):
            n[(refs[r["ref"]][0], t)] = n.get((refs[r["ref"]][0], t), 0) + records.count(b)
    return n


def test_the_stacks_hold_one_record_fewer_than_the_limit(stack_files):
    path, refs, records = stack_files["stacks"]
    assert _records_per_tile(refs, records) == {(name, 0): 65535 for name, _ in refs}
    assert kc.STACK_DEPTH == 65535 == 2 ** 16 - 1
    for ref, (name, code) in enumerate((("all_A", 0), ("all_C", 1), ("all_DEL", 5), ("all_SKIP", 6))):
        assert refs[ref] == (name, 1024)
        c = oracle_base_counters(path, ref, kc.STACK_POS - 8, kc.STACK_POS + 8)[:, 0, :]
        assert c[8, code] == 65535 and c[8].sum() == 65535
        assert c[7].sum() > 0 and c[9].sum() > 0 and c.max(axis=1)[[7, 9]].max() < 65535      # neighbours neither empty nor stacked


def test_the_deep_tiles_hold_exactly_the_limit(stack_files):
    path, refs, records = stack_files["deep"]
    assert _records_per_tile(refs, records) == {("deep", 0): 65536, ("deep_next_to_shallow", 0): 8, ("deep_next_to_shallow", 1): 65536}
    assert oracle_base_counters(path, 0, kc.STACK_POS, kc.STACK_POS + 1)[0, 0, 0] == 65536
    assert oracle_base_counters(path, 1, 1024 + kc.STACK_POS, 1025 + kc.STACK_POS)[0, 0, 1] == 65536


@pytest.mark.parametrize("builder,args", [(kc.alignment_sweep, (1,)), (kc.alignment_sweep, (3,)), (kc.queue_periods, (1,)),
                                          (kc.queue_periods, (2,)), (kc.zero_length_zoo, ()), (kc.stacks, ())])
def test_written_files_inflate_to_the_records(tmp_path, builder, args):
    refs, records, groups = builder(*args)
    path = str(tmp_path / "x.bam")
    info = bg.write_bam(path, refs, records, read_groups=groups)
    u = bytes(oracle_inflate_all(path))
    assert len(u) == info["stream_len"] and u[info["header_len"]:] == b"".join(records)
    assert u[:4] == b"BAM\x01" and all(("SM:" + sm).encode() in u[:info["header_len"]] for _, sm in groups)
