"""The premises of tests/test_gpu_k5_edges.py, checked without a GPU.
* The restatement of reduce.hip's closed forms (tests/k5_ref.py) gives, for every command line of every case of tests/k5_cases.py,
  the text the oracle prints: a disagreement is a mistake in the case or in the restatement and is settled here.
* Every case is where it claims to be: which records share a window and a wavefront, which lanes a run begins and ends in, which
  tile and chunk a range edge falls in, which depth a threshold meets.
* A Python model of k_count_reads_windows with its add_runs (leader / ballot / run length) issues, wavefront by wavefront, atomics
  that add up to the restatement's n_reads; each of five single-defect variants of add_runs gets a named `runs_*` case wrong, in
  whichever lane the file begins."""
import numpy as np
import pytest

from tests import bamgen as bg
from tests import k5_cases as kc
from tests import k5_ref as kr
from tests.util import run_oracle

WAVE = 64


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    """name -> (case, BAM path, BED path or None), written once."""
    d = tmp_path_factory.mktemp("k5cpu")
    made = {}

    def get(name):
        if name not in made:
            c = kc.case(name)
            path = str(d / (name + ".bam"))
            bg.write_bam(path, c.refs, c.records, read_groups=c.read_groups)
            bed = None
            if c.bed:
                bed = str(d / (name + ".bed"))
                with open(bed, "w") as fh:
                    fh.write(c.bed_text())
            made[name] = (c, path, bed)
        return made[name]
    return get


_restated = {}


def restated(name, min_bq=0, combined=False):
    if (name, min_bq, combined) not in _restated:
        _restated[name, min_bq, combined] = kr.Restatement(kc.case(name), min_bq, combined)
    return _restated[name, min_bq, combined]


def options_of(args):
    return int(args[args.index("-q") + 1]) if "-q" in args else 0, "--combined" in args


def same_text(got, want, what):
    if got != want:
        gl, wl = got.decode().splitlines(), want.decode().splitlines()
        k = next((i for i in range(min(len(gl), len(wl))) if gl[i] != wl[i]), min(len(gl), len(wl)))
        raise AssertionError("%s: %d vs %d lines, the first difference at line %d:\n  restated: %r\n  oracle:   %r" % (
            what, len(gl), len(wl), k, gl[k] if k < len(gl) else None, wl[k] if k < len(wl) else None))


@pytest.mark.parametrize("name", kc.ALL_NAMES)
def test_the_restatement_prints_what_the_oracle_prints(files, name):
    c, path, bed = files(name)
    assert c.limit and (c.windows or c.bed or c.overlaps)
    parsed = [kr.parse(b) for b in c.records]
    assert all((a["ref"], a["pos"]) <= (b["ref"], b["pos"]) for a, b in zip(parsed, parsed[1:])), "records out of order"
    assert len(c.records) <= 5000 and max(ln for _, ln in c.refs) <= 40000
    for args in c.cli_lines(bed):
        q, combined = options_of(args)
        rs = restated(name, q, combined)
        if args[0] == "window":
            got = kr.format_window(c, rs, int(args[2]), c.thresholds, combined)
        else:
            got = kr.format_region(c, rs, c.thresholds, combined)
        same_text(got, run_oracle(args + [path]), "%s: %s" % (name, " ".join(args)))


# ---- k_count_reads_windows and add_runs, modelled -------------------------------------------------------------------------
def lanes_of(c, min_bq, w):
    """What every record of the file brings to its lane: (admitted, on0, slot0, straddles, on1, slot1, [slots of further windows])
    -- the expressions of k_count_reads_windows."""
    S = c.n_samples
    groups = [g for g, _ in c.read_groups]
    with_reads = {r["ref"] for r in map(kr.parse, c.records) if kr.admitted(r)}
    n_win = [ln // w if ref in with_reads else 0 for ref, (_, ln) in enumerate(c.refs)]
    base = [sum(n_win[:ref]) for ref in range(len(c.refs))]
    out = []
    for b in c.records:
        r = kr.parse(b, groups)
        s = r["sample"] if S > 1 else 0
        if not kr.admitted(r):
            out.append((False, False, s, False, False, S + s, []))
            continue
        good = {p // w for p, q in kr.bases_as_written(r) if q >= min_bq}
        k0, k1 = r["pos"] // w, (r["pos"] + kr.span(r) - 1) // w
        nw, wb = n_win[r["ref"]], base[r["ref"]]
        more = [(wb + k) * S + s for k in range(k0 + 2, min(k1, nw - 1) + 1) if k in good]
        out.append((True, k0 < nw and k0 in good, (wb + k0) * S + s, k1 > k0, k1 > k0 and k0 + 1 < nw and k0 + 1 in good,
                    (wb + k0 + 1) * S + s, more))
    return out, sum(n_win) * S


DEFECTS = ("leader_without_prev_on", "stop_without_inactive", "above_off_by_one", "lane63_never_ends", "lane0_never_leads")


def add_runs(on, slot, counters, defect=None):
    """One wavefront: on[64], slot[64] -> the atomics its leaders issue, added into `counters`.  Returns the leaders."""
    lead = []
    for lane in range(WAVE):
        prev_on, prev = (on[lane - 1], slot[lane - 1]) if lane else (on[0], slot[0])       # __shfl_up: lane 0 keeps its own
        first = lane == 0 and defect != "lane0_never_leads"
        if defect == "leader_without_prev_on":
            lead.append(on[lane] and (first or prev != slot[lane]))
        else:
            lead.append(on[lane] and (first or not prev_on or prev != slot[lane]))
    for lane in range(WAVE):
        if not lead[lane]:
            continue
        above = range(lane + (2 if defect == "above_off_by_one" else 1), WAVE)
        stop = [l for l in above if lead[l] or (not on[l] and defect != "stop_without_inactive")]
        end = stop[0] if stop else (WAVE - 1 if defect == "lane63_never_ends" else WAVE)
        counters[slot[lane]] += end - lane
    return lead


def model_n_reads(lanes, n_slots, phase=0, defect=None):
    """n_reads as the kernel's atomics leave it, the file begun in lane `phase` (dead lanes in front)."""
    dead = (False, False, 0, False, False, 0, [])
    rows = [dead] * phase + list(lanes)
    rows += [dead] * (-len(rows) % WAVE)
    counters = np.zeros(n_slots + 8, dtype=np.int64)
    for a in range(0, len(rows), WAVE):
        wave = rows[a:a + WAVE]
        add_runs([x[1] for x in wave], [x[2] for x in wave], counters, defect)
        if any(x[0] and x[3] for x in wave):
            add_runs([x[4] for x in wave], [x[5] for x in wave], counters, defect)
        for x in wave:
            for slot in x[6]:
                counters[slot] += 1
    return counters[:n_slots]


def restated_n_reads(name, min_bq, w):
    c, rs = kc.case(name), restated(name, min_bq)
    with_reads = {r["ref"] for r in rs.reads}
    ranges = [g for ref in range(len(c.refs)) if ref in with_reads for g in rs.windows(ref, w)]
    return rs.stats(ranges)[0].reshape(-1)


WINDOW_RUNS = [(n, q, w) for n in kc.ALL_NAMES for q in kc.case(n).min_bqs for w in kc.case(n).windows]


@pytest.mark.parametrize("name,min_bq,w", WINDOW_RUNS, ids=["%s-q%d-w%d" % x for x in WINDOW_RUNS])
def test_the_model_of_the_window_kernel_adds_up_to_the_restatement(name, min_bq, w):
    lanes, n_slots = lanes_of(kc.case(name), min_bq, w)
    want = restated_n_reads(name, min_bq, w)
    assert len(want) == n_slots
    for phase in range(WAVE) if name in kc.RUNS_NAMES else (0,):
        assert np.array_equal(model_n_reads(lanes, n_slots, phase), want), phase


@pytest.mark.parametrize("defect", DEFECTS)
def test_every_defect_of_add_runs_is_caught_by_a_named_case(defect):
    """... whichever lane the file begins in: the designs do not depend on which record lands in lane 0."""
    caught = []
    for name in kc.RUNS_NAMES:
        c = kc.case(name)
        q, w = c.min_bqs[-1], c.windows[0]
        lanes, n_slots = lanes_of(c, q, w)
        want = restated_n_reads(name, q, w)
        wrong = [not np.array_equal(model_n_reads(lanes, n_slots, phase, defect), want) for phase in range(WAVE)]
        if all(wrong):
            caught.append(name)
    expected = {"leader_without_prev_on": "runs_interrupted", "stop_without_inactive": "runs_interrupted",
                "above_off_by_one": "runs_every_lane", "lane63_never_ends": "runs_all64", "lane0_never_leads": "runs_all64"}
    assert expected[defect] in caught, (defect, caught)


def waves(lanes):
    rows = list(lanes) + [(False, False, 0, False, False, 0, [])] * (-len(lanes) % WAVE)
    return [rows[a:a + WAVE] for a in range(0, len(rows), WAVE)]


def run_edges(lanes):
    """(lanes in which a run begins, lanes in which one ends, the longest run) over the first-window pass of the file."""
    begins, ends, longest = set(), set(), 0
    for wave in waves(lanes):
        on, slot = [x[1] for x in wave], [x[2] for x in wave]
        lead = add_runs(on, slot, np.zeros(max(slot) + 1, dtype=np.int64))
        for lane in range(WAVE):
            if lead[lane]:
                end = next((l for l in range(lane + 1, WAVE) if lead[l] or not on[l]), WAVE)
                begins.add(lane)
                ends.add(end - 1)
                longest = max(longest, end - lane)
    return begins, ends, longest


def test_the_runs_cases_are_where_they_claim_to_be():
    every = set(range(WAVE))
    lanes, _ = lanes_of(kc.case("runs_all64"), 0, kc.RUN_W)
    begins, ends, longest = run_edges(lanes)
    assert begins == every and ends == every and longest == WAVE          # a full wavefront; a run ending at 63; one begun at lane 0 ...
    ws = waves(lanes)
    assert any(a[63][1] and b[0][1] and a[63][2] == b[0][2] for a, b in zip(ws, ws[1:]))      # ... that goes on from the wave before
    # interrupted: with -q 20 a lane that is admitted but not on lies between two on lanes of the SAME slot, in every lane 1..62;
    # an unmapped record (not admitted) does too; and a run begins behind / ends in front of such a lane
    c = kc.case("runs_interrupted")
    lanes, _ = lanes_of(c, kc.MIN_BQ, kc.RUN_W)
    inside_low, inside_unm = set(), set()
    for wave in waves(lanes):
        for l in range(1, WAVE - 1):
            a, x, b = wave[l - 1], wave[l], wave[l + 1]
            if a[1] and b[1] and not x[1] and a[2] == b[2]:
                (inside_low if x[0] and x[2] == a[2] else inside_unm).add(l)
    assert inside_low == set(range(1, WAVE - 1)) and inside_unm == set(range(1, WAVE - 1))
    lanes0, _ = lanes_of(c, 0, kc.RUN_W)
    assert sum(x[1] for x in lanes0) > sum(x[1] for x in lanes)           # -q 0 turns the low reads on: plain runs
    # every lane a leader
    for name in ("runs_every_lane", "runs_samples2", "runs_samples3"):
        c = kc.case(name)
        lanes, _ = lanes_of(c, 0, c.windows[0])
        assert run_edges(lanes)[2] == 1 and all(x[1] for x in lanes), name
    slots = [x[2] for x in lanes_of(kc.case("runs_samples3"), 0, kc.RUN_W)[0][:6]]
    assert slots == [0, 1, 2, 0, 1, 2]
    # A B A
    lanes, _ = lanes_of(kc.case("runs_aba"), 0, kc.RUN_W)
    assert [x[2] for x in lanes[:len(kc.ABA)]] == [0, 0, 0, 1, 1, 0, 0, 1, 0, 1, 1, 1, 0, 0]
    assert run_edges(lanes)[0] == every
    # 64 k + 1 records: a last wavefront with one live lane
    assert len(kc.case("runs_tail").records) == 4 * WAVE + 1
    assert all(len(kc.case(n).records) % WAVE == 1 for n in ("runs_every_lane", "runs_samples2", "runs_samples3", "runs_tail"))
    assert run_edges(lanes_of(kc.case("runs_tail"), 0, kc.RUN_W)[0])[2] == 40


def straddlers(name, min_bq, w):
    """(k0, k1, nw, on0, on1, further windows counted) of the admitted records of a one-contig case."""
    c = kc.case(name)
    nw = c.refs[0][1] // w
    out = []
    for b, x in zip(c.records, lanes_of(c, min_bq, w)[0]):
        r = kr.parse(b)
        if x[0]:
            out.append((r["pos"] // w, (r["pos"] + kr.span(r) - 1) // w, nw, x[1], x[4], len(x[6])))
    return out


def test_the_straddle_cases_are_where_they_claim_to_be():
    W, q = kc.STR_W, kc.MIN_BQ
    two = lambda name: {(on0, on1) for k0, k1, nw, on0, on1, _ in straddlers(name, q, W) if k1 == k0 + 1 and k1 < nw}
    assert (True, False) in two("straddle_left_only") and (True, True) in two("straddle_left_only")
    assert (False, True) in two("straddle_right_only")
    assert (False, False) in two("straddle_neither") and (True, True) in two("straddle_neither")
    for name, op in (("straddle_deletion", "D"), ("straddle_skip", "N")):
        assert two(name) >= {(True, True), (True, False), (False, True)}, name
        over = 0
        for r in map(kr.parse, kc.case(name).records):
            rp = r["pos"]
            for o, n in r["cigar"]:
                over += o == op and rp // W != (rp + n - 1) // W          # the gap itself lies on both sides of a window edge
                rp += n if o in kr.REF_OPS else 0
        assert over >= 3, name
    assert any(r["cigar"] == [("M", 4), ("D", 4), ("M", 6)] and (r["pos"] + 8) % W == 0 for r in map(kr.parse, kc.case("straddle_deletion").records))
    # the loop over k0 + 2 ..: three windows of 20, five of 16; counted in a further window alone; cut short by nw
    assert {k1 - k0 for k0, k1, *_ in straddlers("straddle_span3", q, 20)} >= {2}
    assert any(k1 - k0 == 2 and not on0 and not on1 and more == 1 for k0, k1, _, on0, on1, more in straddlers("straddle_span3", q, 20))
    s5 = straddlers("straddle_span5", q, W)
    assert any(k1 - k0 == 4 and not on0 and not on1 and more == 1 for k0, k1, _, on0, on1, more in s5)
    assert any(k1 - k0 == 4 and more == 3 for k0, k1, _, on0, on1, more in straddlers("straddle_span5", 0, W))
    assert any(k1 >= nw and k1 - k0 >= 2 and k0 + 2 < nw for k0, k1, nw, *_ in s5)
    assert all(any(k1 >= k0 + 2 for k0, k1, *_ in straddlers(n, q, w)) for n in ("straddle_span3", "straddle_span5") for w in (W, 20))
    part = straddlers("straddle_into_partial", q, W)
    assert sum(k0 + 1 == nw and k1 == nw for k0, k1, nw, *_ in part) == 3
    assert {(on0, on1) for k0, k1, nw, on0, on1, _ in part if k1 == nw} == {(True, False), (False, False)}
    assert sum(k0 >= nw for k0, k1, nw, *_ in straddlers("straddle_in_partial", 0, W)) == 3
    assert kc.STR_LEN % W and kc.STR_LEN % 20


def chunks_of(a, b):
    return [(p, min(b, p + kc.CHUNK)) for p in range(a, b, kc.CHUNK)]


@pytest.mark.parametrize("n_samples", [1, 2, 3])
def test_the_range_lengths_sit_on_the_stride_the_tile_and_the_chunk(n_samples):
    c = kc.case("ranges_lengths%d" % n_samples)
    T = kc.tile_positions(n_samples)
    assert T == {1: 1024, 2: 512, 3: 256}[n_samples] and kc.CHUNK == 16384
    want = set(kc.range_lengths(T))
    assert {b - a for _, a, b in c.bed} == want and set(c.windows) == want - {1}
    L = c.refs[0][1]
    assert all(2 * w < L < 2 * w + 2 * 64 + 100 for w in (max(c.windows),)) and all(b <= L for _, a, b in c.bed)
    for n in want:
        lines = [(a, b) for _, a, b in c.bed if b - a == n]
        assert any(a // T != (b - 1) // T for a, b in lines) or n == 1, n             # across a tile edge
        assert any(a // T == (b - 1) // T for a, b in lines) or n >= T, n             # and inside one tile
        assert {len(chunks_of(a, b)) for a, b in lines} == {2 if n > kc.CHUNK else 1}
    assert any(b - a == 1 and (a + 1) % T == 0 for _, a, b in c.bed) and any(a % T == 0 and b % T == 0 and b - a == T for _, a, b in c.bed)
    assert [hi - lo for lo, hi in chunks_of(5, 5 + kc.CHUNK + 1)] == [kc.CHUNK, 1]    # the second wavefront of an id adds one position
    rs = restated(c.name, kc.MIN_BQ)
    n_reads, n_bases, cov, seen = rs.stats(c.bed, c.thresholds)
    longer = np.array([b - a > 1 for _, a, b in c.bed])
    assert (n_bases.sum(axis=1) > 0)[longer].all() and seen.all() and (cov[:, :, 0].sum(axis=1) > 0)[longer].all()
    assert (rs.cov[0] != rs.good[0]).any()                                            # deletions, skips: depth is not bases counted


def active_tiles(name, ref, T):
    rs = restated(name)
    return {t for r in rs.reads if r["ref"] == ref for t in range(r["pos"] // T, (r["pos"] + kr.span(r) - 1) // T + 1)}


def test_the_other_ranges_cases_are_where_they_claim_to_be():
    for S in (1, 2):
        c = kc.case("ranges_inactive_tile%d" % S)
        T = kc.tile_positions(S)
        assert active_tiles(c.name, 0, T) == {0, 2, 4} and c.refs[0][1] == 5 * T
        tiles = [set(range(a // T, (b - 1) // T + 1)) for _, a, b in c.bed]
        assert {0, 1, 2} in tiles and {1} in tiles and {0, 1, 2, 3, 4} in tiles and {2, 3, 4} in tiles
        assert c.windows == (T, 3 * T // 2, 5 * T // 2)      # window 1 of T: an inactive tile alone; window 0 of 5T/2: active, inactive, active
    c = kc.case("ranges_overhang")
    T = kc.tile_positions(1)
    ln0 = c.refs[0][1]
    tiles0 = (ln0 + T - 1) // T
    rs = restated(c.name)
    assert max(r["pos"] + kr.span(r) for r in rs.reads if r["ref"] == 0) == ln0           # nothing of c0 hangs over its end
    over = [(a, b) for ref, a, b in c.bed if ref == 0 and b > ln0]
    assert any(b > tiles0 * T + 64 and a < ln0 for a, b in over) and any(a >= tiles0 * T for a, b in over)
    assert rs.col[1][:64].all() and rs.cov[1][0, 0] >= 6                                   # c1 is covered from position 0
    n_reads, n_bases, cov, seen = rs.stats(c.bed, c.thresholds)
    k = c.bed.index((0, tiles0 * T, tiles0 * T + 64))
    assert n_bases[k, 0] == 0 and not seen[k] and n_bases[c.bed.index((1, 0, 64)), 0] > 0
    c = kc.case("ranges_zero_window_contigs")
    rs = restated(c.name)
    with_reads = {r["ref"] for r in rs.reads}
    for w in c.windows:
        n_win = [ln // w if ref in with_reads else 0 for ref, (_, ln) in enumerate(c.refs)]
        assert [n > 0 for n in n_win] == [False, True, False, False, True, False]
        assert c.refs[3][1] // w > 0 and 3 not in with_reads and {0, 2, 5} <= with_reads


@pytest.mark.parametrize("n_samples", [1, 2, 3])
def test_the_thresholds_meet_the_depths_they_name(n_samples):
    c = kc.case("thresholds_stacks%d" % n_samples)
    rs = restated(c.name)
    assert len(c.thresholds) == kc.MAX_THRESHOLDS == 16
    for i, d in enumerate(kc.STACK_DEPTHS):
        at = kc.STACK_AT[d]
        depth = rs.cov[0][:, at:at + 5]
        assert (depth[i % n_samples] == d).all() and depth.sum() == 5 * d and rs.cov[0][:, at - 1].sum() == 0 == rs.cov[0][:, at + 5].sum()
        assert {d, d + 1} <= set(c.thresholds) and (d - 1 in c.thresholds or d == 1)
    assert len(set(c.thresholds)) < len(c.thresholds) and {65535, 65536} <= set(c.thresholds) and 0 not in c.thresholds
    cov = rs.stats([(0, 0, 400)], c.thresholds)[2][0]
    for t, thr in enumerate(c.thresholds):
        assert cov[:, t].sum() == 5 * sum(d >= thr for d in kc.STACK_DEPTHS)
    assert kc.case("thresholds_none").thresholds == () and len(kc.case("thresholds_one").thresholds) == 1
    assert kc.case("thresholds_one").thresholds[0] in kc.STACK_DEPTHS


def test_the_stack_of_300_has_depths_that_are_not_bases_counted():
    c = kc.case("thresholds_stack300")
    for q, depths in ((0, [300] * 8), (kc.MIN_BQ, [240] * 3 + [180, 180] + [240] * 3)):
        rs = restated(c.name, q)
        assert list(rs.cov[0][0, 100:108]) == depths
        assert list(rs.good[0][0, 103:105]) == ([180, 180] if q == 0 else [60, 60])     # D and N: in the depth, not in the bases
        assert {d - 1 for d in depths} | set(depths) | {d + 1 for d in depths} <= set(c.thresholds) | {239}


def test_the_regions_cases_are_where_they_claim_to_be():
    c = kc.case("regions_long_then_short")
    reads = restated(c.name).reads
    srt = sorted(c.bed, key=lambda g: g[1])
    first, last_end = min(r["pos"] for r in reads), max(r["pos"] + kr.span(r) for r in reads)
    below = [g for g in srt if g[1] < last_end]
    assert below[0] == (0, 0, 15000) and sum(g[2] <= first for g in below[1:]) == 200 > WAVE
    c = kc.case("regions_duplicates")
    assert c.bed.count((0, 505, 520)) == 3 and c.bed.count((0, 400, 600)) == 2 and list(c.bed) != sorted(c.bed)
    n_reads = restated(c.name).stats(c.bed)[0][:, 0]
    assert n_reads[0] == n_reads[2] == n_reads[3] > 0
    c = kc.case("regions_touching")
    r = restated(c.name).reads[0]
    a, b = r["pos"], r["pos"] + kr.span(r)
    assert {(0, a - 20, a), (0, a - 20, a + 1), (0, b, b + 10), (0, b - 1, b + 10)} <= set(c.bed)
    n_reads, n_bases, _, seen = restated(c.name).stats(c.bed + c.api_ranges)
    assert [int(x) for x in n_reads[:4, 0]] == [0, 1, 0, 1] and list(seen[:4]) == [0, 1, 0, 1]
    k = c.bed.index((0, 710, 715))
    assert n_reads[k, 0] == 0 and seen[k] == 1                                     # inside the deletion: a column, no base
    assert all(s >= e for _, s, e in c.api_ranges) and not n_reads[len(c.bed):].any() and not seen[len(c.bed):].any()
    c = kc.case("regions_many_over_one_read")
    r = restated(c.name).reads[0]
    assert sum(g[1] < r["pos"] + kr.span(r) and g[2] > r["pos"] for g in c.bed) == 125 > WAVE
    c = kc.case("regions_contig_mismatch")
    with_reads, with_regions = {r["ref"] for r in restated(c.name).reads}, {g[0] for g in c.bed}
    assert with_reads == {0, 2, 3} and with_regions == {1, 2, 4}
    c = kc.case("regions_first_ring")
    assert c.overlaps and all(0 < o < w for w, o in c.overlaps) and not c.windows and not c.bed


def test_the_zero_length_cases_are_where_they_claim_to_be():
    c = kc.case("zero_zoo")
    zero = [r for r in map(kr.parse, c.records) if any(n == 0 and op in kr.REF_OPS for op, n in r["cigar"])]
    assert len(zero) == 5 * 2 * len(kc.k3.ZERO_SHAPES)
    differ = [r for r in zero if sorted(p for p, q in kr.bases_as_written(r)) != sorted(p for p, q in kr.columns(r) if q != 255)]
    assert len(differ) >= len(zero) // 2           # the two walks place the bases differently: what the correction is for
    for r in zero:                                  # every such read is cut by a BED line and by a window edge
        a, b = r["pos"], r["pos"] + kr.span(r)
        assert any(g[0] == r["ref"] and a < g[1] < b for g in c.bed) and any(g[0] == r["ref"] and a < g[2] < b for g in c.bed)
        assert a // min(c.windows) != (b - 1) // min(c.windows)
    c = kc.case("zero_at_position_0")
    parsed = [kr.parse(b) for b in c.records]
    assert sum(r["pos"] == 0 and kr.span(r) == 0 and not r["flag"] & 4 for r in parsed) == 5
    assert [kr.admitted(r) for r in parsed] == [False] * 5 + [True] * 3


@pytest.mark.parametrize("name", ["runs_aba", "ranges_lengths3", "zero_zoo", "thresholds_stack300"])
def test_written_files_inflate_to_the_records(files, name):
    from tests.util import oracle_inflate_all
    c, path, _ = files(name)
    u = bytes(oracle_inflate_all(path))
    assert u[:4] == b"BAM\x01" and u.endswith(b"".join(c.records)) and all(("SM:" + sm).encode() in u[:4096] for _, sm in c.read_groups)
