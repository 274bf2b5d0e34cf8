"""The run planner of the indexed view (sambamba_amd/csrc/view_index_core.hpp) and the joining of runs (file_run.hpp), compiled for
the host with g++ into tests/native/viewidx_host.cpp -- once plainly, once under AddressSanitizer and UBSan.  The chain walk of K2
is played by a list of record offsets.  Expected batches are written out by hand where the case is small and come from a restatement
in Python (plan_ref, written from the header comment of view_index_core.hpp) otherwise; for every plan the properties that make the
indexed view right are asserted: the kept batches cover every record of every run exactly once, in order, every piece starts inside
the block that holds its first record, and only the last piece of a run is closed.  No GPU needed."""
import os
import subprocess

import pytest

from tests.util import ROOT

SRC = os.path.join(ROOT, "tests", "native", "viewidx_host.cpp")
FLAGS = ["-std=c++17", "-Wall"]
OFF = [10 * k for k in range(11)] + [100]           # ten blocks of ten bytes and an empty one (the EOF block)


@pytest.fixture(scope="module")
def hosts(tmp_path_factory):
    d = tmp_path_factory.mktemp("viewidx")
    plain, san = str(d / "viewidx_host"), str(d / "viewidx_host_san")
    subprocess.check_call(["g++", "-O2"] + FLAGS + ["-o", plain, SRC])
    subprocess.check_call(["g++", "-O1", "-g"] + FLAGS + ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", san, SRC])
    return plain, san


def call(hosts, cmd, numbers):
    outs = []
    for exe in hosts:
        r = subprocess.run([exe, cmd], input=" ".join(map(str, numbers)).encode(), stdout=subprocess.PIPE, stderr=subprocess.PIPE)
        assert r.returncode == 0, r.stderr.decode()[-3000:]
        outs.append(r.stdout.decode())
    assert outs[0] == outs[1]
    return outs[0].splitlines()


def table(off):
    return [len(off) - 1] + list(off)


def flat(runs):
    return [len(runs)] + [x for r in runs for x in r]


def plan(hosts, runs, budget, rec, off=OFF):
    """[(kept, [(blk0, blk1, ub, ue, open)], stop)], final budget"""
    lines = call(hosts, "plan", table(off) + [budget] + flat(runs) + [len(rec) - 1] + list(rec))
    assert lines[-1].startswith("budget ")
    out = []
    for line in lines[:-1]:
        parts = line.split("  ")
        out.append((parts[0] == "B", [tuple(int(x) for x in p.split()) for p in parts[1:-1]], int(parts[-1])))
    return out, int(lines[-1].split()[1])


def plan_ref(runs, budget, rec, off=OFF):
    """The planner once more: whole runs while their blocks fit the budget, else pieces cut at block boundaries; the next piece starts
    with the straddling record; a piece without a whole record doubles the budget."""
    out, i = [], 0
    size = lambda r: off[r[1]] - off[r[0]]
    while i < len(runs):
        if size(runs[i]) <= budget:
            group, used = [], 0
            while i < len(runs) and used + size(runs[i]) <= budget:
                used += size(runs[i])
                group.append(tuple(runs[i]) + (0,))
                i += 1
            out.append((True, group, group[-1][3]))
            continue
        blk0, blk1, cur, ue = runs[i]
        while True:
            b0 = max(b for b in range(blk0, blk1) if off[b] <= cur)
            b1 = next((b for b in range(b0 + 1, blk1) if off[b] >= off[b0] + budget), blk1)
            if b1 >= blk1 or off[b1] >= ue:
                out.append((True, [(b0, blk1, cur, ue, 0)], ue))
                break
            stop = next((a for a, b in zip(rec, rec[1:]) if a >= cur and b > off[b1]), off[b1])
            out.append((stop > cur, [(b0, b1, cur, off[b1], 1)], stop))
            if stop > cur:
                cur = stop
            else:
                budget *= 2
        i += 1
    return out, budget


def check_cover(batches, runs, rec):
    """every record of every run lies in exactly one kept batch, in order"""
    seen = []
    for kept, group, stop in batches:
        if not kept:
            continue
        for k, (b0, b1, ub, ue, is_open) in enumerate(group):
            hi = stop if is_open else ue
            seen += [a for a in rec[:-1] if ub <= a < hi]
            assert OFF[b0] <= ub < OFF[b0 + 1], "a batch starts inside the block of its first record"
    want = [a for r in runs for a in rec[:-1] if r[2] <= a < r[3]]
    assert seen == want


def records(lengths, first=0):
    rec = [first]
    for n in lengths:
        rec.append(rec[-1] + n)
    return rec


def test_no_runs(hosts):
    assert plan(hosts, [], 50, [0, 100]) == ([], 50)


def test_one_run_smaller_than_the_budget(hosts):
    rec = records([7] * 2, 23)
    assert plan(hosts, [(2, 4, 23, 37)], 100, rec) == ([(True, [(2, 4, 23, 37, 0)], 37)], 100)


def test_runs_that_exactly_fill_a_budget(hosts):
    runs = [(0, 2, 3, 17), (4, 6, 41, 59), (8, 9, 80, 90)]
    rec = records([1] * 100)
    got, _ = plan(hosts, runs, 40, rec)
    assert got == [(True, [(0, 2, 3, 17, 0), (4, 6, 41, 59, 0)], 59), (True, [(8, 9, 80, 90, 0)], 90)]
    got, _ = plan(hosts, runs, 39, rec)                 # one byte less: the second run no longer fits next to the first
    assert got == [(True, [(0, 2, 3, 17, 0)], 17), (True, [(4, 6, 41, 59, 0), (8, 9, 80, 90, 0)], 90)]
    got, _ = plan(hosts, runs, 50, rec)
    assert [len(g) for _, g, _ in got] == [3]
    for b in (39, 40, 50):
        got, _ = plan(hosts, runs, b, rec)
        assert (got, b) == plan_ref(runs, b, rec)
        check_cover(got, runs, rec)


@pytest.mark.parametrize("straddler", [50, 55, 59])        # the first, a middle and the last byte of block 5
def test_a_run_cut_into_two_pieces(hosts, straddler):
    run = (0, 10, 2, 100)
    rec = records([4] * ((straddler - 2) // 4), 2)
    rec += [straddler] if rec[-1] != straddler else []
    rec += [straddler + 12]
    rec += records([3] * 40, rec[-1])[1:]
    rec = [a for a in rec if a <= 100]
    rec[-1] = 100
    got, budget = plan(hosts, [run], 60, rec)
    assert got == [(True, [(0, 6, 2, 60, 1)], straddler), (True, [(5, 10, straddler, 100, 0)], 100)] and budget == 60
    check_cover(got, [run], rec)


@pytest.mark.parametrize("shift", [0, 5, 9])                # the straddlers at the first, a middle and the last byte of their blocks
def test_a_run_cut_into_five_pieces(hosts, shift):
    run = (0, 10, 0, 100)
    # records of 3 bytes, and one that straddles each of the boundaries 30, 50, 70, 90: it starts `shift` bytes into the block in
    # front of the boundary and ends two bytes behind it
    rec, at = [0], 0
    for boundary in (30, 50, 70, 90):
        start = boundary - 10 + shift
        while at + 3 <= start:
            at += 3
            rec.append(at)
        if at != start:
            at = start
            rec.append(at)
        at = boundary + 2
        rec.append(at)
    while at + 3 <= 100:
        at += 3
        rec.append(at)
    rec[-1] = 100
    got, budget = plan(hosts, [run], 30, rec)
    assert (got, budget) == plan_ref([run], 30, rec) and budget == 30
    assert [k for k, _, _ in got] == [True] * 5
    assert [g[0][4] for _, g, _ in got] == [1, 1, 1, 1, 0]
    assert [stop for _, _, stop in got][:4] == [20 + shift, 40 + shift, 60 + shift, 80 + shift]
    assert [g[0][:2] for _, g, _ in got] == [(0, 3), (2, 5), (4, 7), (6, 9), (8, 10)]
    check_cover(got, [run], rec)


def test_a_record_longer_than_the_budget_doubles_it(hosts):
    run = (0, 10, 0, 100)
    rec = [0, 5, 47, 52, 100]
    got, budget = plan(hosts, [run], 10, rec)
    assert (got, budget) == plan_ref([run], 10, rec)
    assert [(k, g[0][:2]) for k, g, _ in got] == [(True, (0, 1)), (False, (0, 1)), (False, (0, 2)), (False, (0, 4)), (True, (0, 8)), (True, (5, 10))]
    assert budget == 80
    check_cover(got, [run], rec)


def test_the_region_star(hosts):
    # alone: from inside block 7 to the end of the stream, without the empty block behind it
    assert call(hosts, "tail", table(OFF) + [73]) == ["7 10 73 100 0"]
    assert call(hosts, "tail", table(OFF) + [70]) == ["7 10 70 100 0"]
    # a file without unplaced records: nothing is added
    assert call(hosts, "tail", table(OFF) + [100]) == ["none"]
    assert call(hosts, "tail", table([0, 0]) + [0]) == ["none"]
    # next to regions: joined with a run that ends a block in front of it, apart from one further away
    tail = (7, 10, 73, 100, 0)
    assert call(hosts, "join", [1] + flat([(4, 6, 41, 59, 0), tail])) == ["4 10 41 100 0"]
    assert call(hosts, "join", [1] + flat([(0, 2, 3, 17, 0), tail])) == ["0 2 3 17 0", "7 10 73 100 0"]
    got, _ = plan(hosts, [(0, 2, 3, 17), (7, 10, 73, 100)], 100, records([1] * 100))
    assert got == [(True, [(0, 2, 3, 17, 0), (7, 10, 73, 100, 0)], 100)]


def test_join_of_runs_zero_one_and_two_blocks_apart(hosts):
    a = (0, 2, 3, 17, 0)
    for blk0, joined_gap1, joined_gap0 in ((1, True, True), (2, True, True), (3, True, False), (4, False, False)):
        b = (blk0, blk0 + 2, 10 * blk0 + 1, 10 * blk0 + 15, 0)
        for gap, joined in ((1, joined_gap1), (0, joined_gap0)):
            got = call(hosts, "join", [gap] + flat([b, a]))             # (given out of order)
            want = ["0 %d 3 %d 0" % (blk0 + 2, 10 * blk0 + 15)] if joined else ["0 2 3 17 0", "%d %d %d %d 0" % b[:4]]
            assert got == want, (blk0, gap, got)
    # an open end survives only when the run that reaches furthest has it
    assert call(hosts, "join", [0] + flat([(0, 2, 3, 20, 1), (1, 2, 12, 17, 0)])) == ["0 2 3 20 1"]
    assert call(hosts, "join", [0] + flat([(0, 2, 3, 17, 0), (1, 3, 12, 30, 1)])) == ["0 3 3 30 1"]


def test_cost_of_the_runs(hosts):
    assert call(hosts, "cost", table(OFF) + flat([(0, 2, 3, 17), (4, 7, 41, 69)])) == ["5 50"]
    assert call(hosts, "cost", table(OFF) + flat([])) == ["0 0"]
