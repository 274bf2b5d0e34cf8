"""K5 (region / window statistics: k_range_reduce, k_count_reads_windows with add_runs, k_count_reads_regions in reduce.hip, driven by
engine_stats.cpp) on inputs placed on its own limits (tests/k5_cases.py; tests/test_k5_cases_cpu.py checks that they are where
they claim to be and that the restatement of the closed forms, tests/k5_ref.py, prints what the oracle prints).  Through the
Python API every number -- n_reads, n_bases, the threshold counts, `seen` -- is exactly the restatement's, per range, sample and
threshold; through the CLI the text is the oracle's, once more with the seven counters instead of the compact word
(SBX_COMPACT=0) for the `ranges_*` and `thresholds_*` cases and once more through the per-call chunk list
(SBX_WINDOWS_AT_ONCE=0) for every window line.  Integers and text: no tolerance anywhere."""
import numpy as np
import pytest

from tests import bamgen as bg
from tests import k5_cases as kc
from tests import k5_ref as kr
from tests.util import run_cli, run_oracle

pytestmark = pytest.mark.gpu

REFUSAL = "more than 16 coverage thresholds"


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    """name -> (case, BAM path, BED path or None), each BAM built once, when first asked for."""
    d = tmp_path_factory.mktemp("k5edges")
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


def restated(name, min_bq, combined):
    """The restatement of a case, computed once and left unchanged."""
    if (name, min_bq, combined) not in _restated:
        _restated[name, min_bq, combined] = kr.Restatement(kc.case(name), min_bq, combined)
    return _restated[name, min_bq, combined]


def same_numbers(got, want, ranges, what):
    for label, g, w in zip(("n_reads", "n_bases", "cov", "seen"), got, want):
        g, w = np.asarray(g, dtype=np.int64), np.asarray(w, dtype=np.int64)
        assert g.shape == w.shape, (what, label, g.shape, w.shape)
        if not np.array_equal(g, w):
            at = tuple(int(x) for x in np.argwhere(g != w)[0])
            raise AssertionError("%s, %s: %d entries differ, the first at %s (range %s): device %d, restated %d"
                                 % (what, label, (g != w).sum(), at, ranges[at[0]], g[at], w[at]))


API_NAMES = [n for n in kc.ALL_NAMES if kc.case(n).windows or kc.case(n).bed]


@pytest.mark.parametrize("name", API_NAMES)
def test_numbers_through_the_api(files, name):
    import sambamba_amd
    c, path, _ = files(name)
    thr = c.thresholds
    with sambamba_amd.Depth(path) as d:
        assert d.info.n_samples == c.n_samples
        for combined in (False, True) if c.n_samples > 1 else (False,):
            for q in c.min_bqs:
                rs = restated(name, q, combined)
                what = "%s -q %d%s" % (name, q, " --combined" if combined else "")
                if c.bed:
                    ranges = list(c.bed + c.api_ranges)
                    d.set_params(mode=sambamba_amd.SBX_MODE_REGION, min_bq=q, combined=combined, thresholds=thr)
                    d.run()
                    same_numbers(d.region_stats(ranges, len(thr)), rs.stats(ranges, thr), ranges, what + " region")
                for w in c.windows:
                    d.set_params(mode=sambamba_amd.SBX_MODE_WINDOW, min_bq=q, combined=combined, window=w, thresholds=thr)
                    d.run()
                    for ref, (_, ln) in enumerate(c.refs):
                        ranges = rs.windows(ref, w)
                        if not ranges:
                            continue
                        got = d.window_stats(ref, 0, len(ranges), len(thr))
                        same_numbers(got, rs.stats(ranges, thr)[:3], ranges, "%s window -w %d" % (what, w))


CLI_LINES = [(n, k) for n in kc.ALL_NAMES for k in range(len(kc.case(n).cli_lines("bed")))]


def line_id(name, k):
    a = kc.case(name).cli_lines("bed")[k]
    return "%s-%s%s%s" % (name, "w" + a[2] if a[0] == "window" else "bed", "-q" + a[a.index("-q") + 1] if "-q" in a else "",
                          "-combined" if "--combined" in a else "")


def same_text(got, want, what):
    if got != want:
        gl, wl = got.decode().splitlines(), want.decode().splitlines()
        k = next((i for i in range(min(len(gl), len(wl))) if gl[i] != wl[i]), min(len(gl), len(wl)))
        raise AssertionError("%s: %d vs %d lines, the first difference at line %d:\n  device: %r\n  oracle: %r" % (
            what, len(gl), len(wl), k, gl[k] if k < len(gl) else None, wl[k] if k < len(wl) else None))


@pytest.mark.parametrize("name,k", CLI_LINES, ids=[line_id(n, k) for n, k in CLI_LINES])
def test_cli_text(files, name, k):
    """The environment variables are read once per process: each variant is a CLI process of its own."""
    c, path, bed = files(name)
    args = c.cli_lines(bed)[k] + [path]
    what = "%s: %s" % (name, " ".join(args[:-1]))
    want = run_oracle(args)
    assert want.count(b"\n") > 1          # rows, not the header alone
    same_text(run_cli(args), want, what)
    if name in kc.RANGES_NAMES + kc.THRESHOLDS_NAMES:
        same_text(run_cli(args, env={"SBX_COMPACT": "0"}), want, what + " (SBX_COMPACT=0)")
    if args[0] == "window":
        same_text(run_cli(args, env={"SBX_WINDOWS_AT_ONCE": "0"}), want, what + " (SBX_WINDOWS_AT_ONCE=0)")


OVERLAPS = [(n, w, o, q) for n in kc.ALL_NAMES for w, o in kc.case(n).overlaps for q in kc.case(n).min_bqs]


@pytest.mark.parametrize("name,w,o,q", OVERLAPS, ids=["%s-w%d-o%d-q%d" % x for x in OVERLAPS])
def test_cli_text_of_overlapping_windows(files, name, w, o, q):
    """--overlap: the first ring of windows counts only the reads that begin at or after `min_start` (that branch of
    k_count_reads_regions, and k_range_reduce's `no_bases`), the others are plain ranges."""
    path = files(name)[1]
    args = ["window", "-w", str(w), "--overlap", str(o), "-q", str(q), "-T", "1", "-T", "3", path]
    same_text(run_cli(args), run_oracle(args), " ".join(args[:-1]))


def test_seventeen_thresholds_are_refused(files):
    import sambamba_amd
    c, path, bed = files("thresholds_stacks1")
    seventeen = tuple(range(1, kc.MAX_THRESHOLDS + 2))
    with sambamba_amd.Depth(path) as d:
        with pytest.raises(sambamba_amd.SbxError, match=REFUSAL):
            d.set_params(mode=sambamba_amd.SBX_MODE_REGION, thresholds=seventeen)
            d.run()
            d.region_stats(list(c.bed), len(seventeen))
        with pytest.raises(sambamba_amd.SbxError, match=REFUSAL):
            d.set_params(mode=sambamba_amd.SBX_MODE_WINDOW, window=10, thresholds=seventeen)
            d.run()
            d.window_stats(0, 0, 5, len(seventeen))
        d.set_params(mode=sambamba_amd.SBX_MODE_REGION, thresholds=seventeen[:16])          # sixteen are taken
        d.run()
        rs = restated(c.name, 0, False)
        same_numbers(d.region_stats(list(c.bed), 16), rs.stats(c.bed, seventeen[:16]), c.bed, "sixteen thresholds")
    thr = [x for t in seventeen for x in ("-T", str(t))]
    for args in (["region", "-L", bed] + thr, ["window", "-w", "10"] + thr):
        r = run_cli(args + [path], check=False)
        assert r.returncode != 0 and REFUSAL in r.stderr.decode(), (args[0], r.returncode, r.stderr)
        assert [ln for ln in r.stdout.decode().splitlines() if not ln.startswith("#")] == [], args[0]      # no row is written
