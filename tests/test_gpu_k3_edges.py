"""K3 (`decode_accumulate`, depth.hip) on inputs placed on its own limits (tests/k3_cases.py; tests/test_k3_cases_cpu.py checks that
they are where they claim to be): device counters through the C ABI and CLI text, bit-exact against the oracle.  The same files go
through k_accumulate16c (one sample, -q 0), k_accumulate16 (a base-quality threshold, span counts, several samples) and, with the
deep-tile limit lowered to one record, the 32-bit k_accumulate; the stacks of 65,535 / 65,536 records reach the real limit."""
import numpy as np
import pytest

from tests import bamgen as bg
from tests import k3_cases as kc
from tests.util import oracle_base_counters, run_cli, run_oracle

pytestmark = pytest.mark.gpu

BUILDERS = {
    "sweep1": (kc.alignment_sweep, 1), "sweep2": (kc.alignment_sweep, 2), "sweep3": (kc.alignment_sweep, 3),
    "queues1": (kc.queue_periods, 1), "queues2": (kc.queue_periods, 2), "queues3": (kc.queue_periods, 3),
    "zoo": (kc.zero_length_zoo, None), "stacks": (kc.stacks, None), "deep": (kc.stacks_deep, None),
}
SMALL = ["sweep1", "sweep2", "sweep3", "queues1", "queues2", "queues3", "zoo"]


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    """name -> (path, refs, n_samples), each BAM built once, when first asked for."""
    d = tmp_path_factory.mktemp("k3edges")
    made = {}

    def get(name):
        if name not in made:
            builder, n_samples = BUILDERS[name]
            refs, records, groups = builder(n_samples) if n_samples else builder()
            path = str(d / (name + ".bam"))
            bg.write_bam(path, refs, records, read_groups=groups)
            made[name] = (path, refs, n_samples or 1)
        return made[name]
    return get


@pytest.fixture(scope="module")
def oracle(files):
    """(name, min_bq) -> the oracle's counters of every contig, computed once.  A contig whose reads hang over its end (the
    `g_outside` designs) is compared one tile further."""
    memo = {}

    def get(name, min_bq):
        if (name, min_bq) not in memo:
            path, refs, S = files(name)
            memo[name, min_bq] = [oracle_base_counters(path, r, 0, extent(nm, ln, S), n_samples=S, min_bq=min_bq)
                                  for r, (nm, ln) in enumerate(refs)]
            for a in memo[name, min_bq]:
                a.setflags(write=False)
        return memo[name, min_bq]
    return get


def extent(name, length, n_samples):
    return length + (kc.tile_positions(n_samples) if name.startswith("g_") else 0)


def check_counters(files, oracle, name, min_bq):
    import sambamba_amd
    path, refs, S = files(name)
    want, want0 = oracle(name, min_bq), oracle(name, 0)
    with sambamba_amd.Depth(path) as d:
        assert d.info.n_samples == S
        d.set_params(min_bq=min_bq)
        st = d.run()
        for r, (nm, ln) in enumerate(refs):
            got, cov = d.base_counters(r, 0, extent(nm, ln, S), with_covered=True)
            if not np.array_equal(got, want[r]):
                p, s, k = np.argwhere(got != want[r])[0]
                raise AssertionError("%s, contig %s, -q %d: %d positions differ, the first at %d, sample %d, counter %d: device %d, oracle %d"
                                     % (name, nm, min_bq, (got != want[r]).any(axis=(1, 2)).sum(), p, s, k, got[p, s, k], want[r][p, s, k]))
            assert np.array_equal(cov.astype(bool), want0[r].sum(axis=(1, 2)) > 0), (name, nm, min_bq)
    return st


@pytest.mark.parametrize("deep_limit", [None, "1"], ids=["16bit", "32bit"])
@pytest.mark.parametrize("min_bq", [0, kc.MIN_BQ])
@pytest.mark.parametrize("name", SMALL)
def test_counters_on_the_kernels_boundaries(files, oracle, monkeypatch, name, min_bq, deep_limit):
    """-q 0 is k_accumulate16c for one sample and k_accumulate16<.., false, false> for several; -q 20 lies between the qualities
    drawn (12 and 23) and brings the quality test and the span counts (the `covered` bytes); SBX_DEEP_TILE_RECORDS=1 sends every
    tile to the 32-bit kernel."""
    if deep_limit:
        monkeypatch.setenv("SBX_DEEP_TILE_RECORDS", deep_limit)
    check_counters(files, oracle, name, min_bq)


@pytest.mark.parametrize("min_bq", [0, kc.MIN_BQ])
@pytest.mark.parametrize("name", ["stacks", "deep"])
def test_counters_at_the_real_limit_of_the_16_bit_counters(files, oracle, name, min_bq):
    """65,535 records in a tile stay in 16-bit halves (a counter at 0xFFFF beside its neighbour), 65,536 go to the 32-bit kernel:
    no lowered limit here."""
    path, refs, _ = files(name)
    want = oracle(name, min_bq)
    tops = [int(w.max()) for w in want]
    if min_bq == 0:
        assert tops == ([65535] * 4 if name == "stacks" else [65536] * 2)
    check_counters(files, oracle, name, min_bq)


CLI_ARGS = [["base", "-c", "0"], ["window", "-w", "16"], ["window", "-w", "1000"]]
CLI_CASES = [(n, a) for n in SMALL + ["stacks", "deep"] for a in CLI_ARGS]


def same_text(got, want, what):
    if got != want:
        gl, wl = got.decode().splitlines(), want.decode().splitlines()
        k = next((i for i in range(min(len(gl), len(wl))) if gl[i] != wl[i]), min(len(gl), len(wl)))
        raise AssertionError("%s: %d vs %d lines, the first difference at line %d:\n  device: %r\n  oracle: %r" % (
            what, len(gl), len(wl), k, gl[k] if k < len(gl) else None, wl[k] if k < len(wl) else None))


def check_cli(path, args):
    want = run_oracle(args + [path])
    same_text(run_cli(args + [path]), want, " ".join(args))
    if args[0] != "base":
        same_text(run_cli(args + [path], env={"SBX_COMPACT": "0"}), want, " ".join(args) + " (SBX_COMPACT=0)")


@pytest.mark.parametrize("name,args", CLI_CASES, ids=["%s-%s" % (n, "".join(a[:3])) for n, a in CLI_CASES])
def test_cli_text(files, name, args):
    """Window runs keep the compact word {bases : 16 | depth : 16} (SBX_COMPACT=0: the seven counters): the same text either way.
    On `deep` a tile of 65,536 records switches the compact word off and the window run still answers."""
    check_cli(files(name)[0], args)


ZOO_ARGS = [["region"], ["region", "-q", str(kc.MIN_BQ), "-T", "1", "-T", "20"], ["window", "-w", "16", "-q", str(kc.MIN_BQ)],
            ["window", "-w", "64", "--overlap", "16"]]


@pytest.mark.parametrize("args", ZOO_ARGS, ids=["region", "region-q", "w16-q", "overlap"])
def test_region_and_window_sums_with_zero_length_operations(files, tmp_path, args):
    """The reference's region / window sums do not come from the pileup's columns: countOverlappingBases (sambamba/depth.d:671-698)
    walks the CIGAR with the lengths as written, so a zero-length D / N / M takes no column there, while in the per-position
    counters it takes one (pileup.d:195-205) and the read is cut at its end.  reduce.hip adds the difference per read."""
    path, refs, _ = files("zoo")
    if args[0] == "region":
        bed = str(tmp_path / "zoo.bed")
        with open(bed, "w") as fh:
            for nm, ln in refs:
                for a in range(0, ln, 37):
                    fh.write("%s\t%d\t%d\n" % (nm, a, min(ln, a + 50)))
        args = args + ["-L", bed]
    check_cli(path, args)


@pytest.mark.parametrize("name", ["stacks", "deep"])
def test_region_thresholds_around_the_stacked_positions(files, tmp_path, name):
    path, refs, _ = files(name)
    bed = str(tmp_path / "stacked.bed")
    with open(bed, "w") as fh:
        for nm, ln in refs:
            at = ln - 1024 + kc.STACK_POS
            fh.write("%s\t%d\t%d\tcolumn\n%s\t%d\t%d\taround\n" % (nm, at, at + 1, nm, at - 6, at + 7))
    args = ["region", "-L", bed, "-T", "1", "-T", "65535", "-T", "65536", path]
    want = run_oracle(args)
    assert run_cli(args) == want
    assert run_cli(args, env={"SBX_COMPACT": "0"}) == want
