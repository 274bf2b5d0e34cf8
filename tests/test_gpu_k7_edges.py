"""K7 (`--fix-mate-overlaps`, mates.hip) on inputs placed on its own limits (tests/k7_cases.py; tests/test_k7_cases_cpu.py checks
that they are where they claim to be): device counters through the C ABI and CLI text, bit-exact against the oracle.  The limits
and the design on each: the aligned blocks of 16 positions and the 11-block limit of phase 1 (`sweep`), tile borders (`borders`),
the per-position path's rule (`kinds`), the list of 382 records (`worklist`), the u16 record indices (`index65535`, `index65536`),
the window of 1024 records and the table of half hashes of k_find_mates_join (`join`), three partners and seven intervals
(`partners`), and one name in two samples, which is refused."""
import numpy as np
import pytest

from tests import bamgen as bg
from tests import k7_cases as kc
from tests.test_gpu_k3_edges import same_text
from tests.util import oracle_base_counters, run_cli, run_oracle

pytestmark = pytest.mark.gpu

BUILDERS = {
    "sweep1": (kc.pair_sweep, (1,)), "sweep2": (kc.pair_sweep, (2,)), "sweep3": (kc.pair_sweep, (3,)),
    "borders1": (kc.pair_borders, (1,)), "borders2": (kc.pair_borders, (2,)), "borders3": (kc.pair_borders, (3,)),
    "kinds": (kc.pair_kinds, ()), "worklist": (kc.work_list, ()),
    "index65535": (kc.index_limit, (65535,)), "index65536": (kc.index_limit, (65536,)),
    "join": (kc.join_window, ()),
    "partners1": (kc.partner_lists, (1,)), "partners2": (kc.partner_lists, (2,)),
    "short": (kc.short_sequence, ()),
}
PAIRS = ["sweep1", "sweep2", "sweep3", "borders1", "borders2", "borders3", "kinds", "worklist", "index65535", "index65536", "join"]
GROUPS = ["partners1", "partners2"]


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    """name -> (path, refs, n_samples), each BAM built once, when first asked for."""
    d = tmp_path_factory.mktemp("k7edges")
    made = {}

    def put(name, refs, records, groups):
        path = str(d / (name + ".bam"))
        bg.write_bam(path, refs, records, read_groups=groups)
        made[name] = (path, refs, max(1, len(groups)))

    def get(name):
        if name not in made:
            if name in BUILDERS:
                builder, args = BUILDERS[name]
                put(name, *builder(*args))
            else:
                for key, design in list(kc.partner_refusals().items()) + list(kc.same_name_two_samples().items()):
                    put(key, *design)
        return made[name]
    return get


@pytest.fixture(scope="module")
def oracle(files):
    """(name, min_bq) -> the oracle's counters with mate fixing of every contig, computed once."""
    memo = {}

    def get(name, min_bq):
        if (name, min_bq) not in memo:
            path, refs, S = files(name)
            memo[name, min_bq] = [oracle_base_counters(path, r, 0, ln, n_samples=S, min_bq=min_bq, fix_mate=True)
                                  for r, (_, ln) in enumerate(refs)]
            for a in memo[name, min_bq]:
                a.setflags(write=False)
        return memo[name, min_bq]
    return get


def check_counters(files, oracle, name, min_bq):
    import sambamba_amd
    path, refs, S = files(name)
    want, want0 = oracle(name, min_bq), oracle(name, 0)
    with sambamba_amd.Depth(path) as d:
        assert d.info.n_samples == S
        d.set_params(min_bq=min_bq, fix_mate_overlaps=True)
        d.run()
        for r, (nm, ln) in enumerate(refs):
            got, cov = d.base_counters(r, 0, ln, with_covered=True)
            if not np.array_equal(got, want[r]):
                p, s, k = np.argwhere(got != want[r])[0]
                raise AssertionError("%s, contig %s, -q %d: %d positions differ, the first at %d, sample %d, counter %d: device %d, oracle %d"
                                     % (name, nm, min_bq, (got != want[r]).any(axis=(1, 2)).sum(), p, s, k, got[p, s, k], want[r][p, s, k]))
            assert np.array_equal(cov.astype(bool), want0[r].sum(axis=(1, 2)) > 0), (name, nm, min_bq)


@pytest.mark.parametrize("min_bq", [0, kc.MIN_BQ])
@pytest.mark.parametrize("name", PAIRS + GROUPS)
def test_counters_on_the_kernels_limits(files, oracle, name, min_bq):
    """-q 20 lies between the qualities drawn (12 and 23): the quality test, and the span counts (the `covered` bytes) through the
    difference array of phase 1 and the per-position counts of phase 2."""
    check_counters(files, oracle, name, min_bq)


def bed_of(refs, path):
    with open(path, "w") as fh:
        for nm, ln in refs:
            for a in range(0, ln, 37):
                fh.write("%s\t%d\t%d\n" % (nm, a, min(ln, a + 50)))
    return path


CLI_ARGS = [["base", "-m", "-c", "0"], ["window", "-m", "-w", "16"], ["window", "-m", "-w", "1000"], ["region", "-m"]]
CLI_CASES = [(n, a) for n in PAIRS for a in CLI_ARGS]


@pytest.mark.parametrize("name,args", CLI_CASES, ids=["%s-%s" % (n, "".join(a[:1] + a[2:])) for n, a in CLI_CASES])
def test_cli_text(files, tmp_path, name, args):
    """`base -m` is k_accumulate_mates behind the formatter; `window -m` and `region -m` are k_mates_columns and the closed forms of
    reduce.hip, the regions [37 k, 37 k + 50) of every contig overlapping each other."""
    path, refs, _ = files(name)
    if args[0] == "region":
        args = args + ["-L", bed_of(refs, str(tmp_path / "r.bed"))]
    same_text(run_cli(args + [path]), run_oracle(args + [path]), " ".join(args))


@pytest.mark.parametrize("variant", ["0", "1"])
@pytest.mark.parametrize("name", PAIRS + GROUPS)
def test_both_paths_of_accumulate_mates_give_the_oracles_text(files, name, variant):
    """SBX_K7_VARIANT=0 sends every record to the per-position path, 1 (the default) is phase 1 and the list: the same text."""
    path = files(name)[0]
    args = ["base", "-m", "-q", str(kc.MIN_BQ), "-c", "0", path]
    same_text(run_cli(args, env={"SBX_K7_VARIANT": variant}), run_oracle(args), "SBX_K7_VARIANT=" + variant)


def test_a_record_without_a_sequence_counts_the_same_on_both_paths(files):
    """`20M` with SEQ `*`: the reference has no defined answer (k7_cases.short_sequence), so the paths are compared with each other,
    and the ordinary pair next to it with the oracle."""
    path = files("short")[0]
    args = ["base", "-m", "-c", "0", path]
    got = [run_cli(args, env={"SBX_K7_VARIANT": v}) for v in ("0", "1")]
    same_text(got[1], got[0], "SBX_K7_VARIANT=1 against 0")
    rows = lambda text: [ln for ln in text.decode().splitlines() if ln.split("\t")[1:2] and ln.split("\t")[1].isdigit() and int(ln.split("\t")[1]) >= 150]
    assert rows(got[0]) == rows(run_oracle(args)) and len(rows(got[0])) > 20


def refused(args):
    r = run_cli(args, check=False)
    assert r.returncode == 1 and b"same name" in r.stderr, (args, r.returncode, r.stderr)
    return r


@pytest.mark.parametrize("name", ["four_partners", "four_over_one_column"])
def test_more_than_three_partners_are_refused(files, name):
    """`four_partners` holds no column with more than two records of the name: refused because a record lists three partners at most
    (the conservative side of `np > 3`)."""
    path = files(name)[0]
    refused(["base", "-m", path])
    same_text(run_cli(["base", path]), run_oracle(["base", path]), "without -m")


@pytest.mark.parametrize("name", GROUPS)
def test_region_and_window_refuse_partner_lists(files, tmp_path, name):
    path, refs, _ = files(name)
    refused(["window", "-m", "-w", "16", path])
    refused(["region", "-m", "-L", bed_of(refs, str(tmp_path / "r.bed")), path])


@pytest.mark.parametrize("name", ["xyz", "xyzw", "xzy"])
def test_one_name_in_two_samples_is_refused(files, name):
    """X (s1), Y (s2), Z (s1): the reference pairs X with Z only where Y does not sort between them (depth.d:343-377); linking them
    by name and sample alone differed from the oracle on 40 columns of `xyz`, 80 of `xyzw` and 10 of `xzy` (there the oracle pairs X
    with Z, but leaves Z `detected` beside Y behind X's end).  K7 refuses a record that has a partner of its own sample and overlaps
    a same-name record of another one, in every mode."""
    path = files(name)[0]
    for args in (["base", "-m"], ["window", "-m", "-w", "16"]):
        r = refused(args + [path])
        assert b"different samples" in r.stderr
    same_text(run_cli(["base", path]), run_oracle(["base", path]), "without -m")


def test_one_name_in_two_samples_without_a_partner_is_not_refused(files, oracle):
    """X (s1), Y (s2) alone: nobody pairs, on the device as in the oracle."""
    for q in (0, kc.MIN_BQ):
        check_counters(files, oracle, "two", q)
    path = files("two")[0]
    for args in (["base", "-m", "-c", "0"], ["window", "-m", "-w", "16"]):
        same_text(run_cli(args + [path]), run_oracle(args + [path]), " ".join(args))
