"""K9 (`sambamba sort`: K9a keys, K9b radix sort, K9c gather, sort.hip) on inputs placed on the kernels' own limits
(tests/k9_cases.py; tests/test_k9_cases_cpu.py checks that they are where they claim to be, and that a K9b with one defect gets a
named case wrong): `sambamba_amd.sort_bam` against tests/sort_ref.py, byte for byte on the inflated stream, with the stats that show
the case planned the passes it was built for.  The limits and the cases on each: the tile of 4096, the round of 256 and the wave of
64 with the break behind the last live round (`count*`); the pass plan -- unaligned shifts, an overhanging top digit, skipped
digits, 0 to 6 passes, both parities of the two buffers (PLAN_NAMES); which lane of which round holds which digit (LAYOUT_NAMES);
K9a's groups of 256 and its accumulators under -F (`filter_*`); the head, chunks and tail of copy_span16 at every pair of
alignments (`gather`); and a name order whose second word starts from the second value buffer (`names`)."""
import pytest

from tests import k9_cases as kc
from tests import namesort_ref
from tests import sort_ref as ref
from tests.test_gpu_sort import check_file

pytestmark = pytest.mark.gpu


def run_case(name, tmp_path, **order):
    import sambamba_amd
    c = kc.case(name)
    path, out = str(tmp_path / (name + ".bam")), str(tmp_path / (name + ".sorted.bam"))
    c.write(path)
    if order:
        want = namesort_ref.expected(path, namesort_ref.LEX)
    else:
        want = ref.expected(path, c.keep)
    st = sambamba_amd.sort_bam(path, out, filter=c.flt, **order)
    got = {k: st[k] for k in c.expect}
    print(name, got)
    check_file(out, want)
    assert len(ref.split_stream(want)[3]) == c.expect["n_records_out"]
    assert got == c.expect
    return st


@pytest.mark.parametrize("name", kc.COUNT_NAMES)
def test_record_counts_on_wave_round_and_tile_edges(name, tmp_path):
    run_case(name, tmp_path)


@pytest.mark.parametrize("name", kc.PLAN_NAMES)
def test_pass_plans(name, tmp_path):
    """`widest`: positions up to 2^31 - 2 on contigs of 2^31 - 1, beyond what a BAI holds -- through the API, without an index."""
    run_case(name, tmp_path)


@pytest.mark.parametrize("name", kc.LAYOUT_NAMES)
def test_digit_layouts_of_one_pass(name, tmp_path):
    run_case(name, tmp_path)


@pytest.mark.parametrize("name", kc.FILTER_NAMES)
def test_keys_under_a_filter(name, tmp_path):
    """The rejected records lie on another contig at positions around 2^20: `key_bits` and `n_sort_passes` are those of the kept
    keys only if no rejected record reaches the OR / AND words."""
    run_case(name, tmp_path)


def test_gather_alignments(tmp_path):
    run_case("gather", tmp_path)


def test_name_order_continues_from_the_second_value_buffer(tmp_path):
    """Word 1 of the names plans one pass, word 0 four (tests/test_k9_cases_cpu.py): continue_resident_order starts from val2."""
    run_case("names", tmp_path, order="queryname")
