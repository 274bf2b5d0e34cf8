"""`sambamba flagstat` without a GPU: the Python restatement (tests/flagstat_ref.py) against numbers worked out by hand, the
library's text formatter (sbx_format_flagstat, host only) against a float32 emulation of the reference's percent(), and the
library / CLI surface that needs no device."""
import ctypes as C
import os
import subprocess

import pytest

from tests import bamgen
from tests import flagstat_ref as ref

P, PP, U, MU, R1, R2, SEC, QC, DUP, SUP = 0x1, 0x2, 0x4, 0x8, 0x40, 0x80, 0x100, 0x200, 0x400, 0x800


def _rec(flag, mapq=60, ref_id=0, next_ref=0, name="r"):
    if flag & U:
        return bamgen.make_record(ref_id, 100 if ref_id >= 0 else -1, "", "ACGT", 30, name=name, mapq=0, flag=flag,
                                  next_ref=next_ref, next_pos=100)
    return bamgen.make_record(ref_id, 100, "4M", "ACGT", 30, name=name, mapq=mapq, flag=flag, next_ref=next_ref, next_pos=200)


# one record per branch of flagstat.d:33-57
BRANCHES = [
    _rec(SEC | SUP | P | R1),                  # secondary and supplementary: counted as secondary only
    _rec(SUP | P),                             # supplementary: not paired
    _rec(P | PP | U | R1, ref_id=0),           # proper pair but unmapped: no pair_good
    _rec(P | MU | R2),                         # mate unmapped: singleton
    _rec(P | PP | R1, mapq=4, next_ref=1),     # mate on another reference at mapq 4
    _rec(P | PP | R2, mapq=5, next_ref=1),     # ... and at mapq 5
    _rec(P | R2, next_ref=-1),                 # next_refID -1 while the mate counts as mapped
    _rec(P | PP | R1, next_ref=0),             # mate on the same reference
    _rec(DUP),                                 # duplicate, not paired
    _rec(U, ref_id=-1, next_ref=-1),           # unplaced
]
FAILED = [_rec(SEC | SUP | P | R1 | QC), _rec(P | PP | U | R1 | QC), _rec(P | PP | R1 | QC, mapq=4, next_ref=1),
          _rec(P | PP | R2 | QC, mapq=5, next_ref=1)]

EXPECTED = {
    "reads": (10, 4), "secondary": (1, 1), "supplementary": (1, 0), "dup": (1, 0), "mapped": (8, 3), "pair_all": (6, 3),
    "first": (3, 2), "second": (3, 1), "pair_good": (3, 2), "pair_map": (4, 2), "single": (1, 0), "diff_chr": (3, 2),
    "diff_high": (2, 1),
}


def test_restatement_takes_every_branch(tmp_path):
    path = str(tmp_path / "branches.bam")
    bamgen.write_bam(path, [("c1", 1000), ("c2", 1000)], BRANCHES + FAILED, write_index=False,
                     text="@HD\tVN:1.6\tSO:unsorted\n@SQ\tSN:c1\tLN:1000\n@SQ\tSN:c2\tLN:1000\n")
    assert ref.count(path) == EXPECTED


def _zero():
    return {k: (0, 0) for k in ref.FIELDS}


def _cases():
    c_zero = _zero()
    c_small = dict(_zero(), reads=(10, 4), mapped=(8, 3), pair_all=(6, 3), pair_good=(3, 2), single=(1, 0))
    # float32 moves the second decimal: 92.33 % (the double quotient gives 92.32 %), 36.83 % (36.84 %), 78.39 % (78.40 %)
    c_2p24 = dict(_zero(), reads=(16777217, 45546944), mapped=(15489565, 16777217), pair_all=(16777217, 1),
                  pair_good=(16777217, 1), single=(0, 1))
    c_1e12 = dict(_zero(), reads=(340884843527, 778088160177), mapped=(267236675602, 684834304505),
                  pair_all=(10 ** 12, 2), pair_good=(999999999989, 1), single=(1, 0))
    c_full = dict(_zero(), reads=(7, 2 ** 24 + 1), mapped=(7, 2 ** 24 + 1), pair_all=(7, 3), pair_good=(7, 3), single=(7, 3))
    return [c_zero, c_small, c_2p24, c_1e12, c_full]


@pytest.mark.parametrize("tabular", [False, True])
def test_format_matches_the_float32_emulation(tabular):
    import sambamba_amd
    for c in _cases():
        assert sambamba_amd.format_flagstat(c, tabular=tabular) == ref.text(c, tabular=tabular)


def test_format_edge_values():
    import sambamba_amd
    t = sambamba_amd.format_flagstat(_zero())
    assert t.count("\n") == 13 and "0 + 0 mapped (N/A:N/A)" in t
    c = _cases()
    t = sambamba_amd.format_flagstat(c[2])
    assert "15489565 + 16777217 mapped (92.33%:36.83%)" in t
    assert "%.2f%%" % (15489565 / 16777217 * 100) == "92.32%"      # what a double quotient would print
    t = sambamba_amd.format_flagstat(c[3], tabular=True)
    assert "mapped,267236675602:78.39%,684834304505:88.01%" in t
    t = sambamba_amd.format_flagstat(c[4])
    assert "7 + 16777217 mapped (100.00%:100.00%)" in t and "7 + 3 singletons (100.00%:100.00%)" in t
    assert t.splitlines()[0] == "7 + 16777217 in total (QC-passed reads + QC-failed reads)"
    assert sambamba_amd.format_flagstat(c[1], tabular=True).splitlines()[4] == "mapped,8:80.00%,3:75.00%"


def test_format_reports_the_size_it_needs():
    import sambamba_amd
    from sambamba_amd._lib import Flagstat
    L = sambamba_amd.lib()
    f = Flagstat()
    n = C.c_size_t(0)
    assert L.sbx_format_flagstat(C.byref(f), 0, None, 0, C.byref(n)) == -8        # SBX_ENOMEM, the size in n
    want = len(sambamba_amd.format_flagstat(_zero()))
    assert n.value == want
    buf = C.create_string_buffer(want)
    assert L.sbx_format_flagstat(C.byref(f), 0, buf, want, C.byref(n)) == -8       # no room for the terminating zero
    buf = C.create_string_buffer(want + 1)
    assert L.sbx_format_flagstat(C.byref(f), 0, buf, want + 1, C.byref(n)) == 0


def test_library_exports_flagstat_without_a_gpu():
    import sambamba_amd
    L = sambamba_amd.lib()
    assert hasattr(L, "sbx_flagstat") and hasattr(L, "sbx_format_flagstat")
    from sambamba_amd._lib import Flagstat
    assert L.sbx_abi_sizeof(b"sbx_flagstat_counts") == C.sizeof(Flagstat) == 26 * 8


def test_cli_usage_and_bad_options_need_no_device():
    import sambamba_amd
    cli = sambamba_amd.flagstat_cli_path()
    assert os.path.exists(cli)
    r = subprocess.run([cli], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert r.returncode == 1 and r.stdout == b"" and b"Usage" in r.stderr
    r = subprocess.run([cli, "--no-such-option", "x.bam"], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert r.returncode == 1 and r.stdout == b"" and r.stderr
    r = subprocess.run([cli, "x.bam", "-t", "many"], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert r.returncode == 1 and r.stdout == b"" and r.stderr
