"""`sambamba index` on the device through `sbx-index`, sbx_index_bam and build_index(check_bins=True): the bytes build_index writes,
and `-c` -- K16a (bins.hip) next to the index pass -- on the reference's fixtures and on a generated file whose bins are spoiled in
the first batch, in a later batch, in the first placed record, in records that are not placed, and in three records."""
import os
import re
import struct
import subprocess

import pytest

from tests import bins_cases as bc
from tests.util import GOLDEN

pytestmark = pytest.mark.gpu

FIXTURES = ("issue225", "issue_193", "issue_204", "mate_overlaps_1_3M_4M", "match_mates")
EFORMAT, ENOTSORTED = -3, -6


def cli(args, env=None):
    from sambamba_amd import index_cli_path
    return subprocess.run([index_cli_path()] + list(args), stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                          env=dict(os.environ, **env) if env else None)


@pytest.fixture(scope="module")
def generated(tmp_path_factory):
    """(path of the generated file, its records, the index of the first chrB record with a position, the .bai build_index writes)"""
    import sambamba_amd
    d = tmp_path_factory.mktemp("index_cli")
    recs, first_b = bc.records()
    path = str(d / "gen.bam")
    bc.write(path, recs)
    sambamba_amd.build_index(path, path + ".want")
    return path, recs, first_b, open(path + ".want", "rb").read()


@pytest.mark.parametrize("name", FIXTURES)
def test_fixtures_index_and_check(name, tmp_path):
    """sbx-index does to every fixture what build_index does.  Four of the five are sorted by coordinate: the same bytes, with and
    without -c (their stored bins are all correct).  match_mates.bam is sorted by name: build_index refuses it with SBX_ENOTSORTED, as
    `sambamba index` does, and so must sbx-index, with and without -c, with the same message and no file."""
    import sambamba_amd
    src = os.path.join(GOLDEN, name + ".bam")
    bam = str(tmp_path / "f.bam")
    with open(bam, "wb") as fh:
        fh.write(open(src, "rb").read())
    out, out_c, api = str(tmp_path / "out.bai"), str(tmp_path / "c.bai"), str(tmp_path / "api.bai")
    if name == "match_mates":
        with pytest.raises(sambamba_amd.SbxError) as ei:
            sambamba_amd.build_index(src, str(tmp_path / "want.bai"))
        assert ei.value.code == ENOTSORTED
        refusal = ("sbx-index: " + ei.value.msg + "\n").encode()
        for args in ([bam], [bam, out], ["-c", bam, out_c]):
            r = cli(args)
            assert (r.returncode, r.stdout, r.stderr) == (1, b"", refusal)
        with pytest.raises(sambamba_amd.SbxError) as ei_c:
            sambamba_amd.build_index(bam, api, check_bins=True)
        assert (ei_c.value.code, ei_c.value.msg) == (ENOTSORTED, ei.value.msg)
        assert sorted(os.listdir(str(tmp_path))) == ["f.bam"]
        return
    sambamba_amd.build_index(src, str(tmp_path / "want.bai"))
    want = open(str(tmp_path / "want.bai"), "rb").read()
    r = cli([bam])
    assert (r.returncode, r.stdout, r.stderr) == (0, b"", b"")
    assert open(bam + ".bai", "rb").read() == want
    r = cli([bam, out])
    assert (r.returncode, r.stdout, r.stderr) == (0, b"", b"") and open(out, "rb").read() == want
    r = cli(["-c", "-t", "2", "-p", bam, out_c])
    assert (r.returncode, r.stdout, r.stderr) == (0, b"", b"") and open(out_c, "rb").read() == want
    sambamba_amd.build_index(bam, api, check_bins=True)
    assert open(api, "rb").read() == want


def test_generated_file_whole_and_in_batches(generated, tmp_path, monkeypatch):
    import sambamba_amd
    path, recs, _, want = generated
    assert len(recs) > 400 and len(want) > 1000
    out = str(tmp_path / "whole.bai")
    sambamba_amd.build_index(path, out, check_bins=True)
    assert open(out, "rb").read() == want
    r = cli(["-c", path, str(tmp_path / "cli.bai")], env={"SBX_INDEX_BATCH_BYTES": bc.BATCH, "SBX_TIMING": "1"})
    assert r.returncode == 0, r.stderr
    assert int(re.search(rb"build_index: (\d+) batch", r.stderr).group(1)) >= 3
    assert b"on the device" in r.stderr
    assert open(str(tmp_path / "cli.bai"), "rb").read() == want
    monkeypatch.setenv("SBX_INDEX_BATCH_BYTES", bc.BATCH)
    out_b = str(tmp_path / "batches.bai")
    sambamba_amd.build_index(path, out_b, check_bins=True)
    assert open(out_b, "rb").read() == want


def message(recs, bad):
    first = min(bad)
    return "Bin in read with name '%s' is set incorrectly (%d instead of expected %d); %d %s a wrong bin" % (
        bc.name_of(recs[first]), bad[first], bc.expected_bin(recs[first]), len(bad), "record of the file has" if len(bad) == 1 else "records of the file have")


def spoiled_cases(recs, first_b):
    n_placed_a = first_b - 1
    return {
        "first_batch": {5: 4682},
        "later_batch": {n_placed_a - 3: 0},
        "first_placed_record": {0: 37450},
        "chrB_later_batch": {first_b + 40: 4680},
        "three": {first_b + 7: 1, 17: 585, 200: 9},
    }


@pytest.mark.parametrize("case", ["first_batch", "later_batch", "first_placed_record", "chrB_later_batch", "three"])
@pytest.mark.parametrize("batched", [False, True])
def test_wrong_bins_are_refused(generated, tmp_path, monkeypatch, case, batched):
    import sambamba_amd
    _, recs, first_b, _ = generated
    bad = spoiled_cases(recs, first_b)[case]
    assert all(bc.expected_bin(recs[i]) != b for i, b in bad.items())
    path = str(tmp_path / "bad.bam")
    bc.write(path, bc.with_bins(recs, bad))
    if batched:
        monkeypatch.setenv("SBX_INDEX_BATCH_BYTES", bc.BATCH)
    out = str(tmp_path / "bad.bai")
    with pytest.raises(sambamba_amd.SbxError) as ei:
        sambamba_amd.build_index(path, out, check_bins=True)
    assert ei.value.code == EFORMAT and ei.value.msg == message(recs, bad)
    assert not os.path.exists(out)
    r = cli(["--check-bins", path])
    assert (r.returncode, r.stdout, r.stderr) == (1, b"", ("sbx-index: " + message(recs, bad) + "\n").encode())
    assert not os.path.exists(path + ".bai")
    # without -c the file indexes as before: the stored bins are what the index files the chunks under
    sambamba_amd.build_index(path, out)
    r = cli([path])
    assert r.returncode == 0 and open(path + ".bai", "rb").read() == open(out, "rb").read()


def test_records_that_are_not_placed_are_not_checked(generated, tmp_path):
    import sambamba_amd
    _, recs, first_b, _ = generated
    nopos, unmapped = first_b - 1, len(recs) - 3
    assert struct.unpack_from("<ii", recs[nopos], 4) == (1, -1) and struct.unpack_from("<ii", recs[unmapped], 4) == (-1, -1)
    path = str(tmp_path / "np.bam")
    bc.write(path, bc.with_bins(recs, {nopos: 1234, unmapped: 77}))
    sambamba_amd.build_index(path, str(tmp_path / "np.bai"), check_bins=True)
    r = cli(["-c", path])
    assert (r.returncode, r.stderr) == (0, b"")
    assert open(path + ".bai", "rb").read() == open(str(tmp_path / "np.bai"), "rb").read()


def test_unsorted_wins_over_a_wrong_bin(generated, tmp_path):
    """an unsorted file is SBX_ENOTSORTED as without -c, though the wrong bin comes first in the file"""
    import sambamba_amd
    _, recs, first_b, _ = generated
    swapped = bc.with_bins(recs, {3: 0})
    swapped[300], swapped[100] = swapped[100], swapped[300]
    path = str(tmp_path / "unsorted.bam")
    bc.write(path, swapped)
    codes = []
    for check in (False, True):
        with pytest.raises(sambamba_amd.SbxError) as ei:
            sambamba_amd.build_index(path, str(tmp_path / "u.bai"), check_bins=check)
        codes.append((ei.value.code, ei.value.msg))
    assert codes[0][0] == ENOTSORTED and codes[1] == codes[0]
    assert not os.path.exists(str(tmp_path / "u.bai"))
