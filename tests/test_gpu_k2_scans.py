"""The two scans of K2 (index.hip) across their rounds of 4096 items: `k_check_scan` over the BGZF blocks of a launch and
`k_tile_compact` over the position tiles, each in both launch shapes -- the look-back over several workgroups (the default) and the
single workgroup that loops over the rounds (SBX_K2_SCAN=0, also what a launch of more than 4094 rounds gets).

Files from tests/bamgen.py with 4095 / 4096 / 4097 / 8193 blocks or tiles: up to one round, one round, one round and one item, two
rounds and a third workgroup -- the first that adds up more than one predecessor in its look-back.  Every case runs the CLI in a
child process (the switch is read once per process) with SBX_DEBUG=1 and asserts the `blocks=` / `tiles=` figure of the `[sbx]`
line, so that it is known to sit where it claims; the text must equal the oracle's."""
import random
import re

import numpy as np
import pytest

from tests import bamgen as bg
from tests.util import oracle_base_counters, run_cli, run_oracle

pytestmark = pytest.mark.gpu

MODES = {"lookback": {}, "single_workgroup": {"SBX_K2_SCAN": "0"}}
ROUND = 4096            # items of one round of either scan (kScanPerWg)
BLOCK = 128             # bytes of a BGZF block of the block files
TILE = 1024             # positions of a tile with one sample


def _record(rng, pos, i, tags=b""):
    """77 .. 122 bytes with the block_size field: no longer than a block, so every block holds a record start, and nearly
    every record straddles two blocks"""
    n = rng.randint(20, 50)
    return bg.make_record(0, pos, "%dM" % n, "".join(rng.choices("ACGT", k=n)), rng.choices([2, 12, 23, 37], k=n), name="r%05d" % i, tags=tags)


def _blocks_bam(path, n_blocks, decoy_block=None):
    """A BAM whose launch has exactly n_blocks BGZF blocks (the header's block and the record blocks; the empty last block of
    a BGZF file is not part of it).  decoy_block: the file goes on for a few blocks behind that index, and a record there carries the decoy
    of test_decoy_records_inside_a_tag_cannot_change_results with a block cut at its first byte; returns (blocks of the launch,
    records, index of the decoy's block)."""
    rng = random.Random(n_blocks or decoy_block)
    refs = [("c1", 2000000)]
    hdr_len = len(bg.bam_header("@HD\tVN:1.6\tSO:coordinate\n@SQ\tSN:c1\tLN:2000000\n", refs))
    assert hdr_len < BLOCK          # the first record lies in block 0: the launch starts there
    fake = b"".join(bg.make_record(0, 100 + 10 * k, "50M", "".join(rng.choices("ACGT", k=50)), 30, name="fake%d" % k) for k in range(3))
    raw, size, pos, decoy_at = [], hdr_len, 10, None
    limit = n_blocks * BLOCK if decoy_block is None else (decoy_block + 12) * BLOCK
    while True:
        if decoy_block is not None and decoy_at is None and size >= decoy_block * BLOCK:
            r = _record(rng, pos, len(raw), tags=bg.tag_bytes("XD", fake))
            decoy_at = size + r.index(fake)
        else:
            r = _record(rng, pos, len(raw))
        if size + len(r) > limit:
            break
        raw.append(r)
        size += len(r)
        pos += rng.randint(5, 40)
    info = bg.write_bam(path, refs, raw, block_size=BLOCK, cuts=[decoy_at] if decoy_at else None, level=1)
    assert info["stream_len"] == size
    blocks = len(info["pieces"])
    if decoy_block is None:
        assert blocks == n_blocks
        return blocks, len(raw), None
    return blocks, len(raw), [o for o, _ in info["pieces"]].index(decoy_at)


def _tiles_bam(path, n_tiles):
    """One contig whose tile grid has n_tiles tiles, its one spare tile included.  Reads in the first tile, in the tiles on both
    sides of index 4096 and 8192, in the last tile of the contig and -- hanging over its end -- in the spare tile; three records
    in the first tile of every round and in the spare tile, one elsewhere.  Returns the touched tiles."""
    rng = random.Random(n_tiles)
    length = (n_tiles - 1) * TILE
    tiles = sorted(t for t in {0, ROUND - 1, ROUND, ROUND + 1, 2 * ROUND - 1, 2 * ROUND, n_tiles - 2} if t <= n_tiles - 2)
    starts = [t * TILE + 100 + 7 * j for t in tiles for j in range(3 if t % ROUND == 0 else 1)] + [length - 30 + 5 * j for j in range(3)]
    raw = [bg.make_record(0, p, "50M", "".join(rng.choices("ACGT", k=50)), rng.choices([2, 12, 23, 37], k=50), name="t%d" % i)
           for i, p in enumerate(sorted(starts))]
    bg.write_bam(path, [("c1", length)], raw)
    return tiles + [n_tiles - 1]


def _run(path, env, extra_env=None):
    """`base` through the CLI in a child process; returns (text, the figures of the [sbx] line, first_bad of the first attempt)"""
    r = run_cli(["base", path], check=False, env=dict(env, SBX_DEBUG="1", **(extra_env or {})))
    err = r.stderr.decode()
    assert r.returncode == 0, err
    line = [ln for ln in err.splitlines() if ln.startswith("[sbx] blocks=")][-1]
    first_bad = int(re.search(r"index attempt 0: .* first_bad=(\d+)", err).group(1))
    return r.stdout, {k: int(v) for k, v in re.findall(r"(\w+)=(\d+)", line)}, first_bad


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    """every file of the module and the oracle's text for it, made on first use and shared by the two modes"""
    d = tmp_path_factory.mktemp("k2scans")
    made = {}

    def get(kind, n):
        if (kind, n) not in made:
            path = str(d / ("%s%d.bam" % (kind, n)))
            if kind == "blocks":
                what = _blocks_bam(path, n)
            elif kind == "decoy":
                what = _blocks_bam(path, None, decoy_block=n)
            else:
                what = _tiles_bam(path, n)
            made[(kind, n)] = (path, what, run_oracle(["base", path]))
        return made[(kind, n)]
    return get


@pytest.mark.parametrize("mode", sorted(MODES))
@pytest.mark.parametrize("n_blocks", [ROUND - 1, ROUND, ROUND + 1, 2 * ROUND + 1])
def test_check_scan_across_rounds_of_blocks(files, n_blocks, mode):
    path, (blocks, n_records, _), want = files("blocks", n_blocks)
    got, fig, _ = _run(path, MODES[mode])
    assert fig["blocks"] == blocks == n_blocks
    assert fig["records"] == n_records
    assert got == want


@pytest.mark.parametrize("mode", sorted(MODES))
def test_inconsistent_chain_behind_the_second_round(files, mode):
    """The guesser takes the decoy in a block behind index 8192: the lowest inconsistent block is found in the third round -- by
    a late workgroup, through atomicMin on flags[0], in the look-back shape -- and the repaired chain gives the oracle's text."""
    path, (blocks, n_records, decoy_block), want = files("decoy", 2 * ROUND + 4)
    assert decoy_block > 2 * ROUND and blocks > decoy_block + 1
    got, fig, first_bad = _run(path, MODES[mode])
    assert fig["blocks"] == blocks
    assert 2 * ROUND < first_bad <= decoy_block         # (the blocks inside the long record in front of the decoy hold no record start)
    assert fig["rewalked_blocks"] > 0
    assert fig["records"] == n_records
    assert got == want


@pytest.mark.parametrize("mode", sorted(MODES))
@pytest.mark.parametrize("n_tiles", [ROUND - 1, ROUND, ROUND + 1, 2 * ROUND + 1])
def test_tile_compact_across_rounds_of_tiles(files, n_tiles, mode):
    path, touched, want = files("tiles", n_tiles)
    got, fig, _ = _run(path, MODES[mode])
    assert fig["tiles"] == n_tiles and fig["T"] == TILE
    assert fig["active"] == len(touched)
    assert got == want


@pytest.mark.parametrize("mode", sorted(MODES))
def test_deep_tiles_are_counted_over_all_rounds(files, mode):
    """With the limit at three records the first tile of every round and the spare tile are deep: n_active[1] is summed over the
    workgroups, and K3 leaves exactly those tiles to its 32-bit kernel (a wrong count drops or doubles their columns)."""
    n_tiles = 2 * ROUND + 1
    path, touched, want = files("tiles", n_tiles)
    got, fig, _ = _run(path, MODES[mode], {"SBX_DEEP_TILE_RECORDS": "3"})
    assert fig["tiles"] == n_tiles and fig["active"] == len(touched)
    assert got == want


@pytest.mark.parametrize("n_tiles", [ROUND - 1, ROUND, ROUND + 1, 2 * ROUND + 1])
def test_counters_of_the_touched_tiles(files, n_tiles):
    import sambamba_amd
    path, touched, _ = files("tiles", n_tiles)
    with sambamba_amd.Depth(path) as d:
        d.set_params()
        d.run()
        for t in touched:
            got = d.base_counters(0, t * TILE, (t + 1) * TILE)
            assert got.any(), t
            assert np.array_equal(got, oracle_base_counters(path, 0, t * TILE, (t + 1) * TILE)), t
