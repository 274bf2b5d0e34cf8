"""bench.py's command line and input lookup (CPU): a plain run is the default, and the BAM is taken from the input cache build()
fills only when the copy there is complete."""
import os
import sys

from tests.util import ROOT

sys.path.insert(0, ROOT)
import bench  # noqa: E402


def test_plain_run_is_the_default():
    args = bench.parser().parse_args(["--gpus", "1", "--steps", "7", "--warmup", "2"])
    assert args.steps == 7 and args.warmup == 2 and not args.full and args.dump_outputs is None
    args = bench.parser().parse_args(["--full", "--dump-outputs", "out"])
    assert args.full and args.dump_outputs == "out"


def test_the_cached_input_is_used_only_when_complete(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "input_cache_dir", lambda: str(tmp_path))
    key = ("chr1:1000", 30.0, 0x5A4D0002, 6, "zlib", [])
    assert os.path.dirname(bench.bam_path(*key)) == bench.tmp_dir()
    cached = tmp_path / os.path.basename(bench.bam_path(*key))
    for suffix in ("", ".bai"):
        (tmp_path / (cached.name + suffix)).write_bytes(b"x")
        assert os.path.dirname(bench.bam_path(*key)) == bench.tmp_dir()
    (tmp_path / (cached.name + ".json")).write_text("{}")
    assert bench.bam_path(*key) == str(cached)
