"""The command line of sbx-import (sambamba_amd/csrc/import_cli.cpp) where it needs no device: the usage text, every refusal by name,
the reference's message for a region argument, and the exit statuses."""
import os
import subprocess

import pytest

import sambamba_amd
from tests.util import ROOT

SAM = os.path.join(ROOT, "tests", "golden", "issue_356.sam")


def run(*args):
    r = subprocess.run([sambamba_amd.import_cli_path()] + list(args), stdout=subprocess.PIPE, stderr=subprocess.PIPE, stdin=subprocess.DEVNULL)
    return r.returncode, r.stdout, r.stderr.decode()


def test_usage_without_arguments():
    rc, out, err = run()
    assert rc == 0 and out == b""
    assert err.startswith("Usage: sbx-import [-S] [-f bam] [-o out.bam] [-l level] [-h] [-t N] [-p] <input.sam>|-\n")
    for word in ("--sam-input", "--format=bam", "--output-filename", "--compression-level", "--with-header", "--nthreads", "--show-progress"):
        assert word in err
    # options alone are no input either
    rc, out, err = run("-S", "-f", "bam", "-h", "-p", "-t", "4")
    assert rc == 0 and err.startswith("Usage: sbx-import")


@pytest.mark.parametrize("args,name", [(["-F", "mapping_quality > 0"], "-F / --filter"), (["--filter=unmapped"], "-F / --filter"),
                                       (["--num-filter=4/"], "--num-filter"), (["-s", "0.5"], "-s / --subsample"),
                                       (["-L", "x.bed"], "-L / --regions"), (["-c"], "-c / --count"), (["--count"], "-c / --count"),
                                       (["-v"], "-v / --valid")])
def test_selection_is_refused_by_name(args, name):
    for order in (args + [SAM], [SAM] + args):
        rc, out, err = run(*order)
        assert rc == 1 and out == b""
        assert err == "sbx-import: option %s is not supported: records of SAM input are not selected\n" % name


@pytest.mark.parametrize("fmt", ["sam", "json", "msgpack", "unpack", "cram"])
def test_other_formats_are_refused_by_name(fmt):
    rc, out, err = run("-S", "-f", fmt, SAM)
    assert rc == 1 and out == b""
    assert err == "sbx-import: output format %s is not supported: sbx-import writes BAM (-f bam)\n" % fmt


def test_unknown_format_and_options():
    assert run("-f", "bed", SAM)[0::2] == (1, "sbx-import: output format must be one of sam, bam, json\n")
    assert run("--frobnicate", SAM)[0::2] == (1, "sbx-import: Unrecognized option --frobnicate\n")
    assert run("-Sx", SAM)[0::2] == (1, "sbx-import: Unrecognized option -Sx\n")
    assert run(SAM, "-o")[0::2] == (1, "sbx-import: Missing value for argument -o.\n")
    assert run("-l", "10", SAM)[0::2] == (1, "sbx-import: invalid compression level 10\n")
    assert run("-l", "fast", SAM)[0::2] == (1, "sbx-import: invalid compression level fast\n")


def test_region_arguments_get_the_reference_message():
    for args in ([SAM, "chr1"], ["-S", "-f", "bam", SAM, "chr1:1-100", "chr2"], ["--", SAM, "*"]):
        rc, out, err = run(*args)
        assert rc == 1 and out == b"" and err == "region queries are unavailable for SAM input\n"


def test_view_and_sam_keep_refusing_sam_input():
    for exe in (sambamba_amd.view_cli_path(), sambamba_amd.sam_cli_path()):
        r = subprocess.run([exe, "-S", SAM], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
        assert r.returncode == 1 and r.stderr.decode().endswith("option -S / --sam-input is not supported\n")
