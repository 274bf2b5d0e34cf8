"""The host-only helpers of the standalone entry points (sambamba_amd/csrc/entry_util.hpp: the text-to-caller-buffer copy, the
malformed-records message, the output guard's unlink-unless-disarmed, the same-file test, the decimal environment hook and what the
six size hooks make of it, the output file with its latched write failure and its EOF block), compiled for the host with g++ and
-fsanitize=address,undefined into tests/native/entry_host.cpp and run as a program of their own -- no GPU, no Python in the process."""
import os
import subprocess

from tests.util import ROOT

SRC = os.path.join(ROOT, "tests", "native", "entry_host.cpp")


def test_entry_helpers_under_the_sanitizers(tmp_path):
    exe = str(tmp_path / "entry_host")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-o", exe, SRC])
    work = tmp_path / "work"
    work.mkdir()
    r = subprocess.run([exe, str(work)], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert (r.returncode, r.stdout) == (0, b"ok\n"), r.stderr.decode()
