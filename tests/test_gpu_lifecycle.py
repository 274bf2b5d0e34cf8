"""Opening and closing a context gives back what it took: the four pinned staging buffers of the upload ring (32 MiB each), the
pinned result block, the events and the three streams all belong to the context (host_res.hpp) and leave with it.  The sharded
CLI, dist_depth.py and this suite open and close many contexts per process."""
import json
import os
import subprocess
import sys

import pytest

from tests.conftest import GOLDEN, ROOT

pytestmark = pytest.mark.gpu

WARMUP_CYCLES, CYCLES = 2, 16

# runs in a process of its own: the figures are those of the process, and nothing else may allocate next to the cycles
CHILD = r"""
import json, sys
sys.path.insert(0, sys.argv[1])
import sambamba_amd

def status():
    out = {}
    with open("/proc/self/status") as fh:
        for line in fh:
            k, _, v = line.partition(":")
            if k in ("VmRSS", "VmLck", "VmPin"):
                out[k] = int(v.split()[0])          # kB
    return out

def cycle():
    # no preload(): the file bytes travel through the staging ring (upload_ranges), which a run then reports as ms_h2d
    with sambamba_amd.Depth(sys.argv[2]) as d:
        d.set_params()
        st = d.run()
        assert st["n_records"] > 0 and st["uploaded_bytes"] > 0 and st["ms_h2d"] > 0, st

for _ in range(int(sys.argv[3])):
    cycle()
before = status()
for _ in range(int(sys.argv[4])):
    cycle()
print(json.dumps({"before": before, "after": status()}))
"""


def test_open_run_close_cycles_do_not_grow_the_process():
    """A context that used the staging ring once left two of its four 32 MiB pinned buffers behind when it was closed: 16 cycles
    grew VmRSS by 1,048,576 kB, exactly 16 x 2 x 32 MiB (VmLck and VmPin stayed 0).  The bound is
    a quarter of that -- far above what an allocator keeps back, far below the leak."""
    bam = os.path.join(GOLDEN, "issue225.bam")
    out = subprocess.run([sys.executable, "-c", CHILD, ROOT, bam, str(WARMUP_CYCLES), str(CYCLES)], check=True,
                         stdout=subprocess.PIPE, universal_newlines=True, timeout=300).stdout
    r = json.loads(out.strip().splitlines()[-1])
    growth = {k: r["after"][k] - r["before"][k] for k in r["before"]}
    print("kB before %s, after %s, growth over %d cycles %s" % (r["before"], r["after"], CYCLES, growth))
    assert growth["VmRSS"] < 256 * 1024, growth
