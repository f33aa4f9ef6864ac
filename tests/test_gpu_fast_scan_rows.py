"""Scan A of k_fast_rows on wide items (64 dwords per tile row) carries six tile rows and three pairs of vertical differences from one block
of 8 centre rows to the next instead of loading and reducing them again.  The masks must be the same bits whatever the item's height, its
number of blocks, what runs between two blocks (the corner pass, a spill), what the wave worked on before, and the threshold.  Each group of
cases runs tests/_fast_scan_rows_check.py in a process of its own, because the HS_FAST_* knobs are read when a handle is created and calls
this small would otherwise take the narrow items."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WIDE = {"HS_FAST_COLS": "64"}


@pytest.mark.parametrize("group,env", [
    ("heights", WIDE),                                               # interior height modulo 8: 8, 1, ... 7 valid rows in the last block
    ("cells", WIDE),                                                 # 1 to 16 blocks per item, the tall-tile instances
    ("noise", WIDE),                                                 # a saturated frame
    ("noise", dict(WIDE, HS_FAST_TEST_SMALL_LISTS="1")),             # the corner pass and the spill between two blocks
    ("batch", WIDE),                                                 # item after item on one wave, a single-row item
    ("batch", dict(WIDE, HS_FAST_NO_FOLD="1")),                      # ... with the waves on the work queues
    ("thresholds", WIDE),                                            # other biases
    ("narrow", {}),                                                  # the narrow items are what they were
])
def test_fast_scan_rows_in_subprocess(gpu, group, env):
    e = {k: v for k, v in os.environ.items() if not k.startswith("HS_FAST_")}
    e.update(env)
    e["PYTHONPATH"] = ROOT + os.pathsep + e.get("PYTHONPATH", "")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "_fast_scan_rows_check.py"), group], env=e, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "FAST_SCAN_ROWS_OK" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]
