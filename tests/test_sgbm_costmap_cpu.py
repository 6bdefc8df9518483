"""The SGBM cost tile's index maps (csrc/sgbm_costmap.h: pixel-cost task -> left record, right
records and output offset; the BT record offsets; a lane's box-sum runs) walked on the CPU for
every cost-pass shape the library dispatches: tests/sgbm_costmap_check.cpp, a stand-alone host
program over the same header the kernel includes.  No GPU."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_cost_tile_maps_cover_the_tile_in_bounds_and_aligned(tmp_path):
    """D in {64, 96, 128} x (lanes, cols) in {(4, 32), (4, 64), (8, 16), (8, 32), (16, 32)}, the
    block at the first, an interior and the last partial position: every tile cell written exactly
    once, every read inside its array (and inside the part the BT phase writes), every 8- and
    16-byte access aligned, 8-byte reads of a 32-lane group on distinct banks."""
    gxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if gxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path / "sgbm_costmap_check")
    b = subprocess.run([gxx, "-std=c++17", "-O1", "-Wall",os.path.join(ROOT, "tests", "sgbm_costmap_check.cpp"),
                        "-o", exe], capture_output=True, text=True)
    assert b.returncode == 0, b.stderr[-4000:]
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    last = r.stdout.strip().splitlines()[-1]
    assert last.endswith(" 0 failed") and int(last.split()[0]) > 100000, last
