"""Builds and runs one of the stand-alone sanitizer programs of tests/sanitize/: csrc/capi.cpp +
host_stubs.cpp + <name>.cpp under AddressSanitizer + UndefinedBehaviorSanitizer, on the CPU."""
import ctypes
import os
import shutil
import subprocess

import pytest

from conftest import ROOT


def run_check(name, tmp_path):
    """Compile tests/sanitize/<name>.cpp into a program with its own main and run it; returns its
    stdout (which must report "0 failed")."""
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("g++ not available")
    # The sanitizer runtimes are linked into the program itself, so it checks every allocation
    # whatever else the environment loads into processes.  Only when this Python process already
    # runs under an ASan runtime (tools/sanitize.sh leg 3, inherited by children) the program
    # links against that shared runtime instead: two runtimes in one process refuse to start.
    shared = hasattr(ctypes.CDLL(None), "__asan_init")
    rt = subprocess.run([gxx, "-print-file-name=" + ("libasan.so" if shared else "libasan.a")], capture_output=True,
                        text=True).stdout.strip()
    if not os.path.isabs(rt) or not os.path.exists(rt):
        pytest.skip("the ASan runtime of g++ is not installed")
    link = [] if shared else ["-static-libasan", "-static-libubsan"]
    hip_inc = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "include")
    if not os.path.exists(os.path.join(hip_inc, "hip", "hip_runtime.h")):
        pytest.skip("HIP headers not found")
    exe = str(tmp_path / name)
    san = os.path.join(ROOT, "tests", "sanitize")
    cmd = [gxx, "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-fno-omit-frame-pointer", "-g", "-O1", "-D__HIP_PLATFORM_AMD__", "-I", hip_inc,
           "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "forest-slam_amd", "csrc", "capi.cpp"),
           os.path.join(san, "host_stubs.cpp"), os.path.join(san, name + ".cpp"), "-o", exe] + link
    b = subprocess.run(cmd, capture_output=True, text=True)
    assert b.returncode == 0, b.stderr[-4000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([exe], capture_output=True, text=True, env=env)
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    assert "0 failed" in r.stdout
    return r.stdout
