"""The partition geometry of the dense groupby (csrc/dense_partition.h),
checked by a stand-alone host program built with the address and
undefined-behaviour sanitizers.  No GPU and no extension is involved."""

import os
import shutil
import subprocess

import pytest

_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _compiler():
    for name in ("g++", "clang++", "c++"):
        path = shutil.which(name)
        if path:
            return path
    return None


def test_geometry_program_under_sanitizers(tmp_path):
    cxx = _compiler()
    if cxx is None:
        pytest.fail("no host C++ compiler found")
    exe = tmp_path / "dense_partition_geometry"
    subprocess.run(
        [cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined",
         "-fno-sanitize-recover=all", "-I", os.path.join(_ROOT, "csrc"),
         os.path.join(_ROOT, "tests", "dense_partition_geometry_main.cpp"),
         "-o", str(exe)],
        check=True, capture_output=True, text=True)
    run = subprocess.run([str(exe)], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "cases OK" in run.stdout
