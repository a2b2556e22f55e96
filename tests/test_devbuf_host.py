"""The owner types of modelmesh_amd/csrc/devbuf.hpp on the host: tests/devbuf_host/devbuf_test.cc compiled with the host C++
compiler against counting stand-ins for the four HIP calls, and run.  No GPU, no HIP headers."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_devbuf_host_program(tmp_path):
    cxx = shutil.which("c++") or shutil.which("g++")
    if cxx is None:
        pytest.fail("no host C++ compiler (c++ / g++) on PATH")
    exe = str(tmp_path / "devbuf_test")
    subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", os.path.join(ROOT, "tests", "devbuf_host", "devbuf_test.cc"),
                    "-o", exe], check=True)
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "devbuf_test ok" in run.stdout
