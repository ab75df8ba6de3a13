"""examples/instance_subdiv_min.c - a cube as a subdivision mesh, placed three times - builds against the public header on every machine
and, on a GPU, runs under the eager accel and under bvh4.compressed.leaf with its own checks."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, "embree-compressed_amd", "lib")


def _build(tmp_path, name="instance_subdiv_min"):
    exe = str(tmp_path / name)
    subprocess.check_call(["gcc", "-std=c99", "-D_POSIX_C_SOURCE=200112L", "-O2", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "examples", name + ".c"), "-L" + LIBDIR, "-lembree3", "-lm", "-lpthread",
                           "-Wl,-rpath," + LIBDIR, "-o", exe])
    return exe


def test_instance_subdiv_example_links(tmp_path):
    _build(tmp_path)


@pytest.mark.gpu
@pytest.mark.parametrize("cfg", ["gpu=0", "gpu=0,subdiv_accel=bvh4.compressed.leaf"])
def test_instance_subdiv_example_runs(tmp_path, cfg):
    exe = _build(tmp_path)
    out = subprocess.run([exe, cfg], capture_output=True, text=True, timeout=300)
    print(out.stdout)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "instance_subdiv_min: ok" in out.stdout and out.stdout.count("geomID 0 primID 3") == 3
