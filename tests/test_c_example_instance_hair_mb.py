"""examples/instance_hair_mb_min.c - a quad scalp and a tuft of two-step flat B-spline curves in one scene, instanced four times, one
instance moving (device config inst_hair=1,inst_hair_mb=1) - builds against the public header on every machine and, on a GPU, runs with
its own checks."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, "embree-compressed_amd", "lib")


def _build(tmp_path, name="instance_hair_mb_min"):
    exe = str(tmp_path / name)
    subprocess.check_call(["gcc", "-std=c99", "-D_POSIX_C_SOURCE=200112L", "-O2", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "examples", name + ".c"), "-L" + LIBDIR, "-lembree3", "-lm", "-lpthread",
                           "-Wl,-rpath," + LIBDIR, "-o", exe])
    return exe


def test_instance_hair_mb_example_links(tmp_path):
    _build(tmp_path)


@pytest.mark.gpu
def test_instance_hair_mb_example_runs(tmp_path):
    exe = _build(tmp_path)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    print(out.stdout)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "instance_hair_mb_min: ok" in out.stdout and out.stdout.count("rays end on hair") == 12
