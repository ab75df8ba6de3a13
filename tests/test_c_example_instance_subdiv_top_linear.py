"""examples/instance_subdiv_top_linear_min.c - a fast-moving instance of a displaced subdivision mesh beside a static one, traced on a
device without and on one with inst_subdiv_bounds=linear - builds against the public header on every machine and, on a GPU, runs with
its own checks under both leaf families."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, "embree-compressed_amd", "lib")


def _build(tmp_path, name="instance_subdiv_top_linear_min"):
    exe = str(tmp_path / name)
    subprocess.check_call(["gcc", "-std=c99", "-D_POSIX_C_SOURCE=200112L", "-O2", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "examples", name + ".c"), "-L" + LIBDIR, "-lembree3", "-lm", "-lpthread",
                           "-Wl,-rpath," + LIBDIR, "-o", exe])
    return exe


def test_instance_subdiv_top_linear_example_links(tmp_path):
    _build(tmp_path)


@pytest.mark.gpu
@pytest.mark.parametrize("config,kinds", [("", (24, 34)), ("subdiv_accel=bvh4.compressed.leaf", (25, 35))])
def test_instance_subdiv_top_linear_example_runs(tmp_path, config, kinds):
    exe = _build(tmp_path)
    out = subprocess.run([exe] + ([config] if config else []), capture_output=True, text=True, timeout=300)
    print(out.stdout)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "instance_subdiv_top_linear_min: ok" in out.stdout
    assert "accel kind %d, 2 instances" % kinds[0] in out.stdout and "accel kind %d, 2 instances" % kinds[1] in out.stdout
    assert "5 meet the mover where it is at their time, 5 the static instance" in out.stdout
