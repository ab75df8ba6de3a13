"""examples/round_curve_min.c - three tubes (a straight and a tapered round Bezier curve, a round B-spline curve) on a device created with
round_curves=1, ten rays with known answers, RTC_DEVICE_PROPERTY_CURVE_GEOMETRY_SUPPORTED printing 1 - builds against the public header
on every machine and, on a GPU, runs with its own checks."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, "embree-compressed_amd", "lib")


def _build(tmp_path, name="round_curve_min"):
    exe = str(tmp_path / name)
    subprocess.check_call(["gcc", "-std=c99", "-D_POSIX_C_SOURCE=200112L", "-O2", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "examples", name + ".c"), "-L" + LIBDIR, "-lembree3", "-lm", "-lpthread",
                           "-Wl,-rpath," + LIBDIR, "-o", exe])
    return exe


def test_round_curve_example_links(tmp_path):
    _build(tmp_path)


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["", "robust"])
def test_round_curve_example_runs(tmp_path, mode):
    exe = _build(tmp_path)
    out = subprocess.run([exe, "", mode], capture_output=True, text=True, timeout=300)
    print(out.stdout)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "RTC_DEVICE_PROPERTY_CURVE_GEOMETRY_SUPPORTED = 1" in out.stdout and "round_curve_min: ok (10 rays)" in out.stdout
