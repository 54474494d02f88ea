"""The walk kernels' ray-tile map and its column detector (noetic-slam_amd/csrc/ray_tile.h), built
with g++ and checked on the CPU (tests/cpp/ray_tile_check.cpp): the map is a bijection of a scan's
points with at most 1024 per block for every column height, with and without a remainder; H = 0 is
the identity; the detector accepts intact grids and rejects damaged ones."""
import os
import subprocess

from conftest import REPO

SRC = os.path.join(REPO, "tests", "cpp", "ray_tile_check.cpp")


def test_ray_tile_check(tmp_path):
    exe = tmp_path / "ray_tile_check"
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-o", str(exe), SRC])
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert out.stdout.startswith("ok")


def test_ray_tile_sanitizers(tmp_path):
    """The same program under AddressSanitizer and UndefinedBehaviorSanitizer (host code only): the
    detector reads no point outside the scan."""
    exe = tmp_path / "ray_tile_san"
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17",
                           "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-o", str(exe), SRC])
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and out.stdout.startswith("ok"), out.stdout + out.stderr[-3000:]
    assert "runtime error" not in out.stderr and "Sanitizer" not in out.stderr, out.stderr[-3000:]
