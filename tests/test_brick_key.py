"""The host brick-key codec (noetic-slam_amd/csrc/brick_key.h: pack, coordinate, range rule, the
(z, y, x) order of export and mesh, the mesh halo's needed keys) built with g++ and checked on the
CPU against naive restatements (tests/cpp/brick_key_check.cpp)."""
import os
import subprocess

from conftest import REPO

SRC = os.path.join(REPO, "tests", "cpp", "brick_key_check.cpp")


def test_brick_key_check(tmp_path):
    exe = tmp_path / "brick_key_check"
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-o", str(exe), SRC])
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert out.stdout.startswith("ok")


def test_brick_key_sanitizers(tmp_path):
    """The same program under AddressSanitizer and UndefinedBehaviorSanitizer: no signed overflow
    in the bias arithmetic, no shift past a field, no read past the key lists."""
    exe = tmp_path / "brick_key_san"
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-o", str(exe), SRC])
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and out.stdout.startswith("ok"), out.stdout + out.stderr[-3000:]
    assert "runtime error" not in out.stderr and "Sanitizer" not in out.stderr, out.stderr[-3000:]
