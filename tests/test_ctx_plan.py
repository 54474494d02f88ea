"""The context's sizing plan (noetic-slam_amd/csrc/ctx_plan.h: the band a ray's walk covers, the
per-ray slot bounds, one batch's sizes with tsdf_create's two refusals, the F64 gate's threshold and
the parameter validation) built with g++ and checked on the CPU against a straight-line restatement,
field by field (tests/cpp/ctx_plan_check.cpp)."""
import os
import subprocess

from conftest import REPO

SRC = os.path.join(REPO, "tests", "cpp", "ctx_plan_check.cpp")


def test_ctx_plan_check(tmp_path):
    exe = tmp_path / "ctx_plan_check"
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-o", str(exe), SRC])
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert out.stdout.startswith("ok")


def test_ctx_plan_sanitizers(tmp_path):
    """The same program under AddressSanitizer and UndefinedBehaviorSanitizer (host code only): no
    overflowing shift or signed arithmetic in the sizing, no read past a text buffer."""
    exe = tmp_path / "ctx_plan_san"
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17",
                           "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-o", str(exe), SRC])
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and out.stdout.startswith("ok"), out.stdout + out.stderr[-3000:]
    assert "runtime error" not in out.stderr and "Sanitizer" not in out.stderr, out.stderr[-3000:]
