"""The host input helpers (noetic-slam_amd/csrc/host_pack.h: the record -> packed-xyz packer, the
index-share pack, the host split's sector rule and the scheduler over the contexts' staging pools)
built with g++ and checked on the CPU against naive restatements, bit for bit
(tests/cpp/host_pack_check.cpp)."""
import os
import subprocess

from conftest import REPO

SRC = os.path.join(REPO, "tests", "cpp", "host_pack_check.cpp")


def test_host_pack_check(tmp_path):
    exe = tmp_path / "host_pack_check"
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-pthread", "-Wall", "-o", str(exe), SRC])
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert out.stdout.startswith("ok")


def test_host_pack_sanitizers(tmp_path):
    """The same program under AddressSanitizer and UndefinedBehaviorSanitizer (host code only): no
    read past a record, no write past a destination, no misaligned access."""
    exe = tmp_path / "host_pack_san"
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-pthread",
                           "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-o", str(exe), SRC])
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and out.stdout.startswith("ok"), out.stdout + out.stderr[-3000:]
    assert "runtime error" not in out.stderr and "Sanitizer" not in out.stderr, out.stderr[-3000:]
