"""The host arithmetic of the distance field (noetic-slam_amd/csrc/esdf_plan.h: the argument rules
of include/tsdf_hip_esdf.h, the tiles of the three passes with their LDS bytes, the scratch) built
with g++ and checked on the CPU against a Python restatement over a grid
(tests/cpp/esdf_plan_check.cpp answers the queries), plain and under ASan + UBSan."""
import math
import os
import re
import struct
import subprocess

from conftest import REPO

SRC = os.path.join(REPO, "tests", "cpp", "esdf_plan_check.cpp")
I64_MIN, I64_MAX = -(1 << 63), (1 << 63) - 1
OK, RADIUS, BAND, WEIGHT, ORDER, EXTENT, SIZE = range(7)
MAX_VOXELS = 1 << 28
LANES, X_LINES, GRID_CAP = 64, 16, 8192
LDS_PER_CU = 160 << 10
LDS_STATIC = 256


def f32(x):
    return struct.unpack("f", struct.pack("f", x))[0]


def check(lo, hi, radius, band, min_w):
    """The header's argument rules in the order they are reported, and the box."""
    none = (0, 0, 0, 0)
    if radius == 0 or radius > 128:
        return (RADIUS,) + none
    if not band >= 0.0 or math.isinf(band):
        return (BAND,) + none
    if not min_w >= 0.0:
        return (WEIGHT,) + none
    if any(h < l for l, h in zip(lo, hi)):
        return (ORDER,) + none
    n = [h - l for l, h in zip(lo, hi)]
    if any(e >= 1 << 31 for e in n):
        return (EXTENT,) + none
    total = n[0] * n[1] * n[2]
    if total > MAX_VOXELS:
        return (SIZE,) + none
    return (OK, n[0], n[1], n[2], total)


def seg(radius):
    return 32 if radius <= 48 else 64


def tiles(radius, n):
    cd = lambda a, b: -(-a // b)  # noqa: E731
    h = [min(radius, e - 1) if e else 0 for e in n]
    tx = cd(n[0], LANES) * cd(n[1] * n[2], X_LINES)
    return (seg(radius), h[0], h[1], h[2], X_LINES * (LANES + 2 * h[0]) * 2,
            (seg(radius) + 2 * h[1]) * LANES * 2, (seg(radius) + 2 * h[2]) * LANES * 2, tx,
            cd(n[0], LANES) * cd(n[1], seg(radius)) * n[2],
            cd(n[0] * n[1], LANES) * cd(n[2], seg(radius)), max(1, min(tx, GRID_CAP)),
            5 * n[0] * n[1] * n[2])


def arg_grid():
    box = ([0, 0, 0], [4, 5, 6])
    out = [(box[0], box[1], r, 0.1, 0.0) for r in (0, 1, 2, 127, 128, 129, 1 << 31, (1 << 32) - 1)]
    out += [(box[0], box[1], 3, b, 0.0) for b in
            (0.0, -0.0, 1e-30, 3e38, -1e-30, -1.0, math.inf, -math.inf, math.nan)]
    out += [(box[0], box[1], 3, 0.1, w) for w in
            (0.0, -0.0, 2.0, math.inf, -1e-30, -math.inf, math.nan)]
    # the first broken rule is the one reported
    out += [(box[0], box[1], 0, -1.0, -1.0), (box[0], box[1], 3, -1.0, -1.0),
            ([0, 0, 0], [-1, 5, 6], 3, 0.1, -1.0), ([0, 0, 0], [-1, 1 << 40, 6], 3, 0.1, 0.0),
            ([0, 0, 0], [1 << 40, 1, -1], 3, 0.1, 0.0)]
    los = (0, -5, 1 << 23, -(1 << 23) - 3, I64_MIN, I64_MAX - 7, -(1 << 62))
    exts = (0, 1, 7, 64, 65, (1 << 31) - 1, 1 << 31, 1 << 40)
    for l in los:
        for e in exts:
            if l + e <= I64_MAX:
                out.append(([l, 0, -3], [l + e, 1, -2], 5, 0.05, 0.0))
                out.append(([1, l, 0], [2, l + e, 0], 5, 0.05, 0.0))  # an empty box of any length
            if l - 1 >= I64_MIN:
                out.append(([0, l, 0], [1, l - 1, 1], 5, 0.05, 0.0))
    out.append(([I64_MIN] * 3, [I64_MAX] * 3, 5, 0.05, 0.0))
    # around the 2^28 bound, and products that overflow 64 bits
    for n in ([1 << 14, 1 << 14, 1], [1 << 14, 1 << 14, 2], [1 << 28, 1, 1], [(1 << 28) + 1, 1, 1],
              [1 << 10, 1 << 10, 1 << 8], [1 << 10, 1 << 10, (1 << 8) + 1], [645, 645, 645],
              [646, 646, 646], [(1 << 31) - 1] * 3, [(1 << 31) - 1, (1 << 31) - 1, 0],
              [1 << 20, 1 << 20, 1 << 24]):
        out.append(([-7, 3, -(1 << 30)], [-7 + n[0], 3 + n[1], -(1 << 30) + n[2]], 128, 0.1, 1.0))
    return out


def tile_grid():
    shapes = [(1, 1, 1), (97, 1, 1), (1, 80, 33), (2, 3, 130), (67, 45, 21), (600, 9, 5),
              (97, 80, 33), (400, 400, 80), (64, 16, 32), (65, 17, 33), (1 << 28, 1, 1),
              (1, 1 << 28, 1), (1, 1, 1 << 28), (1 << 14, 1 << 14, 1), (0, 5, 5), (5, 0, 5)]
    return [(r, n) for r in (1, 2, 12, 20, 40, 48, 49, 127, 128) for n in shapes]


def queries():
    q, want = [], []
    for lo, hi, r, band, mw in arg_grid():
        band, mw = f32(band), f32(mw)
        q.append("A %d %d %d %d %d %d %d %s %s" % (*lo, *hi, r, float(band).hex(), float(mw).hex()))
        want.append("%d %d %d %d %d" % check(lo, hi, r, band, mw))
    for r, n in tile_grid():
        q.append("T %d %d %d %d" % (r, *n))
        want.append(" ".join("%d" % v for v in tiles(r, n)))
    return q, want


def run_and_compare(exe):
    q, want = queries()
    out = subprocess.run([str(exe)], input="\n".join(q) + "\n", capture_output=True, text=True,
                         timeout=300)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-3000:]
    got = out.stdout.split("\n")
    assert got[len(q)] == "ok %d" % len(q)
    bad = [(a, b, c) for a, b, c in zip(q, got, want) if b != c]
    assert not bad, bad[:10]
    return out


def test_the_stated_rules_on_known_cases():
    assert check([0] * 3, [1] * 3, 0, 0.1, 0.0)[0] == RADIUS
    assert check([0] * 3, [1] * 3, 129, 0.1, 0.0)[0] == RADIUS
    assert check([0] * 3, [1] * 3, 128, math.nan, 0.0)[0] == BAND
    assert check([0] * 3, [1] * 3, 128, 0.0, math.nan)[0] == WEIGHT
    assert check([0] * 3, [1, -1, 1], 1, 0.0, 0.0)[0] == ORDER
    assert check([0] * 3, [1, 1 << 31, 1], 1, 0.0, 0.0)[0] == EXTENT
    assert check([0] * 3, [1 << 14, 1 << 14, 2], 1, 0.0, 0.0)[0] == SIZE
    assert check([0] * 3, [1 << 14, 1 << 14, 1], 1, 0.0, 0.0) == (OK, 1 << 14, 1 << 14, 1, 1 << 28)
    assert check([0] * 3, [5, 0, (1 << 31) - 1], 1, 0.0, 0.0) == (OK, 5, 0, (1 << 31) - 1, 0)
    seen = {check(*a)[0] for a in arg_grid()}
    assert seen == set(range(7))


def test_tiles_fit_the_chip():
    """At least two workgroups of any pass fit a CU's LDS for every radius (four, in fact, and
    three at R = 128; the tile and the 256 bytes of the workgroup vote beside it); no 16-bit plane
    can overflow; the largest scratch is 1.25 GiB."""
    for r in range(1, 129):
        fit = 4 if r < 128 else 3
        assert ((seg(r) + 2 * r) * LANES * 2 + LDS_STATIC) * fit <= LDS_PER_CU
        assert (X_LINES * (LANES + 2 * r) * 2 + LDS_STATIC) * 4 <= LDS_PER_CU
    assert 3 * 128 * 128 < 0xFFFF
    assert 5 * MAX_VOXELS == 1280 << 20


def test_esdf_plan_check(tmp_path):
    exe = tmp_path / "esdf_plan_check"
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-o", str(exe), SRC])
    run_and_compare(exe)


def test_esdf_plan_sanitizers(tmp_path):
    """The same program under AddressSanitizer and UndefinedBehaviorSanitizer (host code only): no
    signed overflow in an extent of int64 bounds, no overflow in the voxel count."""
    exe = tmp_path / "esdf_plan_san"
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-o", str(exe), SRC])
    out = run_and_compare(exe)
    assert "runtime error" not in out.stderr and "Sanitizer" not in out.stderr, out.stderr[-3000:]


def test_the_constants_the_header_and_the_tests_rely_on():
    plan = open(os.path.join(REPO, "noetic-slam_amd", "csrc", "esdf_plan.h")).read()
    assert re.search(r"ESDF_MAX_RADIUS = 128;", plan)
    assert re.search(r"ESDF_MAX_VOXELS = 1ull << 28;", plan)
    assert re.search(r"ESDF_SCRATCH_PER_VOXEL = 5;", plan)
    assert re.search(r"ESDF_LDS_STATIC = %d;" % LDS_STATIC, plan)
    assert "hip" not in re.sub(r"//.*", "", plan).lower()  # plain C++: no HIP in the plan
    hdr = open(os.path.join(REPO, "include", "tsdf_hip_esdf.h")).read()
    assert re.search(r"#define TSDF_ESDF_MAX_RADIUS 128u", hdr)
    assert "5 bytes of device scratch per voxel" in " ".join(hdr.split())
