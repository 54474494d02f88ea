"""The host planning of the indexed mesh (noetic-slam_amd/csrc/mesh_plan.h: the box rules of
include/tsdf_hip_mesh.h, the bricks a box lists, the prefixes) built with g++ and checked on the
CPU against a Python restatement (tests/cpp/mesh_plan_check.cpp answers the queries), plain and
under ASan + UBSan."""
import os
import re
import subprocess

import numpy as np

from conftest import REPO

SRC = os.path.join(REPO, "tests", "cpp", "mesh_plan_check.cpp")
I64_MIN, I64_MAX = -(1 << 63), (1 << 63) - 1
OK, HALF, ORDER, EXTENT = range(4)
LIMIT = 1 << 24


def box_check(has, lo, hi):
    if has in (1, 2):
        return "%d" % HALF
    if has == 0:
        return "%d 0 %d %d %d %d %d %d" % ((OK,) + (-LIMIT,) * 3 + (LIMIT,) * 3)
    if any(h < l for l, h in zip(lo, hi)):
        return "%d" % ORDER
    if any(h - l >= 1 << 31 for l, h in zip(lo, hi)):
        return "%d" % EXTENT
    cl = [min(max(v, -LIMIT), LIMIT) for v in lo]
    ch = [min(max(v, -LIMIT), LIMIT) for v in hi]
    empty = any(h <= l for l, h in zip(cl, ch))
    return "%d %d %d %d %d %d %d %d" % (OK, empty, *cl, *ch)


def list_bricks(lo, hi, bricks):
    """Bricks with a voxel in [lo, hi + 1) in (z, y, x) order; how many have one in [lo, hi)."""
    def touches(b, grow):
        return all(8 * b[a] + 8 > lo[a] and 8 * b[a] < hi[a] + grow for a in range(3))
    listed = sorted((b for b in bricks if touches(b, 1)), key=lambda b: (b[2], b[1], b[0]))
    examined = sum(touches(b, 0) for b in bricks)
    return " ".join("%d" % v for v in [examined, len(listed)] + [c for b in listed for c in b])


def queries():
    q, want = [], []
    vals = (0, 1, -1, 7, 8, -8, LIMIT - 1, LIMIT, LIMIT + 1, -LIMIT, -LIMIT - 1, 1 << 31,
            (1 << 31) - 1, 1 << 40, I64_MIN, I64_MAX, -(1 << 62))
    boxes = [([0, 0, 0], [4, 5, 6])]
    for l in vals:
        for e in (0, 1, 9, (1 << 31) - 1, 1 << 31, 1 << 62):
            if l + e <= I64_MAX:
                boxes.append(([l, 0, -3], [l + e, 1, -2]))
                boxes.append(([1, 2, l], [2, 2, l + e]))
            if l - 1 >= I64_MIN:
                boxes.append(([0, l, 0], [1, l - 1, 1]))
    boxes.append(([I64_MIN] * 3, [I64_MAX] * 3))
    boxes.append(([0, 0, 5], [1 << 40, 1, 4]))  # the order rule comes before the extent rule
    for lo, hi in boxes:
        for has in (3, 0, 1, 2):
            q.append("B %d %d %d %d %d %d %d" % (has, *lo, *hi))
            want.append(box_check(has, lo, hi))
    rng = np.random.default_rng(5)
    edge = (1 << 20) - 1
    sets = [[(0, 0, 0)], [], [(-(1 << 20),) * 3, (edge,) * 3, (0, edge, -(1 << 20))]]
    for _ in range(6):
        b = rng.integers(-4, 4, (40, 3))
        sets.append(sorted({tuple(int(v) for v in r) for r in b}))
    for bricks in sets:
        for lo, hi in (([-LIMIT] * 3, [LIMIT] * 3), ([0, 0, 0], [8, 8, 8]), ([0, 0, 0], [7, 7, 7]),
                       ([-3, -9, 1], [5, 0, 17]), ([-16, -16, -16], [-8, -8, -8]),
                       ([3, 3, 3], [4, 4, 4]), ([8 * edge, 8 * edge, 8 * edge], [LIMIT] * 3),
                       ([-LIMIT] * 3, [-(1 << 23) + 1] * 3)):
            q.append("L %d %d %d %d %d %d %d %s" % (*lo, *hi, len(bricks),
                                                   " ".join("%d %d %d" % b for b in bricks)))
            want.append(list_bricks(lo, hi, bricks))
    for cnt in ([], [(0, 0)], [(5, 3), (0, 0), (2, 9)],
                [((1 << 32) - 1, (1 << 32) - 1)] * 3, [(7, 1 << 31), (1, 1 << 31), (0, 4)]):
        q.append("P %d %s" % (len(cnt), " ".join("%d %d" % c for c in cnt)))
        t = v = 0
        cells = []
        for ct, cv in cnt:
            cells += [t, v & 0xFFFFFFFF]
            t, v = t + ct, v + cv
        want.append(" ".join("%d" % x for x in [t, v] + cells))
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
    assert box_check(1, [0] * 3, [1] * 3) == "%d" % HALF
    assert box_check(3, [0] * 3, [1, -1, 1]) == "%d" % ORDER
    assert box_check(3, [0] * 3, [1, 1 << 31, 1]) == "%d" % EXTENT
    assert box_check(3, [0] * 3, [1, 0, 1]).split()[:2] == ["0", "1"]  # an empty box is no error
    assert list_bricks([0, 0, 0], [8, 8, 8], [(0, 0, 0), (1, 0, 0), (2, 0, 0)]) == "1 2 0 0 0 1 0 0"
    assert list_bricks([0, 0, 0], [7, 8, 8], [(0, 0, 0), (1, 0, 0)]) == "1 1 0 0 0"
    seen = {w.split()[0] for q, w in zip(*queries()) if q[0] == "B"}
    assert seen == {"0", "1", "2", "3"}


def test_mesh_plan_check(tmp_path):
    exe = tmp_path / "mesh_plan_check"
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-o", str(exe), SRC])
    run_and_compare(exe)


def test_mesh_plan_sanitizers(tmp_path):
    """The same program under AddressSanitizer and UndefinedBehaviorSanitizer (host code only): no
    signed overflow in an extent of int64 bounds or in a brick's voxel range."""
    exe = tmp_path / "mesh_plan_san"
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-o", str(exe), SRC])
    out = run_and_compare(exe)
    assert "runtime error" not in out.stderr and "Sanitizer" not in out.stderr, out.stderr[-3000:]


def test_the_constants_the_header_and_the_kernels_rely_on():
    plan = open(os.path.join(REPO, "noetic-slam_amd", "csrc", "mesh_plan.h")).read()
    assert re.search(r"MESH_BOX_LIMIT = 1ll << 24;", plan)
    assert "hip" not in re.sub(r"//.*", "", plan).lower()  # plain C++: no HIP in the plan
    dev = open(os.path.join(REPO, "noetic-slam_amd", "csrc", "tsdf_device.h")).read()
    assert re.search(r"MESH_VMASK_WORDS = 3 \* BRICK_VOX / 32;", dev)  # 48 words, 192 bytes
    hdr = " ".join(open(os.path.join(REPO, "include", "tsdf_hip_mesh.h")).read().split())
    # key 8 + mask 192 + two counts 8 + two offsets 12 <= 224
    assert "224 bytes per listed brick" in hdr and "192 bytes" in hdr
    assert "plus 4 bytes per brick of the map" in hdr  # pool slot -> position in the list
