"""The host arithmetic of the frontier voxels (noetic-slam_amd/csrc/frontier_plan.h: the argument
rules of include/tsdf_hip_frontier.h in their order and with their texts, the offset table, the
grid cap and the prefix) built with g++ and checked on the CPU against a Python restatement
(tests/cpp/frontier_plan_check.cpp answers the queries), plain and under ASan + UBSan."""
import math
import os
import re
import struct
import subprocess

import numpy as np

from conftest import REPO

SRC = os.path.join(REPO, "tests", "cpp", "frontier_plan_check.cpp")
I64_MIN, I64_MAX = -(1 << 63), (1 << 63) - 1
OK, HALF, BAND, WEIGHT, CONN, UNKNOWN, ORDER, EXTENT = range(8)
TEXT = {HALF: "lo and hi must both be given or both be NULL",
        BAND: "free_band is not finite",
        WEIGHT: "min_weight is negative or NaN",
        CONN: "connectivity must be 6, 18 or 26",
        UNKNOWN: "min_unknown must be in 1..connectivity",
        ORDER: "hi < lo",
        EXTENT: "box extent >= 2^31 voxels"}
GRID_CAP = 2048
LIMIT = 1 << 24  # the mesh's clamp of a box


def f32(x):
    return struct.unpack("f", struct.pack("f", x))[0]


def check(box, lo, hi, band, min_w, conn, min_unknown):
    """The header's rules in the order they are reported: (rule, empty, clamped lo, clamped hi)."""
    none = (0,) * 7
    if box in (1, 2):
        return (HALF,) + none
    if not math.isfinite(band):
        return (BAND,) + none
    if not min_w >= 0.0:
        return (WEIGHT,) + none
    if conn not in (6, 18, 26):
        return (CONN,) + none
    if not 1 <= min_unknown <= conn:
        return (UNKNOWN,) + none
    if box == 0:
        return (OK, 0) + (-LIMIT,) * 3 + (LIMIT,) * 3
    if any(h < l for l, h in zip(lo, hi)):
        return (ORDER,) + none
    if any(h - l >= 1 << 31 for l, h in zip(lo, hi)):
        return (EXTENT,) + none
    cl = [min(max(l, -LIMIT), LIMIT) for l in lo]
    ch = [min(max(h, -LIMIT), LIMIT) for h in hi]
    return (OK, int(any(h <= l for l, h in zip(cl, ch))), *cl, *ch)


def arg_grid():
    box = (3, [0, 0, 0], [4, 5, 6])
    ok = (0.05, 0.0, 6, 1)
    out = [(b, [0, 0, 0], [4, 5, 6], *ok) for b in (0, 1, 2, 3)]
    out += [(*box, b, 0.0, 6, 1) for b in
            (0.0, -0.0, 1e-30, 3e38, -1.0, math.inf, -math.inf, math.nan)]
    out += [(*box, 0.05, w, 6, 1) for w in (0.0, -0.0, 2.0, math.inf, -1e-30, -math.inf, math.nan)]
    out += [(*box, 0.05, 0.0, c, 1) for c in (6, 18, 26, 0, 4, 7, 27, -6, 1 << 30)]
    out += [(*box, 0.05, 0.0, c, m) for c in (6, 18, 26)
            for m in (0, 1, 6, 7, 18, 19, 26, 27, -1, c)]
    # the first broken rule is the one reported
    bad_box = (3, [0, 0, 0], [-1, 1 << 40, 6])
    out += [(1, [0, 0, 0], [-1, 5, 6], math.nan, -1.0, 5, 0), (*bad_box, math.nan, -1.0, 5, 0),
            (*bad_box, 0.0, -1.0, 5, 0), (*bad_box, 0.0, 0.0, 5, 0), (*bad_box, 0.0, 0.0, 6, 0),
            (*bad_box, 0.0, 0.0, 6, 1), (3, [0, 0, 0], [1, 1 << 40, 6], *ok),
            (0, [5, 5, 5], [1, 1, 1], *ok)]
    los = (0, -5, -8, 7, LIMIT - 1, LIMIT, LIMIT + 3, -LIMIT, -LIMIT - 1, I64_MIN, I64_MIN + 1,
           I64_MAX - 7, -(1 << 62))
    exts = (0, 1, 8, 9, (1 << 31) - 1, 1 << 31, 1 << 40)
    for l in los:
        for e in exts:
            if l + e <= I64_MAX:
                out.append((3, [l, 0, -3], [l + e, 1, -2], *ok))
                out.append((3, [3, -1, l], [4, 1, l + e], 0.0, 1.0, 26, 26))
            if l - 1 >= I64_MIN:
                out.append((3, [0, l, 0], [1, l - 1, 1], *ok))
    out.append((3, [I64_MIN] * 3, [I64_MAX] * 3, *ok))
    return out


def offsets_restated():
    """Faces, then edges, then corners; 26 distinct nonzero offsets."""
    return [(dx, dy, dz) for dz in (-1, 0, 1) for dy in (-1, 0, 1) for dx in (-1, 0, 1)
            if (dx, dy, dz) != (0, 0, 0)]


def brick_in_box(b, lo, hi):
    return int(all(8 * c + 8 > l and 8 * c < h and h > l for c, l, h in zip(b, lo, hi)))


def queries():
    q, want = [], []
    for box, lo, hi, band, mw, conn, mu in arg_grid():
        band, mw = f32(band), f32(mw)
        q.append("A %d %d %d %d %d %d %d %s %s %d %d"
                 % (box, *lo, *hi, float(band).hex(), float(mw).hex(), conn, mu))
        r = check(box, lo, hi, band, mw, conn, mu)
        want.append(" ".join("%d" % v for v in r))
        want.append(TEXT.get(r[0], "-"))
    for nb in (0, 1, 2, GRID_CAP - 1, GRID_CAP, GRID_CAP + 1, GRID_CAP + 3, 1 << 20, (1 << 32) - 2):
        q.append("G %d" % nb)
        want.append("%d" % max(1, min(nb, GRID_CAP)))
    rng = np.random.default_rng(7)
    for cnt in ([], [0], [5], [0, 0, 3, 0, 512, 1], [512] * 9, [(1 << 32) - 1] * 3,
                rng.integers(0, 513, 1000).tolist()):
        q.append("P %d %s" % (len(cnt), " ".join(map(str, cnt))))
        off = np.concatenate([[0], np.cumsum(np.asarray(cnt, np.uint64))[:-1]]) if cnt else []
        want.append(" ".join(map(str, [sum(cnt), sum(1 for c in cnt if c), sum(cnt),
                                       *[int(o) for o in off]])))
    for b in ([0, 0, 0], [-1, 2, 0], [(1 << 20) - 1, -(1 << 20), 5]):
        v0 = [8 * c for c in b]
        for lo, hi in (([v0[0], v0[1], v0[2]], [v0[0] + 1, v0[1] + 1, v0[2] + 1]),
                       ([v0[0] + 8, v0[1], v0[2]], [v0[0] + 9, v0[1] + 1, v0[2] + 1]),
                       ([v0[0] - 1, v0[1] - 1, v0[2] - 1], [v0[0], v0[1] + 8, v0[2] + 8]),
                       ([v0[0] + 7, v0[1] + 7, v0[2] + 7], [v0[0] + 20, v0[1] + 8, v0[2] + 8]),
                       ([v0[0] + 3, v0[1], v0[2]], [v0[0] + 3, v0[1] + 8, v0[2] + 8]),
                       ([-(1 << 29)] * 3, [1 << 29] * 3)):
            q.append("K %d %d %d %d %d %d %d %d %d" % (*b, *lo, *hi))
            want.append("%d" % brick_in_box(b, lo, hi))
    q.append("O")
    want.append(None)  # checked by test_the_offset_table
    return q, want


def run(exe):
    q, want = queries()
    out = subprocess.run([str(exe)], input="\n".join(q) + "\n", capture_output=True, text=True,
                         timeout=300)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-3000:]
    got = out.stdout.split("\n")
    assert got[len(want)] == "ok %d" % len(q)
    bad = [(i, b, c) for i, (b, c) in enumerate(zip(got, want)) if c is not None and b != c]
    assert not bad, bad[:10]
    return out, got[len(want) - 1]


def test_the_stated_rules_on_known_cases():
    box = (3, [0] * 3, [1] * 3)
    assert check(1, [0] * 3, [1] * 3, math.nan, -1.0, 0, 0)[0] == HALF
    assert check(*box, math.inf, -1.0, 0, 0)[0] == BAND
    assert check(*box, -5.0, 0.0, 6, 1)[0] == OK           # a negative band is allowed
    assert check(*box, 0.0, math.nan, 0, 0)[0] == WEIGHT
    assert check(*box, 0.0, 0.0, 8, 0)[0] == CONN
    assert check(*box, 0.0, 0.0, 6, 7)[0] == UNKNOWN and check(*box, 0.0, 0.0, 18, 0)[0] == UNKNOWN
    assert check(3, [0] * 3, [1, -1, 1], 0.0, 0.0, 6, 6)[0] == ORDER
    assert check(3, [0] * 3, [1, 1 << 31, 1], 0.0, 0.0, 26, 26)[0] == EXTENT
    assert check(3, [0] * 3, [1, 0, 1], 0.0, 0.0, 6, 1)[:2] == (OK, 1)
    assert check(0, None, None, 0.0, 0.0, 6, 1) == (OK, 0) + (-LIMIT,) * 3 + (LIMIT,) * 3
    assert {check(*a)[0] for a in arg_grid()} == set(range(8))


def test_frontier_plan_check(tmp_path):
    exe = tmp_path / "frontier_plan_check"
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-o", str(exe), SRC])
    run(exe)


def test_frontier_plan_sanitizers(tmp_path):
    """The same program under AddressSanitizer and UndefinedBehaviorSanitizer (host code only): no
    signed overflow in an extent of int64 bounds, no read past a count array."""
    exe = tmp_path / "frontier_plan_san"
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-o", str(exe), SRC])
    out, _ = run(exe)
    assert "runtime error" not in out.stderr and "Sanitizer" not in out.stderr, out.stderr[-3000:]


def test_the_offset_table(tmp_path):
    """A connectivity is a prefix: 6 faces, 12 edges, 8 corners, 26 distinct nonzero offsets."""
    exe = tmp_path / "frontier_plan_check"
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-o", str(exe), SRC])
    _, line = run(exe)
    v = [int(t) for t in line.split()]
    offs = [tuple(v[3 * k:3 * k + 3]) for k in range(26)]
    assert len(v) == 78 and sorted(offs) == sorted(offsets_restated())
    cls = [sum(abs(c) for c in o) for o in offs]
    assert cls == [1] * 6 + [2] * 12 + [3] * 8
    assert all(max(abs(c) for c in o) == 1 for o in offs)
    # every prefix is symmetric: with an offset it holds the opposite one
    for n in (6, 18, 26):
        assert {tuple(-c for c in o) for o in offs[:n]} == set(offs[:n])
    import frontierref as fr
    for n in (6, 18, 26):  # the reference's table holds the same classes per prefix
        assert set(fr.OFFSETS[:n]) == set(offs[:n])


def test_the_constants_the_header_and_the_tests_rely_on():
    plan = open(os.path.join(REPO, "noetic-slam_amd", "csrc", "frontier_plan.h")).read()
    assert re.search(r"FRONTIER_GRID_CAP = %d;" % GRID_CAP, plan)
    assert re.search(r"FRONTIER_THREADS = 512;", plan) and re.search(r"FRONTIER_TILE = 10;", plan)
    assert '#include "mesh_plan.h"' in plan and "mesh_box_check(" in plan
    assert "hip" not in re.sub(r"//.*", "", plan).lower()  # plain C++: no HIP in the plan
    hdr = " ".join(open(os.path.join(REPO, "include", "tsdf_hip_frontier.h")).read().split())
    assert '"frontier: "' in hdr and "24 bytes per listed brick" in hdr
    mesh = open(os.path.join(REPO, "noetic-slam_amd", "csrc", "mesh_plan.h")).read()
    assert re.search(r"MESH_BOX_LIMIT = 1ll << 24;", mesh)
