"""The host arithmetic of the column maps (noetic-slam_amd/csrc/columns_plan.h: the argument rules
of include/tsdf_hip_columns.h, the brick columns of a box, the trip mapping of k_column_map) built
with g++ and checked on the CPU against a Python restatement over a grid
(tests/cpp/columns_plan_check.cpp answers the queries), plain and under ASan + UBSan."""
import math
import os
import re
import struct
import subprocess

from conftest import REPO

SRC = os.path.join(REPO, "tests", "cpp", "columns_plan_check.cpp")
I64_MIN, I64_MAX = -(1 << 63), (1 << 63) - 1
OK, BAND, WEIGHT, COUNT, ORDER, EXTENT, HEIGHT, CELLS = range(8)
COL_WAVES, COL_GRID_CAP = 4, 8192
FIRST_TRIP = COL_WAVES * COL_GRID_CAP
MAX_NZ, MAX_CELLS = 65535, 1 << 26


def f32(x):
    return struct.unpack("f", struct.pack("f", x))[0]


def check(lo, hi, band, min_w, min_occ, min_free):
    """The header's argument rules in the order they are reported, the box and its brick columns."""
    none = (0,) * 11
    if not math.isfinite(band):
        return (BAND,) + none
    if not min_w >= 0.0:
        return (WEIGHT,) + none
    if not (1 <= min_occ <= 65535 and 1 <= min_free <= 65535):
        return (COUNT,) + none
    if any(h < l for l, h in zip(lo, hi)):
        return (ORDER,) + none
    n = [h - l for l, h in zip(lo, hi)]
    if any(e >= 1 << 31 for e in n):
        return (EXTENT,) + none
    if 0 in n:
        return (OK, n[0], n[1], n[2]) + (0,) * 8
    if n[2] > MAX_NZ:
        return (HEIGHT,) + none
    if n[0] * n[1] > MAX_CELLS:
        return (CELLS,) + none
    b0 = [l // 8 for l in lo]                    # Python's // floors
    nb = [(h - 1) // 8 - b + 1 for h, b in zip(hi, b0)]
    return (OK, n[0], n[1], n[2], n[0] * n[1], *b0, *nb, nb[0] * nb[1])


def grid_of(cols):
    groups = -(-cols // COL_WAVES)
    grid = max(1, min(groups, COL_GRID_CAP))
    return groups, grid, -(-groups // grid)


def column_of(cols, nbx, bx0, by0, trip, wg, wave):
    """The restated mapping: (index, bx, by), or (index, None, None) past the last brick column."""
    c = (trip * grid_of(cols)[1] + wg) * COL_WAVES + wave
    return (c, bx0 + c % nbx, by0 + c // nbx) if c < cols else (c, None, None)


def arg_grid():
    box = ([0, 0, 0], [4, 5, 6])
    ok = (0.0, 0.0, 1, 1)
    out = [(*box, b, 0.0, 1, 1) for b in
           (0.0, -0.0, 1e-30, 3e38, -1.0, -3e38, math.inf, -math.inf, math.nan)]
    out += [(*box, 0.1, w, 1, 1) for w in (0.0, -0.0, 2.0, math.inf, -1e-30, -math.inf, math.nan)]
    out += [(*box, 0.1, 0.0, a, b) for a, b in
            ((0, 1), (1, 0), (65535, 65535), (65536, 1), (1, 65536), ((1 << 32) - 1, 1), (2, 3))]
    # the first broken rule is the one reported
    out += [(*box, math.nan, -1.0, 0, 0), (*box, 0.0, -1.0, 0, 0),
            ([0, 0, 0], [-1, 5, 6], 0.0, 0.0, 0, 1), ([0, 0, 0], [-1, 1 << 40, 6], *ok),
            ([0, 0, 0], [1 << 40, 1, -1], *ok), ([0, 0, 0], [1 << 31, 1, 70000], *ok),
            ([0, 0, 0], [1 << 14, 1 << 14, 70000], *ok)]
    los = (0, -5, -8, -9, 7, 1 << 23, -(1 << 23) - 3, I64_MIN, I64_MIN + 1, I64_MAX - 7,
           -(1 << 62))
    exts = (0, 1, 7, 8, 9, 64, 65, 65535, 65536, (1 << 31) - 1, 1 << 31, 1 << 40)
    for l in los:
        for e in exts:
            if l + e <= I64_MAX:
                out.append(([l, 0, -3], [l + e, 1, -2], *ok))
                out.append(([3, l, 0], [4, l + e, 1], *ok))
                out.append(([3, -1, l], [4, 1, l + e], *ok))
                out.append(([1, l, 0], [2, l + e, 0], *ok))  # an empty box of any length
            if l - 1 >= I64_MIN:
                out.append(([0, l, 0], [1, l - 1, 1], *ok))
    out.append(([I64_MIN] * 3, [I64_MAX] * 3, *ok))
    out.append(([I64_MAX - 3] * 3, [I64_MAX] * 3, *ok))
    # around the 2^26 bound
    for n in ([1 << 13, 1 << 13, 1], [(1 << 13) + 1, 1 << 13, 1], [1 << 26, 1, 3],
              [(1 << 26) + 1, 1, 3], [1, 1 << 26, 65535], [1 << 20, 1 << 20, 2],
              [(1 << 31) - 1, (1 << 31) - 1, 1], [(1 << 31) - 1, (1 << 31) - 1, 0],
              [1442, 1442, 3], [97, 80, 33], [45, 27, 52]):
        out.append(([-7, 3, -(1 << 30)], [-7 + n[0], 3 + n[1], -(1 << 30) + n[2]], 0.1, 1.0, 2, 3))
    return out


COLS = (0, 1, 3, 4, 5, 63, FIRST_TRIP - 1, FIRST_TRIP, FIRST_TRIP + 1, FIRST_TRIP + 5,
        2 * FIRST_TRIP, 2 * FIRST_TRIP + 3, 182 * 182, 1 << 20, (1 << 23) + 1)


def queries():
    q, want = [], []
    for lo, hi, band, mw, mo, mf in arg_grid():
        band, mw = f32(band), f32(mw)
        q.append("A %d %d %d %d %d %d %s %s %d %d"
                 % (*lo, *hi, float(band).hex(), float(mw).hex(), mo, mf))
        want.append(" ".join("%d" % v for v in check(lo, hi, band, mw, mo, mf)))
    for cols in COLS:
        q.append("G %d" % cols)
        want.append("%d %d %d" % grid_of(cols))
        q.append("C %d" % cols)
        want.append("%d %d %d" % (cols, 1 if cols else 0, 1 if cols else 0))
        if not cols:
            continue
        groups, grid, trips = grid_of(cols)
        for nbx, bx0, by0 in ((1, 0, 0), (7, -3, 1 << 19), (182, -(1 << 60), (1 << 62) + 5)):
            for trip in {0, 1, trips - 1}:
                for wg in {0, 1, grid - 1}:
                    for wave in (0, COL_WAVES - 1):
                        q.append("M %d %d %d %d %d %d %d" % (cols, nbx, bx0, by0, trip, wg, wave))
                        c, bx, by = column_of(cols, nbx, bx0, by0, trip, wg, wave)
                        want.append("%d - -" % c if bx is None else "%d %d %d" % (c, bx, by))
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
    box = ([0] * 3, [1] * 3)
    assert check(*box, math.inf, 0.0, 1, 1)[0] == BAND
    assert check(*box, -5.0, 0.0, 1, 1)[0] == OK           # a negative band is allowed
    assert check(*box, 0.0, math.nan, 1, 1)[0] == WEIGHT
    assert check(*box, 0.0, 0.0, 0, 1)[0] == COUNT and check(*box, 0.0, 0.0, 1, 65536)[0] == COUNT
    assert check([0] * 3, [1, -1, 1], 0.0, 0.0, 1, 1)[0] == ORDER
    assert check([0] * 3, [1, 1 << 31, 1], 0.0, 0.0, 1, 1)[0] == EXTENT
    assert check([0] * 3, [1, 1, 65536], 0.0, 0.0, 1, 1)[0] == HEIGHT
    assert check([0] * 3, [1, 1, 65535], 0.0, 0.0, 1, 1)[0] == OK
    assert check([0] * 3, [(1 << 13) + 1, 1 << 13, 1], 0.0, 0.0, 1, 1)[0] == CELLS
    assert check([0] * 3, [0, 1 << 30, 70000], 0.0, 0.0, 1, 1) == (OK, 0, 1 << 30, 70000) + (0,) * 8
    # negative and unaligned bounds: the bricks floor
    assert check([-9, -8, 7], [1, -7, 9], 0.0, 0.0, 1, 1) == (OK, 10, 1, 2, 10, -2, -1, 0, 3, 1, 2, 3)
    seen = {check(*a)[0] for a in arg_grid()}
    assert seen == set(range(8))


def test_the_trip_mapping_covers_every_brick_column_once():
    """The restated mapping over every (trip, workgroup, wave) of a launch, below, at and above one
    trip's COL_GRID_CAP * COL_WAVES brick columns."""
    for cols in (1, 5, FIRST_TRIP - 1, FIRST_TRIP, FIRST_TRIP + 1, 182 * 182, 2 * FIRST_TRIP + 3):
        groups, grid, trips = grid_of(cols)
        assert (trips > 1) == (cols > FIRST_TRIP)
        seen = []
        for trip in range(trips):
            for wg in range(grid):
                if trip * grid + wg >= groups:
                    continue
                for wave in range(COL_WAVES):
                    c = column_of(cols, 182, 0, 0, trip, wg, wave)
                    if c[1] is not None:
                        seen.append(c[0])
        assert sorted(seen) == list(range(cols))


def test_columns_plan_check(tmp_path):
    exe = tmp_path / "columns_plan_check"
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-o", str(exe), SRC])
    run_and_compare(exe)


def test_columns_plan_sanitizers(tmp_path):
    """The same program under AddressSanitizer and UndefinedBehaviorSanitizer (host code only): no
    signed overflow in an extent or a brick coordinate of int64 bounds."""
    exe = tmp_path / "columns_plan_san"
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-o", str(exe), SRC])
    out = run_and_compare(exe)
    assert "runtime error" not in out.stderr and "Sanitizer" not in out.stderr, out.stderr[-3000:]


def test_the_constants_the_header_and_the_tests_rely_on():
    plan = open(os.path.join(REPO, "noetic-slam_amd", "csrc", "columns_plan.h")).read()
    assert re.search(r"COL_WAVES = %d;" % COL_WAVES, plan)
    assert re.search(r"COL_GRID_CAP = %d;" % COL_GRID_CAP, plan)
    assert re.search(r"COL_MAX_NZ = 65535;", plan) and re.search(r"COL_MAX_CELLS = 1ull << 26;", plan)
    assert '#include "brick_key.h"' in plan
    assert "hip" not in re.sub(r"//.*", "", plan).lower()  # plain C++: no HIP in the plan
    # the smallest square box past the first trip stays below 2^23 voxels at 3 voxels of height
    side = math.isqrt(FIRST_TRIP) + 1
    assert side * side > FIRST_TRIP >= (side - 1) ** 2 and side == 182
    assert 3 * (8 * (side - 2) + 2) ** 2 < 1 << 23
    hdr = " ".join(open(os.path.join(REPO, "include", "tsdf_hip_columns.h")).read().split())
    assert "nz > 65535" in hdr and "2^26" in hdr and '"columns: "' in hdr
