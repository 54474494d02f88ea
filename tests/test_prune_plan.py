"""The host arithmetic of prune and evict (noetic-slam_amd/csrc/prune_plan.h: the copy-out's piece
plan from the scratch bound, the brick box of a world-frame cube)
built with g++ and checked on the CPU against a Python restatement over a grid
(tests/cpp/prune_plan_check.cpp answers the queries), plain and under ASan + UBSan."""
import math
import os
import subprocess

from conftest import REPO

SRC = os.path.join(REPO, "tests", "cpp", "prune_plan_check.cpp")
BMIN, BMAX = -(1 << 20), 1 << 20
SCRATCH = 64 << 20  # the header's stated bound on the copy-out's device scratch


def box_axis(c, r, vs):
    """lo = floor((c - r) / (8 vs)), hi = floor((c + r) / (8 vs)) + 1 in double, clamped to the
    packable range; written out again here, apart from tsdf_map.window.cube_box."""
    def clamp(q):
        if q != q:
            return 0
        return int(min(max(q, BMIN), BMAX))
    side = 8.0 * vs
    qa, qb = (c - r) / side, (c + r) / side
    lo = clamp(math.floor(qa) if math.isfinite(qa) else qa)
    hi = clamp((math.floor(qb) if math.isfinite(qb) else qb) + 1.0)
    return lo, max(lo, hi)


def grid():
    vss = (0.05, 0.1, 0.02, 0.125)
    cs, rs = [], []
    for vs in vss:
        side = 8 * vs
        # centres: negative, zero, on brick faces, just off them, far out
        cs += [0.0, -0.0, side, -side, 3 * side, -3 * side, 0.5 * side, -0.5 * side, 1.2345,
               -1.2345, -17.0, 23.75, math.nextafter(side, 0.0), math.nextafter(-side, 0.0),
               1e5, -1e5, (BMAX - 1) * side, BMIN * side, 1e300, -1e300]
        # radii: 0, whole bricks (cube edges exactly on brick faces), odd ones
        rs += [0.0, side, 2 * side, 0.5 * side, 0.3, 7.0, 25.0, 1e4]
    cs = sorted(set(cs))
    rs = sorted(set(rs))
    return [(c, r, vs) for vs in vss for c in cs for r in rs] + \
        [(math.inf, 1.0, 0.05), (-math.inf, 1.0, 0.05), (math.nan, 1.0, 0.05),
         (0.0, math.inf, 0.05), (0.0, math.nan, 0.05)]


def queries():
    q, want = [], []
    for c, r, vs in grid():
        q.append("B %s %s %s" % (float(c).hex(), float(r).hex(), float(vs).hex()))
        want.append("%d %d" % box_axis(c, r, vs))
    for arrays in (-1, 0, 1, 2):
        q.append("P %d" % arrays)
        want.append("%d" % (SCRATCH // (2048 * arrays) if arrays > 0 else 0))
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


def test_the_stated_rule_on_known_cases():
    # 5 cm voxels: bricks of 0.4 m.  A cube edge exactly on a brick face: the closed cube touches
    # the brick beyond its far face and keeps it; its near face starts a brick
    assert box_axis(0.0, 0.4, 0.05) == (-1, 2)
    assert box_axis(0.0, 0.0, 0.05) == (0, 1)       # r = 0: the brick holding the centre
    assert box_axis(-0.2, 0.0, 0.05) == (-1, 0)
    assert box_axis(-0.4, 0.0, 0.05) == (-1, 0)     # a negative centre on a face
    assert box_axis(-1e300, 1.0, 0.05) == (BMIN, BMIN)
    assert box_axis(1e300, 1.0, 0.05) == (BMAX, BMAX)


def test_python_cube_box_is_the_restatement():
    from tsdf_map.window import cube_box
    for c, r, vs in grid():
        lo, hi = cube_box([c, -c, c], r, vs)
        a, b = box_axis(c, r, vs), box_axis(-c, r, vs)
        assert (lo[0], hi[0]) == a and (lo[1], hi[1]) == b and (lo[2], hi[2]) == a, (c, r, vs)


def test_prune_plan_check(tmp_path):
    exe = tmp_path / "prune_plan_check"
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-o", str(exe), SRC])
    run_and_compare(exe)


def test_prune_plan_sanitizers(tmp_path):
    """The same program under AddressSanitizer and UndefinedBehaviorSanitizer (host code only): no
    out-of-range conversion of a clamped double, no overflow in the piece plan."""
    exe = tmp_path / "prune_plan_san"
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined",
                           "-fsanitize=float-cast-overflow", "-fno-sanitize-recover=undefined",
                           "-o", str(exe), SRC])
    out = run_and_compare(exe)
    assert "runtime error" not in out.stderr and "Sanitizer" not in out.stderr, out.stderr[-3000:]


def test_the_device_constants_the_tests_rely_on():
    """tests/test_prune_gpu.py sizes its slot patterns by the scan block of tsdf_prune.hip."""
    import re
    txt = open(os.path.join(REPO, "noetic-slam_amd", "csrc", "tsdf_device.h")).read()
    assert re.search(r"constexpr uint32_t RM_BLOCK = 256;", txt)
    assert re.search(r"constexpr int RM_SCAN_THREADS = 64;", txt)
    hdr = open(os.path.join(REPO, "noetic-slam_amd", "csrc", "prune_plan.h")).read()
    assert re.search(r"EVICT_SCRATCH_BYTES = 64ull << 20;", hdr)
