"""The host arithmetic of the 2:1 coarsening (noetic-slam_amd/csrc/coarsen_plan.h: the argument
and compatibility rules with their texts, the selection, the parent of a brick, the child index
arithmetic of a lane, the scratch sizes) built with g++ and checked on the CPU
(tests/cpp/coarsen_plan_check.cpp answers the queries), plain and under ASan + UBSan.  The index
arithmetic is not restated line by line but checked against what it stands for: the children
2 V + (a, b, c) of coarse voxel V = 8 D + lane, their brick and their local voxel, by integer floor
division over every lane and over destination bricks of either sign."""
import os
import re
import struct
import subprocess

import numpy as np

from conftest import REPO

SRC = os.path.join(REPO, "tests", "cpp", "coarsen_plan_check.cpp")
PLAN = os.path.join(REPO, "noetic-slam_amd", "csrc", "coarsen_plan.h")
F = np.float32
A_OK, A_SIDE, A_BOX, A_CHILDREN, A_WEIGHT = range(5)
C_OK, C_VOXEL, C_TRUNC, C_BG = range(4)
ARG_TEXT = {A_OK: "-", A_SIDE: "side must be TSDF_COARSEN_INSIDE or _OUTSIDE",
            A_BOX: "exactly one of lo and hi is NULL", A_CHILDREN: "min_children must be 1..8",
            A_WEIGHT: "min_weight is negative or NaN"}
COMPAT_TEXT = {C_OK: "-", C_VOXEL: "the destination's voxel size is not twice the source's",
               C_TRUNC: "the contexts' truncation distances differ",
               C_BG: "the contexts' backgrounds differ (Voxblox against VDBFusion)"}
LIM = 1 << 20
SET_MIN = 1024
COUNTER_BYTES = (16 + 64 * 16) * 8


def bits(x):
    return struct.pack("f", x)


def args_rule(side, has_lo, has_hi, mc, mw):
    if side not in (0, 1):
        return A_SIDE
    if bool(has_lo) != bool(has_hi):
        return A_BOX
    if not 1 <= mc <= 8:
        return A_CHILDREN
    if not mw >= 0.0:
        return A_WEIGHT
    return A_OK


def compat_rule(vs_d, vs_s, tau_d, tau_s, sem_d, sem_s):
    if bits(F(vs_d)) != bits(F(2.0) * F(vs_s)):
        return C_VOXEL
    if bits(F(tau_d)) != bits(F(tau_s)):
        return C_TRUNC
    if (sem_d == 1) != (sem_s == 1):
        return C_BG
    return C_OK


def selected(has_box, side, lo, hi, b):
    if not has_box:
        return True
    inside = all(lo[a] <= b[a] < hi[a] for a in range(3))
    return inside if side == 0 else not inside


def set_slots(n):
    s = SET_MIN
    while s < 2 * n:
        s <<= 1
    return s


def lane_children(l, D=(0, 0, 0)):
    """What the lane arithmetic stands for: coarse voxel V = 8 D + (x, y, z) of lane l, its
    children 2 V + (a, b, c) in the order k = a + 2 b + 4 c: (brick, local index) each."""
    V = [8 * D[0] + (l & 7), 8 * D[1] + ((l >> 3) & 7), 8 * D[2] + (l >> 6)]
    out = []
    for k in range(8):
        c = [2 * V[0] + (k & 1), 2 * V[1] + ((k >> 1) & 1), 2 * V[2] + (k >> 2)]
        brick = tuple(v // 8 for v in c)  # (Python's floor division)
        out.append((brick, (c[0] % 8) + 8 * (c[1] % 8) + 64 * (c[2] % 8)))
    return out


PARENTS = [0, 1, 2, 3, -1, -2, -3, -4, 7, -7, 1023, -1023, LIM - 1, LIM - 2, -LIM, -LIM + 1,
           12345, -12345]
SELECTIONS = [(0, 0, (0, 0, 0), (0, 0, 0)), (0, 1, (5, 5, 5), (6, 6, 6)),
              (1, 0, (0, 0, 0), (1, 1, 1)), (1, 1, (0, 0, 0), (1, 1, 1)),
              (1, 0, (-3, -2, -1), (4, 3, 2)), (1, 1, (-3, -2, -1), (4, 3, 2)),
              (1, 0, (0, 0, 0), (0, 5, 5)), (1, 1, (0, 0, 0), (0, 5, 5)),
              (1, 0, (2, 2, 2), (1, 9, 9)), (1, 1, (2, 2, 2), (1, 9, 9)),
              (1, 0, (-LIM, -LIM, -LIM), (LIM, LIM, LIM)), (1, 1, (-LIM, -LIM, -LIM), (LIM, LIM, LIM))]
BRICKS = [(0, 0, 0), (-3, -2, -1), (4, 3, 2), (3, 2, 1), (-4, 0, 0), (0, 4, 4), (1, 5, 5),
          (-LIM, -LIM, -LIM), (LIM - 1, LIM - 1, LIM - 1), (0, 0, 1)]


def queries():
    q, want = [], []
    for side in (0, 1, -1, 2, 7):
        for has_lo, has_hi in ((0, 0), (1, 1), (1, 0), (0, 1)):
            for mc in (0, 1, 4, 8, 9, -1, 1 << 31):
                for mw, txt in ((0.0, "0x0p+0"), (2.0, "0x1p+1"), (-1.0, "-0x1p+0"),
                                (float("nan"), "nan"), (-0.0, "-0x0p+0"), (-1e-30, "-1e-30"),
                                (float("inf"), "inf")):
                    q.append("A %d %d %d %d %s" % (side, has_lo, has_hi, mc, txt))
                    mcu = mc & 0xFFFFFFFF
                    r = args_rule(side, has_lo, has_hi, mcu, float(F(mw)))
                    want.append("%d %s" % (r, ARG_TEXT[r]))
    nxt = float(np.nextafter(F(0.2), F(1)))
    for a in ((0.2, 0.1, 0.3, 0.3, 2, 2), (0.2, 0.1, 0.3, 0.3, 2, 0), (0.2, 0.1, 0.3, 0.3, 1, 1),
              (0.2, 0.1, 0.3, 0.3, 1, 2), (0.2, 0.1, 0.3, 0.3, 0, 1), (0.1, 0.1, 0.3, 0.3, 2, 2),
              (0.1, 0.2, 0.3, 0.3, 2, 2), (0.4, 0.1, 0.3, 0.3, 2, 2), (nxt, 0.1, 0.3, 0.3, 2, 2),
              (0.2 + 1e-12, 0.1, 0.3, 0.3, 2, 2), (0.2, 0.1 + 1e-12, 0.3, 0.3, 2, 2),
              (0.1, 0.05, 0.15, 0.15, 1, 1), (0.2, 0.1, 0.3, 0.30000004, 2, 2),
              (0.2, 0.1, 0.6, 0.3, 2, 2), (0.1, 0.1, 0.2, 0.3, 1, 2), (0.2, 0.1, 0.2, 0.3, 1, 2),
              (2.0 * float(F(0.1)), 0.1, 0.3, 0.3, 0, 0)):
        q.append("C %s %d %d" % (" ".join(float(v).hex() for v in a[:4]), a[4], a[5]))
        r = compat_rule(*a)
        want.append("%d %s" % (r, COMPAT_TEXT[r]))
    for b in PARENTS:
        q.append("P %d" % b)
        want.append("%d" % (b // 2))
    for has_box, side, lo, hi in SELECTIONS:
        for b in BRICKS:
            q.append("S %d %d %d %d %d %d %d %d %d %d %d" % ((has_box, side) + lo + hi + b))
            want.append("%d" % selected(has_box, side, lo, hi, b))
    for l in range(512):
        q.append("L %d" % l)
        ch = lane_children(l)
        j = ch[0][0][0] + 2 * ch[0][0][1] + 4 * ch[0][0][2]
        base = ch[0][1]
        want.append(" ".join(str(v) for v in [j, base] + [c[1] - base for c in ch]))
    for n in (0, 1, 511, 512, 513, 29485, 1 << 20, (1 << 20) + 1, (1 << 32) - 17):
        q.append("Z %d" % n)
        want.append("%d %d" % (set_slots(n), 8 * set_slots(n) + 16 * n + COUNTER_BYTES))
    return q, want


def run_and_compare(exe):
    q, want = queries()
    out = subprocess.run([str(exe)], input="\n".join(q) + "\n", capture_output=True, text=True,
                         timeout=60)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-3000:]
    got = out.stdout.split("\n")
    assert got[len(q)] == "ok %d" % len(q)
    bad = [(a, b, c) for a, b, c in zip(q, got, want) if b != c]
    assert not bad, bad[:5]
    return out


def test_the_stated_rules_on_known_cases():
    assert args_rule(2, 1, 0, 0, -1.0) == A_SIDE  # the first broken rule is the one reported
    assert args_rule(0, 1, 0, 0, -1.0) == A_BOX and args_rule(0, 1, 1, 9, -1.0) == A_CHILDREN
    assert args_rule(1, 0, 0, 8, float("nan")) == A_WEIGHT and args_rule(1, 0, 0, 8, 0.0) == A_OK
    q, want = queries()
    assert {int(w.split()[0]) for a, w in zip(q, want) if a[0] == "A"} == set(range(5))
    assert {int(w.split()[0]) for a, w in zip(q, want) if a[0] == "C"} == set(range(4))
    # 2.0f * (float)vs, not (float)(2 vs) of some other double: both are the same number here,
    # and a neighbouring float is refused
    assert compat_rule(2.0 * 0.1, 0.1, 0.3, 0.3, 2, 2) == C_OK
    assert compat_rule(float(np.nextafter(F(0.2), F(0))), 0.1, 0.3, 0.3, 2, 2) == C_VOXEL
    assert compat_rule(0.2, 0.1, 0.3, 0.3, 0, 2) == C_OK  # the two VDBFusion modes mix
    assert {selected(*s, b) for s in SELECTIONS for b in BRICKS} == {True, False}


def test_every_lane_reads_one_brick_and_aligned_pairs():
    for D in ((0, 0, 0), (-1, -1, -1), (3, -7, 2), (-(1 << 19), (1 << 19) - 1, 0)):
        for l in range(512):
            ch = lane_children(l, D)
            bricks = {c[0] for c in ch}
            assert len(bricks) == 1  # all eight children in one source brick
            b = bricks.pop()
            off = tuple(b[a] - 2 * D[a] for a in range(3))
            assert all(o in (0, 1) for o in off)
            # the child brick is the lane's, whatever D is
            assert off == ((l >> 2) & 1, (l >> 5) & 1, (l >> 8) & 1)
            assert all(-LIM <= v < LIM for v in b)  # packable again
            loc = [c[1] for c in ch]
            assert loc[0] % 2 == 0 and [v - loc[0] for v in loc] == [0, 1, 8, 9, 64, 65, 72, 73]
            assert ch == [(b, v) for v in [c[1] for c in lane_children(l)]]
    # the 512 lanes' children partition the eight child bricks' 4096 voxels
    seen = {(c[0], c[1]) for l in range(512) for c in lane_children(l)}
    assert len(seen) == 4096


def test_the_parent_is_the_floor_and_stays_packable():
    for b in PARENTS:
        assert -(1 << 19) <= b // 2 < (1 << 19)
        assert b // 2 == (b - (b & 1)) // 2 == b >> 1
    for n in (1, 511, 512, 513, 4097, 1 << 20, (1 << 25) + 1, (1 << 32) - 17):
        assert 8 * set_slots(n) + 16 * n + COUNTER_BYTES <= 48 * n + (32 << 10)
        assert set_slots(n) >= 2 * n


def test_coarsen_plan_check(tmp_path):
    exe = tmp_path / "coarsen_plan_check"
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-o", str(exe), SRC])
    run_and_compare(exe)


def test_coarsen_plan_sanitizers(tmp_path):
    """The same program under AddressSanitizer and UndefinedBehaviorSanitizer (host code only): no
    shift of a negative coordinate, no overflow in the set's size."""
    exe = tmp_path / "coarsen_plan_san"
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-o", str(exe), SRC])
    out = run_and_compare(exe)
    assert "runtime error" not in out.stderr and "Sanitizer" not in out.stderr, out.stderr[-3000:]


def test_the_constants_the_header_and_the_tests_rely_on():
    plan = open(PLAN).read()
    assert re.search(r"COARSEN_SET_MIN = %d;" % SET_MIN, plan)
    assert re.search(r"COARSEN_SCRATCH_PER_BRICK = 48;", plan)
    assert re.search(r"COARSEN_SCRATCH_FIXED = 32ull << 10;", plan)
    assert re.search(r"COARSEN_COUNTER_BYTES = \(16 \+ 64 \* 16\) \* 8;", plan)
    assert "hip" not in re.sub(r"//.*", "", plan).lower()  # plain C++: no HIP in the plan
    hdr = open(os.path.join(REPO, "include", "tsdf_hip_coarsen.h")).read()
    hdr = " ".join(re.sub(r"^ \*", "", hdr, flags=re.M).split())
    assert "at most 48 bytes per source brick plus a fixed 32 KiB" in hdr
    dev = open(os.path.join(REPO, "noetic-slam_amd", "csrc", "tsdf_device.h")).read()
    assert re.search(r"COARSEN_SHARDS = 64, COARSEN_SHARD_WORDS = 16, COARSEN_CTR_HEAD = 16;", dev)
    kern = open(os.path.join(REPO, "noetic-slam_amd", "csrc", "tsdf_coarsen.hip")).read()
    assert re.search(r"COARSEN_GRID_CAP = 4096;", kern)
    # one definition of the insertion: the merge's kernel, launched for both
    assert "k_merge_insert" not in re.sub(r"//.*", "", kern) and "launch_merge_insert" in \
        open(os.path.join(REPO, "noetic-slam_amd", "csrc", "tsdf_capi.cpp")).read()
