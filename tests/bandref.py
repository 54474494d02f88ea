"""Band widths, voxel sizes and worst-case rays for the integrate path (test helper; nothing here
calls libtsdf_hip.so).

The band is 2 * sdf_trunc / voxel_size, the length in voxels of the truncation band a ray's walk
covers.  noetic-slam_amd/csrc/ctx_plan.h sizes a ray's pair slots (maxp), sample slots (spr) and the
single walk's register slots (nstep) from it, in double, while the kernels walk with (float)tau and
1.0f / (float)vs.  GRID holds the (voxel_size, sdf_trunc) pairs at which those numbers change, and
two pairs whose band lies below an integer in double and at or above it in float.

adversarial_rays() builds, in numpy alone, the rays at which a walk, its brick runs and its gates
are most likely to go wrong; ray_facts() walks them through the oracle; plan_of() asks ctx_plan.h
itself (tests/cpp/ctx_plan_print.cpp, built with g++) for the plan of a parameter set.
"""
import atexit
import collections
import math
import os
import shutil
import subprocess
import tempfile

import numpy as np

import oracle
from conftest import REPO
from tsdf_map import _abi

F = np.float32
D = np.float64

# (voxel_size, sdf_trunc).  Classes (asserted against ctx_plan.h by tests/test_band_inputs.py, not
# restated here): maxp 4 / 7 / 10; nstep 16 / 32; single walk eligible or not; two straddling
# pairs; voxel sizes other than 0.05 whose floats the other tests never use.
GRID = [
    (0.05, 0.02),            # band 0.8: below one voxel of truncation
    (0.05, 0.05),            # 2: tau == vs
    (0.05, 0.1),             # 4
    (0.03, 0.1),             # 6.67
    (0.07, 0.21),            # 6
    (0.05, 0.173),           # 6.92: the last band of 16 register slots
    (0.05, 0.1733),          # 6.932: the first of 32
    (0.05, 0.175),           # 6.999... in double
    (0.02, 0.07),            # 7: maxp 7, no single walk
    (0.02, 0.06999999993),   # below 7 in double, 7.0000002 in float
    (0.02, 0.14999999985),   # below 15 in double, at or above in float
    (0.07, 0.37),            # 10.57
    (0.0625, 0.5),           # 16: voxel size exact in binary
    (0.1, 1.0),              # 20
]
# the integer each straddling pair's band straddles
STRADDLE = {(0.02, 0.06999999993): 7, (0.02, 0.14999999985): 15}

SEMANTICS = ("vdbfusion", "vdbfusion_f64", "voxblox")
FAMILIES = {1: "diagonal", 2: "grid", 3: "zero", 4: "centre", 5: "negative", 6: "short",
            7: "repeat"}
# rays per family and scan, as adversarial_rays builds them
FAMILY_SIZE = {1: 200, 2: 204, 3: 200, 4: 200, 5: 200, 6: 200, 7: 300}
N_ZERO_DEPTH = 20  # of family 6: p == origin, dropped by every semantics


def band_double(vs, tau):
    return 2.0 * tau / vs


def band_float(vs, tau):
    """The band as the kernels' floats give it, evaluated in double."""
    return 2.0 * float(F(tau)) / float(F(vs))


# ---- the plan, from the header itself -----------------------------------------------------------

Plan = collections.namedtuple("Plan", "maxp spr nstep fused band_vox")
_exe = {}


def _plan_exe():
    if "path" not in _exe:
        d = tempfile.mkdtemp(prefix="ctx_plan_print")
        atexit.register(shutil.rmtree, d, ignore_errors=True)
        exe = os.path.join(d, "ctx_plan_print")
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-o", exe,
                               os.path.join(REPO, "tests", "cpp", "ctx_plan_print.cpp")])
        _exe["path"] = exe
    return _exe["path"]


def _plan_arg(voxel_size, sdf_trunc, space_carving=False, max_range=math.inf, max_points=1 << 18,
              max_batch=32, semantics="vdbfusion_f64", allow_clear=True, walk="two",
              use_const_weight=False, method="simple", **ignored):
    return ",".join([repr(float(voxel_size)), repr(float(sdf_trunc)),
                     str(_abi.SEMANTICS[semantics]),
                     str({"two": _abi.WALK_TWO, "single": _abi.WALK_SINGLE}[walk]),
                     "1" if space_carving else "0", repr(float(max_range)),
                     str(_abi.VB_METHODS[method]), "0" if use_const_weight else "1",
                     "1" if allow_clear else "0", str(int(max_points)), str(int(max_batch))])


def plans_of(param_sets):
    """The sizing plans ctx_plan.h makes for HipTSDFVolume-style keyword dicts (voxel_size and
    sdf_trunc among them), one program run for all."""
    out = subprocess.run([_plan_exe()] + [_plan_arg(**kw) for kw in param_sets],
                         capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stdout + out.stderr
    lines = out.stdout.splitlines()
    assert len(lines) == len(param_sets)
    plans = []
    for kw, line in zip(param_sets, lines):
        assert not line.startswith("refused"), (kw, line)
        a = [int(x) for x in line.split()]
        plans.append(Plan(a[0], a[1], a[2], bool(a[3]), a[4]))
    return plans


def plan_of(**kw):
    return plans_of([kw])[0]


# ---- the rays -----------------------------------------------------------------------------------

# The origins' grid indices per axis (None: a generic coordinate, not on the grid)
ORIGIN_GRID = [(6, None, None), (0, 0, 0), (-16, -24, -7)]
_GENERIC = (0.41, -0.27, 1.13)


def origins_of(vs):
    """Three origins, every coordinate a float32: one with x on a voxel face and generic y, z; the
    grid's origin, a brick corner at the boundary of index 0; a point of the all-negative octant
    on voxel edges, one voxel above a brick face."""
    v = F(vs)
    return [np.array([F(g) if k is None else F(k) * v for k, g in zip(ks, _GENERIC)], F).astype(D)
            for ks in ORIGIN_GRID]


def _unit(rng, n):
    d = rng.normal(size=(n, 3))
    return d / np.linalg.norm(d, axis=1)[:, None]


def _family_rays(vs, tau, o, grid, rng, reach):
    """(points float32 (n, 3), family (n,), zero_depth (n,) bool) of one scan from origin o, whose
    grid indices are `grid` (ORIGIN_GRID)."""
    v32, t32 = F(vs), F(tau)
    vsd, taud = float(v32), float(t32)
    o32 = o.astype(F)
    rlo = min(max(1.0, 2.5 * taud), 0.5 * reach)
    parts = []

    def add(fam, p):
        p = np.ascontiguousarray(p, F).reshape(-1, 3)
        assert p.shape[0] == FAMILY_SIZE[fam], (fam, p.shape)
        parts.append((fam, p))

    # 1. near-diagonal rays of all eight octants, the hit within 0.6 voxel of a brick corner
    p1 = []
    for s in np.array(np.meshgrid([1, -1], [1, -1], [1, -1])).reshape(3, -1).T:
        r = rng.uniform(rlo, 0.9 * reach, size=25)
        target = o[None] + s[None] * r[:, None] / math.sqrt(3.0)
        corner = np.round(target / (8.0 * vsd)) * 8.0
        p1.append((corner.astype(F) * v32).astype(D) + rng.uniform(-0.6, 0.6, (25, 3)) * vsd)
    add(1, np.concatenate(p1))

    # 2. rays along the grid: coordinates that are multiples of float32(vs) where the origin's are,
    #    so that they lie on voxel faces, on voxel edges and through brick corners, and rays along
    #    face and space diagonals, whose t_next tie
    on = np.array([k is not None for k in grid])  # the origin's on-grid axes
    k0 = np.array([0 if k is None else k for k in grid], D)
    mlo, mhi = int(math.ceil(rlo / vsd)), int(math.floor(0.9 * reach / vsd))

    def along(dirs, ms):
        out = []
        for d in dirs:
            d = np.asarray(d, D)
            for m in ms:
                k = k0 + m * d
                q = np.where(on, (k.astype(F) * v32), (o32 + (m * d).astype(F) * v32).astype(F))
                out.append(np.where(d == 0, o32, q))
        return out

    def lengths(n, scale):
        m = np.unique(np.concatenate([
            np.linspace(mlo / scale, mhi / scale, n).round(),
            8 * np.arange(math.ceil(mlo / scale / 8), math.floor(mhi / scale / 8) + 1)]))
        m = m[m > 0]
        idx = np.round(np.linspace(0, m.size - 1, n)).astype(int)
        return m[idx]  # n lengths (with repeats where the range is short), brick planes among them

    axes = [(1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1)]
    face = [(a, b, 0) for a in (1, -1) for b in (1, -1)] + \
           [(a, 0, b) for a in (1, -1) for b in (1, -1)] + \
           [(0, a, b) for a in (1, -1) for b in (1, -1)]
    space = [(a, b, c) for a in (1, -1) for b in (1, -1) for c in (1, -1)]
    p2 = along(axes, lengths(20, 1.0)) + along(face, lengths(5, math.sqrt(2.0))) + \
        along(space, lengths(3, math.sqrt(3.0)))
    assert len(p2) == FAMILY_SIZE[2]
    add(2, np.array(p2))

    # 3. one and two direction components exactly zero (generic lengths), and one component of
    #    about 1e-7 (a few ulp of the origin's coordinate), whose t_step is huge
    p3 = []
    for i in range(66):
        a = i % 3
        d = _unit(rng, 1)[0] * rng.uniform(rlo, 0.9 * reach)
        d[a] = 0.0
        q = (o + d).astype(F)
        q[a] = o32[a]
        p3.append(q)
    for i in range(66):
        a = i % 3
        q = o32.copy()
        q[a] = F(o[a] + (1 if i % 2 else -1) * rng.uniform(rlo, 0.9 * reach))
        p3.append(q)
    for i in range(68):
        a = i % 3
        d = _unit(rng, 1)[0] * rng.uniform(rlo, 0.9 * reach)
        q = (o + d).astype(F)
        ulp = float(np.spacing(np.abs(o32[a]))) if o32[a] != 0 else 1e-7 * np.linalg.norm(d)
        q[a] = F(o[a] + (1 if i % 2 else -1) * (1 + i % 3) * ulp)
        assert q[a] != o32[a]
        p3.append(q)
    add(3, np.array(p3))

    # 4. hits exactly on voxel centres (proj == 0: the skipped voxel), and hits with a voxel centre
    #    at distance tau (1 + k 2^-24) behind them, k over the near-tau window and the F64 gate
    d = _unit(rng, 200)
    tgt = o[None] + d * rng.uniform(rlo, 0.9 * reach, 200)[:, None]
    c = ((np.floor(tgt / vsd).astype(F) + F(0.5)) * v32).astype(F)
    u = c.astype(D) - o[None]
    u /= np.linalg.norm(u, axis=1)[:, None]
    ks = np.array([0, 1, -1, 2, -2, 4, -4, 8, -8, 16, -16, 32, -32], D)
    delta = ks[np.arange(100) % ks.size] * 2.0 ** -24
    behind = c[100:].astype(D) - u[100:] * (taud * (1.0 + delta))[:, None]
    add(4, np.concatenate([c[:100], behind.astype(F)]))

    # 5. hits in every negative octant and within tau of the planes of index 0 (the brick boundary
    #    there), pulled inside `reach`
    p5 = -rng.uniform(0.3, 0.55 * reach, (200, 3))
    near = rng.integers(0, 4, 200)  # axis 0..2 near the plane, 3: none
    sign = rng.choice([-1.0, 1.0], 200)
    for a in range(3):
        m = near == a
        p5[m, a] = rng.uniform(-1.0, 1.0, m.sum()) * taud
    two = rng.random(200) < 0.25  # a second axis near its plane
    a2 = (near + 1) % 3
    for a in range(3):
        m = two & (a2 == a) & (near < 3)
        p5[m, a] = sign[m] * rng.uniform(0.0, 1.0, m.sum()) * vsd
    dd = p5 - o[None]
    dist = np.linalg.norm(dd, axis=1)
    far = dist > 0.9 * reach
    p5[far] = o[None] + dd[far] * (0.9 * reach / dist[far])[:, None]
    add(5, p5)

    # 6. short rays: depth below tau, depth tau within an ulp, depth about vs / 10 -- the band then
    #    starts behind the origin -- and N_ZERO_DEPTH points at the origin itself
    d = _unit(rng, 180)
    d[::9] = np.eye(3)[np.arange(20) % 3] * np.where(np.arange(20) % 2, 1.0, -1.0)[:, None]
    depth = np.concatenate([rng.uniform(0.1, 0.9, 60) * taud,
                            taud * (1.0 + (np.arange(60) % 7 - 3) * 2.0 ** -23),
                            rng.uniform(0.5, 1.5, 60) * vsd / 10.0])
    p6 = np.concatenate([(o[None] + d * depth[:, None]).astype(F),
                         np.repeat(o32[None], N_ZERO_DEPTH, 0)])
    add(6, p6)

    # 7. identical points: long per-voxel runs of one scan
    d7 = np.array([1.7, -1.1, 0.6]) / np.linalg.norm([1.7, -1.1, 0.6])
    add(7, np.repeat((o + d7 * 0.5 * (rlo + 0.9 * reach)).astype(F)[None], FAMILY_SIZE[7], 0))

    pts = np.concatenate([p for _, p in parts]).astype(F)
    fam = np.concatenate([np.full(p.shape[0], f, np.int32) for f, p in parts])
    zero = np.all(pts == o32[None], axis=1)
    return np.ascontiguousarray(pts), fam, zero


_rays = {}


def adversarial_scans(vs, tau, seed=0, reach=6.0):
    """[(points, origin, family, zero_depth)]: one scan per origin of origins_of(vs); family[i] is
    the FAMILIES key of ray i, zero_depth[i] whether the point is the origin itself.  The hits lie
    within `reach` metres of the origin (the default takes rays of 1 to 6 m, 2.5 tau at least)."""
    key = (float(vs), float(tau), int(seed), float(reach))
    if key not in _rays:
        rng = np.random.default_rng([int(seed), int(round(vs * 1e6)), int(round(tau * 1e9))])
        scans = []
        for o, grid in zip(origins_of(vs), ORIGIN_GRID):
            p, fam, zero = _family_rays(vs, tau, o, grid, rng, float(reach))
            for a in (p, fam, zero, o):
                a.setflags(write=False)
            scans.append((p, o, fam, zero))
        _rays[key] = scans
    return _rays[key]


def adversarial_rays(vs, tau, seed=0, reach=6.0):
    """[(points float32 (n, 3), origin float64 (3,))] of adversarial_scans."""
    return [(p, o) for p, o, _, _ in adversarial_scans(vs, tau, seed, reach)]


def tilted(scans):
    """The scans with a pose each: the origin and a tilted unit quaternion (x, y, z, w), as
    tests/test_voxblox.py::_posed_scans poses its scans."""
    out = []
    for j, (p, o) in enumerate(scans):
        a, b = 0.3 * j - 0.2, 0.15 * j
        q = np.array([math.sin(a / 2) * math.cos(b), math.sin(a / 2) * math.sin(b), 0.1 * j,
                      math.cos(a / 2)])
        out.append((p, np.concatenate([np.asarray(o, D)[:3], q])))
    return out


def initial_t_next(p, org, vs, tau):
    """axis_init of the fp32 VDBFusion walk (tsdf_ray.h ray_init), restated: the three initial
    t_next of every ray (n, 3) float32, inf for a zero component."""
    p = np.asarray(p, F)
    o = np.asarray(org, D).astype(F)
    v32, t32 = F(vs), F(tau)
    inv = F(1.0) / v32
    with np.errstate(all="ignore"):
        d = p - o[None]
        depth = np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])
        u = d / depth[:, None]
        t0i = (depth - t32) * inv
        s = (o * inv)[None] + u * t0i[:, None]
        v = np.floor(s)
        iu = F(1.0) / u
        tn = np.where(u > 0, t0i[:, None] + ((v + F(1.0)) - s) * iu,
                      np.where(u < 0, t0i[:, None] + (v - s) * iu, F(np.inf))).astype(F)
    tn[~(depth > 0)] = np.nan
    return tn


def finite_ties(tn):
    """Rays with two equal finite initial t_next values."""
    with np.errstate(all="ignore"):
        eq = lambda a, b: np.isfinite(tn[:, a]) & (tn[:, a] == tn[:, b])
        return eq(0, 1) | eq(0, 2) | eq(1, 2)


# ---- the reference facts ------------------------------------------------------------------------

ORACLE_DROPS = ("max_batch", "pipeline", "walk", "max_points", "max_bricks", "max_bricks_hard")


def oracle_volume(vs, tau, **kw):
    for k in ORACLE_DROPS:
        kw.pop(k, None)
    return oracle.OracleTSDFVolume(vs, tau, **kw)


RayFacts = collections.namedtuple("RayFacts", "visited gated runs kept")


def ray_facts(oracle_vol, scan):
    """Every ray of scan = (points, origin or pose) through the oracle's own walk: visited (the
    DDA's voxels, -1 for a dropped ray), gated (the voxels handed to the fuse) and runs (the
    distinct-brick runs among them: k_count's pairs) per ray, and the number of rays kept.
    method="merged": per bundle."""
    visited, gated, runs = oracle_vol.ray_facts(scan[0], scan[1])
    return RayFacts(visited, gated, runs, int(np.count_nonzero(visited >= 0)))
