"""numpy restatement of the raycast of include/tsdf_hip_raycast.h (test helper) on top of
sampleref.sample: the full march, every lattice sample of every ray that has not hit yet, with no
skipping.  Every fp32 expression is written in the order the header states, so the kernel (built
with -ffp-contract=off) reproduces it bit for bit.  Vectorised over the rays, a loop over k.
"""
import numpy as np

import sampleref as sr

F = np.float32
NEAREST = sr.NEAREST
TRILINEAR = sr.TRILINEAR
MAX_SAMPLES = 1 << 20


def lattice(t_min, t_max, step):
    """t_k = t_min + (float)k * step for k = 0, 1, ... while t_k <= t_max and k < 2^20 (fp32)."""
    t_min, t_max, step = F(t_min), F(t_max), F(step)
    n = min(MAX_SAMPLES, int((float(t_max) - float(t_min)) / float(step)) + 4)
    while True:
        with np.errstate(over="ignore"):
            t = (t_min + (np.arange(n).astype(F) * step).astype(F)).astype(F)
        ok = t <= t_max
        if not ok[-1] or n == MAX_SAMPLES:
            break
        n = min(MAX_SAMPLES, 2 * n)
    cnt = int(ok.sum())
    assert ok[:cnt].all()  # monotone: the passing k form a prefix
    return t[:cnt]


def rays_of(org, dirs, pose=None):
    """(o, d) fp32 (n, 3): the rays as given, or under the 3x4 pose rounded to fp32:
    o = ((r0 x + r1 y) + r2 z) + t, d = (r0 x + r1 y) + r2 z."""
    d = np.asarray(dirs, F).reshape(-1, 3)
    o = np.asarray(org, F)
    o = np.ascontiguousarray(np.broadcast_to(o, d.shape))
    if pose is None:
        return o, np.ascontiguousarray(d)
    m = np.asarray(pose, np.float64)[:3].reshape(3, 4).astype(F)
    x, y, z = d[:, 0], d[:, 1], d[:, 2]
    with np.errstate(invalid="ignore", over="ignore"):
        dd = [((m[r, 0] * x + m[r, 1] * y).astype(F) + m[r, 2] * z).astype(F) for r in range(3)]
    return sr.transform(m, o), np.stack(dd, 1)


def points_at(o, d, t):
    """p = o + t * d per axis (fp32; t a scalar or an (n,) array)."""
    t = np.asarray(t, F)
    if t.ndim:
        t = t[:, None]
    with np.errstate(invalid="ignore", over="ignore"):
        return (o + (t * d).astype(F)).astype(F)


def raycast(field, org, dirs, pose=None, t_min=0.0, t_max=100.0, step=0.05, mode=NEAREST,
            min_weight=0.0, stats=None):
    """(depth (n,) fp32, normal (n, 3) fp32, hit (n,) uint8).  stats, a dict, receives
    "lattice" (samples per ray of the full lattice) and "marched" (samples taken, all rays)."""
    o, d = rays_of(org, dirs, pose)
    n = d.shape[0]
    t = lattice(t_min, t_max, step)
    depth = np.zeros(n, F)
    hit = np.zeros(n, np.uint8)
    ps = np.zeros(n, F)
    pv = np.zeros(n, bool)
    act = np.arange(n)
    marched = 0
    for k in range(t.shape[0]):
        if not act.size:
            break
        marched += act.size
        s, _, _, v = sr.sample(field, points_at(o[act], d[act], t[k]), mode, min_weight)
        v = v.astype(bool)
        if k >= 1:
            h = pv[act] & v & (ps[act] > 0) & (s <= 0)
            if h.any():
                i = act[h]
                t0 = t[k - 1]
                with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
                    frac = (ps[i] / (ps[i] - s[h]).astype(F)).astype(F)
                    depth[i] = (t0 + ((t[k] - t0) * frac).astype(F)).astype(F)
                hit[i] = 1
                act, s, v = act[~h], s[~h], v[~h]
        pv[act] = v
        ps[act] = s
    if stats is not None:
        stats["lattice"] = int(t.shape[0])
        stats["marched"] = int(marched)
    normal = np.zeros((n, 3), F)
    hb = hit.astype(bool)
    if hb.any():
        _, _, g, gv = sr.sample(field, points_at(o[hb], d[hb], depth[hb]), TRILINEAR, min_weight)
        with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
            n2 = ((g[:, 0] * g[:, 0] + g[:, 1] * g[:, 1]).astype(F) + g[:, 2] * g[:, 2]).astype(F)
            ok = gv.astype(bool) & (n2 > 0)
            nn = (g / np.sqrt(n2).astype(F)[:, None]).astype(F)
        normal[hb] = np.where(ok[:, None], nn, F(0))
    return depth, normal, hit


def base_bricks(field, o, d, t, mode):
    """(len(t), n, 3) float: per lattice sample and ray, the brick coordinate of the sample's base
    voxel -- floorf(p inv) (nearest) or floorf(p inv - 0.5f) (trilinear), floor-divided by 8 as
    the kernel's >> 3 does.  Kept in floating point, so a sample off the index domain (+-inf
    included) has a coordinate too: what the kernel's skip relies on is monotone in k on all of
    them."""
    out = np.empty((t.shape[0],) + d.shape, np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        for k in range(t.shape[0]):
            u = (points_at(o, d, t[k]) * field.inv).astype(F)
            if mode == TRILINEAR:
                u = (u - F(0.5)).astype(F)
            out[k] = np.floor(np.floor(u).astype(np.float64) / 8.0)
    return out


# ---- the shared test workload ---------------------------------------------------------------------
N_SCANS = 8
T_MIN, T_MAX, STEP = 0.5, 40.0, 0.05
DISPLACED = (0.3, -0.2, 0.1)
# hits of the 2048 test rays on the oracle's 8-scan maps at step 0.05, (nearest, trilinear), as
# this reference measured them (test_raycast_ref.py asserts them there, test_raycast_gpu.py on the
# GPU's field)
HITS = {("vdbfusion_f64", "scan", 0.0): (2048, 647), ("vdbfusion_f64", "scan", 2.0): (1856, 538),
        ("vdbfusion_f64", "displaced", 0.0): (876, 733),
        ("voxblox", "scan", 0.0): (2048, 657), ("voxblox", "displaced", 0.0): (873, 735)}


def scan_rays(points, origin):
    """The tests' rays: every 64th point of the scan with range > 0.5 m, seen from the scan's
    origin: (origin fp32 (3,), unit directions fp32 (n, 3), ranges float64 (n,))."""
    p = np.asarray(points, np.float64)[::64]
    v = p - np.asarray(origin, np.float64)
    r = np.linalg.norm(v, axis=1)
    v, r = v[r > 0.5], r[r > 0.5]
    return np.asarray(origin, F), np.ascontiguousarray((v / r[:, None]).astype(F)), r
