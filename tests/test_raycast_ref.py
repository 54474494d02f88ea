"""Pins tests/rayref.py, the numpy restatement the GPU's raycast is compared with
(test_raycast_gpu.py): an analytic plane, the monotonicity the kernel's brick skip rests on, and
the 8-scan map of the oracle's field — CPU suite.  The oracle does not raycast; its field is
bitwise the GPU's, so what holds for the reference here holds for it there."""
import numpy as np
import pytest

import rayref as rr
import sampleref as sr

F = np.float32
VS, TAU = sr.VOXEL_SIZE, sr.SDF_TRUNC

HITS = rr.HITS


# ---- analytic plane -------------------------------------------------------------------------------
X0 = 4.03  # the plane x = X0, seen from x < X0


@pytest.fixture(scope="module")
def plane():
    """A slab of voxels around the plane: S = X0 - x_centre where |S| <= tau, W = 1."""
    i = np.arange(30, 52)
    s = X0 - (i + 0.5) * VS
    keep = np.abs(s) <= TAU
    i, s = i[keep], s[keep]
    assert i.size == 6
    x, y, z = np.meshgrid(i, np.arange(-12, 90), np.arange(-6, 6), indexing="ij")
    ijk = np.stack([x, y, z], -1).reshape(-1, 3)
    sv = (X0 - (ijk[:, 0] + 0.5) * VS).astype(F)
    return sr.Field((ijk, sv, np.ones(ijk.shape[0], F)), VS, TAU)


@pytest.mark.parametrize("deg", [0, 30, 60])
def test_plane_depth_and_normal(plane, deg):
    a = np.deg2rad(deg)
    o = np.array([0.02, 0.013, 0.07], F)
    d = np.array([[np.cos(a), np.sin(a), 0.0]], F)
    exact = (X0 - float(o[0])) / float(d[0, 0])
    assert exact <= 10.0
    depth, normal, hit = rr.raycast(plane, o, d, None, 0.0, 12.0, 0.05, rr.TRILINEAR)
    print("incidence %d deg: depth %.6f, analytic %.6f, normal %s" % (deg, depth[0], exact, normal[0]))
    assert hit[0] == 1
    assert abs(float(depth[0]) - exact) < 1e-4
    assert np.abs(normal[0].astype(np.float64) - [-1.0, 0.0, 0.0]).max() < 1e-5
    # nearest: a staircase of the same field, within a voxel of it
    dn, _, hn = rr.raycast(plane, o, d, None, 0.0, 12.0, 0.05, rr.NEAREST)
    assert hn[0] == 1 and abs(float(dn[0]) - exact) < VS / float(d[0, 0])


def test_plane_from_behind_does_not_hit(plane):
    o = np.array([[6.0, 0.5, 0.0], [4.2, 0.5, 0.0]], F)  # beyond the slab, and inside it at S < 0
    d = np.array([[-1.0, 0.0, 0.0], [-1.0, 0.0, 0.0]], F)
    for mode in (rr.NEAREST, rr.TRILINEAR):
        depth, normal, hit = rr.raycast(plane, o, d, None, 0.0, 12.0, 0.05, mode)
        assert not hit.any() and not depth.any() and not normal.any()
    # ... and the same rays turned round, from in front, do
    depth, _, hit = rr.raycast(plane, np.array([2.0, 0.5, 0.0], F), -d[:1], None, 0.0, 12.0, 0.05,
                               rr.TRILINEAR)
    assert hit[0] == 1 and abs(float(depth[0]) - (X0 - 2.0)) < 1e-4


# ---- monotonicity: what the kernel's skip rests on ------------------------------------------------
def finite_rays(n, seed):
    rng = np.random.default_rng(seed)
    o = rng.uniform(-30.0, 30.0, (n, 3))
    d = rng.normal(size=(n, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    d[n // 8: n // 4] *= rng.uniform(0.01, 100.0, (n // 4 - n // 8, 1))  # not unit length
    z = rng.integers(0, 3, n)
    d[np.arange(n // 4), z[: n // 4]] = 0.0  # zero components
    d[: n // 16] = 0.0  # zero directions
    d[n // 16: n // 8, 1] *= -0.0
    # origins at the edge of the index domain, on either side of it
    edge = (2 ** 23 - 10) * VS
    k = np.arange(n - n // 4, n)
    o[k, rng.integers(0, 3, k.size)] = edge * rng.choice([-1.0, 1.0], k.size)
    return o.astype(F), d.astype(F)


@pytest.mark.parametrize("mode", [rr.NEAREST, rr.TRILINEAR])
def test_base_brick_is_monotone_along_a_ray(mode):
    o, d = finite_rays(1024, 11)
    assert (d < 0).any() and (d == 0).any() and (np.abs(o) > 8e5).any()
    field = sr.Field((np.zeros((1, 3), np.int64), [0.0], [1.0]), VS, TAU)
    for step in (0.03, 0.05):
        t = rr.lattice(0.0, 40.0, step)
        assert t.shape[0] in (int(40 / step), int(40 / step) + 1)
        b = rr.base_bricks(field, o, d, t, mode)
        assert not np.isnan(b).any()
        up = np.all(b[1:] >= b[:-1], axis=0)
        down = np.all(b[1:] <= b[:-1], axis=0)
        assert np.all(up | down), np.argwhere(~(up | down))[:5]
        # the rays move: the property is not vacuous
        assert (b[-1] != b[0]).any(axis=1).mean() > 0.5
    assert float(F(0.03)) != 0.03  # a step fp32 does not represent


@pytest.mark.parametrize("mode", [rr.NEAREST, rr.TRILINEAR])
def test_base_brick_is_monotone_when_the_ray_overflows(mode):
    o, d = finite_rays(256, 5)
    d = (d * F(1e36)).astype(F)  # |d| up to 1e38: finite, and t * d overflows within the lattice
    assert np.isfinite(d).all()
    field = sr.Field((np.zeros((1, 3), np.int64), [0.0], [1.0]), VS, TAU)
    t = rr.lattice(0.0, 40.0, 0.03)
    b = rr.base_bricks(field, o, d, t, mode)
    assert np.isinf(b).any() and not np.isnan(b).any()
    up = np.all(b[1:] >= b[:-1], axis=0)
    down = np.all(b[1:] <= b[:-1], axis=0)
    assert np.all(up | down)


def test_lattice_is_not_accumulated():
    t = rr.lattice(0.5, 40.0, 0.03)
    k = np.arange(t.shape[0])
    assert np.array_equal(t, (F(0.5) + (k.astype(F) * F(0.03)).astype(F)).astype(F))
    assert t[-1] <= F(40.0) < F(0.5) + F(t.shape[0]) * F(0.03)
    assert rr.lattice(1.0, 1.0, 0.05).tolist() == [1.0]


# ---- the oracle's 8-scan map ----------------------------------------------------------------------
@pytest.fixture(scope="module")
def scans(sim):
    return [sim.scan(k) for k in range(rr.N_SCANS)]


def oracle_field(scans, sem):
    import oracle
    v = oracle.OracleTSDFVolume(VS, TAU, semantics=sem)
    for pts, org in scans:
        assert pts.shape[0] == 131072
        v.integrate(pts, org)
    return sr.field_of(v)


@pytest.fixture(scope="module")
def field(scans):
    return oracle_field(scans, "vdbfusion_f64")


@pytest.mark.parametrize("min_weight", [0.0, 2.0])
def test_scan_rays_find_the_scanned_surface(field, scans, min_weight):
    org, dirs, rng = rr.scan_rays(*scans[0])
    assert dirs.shape == (2048, 3)
    got = {}
    for name, mode in (("nearest", rr.NEAREST), ("trilinear", rr.TRILINEAR)):
        st = {}
        depth, normal, hit = rr.raycast(field, org, dirs, None, rr.T_MIN, rr.T_MAX, rr.STEP, mode,
                                        min_weight, st)
        h = hit.astype(bool)
        err = float(np.median(np.abs(depth[h] - rng[h])))
        print("%s min_weight %g: %d of %d hit, median |depth - range| %.4f m, marched %.3f of the "
              "lattice" % (name, min_weight, h.sum(), h.size, err,
                           st["marched"] / (st["lattice"] * h.size)))
        got[name] = (int(h.sum()), err)
        assert not depth[~h].any() and not normal[~h].any()
        assert np.all((depth[h] >= F(rr.T_MIN)) & (depth[h] <= F(rr.T_MAX)))
        nn = np.linalg.norm(normal[h].astype(np.float64), axis=1)
        assert np.all((np.abs(nn - 1) < 1e-6) | (nn == 0))
        if mode == rr.TRILINEAR:
            # a trilinear hit lies in an observed cube; the normal faces the sensor
            assert (nn > 0).mean() > 0.99
            assert (np.einsum("ij,ij->i", normal[h], dirs[h]) < 0).mean() > 0.95
    if min_weight == 0:
        assert got["nearest"][0] / 2048 >= 0.95
    assert got["trilinear"][0] / 2048 >= 0.2
    assert got["nearest"][1] < VS / 2
    assert got["trilinear"][1] < VS / 4
    assert (got["nearest"][0], got["trilinear"][0]) == HITS[("vdbfusion_f64", "scan", min_weight)]


@pytest.mark.parametrize("sem", ["vdbfusion_f64", "voxblox"])
def test_displaced_rays_hit_counts(field, scans, sem):
    """The displaced origin's hit counts the GPU tests assert, measured here on the oracle's
    field; for Voxblox also the undisplaced ones."""
    f = field if sem == "vdbfusion_f64" else oracle_field(scans, sem)
    org, dirs, _ = rr.scan_rays(*scans[0])
    sets = [("displaced", (org + np.array(rr.DISPLACED, F)).astype(F))]
    if sem == "voxblox":
        sets.append(("scan", org))
    for name, o in sets:
        got = tuple(int(rr.raycast(f, o, dirs, None, rr.T_MIN, rr.T_MAX, rr.STEP, mode)[2].sum())
                    for mode in (rr.NEAREST, rr.TRILINEAR))
        print(sem, name, got)
        assert got == HITS[(sem, name, 0.0)]


# ---- tsdf_map.render ------------------------------------------------------------------------------
def test_spherical_rays_are_unit_and_column_major():
    from tsdf_map import render
    lo, hi = np.deg2rad(-20.0), np.deg2rad(15.0)
    r = render.spherical_rays(16, 64, lo, hi)
    assert r.shape == (1024, 3) and r.dtype == F and r.flags["C_CONTIGUOUS"]
    assert np.abs(np.linalg.norm(r.astype(np.float64), axis=1) - 1).max() < 1e-6
    col = r.reshape(64, 16, 3)  # [column][beam]: a column's beams share the azimuth
    az = np.arctan2(col[..., 1], col[..., 0])
    assert np.abs(az - az[:, :1]).max() < 1e-6
    assert np.allclose(az[:, 0], np.angle(np.exp(-2j * np.pi * np.arange(64) / 64)), atol=1e-6)
    el = np.arcsin(col[..., 2].astype(np.float64))
    assert np.allclose(el, np.linspace(lo, hi, 16)[None, :], atol=1e-6)
    assert np.allclose(render.spherical_rays(1, 4, 0.0, 0.0),
                       [[1, 0, 0], [0, -1, 0], [-1, 0, 0], [0, 1, 0]], atol=1e-6)
    with pytest.raises(ValueError):
        render.spherical_rays(0, 4, 0.0, 1.0)
