"""tests/esdfref.py, the numpy restatement of include/tsdf_hip_esdf.h that the GPU tests compare
against, held to a brute-force minimum over all sites, to known answers, to an analytic sphere and
to conditions that keep the shared fixture from being vacuous.  The fields come from the oracle;
CPU suite."""
import numpy as np
import pytest

import esdfref as er
import sampleref as sr

F = np.float32
VS = sr.VOXEL_SIZE


@pytest.fixture(scope="module")
def volumes(scan0):
    import oracle
    pts, org = scan0
    out = {}
    for sem, p in (("vdbfusion_f64", pts), ("voxblox", np.ascontiguousarray(pts[::2]))):
        v = oracle.OracleTSDFVolume(VS, sr.SDF_TRUNC, semantics=sem)
        v.integrate(p, org)
        out[sem] = v
    yield out
    for v in out.values():
        v.close()


def synthetic(voxels, sem="vdbfusion_f64"):
    import oracle
    v = oracle.OracleTSDFVolume(VS, sr.SDF_TRUNC, semantics=sem)
    v.import_bricks(*er.make_bricks(voxels, 0.0 if sem == "voxblox" else F(sr.SDF_TRUNC)))
    return v


@pytest.mark.parametrize("radius", [1, 3, 6, 128])
@pytest.mark.parametrize("sem", ["vdbfusion_f64", "voxblox"])
def test_separable_passes_equal_brute_force(volumes, sem, radius):
    v = volumes[sem]
    c = er.smallest_abs_voxel(v)
    lo, hi = c - np.array([9, 7, 5]), c + np.array([10, 7, 6])
    S, W = v.query_dense(lo, hi)
    assert S.shape == (11, 14, 19)
    observed, site = er.classify(S, W, VS, 0.0)
    print("%s R %d: %d sites" % (sem, radius, site.sum()))
    assert site.sum() >= 50 and not site.all()
    sep, brute = er.squared(site, radius), er.brute_squared(site, radius)
    r2 = radius * radius
    assert np.array_equal(np.minimum(sep, r2 + 1), np.minimum(brute, r2 + 1))
    a = er.finish(sep, S, observed, site, radius, VS)
    b = er.finish(brute, S, observed, site, radius, VS)
    er.assert_same(a, b)
    er.assert_same(er.esdf(S, W, VS, radius, VS), a)


def test_one_site():
    v = synthetic({(3, -2, 5): (0.01, 1.0)})
    lo, hi = np.array([-6, -12, -3]), np.array([12, 7, 14])
    S, W = v.query_dense(lo, hi)
    for radius in (4, 9, 30):
        dist, flags = er.esdf(S, W, VS, radius, VS)
        k, j, i = np.meshgrid(*[np.arange(a, b) for a, b in zip(lo[::-1], hi[::-1])], indexing="ij")
        d2 = (i - 3) ** 2 + (j + 2) ** 2 + (k - 5) ** 2
        capped = d2 > radius * radius
        want = np.sqrt(np.where(capped, radius * radius, d2).astype(F)) * F(VS)
        assert np.array_equal(er.bits(dist), er.bits(want))
        assert capped.any() or radius == 30
        site = d2 == 0
        assert np.array_equal(flags, site * (er.OBSERVED | er.SITE) + capped * er.CAPPED)
    v.close()


def test_tie_sign_and_unobserved():
    # two sites on a line with a voxel halfway; one lies behind the surface; an observed voxel off
    # the band on either side of the surface; everything else unobserved
    v = synthetic({(0, 0, 0): (0.02, 1.0), (4, 0, 0): (-0.03, 2.0),
                   (2, 1, 0): (0.25, 1.0), (2, -1, 0): (-0.25, 1.0)})
    lo, hi = np.array([-3, -3, -2]), np.array([8, 4, 3])
    S, W = v.query_dense(lo, hi)
    dist, flags = er.esdf(S, W, VS, 5, VS)

    def at(x, y, z):
        return dist[z - lo[2], y - lo[1], x - lo[0]], flags[z - lo[2], y - lo[1], x - lo[0]]
    d, f = at(2, 0, 0)  # the tie: 2 voxels from either site, unobserved, positive, flags 0
    assert d == F(2) * F(VS) and f == 0 and not np.signbit(d)
    d, f = at(0, 0, 0)
    assert er.bits(d) == 0 and f == er.OBSERVED | er.SITE
    d, f = at(4, 0, 0)  # a site behind the surface reads -0.0f
    assert er.bits(d) == 0x80000000 and f == er.OBSERVED | er.SITE
    d, f = at(2, 1, 0)
    assert d == np.sqrt(F(5)) * F(VS) and f == er.OBSERVED
    d, f = at(2, -1, 0)
    assert d == -(np.sqrt(F(5)) * F(VS)) and f == er.OBSERVED
    d, f = at(-3, 3, 2)  # 9 + 9 + 4 = 22 <= 25
    assert d == np.sqrt(F(22)) * F(VS) and f == 0
    d, f = at(7, -3, -2)  # 9 + 9 + 4 from (4, 0, 0)
    assert d == np.sqrt(F(22)) * F(VS) and f == 0
    # min_weight 2 leaves the site of weight 2 only
    dist2, flags2 = er.esdf(S, W, VS, 5, VS, min_weight=2.0)
    assert flags2[0 - lo[2], 0 - lo[1], 0 - lo[0]] == 0
    assert dist2[0 - lo[2], 0 - lo[1], 0 - lo[0]] == F(4) * F(VS)
    # the box is the world: a box without (4, 0, 0) does not see it
    S3, W3 = v.query_dense(lo, np.array([4, 4, 3]))
    dist3, flags3 = er.esdf(S3, W3, VS, 5, VS)
    assert dist3[0 - lo[2], 0 - lo[1], 3 - lo[0]] == F(3) * F(VS)
    # a site band of 0.025 keeps (0, 0, 0) only
    dist4, flags4 = er.esdf(S, W, VS, 5, 0.025)
    assert flags4[0 - lo[2], 0 - lo[1], 4 - lo[0]] == er.OBSERVED
    assert dist4[0 - lo[2], 0 - lo[1], 4 - lo[0]] == -(F(4) * F(VS))
    v.close()


def test_analytic_sphere():
    """S the exact signed distance to a sphere, clipped to the band.  A site's centre lies within
    site_band of the surface, so no voxel reads less than its true distance minus site_band; the
    voxel holding the nearest surface point has its centre within (sqrt(3) / 2) vs of it and is a
    site once site_band >= (sqrt(3) / 2) vs, so no voxel reads more than the true distance plus
    that.  (eps: the float32 rounding of S, of the centres and of the result.)"""
    centre, rad, tau = np.array([0.03, -0.02, 0.05]), 1.0, sr.SDF_TRUNC
    n = 16  # voxels -16..15 per axis: the sphere (10 voxels) and a margin
    k, j, i = np.meshgrid(*[np.arange(-n, n)] * 3, indexing="ij")
    p = (np.stack([i, j, k], -1) + 0.5) * VS
    true = np.linalg.norm(p - centre, axis=-1) - rad
    S = np.clip(true, -tau, tau).astype(F)
    b = np.arange(-n // 8, n // 8)
    bz, by, bx = np.meshgrid(b, b, b, indexing="ij")
    coords = np.stack([bx, by, bz], -1).reshape(-1, 3).astype(np.int32)
    sdf = S.reshape(4, 8, 4, 8, 4, 8).transpose(0, 2, 4, 1, 3, 5).reshape(-1, 8, 8, 8)
    import oracle
    v = oracle.OracleTSDFVolume(VS, tau)
    v.import_bricks(coords, sdf, np.ones_like(sdf))
    S2, W2 = v.query_dense([-n] * 3, [n] * 3)
    assert np.array_equal(S2, S) and (W2 == 1).all()
    dist, flags = er.esdf(S2, W2, VS, 60, VS)
    assert not (flags & er.CAPPED).any() and (flags & er.OBSERVED).all()
    assert np.array_equal(np.signbit(dist), true < 0)
    err = np.abs(dist.astype(np.float64)) - np.abs(true)
    eps = 1e-5
    print("sphere: |dist| - |d*| in [%.4f, %.4f] vs" % (err.min() / VS, err.max() / VS))
    assert err.min() >= -VS - eps and err.max() <= np.sqrt(3) / 2 * VS + eps
    v.close()


FIXTURE_FLOORS = {"sites": 500, "capped": 10000, "uncapped_non_sites": 10000, "negative": 1000}


def test_the_shared_fixture_is_not_vacuous(volumes, scan0):
    c = er.fixture_centre(scan0)
    assert tuple(c) == (80, -51, -18)
    lo, hi = er.fixture_box(c)
    for sem, v in volumes.items():
        S, W = v.query_dense(lo, hi)
        assert S.shape == (33, 80, 97)
        dist, flags = er.esdf(S, W, VS, 12, VS)
        site, capped = (flags & er.SITE) != 0, (flags & er.CAPPED) != 0
        got = {"sites": site.sum(), "capped": capped.sum(),
               "uncapped_non_sites": (~capped & ~site).sum(), "negative": np.signbit(dist).sum()}
        print(sem, got)
        for k, floor in FIXTURE_FLOORS.items():
            assert got[k] >= floor, (sem, k, got[k])
        observed, site = er.classify(S, W, VS, 0.0)
        d2 = er.squared(site, 40)
        assert d2.max() <= 40 * 40  # at R = 40 nothing is capped
        if sem == "vdbfusion_f64":
            assert np.unique(d2).size >= 1000


def test_box_around_and_grid():
    from tsdf_map import EsdfGrid, box_around
    lo, hi = box_around([0.0, -0.25, 1.03], 0.2, 0.1)
    # floor(-2) = -2, floor(2) + 1 = 3; floor(-4.5) = -5, floor(-0.5) + 1 = 0; floor(8.3), floor(12.3) + 1
    assert lo.tolist() == [-2, -5, 8] and hi.tolist() == [3, 0, 13]
    lo, hi = box_around([0.05, 0.05, 0.05], [0.0, 0.1, 0.3], 0.1)
    assert lo.tolist() == [0, -1, -3] and hi.tolist() == [1, 2, 4]
    # a hand-made grid: dist = 0.1 (x - 1) + 0.2 (y + 2) - 0.3 (z - 5), voxels (1.., -2.., 5..)
    z, y, x = np.meshgrid(np.arange(3), np.arange(4), np.arange(5), indexing="ij")
    dist = (0.1 * x + 0.2 * y - 0.3 * z).astype(F)
    flags = ((x + y + z) % 2).astype(np.uint8)
    g = EsdfGrid(dist, flags, [1, -2, 5], 0.1)
    assert g.hi.tolist() == [6, 2, 8]
    pts = np.array([[0.15, -0.15, 0.55],   # voxel (1, -2, 5): index (0, 0, 0)
                    [0.59, 0.19, 0.79],    # voxel (5, 1, 7): index (4, 3, 2)
                    [0.61, 0.0, 0.65],     # x = 6: outside
                    [0.3, -0.21, 0.6],     # y = -3: outside
                    [np.nan, 0.0, 0.6], [np.inf, 0.0, 0.6]])
    cl = g.clearance(pts)
    assert cl.dtype == F and cl[0] == dist[0, 0, 0] and cl[1] == dist[2, 3, 4]
    assert np.isnan(cl[2:]).all()
    assert g.known(pts).tolist() == [False, True, False, False, False, False]
    gr = g.gradient()
    assert gr.shape == (3, 4, 5, 3)
    assert np.allclose(gr[..., 0], 1.0, atol=1e-5) and np.allclose(gr[..., 1], 2.0, atol=1e-5)
    assert np.allclose(gr[..., 2], -3.0, atol=1e-5)
    flat = EsdfGrid(dist[:1], flags[:1], [1, -2, 5], 0.1).gradient()
    assert (flat[..., 2] == 0).all() and np.allclose(flat[..., 0], 1.0, atol=1e-5)
