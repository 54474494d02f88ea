"""Pins tests/sampleref.py, the numpy restatement the GPU's sparse map queries are compared with
(test_sample_gpu.py), on the oracle's field — CPU suite.  The oracle does not sample; its field is
bitwise the GPU's, so what holds for the reference here holds for it there."""
import numpy as np
import pytest

import sampleref as sr

F = np.float32


@pytest.fixture(scope="module")
def vol(scan0):
    import oracle
    pts, org = scan0
    assert pts.shape[0] == 131072
    v = oracle.OracleTSDFVolume(sr.VOXEL_SIZE, sr.SDF_TRUNC, semantics="vdbfusion_f64")
    v.integrate(pts, org)
    return v


@pytest.fixture(scope="module")
def field(vol):
    return sr.field_of(vol)


@pytest.fixture(scope="module")
def queries(scan0):
    return sr.jitter_queries(*scan0)


def test_nearest_equals_query_dense(vol, field, queries):
    """Nearest sampling reads the voxel tsdf_query_dense reads: the same (S, W) bits over a box
    around the scan's densest part, queried at jittered positions inside each voxel."""
    near =queries[np.argmin(np.abs(queries - np.median(queries, axis=0)).sum(1))]
    c = np.floor(near / sr.VOXEL_SIZE).astype(np.int64)  # a voxel on the surface
    lo, hi = c - np.array([24, 24, 12]), c + np.array([24, 24, 12])
    s, w = vol.query_dense(lo, hi)
    z, y, x = np.meshgrid(np.arange(lo[2], hi[2]), np.arange(lo[1], hi[1]),
                          np.arange(lo[0], hi[0]), indexing="ij")
    ijk = np.stack([x, y, z], -1).reshape(-1, 3)
    assert (w > 0).sum() > 1000 and (w == 0).sum() > 1000
    off = np.random.default_rng(3).uniform(0.05, 0.95, ijk.shape)
    p = ((ijk + off) * sr.VOXEL_SIZE).astype(F)
    # the queries really fall into their voxels (fp32 rounding of the product included)
    assert np.array_equal(np.floor((p * field.inv).astype(F)).astype(np.int64), ijk)
    rs, rw, rg, rv = sr.sample(field, p, sr.NEAREST)
    assert np.array_equal(rs.view(np.uint32), s.reshape(-1).view(np.uint32))
    assert np.array_equal(rw.view(np.uint32), w.reshape(-1).view(np.uint32))
    assert not rg.any()
    assert np.array_equal(rv.astype(bool), w.reshape(-1) > 0)
    # min_weight gates valid only
    _, rw2, _, rv2 = sr.sample(field, p, sr.NEAREST, min_weight=2.0)
    assert np.array_equal(rw2, rw) and np.array_equal(rv2.astype(bool), rw >= 2)


def test_nearest_outside_the_domain_reads_the_background(field):
    big = F(2.0 ** 23) * field.vs
    p = np.array([[big, 0, 0], [-big * 2, 0, 0], [np.nan, 0, 0], [0, np.inf, 0], [0, 0, -np.inf]], F)
    s, w, g, v = sr.sample(field, p, sr.NEAREST)
    assert np.all(s == field.bg) and not w.any() and not g.any() and not v.any()


def test_trilinear_at_voxel_centres_returns_the_voxel(vol, field):
    """At the exact centre of a voxel whose surrounding cubes are observed, f = 0 on every axis and
    the interpolant is that voxel's S, bit for bit."""
    ijk, s, w = vol.export_voxels()
    ijk = ijk.astype(np.int64)
    p = ((ijk + 0.5) * sr.VOXEL_SIZE).astype(F)
    u = ((p * field.inv).astype(F) - F(0.5)).astype(F)
    exact = np.all(u == ijk, axis=1)  # centres whose fp32 image lands on the voxel exactly
    assert exact.mean() > 0.5
    rs, rw, rg, rv = sr.sample(field, p[exact], sr.TRILINEAR)
    v = rv.astype(bool)
    assert v.sum() > 1000
    assert np.array_equal(rs[v].view(np.uint32), s[exact][v].view(np.uint32))
    assert np.all(rw[v] <= w[exact][v]) and np.all(rw[v] > 0)
    assert np.all(rs[~v] == field.bg) and not rw[~v].any() and not rg[~v].any()


def test_trilinear_is_the_interpolant_and_its_gradient(field, queries):
    """Against a float64 evaluation of the same polynomial: values agree to fp32 rounding, and the
    gradient is the derivative (central differences of the float64 interpolant inside the cube)."""
    s, w, g, v = sr.sample(field, queries, sr.TRILINEAR)
    v = v.astype(bool)
    q = queries[v][:2000]
    u = (q * field.inv).astype(F) - F(0.5)
    b = np.floor(u).astype(np.int64)
    f = (u - np.floor(u)).astype(np.float64)
    c = np.empty((2, 2, 2, q.shape[0]))
    for dz in range(2):
        for dy in range(2):
            for dx in range(2):
                c[dz, dy, dx] = field.lookup(b + np.array([dx, dy, dz]))[0]

    def tri(f):
        wx = np.stack([1 - f[:, 0], f[:, 0]])
        wy = np.stack([1 - f[:, 1], f[:, 1]])
        wz = np.stack([1 - f[:, 2], f[:, 2]])
        return np.einsum("zyxn,zn,yn,xn->n", c, wz, wy, wx)

    assert np.allclose(tri(f), s[v][:2000], atol=4e-6)
    h = 1e-4
    for a in range(3):
        e = np.zeros(3)
        e[a] = h
        d = (tri(f + e) - tri(f - e)) / (2 * h) / sr.VOXEL_SIZE
        assert np.allclose(d, g[v][:2000, a], atol=2e-4), a
    # a projective TSDF's gradient is at least about unit length (longer at grazing incidence)
    gn = np.linalg.norm(g[v].astype(np.float64), axis=1)
    assert np.median(gn) > 0.5 and not g[~v].any()


def test_reference_conditions_hold(field, queries):
    """The queries exercise every class: valid and invalid samples with 0, 1, 2 and 3 axes
    straddling a brick face, about half of them valid."""
    assert queries.shape == (16384, 3)
    _, _, _, v = sr.sample(field, queries, sr.TRILINEAR)
    share, table = sr.check_not_vacuous(field, queries, v)
    print("valid share %.3f, (valid, invalid) by straddling axes %s" % (share, table))
    # min_weight = 2 is a real gate on a single scan's field: fewer valid samples, not none
    _, w2, _, v2 = sr.sample(field, queries, sr.TRILINEAR, 2.0)
    assert 1000 < v2.sum() < v.sum() and np.all(w2[v2.astype(bool)] >= 2)
    assert not np.any(v2.astype(bool) & ~v.astype(bool))


def test_align_terms_are_the_sums_of_their_terms(field, scan0):
    pts = scan0[0][::8]
    H, b, e, nv, ab = sr.align_terms(field, pts, np.eye(4)[:3])
    assert nv > 4000 and np.allclose(H, H.T) and np.all(np.linalg.eigvalsh(H) > 0)
    assert ab.shape == (44,) and ab[43] == nv and np.all(ab[:36].reshape(6, 6) >= np.abs(H))
    assert np.all(ab[36:42] >= np.abs(b)) and ab[42] == e
    # at the true pose the residual is the map's own noise
    assert np.sqrt(e / nv) < 0.03


def test_gauss_newton_recovers_the_pose(field, scan0):
    """From |t| = 2.7 cm and 0.30 degrees off, six undamped steps on the reference's align terms
    bring the scan back onto the map it built."""
    pts = scan0[0][::8]
    T0 = sr.start_pose()
    t0, a0 = sr.pose_error(T0)
    assert abs(t0 - 0.0269) < 1e-3 and abs(a0 - 0.30) < 1e-2
    T, hist = sr.refine_pose(field, pts, T0, iters=6)
    for k, (rms, nv) in enumerate(hist):
        print("step %d: rms %.4f m, n_valid %d" % (k, rms, nv))
    t, a = sr.pose_error(T)
    print("after 6 steps: |t| = %.3f cm, angle = %.4f deg" % (100 * t, a))
    assert t < 0.01
    assert a < 0.1
    _, _, e, nv, _ = sr.align_terms(field, pts, T)
    assert np.sqrt(e / nv) < hist[0][0]
    assert hist[-1][0] < hist[0][0]
