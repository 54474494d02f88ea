"""The numpy restatement of include/tsdf_hip_esdf.h: the five rules of the header on the (S, W)
arrays that `query_dense` returns ([z, y, x] float32).  Squared distances are int64, the three
passes are shifted minima over d = 1..min(R, n - 1), then the cap, one float32 square root, the
product with the voxel size and the sign.  tests/test_esdf_ref.py holds it against a brute-force
minimum over all sites and against known answers; tests/test_esdf_gpu.py holds the kernels to it
bit for bit."""
import numpy as np

import sampleref as sr

F = np.float32
OBSERVED, SITE, CAPPED = 1, 2, 4
MAX_RADIUS = 128
INF = np.int64(1) << 40


def classify(S, W, site_band, min_weight):
    """(observed, site) of rule 1, fp32 compares."""
    S = np.asarray(S, F)
    W = np.asarray(W, F)
    observed = (W > 0) & (W >= F(min_weight))
    site = observed & (np.abs(S) <= F(site_band))
    return observed, site


def min_plus(g, axis, radius):
    """g'(i) = min over |d| <= radius inside the array of g(i + d) + d^2 along `axis`."""
    out = g.copy()
    n = g.shape[axis]

    def sl(a, b):
        s = [slice(None)] * g.ndim
        s[axis] = slice(a, b)
        return tuple(s)
    for d in range(1, min(radius, n - 1) + 1):
        np.minimum(out[sl(0, n - d)], g[sl(d, n)] + d * d, out=out[sl(0, n - d)])
        np.minimum(out[sl(d, n)], g[sl(0, n - d)] + d * d, out=out[sl(d, n)])
    return out


def squared(site, radius):
    """d2 of rule 3 before the cap: int64, >= INF where no site lies within `radius` per axis."""
    g = np.where(site, np.int64(0), INF)
    for axis in (2, 1, 0):  # x, y, z of a [z, y, x] array
        g = min_plus(g, axis, radius)
    return g


def finish(d2, S, observed, site, radius, voxel_size):
    """Rules 3 (the cap), 4 and 5 from the uncapped d2."""
    r2 = np.int64(radius) * radius
    capped = d2 > r2
    d2 = np.where(capped, r2, d2)
    dist = (np.sqrt(d2.astype(F)) * F(voxel_size)).astype(F)
    dist = np.where(observed & (np.asarray(S, F) < 0), -dist, dist).astype(F)
    flags = (observed.astype(np.uint8) * OBSERVED | site.astype(np.uint8) * SITE |
             capped.astype(np.uint8) * CAPPED).astype(np.uint8)
    return dist, flags


def esdf(S, W, voxel_size, radius, site_band, min_weight=0.0):
    """(dist float32, flags uint8), [z, y, x], of the box whose voxels read (S, W)."""
    assert 1 <= radius <= MAX_RADIUS
    observed, site = classify(S, W, site_band, min_weight)
    return finish(squared(site, radius), S, observed, site, radius, voxel_size)


def brute_squared(site, radius):
    """d2 of rule 3 before the cap as a plain minimum over all sites of the box (small boxes)."""
    zs, ys, xs = np.nonzero(site)
    u = np.stack([zs, ys, xs], 1).astype(np.int64)
    v = np.stack(np.meshgrid(*[np.arange(n) for n in site.shape], indexing="ij"), -1)
    v = v.reshape(-1, 1, 3).astype(np.int64)
    if u.shape[0] == 0:
        return np.full(site.shape, INF, np.int64)
    off = u[None] - v
    d2 = (off * off).sum(-1)
    d2 = np.where(np.abs(off).max(-1) <= radius, d2, INF)
    return d2.min(1).reshape(site.shape)


def of_volume(volume, lo, hi, radius, site_band=None, min_weight=0.0):
    """The reference field of a volume's box from its own query_dense."""
    S, W = volume.query_dense(lo, hi)
    band = volume.voxel_size if site_band is None else site_band
    return esdf(S, W, volume.voxel_size, radius, band, min_weight)


def bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def assert_same(got, ref):
    """(dist, flags) against the reference's, bit for bit (flags may be None on either side)."""
    assert got[0].shape == ref[0].shape
    assert np.array_equal(bits(got[0]), bits(ref[0]))
    if got[1] is not None and ref[1] is not None:
        assert got[1].dtype == np.uint8 and np.array_equal(got[1], ref[1])


# ---- the shared fixture box ---------------------------------------------------------------------

def fixture_centre(scan0):
    """The voxel of the jittered query nearest (in the L1 norm) to the queries' per-axis median: a
    voxel in the thick of the scan, with negative y and z."""
    q = np.asarray(sr.jitter_queries(*scan0), np.float64)
    k = np.argmin(np.abs(q - np.median(q, axis=0)).sum(1))
    return np.floor(q[k] / sr.VOXEL_SIZE).astype(np.int64)


def fixture_box(c):
    """The 97 x 80 x 33 box around c."""
    c = np.asarray(c, np.int64)
    return c - np.array([48, 40, 16]), c + np.array([49, 40, 17])


def smallest_abs_voxel(volume):
    """The observed voxel of smallest |S| (the first in (z, y, x) order among equals)."""
    ijk, s, _ = volume.export_voxels()
    return np.asarray(ijk[np.argmin(np.abs(s))], np.int64)


def make_bricks(voxels, bg):
    """(coords, sdf, weight) for import_bricks from {(x, y, z): (S, W)}; other voxels (bg, 0)."""
    bricks = {}
    for (x, y, z), (s, w) in voxels.items():
        b = (x >> 3, y >> 3, z >> 3)
        if b not in bricks:
            bricks[b] = (np.full((8, 8, 8), bg, F), np.zeros((8, 8, 8), F))
        bricks[b][0][z & 7, y & 7, x & 7] = s
        bricks[b][1][z & 7, y & 7, x & 7] = w
    keys = sorted(bricks)
    return (np.array(keys, np.int32).reshape(-1, 3), np.stack([bricks[k][0] for k in keys]),
            np.stack([bricks[k][1] for k in keys]))
