"""The numpy restatement of include/tsdf_hip_columns.h: the seven rules of the header on the (S, W)
arrays that `query_dense` returns ([z, y, x] float32), every step in float32 in the header's order.
`column_map` is vectorised over the field, `column_map_scalar` is its per-column loop twin;
tests/test_columns_ref.py holds the two to each other and to known answers,
tests/test_columns_gpu.py holds the kernel to them bit for bit (floats as uint32)."""
import numpy as np

import esdfref as er
import sampleref as sr

F = np.float32
OBSERVED, OCCUPIED, FREE, HAS_ELEV, HAS_CEIL = 1, 2, 4, 8, 16
NAN = np.uint32(0x7FC00000).view(F)
NAMES = ("elev", "ceil", "n_occ", "n_free", "flags")


def classify(S, W, occ_band, min_weight):
    """(obs, occ, free) of rule 1, fp32 compares."""
    S, W = np.asarray(S, F), np.asarray(W, F)
    obs = (W > 0) & (W >= F(min_weight))
    with np.errstate(invalid="ignore"):
        occ = obs & (S <= F(occ_band))
    return obs, occ, obs & ~occ


def crossings(S, W, min_weight):
    """(up, down) of rule 3 as [z - 1, y, x] arrays: entry k is the pair (k, k + 1) of the field."""
    S, W = np.asarray(S, F), np.asarray(W, F)
    obs = (W > 0) & (W >= F(min_weight))
    both = obs[1:] & obs[:-1]
    with np.errstate(invalid="ignore"):
        up = both & (S[1:] > 0) & (S[:-1] <= 0)
        down = both & (S[:-1] > 0) & (S[1:] <= 0)
    return up, down


def column_map(S, W, z0, vs, occ_band=0.0, min_weight=0.0, min_occ=1, min_free=1):
    """(elev, ceil, n_occ, n_free, flags) as [y, x] arrays of the field S, W ([z, y, x]) whose first
    slice is voxel z0."""
    S, W = np.asarray(S, F), np.asarray(W, F)
    nz = S.shape[0]
    vs = F(vs)
    obs, occ, free = classify(S, W, occ_band, min_weight)
    n_occ = occ.sum(0).astype(np.uint16)
    n_free = free.sum(0).astype(np.uint16)
    elev = np.full(S.shape[1:], NAN, F)
    ceil = np.full(S.shape[1:], NAN, F)
    has_e = np.zeros(S.shape[1:], bool)
    has_c = np.zeros(S.shape[1:], bool)
    if nz > 1:
        up, down = crossings(S, W, min_weight)
        z = (np.int64(z0) + np.arange(1, nz, dtype=np.int64)).astype(F)[:, None, None]  # upper voxel
        zm = (np.int64(z0) + np.arange(0, nz - 1, dtype=np.int64)).astype(F)[:, None, None]
        Sz, Sp = S[1:], S[:-1]
        with np.errstate(all="ignore"):
            e_all = (((z + F(0.5)) - Sz / (Sz - Sp)) * vs).astype(F)
            c_all = (((zm + F(0.5)) + Sp / (Sp - Sz)) * vs).astype(F)
        has_e, has_c = up.any(0), down.any(0)
        top = (nz - 2) - np.argmax(up[::-1], axis=0)   # the up crossing of largest z
        low = np.argmax(down, axis=0)                  # the down crossing of smallest z
        elev = np.where(has_e, np.take_along_axis(e_all, top[None], 0)[0], NAN).astype(F)
        ceil = np.where(has_c, np.take_along_axis(c_all, low[None], 0)[0], NAN).astype(F)
    occupied = n_occ >= min_occ
    free_ = ~occupied & (n_free >= min_free)
    observed = (n_occ.astype(np.uint32) + n_free) > 0
    flags = (observed * OBSERVED | occupied * OCCUPIED | free_ * FREE | has_e * HAS_ELEV |
             has_c * HAS_CEIL).astype(np.uint8)
    return elev, ceil, n_occ, n_free, flags


def column_scalar(s, w, z0, vs, occ_band, min_weight, min_occ, min_free):
    """One column (s, w over z) by the header's rules, one voxel at a time, bottom to top."""
    vs, band, mw = F(vs), F(occ_band), F(min_weight)
    n_occ = n_free = 0
    elev = ceil = NAN
    has_e = has_c = False
    ps, pobs = F(0), False
    with np.errstate(all="ignore"):
        for k in range(len(s)):
            sz, wz, z = F(s[k]), F(w[k]), int(z0) + k
            obs = bool(wz > 0 and wz >= mw)
            occ = bool(obs and sz <= band)
            n_occ += occ
            n_free += obs and not occ
            if obs and pobs:
                if sz > 0 and ps <= 0:
                    t = F(sz / F(sz - ps))
                    elev = F(F(F(F(z) + F(0.5)) - t) * vs)
                    has_e = True
                if ps > 0 and sz <= 0 and not has_c:
                    t = F(ps / F(ps - sz))
                    ceil = F(F(F(F(z - 1) + F(0.5)) + t) * vs)
                    has_c = True
            ps, pobs = sz, obs
    occupied = n_occ >= min_occ
    free_ = (not occupied) and n_free >= min_free
    flags = ((n_occ + n_free > 0) * OBSERVED | occupied * OCCUPIED | free_ * FREE |
             has_e * HAS_ELEV | has_c * HAS_CEIL)
    return elev, ceil, n_occ, n_free, flags


def column_map_scalar(S, W, z0, vs, occ_band=0.0, min_weight=0.0, min_occ=1, min_free=1):
    """`column_map` as a loop over the columns."""
    S, W = np.asarray(S, F), np.asarray(W, F)
    ny, nx = S.shape[1:]
    out = (np.empty((ny, nx), F), np.empty((ny, nx), F), np.empty((ny, nx), np.uint16),
           np.empty((ny, nx), np.uint16), np.empty((ny, nx), np.uint8))
    for y in range(ny):
        for x in range(nx):
            r = column_scalar(S[:, y, x], W[:, y, x], z0, vs, occ_band, min_weight, min_occ,
                              min_free)
            for a, v in zip(out, r):
                a[y, x] = v
    return out


def of_volume(volume, lo, hi, occ_band=0.0, min_weight=0.0, min_occ=1, min_free=1):
    """The reference maps of a volume's box from its own query_dense."""
    S, W = volume.query_dense(lo, hi)
    return column_map(S, W, int(np.asarray(lo).reshape(3)[2]), volume.voxel_size, occ_band,
                      min_weight, min_occ, min_free)


def bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def assert_same(got, ref):
    """The five maps against the reference's, bit for bit; an entry of `got` may be None."""
    assert len(got) == len(ref) == 5
    for name, g, r in zip(NAMES, got, ref):
        if g is None:
            continue
        g = np.asarray(g)
        assert g.shape == r.shape and g.dtype == r.dtype, name
        same = np.array_equal(bits(g), bits(r)) if r.dtype == F else np.array_equal(g, r)
        assert same, "%s differs in %d cells" % (
            name, ((bits(g) != bits(r)) if r.dtype == F else (g != r)).sum())


def counts(S, W, min_weight, ref):
    """What a comparison on (S, W) can show: columns with elev, with ceil, with >= 2 up crossings,
    with >= 2 down crossings, with ceil < elev, free-only, unobserved."""
    if np.asarray(S).shape[0] > 1:
        up, down = crossings(S, W, min_weight)
    else:
        up = down = np.zeros((1,) + np.asarray(S).shape[1:], bool)
    elev, ceil, n_occ, n_free, flags = ref
    with np.errstate(invalid="ignore"):
        under = ceil < elev
    return dict(elev=int((flags & HAS_ELEV != 0).sum()), ceil=int((flags & HAS_CEIL != 0).sum()),
                up2=int((up.sum(0) >= 2).sum()), down2=int((down.sum(0) >= 2).sum()),
                shelf=int(under.sum()), free_only=int(((n_occ == 0) & (n_free > 0)).sum()),
                unobserved=int((flags & OBSERVED == 0).sum()), cells=int(flags.size))


def straddles(S, W, z0, min_weight):
    """(up, down): the columns whose chosen up / down crossing pair (z - 1, z) has z a multiple of
    8, so that the pair's voxels lie in two z-bricks."""
    up, down = crossings(S, W, min_weight)
    nz = np.asarray(S).shape[0]
    top = (nz - 2) - np.argmax(up[::-1], axis=0) + 1 + int(z0)   # z of the chosen pair's upper voxel
    low = np.argmax(down, axis=0) + 1 + int(z0)
    return int((up.any(0) & (top % 8 == 0)).sum()), int((down.any(0) & (low % 8 == 0)).sum())


# ---- the room -----------------------------------------------------------------------------------

VS = sr.VOXEL_SIZE
TAU = sr.SDF_TRUNC
ROOM_N = (45, 27, 52)
ROOM_SLAB = (10, 20)  # z-slices [a, b) above lo[2] between the room's floor and its shelf


def room(lo, n=ROOM_N, seed=7):
    """(S, W) [z, y, x] of a seeded room in the box lo..lo + n - 1, built relative to lo: a tilted
    floor, a tilted ceiling, a shelf slab over the middle third in x and the lower half in y, a
    one-voxel wall plane of constant negative S, weights 1..4, and W = 0 on about 8 % of the voxels
    and on those farther than TAU + 0.1 m from every surface.  Unobserved voxels read
    (TAU, 0), the background of a vdbfusion map."""
    nx, ny, nz = n
    rng = np.random.default_rng(seed)
    z, y, x = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    zc = z + 0.5
    floor = 6.3 + 0.05 * x + 0.03 * y                   # heights in voxels above lo[2]
    top = (nz - 6.6) - 0.04 * x + 0.02 * y
    s0, s1 = 0.43 * nz, 0.43 * nz + 4.3                 # the shelf slab
    d = np.minimum(zc - floor, top - zc)
    shelf = (x >= nx // 3) & (x < nx - nx // 3) & (y < ny // 2)
    d = np.where(shelf, np.minimum(d, np.maximum(s0 - zc, zc - s1)), d) * VS
    S = np.clip(d, -TAU, TAU).astype(F)
    W = rng.integers(1, 5, size=S.shape).astype(F)
    W[np.abs(d) > TAU + 0.1] = 0
    wall = x == nx - 5
    S[wall] = F(-0.1)
    W[wall] = rng.integers(1, 5, size=int(wall.sum())).astype(F)
    W[rng.random(S.shape) < 0.08] = 0
    S[W == 0] = F(TAU)
    return S, W


def bricks_of(S, W, lo, bg=TAU):
    """(coords, sdf, weight) for import_bricks of the field S, W at lo: the bricks that hold an
    observed voxel, other voxels of them (bg, 0)."""
    lo = np.asarray(lo, np.int64).reshape(3)
    nz, ny, nx = S.shape
    b0 = lo >> 3
    b1 = ((lo + np.array([nx, ny, nz]) - 1) >> 3) + 1
    nb = b1 - b0
    off = lo - b0 * 8
    Sp = np.full((nb[2] * 8, nb[1] * 8, nb[0] * 8), bg, F)
    Wp = np.zeros(Sp.shape, F)
    sl = (slice(off[2], off[2] + nz), slice(off[1], off[1] + ny), slice(off[0], off[0] + nx))
    Sp[sl], Wp[sl] = S, W

    def split(a):  # [bz, by, bx, 8, 8, 8]
        return a.reshape(nb[2], 8, nb[1], 8, nb[0], 8).transpose(0, 2, 4, 1, 3, 5)
    Sb, Wb = split(Sp), split(Wp)
    keep = (Wb > 0).any(axis=(3, 4, 5))
    bz, by, bx = np.nonzero(keep)
    coords = np.stack([bx + b0[0], by + b0[1], bz + b0[2]], 1).astype(np.int32)
    return coords, np.ascontiguousarray(Sb[keep]).reshape(-1, 512), \
        np.ascontiguousarray(Wb[keep]).reshape(-1, 512)


make_bricks = er.make_bricks
