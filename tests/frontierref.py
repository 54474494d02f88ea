"""Reference restatements of include/tsdf_hip_frontier.h in numpy, three of them:

  dense(S, W, lo, hi, ...)      vectorised, over the (S, W) of the box grown by one voxel
                                (query_dense(lo - 1, hi + 1): [z, y, x] arrays)
  sparse(coords, S, W, ...)     over export_bricks: 10^3 class tiles gathered from 27 neighbours,
                                in chunks; the only one that covers a whole map
  scalar(S, W, lo, hi, ...)     a triple loop over the same dense arrays, for tiny cases

Each returns a `Ref`: coords (N, 3) int32, n_unknown (N,) uint8, dir (N, 3) int8 in the header's
order (bricks in (z, y, x) order, then the in-brick voxel l = z*64 + y*8 + x) and the counts it can
know (a dense field does not say which bricks are held: n_bricks is None there)."""
import numpy as np

F = np.float32
UNKNOWN, FREE, OTHER = 0, 1, 2
VOX_MIN = -(1 << 23)  # a voxel outside |i| < 2^23 reads (background, 0)

# the 26 offsets (dx, dy, dz): faces, then edges, then corners, so a connectivity is a prefix
OFFSETS = sorted(((dx, dy, dz) for dz in (-1, 0, 1) for dy in (-1, 0, 1) for dx in (-1, 0, 1)
                  if (dx, dy, dz) != (0, 0, 0)),
                 key=lambda o: (abs(o[0]) + abs(o[1]) + abs(o[2]), o[2], o[1], o[0]))
N_OFFSETS = {6: 6, 18: 18, 26: 26}


class Ref:
    def __init__(self, coords, n_unknown, dirs, n_free, n_bricks=None):
        self.coords = np.asarray(coords, np.int32).reshape(-1, 3)
        self.n_unknown = np.asarray(n_unknown, np.uint8).reshape(-1)
        self.dir = np.asarray(dirs, np.int8).reshape(-1, 3)
        b = self.coords >> 3
        self.counts = {"n_bricks": n_bricks,
                       "n_frontier_bricks": len({tuple(r) for r in b.tolist()}),
                       "n_voxels": int(self.coords.shape[0]), "n_free": int(n_free)}


def classes(S, W, free_band, min_weight):
    """The header's classes in fp32: 0 unknown, 1 free, 2 other."""
    S, W = np.asarray(S, F), np.asarray(W, F)
    obs = (W > F(0)) & (W >= F(min_weight))
    return np.where(~obs, UNKNOWN, np.where(S >= F(free_band), FREE, OTHER)).astype(np.uint8)


def order_of(coords):
    """The permutation that puts voxel indices into the header's order."""
    c = np.asarray(coords, np.int64).reshape(-1, 3)
    b, l = c >> 3, c & 7
    return np.lexsort((l[:, 0], l[:, 1], l[:, 2], b[:, 0], b[:, 1], b[:, 2]))


def _box(lo, hi):
    return np.asarray(lo, np.int64).reshape(3), np.asarray(hi, np.int64).reshape(3)


def dense(S, W, lo, hi, free_band, min_weight=0.0, connectivity=6, min_unknown=1):
    """S, W: [z, y, x] arrays of voxels lo - 1 .. hi (the box grown by one voxel per side)."""
    lo, hi = _box(lo, hi)
    n = hi - lo
    if np.any(n <= 0):
        return Ref(np.zeros((0, 3)), [], np.zeros((0, 3)), 0)
    cls = classes(S, W, free_band, min_weight)
    assert cls.shape == (n[2] + 2, n[1] + 2, n[0] + 2)
    core = cls[1:-1, 1:-1, 1:-1]
    nu = np.zeros(core.shape, np.int32)
    d = np.zeros(core.shape + (3,), np.int32)
    for dx, dy, dz in OFFSETS[:N_OFFSETS[connectivity]]:
        u = cls[1 + dz:1 + dz + n[2], 1 + dy:1 + dy + n[1], 1 + dx:1 + dx + n[0]] == UNKNOWN
        nu += u
        d[..., 0] += dx * u
        d[..., 1] += dy * u
        d[..., 2] += dz * u
    free = core == FREE
    z, y, x = np.nonzero(free & (nu >= min_unknown))
    coords = np.stack([x + lo[0], y + lo[1], z + lo[2]], axis=1)
    o = order_of(coords)
    return Ref(coords[o], nu[z, y, x][o], d[z, y, x][o], int(free.sum()))


def scalar(S, W, lo, hi, free_band, min_weight=0.0, connectivity=6, min_unknown=1):
    """The same rule voxel by voxel (tiny boxes only)."""
    lo, hi = _box(lo, hi)
    S, W = np.asarray(S, F), np.asarray(W, F)
    fb, mw = F(free_band), F(min_weight)

    def cls(x, y, z):
        s, w = S[z - lo[2] + 1, y - lo[1] + 1, x - lo[0] + 1], W[z - lo[2] + 1, y - lo[1] + 1,
                                                                 x - lo[0] + 1]
        if not (w > F(0) and w >= mw):
            return UNKNOWN
        return FREE if s >= fb else OTHER

    rows, n_free = [], 0
    for z in range(int(lo[2]), int(hi[2])):
        for y in range(int(lo[1]), int(hi[1])):
            for x in range(int(lo[0]), int(hi[0])):
                if cls(x, y, z) != FREE:
                    continue
                n_free += 1
                nu, d = 0, [0, 0, 0]
                for dx, dy, dz in OFFSETS[:N_OFFSETS[connectivity]]:
                    if cls(x + dx, y + dy, z + dz) == UNKNOWN:
                        nu += 1
                        d = [d[0] + dx, d[1] + dy, d[2] + dz]
                if nu >= min_unknown:
                    rows.append(((z >> 3, y >> 3, x >> 3, z & 7, y & 7, x & 7), (x, y, z), nu, d))
    rows.sort(key=lambda r: r[0])
    return Ref([r[1] for r in rows], [r[2] for r in rows], [r[3] for r in rows], n_free)


def sparse(coords, S, W, free_band, min_weight=0.0, connectivity=6, min_unknown=1, lo=None,
           hi=None, chunk=512):
    """coords (nb, 3) brick coordinates, S / W (nb, 8, 8, 8) [z, y, x] (export_bricks); lo / hi: the
    voxel box, None for the whole map."""
    coords = np.asarray(coords, np.int64).reshape(-1, 3)
    nb = coords.shape[0]
    if lo is None:
        lo, hi = np.full(3, -(1 << 24), np.int64), np.full(3, 1 << 24, np.int64)
    lo, hi = _box(lo, hi)
    cls = classes(np.asarray(S).reshape(nb, 8, 8, 8), np.asarray(W).reshape(nb, 8, 8, 8),
                  free_band, min_weight)
    ar = np.arange(8)
    for a, ax in ((0, 3), (1, 2), (2, 1)):  # voxels outside |i| < 2^23 read (background, 0)
        edge = np.flatnonzero(coords[:, a] * 8 == VOX_MIN)
        idx = [slice(None)] * 4
        idx[0], idx[ax] = edge, 0
        if edge.size:
            cls[tuple(idx)] = UNKNOWN
    v0 = coords * 8
    held = np.all((v0 + 8 > lo) & (v0 < hi), axis=1)
    if np.any(hi <= lo):
        held[:] = False
    index = {tuple(c): i for i, c in enumerate(coords.tolist())}
    listed = np.flatnonzero(held)
    listed = listed[np.lexsort((coords[listed, 0], coords[listed, 1], coords[listed, 2]))]
    out_c, out_n, out_d, n_free = [], [], [], 0
    span = {-1: (slice(0, 1), slice(7, 8)), 0: (slice(1, 9), slice(0, 8)),
            1: (slice(9, 10), slice(0, 1))}
    for c0 in range(0, listed.size, chunk):
        ids = listed[c0:c0 + chunk]
        tile = np.zeros((ids.size, 10, 10, 10), np.uint8)  # an absent brick is unknown
        for dz in (-1, 0, 1):
            for dy in (-1, 0, 1):
                for dx in (-1, 0, 1):
                    nbr = np.array([index.get((c[0] + dx, c[1] + dy, c[2] + dz), -1)
                                    for c in coords[ids].tolist()])
                    have = np.flatnonzero(nbr >= 0)
                    if not have.size:
                        continue
                    (tz, sz), (ty, sy), (tx, sx) = span[dz], span[dy], span[dx]
                    tile[have, tz, ty, tx] = cls[nbr[have], sz, sy, sx]
        core = tile[:, 1:9, 1:9, 1:9]
        nu = np.zeros(core.shape, np.int32)
        d = np.zeros(core.shape + (3,), np.int32)
        for dx, dy, dz in OFFSETS[:N_OFFSETS[connectivity]]:
            u = tile[:, 1 + dz:9 + dz, 1 + dy:9 + dy, 1 + dx:9 + dx] == UNKNOWN
            nu += u
            d[..., 0] += dx * u
            d[..., 1] += dy * u
            d[..., 2] += dz * u
        b = coords[ids]
        gx = b[:, 0, None, None, None] * 8 + ar[None, None, None, :]
        gy = b[:, 1, None, None, None] * 8 + ar[None, None, :, None]
        gz = b[:, 2, None, None, None] * 8 + ar[None, :, None, None]
        inbox = ((gx >= lo[0]) & (gx < hi[0]) & (gy >= lo[1]) & (gy < hi[1]) & (gz >= lo[2]) &
                 (gz < hi[2]))
        free = (core == FREE) & inbox
        n_free += int(free.sum())
        k, z, y, x = np.nonzero(free & (nu >= min_unknown))  # (brick, z, y, x): the header's order
        out_c.append(np.stack([b[k, 0] * 8 + x, b[k, 1] * 8 + y, b[k, 2] * 8 + z], axis=1))
        out_n.append(nu[k, z, y, x])
        out_d.append(d[k, z, y, x])
    if not out_c:
        return Ref(np.zeros((0, 3)), [], np.zeros((0, 3)), 0, n_bricks=0)
    return Ref(np.concatenate(out_c), np.concatenate(out_n), np.concatenate(out_d), n_free,
               n_bricks=int(listed.size))


def of_volume(v, lo, hi, free_band, min_weight=0.0, connectivity=6, min_unknown=1):
    """The dense reference over the volume's own query_dense of the box grown by one voxel."""
    lo, hi = _box(lo, hi)
    if np.any(hi <= lo):
        return Ref(np.zeros((0, 3)), [], np.zeros((0, 3)), 0)
    S, W = v.query_dense(lo - 1, hi + 1)
    return dense(S, W, lo, hi, free_band, min_weight, connectivity, min_unknown)


def of_bricks(v, free_band, min_weight=0.0, connectivity=6, min_unknown=1, lo=None, hi=None):
    """The sparse reference over the volume's own export_bricks."""
    return sparse(*v.export_bricks(), free_band, min_weight, connectivity, min_unknown, lo, hi)


def assert_same(got, ref, counts=None):
    """got: (coords, n_unknown or None, dir or None); every output as integers, then the counts
    the reference knows."""
    coords, nu, d = got
    coords = np.asarray(coords)
    assert coords.dtype == np.int32 and coords.shape == ref.coords.shape, (coords.shape,
                                                                            ref.coords.shape)
    assert np.array_equal(coords, ref.coords)
    if nu is not None:
        nu = np.asarray(nu)
        assert nu.dtype == np.uint8 and np.array_equal(nu, ref.n_unknown)
    if d is not None:
        d = np.asarray(d)
        assert d.dtype == np.int8 and np.array_equal(d, ref.dir)
    if counts is not None:
        for k, want in ref.counts.items():
            if want is not None:
                assert int(counts[k]) == want, (k, counts, ref.counts)


def block_field(lo, n, blocks, S_free=1.0, margin=2):
    """(S, W, lo - margin, hi + margin): a dense field of voxels lo - margin .. lo + n + margin - 1,
    unknown but for the free 8^3 (or given size) blocks [(corner, size), ...]."""
    lo = np.asarray(lo, np.int64)
    n = np.asarray(n, np.int64)
    flo, fhi = lo - margin, lo + n + margin
    shape = tuple(int(e) for e in (fhi - flo)[::-1])
    S, W = np.zeros(shape, F), np.zeros(shape, F)
    for corner, size in blocks:
        c = np.asarray(corner, np.int64) - flo
        S[c[2]:c[2] + size, c[1]:c[1] + size, c[0]:c[0] + size] = S_free
        W[c[2]:c[2] + size, c[1]:c[1] + size, c[0]:c[0] + size] = 1.0
    return S, W, flo, fhi


def bricks_of(S, W, lo):
    """The 8-aligned dense field (S, W) at voxel lo as import_bricks' (coords, S, W); bricks
    without an observed voxel are left out."""
    lo = np.asarray(lo, np.int64)
    nz, ny, nx = (e // 8 for e in S.shape)
    assert np.all(lo % 8 == 0) and S.shape == (8 * nz, 8 * ny, 8 * nx)
    coords, bs, bw = [], [], []
    for z in range(nz):
        for y in range(ny):
            for x in range(nx):
                w = W[8 * z:8 * z + 8, 8 * y:8 * y + 8, 8 * x:8 * x + 8]
                if not np.any(w > 0):
                    continue
                coords.append([lo[0] // 8 + x, lo[1] // 8 + y, lo[2] // 8 + z])
                bs.append(S[8 * z:8 * z + 8, 8 * y:8 * y + 8, 8 * x:8 * x + 8])
                bw.append(w)
    return (np.asarray(coords, np.int32).reshape(-1, 3), np.asarray(bs, F).reshape(-1, 8, 8, 8),
            np.asarray(bw, F).reshape(-1, 8, 8, 8))
