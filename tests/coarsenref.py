"""A numpy restatement of include/tsdf_hip_coarsen.h, rules 1-7, on exported bricks: fp32, a loop
over the children k = a + 2 b + 4 c = 0..7 vectorised over the coarse voxels, every operation in
the stated order and rounded to fp32.  It returns what export_bricks() of the destination must be
after the call and the seven counts, and never sees the library's lists: the coarse voxels come
straight from the source's bricks (a coarse voxel's eight children lie in one source brick).
"""
import collections

import numpy as np

F = np.float32
COUNT_KEYS = ("src_bricks", "parent_bricks", "touched_bricks", "new_bricks", "coarse_voxels",
              "overlap_voxels", "child_voxels")

Expected = collections.namedtuple("Expected", "coords sdf weight counts voxels")


def _brick_key(b):
    b = np.asarray(b, np.int64) + (1 << 20)
    return b[..., 0] | (b[..., 1] << 21) | (b[..., 2] << 42)


def _local(ijk):
    return ((ijk[..., 2] & 7) << 6) | ((ijk[..., 1] & 7) << 3) | (ijk[..., 0] & 7)


def selected(coords, box=None, side="inside"):
    """Rule 1: the mask of the source bricks `coords` (n, 3) a call selects."""
    c = np.asarray(coords, np.int64).reshape(-1, 3)
    if box is None:
        return np.ones(c.shape[0], bool)
    lo, hi = (np.asarray(v, np.int64).reshape(3) for v in box)
    inside = np.all((c >= lo) & (c < hi), axis=1)
    return inside if side == "inside" else ~inside


def octets(sdf, weight, min_weight=0.0):
    """Rules 3 and 5 on bricks (n, 8, 8, 8) indexed [z, y, x]: per coarse voxel (n, 4, 4, 4) the
    number of valid children, and (s, w) where that number is not 0 (else NaN, 0)."""
    S = np.asarray(sdf, F).reshape(-1, 8, 8, 8)
    W = np.asarray(weight, F).reshape(-1, 8, 8, 8)
    mw = F(min_weight)
    sw = np.zeros((S.shape[0], 4, 4, 4), F)
    ssw = np.zeros_like(sw)
    n = np.zeros(sw.shape, np.int32)
    for k in range(8):
        a, b, c = k & 1, (k >> 1) & 1, k >> 2
        Sc, Wc = S[:, c::2, b::2, a::2], W[:, c::2, b::2, a::2]
        ok = (Wc > 0) & (Wc >= mw)
        prod = (Sc * Wc).astype(F)
        ssw = np.where(ok, (ssw + prod).astype(F), ssw)
        sw = np.where(ok, (sw + Wc).astype(F), sw)
        n += ok
    with np.errstate(invalid="ignore", divide="ignore"):
        s = (ssw / sw).astype(F)
        w = (sw / n.astype(F)).astype(F)
    return n, s, np.where(n > 0, w, F(0))


def child_histogram(src_bricks, min_weight=0.0):
    """The coarse voxels of a whole source by their number of valid children, n = 1..8."""
    n, _, _ = octets(src_bricks[1], src_bricks[2], min_weight)
    return np.bincount(n.reshape(-1), minlength=9)[1:].tolist()


def coarsen(dst_bricks, src_bricks, bg, min_children=1, min_weight=0.0, box=None, side="inside",
            max_weight=np.inf):
    """dst_bricks, src_bricks: export_bricks() of the destination before the call and of the
    source.  Returns Expected: the destination's export_bricks() after it (coords sorted
    (z, y, x), sdf and weight (nb, 8, 8, 8)), the seven counts, and the coarse voxels (n, 3)."""
    dc, ds, dw = dst_bricks
    dc = np.asarray(dc, np.int64).reshape(-1, 3)
    S = np.asarray(ds, F).reshape(-1, 512).copy()
    W = np.asarray(dw, F).reshape(-1, 512).copy()
    sc = np.asarray(src_bricks[0], np.int64).reshape(-1, 3)
    sel = selected(sc, box, side)
    sc = sc[sel]
    counts = dict.fromkeys(COUNT_KEYS, 0)
    counts["src_bricks"] = int(sc.shape[0])
    v = np.zeros((0, 3), np.int64)
    if sc.shape[0]:
        counts["parent_bricks"] = int(np.unique(_brick_key(sc >> 1)).size)  # rule 2: floor
        n, s, w = octets(np.asarray(src_bricks[1], F).reshape(-1, 8, 8, 8)[sel],
                         np.asarray(src_bricks[2], F).reshape(-1, 8, 8, 8)[sel], min_weight)
        b, z, y, x = np.nonzero(n >= int(min_children))  # rule 4
        # the coarse voxel of local (x, y, z) of source brick B: children 8 B + 2 (x, y, z) + (a, b, c)
        v = sc[b] * 4 + np.stack([x, y, z], 1)
        s, w, n = s[b, z, y, x], w[b, z, y, x], n[b, z, y, x]
    if v.shape[0]:
        assert np.all(w > 0)
        have = _brick_key(dc)
        bk = _brick_key(v >> 3)
        ub = np.unique(bk)
        new = ub[~np.isin(ub, have)]
        counts["touched_bricks"] = int(ub.size)
        counts["new_bricks"] = int(new.size)
        counts["coarse_voxels"] = int(v.shape[0])
        counts["child_voxels"] = int(n.sum())
        if new.size:
            nc = np.stack([(new & 0x1FFFFF), (new >> 21) & 0x1FFFFF, (new >> 42) & 0x1FFFFF], 1)
            dc = np.concatenate([dc, nc - (1 << 20)])
            S = np.concatenate([S, np.full((new.size, 512), F(bg), F)])
            W = np.concatenate([W, np.zeros((new.size, 512), F)])
            have = _brick_key(dc)
        order = np.argsort(have)
        row = order[np.searchsorted(have[order], bk)]
        loc = _local(v)
        S0, W0 = S[row, loc], W[row, loc]
        counts["overlap_voxels"] = int((W0 > 0).sum())
        with np.errstate(invalid="ignore", divide="ignore"):  # rule 6
            nw = (W0 + w).astype(F)
            fused = (((S0 * W0).astype(F) + (s * w).astype(F)).astype(F) / nw).astype(F)
        copy = W0 == 0
        S[row, loc] = np.where(copy, s, fused)
        W[row, loc] = np.where(copy, w, np.minimum(nw, F(max_weight)))
    order = np.argsort(_brick_key(dc))  # (z, y, x): the order of the keys as integers
    return Expected(dc[order].astype(np.int32), S[order].reshape(-1, 8, 8, 8),
                    W[order].reshape(-1, 8, 8, 8), counts, v)


def background(volume):
    return F(0.0) if volume.semantics == "voxblox" else F(volume.sdf_trunc)


def weight_cap(volume):
    return F(volume.params.max_weight) if volume.semantics == "voxblox" else np.inf


def expected(dst, src, min_children=1, min_weight=0.0, box=None, side="inside", dst_bricks=None,
             src_bricks=None):
    """`coarsen` for two volumes (read through export_bricks; pass cached exports to spare the
    read)."""
    return coarsen(dst.export_bricks() if dst_bricks is None else dst_bricks,
                   src.export_bricks() if src_bricks is None else src_bricks, background(dst),
                   min_children, min_weight, box, side, weight_cap(dst))


def bricks_of(voxels, sdf, weight, bg):
    """export_bricks()' format from voxels (n, 3) with their distances and weights."""
    v = np.asarray(voxels, np.int64).reshape(-1, 3)
    b, inv = np.unique(v >> 3, axis=0, return_inverse=True)
    inv = inv.reshape(-1)
    S = np.full((b.shape[0], 8, 8, 8), F(bg), F)
    W = np.zeros((b.shape[0], 8, 8, 8), F)
    S[inv, v[:, 2] & 7, v[:, 1] & 7, v[:, 0] & 7] = np.asarray(sdf, F)
    W[inv, v[:, 2] & 7, v[:, 1] & 7, v[:, 0] & 7] = np.asarray(weight, F)
    order = np.argsort(_brick_key(b))
    return b[order].astype(np.int32), S[order], W[order]


def empty_bricks():
    return (np.zeros((0, 3), np.int32), np.zeros((0, 8, 8, 8), F), np.zeros((0, 8, 8, 8), F))


def assert_same_bricks(got, exp):
    """export_bricks() against Expected (or another export), bitwise as uint32, the brick set
    included."""
    gc, gs, gw = got[:3]
    ec, es, ew = exp[:3]
    assert gc.shape == ec.shape, (gc.shape, ec.shape)
    assert np.array_equal(gc, ec)
    gw, ew = np.asarray(gw, F).reshape(-1, 512), np.asarray(ew, F).reshape(-1, 512)
    gs, es = np.asarray(gs, F).reshape(-1, 512), np.asarray(es, F).reshape(-1, 512)
    assert np.array_equal(gw.view(np.uint32), ew.view(np.uint32)), int((gw != ew).sum())
    assert np.array_equal(gs.view(np.uint32), es.view(np.uint32)), \
        int((gs.view(np.uint32) != es.view(np.uint32)).sum())
    return gc.shape[0]
