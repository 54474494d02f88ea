"""numpy restatement of include/tsdf_hip_merge.h (test helper): one map merged into another under a
rigid transform, rules 1-5 on top of sampleref's Field, transform and sample.  Every fp32
expression is written in the order the header states, so the kernels (built with -ffp-contract=off)
reproduce it bit for bit.

The destination voxels are enumerated generously and without the library's candidate search: every
voxel within +-reach indices of the image of an observed source voxel's centre.  A valid sample
lies within half a voxel per axis of an observed voxel's centre (its own voxel, nearest; a corner
of its cube, trilinear), a rigid map keeps that distance (at most 0.87 voxels), so reach = 1 holds
every valid voxel while the fp32 rounding of rule 2 stays below 0.1 voxels (coordinates below
2^19 voxels); the tests at the edge of the index domain pass a larger reach.
"""
import collections

import numpy as np

import sampleref as sr

F = np.float32
LIM = 1 << 23
BRICK_MIN, BRICK_MAX = -(1 << 20), 1 << 20

Expected = collections.namedtuple("Expected", "coords sdf weight counts voxels")


def pose34(pose):
    T = np.asarray(pose, np.float64)
    if T.shape == (4, 4):
        T = T[:3]
    assert T.shape == (3, 4)
    return T


def inverse_pose(pose):
    """Rule 1: Ri = R^T, ti[r] = -((Ri[r][0] t0 + Ri[r][1] t1) + Ri[r][2] t2) in double, the twelve
    numbers rounded to fp32: m (3, 4) float32."""
    T = pose34(pose)
    Ri = T[:, :3].T.copy()
    t = T[:, 3]
    m = np.empty((3, 4), np.float64)
    m[:, :3] = Ri
    for r in range(3):
        m[r, 3] = -((Ri[r, 0] * t[0] + Ri[r, 1] * t[1]) + Ri[r, 2] * t[2])
    return m.astype(F)


def centres(v, vs):
    """Rule 2: c[a] = ((float)v[a] + 0.5f) * vs."""
    return ((np.asarray(v, np.int64).astype(F) + F(0.5)).astype(F) * F(vs)).astype(F)


def preimage(m, v, vs):
    """Rule 2: q of the destination voxels v (n, 3)."""
    return sr.transform(np.asarray(m, F).astype(np.float64), centres(v, vs))


def candidate_voxels(src_ijk, pose, vs, reach=1):
    """The generous candidate set: destination voxels (n, 3) int64, unique, inside |i| < 2^23."""
    T = pose34(pose)
    ijk = np.asarray(src_ijk, np.int64).reshape(-1, 3)
    if not ijk.shape[0]:
        return np.zeros((0, 3), np.int64)
    img = (ijk + 0.5) @ T[:, :3].T + T[:, 3] / float(F(vs))
    base = np.floor(img)
    base = base[np.all(np.abs(base) < 2.0 ** 40, axis=1)].astype(np.int64)
    base = _unique_rows(base)
    r = np.arange(-reach, reach + 1)
    off = np.stack(np.meshgrid(r, r, r, indexing="ij"), -1).reshape(-1, 3)
    # (unique bases first: neighbouring source voxels share most of their neighbourhoods)
    v = _unique_rows((base[:, None, :] + off[None, :, :]).reshape(-1, 3))
    return v[np.all((v > -LIM) & (v < LIM), axis=1)]


def _unique_rows(v):
    """np.unique(v, axis=0) of int64 rows (n, 3), through one int64 key per row where the rows'
    bounding box allows it (much faster), in lexicographic order."""
    if not v.shape[0]:
        return v
    lo = v.min(0)
    ext = [int(e) for e in (v.max(0) - lo + 1)]
    if ext[0] * ext[1] * ext[2] >= 1 << 62:
        return np.unique(v, axis=0)
    k = np.unique(((v[:, 0] - lo[0]) * ext[1] + (v[:, 1] - lo[1])) * ext[2] + (v[:, 2] - lo[2]))
    return np.stack([k // (ext[1] * ext[2]), (k // ext[2]) % ext[1], k % ext[2]], 1) + lo


def _brick_key(b):
    b = np.asarray(b, np.int64) + (1 << 20)
    return b[..., 0] | (b[..., 1] << 21) | (b[..., 2] << 42)


def _local(ijk):
    return ((ijk[..., 2] & 7) << 6) | ((ijk[..., 1] & 7) << 3) | (ijk[..., 0] & 7)


def merge(dst_bricks, src_voxels, pose, vs, bg, mode=sr.TRILINEAR, min_weight=0.0,
          max_weight=np.inf, reach=1):
    """dst_bricks: export_bricks() of the destination before the merge; src_voxels:
    export_voxels() of the source.  Returns Expected: the destination's export_bricks() after the
    merge (coords sorted (z, y, x), sdf and weight (nb, 8, 8, 8)), the four counts of the contract
    and the merged voxels (n, 3)."""
    dc, ds, dw = dst_bricks
    dc = np.asarray(dc, np.int64).reshape(-1, 3)
    S = np.asarray(ds, F).reshape(-1, 512).copy()
    W = np.asarray(dw, F).reshape(-1, 512).copy()
    field = sr.Field(src_voxels, vs, bg)
    m = inverse_pose(pose)
    v = candidate_voxels(src_voxels[0], pose, vs, reach)
    counts = dict(touched_bricks=0, new_bricks=0, merged_voxels=0, overlap_voxels=0)
    if v.shape[0]:
        q = preimage(m, v, vs)
        s, w, _, valid = sr.sample(field, q, mode, min_weight)
        ok = valid.astype(bool)
        v, s, w = v[ok], s[ok].astype(F), w[ok].astype(F)
    if v.shape[0]:
        assert np.all(w > 0)
        have = _brick_key(dc)
        order = np.argsort(have)
        bk = _brick_key(v >> 3)
        ub = np.unique(bk)
        new = ub[~np.isin(ub, have)]
        counts["touched_bricks"] = int(ub.size)
        counts["new_bricks"] = int(new.size)
        counts["merged_voxels"] = int(v.shape[0])
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
        with np.errstate(invalid="ignore", divide="ignore"):
            nw = (W0 + w).astype(F)
            fused = (((S0 * W0).astype(F) + (s * w).astype(F)).astype(F) / nw).astype(F)
        copy = W0 == 0
        S[row, loc] = np.where(copy, s, fused)
        W[row, loc] = np.where(copy, w, np.minimum(nw, F(max_weight)))
    order = np.argsort(_brick_key(dc))  # (z, y, x): the order of the keys as integers
    return Expected(dc[order].astype(np.int32), S[order].reshape(-1, 8, 8, 8),
                    W[order].reshape(-1, 8, 8, 8), counts, v)


def background(volume):
    return 0.0 if volume.semantics == "voxblox" else F(volume.sdf_trunc)


def weight_cap(volume):
    return F(volume.params.max_weight) if volume.semantics == "voxblox" else np.inf


def expected(dst, src, pose, mode="trilinear", min_weight=0.0, reach=1, src_voxels=None,
             dst_bricks=None):
    """`merge` for two volumes (read through export_bricks / export_voxels; pass cached exports
    to spare the read)."""
    return merge(dst.export_bricks() if dst_bricks is None else dst_bricks,
                 src.export_voxels() if src_voxels is None else src_voxels, pose, dst.voxel_size,
                 background(dst), sr.NEAREST if mode == "nearest" else sr.TRILINEAR, min_weight,
                 weight_cap(dst), reach)


def assert_same_bricks(got, exp):
    """export_bricks() against Expected (or another export), bitwise as uint32, the brick set
    included."""
    gc, gs, gw = got
    ec, es, ew = exp[:3]
    assert gc.shape == ec.shape, (gc.shape, ec.shape)
    assert np.array_equal(gc, ec)
    gw, ew = np.asarray(gw, F).reshape(-1, 512), np.asarray(ew, F).reshape(-1, 512)
    gs, es = np.asarray(gs, F).reshape(-1, 512), np.asarray(es, F).reshape(-1, 512)
    assert np.array_equal(gw.view(np.uint32), ew.view(np.uint32)), int((gw != ew).sum())
    assert np.array_equal(gs.view(np.uint32), es.view(np.uint32)), \
        int((gs.view(np.uint32) != es.view(np.uint32)).sum())
    return gc.shape[0]


def contract_counts(stats):
    return {k: int(stats[k]) for k in ("touched_bricks", "new_bricks", "merged_voxels",
                                       "overlap_voxels")}


def rigid(rotvec_deg=(0.0, 0.0, 0.0), t=(0.0, 0.0, 0.0)):
    T = np.empty((3, 4))
    T[:, :3] = sr.exp_so3(np.deg2rad(np.asarray(rotvec_deg, np.float64)))
    T[:, 3] = t
    return T


def rot_z90(t=(0.0, 0.0, 0.0)):
    """An exact quarter turn about z (entries 0 and +-1, no rounding)."""
    T = np.zeros((3, 4))
    T[0, 1], T[1, 0], T[2, 2] = -1.0, 1.0, 1.0
    T[:, 3] = t
    return T


def invert(pose):
    T = pose34(pose)
    out = np.empty((3, 4))
    out[:, :3] = T[:, :3].T
    out[:, 3] = -T[:, :3].T @ T[:, 3]
    return out
