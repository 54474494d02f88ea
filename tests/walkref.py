"""numpy restatement of the integrate walks (test helper): every ray of one scan walked sample by
sample, in the precisions and the op order oracle/tsdf_oracle.c states for each semantics, and the
scan's samples fused as the scan-fused mode does (exact fixed-point sums, one update per voxel).
The index domain is a plain mask on the samples (|i| < lim on every axis), so the restatement is a
reference for the domain clip that shares no code with the oracle or the kernels.

Scope: one scan into an empty map, origin-only (Voxblox point weight 1), no carving, no range
limits; every ray's index coordinates far below 2^30 (the far-ray rule is not restated here).

The three `_samples_*` walks return one (ijk, sdf, weight) part per DDA step; with rays=True every
part carries a fourth array, the index of each sample's ray in the cloud (tests/statsref.py counts
a ray's bricks from it).  The default return value is unchanged.
"""
import numpy as np

F = np.float32
D = np.float64
FLT_MAX = F(3.402823466e+38)
TWO32 = F(4294967296.0)


def _samples_vdbfusion(p, org, vs, tau, rays=False):
    """walk_ray: fp32 throughout.  rays: every part also carries its samples' ray indices."""
    o = np.asarray(org, D).astype(F)
    inv = F(1.0) / vs
    d = p - o
    depth = np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])
    act = depth > 0
    u = d / depth[:, None]
    t0i, t1i = (depth - tau) * inv, (depth + tau) * inv
    s = o * inv + u * t0i[:, None]
    v = np.floor(s).astype(np.int64)
    iu = F(1.0) / u
    tn = np.where(u > 0, t0i[:, None] + ((v + 1).astype(F) - s) * iu,
                  np.where(u < 0, t0i[:, None] + (v.astype(F) - s) * iu, F(np.inf))).astype(F)
    td = np.where(u != 0, np.abs(iu), F(np.inf)).astype(F)
    st = np.sign(u).astype(np.int64)
    out = []
    while act.any():
        c = (v.astype(F) + F(0.5)) * vs
        a, b = c - o, p - c
        dist = np.sqrt((b[:, 0] * b[:, 0] + b[:, 1] * b[:, 1]) + b[:, 2] * b[:, 2])
        proj = (a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1]) + a[:, 2] * b[:, 2]
        sdf = np.where(proj > 0, dist, -dist)
        keep = act & (proj != 0) & (sdf > -tau)
        out.append((v[keep].copy(), np.minimum(sdf, tau)[keep], np.ones(keep.sum(), F))
                   + ((np.nonzero(keep)[0],) if rays else ()))
        # math::MinIndex: ties resolve to the higher axis
        ax = np.where((tn[:, 0] < tn[:, 1]) & (tn[:, 0] < tn[:, 2]), 0,
                      np.where(tn[:, 1] < tn[:, 2], 1, 2))
        r = np.arange(p.shape[0])
        act = act & (tn[r, ax] <= t1i)
        tn[r, ax] += np.where(act, td[r, ax], F(0))
        v[r, ax] += np.where(act, st[r, ax], 0)
    return out


def _samples_vdbfusion_f64(p, org, vs, tau, rays=False):
    """walk_ray_vdb: double geometry, openvdb's float ray and DDA."""
    o = np.asarray(org, D)
    pd = p.astype(D)
    vsd = D(vs)
    inv_s = D(1.0) / vsd
    d = pd - o
    depth = np.sqrt(d[:, 0] * d[:, 0] + (d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2])).astype(F)
    act = depth > 0
    il = D(1.0) / np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])
    dird = d * il[:, None]
    eye = (o.astype(F).astype(D) * inv_s).astype(F)
    dj = (dird.astype(F).astype(D) * inv_s).astype(F)
    L = np.sqrt(((dj[:, 0] * dj[:, 0] + dj[:, 1] * dj[:, 1]) + dj[:, 2] * dj[:, 2]).astype(D)).astype(F)
    di = dj / L[:, None]
    iu = F(1.0) / di
    t0i, t1i = L * (depth - tau), L * (depth + tau)
    pos = eye + di * t0i[:, None]
    v = np.floor(pos).astype(np.int64)
    tn = np.where(di == 0, FLT_MAX,
                  np.where(iu > 0, t0i[:, None] + ((v + 1).astype(F) - pos) * iu,
                           t0i[:, None] + (v.astype(F) - pos) * iu)).astype(F)
    td = np.where(di == 0, FLT_MAX, np.abs(iu)).astype(F)
    st = np.where(di == 0, 0, np.where(iu > 0, 1, -1)).astype(np.int64)
    out = []
    r = np.arange(p.shape[0])
    while act.any():
        c = v.astype(D) * vsd + vsd / D(2.0)
        a, b = c - o, pd - c
        dist = np.sqrt(b[:, 0] * b[:, 0] + (b[:, 1] * b[:, 1] + b[:, 2] * b[:, 2]))
        proj = a[:, 0] * b[:, 0] + (a[:, 1] * b[:, 1] + a[:, 2] * b[:, 2])
        sdf = ((proj / np.abs(proj)) * dist).astype(F)  # NaN where proj == 0: fails the gate
        keep = act & (sdf > -tau)
        out.append((v[keep].copy(), np.where(tau < sdf, tau, sdf)[keep], np.ones(keep.sum(), F))
                   + ((np.nonzero(keep)[0],) if rays else ()))
        ax = np.where((tn[:, 0] < tn[:, 1]) & (tn[:, 0] < tn[:, 2]), 0,
                      np.where(tn[:, 1] < tn[:, 2], 1, 2))
        act = act & (tn[r, ax] <= t1i)
        v[r, ax] += np.where(act, st[r, ax], 0)
        tn[r, ax] += np.where(act, td[r, ax], F(0))
    return out


VB_MIN_WEIGHT = F(1.0 / 65536.0)


def _samples_voxblox(p, org, vs, tau, rays=False):
    """walk_ray_vb: fp32, Eigen's x + (y + z) reductions, point weight 1 with the dropoff."""
    o = np.asarray(org, D).astype(F)
    inv = F(1.0) / vs
    d = p - o
    depth = np.sqrt(d[:, 0] * d[:, 0] + (d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2]))
    act = depth > 0
    u = d / depth[:, None]
    ss, es = (p - u * tau) * inv, (p + u * tau) * inv
    v = np.floor(ss + F(1e-6)).astype(np.int64)
    e = np.floor(es + F(1e-6)).astype(np.int64)
    steps = np.abs(e - v).sum(1)
    rr = es - ss
    st = np.sign(rr).astype(np.int64)
    corr = np.where(st > 0, F(1.0), F(0.0))
    tn = np.where(st == 0, F(np.inf), (corr - (ss - v.astype(F))) / rr).astype(F)
    td = np.where(st == 0, F(np.inf), st.astype(F) / rr).astype(F)
    out = []
    r = np.arange(p.shape[0])
    k = 0
    while act.any():
        c = (v.astype(F) + F(0.5)) * vs
        a = c - o
        proj = (a[:, 0] * d[:, 0] + (a[:, 1] * d[:, 1] + a[:, 2] * d[:, 2])) / depth
        sdf = depth - proj
        w = np.where(sdf < -vs, np.maximum((F(1.0) * (tau + sdf)) / (tau - vs), F(0)), F(1.0)).astype(F)
        keep = act & (w >= VB_MIN_WEIGHT)
        out.append((v[keep].copy(), sdf[keep], w[keep]) + ((np.nonzero(keep)[0],) if rays else ()))
        act = act & (k < steps)
        k += 1
        # Eigen minCoeff: the first minimum wins
        ax = np.zeros(p.shape[0], np.int64)
        ax = np.where(tn[:, 1] < tn[r, ax], 1, ax)
        ax = np.where(tn[:, 2] < tn[r, ax], 2, ax)
        v[r, ax] += np.where(act, st[r, ax], 0)
        tn[r, ax] += np.where(act, td[r, ax], F(0))
    return out


_SAMPLES = {"vdbfusion": _samples_vdbfusion, "vdbfusion_f64": _samples_vdbfusion_f64,
            "voxblox": _samples_voxblox}


def integrate_one_scan(points, origin, semantics, voxel_size, sdf_trunc, lim=None,
                       max_weight=10000.0):
    """The field (ijk (n, 3) int64, sdf, weight), sorted (z, y, x), of one scan integrated into an
    empty map; samples of voxels outside |i| < lim are dropped (lim None: no domain)."""
    p = np.ascontiguousarray(points, F)
    vs, tau = F(voxel_size), F(sdf_trunc)
    with np.errstate(all="ignore"):
        parts = _SAMPLES[semantics](p, origin, vs, tau)
        ijk = np.concatenate([x[0] for x in parts])
        s = np.concatenate([x[1] for x in parts]).astype(F)
        w = np.concatenate([x[2] for x in parts]).astype(F)
        if lim is not None:
            m = np.all((ijk > -lim) & (ijk < lim), axis=1)
            ijk, s, w = ijk[m], s[m], w[m]
        # the scan's exact sums per voxel: trunc(s w 2^32), trunc(w 2^32) (a count for VDBFusion)
        vox, idx = np.unique(ijk[:, ::-1], axis=0, return_inverse=True)
        idx = idx.reshape(-1)
        A = np.zeros(vox.shape[0], np.int64)
        B = np.zeros(vox.shape[0], np.int64)
        if semantics == "voxblox":
            np.add.at(A, idx, ((s * w) * TWO32).astype(np.int64))
            np.add.at(B, idx, (w * TWO32).astype(np.int64))
            a = (A.astype(D) * (1.0 / 4294967296.0)).astype(F)
            b = (B.astype(D) * (1.0 / 4294967296.0)).astype(F)
            ns = (a + F(0) * F(0)) / b
            S = np.where(ns > 0, np.minimum(ns, tau), np.maximum(ns, -tau)).astype(F)
            W = np.minimum(b, F(max_weight)).astype(F)
            ok = ~(b < F(1e-6))
            vox, S, W = vox[ok], S[ok], W[ok]
        else:
            np.add.at(A, idx, (s * TWO32).astype(np.int64))
            np.add.at(B, idx, 1)
            a = (A.astype(D) * (1.0 / 4294967296.0)).astype(F)
            W = B.astype(F)
            S = ((F(0) * F(0) + a) / W).astype(F)
    return vox[:, ::-1].copy(), S, W
