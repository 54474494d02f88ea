"""numpy restatement of the sparse map queries of include/tsdf_hip_sample.h (test helper): nearest
and trilinear TSDF samples with the analytic gradient, and the Gauss-Newton terms of the
point-to-TSDF error.  Every fp32 expression is written in the order the header states, so the
kernels (built with -ffp-contract=off) reproduce it bit for bit.

The field is what export_voxels() returns, which is bitwise-pinned between the GPU and the oracle:
the same reference runs on either.
"""
import numpy as np

F = np.float32
VOX_LIMIT = 1 << 23
NEAREST = 0
TRILINEAR = 1


class Field:
    """Voxel lookup over an exported field: (S, W) of integer voxels, (bg, 0) where the voxel is
    unobserved or outside the index domain |i| < 2^23."""

    def __init__(self, voxels, voxel_size, bg):
        ijk, s, w = voxels
        ijk = np.asarray(ijk, np.int64).reshape(-1, 3)
        self.vs = F(voxel_size)
        self.inv = F(1.0) / self.vs  # RayConst::inv_vs
        self.bg = F(bg)
        bk = self._brick_key(ijk >> 3)
        self.bricks = np.unique(bk)
        self.S = np.full((self.bricks.size + 1, 512), self.bg, F)  # last row: no such brick
        self.W = np.zeros((self.bricks.size + 1, 512), F)
        row = np.searchsorted(self.bricks, bk)
        loc = self._local(ijk)
        self.S[row, loc] = np.asarray(s, F)
        self.W[row, loc] = np.asarray(w, F)

    @staticmethod
    def _brick_key(b):
        b = b + (1 << 20)
        return b[..., 0] | (b[..., 1] << 21) | (b[..., 2] << 42)

    @staticmethod
    def _local(ijk):
        return ((ijk[..., 2] & 7) << 6) | ((ijk[..., 1] & 7) << 3) | (ijk[..., 0] & 7)

    def lookup(self, ijk):
        """ijk (..., 3) int64 -> (S, W) fp32 arrays of shape (...)."""
        ijk = np.asarray(ijk, np.int64)
        inside = np.all((ijk > -VOX_LIMIT) & (ijk < VOX_LIMIT), axis=-1)
        q = np.where(inside[..., None], ijk, 0)
        k = self._brick_key(q >> 3)
        row = np.searchsorted(self.bricks, k)
        row = np.minimum(row, self.bricks.size - 1) if self.bricks.size else np.zeros_like(row)
        hit = inside & (self.bricks[row] == k) if self.bricks.size else np.zeros_like(inside)
        row = np.where(hit, row, self.bricks.size)
        loc = self._local(q)
        return self.S[row, loc], self.W[row, loc]


def field_of(volume):
    """The reference's view of a TSDFVolume's field."""
    bg = 0.0 if volume.semantics == "voxblox" else F(volume.sdf_trunc)
    return Field(volume.export_voxels(), volume.voxel_size, bg)


def _lerp(a, b, t):
    return (a + t * (b - a)).astype(F)


def _floor_index(v):
    """floorf(v) as float and as int64 (0 where v is not finite or beyond the int64-safe range:
    such samples are rejected on the float value)."""
    fl = np.floor(v).astype(F)
    ok = np.isfinite(fl) & (np.abs(fl) < F(2.0 ** 40))
    return fl, np.where(ok, fl, 0).astype(np.int64)


def sample(field, points, mode=TRILINEAR, min_weight=0.0):
    """(sdf (n,), weight (n,), grad (n, 3), valid (n,) uint8) of fp32 world points."""
    p = np.asarray(points, F).reshape(-1, 3)
    n = p.shape[0]
    mw = F(min_weight)
    grad = np.zeros((n, 3), F)
    with np.errstate(invalid="ignore", over="ignore"):
        if mode == NEAREST:
            fl, idx = _floor_index((p * field.inv).astype(F))
            inside = np.all((fl > F(-VOX_LIMIT)) & (fl < F(VOX_LIMIT)), axis=1)
            s, w = field.lookup(np.where(inside[:, None], idx, VOX_LIMIT))
            valid = (w > 0) & (w >= mw)
            return s.astype(F), w.astype(F), grad, valid.astype(np.uint8)
        u = ((p * field.inv).astype(F) - F(0.5)).astype(F)
        bf, b = _floor_index(u)
        f = (u - bf).astype(F)
        # every corner inside |i| < 2^23, decided on the float: -(2^23 - 1) <= b <= 2^23 - 2
        inside = np.all((bf >= F(-(VOX_LIMIT - 1))) & (bf <= F(VOX_LIMIT - 2)), axis=1)
        inside &= np.all(np.isfinite(p), axis=1)
    b = np.where(inside[:, None], b, 0)
    cs = np.empty((2, 2, 2, n), F)  # [dz][dy][dx]
    cw = np.empty((2, 2, 2, n), F)
    for dz in range(2):
        for dy in range(2):
            for dx in range(2):
                cs[dz, dy, dx], cw[dz, dy, dx] = field.lookup(b + np.array([dx, dy, dz]))
    wmin = cw.reshape(8, n).min(0)
    valid = inside & np.all((cw.reshape(8, n) > 0) & (cw.reshape(8, n) >= mw), axis=0)
    fx, fy, fz = f[:, 0], f[:, 1], f[:, 2]
    with np.errstate(invalid="ignore", over="ignore"):
        # S: x, then y, then z
        c00 = _lerp(cs[0, 0, 0], cs[0, 0, 1], fx)
        c10 = _lerp(cs[0, 1, 0], cs[0, 1, 1], fx)
        c01 = _lerp(cs[1, 0, 0], cs[1, 0, 1], fx)
        c11 = _lerp(cs[1, 1, 0], cs[1, 1, 1], fx)
        s = _lerp(_lerp(c00, c10, fy), _lerp(c01, c11, fy), fz)
        # d/dx: the x differences over (y, z)
        gx = _lerp(_lerp(cs[0, 0, 1] - cs[0, 0, 0], cs[0, 1, 1] - cs[0, 1, 0], fy),
                   _lerp(cs[1, 0, 1] - cs[1, 0, 0], cs[1, 1, 1] - cs[1, 1, 0], fy), fz)
        # d/dy: the y differences over (x, z)
        gy = _lerp(_lerp(cs[0, 1, 0] - cs[0, 0, 0], cs[0, 1, 1] - cs[0, 0, 1], fx),
                   _lerp(cs[1, 1, 0] - cs[1, 0, 0], cs[1, 1, 1] - cs[1, 0, 1], fx), fz)
        # d/dz: the z differences over (x, y)
        gz = _lerp(_lerp(cs[1, 0, 0] - cs[0, 0, 0], cs[1, 0, 1] - cs[0, 0, 1], fx),
                   _lerp(cs[1, 1, 0] - cs[0, 1, 0], cs[1, 1, 1] - cs[0, 1, 1], fx), fy)
        g = np.stack([gx * field.inv, gy * field.inv, gz * field.inv], 1).astype(F)
    s = np.where(valid, s, field.bg).astype(F)
    w = np.where(valid, wmin, F(0)).astype(F)
    grad = np.where(valid[:, None], g, F(0)).astype(F)
    return s, w, grad, valid.astype(np.uint8)


def straddle_axes(field, points):
    """Per point, the number of axes on which the trilinear cube crosses a brick face
    (b & 7 == 7)."""
    p = np.asarray(points, F).reshape(-1, 3)
    with np.errstate(invalid="ignore", over="ignore"):
        _, b = _floor_index(((p * field.inv).astype(F) - F(0.5)).astype(F))
    return ((b & 7) == 7).sum(1)


def transform(pose, points):
    """q = ((r0 x + r1 y) + r2 z) + t per row, the 3x4 pose rounded to fp32."""
    m = np.asarray(pose, np.float64).reshape(3, 4).astype(F)
    p = np.asarray(points, F).reshape(-1, 3)
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    with np.errstate(invalid="ignore", over="ignore"):
        q = [(((m[r, 0] * x + m[r, 1] * y).astype(F) + m[r, 2] * z).astype(F) + m[r, 3]).astype(F)
             for r in range(3)]
    return np.stack(q, 1)


def align_terms(field, points, pose, min_weight=0.0):
    """(H (6, 6), b (6,), e, n_valid, abs_sums (44,)): the Gauss-Newton normal equations of the
    point-to-TSDF error under `pose`, summed in double; abs_sums holds sum |term| per output word
    (H row-major, b, e, n_valid), the scale of any summation-order difference."""
    q = transform(pose, points)
    s, _, g, valid = sample(field, q, TRILINEAR, min_weight)
    v = valid.astype(bool)
    q = q[v].astype(np.float64)
    g = g[v].astype(np.float64)
    r = s[v].astype(np.float64)
    J = np.empty((q.shape[0], 6))
    J[:, :3] = g
    J[:, 3] = q[:, 1] * g[:, 2] - q[:, 2] * g[:, 1]
    J[:, 4] = q[:, 2] * g[:, 0] - q[:, 0] * g[:, 2]
    J[:, 5] = q[:, 0] * g[:, 1] - q[:, 1] * g[:, 0]
    hterm = J[:, :, None] * J[:, None, :]
    bterm = J * r[:, None]
    eterm = r * r
    n_valid = int(v.sum())
    abs_sums = np.concatenate([np.abs(hterm).sum(0).reshape(36), np.abs(bterm).sum(0),
                               [eterm.sum(), float(n_valid)]])
    return hterm.sum(0), bterm.sum(0), float(eterm.sum()), n_valid, abs_sums


# ---- the shared test workload ---------------------------------------------------------------------
VOXEL_SIZE = 0.1   # one full scan at 10 cm leaves enough fully observed cubes (5 cm: almost none)
SDF_TRUNC = 0.3
T0 = (0.02, -0.015, 0.01)       # the Gauss-Newton check's start: |t| = 2.7 cm ...
ROTVEC0_DEG = (0.2, -0.1, 0.2)  # ... and 0.30 degrees


def jitter_queries(points, origin):
    """The comparison tests' queries: every 8th point of the scan with range > 0.5 m, moved by a
    uniform +-5 cm per axis (default_rng(7)), so they fall on both sides of the surface, in
    observed and unobserved cubes."""
    q = np.asarray(points, F)[::8]
    rng_m = np.linalg.norm(q.astype(np.float64) - np.asarray(origin, np.float64), axis=1)
    q = q[rng_m > 0.5]
    jit = np.random.default_rng(7).uniform(-0.05, 0.05, q.shape)
    return np.ascontiguousarray((q + jit).astype(F))


def check_not_vacuous(field, queries, valid, lo=0.30, hi=0.60):
    """The conditions every comparison asserts on the reference: a valid share inside [lo, hi],
    and a valid and an invalid query in each class of brick-straddling axes (0..3)."""
    valid = np.asarray(valid, bool)
    share = valid.mean()
    assert lo <= share <= hi, share
    k = straddle_axes(field, queries)
    table = [(int((valid & (k == a)).sum()), int((~valid & (k == a)).sum())) for a in range(4)]
    for a, (nv, ni) in enumerate(table):
        assert nv >= 1 and ni >= 1, (a, table)
    return share, table


def start_pose():
    T = np.empty((3, 4))
    T[:, :3] = exp_so3(np.deg2rad(ROTVEC0_DEG))
    T[:, 3] = T0
    return T


def pose_error(T):
    """(|t| in metres, rotation angle in degrees) of a 3x4 pose against the identity."""
    T = np.asarray(T, np.float64).reshape(3, 4)
    c = (np.trace(T[:, :3]) - 1.0) / 2.0
    return float(np.linalg.norm(T[:, 3])), float(np.degrees(np.arccos(np.clip(c, -1.0, 1.0))))


def exp_so3(w):
    """Rodrigues' formula, float64."""
    w = np.asarray(w, np.float64).reshape(3)
    th = float(np.linalg.norm(w))
    K = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])
    if th < 1e-12:
        return np.eye(3) + K
    return np.eye(3) + (np.sin(th) / th) * K + ((1 - np.cos(th)) / (th * th)) * (K @ K)


def refine_pose(field, points, pose0, iters=6, min_weight=0.0):
    """Undamped Gauss-Newton on the reference's align terms; the same update as
    tsdf_map.align.refine_pose.  Returns (pose (3, 4), [(rms, n_valid), ...])."""
    T = np.asarray(pose0, np.float64).reshape(3, 4).copy()
    hist = []
    for _ in range(iters):
        H, b, e, nv, _ = align_terms(field, points, T, min_weight)
        if nv < 6:
            raise ValueError("fewer than 6 valid points")
        hist.append((float(np.sqrt(e / nv)), nv))
        d = np.linalg.solve(H, -b)
        E = exp_so3(d[3:])
        T[:, :3] = E @ T[:, :3]
        T[:, 3] = E @ T[:, 3] + d[:3]
    return T, hist
