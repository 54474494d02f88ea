"""A plain numpy restatement of the indexed mesh (include/tsdf_hip_mesh.h): vertices, normals and
triangles in the contract's order, from a dense (S, W) box.  fp32 throughout, one rounding per
operation in the header's order, so the GPU's output can be compared bit for bit.

The dense box must hold the field two voxels around every cube of interest (the gradients read one
voxel past a cube's corners); voxels outside it count as unobserved.
"""
import numpy as np

F = np.float32
# edge -> corners (a, b), b = a | axis bit, axis-major (tsdf_capi.cpp build_mc_table)
EDGES = [(b, b | (1 << d)) for d in range(3) for b in range(8) if not b & (1 << d)]


def mc_table(lib, which):
    """Case table `which` (TSDF_MC_*) of a library exporting tsdf_mc_table_of."""
    import ctypes as C
    buf = (C.c_uint8 * (256 * 32))()
    assert lib.tsdf_mc_table_of(which, buf) == 0
    return np.frombuffer(buf, np.uint8).reshape(256, 32).copy()


def dense_from_bricks(coords, sdf, weight, margin=2):
    """(S, W, origin): [z, y, x] float32 arrays over the bricks' bounding box grown by `margin`
    voxels, unlisted voxels (0, 0); origin = the voxel index (x, y, z) of element [0, 0, 0]."""
    coords = np.asarray(coords, np.int64).reshape(-1, 3)
    origin = coords.min(0) * 8 - margin
    dims = (coords.max(0) + 1) * 8 + margin - origin
    S = np.zeros(dims[::-1], F)
    W = np.zeros(dims[::-1], F)
    for c, s, w in zip(coords, np.asarray(sdf, F).reshape(-1, 8, 8, 8),
                       np.asarray(weight, F).reshape(-1, 8, 8, 8)):
        o = c * 8 - origin
        S[o[2]:o[2] + 8, o[1]:o[1] + 8, o[0]:o[0] + 8] = s
        W[o[2]:o[2] + 8, o[1]:o[1] + 8, o[0]:o[0] + 8] = w
    return S, W, origin


def _voxel_keys(v):
    """lexsort keys (least significant first) of voxels v (n, 3) (x, y, z) in the contract's
    order: brick (z, y, x), then in-brick (z, y, x)."""
    b, l = v >> 3, v & 7
    return (l[:, 0], l[:, 1], l[:, 2], b[:, 0], b[:, 1], b[:, 2])


def _order(v):
    return np.lexsort(_voxel_keys(v))


def _grad(S, ok, i, j, inv):
    """g_j at the array positions i (n, 3) (x, y, z): rule 3 of the header."""
    d = np.zeros(3, np.int64)
    d[j] = 1
    at = lambda q: (q[:, 2], q[:, 1], q[:, 0])  # noqa: E731
    p, m = i + d, i - d
    op, om = ok[at(p)], ok[at(m)]
    sv, sp, sm = S[at(i)], S[at(p)], S[at(m)]
    central = (sp - sm) * (F(0.5) * inv)
    fwd = (sp - sv) * inv
    bwd = (sv - sm) * inv
    return np.where(op & om, central, np.where(op, fwd, np.where(om, bwd, F(0)))).astype(F)


def indexed_mesh_ref(S, W, origin, voxel_size, tab, min_weight=0.0, lo=None, hi=None, info=None):
    """(vertices (V, 3) float32, normals (V, 3) float32, triangles (T, 3) uint32) of the dense
    field S, W ([z, y, x]; element [0, 0, 0] is voxel `origin` (x, y, z)), case table `tab`
    (256, 32).  lo / hi: the voxel box [lo, hi) of the cubes' min voxels.  info: a dict that takes
    "edges" ((V, 4): each vertex's min voxel and axis) and "cubes_per_vertex" ((V,): the meshed
    cubes whose triangles reference the vertex, 1 to 4)."""
    vs = F(voxel_size)
    inv = F(1.0) / vs
    pad = 2
    S = np.pad(np.asarray(S, F), pad)
    Wp = np.pad(np.asarray(W, F), pad)
    ok = (Wp > 0) & (Wp >= F(min_weight))
    org = np.asarray(origin, np.int64) - pad
    nz, ny, nx = S.shape
    cube_ok = np.ones((nz - 1, ny - 1, nx - 1), bool)
    case = np.zeros(cube_ok.shape, np.int64)
    for q in range(8):
        dx, dy, dz = q & 1, (q >> 1) & 1, q >> 2
        sl = (slice(dz, nz - 1 + dz), slice(dy, ny - 1 + dy), slice(dx, nx - 1 + dx))
        cube_ok &= ok[sl]
        case |= (S[sl] < 0).astype(np.int64) << q
    ntri = np.where(cube_ok, tab[case, 0], 0)
    iz, iy, ix = np.nonzero(ntri)
    cube = np.stack([ix, iy, iz], 1) + org  # min voxels (x, y, z), global
    if lo is not None:
        keep = np.all((cube >= np.asarray(lo, np.int64)) & (cube < np.asarray(hi, np.int64)), 1)
        cube = cube[keep]
    cube = cube[_order(cube)]
    # triangles as edge references (min voxel a, axis), cube by cube in table order
    refs, ref_cube = [], []
    for n_c, c in enumerate(cube):
        i = c - org
        k = int(case[i[2], i[1], i[0]])
        for e in tab[k, 1:1 + 3 * int(tab[k, 0])]:
            a, b = EDGES[e]
            ax = {1: 0, 2: 1, 4: 2}[a ^ b]
            refs.append((c[0] + (a & 1), c[1] + ((a >> 1) & 1), c[2] + (a >> 2), ax))
            ref_cube.append(n_c)
    refs = np.asarray(refs, np.int64).reshape(-1, 4)
    # one vertex per referenced edge, ordered by (brick, in-brick voxel, axis)
    edges = np.unique(refs, axis=0)
    edges = edges[np.lexsort((edges[:, 3],) + _voxel_keys(edges[:, :3]))]
    index = {tuple(e): n for n, e in enumerate(edges.tolist())}
    flat = np.asarray([index[tuple(r)] for r in refs.tolist()], np.int64)
    tris = flat.astype(np.uint32).reshape(-1, 3)
    if info is not None:
        pairs = np.unique(np.stack([flat, np.asarray(ref_cube, np.int64)], 1).reshape(-1, 2), axis=0)
        info["edges"] = edges
        info["cubes_per_vertex"] = np.bincount(pairs[:, 0], minlength=len(edges))
    A, K = edges[:, :3], edges[:, 3]
    ia = A - org
    ib = ia.copy()
    ib[np.arange(len(K)), K] += 1
    sa = S[ia[:, 2], ia[:, 1], ia[:, 0]]
    sb = S[ib[:, 2], ib[:, 1], ib[:, 0]]
    t = (sa / (sa - sb)).astype(F)
    pos = ((A.astype(F) + F(0.5)) * vs).astype(F)
    rows = np.arange(len(K))
    pos[rows, K] = pos[rows, K] + t * vs
    g = np.empty((len(K), 3), F)
    for j in range(3):
        ga, gb = _grad(S, ok, ia, j, inv), _grad(S, ok, ib, j, inv)
        g[:, j] = ga + t * (gb - ga)
    n2 = (g[:, 0] * g[:, 0] + g[:, 1] * g[:, 1]) + g[:, 2] * g[:, 2]
    nrm = np.zeros_like(g)
    nz_ = n2 > 0
    nrm[nz_] = g[nz_] / np.sqrt(n2[nz_])[:, None]
    return pos, nrm, tris


def holed(weight, share=0.1, seed=11):
    """`weight` with a seeded `share` of the voxels unobserved (W = 0)."""
    w = np.array(weight, F)
    w[np.random.default_rng(seed).random(w.shape) < share] = 0
    return w


def deindex(vertices, triangles):
    """The soup (3 T, 3) of an indexed mesh."""
    return vertices[triangles.reshape(-1).astype(np.int64)]
