"""The border-brick reduce and the mesh halo restated in plain numpy (include/tsdf_hip.h, "Border-
brick reduce" and "marching cubes of a sector-sharded field"), and builders of the
inputs that force its edges (test helper).  Nothing here calls a library.

Everything works on exports: per rank (coords int32 (n, 3), sdf f32 (n, 512), weight f32 (n, 512))
sorted by brick (z, y, x), as `export_bricks` returns them.  A listed brick is HELD, whether or not
one of its voxels is observed (W > 0).  The rule:

  * a brick's owner is the lowest rank holding it;
  * every other holder sends the brick's tile (its S and W as they are before the reduce) to the
    owner, which merges its sources in ascending rank order, voxel by voxel, where w_in > 0:
        W == 0:  (S, W) = (s_in, w_in)                                  the copy
        else:    S = (S * W + s_in * w_in) / (W + w_in),  W = min(W + w_in, max_weight)
    in fp32 with one rounding per operation (the library is built with -ffp-contract=off);
    max_weight is +inf under VDBFusion;
  * a sent brick ends as (background, 0) and stays held.  The background is sdf_trunc under
    VDBFusion and 0 under Voxblox.
"""
import functools

import numpy as np

import hashref
import meshref

F = np.float32
TOP = hashref.BRICK_KEY_BIAS - 1  # the highest brick coordinate a key holds


def as_export(e):
    c, s, w = e
    c = np.ascontiguousarray(c, np.int32).reshape(-1, 3)
    return (c, np.ascontiguousarray(s, F).reshape(len(c), 512),
            np.ascontiguousarray(w, F).reshape(len(c), 512))


def keys_of(coords):
    return hashref.brick_key(np.asarray(coords, np.int64).reshape(-1, 3))


def coords_of(keys):
    k = np.asarray(keys).astype(np.uint64)
    m = np.uint64(0x1FFFFF)
    c = np.stack([k & m, (k >> np.uint64(21)) & m, (k >> np.uint64(42)) & m], -1).astype(np.int64)
    return c - hashref.BRICK_KEY_BIAS


def empty_export():
    return np.zeros((0, 3), np.int32), np.zeros((0, 512), F), np.zeros((0, 512), F)


def owners(exports):
    """Per rank, per listed brick: the lowest rank whose export lists that key."""
    low = {}
    for r, e in enumerate(exports):
        for k in keys_of(e[0]).tolist():
            low.setdefault(k, r)
    return [np.array([low[k] for k in keys_of(e[0]).tolist()], np.int64) for e in exports]


def splits(exports):
    """(world, world): tiles that source r sends to owner d (what border_pack returns per rank)."""
    world = len(exports)
    m = np.zeros((world, world), np.int64)
    for r, o in enumerate(owners(exports)):
        for d in o[o != r].tolist():
            m[r, d] += 1
    return m


def merge_tile(S, W, s_in, w_in, max_weight):
    """One source tile merged into (S, W), all fp32 arrays of one shape; returns the new (S, W)."""
    mw = F(max_weight)
    obs = w_in > 0
    copy = obs & (W == 0)
    nw = W + w_in
    with np.errstate(invalid="ignore", divide="ignore"):
        mean = (S * W + s_in * w_in) / nw
    S2 = np.where(copy, s_in, np.where(obs, mean, S)).astype(F)
    W2 = np.where(copy, w_in, np.where(obs, np.where(nw > mw, mw, nw), W)).astype(F)
    return S2, W2


def reduce_in_order(exports, order, max_weight=np.inf, background=0.0):
    """The committed reduce with the sources of every owner taken in the rank order `order` (a
    sequence of all ranks).  Returns (per-rank exports after the reduce, tiles moved)."""
    exports = [as_export(e) for e in exports]
    own = owners(exports)
    out = [(c.copy(), s.copy(), w.copy()) for c, s, w in exports]
    index = [{k: i for i, k in enumerate(keys_of(e[0]).tolist())} for e in exports]
    moved = 0
    for r in order:
        c, s, w = exports[r]
        for i, k in enumerate(keys_of(c).tolist()):
            d = int(own[r][i])
            if d == r:
                continue
            j = index[d][k]
            out[d][1][j], out[d][2][j] = merge_tile(out[d][1][j], out[d][2][j], s[i], w[i],
                                                    max_weight)
            moved += 1
    for r in range(len(exports)):
        sent = own[r] != r
        out[r][1][sent] = F(background)
        out[r][2][sent] = F(0)
    return out, moved


def reduce(exports, max_weight=np.inf, background=0.0):
    """The committed reduce: sources in ascending rank order."""
    return reduce_in_order(exports, range(len(exports)), max_weight, background)


def observed(export):
    c, _, w = as_export(export)
    return (w > 0).any(1)


def halo_needed(export):
    """brick_halo_needed restated: the +x / +y / +z neighbours (7 per brick) of the bricks with an
    observed voxel that are not observed here, as brick coordinates (n, 3) sorted by key; a
    neighbour past the top of a key field has no key and is skipped."""
    c = as_export(export)[0].astype(np.int64)[observed(export)]
    have = {tuple(b) for b in c.tolist()}
    need = set()
    for b in c.tolist():
        for d in range(1, 8):
            q = (b[0] + (d & 1), b[1] + ((d >> 1) & 1), b[2] + (d >> 2))
            if max(q) > TOP or q in have:
                continue
            need.add(q)
    q = np.array(sorted(need), np.int64).reshape(-1, 3)
    return q[np.argsort(keys_of(q))] if len(q) else q


def halo_answer(export, keys):
    """(keys, S, W) of the requested keys (uint64) whose brick this rank observes, sorted by key."""
    c, s, w = as_export(export)
    mine = {k: i for i, k in enumerate(keys_of(c).tolist()) if (w[i] > 0).any()}
    hit = sorted(k for k in set(np.asarray(keys).astype(np.uint64).tolist())
                 if k in mine and k != 0xFFFFFFFFFFFFFFFF)
    rows = [mine[k] for k in hit]
    return np.array(hit, np.uint64), s[rows], w[rows]


def union_field(exports):
    """{brick (x, y, z): (S (512,), W (512,))} of the ranks' observed bricks together; after a
    reduce each brick is observed on one rank."""
    field = {}
    for e in exports:
        c, s, w = as_export(e)
        for i in np.flatnonzero(observed(e)).tolist():
            b = tuple(c[i].tolist())
            assert b not in field, "a brick is observed on two ranks"
            field[b] = (s[i], w[i])
    return field


def _around(field, q, margin=2):
    """The dense (S, W, origin) of the voxels [8 q - margin, 8 q + 9 + margin) cut out of `field`:
    every voxel the cubes of brick q read, the gradients' one voxel more included."""
    lo = 8 * np.asarray(q, np.int64) - margin
    n = 9 + 2 * margin
    S, W = np.zeros((n, n, n), F), np.zeros((n, n, n), F)
    for d in _block(range(-1, 2), range(-1, 2), range(-1, 2)).tolist():
        b = tuple((np.asarray(q, np.int64) + d).tolist())
        if b not in field:
            continue
        s, w = (a.reshape(8, 8, 8) for a in field[b])
        o = 8 * np.asarray(b, np.int64) - lo               # the brick's min voxel in the window
        a0, a1 = np.maximum(o, 0), np.minimum(o + 8, n)    # window range it covers (x, y, z)
        if np.any(a0 >= a1):
            continue
        src = tuple(slice(a0[k] - o[k], a1[k] - o[k]) for k in (2, 1, 0))
        dst = tuple(slice(a0[k], a1[k]) for k in (2, 1, 0))
        S[dst], W[dst] = s[src], w[src]
    return S, W, lo


def rank_soup(field, own_observed_bricks, voxel_size, tab, min_weight=0.0):
    """The triangles (3 T, 3) of the cubes whose min voxel lies in one of the rank's observed
    bricks, bricks in (z, y, x) order.  `field` is the union's (`union_field`).  Per brick q, one
    indexed_mesh_ref box [8 q, 8 q + 8) on the field cut out two voxels around what its cubes read,
    so the cost grows with the bricks and not with the map's extent."""
    b = np.asarray(own_observed_bricks, np.int64).reshape(-1, 3)
    out = [np.zeros((0, 3), F)]
    for q in b[np.argsort(keys_of(b))] if len(b) else b:
        S, W, origin = _around(field, q)
        v, _, t = meshref.indexed_mesh_ref(S, W, origin, voxel_size, tab, min_weight,
                                           lo=8 * q, hi=8 * q + 8)
        if len(t):
            out.append(meshref.deindex(v, t))
    return np.concatenate(out)


# ---- case builders -------------------------------------------------------------------------------
VS, TAU = 0.05, 0.15


def _sorted(coords):
    c = np.asarray(coords, np.int64).reshape(-1, 3)
    return c[np.argsort(keys_of(c))]


def _brick_field(coords, rng, background, normal=(0.6, 0.5, 0.62), through=(0.0, 0.0, 0.0),
                 hole=0.1, noise=0.004, w_lo=0.25, w_hi=3.0, obs=None, scale=1.0):
    """(coords, S, W) of a plane through voxel `through` (voxel units) over the bricks `coords`:
    S is the distance times `scale`, clamped, plus a per-rank noise; W is uniform and non-integer.
    A seeded share `hole` of the voxels is unobserved (W = 0, S = the background), unless `obs`
    (n, 512) says which voxels are observed."""
    c = _sorted(coords)
    l = np.arange(512)
    local = np.stack([l & 7, (l >> 3) & 7, l >> 6], -1)
    v = c[:, None, :] * 8 + local[None] + 0.5 - np.asarray(through, np.float64)
    n = np.asarray(normal, np.float64)
    d = (v @ (n / np.linalg.norm(n))) * (VS * scale) + rng.normal(0.0, noise, v.shape[:2])
    s = np.clip(d, -TAU, TAU).astype(F)
    w = rng.uniform(w_lo, w_hi, s.shape).astype(F)
    seen = rng.random(s.shape) >= hole if obs is None else obs
    w[~seen] = 0
    s[~seen] = F(background)
    return c.astype(np.int32), s, w


def _block(x, y, z):
    return np.stack(np.meshgrid(x, y, z, indexing="ij"), -1).reshape(-1, 3)


def fan_in(background=0.0, seed=3):
    """World 8, 24 bricks: 6 held by all 8 ranks, 6 by ranks {1, 4, 7} (ranks 4 and 7 send them
    to rank 1, past the ranks in between, which do not hold them), 12 by one to three ranks."""
    rng = np.random.default_rng(seed)
    bricks = _block(range(-2, 2), range(-1, 2), range(-1, 1))
    holders = [list(range(8))] * 6 + [[1, 4, 7]] * 6 + [[0]] * 3 + [[2, 5]] * 3 + [[3, 6, 7]] * 3 \
        + [[5]] * 2 + [[0, 7]]
    exports = []
    for r in range(8):
        mine = [b for b, h in zip(bricks.tolist(), holders) if r in h]
        exports.append(_brick_field(mine, rng, background) if mine else empty_export())
    return exports, dict(world=8, bricks=24, all8=bricks[:6], r147=bricks[6:12], holders=holders)


def paths(background=0.0, seed=5):
    """World 3, 12 bricks held by all three: every voxel draws (observed at the owner, at source 1,
    at source 2) independently, so each of the 7 non-empty combinations holds about 768 voxels.  The
    plane is flattened so that few voxels sit on the clamp: S takes many values."""
    rng = np.random.default_rng(seed)
    bricks = _block(range(-1, 2), range(0, 2), range(-1, 1))
    exports, obs = [], []
    for r in range(3):
        o = rng.random((12, 512)) < 0.5
        obs.append(o)
        exports.append(_brick_field(bricks, rng, background, obs=o, scale=0.15))
    combo = obs[0].astype(int) | (obs[1].astype(int) << 1) | (obs[2].astype(int) << 2)
    return exports, dict(world=3, bricks=12, combo=combo)


def capped(background=0.0, seed=7):
    """World 3, 12 bricks held by all three, weights in [0.25, 3.0] for max_weight = 3.0 (Voxblox:
    the background is 0)."""
    rng = np.random.default_rng(seed)
    bricks = _block(range(0, 3), range(-2, 0), range(0, 2))
    exports = [_brick_field(bricks, rng, background) for _ in range(3)]
    return exports, dict(world=3, bricks=12, max_weight=3.0)


def empty_ranks(background=0.0, seed=9, all_empty=False):
    """World 4, 10 bricks: ranks 0 and 2 hold nothing, ranks 1 and 3 seven each, four shared; or
    every rank empty."""
    rng = np.random.default_rng(seed)
    bricks = _block(range(-3, 2), range(0, 2), [0])
    if all_empty:
        return [empty_export() for _ in range(4)], dict(world=4, bricks=0)
    exports = [empty_export(), _brick_field(bricks[:7], rng, background), empty_export(),
               _brick_field(bricks[3:], rng, background)]
    return exports, dict(world=4, bricks=10, shared=4)


def high_ranks(background=0.0, seed=11):
    """World 64, 8 bricks held by ranks 0, 31 and 63 only (the other 61 ranks have no context)."""
    rng = np.random.default_rng(seed)
    bricks = _block(range(0, 8), [-1], [2])
    exports = [empty_export() for _ in range(64)]
    exports[0] = _brick_field(bricks[:5], rng, background)
    exports[31] = _brick_field(bricks[2:7], rng, background)
    exports[63] = _brick_field(bricks[3:], rng, background)
    return exports, dict(world=64, bricks=8, live=(0, 31, 63))


ONE_CHAIN_MAX_BRICKS = 256  # the global table then has 512 slots (hashref.table_mask)


@functools.lru_cache(maxsize=None)
def _chain_set(n, seed):
    bits = (hashref.table_mask(ONE_CHAIN_MAX_BRICKS) + 1).bit_length() - 1
    return hashref.chain_bricks(n, bits, tail=8, seed=seed, r=48)


def one_chain(background=0.0, seed=13):
    """World 3, 80 bricks each out of 120 whose home lies in the last 8 slots of the 512-slot
    global table of a context with max_bricks = 256: every key of every rank sits on one probe
    chain that runs over the table's end."""
    rng = np.random.default_rng(seed)
    pool, _ = _chain_set(120, seed)
    exports, sets = [], []
    for r in range(3):
        mine = pool[rng.choice(120, 80, replace=False)]
        sets.append(mine)
        exports.append(_brick_field(mine, rng, background, normal=(0.0, 0.0, 1.0),
                                    through=(0.0, 0.0, 4.0), noise=0.02))
    mask = hashref.table_mask(ONE_CHAIN_MAX_BRICKS)
    return exports, dict(world=3, max_bricks=ONE_CHAIN_MAX_BRICKS, mask=mask,
                         facts=[hashref.chain_facts(s, mask, 8) for s in sets])


def halo_corner(background=0.0, seed=17):
    """World 3, 28 bricks.  27 are the block [-2, 0] x [-2, 0] x [0, 2] near the origin, brick b
    observed by rank (bx + by + bz) mod 3 alone (the state after a reduce), with a plane through the
    corner shared by the eight bricks [-2, -1] x [-2, -1] x [0, 1]: those eight belong to all three
    ranks.  No hole within 3 voxels of the corner.  Near the origin fp32 resolves the vertices'
    interpolation along every axis.  The 28th brick, on rank 1, is (TOP, 0, 1), at the top of the
    key range in x, with a plane of its own."""
    rng = np.random.default_rng(seed)
    bricks = _block(range(-2, 1), range(-2, 1), range(0, 3))
    corner = np.array([-8, -8, 8], np.int64)  # min voxel of brick (-1, -1, 1)
    rank = (bricks.sum(1)) % 3
    top = np.array([[TOP, 0, 1]], np.int64)
    exports = []
    for r in range(3):
        mine = _sorted(bricks[rank == r])
        l = np.arange(512)
        local = np.stack([l & 7, (l >> 3) & 7, l >> 6], -1)
        v = mine[:, None, :] * 8 + local[None]
        near = np.abs(v - corner).max(-1) <= 3
        obs = near | (rng.random(near.shape) >= 0.05)
        c, s, w = _brick_field(mine, rng, background, through=corner.astype(np.float64),
                               noise=0.0, obs=obs)
        if r == 1:
            tc, ts, tw = _brick_field(top, rng, background, noise=0.0, hole=0.02,
                                      through=8.0 * top[0] + 4.0)
            c, s, w = np.concatenate([c, tc]), np.concatenate([s, ts]), np.concatenate([w, tw])
            o = np.argsort(keys_of(c))
            c, s, w = c[o], s[o], w[o]
        exports.append((c, s, w))
    around = _block(range(-2, 0), range(-2, 0), range(0, 2))
    return exports, dict(world=3, bricks=28, corner=corner, around=around, top=top[0])


def corner_cube_ranks(exports, cube_min):
    """The ranks observing the bricks of the eight voxels of the cube at min voxel `cube_min`, or
    None when one of the voxels is unobserved."""
    ranks = set()
    for q in range(8):
        v = np.asarray(cube_min, np.int64) + [q & 1, (q >> 1) & 1, q >> 2]
        b, loc = v >> 3, v & 7
        hit = None
        for r, e in enumerate(exports):
            c, _, w = as_export(e)
            i = np.flatnonzero((c == b).all(1))
            if len(i) and w[i[0], loc[0] + 8 * loc[1] + 64 * loc[2]] > 0:
                hit = r
        if hit is None:
            return None
        ranks.add(hit)
    return ranks


CASES = dict(fan_in=fan_in, paths=paths, capped=capped, empty_ranks=empty_ranks,
             all_empty=functools.partial(empty_ranks, all_empty=True), high_ranks=high_ranks,
             one_chain=one_chain, halo_corner=halo_corner)


@functools.lru_cache(maxsize=None)
def case(name, background=0.0):
    """(exports, facts) of a case, built once per background; treat as read-only."""
    exports, facts = CASES[name](background=background)
    for e in exports:
        for a in e:
            a.setflags(write=False)
    return exports, facts
