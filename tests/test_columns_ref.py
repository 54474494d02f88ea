"""tests/colref.py, the numpy restatement of include/tsdf_hip_columns.h, held to its per-column
scalar twin and to known answers on the CPU; and the conditions on the room that
tests/test_columns_gpu.py relies on, asserted here on the reference alone."""
import numpy as np
import pytest

import colref as cr

F = np.float32
VS = cr.VS
NAN_BITS = 0x7FC00000


def col(s, w=None, z0=0, vs=VS, **kw):
    """The maps of one column as Python scalars, from both twins (asserted equal)."""
    s = np.asarray(s, F).reshape(-1, 1, 1)
    w = np.ones_like(s) if w is None else np.asarray(w, F).reshape(-1, 1, 1)
    a = cr.column_map(s, w, z0, vs, **kw)
    b = cr.column_map_scalar(s, w, z0, vs, **kw)
    cr.assert_same(b, a)
    return tuple(x[0, 0] for x in a)


@pytest.mark.parametrize("seed", range(4))
def test_vectorised_equals_scalar_on_random_fields(seed):
    rng = np.random.default_rng(seed)
    shape = (23, 7, 9)
    S = rng.uniform(-0.3, 0.3, shape).astype(F)
    S[rng.random(shape) < 0.05] = F(np.nan)
    S[rng.random(shape) < 0.05] = F(-0.0)
    S[rng.random(shape) < 0.05] = F(0.0)
    W = rng.integers(0, 4, shape).astype(F)
    n_cross, kinds = 0, set()
    for band, mw, mo, mf in ((0.0, 0.0, 1, 1), (VS, 2.0, 8, 4), (-0.05, 1.0, 12, 9)):
        a = cr.column_map(S, W, -11 + seed, VS, band, mw, mo, mf)
        b = cr.column_map_scalar(S, W, -11 + seed, VS, band, mw, mo, mf)
        cr.assert_same(b, a)
        n_cross += int((a[4] & cr.HAS_ELEV != 0).sum()) + int((a[4] & cr.HAS_CEIL != 0).sum())
        kinds |= {int(f) & 7 for f in a[4].ravel()}
    assert n_cross > 60 and {1, 3, 5} <= kinds  # unknown, occupied and free columns
    assert np.isnan(S).any() and np.signbit(S[S == 0]).any() and (W == 0).any()


def test_zero_below_gives_the_centre_of_that_voxel():
    # S_{z-1} == 0 (the pair z = 6): t = 1, elev = (z - 0.5) vs, the centre of voxel z - 1
    e, c, no, nf, fl = col([-0.1, 0.0, 0.2], z0=4)
    assert e == F((F(6) + F(0.5)) - F(1)) * F(VS) and fl & cr.HAS_ELEV
    assert cr.bits(c) == NAN_BITS and not fl & cr.HAS_CEIL
    # the same with -0.0
    e2 = col([-0.1, -0.0, 0.2], z0=4)[0]
    assert cr.bits(e2) == cr.bits(e)
    # a down crossing onto S_z == 0: t = 1, the centre of voxel z
    e, c, *_ = col([0.2, 0.0], z0=-3)
    assert c == F((F(-3) + F(0.5)) + F(1)) * F(VS) and cr.bits(e) == NAN_BITS


def test_highest_up_and_lowest_down_win():
    s = [-0.1, 0.1, 0.2, -0.1, -0.2, 0.1, 0.3, -0.2]   # up at z = 1, 5; down at z = 3, 7
    e, c, no, nf, fl = col(s, z0=10)
    t = F(0.1) / (F(0.1) - F(-0.2))
    assert e == ((F(15) + F(0.5)) - t) * F(VS)
    t = F(0.2) / (F(0.2) - F(-0.1))
    assert c == ((F(12) + F(0.5)) + t) * F(VS)
    assert c < e and fl == (cr.OBSERVED | cr.OCCUPIED | cr.HAS_ELEV | cr.HAS_CEIL)
    assert (no, nf) == (4, 4)


def test_a_crossing_through_an_unobserved_voxel_is_not_one():
    e, c, no, nf, fl = col([-0.1, 0.3, 0.1], w=[1, 0, 1])
    assert cr.bits(e) == NAN_BITS and cr.bits(c) == NAN_BITS
    assert (no, nf, fl) == (1, 1, cr.OBSERVED | cr.OCCUPIED)
    e = col([-0.1, 0.3, 0.1], w=[1, 1, 1])[0]
    assert not np.isnan(e)


def test_min_weight_gates_voxels():
    s, w = [-0.1, 0.1, 0.2, -0.1], [2, 1, 2, 2]
    e, c, no, nf, fl = col(s, w, min_weight=0.0)
    assert fl & cr.HAS_ELEV and fl & cr.HAS_CEIL and (no, nf) == (2, 2)
    e, c, no, nf, fl = col(s, w, min_weight=2.0)
    assert not fl & cr.HAS_ELEV and fl & cr.HAS_CEIL and (no, nf) == (2, 1)
    e, c, no, nf, fl = col(s, w, min_weight=3.0)
    assert fl == 0 and (no, nf) == (0, 0)
    # W > 0 holds whatever min_weight is
    assert col([0.1], w=[0.0], min_weight=0.0)[4] == 0


def test_one_voxel_has_no_crossing():
    for s in (-0.1, 0.1):
        e, c, no, nf, fl = col([s])
        assert cr.bits(e) == NAN_BITS and cr.bits(c) == NAN_BITS
        assert fl == cr.OBSERVED | (cr.OCCUPIED if s < 0 else cr.FREE)


def test_thresholds_on_either_side():
    s = [-0.1, -0.1, 0.1, 0.1, 0.1]   # 2 occupied, 3 free at band 0
    assert col(s, min_occ=2)[4] & 7 == cr.OBSERVED | cr.OCCUPIED
    assert col(s, min_occ=3, min_free=3)[4] & 7 == cr.OBSERVED | cr.FREE
    assert col(s, min_occ=3, min_free=4)[4] & 7 == cr.OBSERVED  # unknown
    # occ_band moves voxels from free to occupied; a negative band is allowed
    assert col(s, occ_band=0.1)[2:4] == (5, 0)
    assert col(s, occ_band=-0.2)[2:4] == (0, 5)
    assert col([np.nan, 0.1])[2:4] == (0, 2)  # NaN S is never <= band


@pytest.mark.parametrize("min_weight", [0.0, 2.0])
def test_the_room_has_what_the_gpu_tests_compare(min_weight):
    kinds = []
    for k in range(8):
        lo = np.array([-13, 5, -21 + k])
        S, W = cr.room(lo)
        assert S.shape == cr.ROOM_N[::-1]
        ref = cr.column_map(S, W, lo[2], VS, 0.0, min_weight)
        c = cr.counts(S, W, min_weight, ref)
        st = cr.straddles(S, W, lo[2], min_weight)
        kinds.append(st)
        print(k, c, st)
        surfaces = 800 if min_weight == 0.0 else 400
        assert c["elev"] >= surfaces and c["ceil"] >= surfaces
        assert c["up2"] >= 30 and c["down2"] >= 30 and c["shelf"] >= 30
    # for some k each kind of chosen crossing pair straddles a z-brick boundary
    assert any(u > 0 for u, d in kinds) and any(d > 0 for u, d in kinds)
    assert any(u > 0 and d > 0 for u, d in kinds)


def test_the_room_twins_agree_and_bricks_round_trip():
    lo = np.array([-13, 5, -18])
    S, W = cr.room(lo)
    cr.assert_same(cr.column_map_scalar(S, W, lo[2], VS, VS, 2.0, 2, 3),
                   cr.column_map(S, W, lo[2], VS, VS, 2.0, 2, 3))
    assert ((W == 0) | ((W >= 1) & (W <= 4))).all() and {1, 2, 3, 4} <= set(np.unique(W))
    assert 0.2 < (W == 0).mean() < 0.8  # the voxels far from every surface, and 8 % of the rest
    coords, bs, bw = cr.bricks_of(S, W, lo)
    assert len(np.unique(coords, axis=0)) == len(coords) and (bw > 0).any(1).all()
    # a whole brick between the floor and the shelf is absent in some brick column
    full = {tuple(int(v) for v in c) for c in coords}
    assert any((bx, by, bz + 1) not in full and any((bx, by, bz + k) in full for k in range(2, 7))
               for bx, by, bz in full)
    # the slab box between floor and shelf: FREE and unknown columns at min_free = 3
    a, b = cr.ROOM_SLAB
    ref = cr.column_map(S[a:b], W[a:b], lo[2] + a, VS, 0.0, 0.0, 1, 3)
    kinds = ref[4] & 7
    assert (kinds == cr.OBSERVED | cr.FREE).sum() >= 50 and (kinds == cr.OBSERVED).sum() >= 50
    assert (kinds == 0).sum() >= 20
