"""Scan-to-map pose refinement against the TSDF (include/tsdf_hip_sample.h).

`refine_pose` minimises the point-to-TSDF error sum_i S(T p_i)^2 of a cloud over the pose T by
plain Gauss-Newton: each step asks the map for the normal equations under the current pose
(`HipTSDFVolume.align_terms`: one fused kernel over the cloud, 44 doubles back) and solves one 6x6
system on the host.  There is NO damping, NO robust kernel and no step control: it refines a pose
that is already inside the basin of the map's surface (centimetres, fractions of a degree — an
odometry prior), it is not a global registration.  Points whose 8 surrounding voxels are not all
observed with weight >= min_weight take no part.
"""
import math

import numpy as np


class AlignError(RuntimeError):
    pass


def exp_so3(w):
    """Rotation matrix of a rotation vector (Rodrigues' formula, float64)."""
    w = np.asarray(w, np.float64).reshape(3)
    th = float(np.linalg.norm(w))
    K = np.array([[0.0, -w[2], w[1]], [w[2], 0.0, -w[0]], [-w[1], w[0], 0.0]])
    if th < 1e-12:
        return np.eye(3) + K
    return np.eye(3) + (math.sin(th) / th) * K + ((1.0 - math.cos(th)) / (th * th)) * (K @ K)


def solve_step(H, b, n_valid):
    """delta = (dt, dtheta) of H delta = -b; raises AlignError when the system does not determine
    a pose (fewer than 6 valid points, or H singular)."""
    if n_valid < 6:
        raise AlignError("only %d valid points: the map does not constrain the pose" % n_valid)
    H = np.asarray(H, np.float64)
    if not np.all(np.isfinite(H)) or np.linalg.matrix_rank(H) < 6:
        raise AlignError("singular normal equations (degenerate geometry)")
    try:
        return np.linalg.solve(H, -np.asarray(b, np.float64))
    except np.linalg.LinAlgError as e:
        raise AlignError("singular normal equations (%s)" % e)


def apply_step(pose, delta):
    """The left update R <- exp(dtheta) R, t <- exp(dtheta) t + dt of a 3x4 pose."""
    T = np.asarray(pose, np.float64).reshape(3, 4)
    E = exp_so3(delta[3:])
    out = np.empty((3, 4))
    out[:, :3] = E @ T[:, :3]
    out[:, 3] = E @ T[:, 3] + np.asarray(delta[:3], np.float64)
    return out


def refine_pose(volume, points, pose0, iters=6, min_weight=0.0):
    """Refine `pose0` (3x4 or 4x4, world from cloud) of `points` ((N, 3) array) against `volume`'s
    map.  Returns (pose (3, 4) float64, steps): steps[k] = {"rms", "n_valid"} of the error at the
    pose step k started from.  Undamped Gauss-Newton, no robust kernel (see the module text).
    Raises AlignError if a step has fewer than 6 valid points or singular normal equations."""
    T = np.asarray(pose0, np.float64)
    if T.shape == (4, 4):
        T = T[:3]
    if T.shape != (3, 4):
        raise ValueError("pose0 must be a (3, 4) or (4, 4) matrix")
    T = T.copy()
    import torch
    pts = np.ascontiguousarray(np.asarray(points, np.float32).reshape(-1, 3))
    d_pts = torch.from_numpy(pts).to(volume.tensor_device)  # uploaded once for every step
    torch.cuda.synchronize(d_pts.device)
    steps = []
    for _ in range(int(iters)):
        H, b, e, nv = volume.align_terms(d_pts.data_ptr(), T, min_weight, n=pts.shape[0])
        delta = solve_step(H, b, nv)
        steps.append({"rms": math.sqrt(e / nv), "n_valid": nv})
        T = apply_step(T, delta)
    return T, steps
