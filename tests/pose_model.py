"""float64 model of the listener-pose rule (include/jefferson.h: "listener poses"; csrc/jf_pose_rule.h), plain NumPy:
quaternion -> matrix, rel = R^T (p - c), np.arctan2.  Shared by tests/test_pose.py and tests/test_gpu_pose.py."""
import numpy as np


def rotation(q):
    """q [..., 4] = {qw, qx, qy, qz} (normalised here) -> R [..., 3, 3], head -> world: v_world = R v_head"""
    q = np.asarray(q, np.float64)
    q = q / np.linalg.norm(q, axis=-1, keepdims=True)
    w, x, y, z = q[..., 0], q[..., 1], q[..., 2], q[..., 3]
    R = np.empty(q.shape[:-1] + (3, 3))
    R[..., 0, 0], R[..., 0, 1], R[..., 0, 2] = 1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)
    R[..., 1, 0], R[..., 1, 1], R[..., 1, 2] = 2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)
    R[..., 2, 0], R[..., 2, 1], R[..., 2, 2] = 2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)
    return R


def angles(rel):
    """(ele, azi) in degrees, unrounded, azi in [0, 360): SoundSource.cu:20-36 in float64"""
    rel = np.asarray(rel, np.float64)
    x, y, z = rel[..., 0], rel[..., 1], rel[..., 2]
    ele = np.degrees(np.arctan2(y, np.sqrt(x * x + z * z)))
    azi = np.degrees(np.arctan2(-x, -z))
    return ele, np.where(azi < 0, azi + 360.0, azi)


def relative(poses, world):
    """poses [..., 7] = {c, q}, world [..., 3] -> rel [..., 3] = q* (p - c) q, float64"""
    poses = np.asarray(poses, np.float64)
    d = np.asarray(world, np.float64) - poses[..., :3]
    return np.einsum("...ji,...j->...i", rotation(poses[..., 3:]), d)


def to_world(poses, head):
    """the inverse: a head-relative point as a world position, R p + c in float64"""
    poses = np.asarray(poses, np.float64)
    return np.einsum("...ij,...j->...i", rotation(poses[..., 3:]), np.asarray(head, np.float64)) + poses[..., :3]


def round_deg(a):
    """whole degrees, halves away from zero (roundf)"""
    a = np.asarray(a, np.float64)
    return np.sign(a) * np.floor(np.abs(a) + 0.5)


def off_half(a):
    """distance of an angle from the nearest half degree, where its rounding flips"""
    return np.abs(np.asarray(a, np.float64) % 1.0 - 0.5)


def records(poses, world):
    """the model's latched records [..., 5] (x, y, z rounded to float32 once) and its unrounded (ele, azi)"""
    rel = relative(poses, world)
    ele, azi = angles(rel)
    out = np.empty(rel.shape[:-1] + (5,), np.float32)
    out[..., 0], out[..., 1] = round_deg(ele), round_deg(azi)
    out[..., 2:] = rel.astype(np.float32)
    origin = np.all(rel == 0.0, axis=-1)
    out[origin] = 0.0
    return out, ele, azi


def random_cases(n, seed, c_max=8.0, d_min=0.25, d_max=16.0):
    """n seeded (pose, point) pairs as float32: |c| <= c_max, d_min <= |p - c| <= d_max, random unit quaternions"""
    rng = np.random.default_rng(seed)

    def ball(r_lo, r_hi):
        v = rng.standard_normal((n, 3))
        v /= np.linalg.norm(v, axis=1, keepdims=True)
        return v * rng.uniform(r_lo, r_hi, (n, 1))
    c = ball(0.0, c_max)
    q = rng.standard_normal((n, 4))
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    poses = np.concatenate([c, q], axis=1).astype(np.float32)
    # (float32 rounding of c and p moves |p - c| by 1e-6 at the most: the radii keep a margin of 1e-3 inside the stated bounds)
    world = (poses[:, :3].astype(np.float64) + ball(d_min + 1e-3, d_max - 1e-3)).astype(np.float32)
    return poses, world
