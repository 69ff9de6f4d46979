"""References for the Procrustes analysis (crates/zaru/src/procrustes.rs) that the host mirror
(zaru_amd.host ProcrustesAnalyzer) and the device kernel (kernels/procrustes.hip) are checked
against: a numpy f64 Kabsch, and an f32 restatement of the reference's centroid and scale loops
(remove_translation :165-175, remove_scale :182-195) with every intermediate rounded to
np.float32, sequentially, in the reference's order."""
import json
import os

import numpy as np

F = np.float32
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def cases():
    with open(os.path.join(GOLDEN, "procrustes_cases.json")) as f:
        return json.load(f)


def canonical_mesh():
    return np.load(os.path.join(GOLDEN, "canonical_face_mesh.npy"))


def centroid_scale_f32(points, flip_y=False):
    """(centroid (3,) f32, scale f32) of an (n, 3) set: the two loops, step by step in f32."""
    p = np.array(points, F)
    if flip_y:
        p[:, 1] = -p[:, 1]
    n = F(len(p))
    c = [F(0.0), F(0.0), F(0.0)]
    for k in range(len(p)):
        for a in range(3):
            c[a] = F(c[a] + p[k, a])
    c = [F(v / n) for v in c]
    s = F(0.0)
    for k in range(len(p)):
        x, y, z = (F(p[k, a] - c[a]) for a in range(3))
        s = F(s + F(F(F(x * x) + F(y * y)) + F(z * z)))
    s = F(np.sqrt(F(s / n)))
    return np.array(c, F), s


def kabsch_f64(reference, points, flip_y=False):
    """scale, R (3x3), translation, centroid of the similarity transform reference -> points in
    f64, with the reference's conventions: RMS scale, R = U diag(1, 1, d) V^T of P^T Q,
    translation = centroid - scale * R * ref_centroid."""
    q = np.array(reference, np.float64)
    p = np.array(points, np.float64)
    if flip_y:
        p[:, 1] = -p[:, 1]
    qc, pc = q.mean(0), p.mean(0)
    q0, p0 = q - qc, p - pc
    qs, ps = np.sqrt((q0 ** 2).sum() / len(q)), np.sqrt((p0 ** 2).sum() / len(p))
    if ps == 0.0:
        R = np.eye(3)
    else:
        U, _, Vt = np.linalg.svd((p0 / ps).T @ (q0 / qs))
        d = np.sign(np.linalg.det(Vt @ U))
        R = U @ np.diag([1.0, 1.0, d]) @ Vt
    scale = ps / qs
    return scale, R, pc - scale * (R @ qc), pc


def quat_to_matrix(q):
    """{i, j, k, w} (any norm > 0) -> 3x3, f64."""
    i, j, k, w = (np.float64(v) for v in q)
    n = i * i + j * j + k * k + w * w
    s = 2.0 / n
    return np.array([[1 - s * (j * j + k * k), s * (i * j - k * w), s * (i * k + j * w)],
                     [s * (i * j + k * w), 1 - s * (i * i + k * k), s * (j * k - i * w)],
                     [s * (i * k - j * w), s * (j * k + i * w), 1 - s * (i * i + j * j)]])


def rotation_angle(Ra, Rb):
    """The angle (radians) of the rotation between two rotation matrices (angle_to)."""
    d = np.asarray(Ra, np.float64) @ np.asarray(Rb, np.float64).T
    # atan2 form: accurate near 0, where acos of the trace is not
    sin = np.linalg.norm([d[2, 1] - d[1, 2], d[0, 2] - d[2, 0], d[1, 0] - d[0, 1]]) / 2.0
    cos = (np.trace(d) - 1.0) / 2.0
    return float(np.arctan2(sin, cos))


def euler_matrix(roll, pitch, yaw):
    """UnitQuaternion::from_euler_angles: Rz(yaw) Ry(pitch) Rx(roll), f64."""
    cr, sr, cp, sp, cy, sy = np.cos(roll), np.sin(roll), np.cos(pitch), np.sin(pitch), np.cos(yaw), np.sin(yaw)
    rx = np.array([[1, 0, 0], [0, cr, -sr], [0, sr, cr]])
    ry = np.array([[cp, 0, sp], [0, 1, 0], [-sp, 0, cp]])
    rz = np.array([[cy, -sy, 0], [sy, cy, 0], [0, 0, 1]])
    return rz @ ry @ rx


def random_rotation(rng):
    """A uniformly random rotation matrix (f64) from a seeded generator."""
    q = rng.normal(size=4)
    return quat_to_matrix(q / np.linalg.norm(q))


def apply(matrix4, points):
    """Matrix4::transform_point on (n, 3) points, in f32."""
    m = np.asarray(matrix4, F).reshape(4, 4)
    p = np.asarray(points, F)
    return (p @ m[:3, :3].T + m[:3, 3]).astype(F)
