#!/usr/bin/env python3
"""Writes the Procrustes fixtures under tests/golden/:

  procrustes_cases.json     the eight points of the reference's unit tests (procrustes.rs:263-272)
                            and its test transforms (:348-483) as row-major 4x4 matrices, built
                            here in f64 from their definitions and stored as f32 values
  canonical_face_mesh.npy   the 468 x 3 f32 vertices of the canonical face model (data only),
                            read from a Wavefront .obj given with --obj (its `v x y z` lines)

    tools/make_golden_procrustes.py [--obj canonical_face_model.obj]
"""
import argparse
import json
import os

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(REPO, "tests", "golden")

POINTS = [[-1.0, 1.0, 0.0], [1.0, 1.0, 0.0], [1.0, 1.5, 0.0], [1.75, 0.0, 0.0],
          [1.0, -1.5, 0.0], [1.0, -1.0, 0.0], [-1.0, -1.0, 0.0], [1.0, 1.0, 5.0]]


def T(x, y, z):
    m = np.eye(4)
    m[:3, 3] = [x, y, z]
    return m


def S(s):
    return np.diag([s, s, s, 1.0])


def rot(axisangle):
    """Rotation3::new: the rotation by |v| about v / |v| (Rodrigues)."""
    v = np.asarray(axisangle, np.float64)
    a = np.linalg.norm(v)
    m = np.eye(4)
    if a == 0.0:
        return m
    k = v / a
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    m[:3, :3] = np.eye(3) + np.sin(a) * K + (1 - np.cos(a)) * (K @ K)
    return m


def transforms():
    pi = float(np.float32(np.pi))
    ax = np.array([0.5, 1.0, -1.0])
    return [
        ("identity", np.eye(4)),
        ("translate_z", T(0, 0, 1)), ("translate_y", T(0, -4, 0)), ("translate_xyz", T(2, -4, -0.5)),
        ("scale_4", S(4.0)), ("scale_0.2", S(float(np.float32(0.2)))), ("scale_0", S(0.0)),
        ("rot_z_2", rot([0, 0, 2.0])), ("rot_z_-2", rot([0, 0, -2.0])),
        ("rot_axis_pi", rot(ax * pi)), ("rot_axis_-pi", rot(ax * -pi)),
        # Matrix4::from(R).append_translation(t).append_scaling(2) = S T R
        ("combination_1", S(2.0) @ T(1, 0.5, 2) @ rot(ax * pi)),
        # R * identity.append_translation(t).append_scaling(2) = R S T
        ("combination_2", rot(ax * pi) @ S(2.0) @ T(1, 0.5, 2)),
        ("combination_3", rot(ax * pi) @ S(float(np.float32(2.1))) @ T(-1, -0.5, 2) @ S(float(np.float32(0.3)))),
        ("combination_4", rot(ax * float(np.float32(2.3))) @ S(float(np.float32(2.1))) @ T(-1, -0.5, 2) @
         S(float(np.float32(0.3)))),
    ]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--obj", help="canonical_face_model.obj; without it only the JSON is written")
    args = ap.parse_args()
    cases = {
        "source": "crates/zaru/src/procrustes.rs tests: REFERENCE_POINTS and the transforms of test_identity, "
                  "test_translate, test_uniform_scaling, test_rotation, test_combinations, test_rot_around_z, "
                  "large_scale_and_move, jitter",
        "points": POINTS,
        "transforms": [{"name": n, "matrix": [float(np.float32(v)) for v in m.reshape(-1)]} for n, m in transforms()],
        "exact_scales": [2.0, 0.5],
        "z_rotation": [{"scale": s, "translation": t} for s, t in
                       [(1.0, [0.0, 0.0, 0.0]), (2.0, [0.0, 0.0, 0.0]), (0.5, [0.0, 0.0, 0.0]),
                        (1.0, [10.0, 0.0, 0.0]), (1.0, [-10.0, 7.0, 3.0]), (0.5, [10.0, 0.0, 0.0]),
                        (2.0, [-10.0, 7.0, 3.0]), (500.0, [0.5, 300.0, -1.0])]],
        "z_rotation_degrees": [-180, 360],
        "jitter": {"euler": [3.0, -1.0, 2.0], "factor": 100.0, "offset": [50.0, 200.0, -20.0]},
    }
    with open(os.path.join(GOLDEN, "procrustes_cases.json"), "w") as f:
        json.dump(cases, f, indent=1)
        f.write("\n")
    if args.obj:
        v = [[float(x) for x in line.split()[1:4]] for line in open(args.obj) if line.startswith("v ")]
        mesh = np.asarray(v, np.float32)
        assert mesh.shape == (468, 3), mesh.shape
        np.save(os.path.join(GOLDEN, "canonical_face_mesh.npy"), mesh)


if __name__ == "__main__":
    main()
