#!/usr/bin/env python3
"""One observation of what aligned crops are for (GPU only): the three views of
tests/golden/sad_linus_mesh.npz -- one face at view_deg 0, +10 and -10, `codes` as 192 x 192 frames with
their `landmarks` -- embedded with the golden MobileFaceNet from the bounding crop (landmark_crop_view, what
recognition crops without alignment) and from the aligned crop (aligned_crop_view with the five-point
defaults), and the three embedding distances of each.  One face at +-10 degrees is an observation, not an
accuracy claim.  Prints one JSON document."""
import json
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tools"))


def main():
    import make_golden_recognition as mg
    import zaru_amd.host as H
    g = np.load(os.path.join(REPO, "tests", "golden", "sad_linus_mesh.npz"))
    emb = H.FaceEmbedder(mg.load_model_bytes())
    al = H.FaceAlignment.facemesh_five_point()
    out = {"tool": "tools/align_roll_sensitivity.py", "view_deg": [float(v) for v in g["view_deg"]], "fits": []}
    e = {"bounding": [], "aligned": []}
    for v in range(3):
        frame = np.full((192, 192, 4), 255, np.uint8)
        frame[..., :3] = np.transpose(g["codes"][v], (1, 2, 0))
        lm = np.ascontiguousarray(g["landmarks"][v], np.float32)
        bound = H.landmark_crop_view(lm, 192, 192, 1, 1, 0.4)
        view, rec = H.aligned_crop_view(lm, 192, 192, al)
        assert view is not None
        out["fits"].append({k: float(rec[k]) for k in ("scale", "angle", "residual")})
        e["bounding"].append(np.asarray(emb.embed_views(frame, [bound]), np.float32)[0])
        e["aligned"].append(np.asarray(emb.embed_views(frame, [view]), np.float32)[0])
    for kind, v in e.items():
        out[kind] = {f"d({a},{b})": round(float(H.Embedding(v[a]).difference(H.Embedding(v[b]))), 4)
                     for a, b in ((0, 1), (0, 2), (1, 2))}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
