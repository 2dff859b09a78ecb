"""The quality table of DESIGN 4t from the numpy statement of tests/smooth_ref.py (no GPU): RMS radial error and volume of the unit
icosphere(3) with 2 % radial noise, before and after 10 Taubin pairs and 20 Laplacian steps; how many vertices a clamp of 0.01 stops.
Writes profiles/mesh_smooth_quality.json.
usage: python tools/mesh_smooth_quality.py"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np

import smooth_ref as S


def main():
    v, f, clean = S.noisy_icosphere(3)
    row = lambda x: {"rms radial error": S.rms_radial_error(x), "volume": S.volume(x, f)}
    taubin = S.smooth_steps(v, f, S.factors_of("taubin", 10))[0]
    clamped = S.smooth_steps(v, f, S.factors_of("taubin", 10), max_move=0.01)[0]
    x0 = v.astype(np.float64)
    on = ((clamped == (x0 + 0.01).astype(np.float32)) | (clamped == (x0 - 0.01).astype(np.float32))).any(1)
    out = {"mesh": "icosphere(3), 642 vertices, radial noise 0.02 (seed 5)", "without noise": row(clean), "input": row(v),
           "10 taubin pairs (0.5 / -0.53)": row(taubin), "20 laplacian steps of 0.5": row(S.smooth_steps(v, f, [0.5] * 20)[0]),
           "10 taubin pairs, max_move 0.01": dict(row(clamped), **{"vertices on the clamp": int(on.sum())})}
    text = json.dumps(out, indent=1)
    print(text)
    with open(os.path.join(ROOT, "profiles", "mesh_smooth_quality.json"), "w") as fh:
        fh.write(text + "\n")


if __name__ == "__main__":
    main()
