"""Digests of oracle/sift_oracle.c's keypoints and descriptors (tests/test_sift_oracle.py).

Run from the repository root:  python tests/golden/make_sift_oracle_digests.py
Writes tests/golden/sift_oracle_digests.json: per input the keypoint count and the SHA-256 of the
keypoint bytes (KEYPOINT_DTYPE records) and of the descriptor bytes (float32 rows).  The file was
recorded from the oracle as it stood before its pyramid construction became a function of its own
(orc_sift_pyramid), and pins that the split changed no output.  Regenerating it re-pins whatever the
oracle computes now, so do that only for a deliberate change of the oracle.
"""
import hashlib
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))          # tests/
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))  # repository root


def inputs():
    """(label, image, mask) of every pinned input."""
    from sift_inputs import PYRAMID_SHAPES, pyramid_case
    with np.load(os.path.join(HERE, "sift_images.npz")) as z:
        for k in sorted(z.files):
            if k.startswith("view/"):
                yield k, z[k], None
                yield k + "+mask", z[k], z["mask/" + k[5:]]
            elif k.startswith("scene/"):
                yield k, z[k], None
    for i, (r, c) in enumerate(PYRAMID_SHAPES):
        yield f"multi{100 + i}/{r}x{c}", pyramid_case(i), None


def digest(oracle, img, mask):
    k, d = oracle.sift_detect_compute(img, mask)
    return {"n": int(len(k)), "keypoints": hashlib.sha256(np.ascontiguousarray(k).tobytes()).hexdigest(),
            "descriptors": hashlib.sha256(np.ascontiguousarray(d).tobytes()).hexdigest()}


def main():
    from oracle import oracle as O
    O.build()
    out = {label: digest(O, img, mask) for label, img, mask in inputs()}
    path = os.path.join(HERE, "sift_oracle_digests.json")
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(path, {k: v["n"] for k, v in out.items()})


if __name__ == "__main__":
    main()
