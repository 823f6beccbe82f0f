"""Writes tests/golden/sift_48x64.npz: the 48 x 64 texture of tests/sift_cases.py and what the
float64 restatement tests/sift_ref.py gives for it (num_keypoints = 16, sigma = 1.6): the
keypoints kf (x, y, size, angle, response as fp32), ki (octave, layer) and the descriptors as
uint8. tests/test_sift_ref.py asks the oracle to reproduce it, so a change of the oracle shows.

    python tests/golden/make_sift_golden.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from tests import sift_cases, sift_ref  # noqa: E402

NUM_KEYPOINTS, SIGMA = 16, 1.6


def main() -> None:
    image = np.array(sift_cases.texture(48, 64))
    out = sift_ref.extract(image, NUM_KEYPOINTS, SIGMA)
    assert (out["x"] == np.rint(out["x"])).all()
    path = os.path.join(HERE, "sift_48x64.npz")
    np.savez_compressed(path, image=image, num_keypoints=NUM_KEYPOINTS, sigma=SIGMA,
                        kf=out["kf"], ki=out["ki"], x=out["x"].astype(np.uint8))
    print(f"{path}: {len(out['kf'])} keypoints, {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
