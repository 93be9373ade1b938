"""The reference of the face-chip tests (tests/test_face_chips_cpu.py, tests/test_face_chips_gpu.py, tests/test_eval_cli_chips_gpu.py):
dan_amd.utility.face_chips.rule (the rectangle rule in Python integers) plus oracle.evalpipe.cv2_resize_linear_u8 on numpy arrays.

The oracle takes fx / fy and computes with 1 / fx; the kernel computes with crop / size.  fx = size / crop makes the two scales equal up to
one unit in the last place of a double, and the coordinate they feed is rounded to float32 before it is used (29 bits coarser), so the two
give the same float32 unless the product lies within 2^-29 of a float32 rounding boundary; the tests' fixed boxes are compared bit for bit."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from oracle.evalpipe import cv2_resize_linear_u8  # noqa: E402
from dan_amd.utility.face_chips import rule  # noqa: E402


def chip_of(image, rect, size):
    """cv2.resize(image[yc1 : yc2 + 1, xc1 : xc2 + 1], (size, size), INTER_LINEAR)"""
    x1, y1, x2, y2 = rect
    crop = np.ascontiguousarray(image[y1:y2 + 1, x1:x2 + 1])
    out = cv2_resize_linear_u8(crop, float(size) / crop.shape[1], float(size) / crop.shape[0])
    assert out.shape == (size, size, 3)
    return out


def reference(images, dets, num, size, margin_pm=0, square=True, score_threshold=0.0, max_chips=None):
    """images: list of uint8 [H,W,3] arrays, dets float32 [B,R,5], num int [B] -> (chips: list of the first max_chips chips in (image, row)
    order, chip_src: int32 [len(chips), 6] rows (image, row, xc1, yc1, xc2, yc2), count: the number of rows that give a chip)."""
    dets = np.asarray(dets, dtype=np.float32)
    thr = np.float32(score_threshold)
    chips, src, count = [], [], 0
    for i, image in enumerate(images):
        H, W = image.shape[:2]
        for r in range(dets.shape[1]):
            if r >= int(num[i]) or dets[i, r, 4] < thr:
                continue
            rect = rule(dets[i, r], H, W, margin_pm, square)
            if rect is None:
                continue
            if max_chips is None or count < max_chips:
                chips.append(chip_of(image, rect, size))
                src.append((i, r) + tuple(rect))
            count += 1
    return chips, np.asarray(src, dtype=np.int32).reshape(-1, 6), count
