"""Writes tests/golden/jpeg_entropy_golden.npz: JPEG streams for the Huffman stage on the device (csrc/jpeg_huffman_exact.hip) - streams
only, no pixels: the device stage is compared with the host stage, coefficient for coefficient.

    python tests/golden/make_jpeg_entropy_golden.py

Needs Pillow (libjpeg-turbo) and the built library (the corrupted scans record what the HOST entropy stage says about them).  Keys:
g<i>_jpeg / g_names: one 4:2:0 stream whose scan covers at least three workgroups of the Huffman launches (two seams) with an FF 00 pair
across a subsequence boundary (asserted here against the constants of include/danhip.h; the seed is chosen for it), one of the same kind
with a restart interval longer than a workgroup, one 4:4:4 and one grey stream above 40 KB.  c_base_jpeg: a 45 KB 4:2:0 stream;
c_kinds / c<i>_params / c_outcomes: corrupted scans made from it by tests/jpeg_entropy_fixtures.py::corrupt (three flipped bytes, a run of
FF FF inserted, the scan cut at an odd byte, the scan replaced by seeded noise) and the host stage's outcome: 0 = decodes, else its reason."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import jpeg_entropy_fixtures as F  # noqa: E402
from make_jpeg_golden import encode, synthetic  # noqa: E402


def main():
    from dan_amd import _lib
    K = F.header_constants()
    S, G = K["DANHIP_JPEG_SUBSEQ_BYTES"], K["DANHIP_JPEG_SUBSEQ_PER_GROUP"]
    out, names = {}, []
    seed = 3000
    while True:                                                             # the seed: a stuffed pair must straddle a subsequence boundary
        big = encode(synthetic(392, 520, seed), 2, quality=90)
        if F.straddling_stuffed_pairs(big, S) and F.scan_end(big) - F.scan_start(big) > 2 * S * G + S:
            break
        seed += 1
    assert (F.scan_end(big) - F.scan_start(big) + S * G - 1) // (S * G) >= 3
    names.append("420_520x392_q90_seed%d" % seed)
    out["g0_jpeg"] = big
    rst = encode(synthetic(392, 520, seed + 1), 2, quality=90, restart_marker_rows=10)
    first = rst.index(b"\xff\xd0", F.scan_start(rst)) - F.scan_start(rst)
    assert first > S * G, first                                             # a restart interval longer than one workgroup
    names.append("420_520x392_q90_rst_rows10")
    out["g1_jpeg"] = rst
    names.append("444_184x136_q95")
    out["g2_jpeg"] = encode(synthetic(136, 184, seed + 2), 0, quality=95)
    names.append("grey_288x216_q95")
    out["g3_jpeg"] = encode(synthetic(216, 288, seed + 3), None, quality=95)
    assert len(out["g2_jpeg"]) > 40000 and len(out["g3_jpeg"]) > 40000
    for i in range(len(names)):
        out["g%d_jpeg" % i] = np.frombuffer(out["g%d_jpeg" % i], np.uint8)
    out["g_names"] = np.asarray(names)

    base = encode(synthetic(200, 264, seed + 4), 2, quality=95)
    n = F.scan_end(base) - F.scan_start(base)
    r = np.random.RandomState(seed)
    flips = []
    for pos in (n // 7, n // 2 + 1, n - n // 9):
        flips += [pos, int(r.randint(1, 255)) ^ base[F.scan_start(base) + pos] or 1]
    recipes = [("flip3", flips), ("ff_run", [n // 3, 3]), ("cut_odd", [(n // 2) | 1]), ("noise", [seed])]
    outcomes = []
    for i, (kind, params) in enumerate(recipes):
        out["c%d_params" % i] = np.asarray(params, np.int64)
        data = F.corrupt(base, kind, out["c%d_params" % i])
        outcomes.append(F.host_decode(_lib.lib(), _lib.JpegDesc, _lib.JpegInfo, [data])[2][0])
    out["c_base_jpeg"] = np.frombuffer(base, np.uint8)
    out["c_kinds"] = np.asarray([k for k, _ in recipes])
    out["c_outcomes"] = np.asarray(outcomes, np.int32)
    np.savez_compressed(F.PATH, **out)
    print(F.PATH, os.path.getsize(F.PATH), "bytes;", [(n, len(out["g%d_jpeg" % i])) for i, n in enumerate(names)], "base", len(base), "outcomes", outcomes)
    assert os.path.getsize(F.PATH) < 400 * 1024


if __name__ == "__main__":
    main()
