"""Writes tests/golden/jpeg_encode_golden.npz: the inputs of tests/jpeg_encode_cases.py and, for every case of its matrix, the bytes of
Image.fromarray(a).save(buf, "JPEG", quality=q, subsampling=s).  Needs Pillow with libjpeg-turbo (made with Pillow 12.2.0, libjpeg-turbo
3.1): the fixture pins those bytes for machines without it.

    python tests/golden/make_jpeg_encode_golden.py"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import jpeg_encode_cases as C  # noqa: E402


def main():
    keys, parts, offsets = [], [], [0]
    for key, h, w, content, sub, mode, q in C.cases():
        data = C.pillow_bytes(C.image(h, w, content), q, sub)
        keys.append(key)
        parts.append(np.frombuffer(data, np.uint8))
        offsets.append(offsets[-1] + len(data))
    inputs, ioff = [], [0]
    for (h, w) in C.SIZES:
        for c in C.CONTENTS:
            a = C.image(h, w, c).reshape(-1)
            inputs.append(a)
            ioff.append(ioff[-1] + a.size)
    np.savez_compressed(C.GOLDEN, keys=np.array(keys), offsets=np.array(offsets, np.int64), blob=np.concatenate(parts),
                        input_offsets=np.array(ioff, np.int64), input_blob=np.concatenate(inputs))
    print(C.GOLDEN, os.path.getsize(C.GOLDEN), "bytes,", len(keys), "cases")


if __name__ == "__main__":
    main()
