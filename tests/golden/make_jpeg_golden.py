"""Writes tests/golden/jpeg_golden.npz: small synthetic JPEG streams with Pillow's decoded RGB (the definition of right for the device
decoder of dan_amd/dataset/jpeg.py), and streams the host validator must refuse, each with the reason code it must give.

    python tests/golden/make_jpeg_golden.py

Needs Pillow (libjpeg-turbo).  Accepted cases: grey / 4:4:4 / 4:2:2 / 4:2:0 at 1x1, 7x9, 17x33, 40x56, 65x47 and 136x50 (width x height),
qualities 30 / 75 / 95 / 100, optimised Huffman tables, restart markers per MCU row and every 3 MCUs.  Keys: a<i>_jpeg (uint8 stream),
a<i>_rgb (uint8 [H,W,3]), a_names; r<i>_jpeg, r_names, r_reasons (DANHIP_JPEG_E* of include/danhip.h)."""
import io
import os

import numpy as np
from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))
ENOTJPEG, ETRUNCATED, EPROGRESSIVE, ECOMPONENTS, ETOOLARGE = 1, 2, 3, 7, 12
SIZES = [(1, 1), (7, 9), (17, 33), (40, 56), (65, 47), (136, 50)]          # width, height
MODES = [("grey", None), ("444", 0), ("422", 1), ("420", 2)]
QUALITIES = [30, 75, 95, 100]


def synthetic(h, w, seed):
    """Smooth gradients, a flat rectangle with hard edges, and noise."""
    r = np.random.RandomState(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    img = np.stack([xx * 255 // max(w - 1, 1), yy * 255 // max(h - 1, 1), ((xx + yy) * 7) % 256], 2).astype(np.float64)
    img[h // 3: 2 * h // 3 + 1, w // 4: w // 2 + 1] = r.randint(0, 256, 3)
    img += r.randn(h, w, 3) * 25
    return np.clip(img, 0, 255).astype(np.uint8)


def encode(img, sub, **kw):
    b = io.BytesIO()
    if sub is None:
        Image.fromarray(img[:, :, 1]).save(b, format="JPEG", **kw)
    else:
        Image.fromarray(img).save(b, format="JPEG", subsampling=sub, **kw)
    return b.getvalue()


def decode(data):
    return np.asarray(Image.open(io.BytesIO(data)).convert("RGB"), dtype=np.uint8)


def scan_start(data):
    """Offset of the first entropy-coded byte (after the SOS segment)."""
    p = 2
    while True:
        assert data[p] == 0xFF
        m, n = data[p + 1], (data[p + 2] << 8) | data[p + 3]
        p += 2 + n
        if m == 0xDA:
            return p


def main():
    out, names, seed = {}, [], 0
    for mname, sub in MODES:
        for k, (w, h) in enumerate(SIZES):
            q = QUALITIES[(k + len(names)) % 4]
            names.append("%s_%dx%d_q%d" % (mname, w, h, q))
            out["a%d_jpeg" % (len(names) - 1)] = encode(synthetic(h, w, seed), sub, quality=q)
            seed += 1
        for label, kw in (("optimize", dict(quality=75, optimize=True)), ("rst_rows1", dict(quality=95, restart_marker_rows=1)),
                          ("rst_blocks3", dict(quality=30, restart_marker_blocks=3))):
            names.append("%s_65x47_%s" % (mname, label))
            out["a%d_jpeg" % (len(names) - 1)] = encode(synthetic(47, 65, seed), sub, **kw)
            seed += 1
    for i in range(len(names)):
        out["a%d_rgb" % i] = decode(out["a%d_jpeg" % i])
        out["a%d_jpeg" % i] = np.frombuffer(out["a%d_jpeg" % i], np.uint8)
    out["a_names"] = np.asarray(names)

    base = synthetic(47, 65, 1000)
    rej = []
    rej.append(("progressive", encode(base, 2, quality=75, progressive=True), EPROGRESSIVE))
    b = io.BytesIO()
    Image.fromarray(np.concatenate([base, base[:, :, :1]], 2), mode="CMYK").save(b, format="JPEG", quality=75)
    rej.append(("cmyk", b.getvalue(), ECOMPONENTS))
    good = encode(base, 2, quality=75)
    s = scan_start(good)
    rej.append(("cut_mid_scan", good[: s + (len(good) - s) // 2], ETRUNCATED))
    noise = bytearray(np.random.RandomState(7).randint(0, 256, 64).astype(np.uint8).tobytes())
    noise[0] = 0x3C                                                         # whatever follows SOI must start with FF: this does not
    rej.append(("noise_after_soi", b"\xff\xd8" + bytes(noise), ENOTJPEG))
    huge = bytearray(good)
    p = 2
    while huge[p + 1] != 0xC0:
        p += 2 + ((huge[p + 2] << 8) | huge[p + 3])
    huge[p + 5: p + 9] = b"\xff\xff\xff\xff"                                # SOF0: height, width = 65535
    rej.append(("header_65535x65535", bytes(huge), ETOOLARGE))
    for i, (_, data, _) in enumerate(rej):
        out["r%d_jpeg" % i] = np.frombuffer(data, np.uint8)
    out["r_names"] = np.asarray([r[0] for r in rej])
    out["r_reasons"] = np.asarray([r[2] for r in rej], np.int32)
    path = os.path.join(HERE, "jpeg_golden.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes,", len(names), "accepted,", len(rej), "refused")


if __name__ == "__main__":
    main()
