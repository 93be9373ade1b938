"""Writes tests/golden/jpeg_progressive_golden.npz: small progressive JPEG streams with Pillow's decoded RGB (the definition of right for
JpegDecoder(progressive=True)), and streams the validator must refuse with the flag set, each with the reason code it must give.

    python tests/golden/make_jpeg_progressive_golden.py

Needs Pillow (libjpeg-turbo).  Accepted cases, seeded noisy images at quality 75 unless named otherwise (width x height):
grey / 4:4:4 / 4:2:2 / 4:2:0 at 1x1 (one block, all scans) and 17x9 (a partial MCU in both directions); 4:2:0 and 4:2:2 at 56x40 (the
luma grid of a single-component scan is 7 blocks wide, the padded grid 8); 4:2:0 at 33x47 (odd chroma sizes); 4:2:0 at 56x40 with
restart_marker_blocks=3 (RSTn inside EOB runs and single-component scans); 4:2:0 at 56x40 and quality 30 (long EOB runs); a flat 4:2:0
image (one EOB run over most of a scan).
Refused cases are made from the 4:2:0 56x40 stream by byte surgery; the reason each must give is DERIVED here, by scan_script_reason - a
restatement of the rules of include/danhip.h ("Progressive streams") over the markers alone - and not written down by hand.  For the two
incomplete progressions Pillow's pixels are recorded too: the fallback must still return exactly those.
Keys: a<i>_jpeg (uint8 stream), a<i>_rgb (uint8 [H,W,3]), a_names; r<i>_jpeg, r_names, r_reasons; r<i>_rgb where Pillow decodes the stream."""
import io
import os

import numpy as np
from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))
ETRUNCATED, EPROGRESSION = 2, 18
MODES = [("grey", None), ("444", 0), ("422", 1), ("420", 2)]


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
        Image.fromarray(img[:, :, 1]).save(b, format="JPEG", progressive=True, **kw)
    else:
        Image.fromarray(img).save(b, format="JPEG", subsampling=sub, progressive=True, **kw)
    return b.getvalue()


def decode(data):
    return np.asarray(Image.open(io.BytesIO(data)).convert("RGB"), dtype=np.uint8)


def segments(data):
    """[(marker, offset of its FF, offset of the first byte behind the segment and, for SOS, behind its entropy-coded data)] up to EOI or
    the end of the data (a scan cut short ends at len(data))."""
    out, p = [], 2
    while p + 1 < len(data):
        assert data[p] == 0xFF, p
        m = data[p + 1]
        if m == 0xD9:
            out.append((m, p, p + 2))
            break
        q = p + 2 + ((data[p + 2] << 8) | data[p + 3])
        if m == 0xDA:
            while q < len(data) and not (data[q] == 0xFF and q + 1 < len(data) and data[q + 1] != 0 and not 0xD0 <= data[q + 1] <= 0xD7):
                q += 1
        out.append((m, p, q))
        p = q
    return out


def scan_script(data):
    """[(component count, Ss, Se, Ah, Al)] of the SOS segments."""
    return [(data[p + 4], data[p + 5 + 2 * data[p + 4]], data[p + 6 + 2 * data[p + 4]], data[p + 7 + 2 * data[p + 4]] >> 4,
             data[p + 7 + 2 * data[p + 4]] & 15) for m, p, _ in segments(data) if m == 0xDA]


def scan_script_reason(data):
    """0, EPROGRESSION or ETRUNCATED from the markers alone: T.81 G.1.1.1.1 per scan, every coefficient down to Al = 0 at EOI."""
    segs = segments(data)
    sof = [p for m, p, _ in segs if m == 0xC2][0]
    ids = [data[sof + 10 + 3 * c] for c in range(data[sof + 9])]
    bits = {i: [-1] * 64 for i in ids}
    for m, p, _ in segs:
        if m != 0xDA:
            continue
        ns = data[p + 4]
        comps = [data[p + 5 + 2 * i] for i in range(ns)]
        ss, se, ah, al = data[p + 5 + 2 * ns], data[p + 6 + 2 * ns], data[p + 7 + 2 * ns] >> 4, data[p + 7 + 2 * ns] & 15
        if (ss == 0 and se != 0) or (ss > 0 and (ns != 1 or ss > se or se > 63)) or al > 13 or (ah != 0 and al != ah - 1):
            return EPROGRESSION
        for c in comps:
            if ss > 0 and bits[c][0] < 0:
                return EPROGRESSION
            for k in range(ss, se + 1):
                if (ah != 0) if bits[c][k] < 0 else (ah == 0 or ah != bits[c][k]):
                    return EPROGRESSION
                bits[c][k] = al
    if segs[-1][0] != 0xD9:
        return ETRUNCATED
    return 0 if all(v == 0 for b in bits.values() for v in b) else EPROGRESSION


def main():
    cases, seed = [], 0
    for mname, sub in MODES:
        for w, h in ((1, 1), (17, 9)):
            cases.append(("%s_%dx%d_q75" % (mname, w, h), encode(synthetic(h, w, seed), sub, quality=75)))
            seed += 1
    for mname, sub in (("420", 2), ("422", 1)):
        cases.append(("%s_56x40_q75" % mname, encode(synthetic(40, 56, seed), sub, quality=75)))
        seed += 1
    cases.append(("420_33x47_q75", encode(synthetic(47, 33, seed), 2, quality=75)))
    cases.append(("420_56x40_rst_blocks3", encode(synthetic(40, 56, seed + 1), 2, quality=75, restart_marker_blocks=3)))
    cases.append(("420_56x40_q30", encode(synthetic(40, 56, seed + 2), 2, quality=30)))
    cases.append(("420_48x32_flat", encode(np.full((32, 48, 3), (90, 140, 200), np.uint8), 2, quality=75)))
    out = {"a_names": np.asarray([n for n, _ in cases])}
    for i, (name, data) in enumerate(cases):
        assert scan_script_reason(data) == 0, name
        out["a%d_jpeg" % i] = np.frombuffer(data, np.uint8)
        out["a%d_rgb" % i] = decode(data)
    # Pillow's one scan script (colour): all four procedures
    assert scan_script(dict(cases)["420_56x40_q75"]) == [(3, 0, 0, 0, 1), (1, 1, 5, 0, 2), (1, 1, 63, 0, 1), (1, 1, 63, 0, 1), (1, 6, 63, 0, 2),
                                                          (1, 1, 63, 2, 1), (3, 0, 0, 1, 0), (1, 1, 63, 1, 0), (1, 1, 63, 1, 0), (1, 1, 63, 1, 0)]
    assert b"\xff\xdd" in dict(cases)["420_56x40_rst_blocks3"]             # Pillow writes DRI into progressive files

    base = dict(cases)["420_56x40_q75"]
    sos = [(p, q) for m, p, q in segments(base) if m == 0xDA]
    assert len(sos) == 10 and base[-2:] == b"\xff\xd9"

    def cut_before_scan(k):
        """everything up to the end of scan k - 1 (the DHT in front of scan k goes too), then EOI"""
        return base[:sos[k - 1][1]] + b"\xff\xd9"

    rej = [("last_scan_removed", cut_before_scan(9)), ("cut_after_scan5", cut_before_scan(5))]
    bad = bytearray(base)
    p = sos[5][0]                                                           # the Y refinement 2 -> 1: Ah = 3 is not the previous Al
    assert bad[p + 9] == 0x21
    bad[p + 9] = 0x32
    rej.append(("ah_not_previous_al", bytes(bad)))
    bad = bytearray(base)
    p = sos[1][0]                                                           # Y 1..5 rewritten to Ss = 0
    assert bad[p + 7] == 1 and bad[p + 8] == 5
    bad[p + 7] = 0
    rej.append(("ac_scan_ss0", bytes(bad)))
    rej.append(("cut_mid_refinement", base[:(sos[7][0] + 10 + sos[7][1]) // 2]))
    reasons = [scan_script_reason(d) for _, d in rej]
    assert reasons == [EPROGRESSION, EPROGRESSION, EPROGRESSION, EPROGRESSION, ETRUNCATED], reasons
    for i, (name, data) in enumerate(rej):
        out["r%d_jpeg" % i] = np.frombuffer(data, np.uint8)
        if i < 2:
            out["r%d_rgb" % i] = decode(data)
            print(name, "differs from the complete file by up to", int(np.abs(out["r%d_rgb" % i].astype(int) - decode(base).astype(int)).max()), "grey levels")
    out["r_names"] = np.asarray([n for n, _ in rej])
    out["r_reasons"] = np.asarray(reasons, np.int32)
    path = os.path.join(HERE, "jpeg_progressive_golden.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes,", len(cases), "accepted,", len(rej), "refused")


if __name__ == "__main__":
    main()
