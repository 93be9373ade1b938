"""The case matrix of the JPEG encoder tests (tests/test_jpeg_encode_cpu.py, tests/test_jpeg_encode_gpu.py) and of the fixture
tests/golden/jpeg_encode_golden.npz: sizes that cover no full block, a full MCU, a partial MCU in each direction and in both, and several
MCU rows; both chroma modes; four qualities; five contents.  Everything is generated from fixed seeds."""
import ctypes
import os

import numpy as np

SIZES = [(1, 1), (8, 8), (7, 9), (16, 16), (17, 33), (24, 40), (100, 131)]           # H x W
MODES = [("4:2:0", 3), ("4:4:4", 1)]                                                  # Pillow's subsampling, DANHIP_JPEG_420 / _444
QUALITIES = [10, 75, 95, 100]
CONTENTS = ["zero", "full", "ramp", "noise", "smooth"]
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "jpeg_encode_golden.npz")


def image(h, w, content):
    yy, xx = np.mgrid[0:h, 0:w]
    if content == "zero":
        a = np.zeros((h, w, 3), np.uint8)
    elif content == "full":
        a = np.full((h, w, 3), 255, np.uint8)
    elif content == "ramp":                                       # horizontal
        a = np.stack([xx * 255 // max(w - 1, 1)] * 3, -1).astype(np.uint8)
    elif content == "noise":                                      # long codes, FF stuffing
        a = np.random.RandomState(1000 * h + w).randint(0, 256, (h, w, 3)).astype(np.uint8)
    else:
        a = np.stack([127 + 100 * np.sin(xx / 9.0 + yy / 7.0), 127 + 90 * np.cos(xx / 11.0), 127 + 80 * np.sin(yy / 5.0)], -1).astype(np.uint8)
    return np.ascontiguousarray(a)


def cases():
    """[(key, h, w, content, subsampling, mode, quality)] - 280 of them."""
    return [("%dx%d_%s_%s_q%d" % (h, w, c, sub.replace(":", ""), q), h, w, c, sub, mode, q)
            for (h, w) in SIZES for c in CONTENTS for sub, mode in MODES for q in QUALITIES]


def pillow_bytes(a, quality, subsampling):
    import io
    from PIL import Image
    b = io.BytesIO()
    Image.fromarray(a).save(b, "JPEG", quality=quality, subsampling=subsampling)
    return b.getvalue()


def load_golden():
    """{key: expected bytes}, {(h, w, content): input array} of the committed fixture."""
    z = np.load(GOLDEN)
    keys = [str(k) for k in z["keys"]]
    off = z["offsets"]
    blob = z["blob"].tobytes()
    files = {k: blob[int(off[i]):int(off[i + 1])] for i, k in enumerate(keys)}
    inputs = {}
    ioff = z["input_offsets"]
    iblob = z["input_blob"]
    for i, (h, w, c) in enumerate((h, w, c) for (h, w) in SIZES for c in CONTENTS):
        inputs[(h, w, c)] = np.ascontiguousarray(iblob[int(ioff[i]):int(ioff[i + 1])].reshape(h, w, 3))
    return files, inputs


def host_lib():
    """The built library with the encoder's host prototypes bound (no GPU is touched)."""
    from dan_amd import _lib
    return _lib.lib()


def encode_host(L, a, quality, mode):
    h, w = a.shape[:2]
    cap = L.danhip_jpeg_encode_file_bound(w, h, mode)
    assert cap > 0
    out = np.empty(cap, np.uint8)
    n = ctypes.c_int64(0)
    rc = L.danhip_jpeg_encode_host(ctypes.c_void_p(a.ctypes.data), w, h, mode, quality, ctypes.c_void_p(out.ctypes.data), cap, ctypes.byref(n))
    assert rc == 0, L.danhip_last_error().decode()
    return out[:n.value].tobytes()
