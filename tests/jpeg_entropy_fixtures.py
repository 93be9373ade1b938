"""The streams of tests/golden/jpeg_entropy_golden.npz (written by tests/golden/make_jpeg_entropy_golden.py) as the Huffman-stage tests use them,
the scan walk those tests share, and the corrupted scans: the file holds the 45 KB stream they are made from once, and for each corruption
its recipe (positions, values, a seed) with the outcome recorded from the host entropy stage - four more copies would not fit the file."""
import ctypes
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
PATH = os.path.join(HERE, "golden", "jpeg_entropy_golden.npz")


def header_constants():
    import re
    text = open(os.path.join(os.path.dirname(HERE), "include", "danhip.h")).read()
    return {k: int(re.search(r"#define\s+%s\s+(-?\d+)" % k, text).group(1))
            for k in ("DANHIP_JPEG_SUBSEQ_BYTES", "DANHIP_JPEG_SUBSEQ_PER_GROUP", "DANHIP_JPEG_SYNC_ROUNDS")}


def scan_start(data):
    """Offset of the first entropy-coded byte (after the SOS segment)."""
    p = 2
    while True:
        assert data[p] == 0xFF
        m, n = data[p + 1], (data[p + 2] << 8) | data[p + 3]
        p += 2 + n
        if m == 0xDA:
            return p


def scan_end(data):
    """Offset of the marker that ends the scan: the first FF that neither 00, FF nor an RSTn follows."""
    p = scan_start(data)
    while p + 1 < len(data):
        if data[p] == 0xFF and data[p + 1] not in (0x00, 0xFF) and not 0xD0 <= data[p + 1] <= 0xD7:
            return p
        p += 1
    return len(data)


def straddling_stuffed_pairs(data, subseq):
    """FF 00 pairs whose FF is the last byte of a subsequence of a stream WITHOUT restart markers (one segment from the scan's start)."""
    s, e = scan_start(data), scan_end(data)
    return [p for p in range(s, e - 1) if data[p] == 0xFF and data[p + 1] == 0x00 and (p + 1 - s) % subseq == 0]


def corrupt(base, kind, params):
    """The corrupted stream of one recipe."""
    s, e = scan_start(base), scan_end(base)
    b = bytearray(base)
    if kind == "flip3":                                   # params: position, value, position, value, position, value
        for pos, val in zip(params[0::2], params[1::2]):
            b[s + int(pos)] = int(val)
        return bytes(b)
    if kind == "ff_run":                                  # params: position, count of FF FF pairs
        return bytes(b[:s + int(params[0])] + b"\xff\xff" * int(params[1]) + b[s + int(params[0]):])
    if kind == "cut_odd":                                 # params: bytes of scan kept (odd)
        return bytes(b[:s + int(params[0])])
    if kind == "noise":                                   # params: seed
        noise = np.random.RandomState(int(params[0])).randint(0, 256, e - s).astype(np.uint8).tobytes()
        return bytes(b[:s]) + noise + bytes(b[e:])
    raise ValueError(kind)


def load():
    """-> (good, bad): good = [(name, stream)], bad = [(name, stream, host outcome)] with outcome 0 = decodes, else the reason code."""
    z = np.load(PATH)
    good = [(str(n), z["g%d_jpeg" % i].tobytes()) for i, n in enumerate(z["g_names"])]
    base = z["c_base_jpeg"].tobytes()
    bad = [(str(k), corrupt(base, str(k), z["c%d_params" % i]), int(z["c_outcomes"][i])) for i, k in enumerate(z["c_kinds"])]
    return good, bad


def host_decode(L, JpegDesc, JpegInfo, datas, fill=0):
    """danhip_jpeg_entropy_decode_batch -> (coef, descs, statuses)"""
    B = len(datas)
    capacity = 0
    for d in datas:
        info = JpegInfo()
        L.danhip_jpeg_inspect(d, len(d), ctypes.byref(info))
        capacity += info.coef_count
    coef = np.full(max(capacity, 1), fill, dtype=np.int16)
    descs = (JpegDesc * B)()
    status = (ctypes.c_int32 * B)()
    ptrs = (ctypes.c_char_p * B)(*datas)
    sizes = (ctypes.c_int64 * B)(*[len(d) for d in datas])
    rc = L.danhip_jpeg_entropy_decode_batch(ptrs, sizes, B, 1, coef.ctypes.data_as(ctypes.c_void_p), capacity, descs, status)
    assert rc == 0, L.danhip_last_error()
    return coef, descs, list(status)
