"""Helpers and images of the tests of the JPEG encoder's device Huffman stage (tests/test_jpeg_encode_huffman_cpu.py,
tests/test_jpeg_encode_huffman_gpu.py): descriptors, the host pixel stage, the host Huffman stage (the oracle), the emulation of the device
stage, a plain-Python bit counter for the cases that are chosen by the scan's length, and the images.  Everything from fixed seeds."""
import ctypes
import struct

import numpy as np

import jpeg_encode_cases as C

ZIG_COL_MAJOR = [0, 8, 1, 2, 9, 16, 24, 17, 10, 3, 4, 11, 18, 25, 32, 40, 33, 26, 19, 12, 5, 6, 13, 20, 27, 34, 41, 48, 56, 49, 42, 35, 28,
                 21, 14, 7, 15, 22, 29, 36, 43, 50, 57, 58, 51, 44, 37, 30, 23, 31, 38, 45, 52, 59, 60, 53, 46, 39, 47, 54, 61, 62, 55, 63]
GUARD = 0xC3
PAD0_SEED, PAD1_SEED = 3, 1                   # 16x16 noise, 4:2:0, quality 75: the unstuffed scan ends on a byte boundary | one bit past one


def vp(a):
    return ctypes.c_void_p(a.ctypes.data)


def prepare(L, shapes, mode, quality, arrays=None):
    """descriptors and totals for images of `shapes` [(h, w)]; arrays: the host images behind them (None: srcs = NULL)."""
    from dan_amd._lib import JpegEncDesc
    B = len(shapes)
    descs = (JpegEncDesc * B)()
    widths = (ctypes.c_int32 * B)(*[s[1] for s in shapes])
    heights = (ctypes.c_int32 * B)(*[s[0] for s in shapes])
    srcs = (ctypes.c_void_p * B)(*[a.ctypes.data for a in arrays]) if arrays is not None else None
    totals = (ctypes.c_int64 * 3)()
    assert L.danhip_jpeg_encode_prepare(widths, heights, srcs, B, mode, quality, descs, totals) == 0, L.danhip_last_error()
    return descs, totals


def pixels_host(L, arrays, mode, quality):
    descs, totals = prepare(L, [a.shape[:2] for a in arrays], mode, quality, arrays)
    coef = np.zeros(totals[0], np.int16)
    assert L.danhip_jpeg_encode_pixels_host(descs, len(arrays), vp(coef), totals[0]) == 0, L.danhip_last_error()
    return coef, descs, totals


def host_entropy(L, coef, descs, totals):
    """The oracle: danhip_jpeg_encode_entropy_batch -> list of files."""
    B = len(descs)
    out = np.empty(totals[2], np.uint8)
    sizes = (ctypes.c_int64 * B)()
    assert L.danhip_jpeg_encode_entropy_batch(vp(coef), coef.size, descs, B, 2, vp(out), totals[2], sizes) == 0, L.danhip_last_error()
    return [out[descs[i].file_offset:descs[i].file_offset + sizes[i]].tobytes() for i in range(B)]


def staging(L, descs, totals):
    """(staging buffer as a 16-byte aligned uint8 array, prepare status)."""
    B = len(descs)
    n = L.danhip_jpeg_encode_scan_staging_bytes(B)
    assert n > 0
    raw = np.zeros(n + 16, np.uint8)
    at = (-raw.ctypes.data) % 16
    st = raw[at:at + n]
    status = (ctypes.c_int32 * B)()
    assert L.danhip_jpeg_encode_scan_prepare(descs, B, totals[0], totals[2], vp(st), n, status) == 0, L.danhip_last_error()
    return st, list(status)


def emulate(L, coef, descs, totals):
    """The device stage's phases on the host -> (files buffer pre-filled with GUARD, sizes, status, range_errors)."""
    B = len(descs)
    st, pstatus = staging(L, descs, totals)
    assert pstatus == [0] * B
    assert L.danhip_jpeg_encode_scan_workspace_bytes(vp(st)) > 0
    out = np.full(totals[2], GUARD, np.uint8)
    sizes = (ctypes.c_int64 * B)()
    status = (ctypes.c_int32 * B)()
    errors = ctypes.c_int64(-1)
    rc = L.danhip_jpeg_encode_entropy_emulate_batch(vp(st), st.size, descs, B, vp(coef), coef.size, vp(out), totals[2], sizes, status,
                                                    ctypes.byref(errors))
    assert rc == 0, L.danhip_last_error()
    return out, list(sizes), list(status), errors.value


def files_of(out, descs, sizes):
    return [out[descs[i].file_offset:descs[i].file_offset + sizes[i]].tobytes() for i in range(len(descs))]


def tables(st):
    """The four code / length tables of a staging buffer: [t][symbol] -> (code, length)."""
    off_tabs = struct.unpack_from("<q", st.tobytes(), 32 + 8)[0]
    words = np.frombuffer(st.tobytes(), np.uint32, 1024, off_tabs)
    return [[(int(w) & 0xffff, int(w) >> 16) for w in words[t * 256:(t + 1) * 256]] for t in range(4)]


def scan_blocks(d):
    """The blocks of an image in scan order: (component, first element in the image's coefficient slot)."""
    hs = 2 if d.mode == 3 else 1
    mx_n, my_n, bw0 = d.blocks_w[1], d.blocks_h[1], d.blocks_w[0]
    p1 = d.blocks_w[0] * d.blocks_h[0] * 64
    p2 = p1 + mx_n * my_n * 64
    for my in range(my_n):
        for mx in range(mx_n):
            for v in range(hs):
                for h in range(hs):
                    yield 0, ((my * hs + v) * bw0 + mx * hs + h) * 64
            yield 1, p1 + (my * mx_n + mx) * 64
            yield 2, p2 + (my * mx_n + mx) * 64


def scan_bits(tabs, coef, d):
    """(bits of the image's unstuffed scan before padding, longest zero run that a non-zero value follows), counted as T.81 F.1.2 says."""
    slot = coef[d.coef_offset:d.coef_offset + d.coef_count].astype(np.int64)
    last = [0, 0, 0]
    bits, longest = 0, 0
    for c, el in scan_blocks(d):
        blk = slot[el:el + 64]
        diff = int(blk[0]) - last[c]
        last[c] = int(blk[0])
        nb = abs(diff).bit_length()
        bits += tabs[0 if c == 0 else 2][nb][1] + nb
        ac = tabs[1 if c == 0 else 3]
        run = 0
        for k in range(1, 64):
            v = int(blk[ZIG_COL_MAJOR[k]])
            if v == 0:
                run += 1
                continue
            longest = max(longest, run)
            while run > 15:
                bits += ac[0xf0][1]
                run -= 16
            nb = abs(v).bit_length()
            bits += ac[(run << 4) | nb][1] + nb
            run = 0
        if run:
            bits += ac[0][1]
    return bits, longest


def noise(h, w, seed):
    return np.ascontiguousarray(np.random.RandomState(seed).randint(0, 256, (h, w, 3)).astype(np.uint8))


def harsh_noise(h, w, seed):
    """Noise with a patch of black and white pixels and a step edge: AC values of 10 bits at quality 100.  At least 40 x 40."""
    r = np.random.RandomState(seed)
    a = r.randint(0, 256, (h, w, 3)).astype(np.uint8)
    a[8:24, 8:40] = (r.randint(0, 2, (16, 32, 1)) * 255).astype(np.uint8)
    a[24:40, 8:12] = 0
    a[24:40, 12:16] = 255
    return np.ascontiguousarray(a)


def flat_grey(h, w):
    return np.full((h, w, 3), 128, np.uint8)


def sparse_high_frequency(h=32, w=48):
    """Grey, flat but for the DCT's highest basis function in every third block: the energy sits at the far end of the zig-zag order."""
    a = np.full((h, w), 128, np.int64)
    k = np.cos((2 * np.arange(8) + 1) * 7 * np.pi / 16)
    tile = np.rint(128 + 120 * np.outer(k, k)).astype(np.int64)
    n = 0
    for by in range(h // 8):
        for bx in range(w // 8):
            if n % 3 == 0:
                a[by * 8:by * 8 + 8, bx * 8:bx * 8 + 8] = tile
            n += 1
    return np.ascontiguousarray(np.stack([a] * 3, -1).astype(np.uint8))


def pillow(a, quality, sub):
    return C.pillow_bytes(a, quality, sub)
