"""The device half of the JPEG decoder restated in numpy, from the library's own coefficients and descriptors to RGB:
dequantise -> libjpeg's JDCT_ISLOW inverse DCT -> fancy (triangle) chroma upsampling -> 16-bit fixed-point YCbCr -> RGB.

Every step is written as libjpeg states it, in 64-bit integers (so nothing can wrap), vectorised over blocks / pixels only.  It is the
reference the CPU tests pin against Pillow (tests/test_jpeg_cpu.py) and the text the kernels of dan_amd/csrc/jpeg_exact.hip restate.
Layouts are those of include/danhip.h: a component's blocks in raster order of its block grid, a block's 64 values column-major."""
import ctypes

import numpy as np

GREY, S444, S422, S420 = 0, 1, 2, 3
CONST_BITS, PASS1_BITS = 13, 2


def descale(x, n):
    return (x + (1 << (n - 1))) >> n


def idct_islow_1d(x, shift):
    """One 8-point pass of jidctint.c: x = the 8 inputs (arrays), returns the 8 descaled outputs."""
    z1 = (x[2] + x[6]) * 4433
    e2 = z1 + x[6] * (-15137)
    e3 = z1 + x[2] * 6270
    e0 = (x[0] + x[4]) << CONST_BITS
    e1 = (x[0] - x[4]) << CONST_BITS
    t10, t13, t11, t12 = e0 + e3, e0 - e3, e1 + e2, e1 - e2
    o0, o1, o2, o3 = x[7], x[5], x[3], x[1]
    z1, z2, z3, z4 = o0 + o3, o1 + o2, o0 + o2, o1 + o3
    z5 = (z3 + z4) * 9633
    o0, o1, o2, o3 = o0 * 2446, o1 * 16819, o2 * 25172, o3 * 12299
    z1, z2, z3, z4 = z1 * (-7373), z2 * (-20995), z3 * (-16069) + z5, z4 * (-3196) + z5
    o0, o1, o2, o3 = o0 + z1 + z3, o1 + z2 + z4, o2 + z2 + z3, o3 + z1 + z4
    return [descale(v, shift) for v in (t10 + o3, t11 + o2, t12 + o1, t13 + o0, t13 - o0, t12 - o1, t11 - o2, t10 - o3)]


def component_plane(coef, desc, c):
    """uint8 [blocks_h * 8, blocks_w * 8] of component c (block padding included)."""
    bw, bh = desc.blocks_w[c], desc.blocks_h[c]
    first = desc.coef_offset + 64 * sum(desc.blocks_w[k] * desc.blocks_h[k] for k in range(c))
    blk = np.asarray(coef[first:first + 64 * bw * bh], dtype=np.int64).reshape(bw * bh, 8, 8)        # [block, col, row]
    q = np.asarray(list(desc.quant[desc.quant_index[c]]), dtype=np.int64).reshape(8, 8)             # [row, col]
    x = blk.transpose(0, 2, 1) * q                                                                   # [block, row, col]
    ws = np.stack(idct_islow_1d([x[:, r, :] for r in range(8)], CONST_BITS - PASS1_BITS), axis=1)    # pass 1: down the columns
    px = np.stack(idct_islow_1d([ws[:, :, k] for k in range(8)], CONST_BITS + PASS1_BITS + 3), axis=2)   # pass 2: along the rows
    px = np.clip(px + 128, 0, 255)
    return px.reshape(bh, bw, 8, 8).transpose(0, 2, 1, 3).reshape(bh * 8, bw * 8)


def _edge(a, axis):
    """a with its first and last sample along axis repeated once (the component's own edges)."""
    first, last = np.take(a, [0], axis=axis), np.take(a, [-1], axis=axis)
    return np.concatenate([first, a, last], axis=axis)


def upsample_h2v1(comp):
    p = _edge(comp, 1)
    mid, left, right = p[:, 1:-1], p[:, :-2], p[:, 2:]
    out = np.empty((comp.shape[0], 2 * comp.shape[1]), np.int64)
    out[:, 0::2] = (3 * mid + left + 1) >> 2
    out[:, 1::2] = (3 * mid + right + 2) >> 2
    return out


def upsample_h2v2(comp):
    p = _edge(comp, 0)
    near, above, below = p[1:-1], p[:-2], p[2:]
    out = np.empty((2 * comp.shape[0], 2 * comp.shape[1]), np.int64)
    for phase, far in ((0, above), (1, below)):
        s = _edge(3 * near + far, 1)
        mid, left, right = s[:, 1:-1], s[:, :-2], s[:, 2:]
        out[phase::2, 0::2] = (3 * mid + left + 8) >> 4
        out[phase::2, 1::2] = (3 * mid + right + 7) >> 4
    return out


def reconstruct(coef, desc):
    """coef: the int16 buffer of the batch; desc: one danhip_jpeg_desc with status 0.  -> uint8 [H, W, 3]."""
    assert desc.status == 0
    H, W = desc.height, desc.width
    planes = [component_plane(coef, desc, c)[:desc.comp_h[c], :desc.comp_w[c]] for c in range(desc.ncomp)]
    y = planes[0]
    if desc.mode == GREY:
        return np.repeat(y[:, :, None], 3, axis=2).astype(np.uint8)
    if desc.mode in (S422, S420) and desc.comp_w[1] <= 2:
        # jdsample.c picks the triangle filters only for a component more than 2 samples wide; narrower ones are replicated
        planes[1:] = [np.repeat(np.repeat(p, 2, axis=1), 2 if desc.mode == S420 else 1, axis=0) for p in planes[1:]]
    elif desc.mode == S422:
        planes[1:] = [upsample_h2v1(p) for p in planes[1:]]
    elif desc.mode == S420:
        planes[1:] = [upsample_h2v2(p) for p in planes[1:]]
    cb, cr = (p[:H, :W] - 128 for p in planes[1:])
    r = y + ((91881 * cr + 32768) >> 16)
    g = y + ((-22554 * cb - 46802 * cr + 32768) >> 16)
    b = y + ((116130 * cb + 32768) >> 16)
    return np.clip(np.stack([r, g, b], axis=2), 0, 255).astype(np.uint8)


def entropy_decode(L, JpegDesc, datas, threads=1, capacity=None, fill=0):
    """danhip_jpeg_entropy_decode_batch over a list of byte strings -> (coef int16 array, descs, statuses).  L: the loaded library."""
    from dan_amd import _lib
    B = len(datas)
    if capacity is None:
        capacity = 0
        for d in datas:
            info = _lib.JpegInfo()
            L.danhip_jpeg_inspect(d, len(d), ctypes.byref(info))
            capacity += info.coef_count
    coef = np.full(max(capacity, 1), fill, dtype=np.int16)
    descs = (JpegDesc * B)()
    status = (ctypes.c_int32 * B)()
    bufs = [ctypes.create_string_buffer(d, len(d)) for d in datas]
    ptrs = (ctypes.c_void_p * B)(*[ctypes.addressof(b) for b in bufs])
    sizes = (ctypes.c_int64 * B)(*[len(d) for d in datas])
    rc = L.danhip_jpeg_entropy_decode_batch(ptrs, sizes, B, threads, coef.ctypes.data_as(ctypes.c_void_p), capacity, descs, status)
    assert rc == 0, L.danhip_last_error()
    return coef, descs, list(status)
