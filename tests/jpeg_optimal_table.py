"""Helpers of the tests of the JPEG encoder's optimize=True (tests/test_jpeg_encode_optimize_cpu.py, tests/test_jpeg_encode_optimize_gpu.py):
a plain-Python restatement of the table rule (csrc/jpeg_encode.h dh_jenc_optimal_table), written from the six steps and not from the C
text - nodes are sets of symbols, no chain of `others` - a plain-Python count of the symbols a scan writes, the count sets, the images,
and Pillow with optimize=True."""
import ctypes
import io

import numpy as np

import jpeg_encode_huffman_cases as H

SIZES = [(1, 1), (8, 8), (16, 16), (23, 17), (48, 64)]        # H x W: 17 x 23 has dummy blocks on both edges in 4:2:0
QUALITIES = [1, 25, 75, 95, 100]
MODES = [("4:2:0", 3), ("4:4:4", 1)]


def optimal_table(counts):
    """counts: 256 (or 257, the last ignored) integers -> (bits[17], vals[256], info).  info["longest"]: the longest code before the cut to
    16 bits; info["direct"] / info["walked"]: how often the cut found a code at length i - 2 at once / only further up.  None: a code of
    more than 32 bits (libjpeg fails there)."""
    nodes = {i: (int(counts[i]), [i]) for i in range(256) if counts[i] > 0}
    nodes[256] = (1, [256])                                   # 1 the reserved symbol
    depth = [0] * 257
    while len(nodes) > 1:                                     # 2 the two smallest; of equal counts the larger index first
        low = min(f for f, _ in nodes.values())
        c1 = max(i for i, (f, _) in nodes.items() if f == low)
        rest = {i: v for i, v in nodes.items() if i != c1}
        low2 = min(f for f, _ in rest.values())
        c2 = max(i for i, (f, _) in rest.items() if f == low2)
        members = nodes[c1][1] + nodes[c2][1]
        for m in members:                                     # 3 every symbol under the new node is one level deeper
            depth[m] += 1
        nodes[c1] = (nodes[c1][0] + nodes[c2][0], members)    # the merged node keeps the first one's index
        del nodes[c2]
    if max(depth) > 32:
        return None
    n = [0] * 33
    for d in depth:
        if d:
            n[d] += 1
    info = {"longest": max(depth), "direct": 0, "walked": 0}
    for i in range(32, 16, -1):                               # 4 T.81 figure K.3
        while n[i] > 0:
            j = i - 2
            if n[j]:
                info["direct"] += 1
            else:
                info["walked"] += 1
            while n[j] == 0:
                j -= 1
            n[i] -= 2
            n[i - 1] += 1
            n[j + 1] += 2
            n[j] -= 1
    i = 16
    while n[i] == 0:
        i -= 1
    n[i] -= 1                                                 # 5 the reserved symbol's code
    vals = [s for d in range(1, 33) for s in range(256) if depth[s] == d]      # 6 by the length before the cut, then by value
    return [0] + n[1:17], vals + [0] * (256 - len(vals)), info


def host_table(L, counts):
    """danhip_jpeg_optimal_table_host -> (rc, bits[17], vals[256])"""
    c = (ctypes.c_int32 * 257)(*[int(v) for v in counts][:256], 0)
    bits = (ctypes.c_uint8 * 17)()
    vals = (ctypes.c_uint8 * 256)()
    rc = L.danhip_jpeg_optimal_table_host(c, bits, vals)
    return rc, list(bits), list(vals)


def fib(n):
    a, b = 1, 1
    out = []
    for _ in range(n):
        out.append(a)
        a, b = b, a + b
    return out


def count_sets():
    """{name: 256 counts}.  fibonacci_40: the first 40 Fibonacci numbers over 40 symbols - codes of up to 21 bits before the cut, which then
    finds a code at length i - 2 at once 14 times and only further up 7 times; capped_fibonacci: the same up to the 26th number and that
    value for the rest, where one code of 17 bits is cut."""
    sets = {}
    one = [0] * 256
    one[5] = 1000
    sets["one_symbol"] = one
    two = [0] * 256
    two[3] = two[200] = 17
    sets["two_equal"] = two
    sets["all_equal"] = [9] * 256
    f = fib(40)
    capped = [0] * 256
    plain = [0] * 256
    for k in range(40):
        capped[3 * k + 1] = f[min(k, 25)]
        plain[3 * k + 1] = f[k]
    sets["capped_fibonacci"] = capped
    sets["fibonacci_40"] = plain
    return sets


def symbol_counts(coef, d):
    """The 4 x 257 table of the symbols the image's scan writes (T.81 F.1.2; table order DC luma, AC luma, DC chroma, AC chroma), counted
    block by block in scan order over the image's coefficient slot.  Entry 256 of each row stays 0."""
    slot = coef[d.coef_offset:d.coef_offset + d.coef_count].astype(np.int64)
    counts = np.zeros((4, 257), np.int64)
    last = [0, 0, 0]
    for c, el in H.scan_blocks(d):
        blk = slot[el:el + 64]
        tdc = 0 if c == 0 else 2
        diff = int(blk[0]) - last[c]
        last[c] = int(blk[0])
        counts[tdc, abs(diff).bit_length()] += 1
        run = 0
        for k in range(1, 64):
            v = int(blk[H.ZIG_COL_MAJOR[k]])
            if v == 0:
                run += 1
                continue
            while run > 15:
                counts[tdc + 1, 0xf0] += 1
                run -= 16
            counts[tdc + 1, (run << 4) | abs(v).bit_length()] += 1
            run = 0
        if run:
            counts[tdc + 1, 0] += 1
    return counts


def ramp(h, w):
    yy, xx = np.mgrid[0:h, 0:w]
    return np.ascontiguousarray(np.stack([xx * 255 // max(w - 1, 1), yy * 255 // max(h - 1, 1), (xx + yy) * 255 // max(h + w - 2, 1)], -1).astype(np.uint8))


def images():
    """[(name, array)]: every size as constant grey, a smooth ramp and uniform noise."""
    out = []
    for k, (h, w) in enumerate(SIZES):
        out.append(("grey_%dx%d" % (h, w), H.flat_grey(h, w)))
        out.append(("ramp_%dx%d" % (h, w), ramp(h, w)))
        out.append(("noise_%dx%d" % (h, w), H.noise(h, w, 70 + k)))
    return out


def pillow_optimized(a, quality, sub):
    from PIL import Image
    b = io.BytesIO()
    Image.fromarray(a).save(b, "JPEG", quality=quality, subsampling=sub, optimize=True)
    return b.getvalue()


def markers(data):
    """[(marker byte, payload)] of a file up to and including SOS."""
    out = []
    i = 2
    while i < len(data):
        assert data[i] == 0xff
        n = data[i + 2] * 256 + data[i + 3]
        out.append((data[i + 1], data[i + 4:i + 2 + n]))
        if data[i + 1] == 0xda:
            break
        i += 2 + n
    return out


def host_entropy_optimized(L, coef, descs, totals, threads=2):
    """danhip_jpeg_encode_entropy_batch_ex(DANHIP_JPEG_ENC_OPTIMIZE) -> list of files."""
    B = len(descs)
    out = np.empty(totals[2], np.uint8)
    sizes = (ctypes.c_int64 * B)()
    rc = L.danhip_jpeg_encode_entropy_batch_ex(H.vp(coef), coef.size, descs, B, threads, 1, H.vp(out), totals[2], sizes)
    assert rc == 0, L.danhip_last_error()
    return [out[descs[i].file_offset:descs[i].file_offset + sizes[i]].tobytes() for i in range(B)]
