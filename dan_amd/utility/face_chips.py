"""Face chips: every detection of every image of a list cropped and resized to size x size on the device (danhip_face_chips_u8 and
danhip_face_chips_u8_ex, csrc/face_chips_exact.hip): two launches whatever the number of images and detections, nothing read back.

    chips, chip_src, count = extract(images, dets, num, size=112)
    chips, chip_src, count = extract(images, dets, num, size=112, filter="area", pad=True)

images: list of uint8 [H_i, W_i, 3] device tensors (separate tensors or views into one buffer, at any byte offset; rows may be further
apart than 3 * W_i bytes); dets fp32 [B, R, 5] rows (x1, y1, x2, y2, score) and num int32 [B]: what eval_dan.detect_image_list returns.
chips uint8 [max_chips, size, size, 3], chip_src int32 [max_chips, 6] = (image, row, xc1, yc1, xc2, yc2), count int32 [1]: the number of
rows that give a chip, in (image, row) order; the first min(count, max_chips) rows of chips / chip_src are written.

The rectangle rule is the project's own (include/danhip.h, "Face chips"); `rule` restates it in Python integers.  By default the rectangle
is clipped to the image and the chip is OpenCV's INTER_LINEAR resize of it (oracle/evalpipe.py:cv2_resize_linear_u8), bit for bit.
pad=True keeps the rectangle whole - square and centred on the box - and reads `fill` where it leaves the image (chip_src then carries the
unclipped corners).  filter="area" is an antialiased downscale by the project's own integer rule, restated by `area_weights`: a box filter
on an axis that shrinks, exact half-pixel linear interpolation on one that does not, one rounding.  Either of the two takes
danhip_face_chips_u8_ex, which gives no chip for a rectangle with a side above MAX_SIDE.  Out of scope: alignment by landmarks (the
detectors predict none), border modes other than a constant, chips during training."""
import ctypes
import math

import numpy as np
import torch

from .._lib import ResizeItem, call, ptr, stream

MAX_SIZE = 1024            # danhip_face_chips_u8: 1 <= S <= 1024
MAX_MARGIN_PM = 4000       # 0 <= margin_pm <= 4000
MAX_SIDE = 32768           # DANHIP_FACE_CHIPS_MAX_SIDE: danhip_face_chips_u8_ex gives no chip for a longer side
FILTERS = {"linear": 0, "area": 1}      # DANHIP_FACE_CHIPS_LINEAR / DANHIP_FACE_CHIPS_AREA
_CLAMP = 1 << 30


def margin_per_mille(margin):
    """The float margin (a fraction of the box side added on EACH side) as the integer the rule computes with."""
    pm = int(round(float(margin) * 1000)) if math.isfinite(margin) else -1
    if not 0 <= pm <= MAX_MARGIN_PM:
        raise ValueError("margin %r outside 0 .. %g" % (margin, MAX_MARGIN_PM / 1000.0))
    return pm


def check_size(size):
    if int(size) != size or not 1 <= int(size) <= MAX_SIZE:
        raise ValueError("size %r outside 1 .. %d" % (size, MAX_SIZE))
    return int(size)


def check_filter(filter):
    if filter not in FILTERS:
        raise ValueError("filter %r is not one of %s" % (filter, ", ".join(sorted(FILTERS))))
    return FILTERS[filter]


def check_fill(fill):
    fill = tuple(fill)
    if len(fill) != 3 or any(int(v) != v or not 0 <= int(v) <= 255 for v in fill):
        raise ValueError("fill %r is not three values of 0 .. 255" % (fill,))
    return tuple(int(v) for v in fill)


def rule(dets_row, H, W, margin_pm=0, square=True, pad=False, cap=None):
    """The rectangle of one detection row (x1, y1, x2, y2, ...) in an H x W image -> (xc1, yc1, xc2, yc2), inclusive, or None.  Integers only
    after the corners are read; the score threshold and num[i] are the caller's.  pad: the rectangle is not clipped to the image (one that
    misses the image altogether is still None).  cap: None for a side longer than it (MAX_SIDE is danhip_face_chips_u8_ex's; the default
    None is danhip_face_chips_u8, which has no cap); the side is that of the rectangle returned."""
    c = []
    for v in dets_row[:4]:
        v = float(np.float32(v))
        if not math.isfinite(v):
            return None
        c.append(int(min(max(v, -float(_CLAMP)), float(_CLAMP))))         # toward zero
    x1, y1, x2, y2 = c
    w, h = x2 - x1 + 1, y2 - y1 + 1
    if w < 1 or h < 1:
        return None
    mx, my = w * margin_pm // 1000, h * margin_pm // 1000
    x1, x2, y1, y2 = x1 - mx, x2 + mx, y1 - my, y2 + my
    w, h = w + 2 * mx, h + 2 * my
    if square:
        s = max(w, h)
        x1 -= (s - w) // 2
        x2 = x1 + s - 1
        y1 -= (s - h) // 2
        y2 = y1 + s - 1
    if x2 < 0 or y2 < 0 or x1 > W - 1 or y1 > H - 1:
        return None
    if not pad:
        x1, y1, x2, y2 = max(x1, 0), max(y1, 0), min(x2, W - 1), min(y2, H - 1)
    if cap is not None and (x2 - x1 + 1 > cap or y2 - y1 + 1 > cap):
        return None
    return x1, y1, x2, y2


def area_weights(n, S, j):
    """One axis of filter="area": n source positions resampled to S outputs -> (indices, weights, D) of output j: the source positions
    with a nonzero weight, ascending, their integer weights, and the divisor D the weights sum to.
    n > S: a box filter, D = n; position i covers [i * S, (i + 1) * S) and output j covers [j * n, (j + 1) * n): the weight is the overlap.
    n <= S: half-pixel linear interpolation in exact integers, D = 2 * S; t = (2 * j + 1) * n - S, i0 = t // (2 * S), f = t - 2 * S * i0:
    2 * S - f on clamp(i0) and f on clamp(i0 + 1), clamped to 0 .. n - 1 (two taps clamped onto one position are returned as one)."""
    n, S, j = int(n), int(S), int(j)
    assert n >= 1 and S >= 1 and 0 <= j < S
    taps = {}
    if n > S:
        for i in range(j * n // S, ((j + 1) * n - 1) // S + 1):
            taps[i] = min((j + 1) * n, (i + 1) * S) - max(j * n, i * S)
        D = n
    else:
        t = (2 * j + 1) * n - S
        i0 = t // (2 * S)                                                  # Python's //: toward minus infinity
        f = t - 2 * S * i0
        for i, w in ((i0, 2 * S - f), (i0 + 1, f)):
            i = min(max(i, 0), n - 1)
            taps[i] = taps.get(i, 0) + w
        D = 2 * S
    indices = sorted(i for i, w in taps.items() if w > 0)
    return indices, [taps[i] for i in indices], D


class FaceChips(tuple):
    """(chips, chip_src, count), device tensors; to_host() is the one deliberate synchronisation."""

    def __new__(cls, chips, chip_src, count, n_images):
        self = tuple.__new__(cls, (chips, chip_src, count))
        self.n_images = n_images
        return self

    chips = property(lambda self: self[0])
    chip_src = property(lambda self: self[1])
    count = property(lambda self: self[2])

    def to_host(self):
        """-> per image a list of (row, (xc1, yc1, xc2, yc2), chip ndarray uint8 [size, size, 3]), rows ascending: the chips that were
        written (the first max_chips of `count`)."""
        n = min(int(self.count.item()), int(self.chips.shape[0]))
        src, chips = self.chip_src[:n].cpu().numpy(), self.chips[:n].cpu().numpy()
        out = [[] for _ in range(self.n_images)]
        for k in range(n):
            out[int(src[k, 0])].append((int(src[k, 1]), tuple(int(v) for v in src[k, 2:6]), chips[k]))
        return out


def extract(images, dets, num, size=112, margin=0.0, square=True, score_threshold=0.0, max_chips=None, out=None, *, filter="linear", pad=False,
            fill=(0, 0, 0)):
    """-> FaceChips (chips, chip_src, count), device tensors; nothing is synchronised.  margin: the fraction of the box side added on each
    side, converted to per mille once, here.  max_chips=None: len(images) * rows_per_image, room for every row.  out: (chips, chip_src,
    count) tensors of a previous call (or the caller's own, of max_chips rows) to write into instead of new ones.  filter: "linear" or
    "area"; pad: keep the rectangle whole and read `fill` (three values of 0 .. 255) outside the image.  filter="linear", pad=False is
    danhip_face_chips_u8; anything else danhip_face_chips_u8_ex."""
    size, pm = check_size(size), margin_per_mille(margin)
    filter_id, fill = check_filter(filter), check_fill(fill)
    images = list(images)
    B = len(images)
    device = dets.device
    assert dets.dtype == torch.float32 and dets.dim() == 3 and dets.shape[0] == B and dets.shape[2] == 5 and dets.is_contiguous()
    assert num.dtype == torch.int32 and tuple(num.shape) == (B,) and num.is_contiguous() and num.device == device
    R = int(dets.shape[1])
    if max_chips is None:
        max_chips = B * R
    if max_chips < 0:
        raise ValueError("max_chips %r is negative" % (max_chips,))
    if out is None:
        chips = torch.empty((max_chips, size, size, 3), dtype=torch.uint8, device=device)
        chip_src = torch.empty((max_chips, 6), dtype=torch.int32, device=device)
        count = torch.empty((1,), dtype=torch.int32, device=device)
    else:
        chips, chip_src, count = out
        assert chips.dtype == torch.uint8 and tuple(chips.shape) == (max_chips, size, size, 3) and chips.is_contiguous() and chips.device == device
        assert chip_src.dtype == torch.int32 and tuple(chip_src.shape) == (max_chips, 6) and chip_src.is_contiguous() and chip_src.device == device
        assert count.dtype == torch.int32 and count.numel() == 1 and count.device == device
    table = staging = None
    base = src_bytes = 0
    if B:
        for im in images:
            assert im.dtype == torch.uint8 and im.dim() == 3 and im.shape[2] == 3 and im.device == device
            assert im.stride(2) == 1 and im.stride(1) == 3 and im.stride(0) >= 3 * im.shape[1], "rows of packed RGB pixels, `pitch` bytes apart"
        base = min(im.data_ptr() for im in images)                # "one source buffer": the span of the images' addresses
        src_bytes = max(im.data_ptr() + (im.shape[0] - 1) * im.stride(0) + 3 * im.shape[1] for im in images) - base
        nitem = ctypes.sizeof(ResizeItem)
        staging = torch.empty(B * nitem, dtype=torch.uint8, pin_memory=True)
        nt = ctypes.c_int32(0)
        for i, im in enumerate(images):                           # the identity item: source offset, size and pitch are what the chips read
            H, W = int(im.shape[0]), int(im.shape[1])
            call("danhip_resize_item_init", ctypes.c_void_p(staging.data_ptr() + i * nitem), im.data_ptr() - base, H, W, int(im.stride(0)), 0, H, W,
                 1.0, 1.0, 0, 0, ctypes.byref(nt))
        table = staging.to(device, non_blocking=True)
    args = (None if staging is None else ctypes.c_void_p(staging.data_ptr()), ptr(table), B, ctypes.c_void_p(base), src_bytes, ptr(dets), ptr(num),
            R, size, pm, int(bool(square)), float(score_threshold), ptr(chips), ptr(chip_src), ptr(count), int(max_chips), None, 0, stream())
    if filter_id == 0 and not pad:
        call("danhip_face_chips_u8", *args)
    else:
        call("danhip_face_chips_u8_ex", *(args + (filter_id, int(bool(pad)), (ctypes.c_uint8 * 3)(*fill))))
    return FaceChips(chips, chip_src, count, B)
