"""Face redaction: every detection of every image of a list blurred, pixelated or filled on the device (danhip_redact_u8,
csrc/redact_exact.hip), out of place: LAUNCHES launches whatever the number of images, detections and sizes, nothing read back.

    redacted, count = apply(images, dets, num)                                        # a box blur scaled to each face
    redacted, count = apply(images, dets, num, mode="mosaic", shape="ellipse", strength=0.1)
    redacted, count = apply(images, dets, num, mode="fill", fill=(0, 0, 0), score_threshold=0.5)

images: list of uint8 [H_i, W_i, 3] device tensors (separate tensors or views into one buffer, at any byte offset; rows may be further
apart than 3 * W_i bytes); dets fp32 [B, R, 5] rows (x1, y1, x2, y2, score) and num int32 [B]: what eval_dan.detect_image_list returns.
redacted: a list of uint8 [H_i, W_i, 3] device tensors, views into one new buffer; count int32 [1]: the number of rows that were redacted.

The rule is the project's own (include/danhip.h, "Face redaction"); `rule_pixel` and `reference` restate it in Python integers.  A row's
rectangle is face_chips.rule(row, H, W, margin_pm, square=False, pad=False, cap=MAX_SIDE); its extent e = clamp(max(wc, hc) * strength_pm
// 1000, 1, MAX_EXTENT) of the clipped sides; shape "rect" is the rectangle, "ellipse" the pixels with (2*(px-x1)+1-wc)^2 * hc^2 +
(2*(py-y1)+1-hc)^2 * wc^2 <= wc^2 * hc^2.  A pixel inside several rows' shapes belongs to the highest row; a pixel inside none is copied.
Every mode reads the original image only: "fill" writes the colour; "mosaic" the rounded mean (S + A // 2) // A of the cell of side
max(2, e), anchored at the rectangle's corner and clipped to it; "blur" one box filter of radius e whose window is clipped to the IMAGE.
Out of scope: iterated or gaussian blurs, rotated shapes, in-place operation, parity with any OpenCV filter."""
import ctypes
import math

import numpy as np
import torch

from . import face_chips
from .._lib import ResizeItem, call, ptr, stream

MODES = {"blur": 0, "mosaic": 1, "fill": 2}      # DANHIP_REDACT_BLUR / _MOSAIC / _FILL
SHAPES = {"rect": 0, "ellipse": 1}               # DANHIP_REDACT_RECT / _ELLIPSE
MAX_EXTENT = 255           # DANHIP_REDACT_MAX_EXTENT
BAND, STRIP = 64, 256      # DANHIP_REDACT_BAND / DANHIP_REDACT_STRIP: output rows x columns of a blur or fill work item
LAUNCHES = 3               # DANHIP_REDACT_LAUNCHES
MAX_STRENGTH_PM = 1000
MAX_SIDE = face_chips.MAX_SIDE
check_fill = face_chips.check_fill
margin_per_mille = face_chips.margin_per_mille


def strength_per_mille(strength):
    """The float strength (the extent as a fraction of the longer clipped side) as the integer the rule computes with."""
    ok = isinstance(strength, (int, float)) and math.isfinite(strength)
    pm = int(round(float(strength) * 1000)) if ok else -1
    if not 1 <= pm <= MAX_STRENGTH_PM:
        raise ValueError("strength %r outside %g .. 1" % (strength, 1.0 / MAX_STRENGTH_PM))
    return pm


def check_mode(mode):
    if not isinstance(mode, str) or mode not in MODES:
        raise ValueError("mode %r is not one of %s" % (mode, ", ".join(sorted(MODES))))
    return MODES[mode]


def check_shape(shape):
    if not isinstance(shape, str) or shape not in SHAPES:
        raise ValueError("shape %r is not one of %s" % (shape, ", ".join(sorted(SHAPES))))
    return SHAPES[shape]


def check_threshold(score_threshold):
    if not isinstance(score_threshold, (int, float)) or math.isnan(score_threshold):
        raise ValueError("score_threshold %r is not a number" % (score_threshold,))
    return float(score_threshold)


# ------------------------------------------------------------------------------------------------------------ the rule
def extent(wc, hc, strength_pm):
    return min(max(max(wc, hc) * strength_pm // 1000, 1), MAX_EXTENT)


def in_shape(shape, rect, px, py):
    x1, y1, x2, y2 = rect
    if not (x1 <= px <= x2 and y1 <= py <= y2):
        return False
    if shape == "rect":
        return True
    wc, hc = x2 - x1 + 1, y2 - y1 + 1
    return (2 * (px - x1) + 1 - wc) ** 2 * hc * hc + (2 * (py - y1) + 1 - hc) ** 2 * wc * wc <= wc * wc * hc * hc


def valid_rows(rows, H, W, num=None, strength_pm=125, margin_pm=0, score_threshold=0.0):
    """-> [(row index, (x1, y1, x2, y2), e)] of the rows of one image that give a rectangle, ascending."""
    rows = np.asarray(rows, np.float32).reshape(-1, 5)
    out = []
    for r in range(len(rows) if num is None else min(int(num), len(rows))):
        if rows[r, 4] < np.float32(score_threshold):             # an fp32 compare: a NaN score is kept, as the device keeps it
            continue
        rect = face_chips.rule(rows[r], H, W, margin_pm, square=False, pad=False, cap=MAX_SIDE)
        if rect is not None:
            out.append((r, rect, extent(rect[2] - rect[0] + 1, rect[3] - rect[1] + 1, strength_pm)))
    return out


def _value(image, rect, e, mode, fill, px, py):
    H, W = image.shape[:2]
    if mode == "fill":
        return tuple(fill)
    if mode == "mosaic":
        c = max(2, e)
        ax = rect[0] + (px - rect[0]) // c * c
        ay = rect[1] + (py - rect[1]) // c * c
        bx, by = min(ax + c - 1, rect[2]), min(ay + c - 1, rect[3])
    else:
        ax, bx, ay, by = max(px - e, 0), min(px + e, W - 1), max(py - e, 0), min(py + e, H - 1)
    A = (bx - ax + 1) * (by - ay + 1)
    out = []
    for c3 in range(3):
        S = 0
        for y in range(ay, by + 1):
            for x in range(ax, bx + 1):
                S += int(image[y, x, c3])
        out.append((S + A // 2) // A)
    return tuple(out)


def rule_pixel(image, rows, px, py, num=None, mode="blur", shape="rect", strength_pm=125, margin_pm=0, score_threshold=0.0, fill=(0, 0, 0)):
    """The redacted value (r, g, b) of pixel (px, py) of one uint8 [H, W, 3] image with detection rows [R, 5], in Python integers."""
    H, W = image.shape[:2]
    for r, rect, e in reversed(valid_rows(rows, H, W, num, strength_pm, margin_pm, score_threshold)):      # the highest row owns the pixel
        if in_shape(shape, rect, px, py):
            return _value(image, rect, e, mode, fill, px, py)
    return tuple(int(v) for v in image[py, px])


def reference(image, rows, num=None, mode="blur", shape="rect", strength_pm=125, margin_pm=0, score_threshold=0.0, fill=(0, 0, 0)):
    """-> (the redacted image, the number of valid rows): rule_pixel on every pixel a valid row's rectangle holds."""
    image = np.asarray(image)
    H, W = image.shape[:2]
    valid = valid_rows(rows, H, W, num, strength_pm, margin_pm, score_threshold)
    out = image.copy()
    done = np.zeros((H, W), bool)
    for r, rect, e in reversed(valid):
        for py in range(rect[1], rect[3] + 1):
            for px in range(rect[0], rect[2] + 1):
                if not done[py, px] and in_shape(shape, rect, px, py):
                    out[py, px] = _value(image, rect, e, mode, fill, px, py)
                    done[py, px] = True
    return out, len(valid)


# ------------------------------------------------------------------------------------------------------------ the device call
def _items(staging, first, tensors, base):
    nitem = ctypes.sizeof(ResizeItem)
    nt = ctypes.c_int32(0)
    for i, im in enumerate(tensors):                              # the identity item: offset, size and pitch are what the kernels read
        H, W = int(im.shape[0]), int(im.shape[1])
        call("danhip_resize_item_init", ctypes.c_void_p(staging.data_ptr() + (first + i) * nitem), im.data_ptr() - base, H, W, int(im.stride(0)),
             0, H, W, 1.0, 1.0, 0, 0, ctypes.byref(nt))


def _span(tensors):
    base = min(im.data_ptr() for im in tensors)
    return base, max(im.data_ptr() + (im.shape[0] - 1) * im.stride(0) + 3 * im.shape[1] for im in tensors) - base


def apply(images, dets, num, mode="blur", shape="rect", strength=0.125, margin=0.0, score_threshold=0.0, fill=(0, 0, 0), out=None):
    """-> (redacted, count): a list of uint8 [H_i, W_i, 3] device tensors (views into one buffer) and int32 [1], the number of redacted
    rows; nothing is synchronised.  strength: the extent (blur radius, mosaic cell side) as a fraction of the longer side of the clipped
    rectangle, margin: the fraction of the box side added on each side; both become per mille once, here.  out: (redacted, count) of a
    previous call on images of the same sizes (or the caller's own tensors) to write into instead of new ones."""
    mode_id, shape_id = check_mode(mode), check_shape(shape)
    strength_pm, margin_pm = strength_per_mille(strength), margin_per_mille(margin)
    threshold, fill = check_threshold(score_threshold), check_fill(fill)
    images = list(images)
    B = len(images)
    if B == 0:
        return [], (torch.zeros((1,), dtype=torch.int32, device=dets.device) if out is None else out[1])
    device = dets.device
    assert dets.dtype == torch.float32 and dets.dim() == 3 and dets.shape[0] == B and dets.shape[2] == 5 and dets.is_contiguous()
    assert num.dtype == torch.int32 and tuple(num.shape) == (B,) and num.is_contiguous() and num.device == device
    R = int(dets.shape[1])
    for im in images:
        assert im.dtype == torch.uint8 and im.dim() == 3 and im.shape[2] == 3 and im.device == device
        assert im.stride(2) == 1 and im.stride(1) == 3 and im.stride(0) >= 3 * im.shape[1], "rows of packed RGB pixels, `pitch` bytes apart"
    if out is None:
        offsets, size = [], 0
        for im in images:                                         # every image starts at a multiple of 16 bytes
            offsets.append(size)
            size += (int(im.shape[0]) * int(im.shape[1]) * 3 + 15) // 16 * 16
        buffer = torch.empty((size,), dtype=torch.uint8, device=device)
        redacted = [buffer[o:o + int(im.shape[0]) * int(im.shape[1]) * 3].view(int(im.shape[0]), int(im.shape[1]), 3) for o, im in zip(offsets, images)]
        count = torch.empty((1,), dtype=torch.int32, device=device)
    else:
        redacted, count = list(out[0]), out[1]
        assert len(redacted) == B and count.dtype == torch.int32 and count.numel() == 1 and count.device == device
        for o, im in zip(redacted, images):
            assert o.dtype == torch.uint8 and o.shape == im.shape and o.device == device and o.stride(2) == 1 and o.stride(1) == 3
    src_base, src_bytes = _span(images)
    dst_base, dst_bytes = _span(redacted)
    nitem = ctypes.sizeof(ResizeItem)
    staging = torch.empty(2 * B * nitem, dtype=torch.uint8, pin_memory=True)
    _items(staging, 0, images, src_base)
    _items(staging, B, redacted, dst_base)
    table = staging.to(device, non_blocking=True)
    need = ctypes.c_size_t(0)
    call("danhip_redact_workspace", B, R, ctypes.byref(need))
    workspace = torch.empty((need.value,), dtype=torch.uint8, device=device)
    call("danhip_redact_u8", ctypes.c_void_p(staging.data_ptr()), ptr(table), B, ctypes.c_void_p(src_base), src_bytes, ptr(dets), ptr(num), R,
         mode_id, shape_id, strength_pm, margin_pm, threshold, (ctypes.c_uint8 * 3)(*fill), ctypes.c_void_p(staging.data_ptr() + B * nitem),
         ctypes.c_void_p(table.data_ptr() + B * nitem), ctypes.c_void_p(dst_base), dst_bytes, ptr(count), ptr(workspace), need.value, stream())
    return redacted, count
