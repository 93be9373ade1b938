"""utility/draw_toolbox.py of the reference on the device: the detection rectangles of the debug images (eval_dan.py:455-458) and, with
labels=True, their score labels, drawn into uint8 [H,W,3] device tensors by one launch for a whole list of images (csrc/draw_exact.hip).

The reference draws with cv2.rectangle and cv2.putText; OpenCV is not a dependency here and nothing could be compared with it, so the rule
is this project's own, stated once and restated in numpy by draw_reference below:

  * box i is skipped when classes[i] < 1 or one of its coordinates is not finite;
  * corners: x1, y1, x2, y2 = int(bbox[0]), int(bbox[1]), int(bbox[2]), int(bbox[3]), truncated toward zero as draw_toolbox.py:51-52 does
    (bbox[0] / bbox[2] run along the width, as in the reference's call with rows of (xmin, ymin, xmax, ymax); clamped to +-2^30);
  * the box is skipped when x2 < x1 or y2 < y1 (:53-54);
  * with t = thickness, pixel (x, y) of the image is painted colors_tableau[1] = (203, 71, 119) when
        x1 - t//2 <= x <= x2 + t//2  and  y1 - t//2 <= y <= y2 + t//2
    unless it lies in the interior
        x1 + (t+1)//2 <= x <= x2 - (t+1)//2  and  y1 + (t+1)//2 <= y <= y2 - (t+1)//2;
    for t = 2 the band is the two pixels x1 - 1, x1 on the left, x2, x2 + 1 on the right, and likewise above and below.

Without labels there is one colour, so the result does not depend on the order of the boxes.

The score label (labels=True; '%.1f%%' % (score * 100) in white on a filled tab above the box, :57-65).  A skipped box has none.

  * text: v = float32(score) * float32(100), one float32 multiply; tenths = v * 10 rounded to the nearest integer, ties to even, on the
    exact value.  The string is the decimal digits of tenths // 10, '.', the digit tenths % 10, '%': what Python prints for '%.1f%%' % v.
    The label is drawn only when the score is finite and 0 <= tenths <= 9999 (4 to 6 characters); otherwise only the rectangle is drawn.
    -0.0 (and a negative score that rounds to it) prints as 0.0%, where Python would print -0.0%.  The kernel computes v * 10 in double,
    where the product is exact: in float32 it would round a second time and print another digit for some scores;
  * font: the project's own 5 x 7 bitmap glyphs for 0 - 9, '.' and '%' (GLYPHS below; csrc/draw_font.h holds the library's copy), advance
    6 px: n characters have text_w = 6 n - 1; text_h = 7, baseline = 2.  OpenCV's Hershey glyphs and getTextSize are not matched;
  * tab: painted (203, 71, 119) for x1 - t//2 <= x <= x1 + text_w and y1 - text_h - t - baseline <= y <= y1 (the arithmetic of :60-65);
  * text: white (255, 255, 255); the glyph's bottom row is y = y1 - text_h + baseline, the left column of character k is x1 + 6 k;
  * everything is clipped to the image: a label that leaves the top or the right edge is cut, not moved;
  * order: the reference's loop.  Box i paints its band, then its tab, then its text; box i + 1 paints over all of it.  A pixel shows what
    the highest-index box that touches it paints there, and within that box text beats tab beats band."""
import ctypes

import numpy as np
import torch

from .._lib import DrawItem, call, ptr, stream

colors_tableau = [(12, 7, 134), (203, 71, 119)]
_LIMIT = 1 << 30


TEXT_H, BASELINE, ADVANCE = 7, 2, 6
GLYPH_ORDER = "0123456789.%"
GLYPHS = {       # the restatement's own copy of the font; tests/test_draw_labels_cpu.py holds it against danhip_draw_glyph
    "0": (".###.", "#...#", "#..##", "#.#.#", "##..#", "#...#", ".###."),
    "1": ("..#..", ".##..", "..#..", "..#..", "..#..", "..#..", ".###."),
    "2": (".###.", "#...#", "....#", "...#.", "..#..", ".#...", "#####"),
    "3": ("#####", "...#.", "..#..", "...#.", "....#", "#...#", ".###."),
    "4": ("...#.", "..##.", ".#.#.", "#..#.", "#####", "...#.", "...#."),
    "5": ("#####", "#....", "####.", "....#", "....#", "#...#", ".###."),
    "6": ("..##.", ".#...", "#....", "####.", "#...#", "#...#", ".###."),
    "7": ("#####", "....#", "...#.", "..#..", ".#...", ".#...", ".#..."),
    "8": (".###.", "#...#", "#...#", ".###.", "#...#", "#...#", ".###."),
    "9": (".###.", "#...#", "#...#", ".####", "....#", "...#.", ".##.."),
    ".": (".....", ".....", ".....", ".....", ".....", ".##..", ".##.."),
    "%": ("##...", "##..#", "...#.", "..#..", ".#...", "#..##", "...##"),
}


def score_text(score):
    """The label's string by the rule above, "" when no label is drawn: Python's own '%.1f' of the float32 product, its digits read back
    as tenths for the range rule."""
    with np.errstate(over="ignore", invalid="ignore"):
        v = np.float32(score) * np.float32(100)
    if not np.isfinite(v):
        return ""
    s = "%.1f" % v
    tenths = int(s.replace(".", ""))                 # '-0.0' -> 0
    if not 0 <= tenths <= 9999:
        return ""
    return s.lstrip("-") + "%"


def draw_reference(image, classes, bboxes, thickness=2, scores=None):
    """The rule above in numpy, on a copy of a uint8 [H,W,3] array -> the drawn array; with scores, the labels too.  What the kernel is
    tested against.  A loop over the boxes in order, each painting over what is there: painter's order falls out of the loop."""
    out = np.array(image, dtype=np.uint8, copy=True)
    H, W = out.shape[:2]
    t = int(thickness)
    ys, xs = np.mgrid[0:H, 0:W]
    boxes = np.asarray(bboxes, dtype=np.float32).reshape(-1, 4)
    for i in range(boxes.shape[0]):
        if classes[i] < 1 or not np.all(np.isfinite(boxes[i])):
            continue
        x1, y1, x2, y2 = (max(-_LIMIT, min(_LIMIT, int(v))) for v in boxes[i])
        if x2 < x1 or y2 < y1:
            continue
        outer = (xs >= x1 - t // 2) & (xs <= x2 + t // 2) & (ys >= y1 - t // 2) & (ys <= y2 + t // 2)
        h = (t + 1) // 2
        inner = (xs >= x1 + h) & (xs <= x2 - h) & (ys >= y1 + h) & (ys <= y2 - h)
        out[outer & ~inner] = colors_tableau[1]
        text = "" if scores is None else score_text(scores[i])
        if not text:
            continue
        text_w = ADVANCE * len(text) - 1
        out[(xs >= x1 - t // 2) & (xs <= x1 + text_w) & (ys >= y1 - TEXT_H - t - BASELINE) & (ys <= y1)] = colors_tableau[1]
        bottom = y1 - TEXT_H + BASELINE
        for k, ch in enumerate(text):
            for r, row in enumerate(GLYPHS[ch]):
                for c, bit in enumerate(row):
                    x, y = x1 + ADVANCE * k + c, bottom - (TEXT_H - 1) + r
                    if bit == "#" and 0 <= x < W and 0 <= y < H:
                        out[y, x] = (255, 255, 255)
    return out


def bboxes_draw_on_img_list(images, classes, scores, bboxes, thickness=2, inplace=True, labels=False):
    """bboxes_draw_on_img for a list of uint8 [H_i,W_i,3] device tensors of any sizes (separate tensors or views into one buffer) in ONE
    launch: classes[i] int [n_i], scores[i] float [n_i] (read with labels=True only), bboxes[i] float [n_i,4].  labels=True draws the
    score label of every box as well.  -> the drawn images: the same tensors, or copies with inplace=False."""
    n = len(images)
    assert n > 0 and len(classes) == n and len(bboxes) == n
    device = images[0].device
    for im in images:
        assert im.dtype == torch.uint8 and im.dim() == 3 and im.shape[2] == 3 and im.is_contiguous() and im.device == device
    if not inplace:
        images = [im.clone() for im in images]
    boxes = torch.cat([b.to(device=device, dtype=torch.float32).reshape(-1, 4) for b in bboxes]).contiguous()
    cls = torch.cat([c.to(device=device, dtype=torch.int32).reshape(-1) for c in classes]).contiguous()
    if labels:
        assert len(scores) == n
        sc = torch.cat([s.to(device=device, dtype=torch.float32).reshape(-1) for s in scores]).contiguous()
        assert sc.numel() == cls.numel()
    nitem = ctypes.sizeof(DrawItem)
    table = torch.empty(n * nitem, dtype=torch.uint8, pin_memory=True)
    items = (DrawItem * n).from_address(table.data_ptr())
    first = 0
    for i, im in enumerate(images):
        H, W = int(im.shape[0]), int(im.shape[1])
        count = int(bboxes[i].reshape(-1, 4).shape[0])
        assert int(classes[i].numel()) == count and (not labels or int(scores[i].numel()) == count)
        items[i].image, items[i].width, items[i].height = im.data_ptr(), W, H
        items[i].first_box, items[i].num_boxes, items[i].groups, items[i].reserved = first, count, (W * H + 255) // 256, 0
        first += count
    with torch.cuda.device(device):
        table_dev = table.to(device, non_blocking=True)
        if labels:
            call("danhip_draw_boxes_labels_u8", items, ptr(table_dev), n, ptr(boxes) if first else None, ptr(cls) if first else None,
                 ptr(sc) if first else None, first, int(thickness), stream())
        else:
            call("danhip_draw_boxes_u8", items, ptr(table_dev), n, ptr(boxes) if first else None, ptr(cls) if first else None, first,
                 int(thickness), stream())
    return images


def bboxes_draw_on_img(image, classes, scores, bboxes, thickness=2, inplace=True, labels=False):
    """draw_toolbox.py:37-67 (the reference's name and argument order) for one uint8 [H,W,3] device tensor: drawn in place (as cv2 draws
    into its argument) or into a copy.  The rectangles, and with labels=True the score labels: see the module text for the rule."""
    return bboxes_draw_on_img_list([image], [classes], [scores], [bboxes], thickness, inplace, labels)[0]
