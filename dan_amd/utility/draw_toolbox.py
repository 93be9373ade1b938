"""utility/draw_toolbox.py of the reference on the device: the detection rectangles of the debug images (eval_dan.py:455-458), drawn into
uint8 [H,W,3] device tensors by one launch for a whole list of images (csrc/draw_exact.hip).

The reference draws with cv2.rectangle; OpenCV is not a dependency here and nothing could be compared with it, so the rule is this
project's own, stated once and restated in numpy by draw_reference below:

  * box i is skipped when classes[i] < 1 or one of its coordinates is not finite;
  * corners: x1, y1, x2, y2 = int(bbox[0]), int(bbox[1]), int(bbox[2]), int(bbox[3]), truncated toward zero as draw_toolbox.py:51-52 does
    (bbox[0] / bbox[2] run along the width, as in the reference's call with rows of (xmin, ymin, xmax, ymax); clamped to +-2^30);
  * the box is skipped when x2 < x1 or y2 < y1 (:53-54);
  * with t = thickness, pixel (x, y) of the image is painted colors_tableau[1] = (203, 71, 119) when
        x1 - t//2 <= x <= x2 + t//2  and  y1 - t//2 <= y <= y2 + t//2
    unless it lies in the interior
        x1 + (t+1)//2 <= x <= x2 - (t+1)//2  and  y1 + (t+1)//2 <= y <= y2 - (t+1)//2;
    for t = 2 the band is the two pixels x1 - 1, x1 on the left, x2, x2 + 1 on the right, and likewise above and below.

There is one colour, so the result does not depend on the order of the boxes.  THE SCORE LABEL ('%.1f%%' in FONT_HERSHEY_SIMPLEX on a
filled rectangle, :57-65) IS NOT DRAWN: it needs Hershey-font text rendering, and nothing here could check that against OpenCV; `scores`
is taken for the reference's argument order and not read."""
import ctypes

import numpy as np
import torch

from .._lib import DrawItem, call, ptr, stream

colors_tableau = [(12, 7, 134), (203, 71, 119)]
_LIMIT = 1 << 30


def draw_reference(image, classes, bboxes, thickness=2):
    """The rule above in numpy, on a copy of a uint8 [H,W,3] array -> the drawn array.  What the kernel is tested against."""
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
    return out


def bboxes_draw_on_img_list(images, classes, scores, bboxes, thickness=2, inplace=True):
    """bboxes_draw_on_img for a list of uint8 [H_i,W_i,3] device tensors of any sizes (separate tensors or views into one buffer) in ONE
    launch: classes[i] int [n_i], scores[i] (not read), bboxes[i] float [n_i,4].  -> the drawn images: the same tensors, or copies with
    inplace=False."""
    n = len(images)
    assert n > 0 and len(classes) == n and len(bboxes) == n
    device = images[0].device
    for im in images:
        assert im.dtype == torch.uint8 and im.dim() == 3 and im.shape[2] == 3 and im.is_contiguous() and im.device == device
    if not inplace:
        images = [im.clone() for im in images]
    boxes = torch.cat([b.to(device=device, dtype=torch.float32).reshape(-1, 4) for b in bboxes]).contiguous()
    cls = torch.cat([c.to(device=device, dtype=torch.int32).reshape(-1) for c in classes]).contiguous()
    nitem = ctypes.sizeof(DrawItem)
    table = torch.empty(n * nitem, dtype=torch.uint8, pin_memory=True)
    items = (DrawItem * n).from_address(table.data_ptr())
    first = 0
    for i, im in enumerate(images):
        H, W = int(im.shape[0]), int(im.shape[1])
        count = int(bboxes[i].reshape(-1, 4).shape[0])
        assert int(classes[i].numel()) == count
        items[i].image, items[i].width, items[i].height = im.data_ptr(), W, H
        items[i].first_box, items[i].num_boxes, items[i].groups, items[i].reserved = first, count, (W * H + 255) // 256, 0
        first += count
    with torch.cuda.device(device):
        table_dev = table.to(device, non_blocking=True)
        call("danhip_draw_boxes_u8", items, ptr(table_dev), n, ptr(boxes) if first else None, ptr(cls) if first else None, first, int(thickness),
             stream())
    return images


def bboxes_draw_on_img(image, classes, scores, bboxes, thickness=2, inplace=True):
    """draw_toolbox.py:37-67 (the reference's name and argument order) for one uint8 [H,W,3] device tensor: drawn in place (as cv2 draws
    into its argument) or into a copy.  The rectangles only: see the module text for the rule and for the label that is not drawn."""
    return bboxes_draw_on_img_list([image], [classes], [scores], [bboxes], thickness, inplace)[0]
