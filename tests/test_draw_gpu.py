"""danhip_draw_boxes_u8 (csrc/draw_exact.hip) on the GPU against the rule's numpy restatement (utility.draw_toolbox.draw_reference, itself
pinned on hand-traced cases by tests/test_eval_cli_cpu.py): the traced cases, a list of three images of different sizes with 0, 1 and 750
boxes in ONE launch, other thicknesses, in place and into a copy.  Equality, no tolerance."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_eval_cli_cpu import TRACED  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("case", TRACED, ids=[c[0] for c in TRACED])
def test_traced_cases(case, dev):
    from dan_amd.utility import draw_toolbox as D
    _, boxes, classes, _ = case
    image = np.random.RandomState(5).randint(0, 200, (12, 12, 3)).astype(np.uint8)
    t = torch.from_numpy(image).to(dev)
    b, c = torch.tensor(boxes, dtype=torch.float32), torch.tensor(classes, dtype=torch.int32)
    copy = D.bboxes_draw_on_img(t, c, None, b, thickness=2, inplace=False)
    want = D.draw_reference(image, classes, np.array(boxes, np.float32), 2)
    assert np.array_equal(copy.cpu().numpy(), want) and np.array_equal(t.cpu().numpy(), image)       # the copy is drawn, the source kept
    same = D.bboxes_draw_on_img(t, c, None, b)
    assert same.data_ptr() == t.data_ptr() and np.array_equal(t.cpu().numpy(), want)                 # in place, as cv2 draws


def _boxes(n, h, w, seed):
    rng = np.random.RandomState(seed)
    xy = rng.rand(n, 2) * [w, h] - 8                                          # some start outside
    wh = np.exp(rng.rand(n, 2) * np.log(60)) - 2                              # some negative: skipped
    b = np.concatenate([xy, xy + wh], 1).astype(np.float32)
    c = (rng.rand(n) > 0.3).astype(np.int32)
    return b, c


@pytest.mark.parametrize("thickness", [1, 2, 3, 5])
def test_list_of_three_sizes_one_launch(thickness, dev):
    from dan_amd.utility import draw_toolbox as D
    sizes, counts = [(37, 53), (120, 160), (203, 331)], [0, 1, 750]          # 750 boxes: three LDS chunks, the last one partial
    images = [np.random.RandomState(k).randint(0, 256, (h, w, 3)).astype(np.uint8) for k, (h, w) in enumerate(sizes)]
    sets = [_boxes(n, h, w, 70 + n) for n, (h, w) in zip(counts, sizes)]
    sets[1] = (np.array([[10.5, 20.5, 100.0, 90.0]], np.float32), np.array([1], np.int32))
    buf = torch.empty(sum((3 * h * w + 255) // 256 * 256 for h, w in sizes) + 1, dtype=torch.uint8, device=dev)
    tensors, at = [], 1                                                       # views into one buffer, at odd byte offsets
    for im in images:
        n = im.size
        v = buf[at:at + n].view(im.shape)
        v.copy_(torch.from_numpy(im))
        tensors.append(v)
        at += (n + 255) // 256 * 256
    names = []
    real = D.call

    def call(name, *args):
        names.append(name)
        return real(name, *args)
    D.call = call
    try:
        out = D.bboxes_draw_on_img_list(tensors, [torch.from_numpy(c) for _, c in sets], [None] * 3, [torch.from_numpy(b) for b, _ in sets], thickness)
    finally:
        D.call = real
    assert names == ["danhip_draw_boxes_u8"]                                  # one library call, which issues one launch
    painted = 0
    for im, (b, c), o in zip(images, sets, out):
        want = D.draw_reference(im, c, b, thickness)
        assert np.array_equal(o.cpu().numpy(), want), im.shape
        painted += int((want != im).any(axis=2).sum())
    assert np.array_equal(out[0].cpu().numpy(), images[0]) and painted > 5000


def test_bad_items_are_refused(dev):
    from dan_amd import _lib
    from dan_amd._lib import DrawItem
    import ctypes
    L = _lib.lib()
    img = torch.zeros((12, 12, 3), dtype=torch.uint8, device=dev)
    boxes = torch.zeros((2, 4), dtype=torch.float32, device=dev)
    cls = torch.ones((2,), dtype=torch.int32, device=dev)
    items = (DrawItem * 1)()
    items[0].image, items[0].width, items[0].height, items[0].first_box, items[0].num_boxes, items[0].groups = img.data_ptr(), 12, 12, 0, 2, 1
    table = torch.frombuffer(bytearray(bytes(items)), dtype=torch.uint8).to(dev)
    run = lambda t=2, n=2: L.danhip_draw_boxes_u8(items, _lib.ptr(table), 1, _lib.ptr(boxes), _lib.ptr(cls), n, t, _lib.stream())
    assert run() == 0
    assert run(t=0) != 0 and run(t=65) != 0 and run(n=1) != 0                 # thickness outside 1 .. 64; boxes leave the rows
    items[0].groups = 2
    assert run() != 0                                                          # groups is re-derived from the size
    torch.cuda.synchronize()
