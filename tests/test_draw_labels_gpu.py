"""danhip_draw_boxes_labels_u8 (csrc/draw_exact.hip: draw_boxes_labels_kernel) on the GPU against the rule's numpy restatement
(utility.draw_toolbox.draw_reference with scores, pinned by hand in tests/test_draw_labels_cpu.py): every byte equal, no tolerance.  Images
are at most 96 x 128.  Then `python -m dan_amd.eval_sfd --debug_labels` on the tiny tree of tests/test_eval_cli_gpu.py."""
import io
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import jpeg_encode_cases as C  # noqa: E402
from test_draw_labels_cpu import double_rounding_scores, tie_scores  # noqa: E402
from test_eval_cli_gpu import EVENTS, SEED, _tree  # noqa: E402

pytestmark = pytest.mark.gpu

WHITE = np.array([255, 255, 255], np.uint8)


def _image(h, w, seed=5):
    return np.random.RandomState(seed).randint(0, 200, (h, w, 3)).astype(np.uint8)          # below 203: no pixel is white or the colour


def _draw(dev, images, sets, thickness=2, labels=True):
    """sets: (boxes [n,4], classes [n], scores [n]) per image -> the drawn arrays and the library entry points that were called."""
    from dan_amd.utility import draw_toolbox as D
    tensors = [torch.from_numpy(im).to(dev) for im in images]
    names, real = [], D.call

    def call(name, *args):
        names.append(name)
        return real(name, *args)
    D.call = call
    try:
        out = D.bboxes_draw_on_img_list(tensors, [torch.from_numpy(np.asarray(c, np.int32)) for _, c, _ in sets],
                                        [torch.from_numpy(np.asarray(s, np.float32)) for _, _, s in sets],
                                        [torch.from_numpy(np.asarray(b, np.float32).reshape(-1, 4)) for b, _, _ in sets], thickness, labels=labels)
    finally:
        D.call = real
    return [o.cpu().numpy() for o in out], names


def _check(dev, image, boxes, classes, scores, thickness=2):
    """One image through the kernel, compared with the restatement -> (the drawn array, the number of white pixels)."""
    from dan_amd.utility import draw_toolbox as D
    boxes = np.asarray(boxes, np.float32).reshape(-1, 4)
    (got,), names = _draw(dev, [image], [(boxes, classes, scores)], thickness)
    want = D.draw_reference(image, classes, boxes, thickness, scores=np.asarray(scores, np.float32))
    assert names == ["danhip_draw_boxes_labels_u8"]
    assert np.array_equal(got, want)
    return got, int((got == WHITE).all(axis=2).sum())


def _glyph_pixels(text):
    from dan_amd.utility import draw_toolbox as D
    return sum(r.count("#") for ch in text for r in D.GLYPHS[ch])


@pytest.mark.parametrize("thickness", [1, 2, 5])
def test_one_box(thickness, dev):
    image = _image(64, 96)
    got, white = _check(dev, image, [[20.0, 30.0, 70.0, 50.0]], [1], [0.873], thickness)
    assert white == _glyph_pixels("87.3%")
    # (49, 27): the tab's last column x1 + text_w, below the text (its bottom row is y1 - 5) and above the band (from y1 - t // 2)
    assert tuple(got[27, 49]) == (203, 71, 119) and np.array_equal(got[27, 50], image[27, 50])


def test_overlapping_labels_in_both_orders(dev):
    image = _image(64, 96)
    a, b = [20.0, 30.0, 60.0, 50.0], [30.0, 34.0, 80.0, 55.0]              # b's tab (y 23 .. 34, x 29 .. 59) lies over a's (y 19 .. 30, x 19 .. 49)
    ab, _ = _check(dev, image, [a, b], [1, 1], [0.25, 0.75])
    ba, _ = _check(dev, image, [b, a], [1, 1], [0.75, 0.25])
    assert not np.array_equal(ab, ba)                                       # the later box wins: painter's order


@pytest.mark.parametrize("box", [[30.0, 3.0, 70.0, 20.0], [30.0, 8.0, 70.0, 20.0], [88.0, 30.0, 94.0, 50.0], [-8.0, 30.0, 20.0, 50.0],
                                 [-40.0, 30.0, 20.0, 50.0], [70.0, 2.0, 95.0, 63.0]],
                         ids=["top_tab_only", "top_four_glyph_rows_left", "right", "left", "left_of_the_image", "top_right_corner"])
def test_clipped_labels(box, dev):
    got, white = _check(dev, _image(64, 96), [box], [1], [0.5])
    assert white < _glyph_pixels("50.0%")                                   # cut, not moved
    assert (got != _image(64, 96)).any()


@pytest.mark.parametrize("score,text", [(0.0, "0.0%"), (0.125, "12.5%"), (1.0, "100.0%"), (-0.0, "0.0%"), (9.9994, "999.9%")])
def test_label_lengths(score, text, dev):
    _, white = _check(dev, _image(48, 64), [[10.0, 20.0, 50.0, 40.0]], [1], [score])
    assert white == _glyph_pixels(text)


@pytest.mark.parametrize("score", [float("nan"), 10.0, float("inf"), -0.1], ids=["nan", "10.0", "inf", "-0.1"])
def test_score_without_a_label_keeps_the_rectangle(score, dev):
    from dan_amd.utility import draw_toolbox as D
    image, box = _image(48, 64), [[10.0, 20.0, 50.0, 40.0]]
    got, white = _check(dev, image, box, [1], [score])
    assert white == 0 and np.array_equal(got, D.draw_reference(image, [1], np.array(box, np.float32), 2))
    assert (got != image).any()


def test_skipped_boxes_draw_no_label(dev):
    image = _image(48, 64)
    got, white = _check(dev, image, [[10.0, 20.0, 50.0, 40.0], [40.0, 20.0, 30.0, 40.0], [10.0, 20.0, float("nan"), 40.0]], [0, 1, 1], [0.9, 0.9, 0.9])
    assert white == 0 and np.array_equal(got, image)


def test_300_boxes_two_chunks(dev):
    from dan_amd.utility import draw_toolbox as D
    h, w = 96, 128
    rng = np.random.RandomState(9)
    xy = rng.rand(300, 2) * [w, h] - 8
    wh = np.exp(rng.rand(300, 2) * np.log(60)) - 2                          # some negative: skipped
    boxes = np.concatenate([xy, xy + wh], 1).astype(np.float32)
    classes = (rng.rand(300) > 0.3).astype(np.int32)
    scores = rng.rand(300).astype(np.float32)
    boxes[3], classes[3], scores[3] = [40.0, 50.0, 90.0, 70.0], 1, 0.25     # first chunk
    boxes[299], classes[299], scores[299] = [46.0, 54.0, 100.0, 80.0], 1, 0.75      # second chunk, over box 3's label
    image = _image(h, w)
    got, white = _check(dev, image, boxes, classes, scores)
    assert white > 0
    swapped = np.arange(300)
    swapped[[3, 299]] = [299, 3]
    other = D.draw_reference(image, classes[swapped], boxes[swapped], 2, scores=scores[swapped])
    assert not np.array_equal(got, other)                                   # the order across the two chunks shows in the picture


def test_three_sizes_one_call(dev):
    from dan_amd.utility import draw_toolbox as D
    sizes = [(37, 53), (95, 127), (61, 77)]                                 # neither the widths nor the pixel counts are multiples of 256
    assert all(w % 256 and (h * w) % 256 for h, w in sizes)
    images = [_image(h, w, seed=k) for k, (h, w) in enumerate(sizes)]
    sets = [(np.array([[5.0, 14.0, 30.0, 30.0], [20.0, 20.0, 52.0, 36.0]], np.float32), [1, 1], [0.31, 0.995]),
            (np.zeros((0, 4), np.float32), [], []),
            (np.array([[40.0, 40.0, 76.0, 60.0]], np.float32), [1], [0.07])]
    out, names = _draw(dev, images, sets, 3)
    assert names == ["danhip_draw_boxes_labels_u8"]                         # one library call, which issues one launch
    for im, (b, c, s), o in zip(images, sets, out):
        assert np.array_equal(o, D.draw_reference(im, c, b, 3, scores=s)), im.shape
    assert np.array_equal(out[1], images[1]) and (out[2][60, 76] != images[2][60, 76]).any()       # the last pixel row and column are reached


def test_labels_false_is_the_rectangle_entry(dev):
    from dan_amd import _lib
    from dan_amd.utility import draw_toolbox as D
    image = _image(61, 77)
    boxes = np.array([[5.0, 14.0, 30.0, 30.0], [20.0, 20.0, 52.0, 36.0]], np.float32)
    (got,), names = _draw(dev, [image], [(boxes, [1, 1], [0.31, 0.995])], 2, labels=False)
    assert names == ["danhip_draw_boxes_u8"]
    t, b, c = torch.from_numpy(image).to(dev), torch.from_numpy(boxes).to(dev), torch.ones(2, dtype=torch.int32, device=dev)
    items = (_lib.DrawItem * 1)()
    items[0].image, items[0].width, items[0].height, items[0].first_box, items[0].num_boxes = t.data_ptr(), 77, 61, 0, 2
    items[0].groups = (61 * 77 + 255) // 256
    table = torch.frombuffer(bytearray(bytes(items)), dtype=torch.uint8).to(dev)
    _lib.call("danhip_draw_boxes_u8", items, _lib.ptr(table), 1, _lib.ptr(b), _lib.ptr(c), 2, 2, _lib.stream())
    assert np.array_equal(got, t.cpu().numpy()) and np.array_equal(got, D.draw_reference(image, [1, 1], boxes, 2))
    # the label entry on the same table: refused without scores, other bytes with them
    L = _lib.lib()
    assert L.danhip_draw_boxes_labels_u8(items, _lib.ptr(table), 1, _lib.ptr(b), _lib.ptr(c), None, 2, 2, _lib.stream()) != 0
    assert L.danhip_draw_boxes_labels_u8(items, _lib.ptr(table), 1, _lib.ptr(b), _lib.ptr(c), _lib.ptr(b), 2, 0, _lib.stream()) != 0
    torch.cuda.synchronize()
    labelled, _ = _draw(dev, [image], [(boxes, [1, 1], [0.31, 0.995])], 2)
    assert not np.array_equal(labelled[0], got)


def test_tie_and_double_rounding_scores_through_the_kernel(dev):
    ties, _ = tie_scores()
    twice = double_rounding_scores()
    scores = np.concatenate([ties[::len(ties) // 9][:9], twice[:9]]).astype(np.float32)
    assert len(scores) == 18
    boxes = np.array([[4.0 + 42 * (k % 3), 14.0 + 15 * (k // 3), 34.0 + 42 * (k % 3), 16.0 + 15 * (k // 3)] for k in range(18)], np.float32)
    _, white = _check(dev, _image(96, 128), boxes, [1] * 18, scores)
    assert white > 18 * 30


# ------------------------------------------------------------------------------------------------- the evaluation command
def test_eval_cli_debug_labels(dev, tmp_path):
    from dan_amd import eval_cli, eval_sfd
    from dan_amd.dataset.jpeg import JpegDecoder
    from dan_amd.utility import checkpoint, draw_toolbox
    root = tmp_path
    datas = _tree(root)
    event, names = EVENTS[0]
    names = names[:2]
    (root / "two.txt").write_text("".join("%s/%s\n" % (event, n) for n in names))
    net = eval_cli.build_detector("sfd", dev, "act", seed=SEED)
    os.makedirs(str(root / "logs"))
    checkpoint.save_checkpoint(net.model.vs, str(root / "logs" / "model.ckpt-5"), "sfd", checksums=True)
    common = ["--data_dir", str(root), "--image_list", str(root / "two.txt"), "--det_dir", str(root / "det"), "--checkpoint_path",
              str(root / "logs" / "model.ckpt-5"), "--log_every_n_steps", "1", "--batch_images", "2"]
    calls, real = [], draw_toolbox.call

    def call(name, *args):
        calls.append(name)
        return real(name, *args)
    draw_toolbox.call = call
    try:
        eval_sfd.main(common + ["--debug_dir", str(root / "plain")], out=io.StringIO())
        eval_sfd.main(common + ["--debug_dir", str(root / "labels"), "--debug_labels"], out=io.StringIO())
    finally:
        draw_toolbox.call = real
    assert calls == ["danhip_draw_boxes_u8", "danhip_draw_boxes_labels_u8"]              # one draw launch per group, with and without
    L = C.host_lib()
    white = 0
    for n in names:
        image_dev = JpegDecoder(dev).decode(datas[event + "/" + n])
        det = eval_sfd.detect_image(net, image_dev).cpu().numpy()
        image = image_dev.cpu().numpy()
        classes = (det[:, 4] > 0.2).astype(np.int32)
        plain = draw_toolbox.draw_reference(image, classes, det[:, :4], thickness=2)
        labelled = draw_toolbox.draw_reference(image, classes, det[:, :4], thickness=2, scores=det[:, 4])
        white += int(((labelled == WHITE).all(axis=2) & ~(plain == WHITE).all(axis=2)).sum())
        assert (root / "plain" / (n + ".jpg")).read_bytes() == C.encode_host(L, plain, 75, 3), n         # without the flag: today's bytes
        assert (root / "labels" / (n + ".jpg")).read_bytes() == C.encode_host(L, labelled, 75, 3), n
    assert white > 0, "the seeded network scores some box above 0.2: a label is in the files"
