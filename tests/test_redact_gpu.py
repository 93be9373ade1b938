"""Face redaction on the GPU (danhip_redact_u8 through dan_amd/utility/redact.py apply): every byte of every output image - the pixels
no rectangle touches included - equals tests/redact_rule.py's independent restatement, the device count equals the rule's, and the source
tensors are unchanged.  Shapes are the smallest at which each path can go wrong; strip and band sizes come from the header's constants
(redact.STRIP / redact.BAND, held to include/danhip.h by tests/test_redact_cpu.py)."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import redact_rule as R  # noqa: E402
from dan_amd.utility import redact  # noqa: E402

pytestmark = pytest.mark.gpu

NAN, INF = float("nan"), float("inf")
STRIP, BAND = redact.STRIP, redact.BAND
MODE_SHAPES = [(m, s) for m in ("blur", "mosaic", "fill") for s in ("rect", "ellipse")]


def noise(H, W, seed):
    return np.random.RandomState(seed).randint(0, 256, (H, W, 3)).astype(np.uint8)


def upload(image, dev, offset=0, pad=0):
    """The image as a device view at byte `offset` of a buffer, rows 3 * W + pad bytes apart; the bytes between rows are 0xEE."""
    H, W = image.shape[:2]
    pitch = 3 * W + pad
    host = np.full(offset + H * pitch, 0xEE, np.uint8)
    for y in range(H):
        host[offset + y * pitch:offset + y * pitch + 3 * W] = image[y].reshape(-1)
    buffer = torch.from_numpy(host).to(dev)
    return buffer, buffer[offset:].as_strided((H, W, 3), (pitch, 3, 1))


def table(rows_per_image, R_):
    """-> dets fp32 [B, R_, 5] (unused rows hold a box that would be redacted if num did not exclude it) and nums"""
    dets = np.zeros((len(rows_per_image), R_, 5), np.float32)
    dets[..., 2:4] = 3.0
    dets[..., 4] = 1.0
    for b, rows in enumerate(rows_per_image):
        for r, row in enumerate(rows):
            dets[b, r] = row
    return dets, [len(rows) for rows in rows_per_image]


def check(dev, images, dets, nums, offset=0, pad=0, repeat=False, **kw):
    """apply on the device against the rule, byte for byte; -> the device outputs as numpy"""
    held = [upload(im, dev, offset, pad) for im in images]
    before = [b.clone() for b, _ in held]
    d = torch.from_numpy(np.asarray(dets, np.float32)).to(dev)
    n = torch.tensor(nums, dtype=torch.int32, device=dev)
    got, count = redact.apply([v for _, v in held], d, n, **kw)
    if repeat:
        again, count2 = redact.apply([v for _, v in held], d, n, **kw)
    rule = dict(kw)
    rule["strength_pm"] = redact.strength_per_mille(rule.pop("strength", 0.125))
    rule["margin_pm"] = redact.margin_per_mille(rule.pop("margin", 0.0))
    rule["threshold"] = rule.pop("score_threshold", 0.0)
    want, want_count = R.reference(images, dets, nums, **rule)
    assert int(count.item()) == want_count
    assert len(got) == len(images)
    outs = []
    for i, (g, w) in enumerate(zip(got, want)):
        assert g.dtype == torch.uint8 and tuple(g.shape) == images[i].shape and g.is_contiguous()
        g = g.cpu().numpy()
        bad = np.argwhere((g != w).any(-1))
        assert bad.size == 0, "image %d: %d pixels differ, the first at (y, x) = %s: %s against the rule's %s" % (
            i, len(bad), tuple(bad[0]), g[tuple(bad[0])], w[tuple(bad[0])])
        outs.append(g)
    for (buffer, _), b in zip(held, before):
        assert torch.equal(buffer, b), "the source was written"
    if repeat:
        assert int(count2.item()) == want_count and all(np.array_equal(a.cpu().numpy(), g) for a, g in zip(again, outs))
    return outs


def test_image_smaller_than_the_window_in_both_directions(dev):
    im = noise(5, 7, 1)                                          # 7 x 5 with e = 7 * 600 // 1000 = 4: every window is clipped on all four sides
    dets, nums = table([[[0, 0, 6, 4, 0.9]]], 1)
    out = check(dev, [im], dets, nums, strength=0.6)
    assert redact.extent(7, 5, 600) == 4 and (out[0][2, 3] == (im.astype(np.int64).sum((0, 1)) + 17) // 35).all()      # the centre sees it all


@pytest.mark.parametrize("mode,shape", MODE_SHAPES)
def test_rectangles_flush_with_each_border_and_the_smallest_extent(dev, mode, shape):
    im = noise(30, 40, 2)
    rows = [[0, 10, 5, 20, 0.9], [34, 10, 39, 20, 0.9], [10, 0, 20, 4, 0.9], [10, 25, 20, 29, 0.9], [0, 0, 0, 0, 0.9], [39, 29, 39, 29, 0.9]]
    dets, nums = table([rows], 6)
    check(dev, [im], dets, nums, mode=mode, shape=shape, strength=0.001, fill=(200, 100, 50))       # e = 1, c = 2


def test_the_largest_extent_on_random_black_and_white_images(dev):
    H, W = 280, 300
    images = [noise(H, W, 3), np.zeros((H, W, 3), np.uint8), np.full((H, W, 3), 255, np.uint8)]
    dets, nums = table([[[20, 10, 274, 200, 0.9]]] * 3, 1)       # 255 wide, strength 1: e = 255
    assert redact.extent(255, 191, 1000) == 255
    out = check(dev, images, dets, nums, strength=1.0)
    assert (out[1] == 0).all() and (out[2] == 255).all()         # the largest sums do not wrap
    out = check(dev, images, dets, nums, strength=1.0, mode="mosaic", shape="ellipse")       # c = 255: one cell
    assert (out[2] == 255).all()


@pytest.mark.parametrize("mode", ["blur", "fill"])
def test_rectangles_a_strip_wide_and_one_column_wider(dev, mode):
    im = noise(20, STRIP + 12, 4)
    rows = [[5, 2, 5 + STRIP, 4, 0.9], [10, 10, 10 + STRIP - 1, 12, 0.9]]       # STRIP + 1 and STRIP columns
    dets, nums = table([rows], 2)
    check(dev, [im], dets, nums, mode=mode, strength=0.008, fill=(1, 2, 3))      # e = 2


@pytest.mark.parametrize("mode", ["blur", "fill"])
def test_rectangles_a_band_tall_and_one_row_taller(dev, mode):
    im = noise(BAND + 10, 20, 5)
    rows = [[2, 3, 4, 3 + BAND, 0.9], [10, 5, 12, 5 + BAND - 1, 0.9]]           # BAND + 1 and BAND rows
    dets, nums = table([rows], 2)
    check(dev, [im], dets, nums, mode=mode, strength=0.05, fill=(1, 2, 3))       # e = 3
    both = [[1, 1, 1 + STRIP, 1 + BAND, 0.9]]                                   # four items, the last one a single pixel
    dets, nums = table([both], 1)
    check(dev, [noise(BAND + 3, STRIP + 3, 6)], dets, nums, mode=mode, shape="ellipse", strength=0.02, fill=(1, 2, 3))


@pytest.mark.parametrize("mode,shape", MODE_SHAPES)
def test_odd_offset_padded_pitch_and_a_row_length_that_is_no_multiple_of_four(dev, mode, shape):
    im = noise(23, 37, 7)                                        # 3 * 37 = 111 bytes per row
    rows = [[3, 2, 20, 15, 0.9], [15, 10, 36, 22, 0.8], [0, 18, 9, 22, 0.7]]
    dets, nums = table([rows], 3)
    check(dev, [im], dets, nums, offset=5, pad=1, mode=mode, shape=shape, strength=0.2, fill=(7, 8, 9))
    check(dev, [im], dets, nums, offset=2, pad=2, mode=mode, shape=shape, strength=0.2, margin=0.25, fill=(7, 8, 9))


@pytest.mark.parametrize("mode,shape", MODE_SHAPES)
def test_overlapping_rows_belong_to_the_last_valid_one(dev, mode, shape):
    im = noise(40, 48, 8)
    rows = [[4, 4, 30, 30, 0.9], [10, 8, 40, 36, 0.9], [6, 6, 35, 25, 0.9], [6, 6, 35, 25, 0.9],       # three overlapping, two identical
            [0, 0, 47, 39, 0.1]]                                                                        # the last row, over everything, is invalid
    dets, nums = table([rows], 5)
    check(dev, [im], dets, nums, mode=mode, shape=shape, strength=0.15, score_threshold=0.5, fill=(255, 0, 128))


@pytest.mark.parametrize("mode", ["blur", "mosaic", "fill"])
def test_rows_that_give_no_rectangle(dev, mode):
    im = noise(32, 32, 9)
    thr = float(np.float32(0.3))
    rows = [[2, 2, 9, 9, 0.9], [NAN, 2, 20, 20, 0.9], [2, 2, INF, 20, 0.9], [2, -INF, 20, 20, 0.9], [12, 12, 20, 20, 0.2999],
            [14, 3, 25, 9, thr],                                  # a score equal to the threshold is kept
            [40, 40, 50, 50, 0.9], [-20, -20, -1, -1, 0.9], [5, 33, 9, 40, 0.9],      # entirely outside the image
            [9, 9, 2, 2, 0.9],                                    # w, h < 1
            [22, 22, 30, 30, 0.9], [0, 0, 31, 31, 0.9]]           # beyond num
    dets, _ = table([rows], 12)
    check(dev, [im], dets, [10], mode=mode, score_threshold=thr, strength=0.25, fill=(0, 255, 0))
    assert R.reference([im], dets, [10], mode=mode, threshold=thr, strength_pm=250)[1] == 2


def test_no_rows_and_no_detections_copy_the_images(dev):
    images = [noise(9, 13, 10), noise(4, 5, 11)]
    out = check(dev, images, np.zeros((2, 0, 5), np.float32), [0, 0], offset=3, pad=1)
    assert all(np.array_equal(o, im) for o, im in zip(out, images))
    dets, _ = table([[[0, 0, 8, 8, 0.9]], [[0, 0, 3, 3, 0.9]]], 2)
    out = check(dev, images, dets, [0, 0])
    assert all(np.array_equal(o, im) for o, im in zip(out, images))


@pytest.mark.parametrize("mode,shape", MODE_SHAPES)
def test_four_images_of_different_sizes_in_one_call(dev, mode, shape):
    images = [noise(31, 45, 12), noise(8, 9, 13), noise(70, 33, 14), noise(17, 64, 15)]
    rows = [[[5, 5, 25, 20, 0.9], [20, 10, 44, 30, 0.6]], [], [[0, 0, 32, 69, 0.7], [3, 30, 20, 50, 0.9], [10, 40, 30, 60, 0.8]], []]
    dets, nums = table(rows, 3)
    check(dev, images, dets, nums, mode=mode, shape=shape, strength=0.125, margin=0.1, fill=(10, 20, 30), repeat=True)


def test_mosaic_cells_of_two_and_a_rectangle_smaller_than_its_cell(dev):
    im = noise(24, 28, 16)
    rows = [[1, 1, 17, 13, 0.9], [20, 3, 24, 5, 0.9], [26, 20, 26, 20, 0.9]]
    dets, nums = table([rows], 3)
    check(dev, [im], dets, nums, mode="mosaic", strength=0.001)                  # c = 2: 9 x 7 cells, the last column and row one pixel wide
    check(dev, [im], dets, nums, mode="mosaic", strength=1.0)                    # c = the longer side: 5 x 3 and 1 x 1 rectangles inside one cell
    check(dev, [im], dets, nums, mode="mosaic", shape="ellipse", strength=0.3)


def test_more_later_rectangles_than_the_list_holds_and_more_rows_than_a_round(dev):
    rng = np.random.RandomState(17)
    im = noise(36, 44, 18)
    rows = []
    for _ in range(300):                                         # 300 rows of one image: two rounds of 256 table rows; most meet every tile
        x1, y1 = rng.randint(0, 30), rng.randint(0, 24)
        rows.append([x1, y1, x1 + rng.randint(4, 14), y1 + rng.randint(4, 12), 0.9])
    dets, nums = table([rows, rows[:70]], 300)
    for mode, shape in (("blur", "ellipse"), ("mosaic", "rect"), ("fill", "ellipse")):
        check(dev, [im, im[:30, :40].copy()], dets, nums, mode=mode, shape=shape, strength=0.2, fill=(3, 2, 1))


def test_a_non_black_fill_and_an_output_of_a_previous_call(dev):
    im = noise(20, 20, 19)
    dets, nums = table([[[2, 2, 12, 12, 0.9]]], 1)
    out = check(dev, [im], dets, nums, mode="fill", fill=(255, 128, 1))
    assert out[0][5, 5].tolist() == [255, 128, 1] and out[0][0, 0].tolist() == im[0, 0].tolist()
    src = torch.from_numpy(im).to(dev)
    d, n = torch.from_numpy(dets).to(dev), torch.tensor(nums, dtype=torch.int32, device=dev)
    first = redact.apply([src], d, n, mode="fill", fill=(1, 1, 1))
    second = redact.apply([src], d, n, mode="blur", out=first)
    assert second[0][0].data_ptr() == first[0][0].data_ptr()
    assert np.array_equal(second[0][0].cpu().numpy(), R.reference([im], dets, nums)[0][0])
