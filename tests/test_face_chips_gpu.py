"""Face chips on the GPU (dan_amd/utility/face_chips.py extract -> danhip_face_chips_u8, csrc/face_chips_exact.hip) against
tests/face_chips_rule.py: chips, chip_src and count bit for bit.  Two images of odd sizes (the second a view with pitch != 3 * W that starts
at an odd byte), boxes listed as literals, one per class of the rule and of the resize; then capacity, empty inputs, repeatability and one
case in which every loop of the two kernels wraps."""
import numpy as np
import pytest
import torch

import face_chips_rule as R
from dan_amd.utility import face_chips

pytestmark = pytest.mark.gpu

SIZES = [(37, 53), (64, 41)]                 # (H, W)
PITCH1 = 3 * 41 + 5
THRESHOLD = 0.1
ROWS = 12
NUM = [10, 7]
NAN = float("nan")
# (x1, y1, x2, y2, score), class
BOXES = [
    [((10.3, 8.9, 25.0, 20.5, 0.9), "interior"),
     ((0.0, 5.0, 12.0, 18.0, 0.8), "left edge"),
     ((20.0, 0.0, 30.7, 9.2, 0.8), "top edge"),
     ((40.0, 10.0, 52.0, 22.0, 0.8), "right edge"),
     ((15.0, 25.0, 28.0, 36.0, 0.8), "bottom edge"),
     ((52.0, 36.0, 52.9, 36.9, 0.7), "1 x 1 at the last pixel"),
     ((-20.0, -30.0, 90.0, 80.0, 0.95), "larger than the image"),
     ((30.0, 15.0, 31.0, 16.0, 0.6), "2 x 2"),
     ((60.0, 40.0, 70.0, 50.0, 0.9), "outside"),
     ((5.0, 5.0, 15.0, 15.0, 0.05), "under the threshold"),
     ((3.0, 3.0, 20.0, 20.0, 0.99), "beyond num"),
     ((NAN, NAN, NAN, NAN, NAN), "beyond num")],
    [((5.5, 10.2, 30.9, 50.1, 0.9), "interior"),
     ((40.0, 63.0, 40.0, 63.0, 0.6), "1 x 1 at the last pixel"),
     ((30.0, 50.0, 40.0, 63.0, 0.5), "right edge"),
     ((-5.0, -5.0, 100.0, 100.0, 0.99), "larger than the image"),
     ((10.0, 10.0, 11.0, 11.0, 0.1), "2 x 2"),                     # the score equals the threshold: kept
     ((NAN, 10.0, 30.0, 30.0, 0.9), "not finite"),
     ((20.0, 10.0, 19.0, 30.0, 0.9), "w = 0"),
     ((1.0, 1.0, 30.0, 30.0, 0.99), "beyond num"),
     ((1.0e30, -1.0e30, 3.0e38, 5.0, 7.0), "beyond num"),
     ((0.0, 0.0, 40.0, 63.0, 1.0), "beyond num"),
     ((2.0, 2.0, 9.0, 9.0, 0.5), "beyond num"),
     ((2.0, 2.0, 9.0, 9.0, 0.5), "beyond num")],
]
CONFIGS = [(S, pm, sq) for S in (1, 7, 16) for pm in (0, 250) for sq in (True, False)]


@pytest.fixture(scope="module")
def case(dev):
    rng = np.random.RandomState(20240611)
    host = [rng.randint(0, 256, size=(h, w, 3)).astype(np.uint8) for h, w in SIZES]
    first = torch.from_numpy(host[0]).to(dev)
    buf = torch.full((1 + 64 * PITCH1,), 0x5A, dtype=torch.uint8, device=dev)
    second = torch.as_strided(buf, (64, 41, 3), (PITCH1, 3, 1), storage_offset=1)
    second.copy_(torch.from_numpy(host[1]).to(dev))
    assert second.data_ptr() % 2 == 1 and second.stride(0) != 3 * 41 and torch.equal(second.cpu(), torch.from_numpy(host[1]))
    dets = np.array([[b for b, _ in rows] for rows in BOXES], dtype=np.float32)
    assert dets.shape == (2, ROWS, 5)
    ref = {c: R.reference(host, dets, NUM, c[0], c[1], c[2], THRESHOLD) for c in CONFIGS}      # computed once, read by every test
    return dict(host=host, images=[first, second], dets_host=dets, dets=torch.from_numpy(dets).to(dev),
                num=torch.tensor(NUM, dtype=torch.int32, device=dev), ref=ref, keep=buf)


def _run(case, S, pm, sq, **kw):
    return face_chips.extract(case["images"], case["dets"], case["num"], size=S, margin=pm / 1000.0, square=sq, score_threshold=THRESHOLD, **kw)


def test_the_reference_has_a_chip_of_every_class(case):
    """The helper alone: no class of box may silently drop out of the comparison below."""
    for (S, pm, sq), (chips, src, count) in case["ref"].items():
        got = {(int(i), int(r)) for i, r in src[:, :2]}
        for i, rows in enumerate(BOXES):
            for r, (_, cls) in enumerate(rows):
                gives = cls not in ("outside", "under the threshold", "beyond num", "not finite", "w = 0")
                assert ((i, r) in got) == gives, (S, pm, sq, i, r, cls)
        assert count == len(chips) == 13
        by = {(int(s[0]), int(s[1])): tuple(int(v) for v in s[2:]) for s in src}
        assert by[(0, 6)] == (0, 0, 52, 36) and by[(1, 3)] == (0, 0, 40, 63)                    # clamped to the whole image
        if pm == 0 and not sq:
            assert by[(0, 5)] == (52, 36, 52, 36) and by[(1, 1)] == (40, 63, 40, 63)            # 1 x 1: the xedge path at column 0 of the crop
            assert by[(0, 1)][0] == 0 and by[(0, 2)][1] == 0 and by[(0, 3)][2] == 52 and by[(0, 4)][3] == 36
            assert by[(0, 7)] == (30, 15, 31, 16)
    # an upscale of more than 4 x (2 x 2 -> 16) and a downscale of more than 4 x (53 x 37 -> 7, 41 x 64 -> 7 and -> 1)
    src16 = case["ref"][(16, 0, False)][1]
    assert any((s[4] - s[2] + 1) * 4 < 16 and (s[5] - s[3] + 1) * 4 < 16 for s in src16)
    src7 = case["ref"][(7, 0, False)][1]
    assert any(s[4] - s[2] + 1 > 4 * 7 and s[5] - s[3] + 1 > 4 * 7 for s in src7)


@pytest.mark.parametrize("S, pm, sq", CONFIGS)
def test_chips_equal_the_reference(case, S, pm, sq):
    chips, src, count = case["ref"][(S, pm, sq)]
    out = _run(case, S, pm, sq)
    assert tuple(out.chips.shape) == (2 * ROWS, S, S, 3) and tuple(out.chip_src.shape) == (2 * ROWS, 6)
    assert int(out.count.item()) == count
    assert np.array_equal(out.chip_src[:count].cpu().numpy(), src)
    got = out.chips[:count].cpu().numpy()
    for k in range(count):
        assert np.array_equal(got[k], chips[k]), (k, src[k].tolist())
    per_image = out.to_host()
    assert [len(v) for v in per_image] == [int((src[:, 0] == i).sum()) for i in range(2)]
    row, rect, chip = per_image[1][0]
    k = int(np.nonzero(src[:, 0] == 1)[0][0])
    assert (row, rect) == (int(src[k, 1]), tuple(int(v) for v in src[k, 2:])) and np.array_equal(chip, chips[k])


def _sentinel(dev, S, cap, extra=2):
    chips = torch.full((cap + extra, S, S, 3), 0xA5, dtype=torch.uint8, device=dev)
    src = torch.full((cap + extra, 6), -7, dtype=torch.int32, device=dev)
    count = torch.full((1,), -7, dtype=torch.int32, device=dev)
    return chips, src, count


def test_capacity_below_the_total_keeps_the_first_chips_and_the_true_count(case, dev):
    S, cap = 7, 5
    chips, src, count = case["ref"][(S, 250, True)]
    full = _sentinel(dev, S, cap)
    out = _run(case, S, 250, True, max_chips=cap, out=(full[0][:cap], full[1][:cap], full[2]))
    assert int(out.count.item()) == count == 13
    assert np.array_equal(full[1][:cap].cpu().numpy(), src[:cap]) and np.array_equal(full[0][:cap].cpu().numpy(), np.stack(chips[:cap]))
    assert bool((full[0][cap:] == 0xA5).all()) and bool((full[1][cap:] == -7).all())
    assert len(sum(out.to_host(), [])) == cap


def test_no_detections_write_a_zero_count_and_nothing_else(case, dev):
    S = 16
    full = _sentinel(dev, S, 2 * ROWS, extra=0)
    zero = torch.zeros_like(case["num"])
    out = face_chips.extract(case["images"], case["dets"], zero, size=S, score_threshold=THRESHOLD, out=full)
    assert int(out.count.item()) == 0 and bool((full[0] == 0xA5).all()) and bool((full[1] == -7).all())
    assert out.to_host() == [[], []]


def test_an_empty_image_list_succeeds(case, dev):
    out = face_chips.extract([], case["dets"][:0], case["num"][:0], size=16)
    assert int(out.count.item()) == 0 and tuple(out.chips.shape) == (0, 16, 16, 3) and out.to_host() == []
    rows0 = face_chips.extract(case["images"], case["dets"][:, :0].contiguous(), case["num"], size=16)
    assert int(rows0.count.item()) == 0 and rows0.to_host() == [[], []]


def test_two_calls_give_the_same_bytes(case):
    a, b = _run(case, 16, 250, True), _run(case, 16, 250, True)
    n = int(a.count.item())
    assert n == int(b.count.item()) == 13
    assert torch.equal(a.chips[:n], b.chips[:n]) and torch.equal(a.chip_src[:n], b.chip_src[:n])


def test_every_loop_wraps(dev):
    """5 images x 300 rows at size 32: 1500 slots are two rounds of the select launch's 1024 lanes, and the valid ones are more (chip, tile)
    items than the resize launch has workgroups (1024), so its item loop runs twice in some of them."""
    rng = np.random.RandomState(77)
    sizes = [(96, 80), (61, 127), (128, 128), (75, 50), (90, 101)]
    host = [rng.randint(0, 256, size=(h, w, 3)).astype(np.uint8) for h, w in sizes]
    B, rows, S = 5, 300, 32
    dets = np.zeros((B, rows, 5), np.float32)
    for i, (h, w) in enumerate(sizes):
        x1, y1 = rng.uniform(-10, w - 2, rows), rng.uniform(-10, h - 2, rows)
        dets[i, :, 0], dets[i, :, 1] = x1, y1
        dets[i, :, 2], dets[i, :, 3] = x1 + rng.uniform(1, 70, rows), y1 + rng.uniform(1, 70, rows)
        dets[i, :, 4] = rng.uniform(0.0, 1.0, rows)
    num = [300, 290, 300, 0, 299]
    chips, src, count = R.reference(host, dets, num, S, 100, True, 0.05)
    assert count > 1024 and count < sum(num)                                                    # more items than workgroups; some rows dropped
    out = face_chips.extract([torch.from_numpy(a).to(dev) for a in host], torch.from_numpy(dets).to(dev),
                             torch.tensor(num, dtype=torch.int32, device=dev), size=S, margin=0.1, square=True, score_threshold=0.05)
    assert int(out.count.item()) == count
    assert np.array_equal(out.chip_src[:count].cpu().numpy(), src)
    assert np.array_equal(out.chips[:count].cpu().numpy(), np.stack(chips))
