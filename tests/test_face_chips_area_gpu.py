"""The extended face chips on the GPU (dan_amd/utility/face_chips.py extract(filter=, pad=, fill=) -> danhip_face_chips_u8_ex,
csrc/face_chips_exact.hip) against tests/face_chips_area_rule.py: chips, chip_src and count bit for bit.  Three images of odd sizes in ONE
buffer, each at an odd byte offset with rows further apart than 3 * W; boxes listed as literals, one per class of the extended rectangle
rule and of the two resampling forms, at sizes 1, 7, 16 and 112; then capacity, buffer reuse, the old entry point's bytes through the new
one, and one command-level run.  (tests/test_face_chips_gpu.py does not count launches, so no test here does: the two launches per call
are read off csrc/face_chips_exact.hip's entry point.)"""
import io
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import face_chips_area_rule as A  # noqa: E402
import face_chips_rule as R  # noqa: E402
from dan_amd.utility import face_chips  # noqa: E402

pytestmark = pytest.mark.gpu

SIZES = [(37, 53), (64, 48), (150, 200)]                    # (H, W)
PITCHES = [3 * 53 + 2, 3 * 48 + 7, 3 * 200 + 1]
THRESHOLD = 0.1
ROWS = 14
NUM = [9, 8, 13]
FILL = (200, 17, 96)
# (x1, y1, x2, y2, score), class
BOXES = [
    [((10.3, 8.9, 25.0, 20.5, 0.9), "interior"),                         # 16 x 13
     ((-6.0, 5.0, 12.0, 18.0, 0.8), "left edge"),
     ((20.0, -4.0, 30.7, 9.2, 0.8), "top edge"),
     ((40.0, 10.0, 58.0, 22.0, 0.8), "right edge"),
     ((15.0, 25.0, 28.0, 41.0, 0.8), "bottom edge"),
     ((45.0, 30.0, 60.0, 45.0, 0.7), "bottom-right corner"),
     ((-20.0, -30.0, 90.0, 80.0, 0.95), "larger than the image"),        # 111 x 111 around a 53 x 37 image
     ((60.0, 40.0, 70.0, 50.0, 0.9), "outside"),
     ((5.0, 5.0, 15.0, 15.0, 0.05), "under the threshold"),
     ((3.0, 3.0, 20.0, 20.0, 0.99), "beyond num"),
     ((float("nan"),) * 5, "beyond num")] + [((1.0, 1.0, 9.0, 9.0, 0.9), "beyond num")] * 3,
    [((-3.0, -5.0, 8.0, 6.0, 0.9), "top-left corner"),                   # 12 x 12
     ((5.5, 10.2, 30.9, 50.1, 0.9), "interior"),                         # 26 x 41
     ((47.0, 63.0, 47.0, 63.0, 0.6), "1 x 1 at the last pixel"),         # n == S for S = 1
     ((46.0, 62.0, 49.0, 65.0, 0.5), "bottom-right corner"),             # 4 x 4 with 2 x 2 inside
     ((10.0, 10.0, 11.0, 11.0, 0.1), "2 x 2"),                           # n == S + 1 for S = 1; the score equals the threshold: kept
     ((-40000.0, 10.0, 39000.0, 30.0, 0.9), "over the cap when padded"),  # 79001 wide; clipped it is 48 x 21
     ((20.0, 10.0, 19.0, 30.0, 0.9), "w = 0"),
     ((48.0, 10.0, 60.0, 30.0, 0.9), "outside")] + [((2.0, 2.0, 9.0, 9.0, 0.5), "beyond num")] * 6,
    [((0.0, 0.0, 199.0, 149.0, 1.0), "the whole image"),                 # 200 -> 16 is the ratio 12.5, 150 -> 16 is 9.375
     ((10.0, 10.0, 16.0, 16.0, 0.9), "side 7"),                          # n == S for S = 7
     ((10.0, 20.0, 17.0, 27.0, 0.9), "side 8"),                          # n == S + 1 for S = 7
     ((20.0, 20.0, 35.0, 35.0, 0.9), "side 16"),
     ((21.0, 20.0, 37.0, 36.0, 0.9), "side 17"),
     ((30.0, 30.0, 141.0, 141.0, 0.9), "side 112"),
     ((31.0, 30.0, 143.0, 142.0, 0.9), "side 113"),
     ((100.0, 70.0, 104.0, 74.0, 0.9), "side 5"),                        # n < S for S = 7, 16, 112
     ((150.0, 100.0, 260.0, 104.0, 0.9), "right edge"),                  # clipped: 50 x 5, shrinks on x and grows on y at S = 7 and 16
     ((-100.0, 39990.0, 40000.0, 40010.0, 0.9), "outside"),              # corners near 40000, below the image
     ((-100.0, -39000.0, 40000.0, 140.0, 0.9), "over the cap when padded"),   # clipped it is the 200 x 141 top of the image
     ((150.0, 100.0, 190.0, 140.0, 0.05), "under the threshold"),
     ((-30.0, 120.0, 25.0, 170.0, 0.3), "bottom-left corner"),           # 56 x 51
     ((1.0, 1.0, 30.0, 30.0, 0.99), "beyond num")],
]
NO_CHIP = ("outside", "under the threshold", "beyond num", "w = 0")
MODES = [("area", False), ("area", True), ("linear", True)]
CASES = [(S, f, p, 0, False) for S in (1, 7, 16, 112) for f, p in MODES] + [(16, "area", True, 250, True), (7, "linear", True, 250, True)]


@pytest.fixture(scope="module")
def case(dev):
    rng = np.random.RandomState(20250117)
    host = [rng.randint(0, 256, size=(h, w, 3)).astype(np.uint8) for h, w in SIZES]
    offsets, total = [], 1
    for (h, w), pitch in zip(SIZES, PITCHES):
        offsets.append(total)
        total += h * pitch + (h * pitch) % 2                                                   # the next image starts at an odd byte too
    buf = torch.full((total,), 0x5A, dtype=torch.uint8, device=dev)
    images = []
    for (h, w), pitch, off, a in zip(SIZES, PITCHES, offsets, host):
        view = torch.as_strided(buf, (h, w, 3), (pitch, 3, 1), storage_offset=off)
        view.copy_(torch.from_numpy(a).to(dev))
        assert view.data_ptr() % 2 == 1 and view.stride(0) > 3 * w
        images.append(view)
    dets = np.array([[b for b, _ in rows] for rows in BOXES], dtype=np.float32)
    assert dets.shape == (3, ROWS, 5)
    refs = {}

    def ref(S, filt, pad, pm, sq):                               # each reference is computed once and read by every test that needs it
        key = (S, filt, pad, pm, sq)
        if key not in refs:
            refs[key] = A.reference(host, dets, NUM, S, pm, sq, THRESHOLD, filter=filt, pad=pad, fill=FILL)
        return refs[key]
    return dict(host=host, images=images, dets_host=dets, dets=torch.from_numpy(dets).to(dev), num=torch.tensor(NUM, dtype=torch.int32, device=dev),
                ref=ref, keep=buf)


def _run(case, S, filt, pad, pm=0, sq=False, **kw):
    return face_chips.extract(case["images"], case["dets"], case["num"], size=S, margin=pm / 1000.0, square=sq, score_threshold=THRESHOLD,
                              filter=filt, pad=pad, fill=FILL, **kw)


def test_the_reference_has_a_chip_of_every_class(case):
    """The helper alone: no class of box may silently drop out of the comparisons below."""
    for pad in (False, True):
        chips, src, count = case["ref"](7, "area", pad, 0, False)
        got = {(int(i), int(r)) for i, r in src[:, :2]}
        for i, rows in enumerate(BOXES):
            for r, (_, cls) in enumerate(rows):
                gives = cls not in NO_CHIP and not (pad and cls == "over the cap when padded")
                assert ((i, r) in got) == gives, (pad, i, r, cls)
        assert count == len(chips) == (22 if pad else 24)
        by = {(int(s[0]), int(s[1])): tuple(int(v) for v in s[2:]) for s in src}
        if pad:
            assert by[(0, 1)] == (-6, 5, 12, 18) and by[(0, 2)] == (20, -4, 30, 9) and by[(0, 3)] == (40, 10, 58, 22) and by[(0, 4)] == (15, 25, 28, 41)
            assert by[(0, 5)] == (45, 30, 60, 45) and by[(0, 6)] == (-20, -30, 90, 80) and by[(1, 0)] == (-3, -5, 8, 6)
            assert by[(2, 12)] == (-30, 120, 25, 170)
        else:
            assert by[(0, 6)] == (0, 0, 52, 36) and by[(1, 5)] == (0, 10, 47, 30) and by[(2, 10)] == (0, 0, 199, 140)
            assert by[(2, 8)] == (150, 100, 199, 104)                                            # 50 x 5: a box on x, linear on y at S = 7 and 16
        assert by[(2, 0)] == (0, 0, 199, 149) and by[(2, 1)] == (10, 10, 16, 16) and by[(2, 2)] == (10, 20, 17, 27)


@pytest.mark.parametrize("S, filt, pad, pm, sq", CASES)
def test_chips_equal_the_reference(case, S, filt, pad, pm, sq):
    chips, src, count = case["ref"](S, filt, pad, pm, sq)
    out = _run(case, S, filt, pad, pm, sq)
    assert tuple(out.chips.shape) == (3 * ROWS, S, S, 3) and tuple(out.chip_src.shape) == (3 * ROWS, 6)
    assert int(out.count.item()) == count and count >= 20
    assert np.array_equal(out.chip_src[:count].cpu().numpy(), src)
    got = out.chips[:count].cpu().numpy()
    for k in range(count):
        assert np.array_equal(got[k], chips[k]), (k, src[k].tolist(), int(np.abs(got[k].astype(int) - chips[k]).max()))


@pytest.mark.parametrize("S, pm, sq", [(1, 0, False), (7, 250, True), (16, 0, False), (112, 0, True)])
def test_linear_without_padding_through_the_new_entry_point_gives_the_old_bytes(case, dev, S, pm, sq):
    old = face_chips.extract(case["images"], case["dets"], case["num"], size=S, margin=pm / 1000.0, square=sq, score_threshold=THRESHOLD)
    new = tuple(torch.full_like(t, 0x33) for t in old)
    # extract's defaults take the old entry point, so the new one is called as extract calls it
    from dan_amd._lib import call, ptr, stream
    import ctypes
    B = len(case["images"])
    nitem = ctypes.sizeof(face_chips.ResizeItem)
    base = min(im.data_ptr() for im in case["images"])
    end = max(im.data_ptr() + (im.shape[0] - 1) * im.stride(0) + 3 * im.shape[1] for im in case["images"])
    staging = torch.empty(B * nitem, dtype=torch.uint8)
    nt = ctypes.c_int32(0)
    for i, im in enumerate(case["images"]):
        call("danhip_resize_item_init", ctypes.c_void_p(staging.data_ptr() + i * nitem), im.data_ptr() - base, int(im.shape[0]), int(im.shape[1]),
             int(im.stride(0)), 0, int(im.shape[0]), int(im.shape[1]), 1.0, 1.0, 0, 0, ctypes.byref(nt))
    table = staging.to(dev)
    call("danhip_face_chips_u8_ex", ctypes.c_void_p(staging.data_ptr()), ptr(table), B, ctypes.c_void_p(base), end - base, ptr(case["dets"]),
         ptr(case["num"]), ROWS, S, pm, int(sq), THRESHOLD, ptr(new[0]), ptr(new[1]), ptr(new[2]), 3 * ROWS, None, 0, stream(), 0, 0, None)
    n = int(old.count.item())
    assert n == int(new[2].item()) == R.reference(case["host"], case["dets_host"], NUM, S, pm, sq, THRESHOLD)[2] and n >= 20
    assert torch.equal(old.chips[:n], new[0][:n]) and torch.equal(old.chip_src[:n], new[1][:n])
    assert bool((new[0][n:] == 0x33).all())


def _sentinel(dev, S, cap, extra=2):
    chips = torch.full((cap + extra, S, S, 3), 0xA5, dtype=torch.uint8, device=dev)
    src = torch.full((cap + extra, 6), -7, dtype=torch.int32, device=dev)
    count = torch.full((1,), -7, dtype=torch.int32, device=dev)
    return chips, src, count


@pytest.mark.parametrize("filt, pad", MODES)
def test_capacity_below_the_total_keeps_the_first_chips_and_the_true_count(case, dev, filt, pad):
    S, cap = 7, 5
    chips, src, count = case["ref"](S, filt, pad, 0, False)
    full = _sentinel(dev, S, cap)
    out = _run(case, S, filt, pad, max_chips=cap, out=(full[0][:cap], full[1][:cap], full[2]))
    assert int(out.count.item()) == count > cap
    assert np.array_equal(full[1][:cap].cpu().numpy(), src[:cap]) and np.array_equal(full[0][:cap].cpu().numpy(), np.stack(chips[:cap]))
    assert bool((full[0][cap:] == 0xA5).all()) and bool((full[1][cap:] == -7).all())
    assert len(sum(out.to_host(), [])) == cap


def test_buffers_of_one_call_are_reused_by_the_next(case):
    S = 16
    first = _run(case, S, "area", True)
    ptrs = [t.data_ptr() for t in first]
    first.chips.fill_(0x11)
    again = _run(case, S, "area", True, out=tuple(first))
    assert [t.data_ptr() for t in again] == ptrs
    chips, src, count = case["ref"](S, "area", True, 0, False)
    assert int(again.count.item()) == count and np.array_equal(again.chip_src[:count].cpu().numpy(), src)
    assert np.array_equal(again.chips[:count].cpu().numpy(), np.stack(chips)) and bool((again.chips[count:] == 0x11).all())
    # the same buffers, another form: nothing of the previous call shows through
    other = _run(case, S, "linear", True, out=tuple(first))
    chips, src, count = case["ref"](S, "linear", True, 0, False)
    assert int(other.count.item()) == count and np.array_equal(other.chips[:count].cpu().numpy(), np.stack(chips))


def test_no_detections_write_a_zero_count_and_nothing_else(case, dev):
    full = _sentinel(dev, 16, 3 * ROWS, extra=0)
    out = face_chips.extract(case["images"], case["dets"], torch.zeros_like(case["num"]), size=16, score_threshold=THRESHOLD, out=full,
                             filter="area", pad=True)
    assert int(out.count.item()) == 0 and bool((full[0] == 0xA5).all()) and bool((full[1] == -7).all())
    empty = face_chips.extract([], case["dets"][:0], case["num"][:0], size=16, filter="area", pad=True)
    assert int(empty.count.item()) == 0 and empty.to_host() == []


def test_a_row_wider_than_a_piece_and_a_size_of_two_column_tiles(case, dev):
    """The area kernel's other loops: a padded rectangle 5000 wide is read in two pieces (4096 pixels at most each), and at size 257 an
    output row is two items (256 columns at most each); at 257 a 600 x 600 rectangle is a box on both axes and a 40 x 40 one linear."""
    dets = np.array([[[-2400.0, 10.0, 2599.0, 29.0, 0.9], [-200.0, -225.0, 399.0, 374.0, 0.9], [60.0, 50.0, 99.0, 89.0, 0.9]]], np.float32)
    image, host = case["images"][2:], case["host"][2:]
    for S, rows in ((7, [0]), (257, [1, 2])):
        d = np.ascontiguousarray(dets[:, rows])
        n = torch.tensor([len(rows)], dtype=torch.int32, device=dev)
        chips, src, count = A.reference(host, d, [len(rows)], S, 0, False, filter="area", pad=True, fill=FILL)
        assert count == len(rows) and [int(s[4] - s[2] + 1) for s in src] == [[5000], [600, 40]][S == 257]
        out = face_chips.extract(image, torch.from_numpy(d).to(dev), n, size=S, square=False, filter="area", pad=True, fill=FILL)
        assert int(out.count.item()) == count and np.array_equal(out.chip_src[:count].cpu().numpy(), src)
        assert np.array_equal(out.chips[:count].cpu().numpy(), np.stack(chips)), S


def test_the_select_loop_wraps(case, dev):
    """3 images x 350 rows are two rounds of the select launch's 1024 lanes, with valid rows in both; the chips are tiny (size 2)."""
    rng = np.random.RandomState(31)
    B, rows, S = 3, 350, 2
    dets = np.zeros((B, rows, 5), np.float32)
    for i, (h, w) in enumerate(SIZES):
        x1, y1 = rng.uniform(-8, w + 2, rows), rng.uniform(-8, h + 2, rows)
        dets[i, :, 0], dets[i, :, 1] = x1, y1
        dets[i, :, 2], dets[i, :, 3] = x1 + rng.uniform(0, 7, rows), y1 + rng.uniform(0, 7, rows)
        dets[i, :, 4] = rng.uniform(0.0, 1.0, rows)
    num = [350, 0, 340]
    chips, src, count = A.reference(case["host"], dets, num, S, 100, True, 0.2, filter="area", pad=True, fill=FILL)
    assert 350 < count < sum(num) and (src[:, 0] == 2).sum() > 100 and (src[:, 2] < 0).any()
    out = face_chips.extract(case["images"], torch.from_numpy(dets).to(dev), torch.tensor(num, dtype=torch.int32, device=dev), size=S, margin=0.1,
                             square=True, score_threshold=0.2, filter="area", pad=True, fill=FILL)
    assert int(out.count.item()) == count
    assert np.array_equal(out.chip_src[:count].cpu().numpy(), src)
    assert np.array_equal(out.chips[:count].cpu().numpy(), np.stack(chips))


# ------------------------------------------------------------------------------------------------------------ the command
EVENT, NAMES = "0--Parade", ["0_Parade_a", "0_Parade_b"]
CLI_SIZES = [(120, 160), (97, 131)]
CLI_SIZE, CLI_MARGIN, MAX_PER_IMAGE = 24, 0.25, 30


def test_eval_sfd_writes_padded_area_chips(dev, tmp_path):
    """`python -m dan_amd.eval_sfd --chips_dir D --chips_filter area --chips_pad` on two synthetic JPEGs (a tree in the style of
    tests/test_eval_cli_chips_gpu.py): the files are the rows the extended rule keeps, each the reference chip through JpegEncoder."""
    import jpeg_encode_cases as C
    from dan_amd import eval_cli, eval_dan, eval_sfd
    from dan_amd.dataset.jpeg import JpegDecoder, JpegEncoder
    from dan_amd.utility import checkpoint
    root = tmp_path
    L = C.host_lib()
    d = root / "WIDER_val" / "images" / EVENT
    d.mkdir(parents=True)
    datas = []
    for k, name in enumerate(NAMES):
        h, w = CLI_SIZES[k]
        rng = np.random.RandomState(50 + k)
        img = (rng.rand(h // 8 + 1, w // 8 + 1, 3) * 255).astype(np.uint8).repeat(8, 0).repeat(8, 1)[:h, :w]
        datas.append(C.encode_host(L, np.ascontiguousarray(img), 92, 3))
        (d / (name + ".jpg")).write_bytes(datas[-1])
    (root / "list.txt").write_text("".join("%s/%s\n" % (EVENT, n) for n in NAMES))
    net = eval_cli.build_detector("sfd", dev, "act", seed=7)
    os.makedirs(str(root / "logs"))
    checkpoint.save_checkpoint(net.model.vs, str(root / "logs" / "model.ckpt-5"), "sfd", checksums=True)
    (root / "logs" / "checkpoint").write_text('model_checkpoint_path: "model.ckpt-5"\nall_model_checkpoint_paths: "model.ckpt-5"\n')
    images = [im.cpu().numpy() for im in JpegDecoder(dev).decode_batch(datas)]
    rows, real = [], eval_dan.detect_image_list

    def recording(*a, **k):                                       # the detections the command itself sees
        dets, num = real(*a, **k)
        rows.extend(dets[b, :int(num[b])].cpu().numpy() for b in range(dets.shape[0]))
        return dets, num
    eval_dan.detect_image_list = recording
    try:
        result = eval_sfd.main(["--data_dir", str(root), "--image_list", str(root / "list.txt"), "--checkpoint_path", str(root / "logs"), "--debug_dir", "",
                                "--batch_images", "2", "--max_per_image", str(MAX_PER_IMAGE), "--det_dir", str(root / "det"), "--chips_dir",
                                str(root / "chips"), "--chips_size", str(CLI_SIZE), "--chips_margin", str(CLI_MARGIN), "--chips_filter", "area",
                                "--chips_pad"], out=io.StringIO())
    finally:
        eval_dan.detect_image_list = real
    encoder = JpegEncoder(quality=75)
    want, leaving = {}, 0
    for b, name in enumerate(NAMES):
        det = rows[b]
        chips, src, count = A.reference([images[b]], det[None], [det.shape[0]], CLI_SIZE, 250, True, 0.01, filter="area", pad=True)
        assert count == len(chips)
        h, w = images[b].shape[:2]
        leaving += sum(1 for s in src if s[2] < 0 or s[3] < 0 or s[4] > w - 1 or s[5] > h - 1)
        for chip, s in zip(chips, src):
            want["%s_%d.jpg" % (name, int(s[1]))] = chip
    assert want and leaving > 0, "no detection of the seeded network leaves its image: the padding is not exercised"
    files = sorted(os.listdir(str(root / "chips" / EVENT)))
    assert files == sorted(want) and sorted(os.path.basename(p) for p in result["chips"]) == files
    for name, chip in want.items():
        assert (root / "chips" / EVENT / name).read_bytes() == encoder.encode(chip), name
