"""The extended face chips without a GPU (dan_amd/utility/face_chips.py, csrc/face_chips_exact.hip: danhip_face_chips_u8_ex): the axis
rule of filter "area" on hand-traced rows written out as literal numbers and by its properties, the rectangle rule with pad and the side
cap on hand-traced boxes, what the new entry point refuses on the host (every call here fails its validation: nothing is launched, the
pointers are host addresses that are never used as device memory), the prototype table, and the commands' two new flags."""
import ctypes

import numpy as np
import pytest

import face_chips_area_rule as A
import face_chips_rule as R
from dan_amd import _lib
from dan_amd.utility import face_chips
from dan_amd.utility.face_chips import MAX_SIDE, area_weights, rule

H, W = 100, 200
MODELS = ("sfd", "pb", "dan", "dan_deform")


# ------------------------------------------------------------------------------------------------------------ the axis rule
def test_box_rows_5_to_2_and_7_to_3():
    # n = 5, S = 2: position i covers [2i, 2i + 2), output j covers [5j, 5j + 5); position 2 = [4, 6) is split 1 : 1
    assert area_weights(5, 2, 0) == ([0, 1, 2], [2, 2, 1], 5)
    assert area_weights(5, 2, 1) == ([2, 3, 4], [1, 2, 2], 5)
    # n = 7, S = 3: position i covers [3i, 3i + 3), output j covers [7j, 7j + 7)
    assert area_weights(7, 3, 0) == ([0, 1, 2], [3, 3, 1], 7)            # [6, 9) meets [0, 7) in 1
    assert area_weights(7, 3, 1) == ([2, 3, 4], [2, 3, 2], 7)            # [6, 9) meets [7, 14) in 2, [12, 15) in 2
    assert area_weights(7, 3, 2) == ([4, 5, 6], [1, 3, 3], 7)


def test_one_more_source_than_outputs_is_a_box():
    # n = 5, S = 4: position i covers [4i, 4i + 4), output j covers [5j, 5j + 5)
    assert [area_weights(5, 4, j) for j in range(4)] == [([0, 1], [4, 1], 5), ([1, 2], [3, 2], 5), ([2, 3], [2, 3], 5), ([3, 4], [1, 4], 5)]


def test_equal_sizes_are_the_identity():
    assert [area_weights(3, 3, j) for j in range(3)] == [([0], [6], 6), ([1], [6], 6), ([2], [6], 6)]
    assert area_weights(1, 1, 0) == ([0], [2], 2)


def test_linear_rows_2_to_5_with_the_negative_t():
    # n = 2, S = 5, D = 10; t = 2 (2j + 1) - 5 = -3, 1, 5, 9, 13
    assert area_weights(2, 5, 0) == ([0], [10], 10)                      # i0 = floor(-3 / 10) = -1, f = 7: 3 on clamp(-1) = 0 and 7 on 0
    assert area_weights(2, 5, 1) == ([0, 1], [9, 1], 10)                 # i0 = 0, f = 1
    assert area_weights(2, 5, 2) == ([0, 1], [5, 5], 10)                 # the centre: halves
    assert area_weights(2, 5, 3) == ([0, 1], [1, 9], 10)
    assert area_weights(2, 5, 4) == ([1], [10], 10)                      # i0 = 1, f = 3: 7 on 1 and 3 on clamp(2) = 1
    assert area_weights(1, 4, 2) == ([0], [8], 8)                        # one source position: every tap is clamped onto it


def test_weights_sum_to_the_divisor_and_stay_inside_the_axis():
    for n in range(1, 41):
        for S in range(1, 41):
            last = -1
            for j in range(S):
                idx, w, D = area_weights(n, S, j)
                assert D == (n if n > S else 2 * S) and sum(w) == D and all(v > 0 for v in w), (n, S, j)
                assert idx == sorted(set(idx)) and 0 <= idx[0] and idx[-1] <= n - 1 and len(idx) <= (n + S - 1) // S + 1, (n, S, j)
                if n > S:                                                # a box: contiguous, starts where the previous output ended
                    assert idx == list(range(j * n // S, ((j + 1) * n - 1) // S + 1)) and idx[0] in (last, last + 1)
                    last = idx[-1]
            if n > S:
                assert last == n - 1
                per_source = [0] * n                                     # every source position is used S times in all
                for j in range(S):
                    idx, w, _ = area_weights(n, S, j)
                    for i, v in zip(idx, w):
                        per_source[i] += v
                assert per_source == [S] * n, (n, S)


# ------------------------------------------------------------------------------------------------------------ the area chip
@pytest.fixture(scope="module")
def image():
    return np.random.RandomState(5).randint(0, 256, size=(30, 41, 3)).astype(np.uint8)


def test_equal_size_on_both_axes_is_the_crop(image):
    assert np.array_equal(A.area_chip(image, (4, 6, 14, 16), 11), image[6:17, 4:15])


def test_an_integer_ratio_is_the_rounded_block_mean(image):
    for k, S in ((2, 5), (3, 4), (5, 2)):
        x1, y1 = 3, 2
        chip = A.area_chip(image, (x1, y1, x1 + k * S - 1, y1 + k * S - 1), S)
        block = image[y1:y1 + k * S, x1:x1 + k * S].astype(np.int64).reshape(S, k, S, k, 3).sum(axis=(1, 3))
        assert np.array_equal(chip, (block + k * k // 2) // (k * k)), k


def test_a_constant_image_gives_the_constant():
    const = np.empty((20, 23, 3), np.uint8)
    const[:] = (7, 130, 255)
    for rect, S in (((0, 0, 22, 19), 4), ((2, 3, 9, 8), 16), ((0, 0, 22, 19), 23), ((1, 1, 17, 3), 7)):      # the last shrinks on x and grows on y
        assert (A.area_chip(const, rect, S) == np.array([7, 130, 255])).all(), (rect, S)
    assert (A.area_chip(const, (-5, -4, 30, 25), 6, fill=(7, 130, 255)) == np.array([7, 130, 255])).all()      # padded with the same colour


def test_every_byte_lies_between_its_sources(image):
    for rect, S in (((0, 0, 40, 29), 7), ((5, 5, 12, 20), 9), ((3, 4, 6, 7), 16)):
        chip = A.area_chip(image, rect, S)
        x1, y1, x2, y2 = rect
        for jy in range(S):
            iy = area_weights(y2 - y1 + 1, S, jy)[0]
            for jx in range(S):
                ix = area_weights(x2 - x1 + 1, S, jx)[0]
                part = image[y1 + iy[0]:y1 + iy[-1] + 1, x1 + ix[0]:x1 + ix[-1] + 1].reshape(-1, 3)
                assert (part.min(axis=0) <= chip[jy, jx]).all() and (chip[jy, jx] <= part.max(axis=0)).all(), (rect, S, jy, jx)


def test_padding_reads_the_fill_colour(image):
    # a 2 x 2 block mean at the top-left corner with one row and one column outside: (p + 3 * fill + 2) // 4
    chip = A.area_chip(image, (-1, -1, 2, 2), 2, fill=(10, 20, 30))
    assert chip[0, 0].tolist() == [(int(image[0, 0, c]) + 3 * f + 2) // 4 for c, f in enumerate((10, 20, 30))]
    assert np.array_equal(chip[1, 1], (image[1:3, 1:3].astype(np.int64).sum(axis=(0, 1)) + 2) // 4)
    # the padded linear chip at the crop's own size is the padded crop
    lin = A.padded_linear_chip(image, (-2, 27, 3, 32), 6, fill=(9, 8, 7))
    assert np.array_equal(lin[:3, 2:], image[27:30, 0:4]) and (lin[3:] == np.array([9, 8, 7])).all() and (lin[:, :2] == np.array([9, 8, 7])).all()
    # without padding the two references agree with the old one
    assert np.array_equal(A.padded_linear_chip(image, (3, 4, 20, 25), 8), R.chip_of(image, (3, 4, 20, 25), 8))


# ------------------------------------------------------------------------------------------------------------ the rectangle rule
def test_pad_keeps_the_rectangle_across_each_edge_and_a_corner():
    assert rule((-10.0, 10.0, 20.0, 30.0), H, W, 0, False, pad=True) == (-10, 10, 20, 30)
    assert rule((10.0, -10.0, 20.0, 30.0), H, W, 0, False, pad=True) == (10, -10, 20, 30)
    assert rule((180.0, 10.0, 250.0, 30.0), H, W, 0, False, pad=True) == (180, 10, 250, 30)
    assert rule((10.0, 80.0, 20.0, 130.0), H, W, 0, False, pad=True) == (10, 80, 20, 130)
    assert rule((-5.5, -2.5, 10.0, 12.0), H, W, 0, False, pad=True) == (-5, -2, 10, 12)          # the top-left corner; int() toward zero
    # squared: s = 71, y1 = 10 - 25 = -15, y2 = 55: the square stays whole and centred (clipped it is (180, 0, 199, 55))
    assert rule((180.0, 10.0, 250.0, 30.0), H, W, 0, True, pad=True) == (180, -15, 250, 55)
    assert rule((180.0, 10.0, 250.0, 30.0), H, W, 0, True, pad=False, cap=MAX_SIDE) == (180, 0, 199, 55)
    # margin then square, across the bottom-right corner: w = h = 21, m = 5, (185, 85, 215, 115)
    assert rule((190.0, 90.0, 210.0, 110.0), H, W, 250, True, pad=True) == (185, 85, 215, 115)
    # a rectangle that only touches the image is kept: x2 = int(-0.5) = 0 is column 0
    assert rule((-5.5, -2.5, -0.5, 3.0), H, W, 0, False, pad=True) == (-5, -2, 0, 3)


def test_a_rectangle_outside_the_image_gives_no_chip_padded_or_not():
    for pad in (False, True):
        assert rule((300.0, 10.0, 320.0, 30.0), H, W, 0, True, pad=pad, cap=MAX_SIDE) is None
        assert rule((-50.0, -50.0, -10.0, -10.0), H, W, 0, True, pad=pad, cap=MAX_SIDE) is None
        assert rule((10.0, 100.0, 30.0, 120.0), H, W, 0, False, pad=pad, cap=MAX_SIDE) is None     # y1 = H
        assert rule((20.0, 10.0, 19.0, 30.0), H, W, 0, True, pad=pad, cap=MAX_SIDE) is None        # w = 0
        assert rule((float("nan"), 10.0, 30.0, 30.0), H, W, 0, True, pad=pad, cap=MAX_SIDE) is None


def test_the_side_cap():
    assert MAX_SIDE == 32768
    # padded: the unclipped side counts; w = 32768 is the last that is kept
    assert rule((-16000.0, 10.0, 16767.0, 30.0), H, W, 0, False, pad=True, cap=MAX_SIDE) == (-16000, 10, 16767, 30)
    assert rule((-16000.0, 10.0, 16768.0, 30.0), H, W, 0, False, pad=True, cap=MAX_SIDE) is None
    assert rule((-16000.0, 10.0, 16768.0, 30.0), H, W, 0, False, pad=True) == (-16000, 10, 16768, 30)     # no cap asked
    assert rule((0.0, 0.0, 40000.0, 40000.0), H, W, 0, True, pad=True, cap=MAX_SIDE) is None
    # squaring makes the short side long too: h = 21 -> s = 32769
    assert rule((-16000.0, 10.0, 16768.0, 30.0), H, W, 0, True, pad=True, cap=MAX_SIDE) is None
    # not padded: the clipped side counts, and an image of this size never reaches the cap
    assert rule((0.0, 0.0, 40000.0, 40000.0), H, W, 0, True, pad=False, cap=MAX_SIDE) == (0, 0, 199, 99)
    assert rule((0.0, 5.0, 40000.0, 8.0), 10, 40000, 0, False, pad=False, cap=MAX_SIDE) is None             # ... a 40000-wide one does
    assert rule((0.0, 5.0, 40000.0, 8.0), 10, 40000, 0, False) == (0, 5, 39999, 8)                          # the old entry point has none


def test_the_reference_numbers_rows_and_reports_the_true_count(image):
    dets = np.array([[[2, 2, 9, 9, 0.9], [-4, -4, 3, 3, 0.8], [100, 100, 110, 110, 0.9], [5, 5, 8, 8, 0.1], [0, 0, 40000, 40000, 0.9],
                      [1, 1, 4, 4, 0.9]]], np.float32)
    chips, src, count = A.reference([image], dets, [5], 4, score_threshold=0.5, filter="area", pad=True)
    assert count == 2 and src.tolist() == [[0, 0, 2, 2, 9, 9], [0, 1, -4, -4, 3, 3]]        # outside, under the threshold, over the cap, beyond num
    assert np.array_equal(chips[1], A.area_chip(image, (-4, -4, 3, 3), 4))
    one = A.reference([image], dets, [5], 4, score_threshold=0.5, max_chips=1, filter="area", pad=True)
    assert one[2] == 2 and len(one[0]) == 1 and one[1].tolist() == [[0, 0, 2, 2, 9, 9]]
    clipped = A.reference([image], dets, [5], 4, score_threshold=0.5, filter="linear", pad=False)
    old = R.reference([image], dets, [5], 4, score_threshold=0.5)
    assert clipped[2] == old[2] == 3 and np.array_equal(clipped[1], old[1]) and all(np.array_equal(a, b) for a, b in zip(clipped[0], old[0]))


# ------------------------------------------------------------------------------------------------------------ the Python interface
def test_extract_refuses_an_unknown_filter_and_a_bad_fill_before_anything_else():
    for bad in ("cubic", "AREA", None, 1):
        with pytest.raises(ValueError, match="filter"):
            face_chips.extract([], None, None, filter=bad)
    for bad in ((0, 0, 256), (-1, 0, 0), (0, 0), (0.5, 0, 0)):
        with pytest.raises(ValueError, match="fill"):
            face_chips.extract([], None, None, pad=True, fill=bad)
    with pytest.raises(TypeError):
        face_chips.extract([], None, None, 112, 0.0, True, 0.0, None, None, "area")            # keyword-only
    assert face_chips.FILTERS == {"linear": 0, "area": 1}


# ------------------------------------------------------------------------------------------------------------ the library
@pytest.fixture(scope="module")
def lib():
    return _lib.lib()


def test_prototype_table_lists_the_new_entries(lib):
    assert lib.danhip_version() >= 23
    for name in ("danhip_face_chips_ex_workspace", "danhip_face_chips_u8_ex"):
        assert name in _lib.PROTOTYPES and name in _lib.SIGNATURES
        fn = getattr(lib, name)
        assert fn.argtypes == _lib.SIGNATURES[name] and fn.restype is ctypes.c_int
    old, new = _lib.SIGNATURES["danhip_face_chips_u8"], _lib.SIGNATURES["danhip_face_chips_u8_ex"]
    assert len(old) == 19 and new[:19] == old and new[19:] == [_lib.I32, _lib.I32, _lib.P]


def test_workspace_query(lib):
    n = ctypes.c_size_t(77)
    for filt in (0, 1):
        assert lib.danhip_face_chips_ex_workspace(8, 750, 112, filt, ctypes.byref(n)) == 0 and n.value == 0     # the band lives in LDS
    assert lib.danhip_face_chips_ex_workspace(8, 750, 112, 2, ctypes.byref(n)) == -1 and b"filter 2" in lib.danhip_last_error()
    assert lib.danhip_face_chips_ex_workspace(8, 750, 112, -1, ctypes.byref(n)) == -1 and b"filter -1" in lib.danhip_last_error()
    assert lib.danhip_face_chips_ex_workspace(8, 750, 0, 1, ctypes.byref(n)) == -1 and b"S 0" in lib.danhip_last_error()
    assert lib.danhip_face_chips_ex_workspace(8, 750, 1025, 1, ctypes.byref(n)) == -1 and b"S 1025" in lib.danhip_last_error()
    assert lib.danhip_face_chips_ex_workspace(-1, 5, 16, 1, ctypes.byref(n)) == -1
    assert lib.danhip_face_chips_ex_workspace(1 << 13, 1 << 12, 16, 1, ctypes.byref(n)) == -1 and b"2^24" in lib.danhip_last_error()
    assert lib.danhip_face_chips_ex_workspace(8, 750, 16, 1, None) == -1


def test_validation_failures_launch_nothing(lib):
    buf = ctypes.create_string_buffer(4096)
    p = ctypes.addressof(buf)
    tab = (_lib.ResizeItem * 2)()
    nt = ctypes.c_int32(0)
    assert lib.danhip_resize_item_init(ctypes.byref(tab[0]), 0, 10, 20, 60, 0, 10, 20, 1.0, 1.0, 0, 0, ctypes.byref(nt)) == 0       # bytes [0, 600)
    assert lib.danhip_resize_item_init(ctypes.byref(tab[1]), 601, 7, 9, 30, 0, 7, 9, 1.0, 1.0, 0, 0, ctypes.byref(nt)) == 0        # [601, 808)
    fill = (ctypes.c_uint8 * 3)(1, 2, 3)

    def chips(host=ctypes.addressof(tab), dev=p, n=2, src=p, src_bytes=808, dets=p, num=p, rows=5, S=16, pm=0, square=1, thr=0.0, out=p,
              chip_src=p, count=p, max_chips=4, ws=None, ws_bytes=0, filt=1, pad=1, fill=fill):
        return lib.danhip_face_chips_u8_ex(host, dev, n, src, src_bytes, dets, num, rows, S, pm, square, thr, out, chip_src, count, max_chips,
                                           ws, ws_bytes, None, filt, pad, fill)
    for bad, word in ((dict(filt=2), b"filter 2"), (dict(filt=-1), b"filter -1"), (dict(pad=2), b"pad"), (dict(pad=-1), b"pad"),
                      (dict(S=0), b"S 0"), (dict(S=-3), b"S -3"), (dict(S=1025), b"S 1025"), (dict(pm=-1), b"margin_pm"), (dict(pm=4001), b"margin_pm"),
                      (dict(square=2), b"square"), (dict(thr=float("nan")), b"NaN"), (dict(max_chips=-1), b"max_chips"),
                      (dict(n=-1), b"n_images"), (dict(rows=-1), b"rows_per_image"), (dict(n=1 << 13, rows=1 << 12), b"2^24"),
                      (dict(count=None), b"count_out"), (dict(host=None), b"NULL"), (dict(dev=None), b"NULL"), (dict(src=None), b"NULL"),
                      (dict(dets=None), b"NULL"), (dict(num=None), b"NULL"), (dict(out=None), b"chips_out"), (dict(chip_src=None), b"chips_out"),
                      (dict(src_bytes=807), b"image 1 reads past")):
        for filt_pad in (dict(), dict(filt=0, pad=0), dict(filt=0, pad=1, fill=None)):
            kw = dict(filt_pad, **bad)
            assert chips(**kw) == -1 and word in lib.danhip_last_error(), (kw, lib.danhip_last_error())
    tab[0].pitch = 59
    assert chips() == -1 and b"image 0" in lib.danhip_last_error()
    tab[0].pitch = 60
    tab[1].H = 0
    assert chips() == -1 and b"image 1" in lib.danhip_last_error()


# ------------------------------------------------------------------------------------------------------------ the commands
@pytest.fixture
def no_device(monkeypatch):
    """any use of the device from here on fails the test"""
    import torch

    def touched(*a, **k):
        raise AssertionError("the device was touched")
    for name in ("set_device", "init", "current_stream", "synchronize"):
        monkeypatch.setattr(torch.cuda, name, touched)
    monkeypatch.setattr(_lib, "lib", touched)


@pytest.mark.parametrize("flags", [["--chips_filter", "cubic"], ["--chips_filter", "AREA"], ["--chips_filter"], ["--chips_pad", "1"]])
def test_bad_values_of_the_new_flags_exit_before_the_device(flags, no_device, tmp_path, capsys):
    from dan_amd import eval_dan, eval_sfd
    for command in (eval_sfd, eval_dan):
        with pytest.raises(SystemExit) as e:
            command.main(["--chips_dir", str(tmp_path / "chips"), "--data_dir", str(tmp_path), "--det_dir", str(tmp_path / "det")] + flags)
        assert e.value.code == 2                                             # the argument parser's own refusal
        error = capsys.readouterr().err.splitlines()[-1]                     # (the usage text above it names every flag)
        assert ("--chips_filter" in error) if flags[0] == "--chips_filter" else ("unrecognized arguments: 1" in error)
    assert not (tmp_path / "chips").exists() and not (tmp_path / "det").exists()


def test_the_new_flags_leave_the_earlier_checks_in_front_of_the_device(no_device, tmp_path):
    from dan_amd import eval_sfd
    with pytest.raises(SystemExit, match="size 0 outside"):
        eval_sfd.main(["--chips_dir", str(tmp_path / "chips"), "--data_dir", str(tmp_path), "--det_dir", str(tmp_path / "det"), "--chips_filter", "area",
                       "--chips_pad", "--chips_size", "0"])
    assert not (tmp_path / "chips").exists() and not (tmp_path / "det").exists()


def test_help_names_the_flags_and_their_defaults():
    from dan_amd import eval_cli
    for model in MODELS:
        text = eval_cli.build_parser(model).format_help()
        assert "--chips_filter {linear,area}" in text and "--chips_pad" in text, model
        assert "chips_filter" not in eval_cli.REFERENCE_FLAGS and "chips_pad" not in eval_cli.REFERENCE_FLAGS
        args = eval_cli.build_parser(model).parse_args([])
        assert (args.chips_filter, args.chips_pad) == ("linear", False)
        assert (args.chips_dir, args.chips_size, args.chips_margin, args.chips_threshold) == (None, 112, 0.0, None)      # the earlier four
        args = eval_cli.build_parser(model).parse_args(["--chips_filter", "area", "--chips_pad"])
        assert (args.chips_filter, args.chips_pad) == ("area", True)
