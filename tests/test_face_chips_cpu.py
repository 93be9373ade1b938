"""Face chips without a GPU (dan_amd/utility/face_chips.py, csrc/face_chips_exact.hip): the rectangle rule on hand-traced boxes written out
as literal numbers, what danhip_face_chips_u8 refuses on the host (every call here fails its validation: nothing is launched, the pointers
are host addresses that are never used as device memory), the prototype table, and the evaluation commands' --chips_* flags."""
import ctypes
import json
import os

import numpy as np
import pytest

import face_chips_rule as R
from dan_amd import _lib
from dan_amd.utility.face_chips import margin_per_mille, rule

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H, W = 100, 200
MODELS = ("sfd", "pb", "dan", "dan_deform")


# ------------------------------------------------------------------------------------------------------------ the rule
def test_a_box_inside_the_image():
    # int() of the corners: (10, 20, 49, 40), w = 40, h = 21
    assert rule((10.7, 20.2, 49.9, 40.0), H, W, 0, False) == (10, 20, 49, 40)


def test_squaring_with_an_odd_difference_puts_the_smaller_half_in_front():
    # s = 40, s - h = 19: 9 rows above (y1 = 20 - 9 = 11), 10 below (y2 = 11 + 39 = 50)
    assert rule((10.7, 20.2, 49.9, 40.0), H, W, 0, True) == (10, 11, 49, 50)
    # the same on x: w = 4, h = 9, s - w = 5: 2 columns before (x1 = 48), 3 after (x2 = 56)
    assert rule((50.0, 30.0, 53.0, 38.0), H, W, 0, True) == (48, 30, 56, 38)


def test_negative_floats_are_truncated_toward_zero():
    # (-5.5, -2.5, -0.5, 3.0) -> (-5, -2, 0, 3): x2 = 0 keeps column 0 (floor would give x2 = -1, a box outside the image)
    assert rule((-5.5, -2.5, -0.5, 3.0), H, W, 0, False) == (0, 0, 0, 3)
    assert rule((-0.9, -3.7, 5.5, 6.2), H, W, 0, False) == (0, 0, 5, 6)


def test_margin_with_an_odd_product_is_floored():
    # w = 13, h = 21, 250 per mille: mx = 3250 // 1000 = 3, my = 5250 // 1000 = 5
    assert rule((10.0, 10.0, 22.0, 30.0), H, W, 250, False) == (7, 5, 25, 35)
    # squared after the margin: w' = 19, h' = 31, s = 31, x1 = 7 - 6 = 1, x2 = 1 + 30 = 31
    assert rule((10.0, 10.0, 22.0, 30.0), H, W, 250, True) == (1, 5, 31, 35)
    assert margin_per_mille(0.25) == 250 and margin_per_mille(0.0) == 0 and margin_per_mille(4.0) == 4000
    for bad in (-0.001, 4.001, float("inf"), float("nan")):
        with pytest.raises(ValueError):
            margin_per_mille(bad)


def test_clamping_at_each_of_the_four_edges():
    assert rule((-10.0, 10.0, 20.0, 30.0), H, W, 0, False) == (0, 10, 20, 30)
    assert rule((10.0, -10.0, 20.0, 30.0), H, W, 0, False) == (10, 0, 20, 30)
    assert rule((180.0, 10.0, 250.0, 30.0), H, W, 0, False) == (180, 10, 199, 30)
    assert rule((10.0, 80.0, 20.0, 130.0), H, W, 0, False) == (10, 80, 20, 99)
    # there is no zero padding: a squared box that leaves the image is cut, and is then no longer square
    assert rule((180.0, 10.0, 250.0, 30.0), H, W, 0, True) == (180, 0, 199, 55)          # s = 71, y1 = 10 - 25 = -15, y2 = 55
    # corners beyond +-2^30 are clamped there before any arithmetic
    assert rule((-3.0e9, 0.0, 3.0e9, 10.0), H, W, 4000, False) == (0, 0, 199, 54)          # h = 11, my = 44


def test_rows_that_give_no_chip():
    assert rule((300.0, 10.0, 320.0, 30.0), H, W, 0, True) is None                        # wholly outside, right
    assert rule((-50.0, -50.0, -10.0, -10.0), H, W, 0, True) is None                      # wholly outside, top left
    assert rule((20.0, 10.0, 19.0, 30.0), H, W, 0, True) is None                          # w = 0
    assert rule((20.0, 10.0, 19.0, 30.0), H, W, 4000, True) is None                       # ... whatever the margin
    assert rule((20.0, 30.0, 40.0, 29.9), H, W, 0, True) is None                          # h = 29 - 30 + 1 = 0
    assert rule((float("nan"), 10.0, 30.0, 30.0), H, W, 0, True) is None
    assert rule((10.0, 10.0, float("inf"), 30.0), H, W, 0, True) is None
    assert rule((10.0, float("-inf"), 30.0, 30.0), H, W, 0, True) is None


def test_a_score_equal_to_the_threshold_is_kept():
    image = np.arange(H * W * 3, dtype=np.uint32).astype(np.uint8).reshape(H, W, 3)
    thr = 0.3                                                                             # not a float32: the compare is on float32(thr)
    under = np.nextafter(np.float32(thr), np.float32(0))
    dets = np.array([[[10, 10, 20, 20, np.float32(thr)], [30, 30, 40, 40, under], [50, 50, 60, 60, 0.9], [70, 70, 80, 80, 1.0]]], np.float32)
    chips, src, count = R.reference([image], dets, [3], 4, score_threshold=thr)
    assert count == 2 and src.tolist() == [[0, 0, 10, 10, 20, 20], [0, 2, 50, 50, 60, 60]]  # row 1 under the threshold, row 3 beyond num
    assert R.reference([image], dets, [3], 4, score_threshold=thr, max_chips=1)[2] == 2
    assert len(R.reference([image], dets, [3], 4, score_threshold=thr, max_chips=1)[0]) == 1
    # a 1 x 1 crop resized is its pixel everywhere; an 11 x 11 crop at size 11 is the crop
    assert (R.chip_of(image, (7, 9, 7, 9), 5) == image[9, 7]).all()
    assert (chips[0] == R.chip_of(image, (10, 10, 20, 20), 4)).all() and (R.chip_of(image, (10, 10, 20, 20), 11) == image[10:21, 10:21]).all()


# ------------------------------------------------------------------------------------------------------------ the library
@pytest.fixture(scope="module")
def lib():
    return _lib.lib()


def test_prototype_table_lists_both_entries(lib):
    assert lib.danhip_version() >= 22
    for name in ("danhip_face_chips_workspace", "danhip_face_chips_u8"):
        assert name in _lib.PROTOTYPES and name in _lib.SIGNATURES
        fn = getattr(lib, name)
        assert fn.argtypes == _lib.SIGNATURES[name] and fn.restype is ctypes.c_int
    assert len(_lib.SIGNATURES["danhip_face_chips_u8"]) == 19


def test_workspace_query(lib):
    n = ctypes.c_size_t(77)
    assert lib.danhip_face_chips_workspace(8, 750, ctypes.byref(n)) == 0 and n.value == 0   # one looping workgroup: nothing to keep
    assert lib.danhip_face_chips_workspace(0, 0, ctypes.byref(n)) == 0
    assert lib.danhip_face_chips_workspace(-1, 5, ctypes.byref(n)) == -1 and lib.danhip_face_chips_workspace(5, -1, ctypes.byref(n)) == -1
    assert lib.danhip_face_chips_workspace(1 << 13, 1 << 12, ctypes.byref(n)) == -1 and b"2^24" in lib.danhip_last_error()
    assert lib.danhip_face_chips_workspace(8, 750, None) == -1


def test_validation_failures_launch_nothing(lib):
    buf = ctypes.create_string_buffer(4096)
    p = ctypes.addressof(buf)
    tab = (_lib.ResizeItem * 2)()
    nt = ctypes.c_int32(0)
    assert lib.danhip_resize_item_init(ctypes.byref(tab[0]), 0, 10, 20, 60, 0, 10, 20, 1.0, 1.0, 0, 0, ctypes.byref(nt)) == 0       # bytes [0, 600)
    assert lib.danhip_resize_item_init(ctypes.byref(tab[1]), 601, 7, 9, 30, 0, 7, 9, 1.0, 1.0, 0, 0, ctypes.byref(nt)) == 0        # [601, 808)

    def chips(host=ctypes.addressof(tab), dev=p, n=2, src=p, src_bytes=808, dets=p, num=p, rows=5, S=16, pm=0, square=1, thr=0.0, out=p,
              chip_src=p, count=p, max_chips=4, ws=None, ws_bytes=0):
        return lib.danhip_face_chips_u8(host, dev, n, src, src_bytes, dets, num, rows, S, pm, square, thr, out, chip_src, count, max_chips,
                                        ws, ws_bytes, None)
    for bad, word in ((dict(S=0), b"S 0"), (dict(S=-3), b"S -3"), (dict(S=1025), b"S 1025"), (dict(pm=-1), b"margin_pm"), (dict(pm=4001), b"margin_pm"),
                      (dict(square=2), b"square"), (dict(thr=float("nan")), b"NaN"), (dict(max_chips=-1), b"max_chips"),
                      (dict(n=-1), b"n_images"), (dict(rows=-1), b"rows_per_image"), (dict(n=1 << 13, rows=1 << 12), b"2^24"),
                      (dict(count=None), b"count_out"), (dict(host=None), b"NULL"), (dict(dev=None), b"NULL"), (dict(src=None), b"NULL"),
                      (dict(dets=None), b"NULL"), (dict(num=None), b"NULL"), (dict(out=None), b"chips_out"), (dict(chip_src=None), b"chips_out"),
                      (dict(src_bytes=807), b"image 1 reads past")):
        assert chips(**bad) == -1 and word in lib.danhip_last_error(), (bad, lib.danhip_last_error())
    tab[0].pitch = 59
    assert chips() == -1 and b"image 0" in lib.danhip_last_error()
    tab[0].pitch = 60
    tab[1].H = 0
    assert chips() == -1 and b"image 1" in lib.danhip_last_error()
    # the workspace the query asks for is 0 bytes: a NULL workspace passes that check and the call is refused for something else
    assert chips(ws=None, ws_bytes=0, S=0) == -1 and b"workspace" not in lib.danhip_last_error()


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


@pytest.mark.parametrize("flags, word", [(["--chips_size", "0"], "size 0 outside"), (["--chips_size", "1025"], "size 1025 outside"),
                                         (["--chips_margin", "-0.1"], "margin -0.1 outside"), (["--chips_margin", "4.5"], "margin 4.5 outside")])
def test_bad_chip_arguments_exit_before_the_device(flags, word, no_device, tmp_path):
    from dan_amd import eval_dan, eval_sfd
    for command in (eval_sfd, eval_dan):
        with pytest.raises(SystemExit, match=word):
            command.main(["--chips_dir", str(tmp_path / "chips"), "--data_dir", str(tmp_path), "--det_dir", str(tmp_path / "det")] + flags)
    assert not (tmp_path / "chips").exists() and not (tmp_path / "det").exists()


def test_help_names_the_flags_and_the_reference_set_does_not():
    from dan_amd import eval_cli
    golden = json.load(open(os.path.join(ROOT, "tests", "golden", "eval_flags.json")))
    for model in MODELS:
        text = eval_cli.build_parser(model).format_help()
        for flag in ("chips_dir", "chips_size", "chips_margin", "chips_threshold"):
            assert "--%s " % flag in text, (model, flag)
            assert flag not in golden[model] and flag not in eval_cli.REFERENCE_FLAGS
        args = eval_cli.build_parser(model).parse_args([])
        assert (args.chips_dir, args.chips_size, args.chips_margin, args.chips_threshold) == (None, 112, 0.0, None)
