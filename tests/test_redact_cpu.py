"""Face redaction without a device: the rule (dan_amd/utility/redact.py rule_pixel / reference and tests/redact_rule.py) on hand-traced
answers, the exported index arithmetic of the item walk (csrc/redact_walk.h through danhip_redact_extent / _item_count / _tile / _window /
_cell / _in_shape) against the Python rule for every small (side, e, band, strip), every refusal of danhip_redact_u8 (host addresses that
are never dereferenced), the prototype table and the commands' flags."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import redact_rule as R  # noqa: E402
from dan_amd import _lib  # noqa: E402
from dan_amd.utility import redact  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODELS = ("sfd", "pb", "dan", "dan_deform")


def ramp(H, W):
    """channel 0 = 10 * y + x, channel 1 = 255 - that, channel 2 = 7"""
    im = np.empty((H, W, 3), np.uint8)
    im[..., 0] = 10 * np.arange(H)[:, None] + np.arange(W)[None, :]
    im[..., 1] = 255 - im[..., 0]
    im[..., 2] = 7
    return im


def both(image, rows, **kw):
    """redact.reference and tests/redact_rule.py on one image: they agree, and rule_pixel agrees on every pixel"""
    a, n = redact.reference(image, rows, **kw)
    b, m = R.redact_image(image, rows, len(rows), **{("threshold" if k == "score_threshold" else k): v for k, v in kw.items()})
    assert n == m and np.array_equal(a, b)
    for py in range(image.shape[0]):
        for px in range(image.shape[1]):
            assert redact.rule_pixel(image, rows, px, py, **kw) == tuple(a[py, px]), (px, py)
    return a


# ------------------------------------------------------------------------------------------------------------ hand-traced answers
def test_blur_of_a_5_by_4_image_at_a_corner_an_edge_and_the_interior():
    im = ramp(4, 5)
    out = both(im, [[0, 0, 4, 3, 0.9]], strength_pm=1)           # e = max(5 * 1 // 1000, 1) = 1
    # corner (0, 0): 0 + 1 + 10 + 11 = 22 over A = 4; edge (2, 0): 1 + 2 + 3 + 11 + 12 + 13 = 42 over 6; interior (2, 1): 108 over 9
    assert out[0, 0].tolist() == [(22 + 2) // 4, (4 * 255 - 22 + 2) // 4, 7] == [6, 250, 7]
    assert out[0, 2].tolist() == [(42 + 3) // 6, (6 * 255 - 42 + 3) // 6, 7] == [7, 248, 7]
    assert out[1, 2].tolist() == [(108 + 4) // 9, (9 * 255 - 108 + 4) // 9, 7] == [12, 243, 7]
    lib = _lib.lib()
    w = (ctypes.c_int32 * 5)()
    for (px, py), A in (((0, 0), 4), ((2, 0), 6), ((2, 1), 9), ((4, 3), 4), ((4, 1), 6)):
        assert lib.danhip_redact_window(4, 5, 1, px, py, w) == 0 and w[4] == A


def test_a_sum_on_one_half_rounds_up():
    im = np.zeros((2, 2, 3), np.uint8)
    im[0, 0] = im[1, 1] = (1, 3, 255)                            # every window is the whole image: sums 2, 6, 510 over A = 4
    out = both(im, [[0, 0, 1, 1, 1.0]], strength_pm=1)
    assert (out == np.array([1, 2, 128], np.uint8)).all()        # 0.5 -> 1, 1.5 -> 2, 127.5 -> 128
    out = both(im, [[0, 0, 1, 1, 1.0]], strength_pm=1, mode="mosaic")
    assert (out == np.array([1, 2, 128], np.uint8)).all()


def test_mosaic_whose_last_cell_column_is_one_pixel_wide():
    im = ramp(2, 5)
    out = both(im, [[0, 0, 4, 1, 0.9]], strength_pm=1, mode="mosaic")        # c = max(2, 1) = 2: columns [0, 1], [2, 3], [4]
    assert out[..., 0].tolist() == [[6, 6, 8, 8, 9]] * 2          # (22 + 2) // 4, (30 + 2) // 4, (4 + 14 + 1) // 2
    assert (out[..., 2] == 7).all()
    lib = _lib.lib()
    rect, cell = (ctypes.c_int32 * 4)(0, 0, 4, 1), (ctypes.c_int32 * 5)()
    assert lib.danhip_redact_item_count(1, rect, 1, 64, 256) == 3
    assert lib.danhip_redact_cell(rect, 2, 2, cell) == 0 and list(cell) == [4, 0, 4, 1, 2]


def test_ellipse_membership_written_out():
    def bits(wc, hc):
        return ["".join("1" if redact.in_shape("ellipse", (3, 2, 3 + wc - 1, 2 + hc - 1), 3 + x, 2 + y) else "0" for x in range(wc)) for y in range(hc)]
    assert bits(4, 3) == ["0110", "1111", "0110"]                # corner: 9 * 9 + 4 * 16 = 145 > 144
    assert bits(5, 5) == ["01110", "11111", "11111", "11111", "01110"]       # 16 + 4 <= 25 < 16 + 16
    for wc, hc in ((4, 3), (5, 5)):
        assert ["".join("1" if v else "0" for v in row) for row in R.shape_mask("ellipse", wc, hc)] == bits(wc, hc)
    assert not redact.in_shape("ellipse", (3, 2, 6, 4), 2, 3) and not redact.in_shape("rect", (3, 2, 6, 4), 7, 3)          # outside the rectangle
    assert R.shape_mask("rect", 4, 3).all()


def test_extent_is_clamped_at_1_and_at_255():
    lib = _lib.lib()
    for wc, hc, pm, e in ((5, 4, 1, 1), (999, 3, 1, 1), (1000, 3, 1, 1), (2000, 3, 1, 2), (400, 300, 125, 50), (300, 400, 125, 50),
                          (2039, 1, 125, 254), (2040, 1, 125, 255), (2048, 1, 125, 255), (32768, 10, 1000, 255), (255, 255, 1000, 255),
                          (254, 100, 1000, 254), (1, 1, 1000, 1)):
        assert redact.extent(wc, hc, pm) == e == R.extent((0, 0, wc - 1, hc - 1), pm) == lib.danhip_redact_extent(wc, hc, pm), (wc, hc, pm)
    for bad in ((0, 1, 1), (1, 32769, 1), (1, 1, 0), (1, 1, 1001)):
        assert lib.danhip_redact_extent(*bad) == -1
    assert redact.MAX_EXTENT == 255 and 255 * 511 * 511 < 2 ** 32


def test_a_pixel_under_three_rows_belongs_to_the_last_valid_one():
    im = ramp(4, 4)
    rows = [[0, 0, 3, 3, 0.9], [float("nan"), 0, 3, 3, 0.9], [1, 1, 2, 2, 0.9]]
    out = both(im, rows, strength_pm=1, mode="mosaic")
    assert out[1, 1, 0] == (11 + 12 + 21 + 22 + 2) // 4 == 17    # row 2's one cell
    assert out[0, 0, 0] == out[1, 0, 0] == (0 + 1 + 10 + 11 + 2) // 4 == 6      # row 0's first cell, where row 2 is not
    two = redact.reference(im, rows, num=2, strength_pm=1, mode="mosaic")
    assert two[1] == 1 and two[0][1, 1, 0] == 6                  # the invalid middle row owns nothing: row 0
    rows[2][4] = 0.1
    assert both(im, rows, strength_pm=1, mode="mosaic", score_threshold=0.5)[1, 1, 0] == 6
    assert both(im, [rows[0], rows[2], rows[0]], strength_pm=1, mode="fill", fill=(1, 2, 3)).reshape(-1, 3).tolist() == [[1, 2, 3]] * 16


def test_the_two_restatements_agree_on_random_scenes():
    rng = np.random.RandomState(3)
    im = rng.randint(0, 256, (9, 11, 3)).astype(np.uint8)
    rows = [[1, 1, 6, 7, 0.9], [4, -3, 30, 5, 0.5], [8, 6, 10, 8, 0.3], [20, 20, 30, 30, 0.9], [2, 2, float("inf"), 4, 0.9]]
    for mode in redact.MODES:
        for shape in redact.SHAPES:
            for pm, margin in ((1, 0), (400, 0), (1000, 250)):
                both(im, rows, mode=mode, shape=shape, strength_pm=pm, margin_pm=margin, score_threshold=0.4, fill=(9, 8, 7))


# ------------------------------------------------------------------------------------------------------------ the exported walk
def header_constant(name):
    with open(os.path.join(ROOT, "include", "danhip.h")) as f:
        return int(re.search(r"#define\s+%s\s+(\d+)" % name, f.read()).group(1))


def test_the_python_constants_are_the_headers():
    assert redact.BAND == header_constant("DANHIP_REDACT_BAND") and redact.STRIP == header_constant("DANHIP_REDACT_STRIP")
    assert redact.MAX_EXTENT == header_constant("DANHIP_REDACT_MAX_EXTENT") and redact.LAUNCHES == header_constant("DANHIP_REDACT_LAUNCHES")
    assert redact.MAX_SIDE == header_constant("DANHIP_FACE_CHIPS_MAX_SIDE")
    assert redact.MODES == {n: header_constant("DANHIP_REDACT_" + n.upper()) for n in ("blur", "mosaic", "fill")}
    assert redact.SHAPES == {n: header_constant("DANHIP_REDACT_" + n.upper()) for n in ("rect", "ellipse")}
    assert (redact.STRIP + 2 * redact.MAX_EXTENT) * 3 * 4 == 9192            # the LDS bytes of a blur item's column sums


def test_the_tile_walk_covers_each_rectangle_once_reads_inside_the_image_and_counts_as_the_rule():
    lib = _lib.lib()
    out, win = (ctypes.c_int32 * 8)(), (ctypes.c_int32 * 5)()
    checked = 0
    for wc in range(1, 7):
        for hc in (1, 2, 5):
            for ox, oy, H, W in ((0, 0, hc, wc), (2, 1, hc + 3, wc + 4)):      # the rectangle is the image / lies inside a larger one
                rect = (ctypes.c_int32 * 4)(ox, oy, ox + wc - 1, oy + hc - 1)
                for e in (1, 2, 3, 7):
                    for band in (1, 2, 3, 5):
                        for strip in (1, 2, 4, 6):
                            n = lib.danhip_redact_item_count(0, rect, e, band, strip)
                            assert n == -(-wc // strip) * -(-hc // band) == lib.danhip_redact_item_count(2, rect, e, band, strip)
                            seen = np.zeros((H, W), np.int32)
                            for item in range(n):
                                assert lib.danhip_redact_tile(H, W, rect, e, band, strip, item, out) == 0
                                tx1, ty1, tx2, ty2, sx1, sy1, sx2, sy2 = out
                                assert ox <= tx1 <= tx2 <= ox + wc - 1 and oy <= ty1 <= ty2 <= oy + hc - 1
                                assert tx2 - tx1 < strip and ty2 - ty1 < band
                                assert 0 <= sx1 <= sx2 <= W - 1 and 0 <= sy1 <= sy2 <= H - 1          # every source row and column is in the image
                                assert (sx1, sy1, sx2, sy2) == (max(tx1 - e, 0), max(ty1 - e, 0), min(tx2 + e, W - 1), min(ty2 + e, H - 1))
                                seen[ty1:ty2 + 1, tx1:tx2 + 1] += 1
                                for py in range(ty1, ty2 + 1):
                                    for px in range(tx1, tx2 + 1):
                                        assert lib.danhip_redact_window(H, W, e, px, py, win) == 0
                                        lo_x, lo_y, hi_x, hi_y, A = win
                                        assert sx1 <= lo_x <= hi_x <= sx2 and sy1 <= lo_y <= hi_y <= sy2       # the window lies in what the item reads
                                        inside = sum(1 for y in range(py - e, py + e + 1) for x in range(px - e, px + e + 1) if 0 <= y < H and 0 <= x < W)
                                        assert A == inside and (lo_x, lo_y, hi_x, hi_y) == (max(px - e, 0), max(py - e, 0), min(px + e, W - 1), min(py + e, H - 1))
                                        checked += 1
                            want = np.zeros((H, W), np.int32)
                            want[oy:oy + hc, ox:ox + wc] = 1
                            assert np.array_equal(seen, want)
                            assert lib.danhip_redact_tile(H, W, rect, e, band, strip, n, out) == -1 and lib.danhip_redact_tile(H, W, rect, e, band, strip, -1, out) == -1
    assert checked > 20000
    # the kernel's own tile at the largest extent: the halo never exceeds STRIP + 2 * MAX_EXTENT columns
    rect = (ctypes.c_int32 * 4)(100, 50, 100 + 2 * redact.STRIP, 50 + 2 * redact.BAND)
    assert lib.danhip_redact_item_count(0, rect, 255, redact.BAND, redact.STRIP) == 9
    for item in range(9):
        assert lib.danhip_redact_tile(4000, 5000, rect, 255, redact.BAND, redact.STRIP, item, out) == 0
        assert out[6] - out[4] + 1 <= redact.STRIP + 2 * redact.MAX_EXTENT and out[7] - out[5] + 1 <= redact.BAND + 2 * redact.MAX_EXTENT


def test_the_cell_walk_and_the_shape_are_the_rules():
    lib = _lib.lib()
    cell = (ctypes.c_int32 * 5)()
    for wc in range(1, 10):
        for hc in (1, 3, 4, 9):
            rect = (ctypes.c_int32 * 4)(3, 2, 3 + wc - 1, 2 + hc - 1)
            for c in (2, 3, 4, 5, 255):
                n = lib.danhip_redact_item_count(1, rect, c, 64, 256)        # e = c >= 2: the cell side is e
                assert n == -(-wc // c) * -(-hc // c)
                owner = np.full((hc, wc), -1)
                for q in range(n):
                    assert lib.danhip_redact_cell(rect, c, q, cell) == 0
                    cx1, cy1, cx2, cy2, A = cell
                    assert A == (cx2 - cx1 + 1) * (cy2 - cy1 + 1) and (owner[cy1 - 2:cy2 - 1, cx1 - 3:cx2 - 2] == -1).all()
                    owner[cy1 - 2:cy2 - 1, cx1 - 3:cx2 - 2] = q
                    assert (cx1 - 3) % c == 0 and (cy1 - 2) % c == 0 and cx2 == min(cx1 + c - 1, 3 + wc - 1) and cy2 == min(cy1 + c - 1, 2 + hc - 1)
                for y in range(hc):
                    for x in range(wc):
                        assert owner[y, x] == (y // c) * -(-wc // c) + x // c       # the rule's cell of the pixel, row-major
                assert lib.danhip_redact_cell(rect, c, n, cell) == -1
            for shape, name in ((0, "rect"), (1, "ellipse")):
                for py in range(1, 2 + hc + 1):
                    for px in range(2, 3 + wc + 1):
                        assert lib.danhip_redact_in_shape(shape, rect, px, py) == int(redact.in_shape(name, tuple(rect), px, py))
    big = (ctypes.c_int32 * 4)(0, 0, 32767, 32767)               # the largest sides: the 64-bit products stay exact
    for px, py in ((0, 0), (4798, 4798), (4799, 4799), (16383, 0), (32767, 16384), (32767, 32767)):
        assert lib.danhip_redact_in_shape(1, big, px, py) == int(redact.in_shape("ellipse", tuple(big), px, py))
    assert lib.danhip_redact_in_shape(2, big, 0, 0) == -1 and lib.danhip_redact_item_count(3, big, 1, 64, 256) == -1
    assert lib.danhip_redact_item_count(1, big, 1, 64, 256) == 16384 * 16384


# ------------------------------------------------------------------------------------------------------------ the library
def test_prototype_table_lists_the_new_entries():
    lib = _lib.lib()
    assert lib.danhip_version() >= 24
    for name in ("danhip_redact_workspace", "danhip_redact_u8"):
        assert name in _lib.PROTOTYPES and name in _lib.SIGNATURES
        fn = getattr(lib, name)
        assert fn.argtypes == _lib.SIGNATURES[name] and fn.restype is ctypes.c_int
    assert len(_lib.SIGNATURES["danhip_redact_u8"]) == 22
    for name in ("danhip_redact_extent", "danhip_redact_item_count", "danhip_redact_tile", "danhip_redact_window", "danhip_redact_cell",
                 "danhip_redact_in_shape"):
        assert name in _lib.PROTOTYPES and getattr(lib, name).argtypes == _lib.PROTOTYPES[name][1]
    assert _lib.PROTOTYPES["danhip_redact_item_count"][0] is ctypes.c_int64


def test_workspace_query():
    lib = _lib.lib()
    n = ctypes.c_size_t(77)
    assert lib.danhip_redact_workspace(8, 750, ctypes.byref(n)) == 0 and n.value == 16 + 8 * 750 * 40
    assert lib.danhip_redact_workspace(0, 0, ctypes.byref(n)) == 0 and n.value == 16
    assert lib.danhip_redact_workspace(-1, 5, ctypes.byref(n)) == -1 and lib.danhip_redact_workspace(5, -1, ctypes.byref(n)) == -1
    assert lib.danhip_redact_workspace(1 << 13, 1 << 12, ctypes.byref(n)) == -1 and b"2^24" in lib.danhip_last_error()
    assert lib.danhip_redact_workspace(8, 750, None) == -1


def test_validation_failures_launch_nothing():
    lib = _lib.lib()
    buf = ctypes.create_string_buffer(8192)
    p = (ctypes.addressof(buf) + 15) // 16 * 16
    q = p + 2048                                                 # the destination "buffer": 808 bytes apart from the source's
    ws = p + 4096
    src_tab, dst_tab = (_lib.ResizeItem * 2)(), (_lib.ResizeItem * 2)()
    nt = ctypes.c_int32(0)
    for tab in (src_tab, dst_tab):
        assert lib.danhip_resize_item_init(ctypes.byref(tab[0]), 0, 10, 20, 60, 0, 10, 20, 1.0, 1.0, 0, 0, ctypes.byref(nt)) == 0       # bytes [0, 600)
        assert lib.danhip_resize_item_init(ctypes.byref(tab[1]), 601, 7, 9, 30, 0, 7, 9, 1.0, 1.0, 0, 0, ctypes.byref(nt)) == 0        # [601, 808)
    fill = (ctypes.c_uint8 * 3)(1, 2, 3)

    def call(host=ctypes.addressof(src_tab), dev=p, n=2, src=p, src_bytes=808, dets=p, num=p, rows=5, mode=0, shape=0, strength=125, pm=0, thr=0.0,
             fill=fill, dhost=ctypes.addressof(dst_tab), ddev=p, dst=q, dst_bytes=808, count=p, ws=ws, ws_bytes=16 + 10 * 40):
        return lib.danhip_redact_u8(host, dev, n, src, src_bytes, dets, num, rows, mode, shape, strength, pm, thr, fill, dhost, ddev, dst,
                                    dst_bytes, count, ws, ws_bytes, None)
    for bad, word in ((dict(mode=3), b"mode 3"), (dict(mode=-1), b"mode -1"), (dict(shape=2), b"shape 2"), (dict(shape=-1), b"shape -1"),
                      (dict(strength=0), b"strength_pm 0"), (dict(strength=1001), b"strength_pm 1001"), (dict(pm=-1), b"margin_pm"),
                      (dict(pm=4001), b"margin_pm"), (dict(thr=float("nan")), b"NaN"), (dict(n=-1), b"n_images"), (dict(rows=-1), b"rows_per_image"),
                      (dict(n=1 << 13, rows=1 << 12), b"2^24"), (dict(fill=None), b"fill_rgb"), (dict(count=None), b"count_out"),
                      (dict(host=None), b"NULL"), (dict(dev=None), b"NULL"), (dict(src=None), b"NULL"), (dict(dhost=None), b"NULL"),
                      (dict(ddev=None), b"NULL"), (dict(dst=None), b"NULL"), (dict(dets=None), b"dets"), (dict(num=None), b"dets"),
                      (dict(ws=None), b"workspace"), (dict(ws_bytes=16 + 10 * 40 - 1), b"workspace"), (dict(ws=ws + 4), b"workspace"),
                      (dict(src_bytes=807), b"image 1 reads past"), (dict(dst_bytes=807), b"destination 1 writes past"),
                      (dict(dst=p + 807), b"overlaps source"), (dict(dst=p - 807, dst_bytes=808), b"overlaps source"),
                      (dict(dst=p + 300, dst_bytes=808), b"overlaps source"), (dict(dst=p), b"overlaps source")):
        for mode_shape in (dict(), dict(mode=1, shape=1), dict(mode=2)):
            kw = dict(mode_shape, **bad)
            assert call(**kw) == -1 and word in lib.danhip_last_error(), (kw, lib.danhip_last_error())
    src_tab[0].pitch = 59
    assert call() == -1 and b"image 0" in lib.danhip_last_error()
    src_tab[0].pitch = 60
    src_tab[1].H = 0
    assert call() == -1 and b"image 1" in lib.danhip_last_error()
    src_tab[1].H = 7
    dst_tab[1].W = 8                                             # a destination of another size
    assert call() == -1 and b"destination 1 is 7 x 8" in lib.danhip_last_error()
    dst_tab[1].W = 9
    dst_tab[0].pitch = 59
    assert call() == -1 and b"destination 0" in lib.danhip_last_error()
    dst_tab[0].pitch = 60
    dst_tab[1].src_offset = 599                                  # one byte into destination 0
    assert call() == -1 and b"destinations 0 and 1 overlap" in lib.danhip_last_error()
    dst_tab[1].src_offset = 600                                  # flush against it: no overlap (and no further refusal but the launch itself)
    dst_tab[1].src_offset = 601
    assert call(n=0, host=None, dev=None, src=None, dets=None, num=None, dhost=None, ddev=None, dst=None, ws=None, ws_bytes=0) == 0      # nothing to do


def test_apply_refuses_bad_values_before_any_device_call(monkeypatch):
    def touched(*a, **k):
        raise AssertionError("the device was touched")
    monkeypatch.setattr(_lib, "lib", touched)
    monkeypatch.setattr(redact, "call", touched)
    for kw, word in ((dict(mode="gauss"), "mode"), (dict(mode=0), "mode"), (dict(shape="circle"), "shape"), (dict(shape=None), "shape"),
                     (dict(strength=0.0), "strength"), (dict(strength=0.0004), "strength"), (dict(strength=1.001), "strength"),
                     (dict(strength=float("nan")), "strength"), (dict(strength="1"), "strength"), (dict(margin=-0.1), "margin"),
                     (dict(margin=4.5), "margin"), (dict(score_threshold=float("nan")), "score_threshold"), (dict(fill=(0, 0, 256)), "fill"),
                     (dict(fill=(1, 2)), "fill")):
        with pytest.raises(ValueError, match=word):
            redact.apply([], None, None, **kw)
    assert redact.strength_per_mille(0.125) == 125 and redact.strength_per_mille(1) == 1000 and redact.strength_per_mille(0.001) == 1


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


def test_help_names_the_flags_and_their_defaults():
    from dan_amd import eval_cli
    names = ("redact_dir", "redact_mode", "redact_shape", "redact_strength", "redact_margin", "redact_threshold")
    for model in MODELS:
        text = eval_cli.build_parser(model).format_help()
        assert "--redact_mode {blur,mosaic,fill}" in text and "--redact_shape {rect,ellipse}" in text
        assert all("--" + n in text for n in names) and not any(n in eval_cli.REFERENCE_FLAGS for n in names), model
        args = eval_cli.build_parser(model).parse_args([])
        assert [getattr(args, n) for n in names] == [None, "blur", "rect", 0.125, 0.0, None]
        args = eval_cli.build_parser(model).parse_args(["--redact_dir", "d", "--redact_mode", "mosaic", "--redact_shape", "ellipse", "--redact_strength", "0.2",
                                                        "--redact_margin", "0.1", "--redact_threshold", "0.5"])
        assert [getattr(args, n) for n in names] == ["d", "mosaic", "ellipse", 0.2, 0.1, 0.5]


@pytest.mark.parametrize("flags,code", [(["--redact_mode", "gauss"], 2), (["--redact_mode"], 2), (["--redact_shape", "circle"], 2),
                                        (["--redact_strength", "x"], 2), (["--redact_strength", "0"], "strength"),
                                        (["--redact_strength", "1.5"], "strength"), (["--redact_strength", "nan"], "strength"),
                                        (["--redact_margin", "-1"], "margin"), (["--redact_margin", "5"], "margin"),
                                        (["--redact_threshold", "nan"], "score_threshold")])
def test_bad_values_of_the_flags_exit_before_the_device(flags, code, no_device, tmp_path, capsys):
    from dan_amd import eval_dan, eval_sfd
    for command in (eval_sfd, eval_dan):
        with pytest.raises(SystemExit) as e:
            command.main(["--redact_dir", str(tmp_path / "redacted"), "--data_dir", str(tmp_path), "--det_dir", str(tmp_path / "det")] + flags)
        if code == 2:
            assert e.value.code == 2 and flags[0] in capsys.readouterr().err.splitlines()[-1]      # the argument parser's own refusal
        else:
            assert code in str(e.value.code) and "--redact_strength / --redact_margin / --redact_threshold" in str(e.value.code)
    assert not (tmp_path / "redacted").exists() and not (tmp_path / "det").exists()
