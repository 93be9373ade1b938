"""The score label of the debug images without a GPU (include/danhip.h, "Box drawing"; csrc/draw_font.h): the library's glyph table against
the copy dan_amd/utility/draw_toolbox.py keeps as '.###.' strings; danhip_draw_format_score - the inline function the kernel runs - against
Python's own '%.1f%%' of the float32 product under the range rule (draw_toolbox.score_text), on named values, on exact ties, on scores for
which a float32 `v * 10` prints another digit, and on 100 000 random scores; draw_reference with scores traced by hand.  Equality only."""
import ctypes

import numpy as np
import pytest

F32 = np.float32


@pytest.fixture(scope="module")
def L():
    from dan_amd import _lib
    return _lib.lib()


def _c_text(L, score):
    out = ctypes.create_string_buffer(8)
    assert L.danhip_draw_format_score(ctypes.c_float(float(score)), out) == 0, L.danhip_last_error().decode()
    return out.value.decode()


def _python_text(score):
    """The issue's rule with nothing of the library in it: Python's '%.1f%%' of the float32 product; no label unless the score is finite and
    0 <= tenths <= 9999; -0.0 without its sign."""
    with np.errstate(over="ignore", invalid="ignore"):
        v = F32(score) * F32(100)
    if not np.isfinite(v):
        return ""
    s = "%.1f%%" % v
    tenths = int(s[:-1].replace(".", ""))
    if tenths < 0 or tenths > 9999:
        return ""
    return s[1:] if s.startswith("-") else s


def tie_scores():
    """float32 scores whose float32 product with 100 is an odd multiple of 0.25, so that v * 10 = 5 j + 2.5 is an exact tie: the quotient
    v / 100 and its float32 neighbours, kept where the product lands on v.  -> (scores, products)."""
    targets = (2 * np.arange(200, dtype=np.float64) + 1) / 4                       # 0.25 .. 99.75
    base = (targets / 100).astype(F32)
    cands = np.concatenate([base, np.nextafter(base, F32(0)), np.nextafter(base, F32(2))])
    v = cands * F32(100)
    keep = v.astype(np.float64) == np.tile(targets, 3)
    return cands[keep], v[keep]


def double_rounding_scores(want=20):
    """float32 scores in [0, 1], drawn with a fixed seed, for which float32(v * 10) rounded to the nearest integer is another number than
    the exact v * 10 rounded (the product is exact in float64): what a kernel that multiplies in float32 prints wrongly."""
    rng = np.random.RandomState(20)
    found = []
    for _ in range(16):
        s = rng.random_sample(1 << 20).astype(F32)
        s = s[s <= 1]
        v = s * F32(100)
        twice = np.rint((v * F32(10)).astype(np.float64))
        once = np.rint(v.astype(np.float64) * 10.0)
        found.append(s[twice != once])
        if sum(len(f) for f in found) >= want:
            break
    return np.concatenate(found)


def test_abi_version(L):
    assert L.danhip_version() >= 18


def test_glyph_table_equals_the_python_copy(L):
    from dan_amd.utility import draw_toolbox as D
    assert D.GLYPH_ORDER == "0123456789.%" and sorted(D.GLYPHS) == sorted(D.GLYPH_ORDER)
    assert (D.TEXT_H, D.BASELINE, D.ADVANCE) == (7, 2, 6)
    for index, ch in enumerate(D.GLYPH_ORDER):
        rows = (ctypes.c_uint8 * 7)()
        assert L.danhip_draw_glyph(index, rows) == 0
        strings = D.GLYPHS[ch]
        assert len(strings) == 7 and all(len(r) == 5 and set(r) <= set(".#") for r in strings), ch
        want = [int(r.replace("#", "1").replace(".", "0"), 2) for r in strings]            # the left column is bit 4
        assert list(rows) == want, ch
        assert any(rows), ch                                                               # something is drawn
        assert all(r < 32 for r in rows), ch                                               # nothing outside 5 columns
    rows = (ctypes.c_uint8 * 7)()
    assert L.danhip_draw_glyph(12, rows) != 0 and L.danhip_draw_glyph(-1, rows) != 0
    assert len(set(D.GLYPHS.values())) == 12                                               # no two characters look alike


NAMED = [(0.0, "0.0%"), (1.0, "100.0%"), (0.2, "20.0%"), (0.99951, "100.0%"), (0.9995, "99.9%"), (1e-4, "0.0%"),
         (float(np.nextafter(F32(1), F32(0))), "100.0%"), (float("nan"), ""), (float("inf"), ""), (float("-inf"), ""), (-0.0, "0.0%"),
         (-0.1, ""), (10.0, ""), (9.9994, "999.9%"), (0.5, "50.0%"), (0.125, "12.5%"), (3.0e38, "")]


@pytest.mark.parametrize("score,text", NAMED, ids=[repr(s) for s, _ in NAMED])
def test_named_scores(L, score, text):
    from dan_amd.utility import draw_toolbox as D
    assert _python_text(score) == text                   # the expectation written here is what Python prints
    assert D.score_text(score) == text
    assert _c_text(L, score) == text


def test_exact_ties_round_to_even(L):
    scores, v = tie_scores()
    assert len(scores) >= 50
    tenths = v.astype(np.float64) * 10
    assert np.array_equal(tenths - np.floor(tenths), np.full(len(v), 0.5))          # ties, all of them
    half_up = np.floor(tenths + 0.5)
    differ = 0
    for s, up in zip(scores, half_up):
        want = _python_text(s)
        assert _c_text(L, s) == want, (s, want)
        differ += want != "%d.%d%%" % (up // 10, up % 10)
    assert differ >= 20, "ties onto an even tenth are among them: half-up would print another digit there"


def test_scores_a_float32_product_prints_wrongly(L):
    scores = double_rounding_scores()
    assert len(scores) >= 20
    for s in scores:
        want = _python_text(s)
        wrong = np.rint(np.float64((s * F32(100)) * F32(10)))
        assert want != "%d.%d%%" % (wrong // 10, wrong % 10)                        # the search found what it was after
        assert _c_text(L, s) == want, (s, want)


def test_100000_random_scores(L):
    from dan_amd.utility import draw_toolbox as D
    scores = np.random.RandomState(3).random_sample(100000).astype(F32)
    out = ctypes.create_string_buffer(8)
    lengths = set()
    for s in scores:
        L.danhip_draw_format_score(ctypes.c_float(float(s)), out)
        got = out.value.decode()
        assert got == "%.1f%%" % (s * F32(100)), s
        lengths.add(len(got))
    assert lengths == {4, 5, 6}
    for s in scores[:2000]:
        assert D.score_text(s) == _python_text(s)


def test_draw_reference_label_traced_by_hand():
    """One 24 x 48 image, box (10, 15) - (40, 20), t = 2, score 0.5 -> '50.0%', 5 characters, text_w = 29.
    tab: x 9 .. 39, y 15 - 7 - 2 - 2 = 4 .. 15.  text: bottom row y = 15 - 7 + 2 = 10, top row y = 4; '5' in columns 10 .. 14, its rows
    '#####', '#....', ...; column 15 is the gap; '.' (character 2) in columns 22 .. 26 with '.##..' on the two bottom rows."""
    from dan_amd.utility import draw_toolbox as D
    image = np.full((24, 48, 3), 7, np.uint8)
    out = D.draw_reference(image, [1], np.array([[10.0, 15.0, 40.0, 20.0]], np.float32), thickness=2, scores=[0.5])
    colour, white, kept = (203, 71, 119), (255, 255, 255), (7, 7, 7)
    at = lambda x, y: tuple(int(c) for c in out[y, x])
    assert at(9, 4) == colour and at(39, 4) == colour and at(9, 15) == colour and at(39, 15) == colour       # the tab's corners
    assert at(8, 4) == kept and at(40, 4) == kept and at(9, 3) == kept and at(39, 3) == kept                 # and just outside them
    assert at(10, 4) == white and at(14, 4) == white and at(10, 5) == white                                  # the 5: its top bar, its stem
    assert at(11, 5) == colour and at(15, 4) == colour and at(20, 12) == colour                              # inside the tab, outside every glyph
    assert at(23, 10) == white and at(24, 9) == white and at(22, 10) == colour and at(23, 8) == colour       # the point
    assert at(38, 10) == white and at(39, 10) == colour                                                      # the last column of '%', then the tab's edge
    assert at(9, 21) == colour and at(41, 14) == colour and at(12, 18) == kept                               # the rectangle itself
    plain = D.draw_reference(image, [1], np.array([[10.0, 15.0, 40.0, 20.0]], np.float32), thickness=2)
    assert np.array_equal(out[16:], plain[16:]) and not np.array_equal(out[:16], plain[:16])                 # the label lies above y1
    assert int((out == 255).all(axis=2).sum()) == sum(r.count("#") for ch in "50.0%" for r in D.GLYPHS[ch])
    # no label: the rectangle alone
    for s in (float("nan"), 10.0, -0.1):
        assert np.array_equal(D.draw_reference(image, [1], np.array([[10.0, 15.0, 40.0, 20.0]], np.float32), 2, scores=[s]), plain)
    assert np.array_equal(D.draw_reference(image, [0], np.array([[10.0, 15.0, 40.0, 20.0]], np.float32), 2, scores=[0.5]), image)
