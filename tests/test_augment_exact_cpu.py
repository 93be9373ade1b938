"""Pins tests/augment_exact.py itself (no GPU, the oracle alone): the preconditions of the cases of tests/test_augment_exact_gpu.py, so that
none of them can be satisfied trivially - every palette chain reaches the branches it is named for, every looping size loops, and every
contrast mean is one float32 whatever the summation order."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import augment_exact as AE  # noqa: E402
from oracle import preprocess as O  # noqa: E402

F = np.float32


def test_palette_holds_every_kind_more_than_once():
    p = AE.palette().reshape(-1, 3).astype(int)
    r, g, b = p[:, 0], p[:, 1], p[:, 2]
    M, m = p.max(1), p.min(1)
    kinds = {"black": M == 0, "white": m == 255, "gray": (M == m) & (M > 0) & (M < 255), "hue exactly 0": (r > g) & (g == b),
             "r == g > b": (r == g) & (g > b), "r == b > g": (r == b) & (b > g), "g == b > r": (g == b) & (b > r),
             "r == g < b": (r == g) & (g < b), "r == b < g": (r == b) & (b < g),
             "one level apart": (M - m == 1), "value 1": (p == 1).any(1), "value 254": (p == 254).any(1), "value 255": (p == 255).any(1)}
    for c in ((255, 0, 0), (0, 255, 0), (0, 0, 255), (255, 255, 0), (0, 255, 255), (255, 0, 255)):
        kinds["pure %s" % (c,)] = (p == np.asarray(c)).all(1) | (p == np.asarray(c) * 200 // 255).all(1)
    for name, mask in kinds.items():
        assert mask.sum() > 1, name
    assert AE.palette().shape == (AE.PALETTE_H, AE.PALETTE_W, 3) and AE.PALETTE_WINDOW == (0, 0) + AE.PALETTE_OUT      # identity geometry


@pytest.mark.parametrize("name", sorted(AE.PALETTE_CHAINS))
def test_palette_chain_reaches_the_branches_it_is_named_for(name):
    ops, want = AE.PALETTE_CHAINS[name]
    counts = AE.census(AE.to01(AE.palette()), ops)
    for branch in want:
        assert counts[branch] > 0, (name, branch, counts)
    assert name in AE.PALETTE_ORDER and len(AE.PALETTE_ORDER) == len(AE.PALETTE_CHAINS)


def test_palette_chains_cover_every_branch_and_the_ends_of_every_range():
    reached = set(b for _, want in AE.PALETTE_CHAINS.values() for b in want)
    assert reached == set(AE.census(AE.to01(AE.palette()), []))
    alone = {(ops[0][0], round(float(ops[0][1]), 6)) for ops, _ in AE.PALETTE_CHAINS.values() if len(ops) == 1}
    for op, vals in (("brightness", (-AE.B32, 0.0, AE.B32)), ("saturation", (0.5, 1.5, 1.0, 0.0)), ("hue", (-0.2, 0.0, 0.2)), ("contrast", (0.5, 1.5, 1.0))):
        for v in vals:
            assert (op, round(v, 6)) in alone, (op, v)
    orders = {tuple(n for n, _ in ops) for ops, _ in AE.PALETTE_CHAINS.values() if len(ops) == 4}
    assert orders == set(O.ORDERINGS.values())
    # the batch of all chains starts and ends with an item that owns no workgroup of the mean reduction, and has such items in between
    first, last = AE.PALETTE_CHAINS[AE.PALETTE_ORDER[0]][0], AE.PALETTE_CHAINS[AE.PALETTE_ORDER[-1]][0]
    assert not AE.has_contrast(first) and not AE.has_contrast(last)


def test_census_walks_the_oracle_chain():
    """The op-by-op walk of census / before_contrast is distort_color: same image at the end, same contrast mean."""
    img = AE.to01(AE.palette())
    for name, (ops, _) in AE.PALETTE_CHAINS.items():
        x = img
        for op, val in ops:
            x = AE._apply_one(x, op, val)
        dist, mean = O.distort_color(img, ops)
        assert np.array_equal(np.clip(x, F(0), F(1)), dist), name
        pre, at = AE.before_contrast(AE.palette(), ops)
        assert (at >= 0) == AE.has_contrast(ops) and (at < 0 or np.array_equal(pre.reshape(-1, 3).mean(0, dtype=np.float64).astype(F), mean)), name


def test_hue_wrap_case_lands_on_sector_six():
    """-1e-9 is below half an ulp of 1: hue 0 becomes exactly 1.0, h * 6 exactly 6 - the sector the kernel clamps to 5."""
    d = F(AE.PALETTE_CHAINS["hue_wraps_to_one"][0][0][1])
    h = F(0) + d
    h = F(h - np.floor(h))
    assert d < 0 and h == F(1) and int(F(h * F(6))) == 6


def test_oracle_covers_the_three_flip_modes():
    img = AE.random_image(*AE.GEOMETRY_IMAGE)
    win = AE.GEOMETRY_WINDOWS["leaves_left"]
    a, b, c = (AE.oracle(img, [], win, f, (9, 33)) for f in (0, 1, 2))
    assert np.array_equal(b, a[:, ::-1]) and not np.array_equal(c, b) and not np.array_equal(c, a)      # resize, then mirror != mirror, then resize
    assert np.array_equal(AE.oracle(img, [], win, True, (9, 33)), b) and np.array_equal(AE.oracle(img, [], win, False, (9, 33)), a)
    same = AE.oracle(img, [], win, 2, (6, 8))                                    # window size = output size: lx = ly = 0, the two orders agree
    assert np.array_equal(same, AE.oracle(img, [], win, 1, (6, 8)))


def test_geometry_cases_are_what_their_names_say():
    _, H, W = AE.GEOMETRY_IMAGE
    for name, (y, x, h, w) in AE.GEOMETRY_WINDOWS.items():
        out = [y < 0, y + h > H, x < 0, x + w > W]                                # top, bottom, left, right
        if name.startswith("leaves_") and name != "leaves_all":
            assert out == [name == "leaves_" + s for s in ("top", "bottom", "left", "right")], name
        elif name == "leaves_all":
            assert all(out)
        elif name.startswith("outside"):
            assert y >= H or x >= W or y + h <= 0 or x + w <= 0, name
        else:
            assert not any(out), name
    assert AE.GEOMETRY_WINDOWS["one_row"][2] == 1 and AE.GEOMETRY_WINDOWS["one_column"][3] == 1 and AE.GEOMETRY_WINDOWS["one_pixel"][2:] == (1, 1)
    assert AE.GEOMETRY_WINDOWS["inside_7x5"][2:] == (7, 5) and (33, 31) in AE.GEOMETRY_OUT_SHAPES                  # 33 / 7, 31 / 5: not dyadic
    assert AE.contrast_mean_is_pinned(AE.random_image(*AE.GEOMETRY_IMAGE), AE.GEOMETRY_CHAIN) and AE.GEOMETRY_CHAIN[0][0] == "contrast"
    rem = {(h % AE.TILE_H, w % AE.TILE_W) for h, w in AE.GEOMETRY_OUT_SHAPES}
    assert {(0, 0), (1, 1), (AE.TILE_H - 1, AE.TILE_W - 1), (0, 1), (1, 1)} <= rem                 # each axis: exact, one over, one under
    assert any(h > AE.TILE_H and w > AE.TILE_W for h, w in AE.GEOMETRY_OUT_SHAPES) and (1, 1) in AE.GEOMETRY_OUT_SHAPES
    names = [n for n, _, _, _ in AE.geometry_items((0, 1, 2))]
    assert len(names) == len(set(names)) == len(AE.GEOMETRY_WINDOWS) * 3 * 2


def test_looping_sizes_loop():
    (_, h, w), _, _, out = AE.LOOPING["output_second_trip"]
    assert (h, w) == (61, 47) and AE.AUGMENT_PER_TRIP == 1048576 and out[0] * out[1] == 1056768 > AE.AUGMENT_PER_TRIP
    (_, h, w), ops, _, _ = AE.LOOPING["mean_second_trip"]
    assert ops[0][0] == "contrast" and AE.MEAN_PER_TRIP == 262144 and h * w == 266240 > AE.MEAN_PER_TRIP
    (_, h, w), ops, _, _ = AE.LOOPING["batch_mean_above_cap"]
    assert ops[0][0] == "contrast" and h * w > AE.AUG_MEAN_MAX_BLOCKS * AE.AUG_MEAN_PIX_PER_BLOCK
    assert AE.mean_blocks(h, w, ops) == AE.AUG_MEAN_MAX_BLOCKS < -(-h * w // AE.AUG_MEAN_PIX_PER_BLOCK) and h * w > AE.BATCH_MEAN_PER_TRIP
    images, items = AE.looping_batch()
    owns = [AE.mean_blocks(im.shape[0], im.shape[1], ops) for im, (ops, _, _) in zip(images, items)]
    assert owns[0] == 0 and owns[1] == AE.AUG_MEAN_MAX_BLOCKS and owns[2] == 0 and owns[3] > 0 and len(owns) == 4
    assert {f for _, _, f in items} == {0, 1, 2}


def _contrast_cases():
    cases = [("looping " + n, AE.noisy_image(*src), ops) for n, (src, ops, _, _) in AE.LOOPING.items()]
    cases += [("looping batch item %d" % k, im, ops) for k, (im, (ops, _, _)) in enumerate(zip(*AE.looping_batch()))]
    cases += [(n, AE.noisy_image(*src), ops) for n, (src, ops, _, _) in list(AE.CONTRAST_LATER.items()) + list(AE.CONTRAST_FIRST.items())]
    cases += [("palette " + n, AE.palette(), ops) for n, (ops, _) in AE.PALETTE_CHAINS.items()]
    cases += [("isolation item %d" % k, im, ops) for k, (im, (ops, _, _)) in enumerate(zip(AE.isolation_images(), AE.ISOLATION[1]))]
    return [c for c in cases if AE.has_contrast(c[2])]


def test_contrast_means_do_not_depend_on_the_summation_order():
    later = first = 0
    for name, img, ops in _contrast_cases():
        pre, at = AE.before_contrast(img, ops)
        if at == 0:                                                              # the exact-sum argument
            x = pre.astype(np.float64) * 2.0 ** 31
            assert np.array_equal(pre, AE.to01(img)) and np.all(x == np.floor(x)) and x.max() <= 2.0 ** 31, name
            assert img.shape[0] * img.shape[1] <= 2 ** 22, name
            assert AE.contrast_first_is_exact(img), name
            first += 1
        else:
            for k in range(3):
                assert AE.mean_is_order_independent(pre[..., k]), (name, "channel %d: pick another seed" % k)
            later += 1
        assert AE.contrast_mean_is_pinned(img, ops), name
    assert all(ops[0][0] == "contrast" for _, ops, _, _ in AE.CONTRAST_FIRST.values())
    assert all(AE.has_contrast(ops) and ops[0][0] != "contrast" for _, ops, _, _ in AE.CONTRAST_LATER.values())
    assert later >= len(AE.CONTRAST_LATER) + 3 and first >= len(AE.CONTRAST_FIRST) + 3


def test_order_independence_condition_rejects_a_sum_on_a_rounding_boundary():
    """The condition is a real one: a channel whose mean sits on the midpoint of two float32 values fails it."""
    lo = F(0.5)
    hi = np.nextafter(lo, F(1))
    assert not AE.mean_is_order_independent(np.asarray([lo, hi], F))            # mean = the midpoint: a tie
    assert AE.mean_is_order_independent(np.asarray([lo, lo, hi, hi, hi], F))


def test_existing_suites_contrast_items_are_pinned():
    """The items of tests/test_preprocess_batch_gpu.py that are compared bit for bit between the batched and the per-image entry point."""
    import test_preprocess_batch_gpu as TB
    n = 0
    for name, img, ops in TB.pinned_contrast_items():
        assert AE.has_contrast(ops) and AE.contrast_mean_is_pinned(img, ops), name
        n += 1
    assert n >= 12
