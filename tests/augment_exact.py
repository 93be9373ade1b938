"""Helper of tests/test_augment_exact_cpu.py, tests/test_augment_exact_gpu.py, the two preprocessing suites and the fp16 child
(tests/fp16/cases.py); not collected by pytest.

The training input pass (dan_amd/csrc/augment_exact.hip) against the oracle chain (oracle/preprocess.py) by EQUALITY.  The file is built with
-ffp-contract=off, and apart from the contrast mean every value it produces is one IEEE float32 operation after another (+ - * /, fmodf,
floorf, truncf, float <-> int conversions, one round-to-nearest-even convert to the 16-bit type) in the order the oracle restates in numpy
float32: there is no summation order, no fused multiply-add and no approximate instruction to differ by, so the device result must EQUAL the
oracle's float32 result rounded to the storage type (assert_exact), in the bf16 build and in the fp16 build.
The contrast mean is the one cross-workgroup quantity: a float64 sum, divided by the pixel count in float64, rounded to float32.  It is
exact in two situations, and test_augment_exact_cpu.py asserts for every contrast case here which one holds:
  * contrast FIRST: every term is u8 * float32(1/255), a multiple of 2^-31 that is at most 1, and there are at most 2^22 of them, so every
    partial sum in any order is an exact float64 (contrast_first_is_exact);
  * contrast LATER: the float32 mean does not depend on the order when (S +- N 2^-52 A) / N round to one float32, S = math.fsum of the
    channel, A = fsum of the absolute values (mean_is_order_independent) - a condition on the INPUT, met by the choice of images and seeds.

Measured on an MI355X before any criterion was tightened - the cases of tests/test_preprocess_gpu.py and tests/test_preprocess_batch_gpu.py as
they stood, share of the values that differ from the oracle after the 16-bit rounding (bf16 build), and the largest difference:
  preprocess_for_train, seeds 0 .. 7 (76 800 or 307 200 values each, drawn chains with a contrast op)      0 of 8 cases differ: share 0, largest 0
  colour chain, each op alone / the 4-op chain / no op (8 cases of 18 432 values)                          share 0, largest 0
  window leaving the image, flip off and on (2 x 19 200 values)                                            share 0, largest 0
  batches single_ops and all_four, 5 items each, outputs 80 x 80 and 64 x 96 (20 slices)                   share 0, largest 0
  flip of the window before the resize (3 items), the changed item of the isolation test                   share 0, largest 0
  the drawn S3FD batch against the oracle (3 images)                                                       share 0, largest 0
and every batch slice above, contrast items and the 18 drawn pipeline images included, was torch.equal to the per-image result.  The "ulp of
float op order" that the earlier criterion (fewer than 2e-3 of the values, none by more than 1.01) allowed for does not exist, so both suites
now use assert_exact, and no case keeps a bound against the oracle.  One comparison keeps the earlier bound: batch slice against per-image
result for the DRAWN chains of the pipelines (tests/test_preprocess_batch_gpu.py, pinned=False), whose two float64 sums run in different
orders over inputs that no CPU test has shown to be order-independent; measured equal as well.
"""
import functools
import math

import numpy as np
import torch

from oracle import preprocess as O

F = np.float32

# ---------------------------------------------------------------------------------------------------------------- launch constants
# Each mirrors the line of dan_amd/csrc/augment_exact.hip it names; the loop-trip conditions of LOOPING are computed from them.
THREADS = 256                     # `dim3(256)` of every launch in the file
AUGMENT_MAX_BLOCKS = 4096         # danhip_augment_preprocess: `if (blocks > 4096) blocks = 4096;` before augment_kernel
MEAN_MAX_BLOCKS = 1024            # danhip_augment_preprocess: `if (blocks > 1024) blocks = 1024;` before aug_mean_kernel
TILE_W, TILE_H = 32, 8            # `enum { AUG_TILE_W = 32, AUG_TILE_H = 8, ...` (augment_batch_kernel: one thread per output pixel)
AUG_MEAN_PIX_PER_BLOCK = 2048     # `... AUG_MEAN_PIX_PER_BLOCK = 2048, ...` (danhip_augment_item_init: workgroups of an item's mean)
AUG_MEAN_MAX_BLOCKS = 512         # `... AUG_MEAN_MAX_BLOCKS = 512, ...`
AUGMENT_PER_TRIP = AUGMENT_MAX_BLOCKS * THREADS          # 1 048 576 output pixels per trip of augment_kernel
MEAN_PER_TRIP = MEAN_MAX_BLOCKS * THREADS                # 262 144 source pixels per trip of aug_mean_kernel
BATCH_MEAN_PER_TRIP = AUG_MEAN_MAX_BLOCKS * THREADS      # 131 072 source pixels per trip of aug_mean_batch_kernel at the cap
FLIP_NONE, FLIP_RESIZED, FLIP_WINDOW = 0, 1, 2           # danhip_augment_item.flip


def mean_blocks(h, w, ops):
    """danhip_augment_item_init: workgroups of one item in aug_mean_batch_kernel (0 without a contrast op)."""
    if not has_contrast(ops):
        return 0
    return min(-(-h * w // AUG_MEAN_PIX_PER_BLOCK), AUG_MEAN_MAX_BLOCKS)


def has_contrast(ops):
    return any(n == "contrast" for n, _ in ops)


# ---------------------------------------------------------------------------------------------------------------- the oracle chain
def to01(img_u8):
    return (img_u8.astype(F) * F(1.0 / 255)).astype(F)                              # convert_image_dtype(uint8 -> float32)


def oracle(img_u8, ops, win, flip, out_shape):
    """uint8 [H,W,3] -> float32 [out_h,out_w,3] (BGR, mean-subtracted) before the 16-bit rounding.  flip: 0 / False none, 1 / True the
    RESIZED image is mirrored, 2 the WINDOW is mirrored before the resize."""
    flip = int(flip)
    dist, _ = O.distort_color(to01(img_u8), ops)
    patch = O.crop_with_mean_fill(dist, win)
    if flip == FLIP_WINDOW:
        patch = np.ascontiguousarray(patch[:, ::-1])
    return O.finish(O.resize_bilinear_legacy(patch, out_shape[0], out_shape[1]), flip == FLIP_RESIZED)


def exact_share(got, ref32):
    """(share of differing values, largest difference) of got[..., :3] against ref32 rounded to got's 16-bit type."""
    g = got.float().cpu().numpy()[..., :3]
    ref16 = torch.from_numpy(np.array(ref32, np.float32)).to(got.dtype).float().numpy()
    d = np.abs(g - ref16)
    return float((d > 0).mean()), float(d.max())


def assert_exact(got, ref32, what):
    """got: [..., 8] device result (16-bit); ref32: float32 [..., 3] reference before the 16-bit rounding.  Channels 3..7 are zero and the
    first three EQUAL the reference rounded to got.dtype."""
    assert got.dtype in (torch.bfloat16, torch.float16) and got.shape[-1] == 8 and tuple(got.shape[:-1]) == tuple(ref32.shape[:-1]), \
        (what, got.dtype, tuple(got.shape), ref32.shape)
    g = got.cpu()
    assert torch.all(g[..., 3:] == 0), (what, "padding channels are not zero")
    ref16 = torch.from_numpy(np.array(ref32, np.float32)).to(got.dtype)
    bad = g[..., :3] != ref16
    n = int(bad.sum())
    if n:
        where = bad.nonzero()[:6]
        lines = ["%s: got %r, reference %r" % (tuple(int(i) for i in w), float(g[..., :3][tuple(w)]), float(ref16[tuple(w)])) for w in where]
        print("%s: %d of %d values differ\n  %s" % (what, n, bad.numel(), "\n  ".join(lines)))
    assert n == 0, "%s: %d of %d values differ from the oracle (first at %s)" % (what, n, bad.numel(), bad.nonzero()[0].tolist())


# ---------------------------------------------------------------------------------------------------------------- inputs
def noisy_image(seed, h, w):
    """The blocky + noise image of the two preprocessing suites: smooth and sharp parts."""
    rng = np.random.RandomState(seed)
    base = rng.randint(0, 256, (h // 8 + 1, w // 8 + 1, 3)).astype(np.float32)
    img = np.kron(base, np.ones((8, 8, 1), np.float32))[:h, :w] + rng.randn(h, w, 3) * 12
    return np.clip(img, 0, 255).astype(np.uint8)


def random_image(seed, h, w):
    return np.random.RandomState(seed).randint(0, 256, (h, w, 3)).astype(np.uint8)


_GRAYS = [1, 2, 37, 64, 127, 128, 200, 254]
_PRIMARIES = [(1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 0), (0, 1, 1), (1, 0, 1)]
# hue exactly 0 with saturation > 0: r the maximum, g == b.  The last rows are the pixels at which adjust_hue(HUE_ONE_DELTA) puts a
# float32 right at a uint8 truncation boundary: hue 0 and hue 1 (the same colour) give different levels there, see hue_one_differs
_HUE_ZERO = [(255, 0, 0), (200, 50, 50), (255, 254, 254), (2, 1, 1), (128, 64, 64), (1, 0, 0), (255, 1, 1), (254, 127, 127), (90, 17, 17)]
HUE_ONE_PIXELS = [(50, 5, 5), (100, 10, 10), (150, 15, 15), (200, 20, 20), (232, 115, 115), (250, 25, 25)]      # found by a search over (r, g == b) x delta
HUE_ONE_DELTA = 0.0665
_SPECIAL = (
    [(0, 0, 0)] * 3 + [(255, 255, 255)] * 3 + [(v, v, v) for v in _GRAYS]
    + [tuple(255 * c for c in p) for p in _PRIMARIES] + [tuple(200 * c for c in p) for p in _PRIMARIES] + [tuple(3 * c for c in p) for p in _PRIMARIES]
    + [(200, 200, 50), (255, 255, 254), (2, 2, 1), (128, 128, 0)]                 # r == g > b
    + [(200, 50, 200), (255, 254, 255), (2, 1, 2), (128, 0, 128)]                 # r == b > g
    + [(50, 200, 200), (254, 255, 255), (1, 2, 2), (0, 128, 128)]                 # g == b > r
    + [(50, 50, 200), (0, 0, 1), (254, 254, 255), (50, 200, 50), (0, 1, 0), (254, 255, 254)]      # ties of the minimum (g == b < r: _HUE_ZERO)
    + _HUE_ZERO
    + [(100, 100, 101), (100, 101, 100), (101, 100, 100), (100, 101, 101), (101, 100, 101), (101, 101, 100), (254, 255, 255), (1, 0, 0)]
    + [(1, 254, 255), (255, 254, 1), (254, 255, 1), (1, 1, 254), (255, 1, 254), (254, 1, 1), (1, 255, 1), (255, 255, 1)]
    + [(50, 0, 0), (0, 40, 3), (3, 0, 60), (60, 2, 1), (20, 30, 10), (33, 31, 32)]  # dark: a negative brightness leaves M > 0 > m, or M <= 0 < c
)
PALETTE_H, PALETTE_W = 16, 16


@functools.lru_cache(maxsize=None)
def _palette():
    px = list(_SPECIAL) + [tuple(p) for p in HUE_ONE_PIXELS]
    assert len(px) <= PALETTE_H * PALETTE_W
    px = px + [tuple(p) for p in np.random.RandomState(7).randint(0, 256, (PALETTE_H * PALETTE_W - len(px), 3))]
    order = np.random.RandomState(8).permutation(len(px))                         # (no kind sits in one wave or one tile row only)
    a = np.asarray(px, np.uint8)[order].reshape(PALETTE_H, PALETTE_W, 3)
    a.setflags(write=False)
    return a


def palette():
    return _palette()


B32 = 32.0 / 255.0
# name -> (chain, the branches the case is there for: test_augment_exact_cpu.py asserts that census() counts each of them > 0)
PALETTE_CHAINS = {
    "identity": ([], []),
    "brightness_lo": ([("brightness", -B32)], ["clip_lo"]),
    "brightness_0": ([("brightness", 0.0)], []),
    "brightness_hi": ([("brightness", B32)], ["clip_hi"]),
    "saturation_0.5": ([("saturation", 0.5)], ["c_eq_0", "M_eq_0", "sat_at_0"]),
    "saturation_1.5": ([("saturation", 1.5)], ["c_eq_0", "M_eq_0", "sat_at_0", "sat_at_1"]),
    "saturation_1": ([("saturation", 1.0)], ["c_eq_0", "M_eq_0", "sat_at_0", "sat_at_1", "hue_0"]),
    "saturation_0": ([("saturation", 0.0)], ["c_eq_0", "M_eq_0", "sat_at_0"]),
    "hue_lo": ([("hue", -0.2)], ["c_eq_0", "M_eq_0", "hue_0"]),
    "hue_0": ([("hue", 0.0)], ["c_eq_0", "M_eq_0", "hue_0", "wrapped_0"]),
    "hue_hi": ([("hue", 0.2)], ["c_eq_0", "M_eq_0", "hue_0"]),
    "hue_wraps_to_one": ([("hue", -1e-9)], ["hue_0", "wrapped_1"]),                # 0 + d - floor(0 + d) rounds to exactly 1.0: sector 6 -> 5
    "hue_plus_half": ([("hue", 0.5)], ["wrapped_0"]),                            # cyan (hue exactly 0.5) arrives at 1.0 - floor(1.0) = 0
    "hue_minus_half": ([("hue", -0.5)], ["wrapped_0"]),                          # ... and at 0.5 - 0.5 = 0
    "hue_zero_or_one": ([("hue", HUE_ONE_DELTA)], ["hue_0", "hue_one_differs"]),
    "contrast_0.5": ([("contrast", 0.5)], []),
    "contrast_1": ([("contrast", 1.0)], []),
    "contrast_1.5": ([("contrast", 1.5)], ["clip_lo", "clip_hi"]),
    # the four orderings of oracle.preprocess.ORDERINGS at the ends of the drawn ranges; in 0 and 1 the brightness precedes an HSV op
    "order0_lo": ([("brightness", -B32), ("saturation", 1.5), ("hue", 0.2), ("contrast", 1.5)],
                  ["M_le_0_after_brightness", "s_gt_1_after_brightness", "sat_at_1", "clip_lo", "clip_hi"]),
    "order0_hi": ([("brightness", B32), ("saturation", 0.5), ("hue", -0.2), ("contrast", 0.5)], ["c_eq_0"]),
    "order1_lo": ([("saturation", 1.5), ("brightness", -B32), ("contrast", 1.5), ("hue", -0.2)],
                  ["M_le_0_after_brightness", "s_gt_1_after_brightness", "sat_at_1", "clip_lo", "clip_hi"]),
    "order1_hi": ([("saturation", 0.5), ("brightness", B32), ("contrast", 0.5), ("hue", 0.2)], ["c_eq_0"]),
    "order2_lo": ([("contrast", 1.5), ("hue", 0.2), ("brightness", -B32), ("saturation", 1.5)],
                  ["M_le_0_after_brightness", "s_gt_1_after_brightness", "sat_at_1", "clip_lo", "clip_hi"]),
    "order2_hi": ([("contrast", 1.5), ("hue", -0.2), ("brightness", B32), ("saturation", 0.5)], ["s_gt_1_after_brightness", "clip_hi"]),
    "order3_lo": ([("hue", -0.2), ("saturation", 1.5), ("contrast", 1.5), ("brightness", -B32)], ["sat_at_1", "clip_lo", "clip_hi"]),
    "order3_hi": ([("hue", 0.2), ("saturation", 0.5), ("contrast", 1.5), ("brightness", B32)], ["clip_lo", "clip_hi"]),
    "order3_end": ([("hue", 0.2), ("saturation", 0.0), ("contrast", 0.5), ("brightness", 0.0)], ["sat_at_0"]),      # (a batch ends op-free below)
}
PALETTE_ORDER = ["identity"] + [n for n in PALETTE_CHAINS if n not in ("identity", "brightness_0")] + ["brightness_0"]    # contrast-free at both ends
PALETTE_WINDOW = (0, 0, PALETTE_H, PALETTE_W)                                     # identity geometry: lx = ly = 0, no blend
PALETTE_OUT = (PALETTE_H, PALETTE_W)


def census(img01, ops):
    """The oracle chain of distort_color, op by op, counting the pixels that take each special branch of the kernel's rgb2hsv / hsv2rgb /
    apply_ops / final clip.  -> dict of counts."""
    n = dict.fromkeys(["c_eq_0", "M_eq_0", "M_le_0_after_brightness", "s_gt_1_after_brightness", "sat_at_0", "sat_at_1", "hue_0", "wrapped_0",
                       "wrapped_1", "hue_one_differs", "clip_lo", "clip_hi"], 0)
    img, after_brightness = img01, False
    for name, val in ops:
        if name in ("saturation", "hue"):
            h, s, v = O.rgb_to_hsv(img[..., 0], img[..., 1], img[..., 2])
            M = np.maximum(np.maximum(img[..., 0], img[..., 1]), img[..., 2])
            c = M - np.minimum(np.minimum(img[..., 0], img[..., 1]), img[..., 2])
            n["c_eq_0"] += int((c == 0).sum())
            n["M_eq_0"] += int((M == 0).sum())
            n["hue_0"] += int(((h == 0) & (c > 0) & (s > 0)).sum())
            if after_brightness:
                n["M_le_0_after_brightness"] += int(((M <= 0) & (c > 0)).sum())
                n["s_gt_1_after_brightness"] += int((s > 1).sum())
            if name == "saturation":
                sf = (s * F(val)).astype(F)
                n["sat_at_0"] += int((sf <= 0).sum())
                n["sat_at_1"] += int((sf >= 1).sum())
            else:
                hw = (h + F(val)).astype(F)
                hw = (hw - np.floor(hw)).astype(F)
                live = (c > 0) & (s * v != 0)
                n["wrapped_1"] += int(((hw == 1) & ((hw * F(6)).astype(F).astype(np.int32) == 6) & live).sum())
                n["wrapped_0"] += int(((hw == 0) & live).sum())
                # hue 0 taken as hue 1 (`h < 0` written `h <= 0` in rgb2hsv): the same colour, but 1 + d - floor(1 + d) is another float32
                zero = (h == 0) & live
                h1 = (np.where(zero, F(1), h) + F(val)).astype(F)
                h1 = (h1 - np.floor(h1)).astype(F)
                a, b = np.stack(O.hsv_to_rgb(hw, s, v), -1), np.stack(O.hsv_to_rgb(h1, s, v), -1)
                if len(ops) == 1:
                    lv = lambda x: np.clip(np.clip(x, F(0), F(1)) * F(255.5), F(0), F(255)).astype(np.uint8)
                    n["hue_one_differs"] += int((lv(a) != lv(b)).any(-1).sum())
        if name == "brightness":
            after_brightness = True
        img = _apply_one(img, name, val)
    n["clip_lo"] = int((img < 0).sum())
    n["clip_hi"] = int((img > 1).sum())
    return n


def _apply_one(img, name, val):
    """One op of oracle.preprocess.distort_color WITHOUT its final clip."""
    if name == "brightness":
        return (img + F(val)).astype(F)
    if name == "saturation":
        return O.adjust_saturation(img, val)
    if name == "hue":
        return O.adjust_hue(img, val)
    return O.adjust_contrast(img, val, img.reshape(-1, 3).mean(0, dtype=np.float64).astype(F))


def before_contrast(img_u8, ops):
    """-> (float32 image the contrast op of the chain takes its mean of, index of the contrast op); (None, -1) without one."""
    img = to01(img_u8)
    for i, (name, val) in enumerate(ops):
        if name == "contrast":
            return img, i
        img = _apply_one(img, name, val)
    return None, -1


def contrast_first_is_exact(img_u8):
    """The exact-sum argument of a chain that starts with the contrast op: every term is u8 * float32(1/255), hence 0 or a multiple of
    2^-31 that is at most 1, and N <= 2^22, so every partial sum in any order is an integer below 2^53 times 2^-31: an exact float64."""
    x = to01(img_u8).astype(np.float64) * 2.0 ** 31
    return bool(np.all(x == np.floor(x)) and x.max() <= 2.0 ** 31 and x.shape[0] * x.shape[1] <= 2 ** 22)


def mean_is_order_independent(channel):
    """channel: float32 values one mean is taken of.  Any order of float64 additions of N terms is within (N - 1) 2^-53 A of the exact sum S
    (A = sum of absolute values); twice that covers the division's own rounding.  True when (S - e) / N, S / N and (S + e) / N, with
    e = N 2^-52 A, round to the same float32: then every summation order gives that float32."""
    x = [float(t) for t in np.asarray(channel, np.float64).reshape(-1)]
    S, A, N = math.fsum(x), math.fsum(abs(t) for t in x), len(x)
    e = N * 2.0 ** -52 * A
    return F((S - e) / N) == F(S / N) == F((S + e) / N)


def contrast_mean_is_pinned(img_u8, ops):
    """True when the chain's contrast mean cannot depend on the summation order (see the module docstring); chains without one: True."""
    pre, at = before_contrast(img_u8, ops)
    if at < 0:
        return True
    if at == 0:
        return contrast_first_is_exact(img_u8)
    return all(mean_is_order_independent(pre[..., k]) for k in range(3))


# ---------------------------------------------------------------------------------------------------------------- geometry cases
GEOMETRY_IMAGE = (31, 13, 11)                                                     # random_image(seed, h, w)
GEOMETRY_CHAIN = [("contrast", 1.3), ("hue", 0.1), ("brightness", -0.05), ("saturation", 1.2)]       # contrast first: exact mean
GEOMETRY_WINDOWS = {                                                              # (y, x, h, w) on the 13 x 11 image
    "inside_7x5": (3, 2, 7, 5),                                                   # -> 33 x 31: a non-dyadic up-scale
    "whole": (0, 0, 13, 11),                                                      # -> 5 x 4, 1 x 1: down-scales
    "one_row": (4, 1, 1, 9),                                                      # y1 = min(y0 + 1, wh - 1) collapses
    "one_column": (2, 5, 9, 1),
    "one_pixel": (6, 6, 1, 1),
    "leaves_top": (-3, 2, 8, 6),
    "leaves_bottom": (9, 2, 8, 6),
    "leaves_left": (3, -4, 6, 8),
    "leaves_right": (3, 7, 6, 8),
    "leaves_all": (-2, -3, 18, 17),
    "outside": (40, 40, 5, 5),
    "outside_negative": (-20, 3, 4, 4),
}
GEOMETRY_OUT_SHAPES = [(1, 1), (8, 32), (9, 33), (7, 31), (8, 33), (33, 31), (5, 4)]      # the 32 x 8 tile: exact, one over, one under, per axis


def geometry_items(flips):
    """[(name, ops, window, flip)] - every window under every flip mode, identity colour and the 4-op chain."""
    return [("%s flip %d %s" % (w, f, "chain" if ops else "identity"), ops, win, f)
            for w, win in GEOMETRY_WINDOWS.items() for f in flips for ops in ([], GEOMETRY_CHAIN)]


# ---------------------------------------------------------------------------------------------------------------- looping sizes
# name -> (source (seed, h, w), chain, window, output shape).  test_augment_exact_cpu.py computes the trip counts from the constants above.
LOOPING = {
    "output_second_trip": ((41, 61, 47), [("hue", 0.1)], (0, 0, 61, 47), (1032, 1024)),                   # augment_kernel: 1 056 768 > 1 048 576
    "mean_second_trip": ((42, 520, 512), [("contrast", 1.5), ("saturation", 1.2)], (0, 0, 520, 512), (520, 512)),     # aug_mean_kernel: 266 240 > 262 144
    "batch_mean_above_cap": ((43, 1032, 1024), [("contrast", 0.5), ("hue", -0.1)], (0, 0, 1032, 1024), (520, 512)),   # 516 workgroups wanted, 512 given
}
LOOPING_BATCH_OUT = (520, 512)


def looping_batch():
    """The batch around the 1032 x 1024 contrast-first source: an op-free item before and after it, a second contrast item last, so that the
    segment search of aug_mean_batch_kernel meets items that own no workgroup at the start and in the middle.  -> (images, items)"""
    src, chain, win, _ = LOOPING["batch_mean_above_cap"]
    small, other = noisy_image(44, 40, 56), noisy_image(45, 90, 70)
    return ([small, noisy_image(*src), small, other],
            [([], (3, 4, 30, 40), FLIP_RESIZED), (chain, win, FLIP_NONE), ([("hue", 0.15)], (-5, -5, 50, 66), FLIP_WINDOW),
             ([("contrast", 1.5), ("brightness", 0.05)], (10, 5, 70, 60), FLIP_NONE)])


# contrast not first, on images whose pre-contrast channel sums are order-independent (asserted on the CPU): the batched mean, the
# per-image mean and numpy's pairwise float64 mean are then one float32, and the three results are bit-identical
CONTRAST_LATER = {
    "noisy_96x128_middle": ((51, 96, 128), [("saturation", 0.7), ("brightness", 0.08), ("contrast", 0.6), ("hue", -0.15)], (5, 7, 80, 100), 1),
    "noisy_333x333_last": ((52, 333, 333), [("brightness", 0.1), ("saturation", 1.4), ("hue", 0.17), ("contrast", 1.5)], (33, 1, 300, 299), 0),
    "noisy_50x60_second": ((53, 50, 60), [("hue", 0.1), ("contrast", 1.1), ("brightness", -0.1)], (-8, -9, 70, 80), 1),
}
CONTRAST_FIRST = {
    "noisy_413x577": ((54, 413, 577), [("contrast", 0.5)], (13, 29, 377, 401), 0),
    "noisy_200x900_chain": ((55, 200, 900), GEOMETRY_CHAIN, (-8, -9, 170, 480), 1),
}
CONTRAST_OUT = (64, 96)
# the call that runs on an output and a workspace filled with NaN patterns: (sources, items, output shape); "palette" = the palette image
ISOLATION = ([(61, 70, 90), "palette", (62, 150, 33)],
             [([("contrast", 1.5), ("hue", 0.1)], (-4, 3, 60, 80), 1), ([], (0, 0, 16, 16), 0), ([("brightness", 0.1), ("contrast", 0.5)], (0, 0, 150, 33), 2)],
             (21, 37))


def isolation_images():
    return [np.array(palette()) if s == "palette" else noisy_image(*s) for s in ISOLATION[0]]


# ---------------------------------------------------------------------------------------------------------------- runners (GPU)
@functools.lru_cache(maxsize=None)
def palette_refs():
    """name -> oracle result of the palette under that chain; computed once, read-only."""
    out = {}
    for name in PALETTE_ORDER:
        r = oracle(palette(), PALETTE_CHAINS[name][0], PALETTE_WINDOW, 0, PALETTE_OUT)
        r.setflags(write=False)
        out[name] = r
    return out


@functools.lru_cache(maxsize=None)
def geometry_refs(out_shape):
    img = random_image(*GEOMETRY_IMAGE)
    out = {}
    for name, ops, win, flip in geometry_items((0, 1, 2)):
        r = oracle(img, ops, win, flip, out_shape)
        r.setflags(write=False)
        out[name] = r
    return out


def run_palette(dev):
    """The palette under every chain through both entry points; the batch holds all chains as separate items of one call."""
    from dan_amd.preprocessing import dan_preprocessing as P
    refs, timg = palette_refs(), torch.from_numpy(np.array(palette())).to(dev)
    for name in PALETTE_ORDER:
        assert_exact(P.augment_image(timg, PALETTE_CHAINS[name][0], PALETTE_WINDOW, False, PALETTE_OUT), refs[name], "palette %s, per image" % name)
    out = P.augment_batch([timg] * len(PALETTE_ORDER), [(PALETTE_CHAINS[n][0], PALETTE_WINDOW, 0) for n in PALETTE_ORDER], PALETTE_OUT)
    for k, name in enumerate(PALETTE_ORDER):
        assert_exact(out[k], refs[name], "palette %s, batch item %d" % (name, k))
    return 2 * len(PALETTE_ORDER)


def run_geometry(out_shape, dev, per_image=True, batch=True):
    """Every window x flip x {identity, chain} at one output shape; flip 2 through the batch only."""
    from dan_amd.preprocessing import dan_preprocessing as P
    refs, timg = geometry_refs(tuple(out_shape)), torch.from_numpy(random_image(*GEOMETRY_IMAGE)).to(dev)
    n = 0
    if per_image:
        for name, ops, win, flip in geometry_items((0, 1)):
            assert_exact(P.augment_image(timg, ops, win, bool(flip), out_shape), refs[name], "%s -> %s, per image" % (name, out_shape))
            n += 1
    if batch:
        items = geometry_items((0, 1, 2))
        out = P.augment_batch([timg] * len(items), [(ops, win, flip) for _, ops, win, flip in items], out_shape)
        assert tuple(out.shape) == (len(items), out_shape[0], out_shape[1], 8)
        for k, (name, _, _, _) in enumerate(items):
            assert_exact(out[k], refs[name], "%s -> %s, batch item %d" % (name, out_shape, k))
            n += 1
    return n


def run_fp16_group(dev):
    """What the fp16 child runs: the palette and two output shapes of the geometry cases (the arithmetic is float32 in both builds; the
    16-bit convert and the store are what differs)."""
    return run_palette(dev) + run_geometry((9, 33), dev) + run_geometry((33, 31), dev)
