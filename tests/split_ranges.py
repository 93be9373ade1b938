"""Helpers for testing the split-operand path (csrc/split_infer.hip, ops.SPLIT_EVAL) away from the value ranges of a freshly initialised
network: an fp64 reference with a scale-invariant per-element bound, an fp64 emulation of the limb arithmetic, and function-preserving
power-of-two rescaling of the oracle's parameters.  A plain module (imported by the tests), not a conftest.

Error model of one split product.  x = hi + lo with hi = half(x), lo = half(x - hi): |x - hi - lo| <= 2^-22 |x| while both limbs are normal
numbers (the same for w).  The kernels form hi.hi + lo.hi + hi.lo, each product exact in fp32, so one product x.w is off by at most
2^-22 (x's limbs) + 2^-22 (w's limbs) + 2^-22 (the dropped lo.lo) = 3 * 2^-22 of |x||w|.  Summed over the reduction this is 3 * 2^-22 * A,
A = sum |x||w| + |b|.  The kernels accumulate in fp32 in blocks of 32 (one MFMA) and then serially over K / 32 steps; the rounding of
those partial sums is a random walk of 2^-24-sized steps relative to A, a few 2^-22 A at K = 13824 (3 x 3 x 1536 limb channels).  A
limb-layout output is split once more (2^-22 |y| <= 2^-22 A).  C_BOUND = 16 covers the sum of those terms.

Both sides of `|got - ref| <= C_BOUND * 2^-22 * A` scale together with x and w, so the bound holds at every scale of a correct
implementation, and an error that grows when x or w move away from 1 (a subnormal limb, an overflowing limb, a lost exponent) shows up as
a failure instead of hiding under a tolerance relative to max|ref|.

The one scale-dependent term is the limbs' own floor.  A limb map holds v * 2^-e (e: its exponent, ops.LIMB_EXP for the maps the split path
writes); a value below 2^-3 of that scale has a subnormal lo limb, so its error is that of a value AT 2^(e-3): 2^(e-25) absolute (the same
holds for weights, whose tensors carry max|w| in [2^13, 2^14)).  magnitude() therefore sums max(|x|, x_floor) * max(|w|, w_floor) and adds
y_floor for a limb-layout output: with floors = 2^-3 of the scales (floors()) the bound holds at every scale too; with the floors at zero
it is the pure relative bound, which an implementation without exponents fails by orders of magnitude as soon as w or x move away from 1.
"""
import math

import torch
import torch.nn.functional as F

C_BOUND = 16.0
EPS = 2.0 ** -22
# the documented exponent of the limb maps the split path writes (dan_amd/ops.py LIMB_EXP): maps are carried as limbs of x * 2^-2, i.e.
# |x| < 65520 * 4 = 262080, to 22 bits from |x| >= 2^(2-3) = 0.5 and with an absolute error of 2^(2-25) = 2^-23 below (4 x that of
# unscaled limbs).  Fixed here, not read from the code under test, so that the tolerance cannot move with an implementation constant.
MAP_EXP = 2

# consecutive convolutions of the VGG trunk (oracle.nets.get_featmaps) whose first member's output feeds only the second one, directly
# or through a 2x2 max-pool: conv_l's kernel and bias times 2^s and conv_{l+1}'s kernel times 2^-s leave the network unchanged
TRUNK_PAIRS = [("conv1/conv1_1", "conv1/conv1_2"), ("conv1/conv1_2", "conv2/conv2_1"), ("conv2/conv2_1", "conv2/conv2_2"),
               ("conv2/conv2_2", "conv3/conv3_1"), ("conv3/conv3_1", "conv3/conv3_2"), ("conv3/conv3_2", "conv3/conv3_3"),
               ("conv4/conv4_1", "conv4/conv4_2"), ("conv4/conv4_2", "conv4/conv4_3"), ("conv5/conv5_1", "conv5/conv5_2"),
               ("conv5/conv5_2", "conv5/conv5_3"), ("fc6", "fc7")]


def _same_pads(n, k, s):
    out = -(-n // s)
    total = max((out - 1) * s + k - n, 0)
    return total // 2, total - total // 2


def conv64(x, w, stride=1, padding="same"):
    """fp64 NHWC x HWIO convolution with TF's 'same' (asymmetric) or 'valid' padding."""
    x = x.double().permute(0, 3, 1, 2)
    w = w.double().permute(3, 2, 0, 1)
    kh, kw = w.shape[2], w.shape[3]
    if padding == "same":
        pt, pb = _same_pads(x.shape[2], kh, stride)
        pl, pr = _same_pads(x.shape[3], kw, stride)
        x = F.pad(x, (pl, pr, pt, pb))
    return F.conv2d(x, w, stride=stride).permute(0, 2, 3, 1)


def magnitude_parts(x, w, stride=1, padding="same"):
    """The fp64 sums the bound is built from: |x| * |w|, [x != 0] * |w|, |x| * [w != 0] and [x != 0] * [w != 0] (convolutions)."""
    mx, mw = (x != 0).double(), (w != 0).double()
    return (conv64(x.abs(), w.abs(), stride, padding), conv64(mx, w.abs(), stride, padding), conv64(x.abs(), mw, stride, padding),
            conv64(mx, mw, stride, padding))


def magnitude(parts, b=None, sx=1.0, sw=1.0, x_floor=0.0, w_floor=0.0, y_floor=0.0):
    """A for x * sx and w * sw (powers of two) from magnitude_parts(x, w): sum max(|x|, x_floor) * max(|w|, w_floor) over the nonzero operands
    (bounded by the four parts), + |b| + y_floor.  The floors are the smallest magnitudes the limbs carry to 22 bits (2^-3 of a map's or weight
    tensor's scale, see the module docstring); 0 = none."""
    axw, mxw, axm, mxm = parts
    A = sx * sw * axw + x_floor * sw * mxw + sx * w_floor * axm + x_floor * w_floor * mxm + y_floor
    return A + b.double().abs() if b is not None else A


def reference(x, w, b=None, stride=1, padding="same", relu=False, x_floor=0.0, w_floor=0.0, y_floor=0.0):
    """-> (ref, A): the fp64 convolution of the exact fp32 operands (bias, ReLU) and the fp64 magnitude sum |x| * |w| + |b| (with floors:
    magnitude())."""
    ref = conv64(x, w, stride, padding)
    if b is not None:
        ref = ref + b.double()
    if relu:
        ref = ref.clamp_min(0)
    if x_floor == 0.0 and w_floor == 0.0:
        A = conv64(x.abs(), w.abs(), stride, padding) + y_floor
        return ref, (A + b.double().abs() if b is not None else A)
    return ref, magnitude(magnitude_parts(x, w, stride, padding), b, x_floor=x_floor, w_floor=w_floor, y_floor=y_floor)


def floors(x_exp=None, w_exp=None, y_exp=None):
    """(x_floor, w_floor, y_floor) of maps with exponents x_exp / y_exp (limbs of v * 2^-exp) and weights with exponent w_exp (limbs of
    w * 2^w_exp); None = that operand is not carried in limbs (fp32)."""
    f = lambda e: 0.0 if e is None else 2.0 ** (e - 3)
    return f(x_exp), (0.0 if w_exp is None else 2.0 ** (-w_exp - 3)), f(y_exp)


def assert_not_vacuous(ref, A, c=C_BOUND, what=""):
    """The bound must be able to fail: an all-zero result has to exceed it somewhere."""
    assert bool((ref.abs() > c * EPS * A).any()), "%s: the bound admits an all-zero result" % what


def check(got, ref, A, c=C_BOUND, what=""):
    """Asserts |got - ref| <= c * 2^-22 * A elementwise (a NaN or inf in got fails); the message names the worst element, its A and how
    many elements fail."""
    got = got.detach().double().cpu()
    err = (got - ref).abs()
    lim = c * EPS * A
    bad = ~(err <= lim)
    if bool(bad.any()):
        ratio = torch.where(torch.isfinite(err), err / lim.clamp_min(1e-300), torch.full_like(err, math.inf))
        i = int(ratio.flatten().argmax())
        idx = tuple(int(v) for v in torch.unravel_index(torch.tensor(i), ratio.shape))
        raise AssertionError("%s: %d of %d elements exceed %g * 2^-22 * A; worst at %s: got %r, ref %r, A %r (%.3g x the bound)"
                             % (what, int(bad.sum()), bad.numel(), c, idx, float(got[idx]), float(ref[idx]), float(A[idx]), float(ratio[idx])))


def limbs(x, exp=0):
    """The two IEEE-half limbs of x * 2^-exp (as the split kernels store them), widened to fp64."""
    xs = x.float() * 2.0 ** -exp
    hi = xs.half()
    lo = (xs - hi.float()).half()
    return hi.double(), lo.double()


def weight_exp(w):
    """The weights' exponent of the split path: max|w * 2^e| in [2^13, 2^14) (ops._weight_exp)."""
    m = float(w.abs().max())
    return 0 if m == 0.0 else 14 - math.frexp(m)[1]


def emulate_split_conv(x, w, b=None, stride=1, padding="same", relu=False, x_exp=0, w_exp=0):
    """The split product hi.hi + lo.hi + hi.lo with x's limbs holding x * 2^-x_exp and w's limbs w * 2^w_exp; fp64 sums stand in for the
    MFMA's exact products and fp32 accumulation.  x_exp = w_exp = 0: the limbs without any scaling.  ReLU as the kernels' epilogue takes it
    (v_max_f32 0, v: a NaN becomes 0)."""
    xh, xl = limbs(x, x_exp)
    wh, wl = limbs(w, -w_exp)
    acc = conv64(xh, wh, stride, padding) + conv64(xl, wh, stride, padding) + conv64(xh, wl, stride, padding)
    v = acc * 2.0 ** (x_exp - w_exp)
    if b is not None:
        v = v + b.double()
    if relu:
        v = torch.where(v > 0, v, torch.zeros_like(v))
    return v


def heavy_tailed(shape, gen, sigma=1.0):
    """Half-zero activations with a heavy tail: relu(sign * exp(N(0, sigma))), about 2^-7 .. 2^7 at sigma = 1."""
    sign = torch.where(torch.rand(shape, generator=gen) < 0.5, -1.0, 1.0)
    return torch.relu(sign * torch.exp(sigma * torch.randn(shape, generator=gen)))


def spread_weights(shape, gen, spread_log2=12):
    """HWIO weights randn / sqrt(fan-in) whose per-output-channel scale spreads over 2^-spread_log2 .. 1 within the tensor."""
    kh, kw, ci, co = shape
    w = torch.randn(shape, generator=gen) / math.sqrt(kh * kw * ci)
    return w * torch.pow(2.0, -spread_log2 * torch.linspace(0, 1, co))


def rescale_params(P, pairs):
    """Oracle Params with conv_l's kernel and bias times 2^s and conv_{l+1}'s kernel times 2^-s for every (l, l+1, s) in pairs (scopes as in
    TRUNK_PAIRS; a scope may appear in several pairs, the factors multiply).  The network is unchanged in exact and in fp32 arithmetic:
    power-of-two factors commute with every rounding, with ReLU and with max-pool."""
    from oracle import nets as ON
    t = dict(P.t)
    for first, second, s in pairs:
        assert (first, second) in TRUNK_PAIRS, (first, second)
        for name, f in ((first + "/conv2d/kernel", 2.0 ** s), (first + "/conv2d/bias", 2.0 ** s), (second + "/conv2d/kernel", 2.0 ** -s)):
            t[name] = t[name] * f
    return ON.Params(t)
