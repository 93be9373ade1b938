"""Helpers of the transposed-convolution tests (dan_amd/csrc/conv_transpose.hip; the rule: include/danhip.h).

The reference is independent of the code under test: torch.nn.functional.conv_transpose2d(x, w, b, stride=2, padding=1) on the CPU in
float64, with its autograd for both gradients, applied to the values the device sees.  PyTorch's rule is out[oy] += x[iy] w[ky] with
oy = 2 iy - 1 + ky - the header's - with the weight laid out [Cin, Cout, ky, kx], so the variable W [4, 4, Cout, Cin] goes in permuted.

The exact cases hold integers only: x, W and dOut ternary at a density that keeps about 64 non-zero products per output, bias / lateral /
the accumulate-into-slot start value small integers.  Every partial sum of any summation order is then an integer below 2^24 (fp32 adds
them without rounding) and every stored 16-bit value an integer of magnitude <= 256 (bf16 and fp16 hold those exactly), so the comparison
is an equality whatever order the kernel sums in; check_inputs asserts exactly that on the reference alone."""
import functools
import os
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from conv_exact import F64, LIMIT16, assert_equal, signs, small, ternary  # noqa: E402,F401

PRODUCTS = 64            # expected non-zero products per output element of the forward and of the data gradient
# The kernels' tiles (conv_transpose_plan.h): forward and data gradient own 128 consecutive pixels (n, y, x) of the INPUT grid, flat over
# the batch; the weight gradient walks the same pixels in K steps of 64.  9 x 17 = 153 pixels cross the 128-pixel tile edge by one row
# (8 x 17 = 136 > 128 > 7 x 17) and, against an 8 x 16 window, by one column.
TILE_PIXELS = 128
WGRAD_STEP = 64
MAPS = ((1, 1), (1, 3), (3, 1), (5, 7), (9, 17))
CHANNELS = ((64, 64), (128, 64), (64, 128))


def _case(N, Hi, Wi, crop, cin, cout, kind="random"):
    name = "%s_n%d_%dx%d_%s_%dto%d" % (kind, N, Hi, Wi, "crop" if crop else "full", cin, cout)
    return dict(name=name, N=N, Hi=Hi, Wi=Wi, Ho=2 * Hi - int(crop), Wo=2 * Wi - int(crop), Cin=cin, Cout=cout, kind=kind)


def all_cases():
    cases = [_case(N, h, w, crop, ci, co) for (h, w) in MAPS for crop in (False, True) for (ci, co) in CHANNELS for N in (1, 3)]
    cases += [_case(1, 3, 5, crop, 512, 512) for crop in (False, True)]            # the K loop runs more than one round per tap
    cases += [_case(N, h, w, crop, 64, 64, "taps") for (h, w) in ((1, 1), (5, 7), (9, 17)) for crop in (False, True) for N in (1, 3)]
    return cases


def tap_counts(n_in, n_out):
    """How many (input position i, tap k) pairs reach each output position o = 2 i + k - 1 of one axis, counted by enumeration: 1 at the first
    and at the last position of the FULL 2 n_in map, 2 in between."""
    out = []
    for o in range(n_out):
        out.append(sum(1 for i in range(n_in) for k in range(4) if 2 * i + k - 1 == o))
    return out


@functools.lru_cache(maxsize=None)
def _inputs(name):
    c = {k["name"]: k for k in all_cases()}[name]
    g = torch.Generator().manual_seed(abs(hash_name(name)) % (1 << 31))
    N, Hi, Wi, Ho, Wo, Cin, Cout = (c[k] for k in ("N", "Hi", "Wi", "Ho", "Wo", "Cin", "Cout"))
    if c["kind"] == "taps":
        x, w, b = torch.ones((N, Hi, Wi, Cin), dtype=F64), torch.ones((4, 4, Cout, Cin), dtype=F64), torch.zeros(Cout, dtype=F64)
        dout = ternary((N, Ho, Wo, Cout), PRODUCTS / (16.0 * Cout), g)
    else:
        p = min(1.0, (PRODUCTS / (4.0 * Cin)) ** 0.5)                      # forward: 4 Cin products per interior output
        x, w = ternary((N, Hi, Wi, Cin), p, g), ternary((4, 4, Cout, Cin), p, g)
        b = small((Cout,), g)
        dout = ternary((N, Ho, Wo, Cout), min(1.0, PRODUCTS / (16.0 * Cout * p)), g)     # data gradient: 16 Cout products
    lateral = small((N, Ho, Wo, Cout), g, lo=-8, hi=0 if c["kind"] == "taps" else 8)      # (taps: the interior is 4 Cin = 256 already)
    dx0 = small((N, Hi, Wi, Cin), g)                                       # what the gradient slot holds before an accumulating delivery
    return dict(c, x=x, w=w, b=b, lateral=lateral, dout=dout, dx0=dx0)


def hash_name(name):
    h = 0
    for ch in name:
        h = (h * 131 + ord(ch)) % 2147483629
    return h


def inputs(case):
    return _inputs(case["name"])


def reference(x, w, b, lateral, Ho, Wo, dout=None):
    """float64 on the CPU.  x [N,Hi,Wi,Cin], w [4,4,Cout,Cin], b [Cout] or None, lateral [N,Ho,Wo,Cout] or None ->
    dict(out [N,Ho,Wo,Cout]) and, with dout, dx, dw [4,4,Cout,Cin], db."""
    x = x.to(F64).clone().requires_grad_(dout is not None)
    w = w.to(F64).clone().requires_grad_(dout is not None)
    bb = (b.to(F64) if b is not None else torch.zeros(w.shape[2], dtype=F64)).clone().requires_grad_(dout is not None)
    full = F.conv_transpose2d(x.permute(0, 3, 1, 2), w.permute(3, 2, 0, 1), bb, stride=2, padding=1).permute(0, 2, 3, 1)
    assert full.shape[1] == 2 * x.shape[1] and full.shape[2] == 2 * x.shape[2]
    out = full[:, :Ho, :Wo, :]
    if lateral is not None:
        out = out + lateral.to(F64)
    res = dict(out=out.detach())
    if dout is not None:
        out.backward(dout.to(F64))
        res.update(dx=x.grad, dw=w.grad, db=bb.grad)
    return res


@functools.lru_cache(maxsize=None)
def _expected(name):
    c = _inputs(name)
    return reference(c["x"], c["w"], c["b"], None, c["Ho"], c["Wo"], c["dout"])


def expected(case):
    """The reference of a case, computed once: out WITHOUT lateral (the tests add bias-free / lateral variants by hand: they are sums of
    integers), dx, dw, db."""
    return _expected(case["name"])


def expected_forward(case, with_lateral, with_bias):
    c, e = inputs(case), expected(case)
    out = e["out"] if with_bias else e["out"] - c["b"]
    return out + c["lateral"] if with_lateral else out


def _is_int(t):
    return bool(torch.equal(t, t.round()))


def check_inputs(case):
    """The condition the exact tests rest on, asserted on the reference alone: all values integers, every partial sum below 2^24 in
    magnitude (bounded by the sum of the terms' magnitudes), every 16-bit result within +-256."""
    c, e = inputs(case), expected(case)
    for k in ("x", "w", "b", "lateral", "dout", "dx0"):
        assert _is_int(c[k]) and c[k].abs().max() <= LIMIT16, (case["name"], k)
    mags = reference(c["x"].abs(), c["w"].abs(), c["b"].abs(), c["lateral"].abs(), c["Ho"], c["Wo"], c["dout"].abs())
    for k in ("out", "dx", "dw", "db"):
        assert _is_int(e[k]), (case["name"], k)
        bound = mags[k] + (c["dx0"].abs() if k == "dx" else 0)
        assert bound.max() < 2 ** 24, (case["name"], k, bound.max().item())
    # what is stored in 16 bits: the forward in all four bias / lateral variants, the data gradient with and without the slot's old value
    for lat in (False, True):
        for bias in (False, True):
            assert expected_forward(case, lat, bias).abs().max() <= LIMIT16, (case["name"], "out", lat, bias)
    assert e["dx"].abs().max() <= LIMIT16 and (e["dx"] + c["dx0"]).abs().max() <= LIMIT16, (case["name"], "dx")


def deconv_initializer(cout, cin):
    """kernel[ky, kx, co, ci] = f[ky] f[kx] delta(co, ci), f = (0.25, 0.75, 0.75, 0.25) - the formula of the issue, written independently of
    dan_amd.net.variables."""
    f = (0.25, 0.75, 0.75, 0.25)
    k = torch.zeros((4, 4, cout, cin), dtype=F64)
    for ky in range(4):
        for kx in range(4):
            for c in range(min(cout, cin)):
                k[ky, kx, c, c] = f[ky] * f[kx]
    return k
