"""The helpers of tests/split_ranges.py on the CPU: function-preserving rescaling leaves the oracle bit-identical, and the per-element bound
|got - ref| <= C_BOUND * 2^-22 * A passes the limb arithmetic with the split path's power-of-two exponents at every scale while it fails the
limbs without them (small weights, activations above half's range)."""
import pytest
import torch

import split_ranges as S


def test_rescaling_leaves_the_oracle_bit_identical():
    from dan_amd import synthetic
    from oracle import nets as ON
    imgs = synthetic.make_images(1, 96, 128, "cpu", seed=3)
    x = ON.preprocess_synthetic(imgs)
    P = ON.Params(create=True, seed=7)
    with torch.no_grad():
        loc, cls = ON.sfd_forward(P, x)
        P2 = S.rescale_params(P, [("conv1/conv1_1", "conv1/conv1_2", 10), ("conv3/conv3_1", "conv3/conv3_2", -10)])
        assert not torch.equal(P2.t["conv1/conv1_1/conv2d/kernel"], P.t["conv1/conv1_1/conv2d/kernel"])
        loc2, cls2 = ON.sfd_forward(P2, x)
    assert torch.equal(loc, loc2) and torch.equal(cls, cls2)


def _case(seed, ci=256, co=64):
    g = torch.Generator().manual_seed(seed)
    x = S.heavy_tailed((1, 12, 12, ci), g)
    w = S.spread_weights((3, 3, ci, co), g)
    b = 0.1 * torch.randn(co, generator=g)
    return x, w, b


@pytest.mark.parametrize("s", [-16, -8, -4, 0, 4])
@pytest.mark.parametrize("t", [-8, 0, 8])
def test_bound_passes_the_scaled_limbs_at_every_scale(s, t):
    x, w, b = _case(1)
    xs, ws, bs = x * 2.0 ** t, w * 2.0 ** s, b * 2.0 ** (s + t)
    ref, A = S.reference(xs, ws, bs, relu=True)
    got = S.emulate_split_conv(xs, ws, bs, relu=True, x_exp=2, w_exp=S.weight_exp(ws))
    S.check(got, ref, A, what="scaled limbs s=%d t=%d" % (s, t))


@pytest.mark.parametrize("sigma_w", [2e-4, 2e-5])
def test_bound_fails_unscaled_limbs_of_small_weights(sigma_w):
    g = torch.Generator().manual_seed(2)
    x = torch.randn((1, 12, 12, 256), generator=g)
    w = torch.randn((3, 3, 256, 64), generator=g) * sigma_w
    ref, A = S.reference(x, w)
    S.check(S.emulate_split_conv(x, w, x_exp=2, w_exp=S.weight_exp(w)), ref, A, what="scaled")
    with pytest.raises(AssertionError, match="exceed"):
        S.check(S.emulate_split_conv(x, w), ref, A, what="unscaled")


@pytest.mark.parametrize("big", [70000.0, 2.0 ** 17])
def test_bound_fails_an_activation_above_half_range(big):
    """hi = inf, lo = -inf: the product sums to NaN, the ReLU epilogue turns it into 0 - a finite wrong value the bound must catch.  With
    the split path's map exponent (2) the same value is carried."""
    x, w, b = _case(3)
    x[0, 5, 5, :8] = big
    ref, A = S.reference(x, w, b, relu=True)
    got = S.emulate_split_conv(x, w, b, relu=True)
    assert torch.isfinite(got).all()
    with pytest.raises(AssertionError, match="exceed"):
        S.check(got, ref, A, what="unscaled")
    S.check(S.emulate_split_conv(x, w, b, relu=True, x_exp=2, w_exp=S.weight_exp(w)), ref, A, what="scaled")
