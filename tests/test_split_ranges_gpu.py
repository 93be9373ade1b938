"""The split-operand path (csrc/split_infer.hip, precision "split") away from the value ranges of a freshly initialised network: limb conversions
at the edges of half's range, per-layer parity over a sweep of weight and activation scales with the scale-invariant bound of
tests/split_ranges.py, and the evaluation graphs under function-preserving power-of-two rescaling of their parameters.

Documented range (tests/split_ranges.py MAP_EXP = dan_amd/ops.py LIMB_EXP = 2): a map is carried as limbs of x * 2^-2, so |x| < 262080, to
22 bits from |x| >= 0.5 and 2^-23 absolute below; weights of any scale.  Above the range every entry point raises the range flag and
ops.split_range_check() raises SplitRangeError: no finite wrong value, no zeros."""
import ctypes

import numpy as np
import pytest
import torch

import split_ranges as S

pytestmark = pytest.mark.gpu


def _ops():
    from dan_amd import ops
    return ops


def _limit():
    return 65520.0 * 2.0 ** S.MAP_EXP


def test_documented_map_exponent():
    assert _ops().LIMB_EXP == S.MAP_EXP


def _expect_range_error(ops, out_of_range):
    if out_of_range:
        with pytest.raises(ops.SplitRangeError):
            ops.split_range_check()
    else:
        ops.split_range_check()


def _edge_values(lim):
    v = [1.0, -2.0, 0.5, 1024.0, -3.0, 0.0, -0.0]                                          # exact halves (lo = 0), +-0
    v += [2.0 ** -24, -(2.0 ** -20), 3 * 2.0 ** -17, 2.0 ** -14, 1.5 * 2.0 ** -15]           # subnormal in half
    v += [0.125 * (1 + 2.0 ** -k) for k in (1, 5, 12, 20)] + [0.125 * (1 - 2.0 ** -k) for k in (2, 11, 22)]   # lo turns subnormal
    v += [65504.0, -65504.0, 65519.0, 65503.99, 65504.5]                                    # around half's largest value
    v += [2.0 ** 17, -(2.0 ** 17) * 1.3, 2.0 ** 17 + 3.0, lim * 0.9999]                     # inside the map range
    return torch.tensor(v, dtype=torch.float32)


def _over_values(lim):
    return torch.tensor([lim, -lim * 1.01, 2.0 ** 20, float("inf")], dtype=torch.float32)


def _close(got, want, exp):
    """hi + lo of a value within 2^-22 |x| + 2^-25 of the map's scale 2^exp."""
    err = (got.double().cpu() - want.double()).abs()
    lim = 2.0 ** -22 * want.double().abs() + 2.0 ** -25 * 2.0 ** exp
    assert (err <= lim).all(), (got[~(err <= lim)], want[~(err <= lim)])


@pytest.mark.parametrize("C", [4, 3, 5])                 # split3_vec4_kernel, split3_c3_kernel, split3_any_kernel
@pytest.mark.parametrize("exp", [0, 2])
def test_split3_and_unsplit3_at_range_edges(C, exp, dev):
    ops = _ops()
    ops.split_range_check()
    lim = 65520.0 * 2.0 ** exp
    v = _edge_values(lim)
    v = v[v.abs() < lim]
    x = v.repeat(C).view(C, -1).t().contiguous().view(1, 1, -1, C)
    xv = ops._limb_view(ops.split3(x.to(dev), exp), C, exp)
    _expect_range_error(ops, False)
    _close(ops.unsplit3(xv), x, exp)
    for bad in _over_values(lim):
        y = x.clone()
        y[0, 0, 3, C - 1] = bad
        ops.split3(y.to(dev), exp)
        _expect_range_error(ops, True)


def _identity_conv(ops, x, k, dev):
    """A convolution that reproduces its input (centre tap = identity): the epilogue's limb writer sees exactly the input values."""
    C = x.shape[-1]
    w = torch.zeros((k, k, C, C))
    w[k // 2, k // 2] = torch.eye(C)
    with ops.use_context(ops.OpsContext(SPLIT_EVAL=True)), torch.no_grad():
        y = ops.conv2d(x.to(dev), w.to(dev), torch.zeros(C, device=dev), relu=False)
    assert ops._is_limbs(y)
    return y


@pytest.mark.parametrize("N,H,W,C,k", [(1, 4, 16, 8, 1), (2, 96, 96, 64, 3)])        # flat-M conv_store4, halo general epilogue
def test_conv_epilogue_limbs_at_range_edges(N, H, W, C, k, dev):
    ops = _ops()
    ops.split_range_check()
    lim = _limit()
    v = _edge_values(lim)
    x = v[torch.arange(N * H * W * C) % v.numel()].view(N, H, W, C)
    y = _identity_conv(ops, x, k, dev)
    _expect_range_error(ops, False)
    _close(ops.unsplit3(y), x, S.MAP_EXP)
    base = x * (x.abs() < lim / 4)                   # in range even after the doubling below: only the inserted element can overflow
    for bad in (lim, -1.01 * lim, 1.9 * lim):
        x2 = base.clone()
        x2[0, 1, 2, 5] = bad / 2                       # in range at the input, out of range after the doubling weight
        w = torch.zeros((k, k, C, C))
        w[k // 2, k // 2] = 2 * torch.eye(C)
        with ops.use_context(ops.OpsContext(SPLIT_EVAL=True)), torch.no_grad():
            ops.conv2d(x2.to(dev), w.to(dev), None, relu=False)
        _expect_range_error(ops, True)


def test_first_layer_maxpool_and_l2norm_limbs_at_range_edges(dev):
    """danhip_conv3x3_c3_f32_split3 (centre tap copies the 3 image channels), danhip_maxpool2x2_split3 on its limbs, danhip_l2norm_split3."""
    ops = _ops()
    ops.split_range_check()
    lim = _limit()
    v = _edge_values(lim)
    x = v[torch.arange(2 * 8 * 12 * 3) % v.numel()].view(2, 8, 12, 3)
    w = torch.zeros((3, 3, 3, 64))
    w[1, 1, :, :3] = torch.eye(3)
    with ops.use_context(ops.OpsContext(SPLIT_EVAL=True)), torch.no_grad():
        y = ops.conv2d(x.to(dev), w.to(dev), None, relu=False)
        assert ops._is_limbs(y)
        _expect_range_error(ops, False)
        yf = ops.unsplit3(y)
        _close(yf[..., :3], x, S.MAP_EXP)
        assert (yf[..., 3:] == 0).all()
        p = ops.max_pool_2x2(y)
        assert ops._is_limbs(p)
        want = ops.max_pool_2x2(yf.contiguous())
        _expect_range_error(ops, False)
        assert torch.equal(ops.unsplit3(p), want)
        for bad in _over_values(lim)[:3]:
            x2 = x.clone()
            x2[1, 3, 4, 2] = bad
            ops.conv2d(x2.to(dev), w.to(dev), None, relu=False)
            _expect_range_error(ops, True)
        g = torch.Generator().manual_seed(1)
        m = (torch.randn((1, 6, 6, 64), generator=g) * 1000).to(dev)
        mv = _identity_conv(ops, m, 1, dev)
        gamma = torch.full((64,), 10.0, device=dev)
        n = ops.l2_normalize(mv, gamma)
        _expect_range_error(ops, False)
        want = ops.l2_normalize(ops.unsplit3(mv), gamma)
        assert (ops.unsplit3(n) - want).abs().max().item() <= 2.0 ** -20 * want.abs().max().item()
        ops.l2_normalize(mv, torch.full((64,), 2.0 ** 20, device=dev))        # |y| up to gamma: beyond the limbs of exponent 0
        _expect_range_error(ops, True)


# ---- per-layer parity over a scale sweep
CASES = {
    # name: (N, H, W, Cin, Cout, k, stride, relu, out_f32, kernel label prefix)
    "halo": (2, 96, 96, 64, 128, 3, 1, True, False, "conv3x3_halo_kernel"),
    "flat_m": (2, 48, 40, 64, 64, 3, 1, True, False, "conv_igemm_kernel<256, 64, 1, true>"),
    "split_k": (1, 10, 10, 512, 512, 3, 1, True, False, "conv_igemm_kernel<128, 128, 2, true>"),
    "stride2": (2, 33, 31, 128, 256, 3, 2, True, False, "conv_igemm_kernel<128, 128, 2, true>"),
    "ragged85": (1, 40, 40, 85, 64, 3, 1, True, False, "conv_igemm_kernel<256, 64, 1, true>"),
    "ragged72": (1, 40, 40, 72, 64, 3, 1, True, False, "conv_igemm_kernel<256, 64, 1, false>"),
    "head6": (1, 40, 40, 512, 6, 3, 1, False, True, "conv_igemm_kernel<64, 16, 1, true>"),
    "head8": (1, 20, 20, 256, 8, 3, 1, False, True, "conv_igemm_kernel<64, 16, 1, true>"),
    "first": (1, 64, 96, 3, 64, 3, 1, True, False, None),
    "pointwise": (1, 20, 20, 1024, 1024, 1, 1, True, False, "conv_igemm_kernel<128, 128, 2, true>"),
}
S_W = [-16, -8, -4, 0, 4]
T_X = [-8, 0, 8, 14]


def _inputs(name, N, H, W, Cin, Cout, k):
    g = torch.Generator().manual_seed(sum(map(ord, name)))
    if name == "first":
        x = torch.randint(0, 256, (N, H, W, 3), generator=g).float() - torch.tensor([123.68, 116.78, 103.94])
    else:
        x = S.heavy_tailed((N, H, W, Cin), g)
    w = S.spread_weights((k, k, Cin, Cout), g)
    b = 0.1 * torch.randn(Cout, generator=g) * w.abs().amax(dim=(0, 1, 2)) * 16
    return x, w, b


@pytest.mark.parametrize("name", list(CASES))
def test_split_conv_over_a_scale_sweep(name, dev):
    ops = _ops()
    from dan_amd import _lib
    N, H, W, Cin, Cout, k, stride, relu, out_f32, label = CASES[name]
    C3 = (3 * Cin + 7) // 8 * 8
    d3 = ops._desc(N, H, W, C3, Cout, k, k, stride, False)
    if label is not None:
        assert _lib.lib_f16().danhip_conv_kernel_label(ctypes.byref(d3), 0).decode().startswith(label)
    if name == "split_k":
        assert _lib.lib_f16().danhip_conv2d_workspace_bytes(ctypes.byref(d3), 0) > 0
    x, w, b = _inputs(name, N, H, W, Cin, Cout, k)
    ref, _ = S.reference(x, w, b, stride=stride, relu=relu)
    parts = S.magnitude_parts(x, w, stride)
    xmax, ymax = float(x.abs().max()), float(ref.abs().max())
    lim = _limit()
    ops.split_range_check()
    failures = []
    for s in S_W:
        for t in T_X:
            f = 2.0 ** (s + t)
            over = xmax * 2.0 ** t >= lim and name != "first"
            over |= (not out_f32) and ymax * f >= lim
            ws = w * 2.0 ** s
            with ops.use_context(ops.OpsContext(SPLIT_EVAL=True)), torch.no_grad():
                y = ops.conv2d((x * 2.0 ** t).to(dev), ws.to(dev), (b * f).to(dev), stride=stride, relu=relu, out_f32=out_f32)
                assert ops._is_limbs(y) != out_f32
                got = ops._f32_in(y)
            try:
                _expect_range_error(ops, over)
                if not over:
                    what = "%s s=%d t=%d" % (name, s, t)
                    fx, fw, fy = S.floors(None if name == "first" else S.MAP_EXP, S.weight_exp(ws), None if out_f32 else S.MAP_EXP)
                    A = S.magnitude(parts, b * f, 2.0 ** t, 2.0 ** s, fx, fw, fy)
                    if out_f32 or (s, t) != (-16, -8):
                        S.assert_not_vacuous(ref * f, A, what=what)
                    else:                                  # outputs near 2^-24 of their usual scale: the whole map lies below the
                        assert ymax * f < 2.0 ** (S.MAP_EXP - 3)   # documented floor of a limb map, where the bound cannot be tight
                    S.check(got, ref * f, A, what=what)
            except (AssertionError, pytest.fail.Exception) as e:
                msg = "%s s=%d t=%d: %s" % (name, s, t, str(e).splitlines()[0][:200])
                if over:                                   # no error raised: say what was returned instead
                    msg += "; returned %d zeros where ref != 0, max |got - ref| / max |ref| = %.3g" % (
                        int(((got.cpu() == 0) & (ref * f != 0)).sum()), float((got.double().cpu() - ref * f).abs().max() / (ymax * f)))
                failures.append(msg)
    assert not failures, "\n".join(failures)


def test_split_conv_batch_slices_with_small_weights(dev):
    """The >2^31-element batch-slice path (_conv2d_split) with weights at 2^-8 of their usual scale."""
    ops = _ops()
    g = torch.Generator(device=dev).manual_seed(4)
    x = torch.randn((6, 160, 160, 6144), generator=g, device=dev)
    w = (torch.randn((1, 1, 6144, 8), generator=torch.Generator().manual_seed(5)) / 6144 ** 0.5) * 2.0 ** -8
    with ops.use_context(ops.OpsContext(SPLIT_EVAL=True)), torch.no_grad():
        got = ops._f32_in(ops.conv2d(x, w.to(dev), None, relu=False))
    ops.split_range_check()
    for n in (0, 5):                                          # first and last slice
        xs = x[n, ::7, ::5].cpu()
        ref, A = S.reference(xs.unsqueeze(0), w, x_floor=S.floors(S.MAP_EXP)[0], w_floor=S.floors(None, S.weight_exp(w))[1])
        S.assert_not_vacuous(ref, A, what="image %d" % n)
        S.check(got[n, ::7, ::5].unsqueeze(0), ref, A, what="image %d" % n)


# ---- whole graphs under function-preserving rescaling
def _assert_oracle_unchanged(P, P2, x, forward):
    from oracle import nets as ON
    with torch.no_grad():
        ref = forward(ON.Params(P.t), x)
        out = forward(P2, x)
    flat = lambda o: [t for pair in (o if isinstance(o[0], tuple) else (o,)) for t in pair]
    assert all(torch.equal(u, v) for u, v in zip(flat(ref), flat(out)))      # the oracle does not see the rescaling


def _trained_like(P, x, forward):
    """Trunk weights x 2^-6 on every second layer with the activations between them x 2^6 (trained VGG trunks: small weights, large maps)."""
    P2 = S.rescale_params(P, [(a, b, 6) for a, b in S.TRUNK_PAIRS[0::2]])
    _assert_oracle_unchanged(P, P2, x, forward)
    return P2


def _overflowing(P, x, forward, lo_log2, hi_log2):
    """s on conv2_1 -> conv2_2 chosen from the oracle's own maximum of conv2_1's output so that it lands in [2^lo, 2^hi)."""
    from oracle import tf_ops as T
    a = T.conv2d_same(x, P.t["conv1/conv1_1/conv2d/kernel"], P.t["conv1/conv1_1/conv2d/bias"], relu=True)
    a = T.conv2d_same(a, P.t["conv1/conv1_2/conv2d/kernel"], P.t["conv1/conv1_2/conv2d/bias"], relu=True)
    a = T.max_pool_2x2_same(a)
    a = T.conv2d_same(a, P.t["conv2/conv2_1/conv2d/kernel"], P.t["conv2/conv2_1/conv2d/bias"], relu=True)
    m = float(a.abs().max())
    s = int(np.floor(lo_log2 - np.log2(m))) + 1
    assert 2.0 ** lo_log2 <= m * 2.0 ** s < 2.0 ** hi_log2, (m, s)
    P2 = S.rescale_params(P, [("conv2/conv2_1", "conv2/conv2_2", s)])
    _assert_oracle_unchanged(P, P2, x, forward)
    return P2


@pytest.mark.parametrize("kind", ["trained_like", "overflow_in_range", "overflow_beyond"])
@pytest.mark.parametrize("which", ["sfd", "dan"])
def test_eval_graph_under_rescaling(which, kind, dev):
    from oracle import nets as ON
    from test_eval_f32_gpu import SIZES, dan_eval_case, single_stage_case
    h, w = SIZES[0]
    fwd = ON.sfd_forward if which == "sfd" else (lambda P, xx: ON.dan_forward(P, xx))

    def rescale(P, x):
        if kind == "trained_like":
            return _trained_like(P, x, fwd)
        return _overflowing(P, x, fwd, 17, 18) if kind == "overflow_in_range" else _overflowing(P, x, fwd, 19, 20)

    run = (lambda: single_stage_case("sfd", h, w, dev, "split", rescale=rescale)) if which == "sfd" else \
        (lambda: dan_eval_case(False, h, w, dev, precision="split", rescale=rescale))
    if kind == "overflow_beyond":
        with pytest.raises(_ops().SplitRangeError):
            run()
    else:
        run()


def test_a_stale_range_flag_is_cleared_when_an_evaluation_starts(dev):
    """A flag raised by a direct call that nobody checked does not fail the next "split" evaluation."""
    ops = _ops()
    from dan_amd.net import sfd_net
    ops.split3(torch.full((1, 1, 4, 4), 2.0 ** 20, device=dev), S.MAP_EXP)     # raises the flag, unchecked
    with sfd_net.precision_scope("split"):
        pass
    ops.split_range_check()
