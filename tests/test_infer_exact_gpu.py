"""The two forward-only inference paths against float64 references, as equalities wherever the arithmetic allows one (tests/infer_exact.py says
why): the split-operand convolution limb for limb in every epilogue that writes limbs or applies the accumulator exponent (halo forms, flat-M
store, split-K finish), with the launched kernel instance asserted after each call; the first layer's fp32 chain; the max-pool and l2norm on the
limb layout; the fp32 convolution and layer kernels at their edges and past their grid-stride loop caps."""
import ctypes
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import conv_exact as CE  # noqa: E402
import infer_exact as IE  # noqa: E402

pytestmark = pytest.mark.gpu

F64 = torch.float64
_LAUNCHED = {}          # case id -> {(label, splits)}: filled by the case tests, read (and completed) by the coverage test


def _launched(case, dev):
    if case[0] not in _LAUNCHED:
        _LAUNCHED[case[0]] = IE.run_split_case(IE.Api(dev), case)
    return _LAUNCHED[case[0]]


# ================================================================================================================ A: split-operand convolution
@pytest.mark.parametrize("case", IE.SPLIT_CASES, ids=[c[0] for c in IE.SPLIT_CASES])
def test_split_convolution_equals_float64_limb_for_limb(case, dev):
    _LAUNCHED.pop(case[0], None)
    print(case[0], sorted(_launched(case, dev)))


@pytest.mark.parametrize("cls", IE.CHAIN_CLASSES)
def test_chained_split_convolutions_stay_exact_through_limb_views_and_a_pool(cls, dev):
    IE.run_chain(IE.Api(dev), cls)


def test_split_tables_cover_every_limb_writing_epilogue(dev):
    seen = set()
    for case in IE.SPLIT_CASES:
        seen |= _launched(case, dev)
    labels = {l for l, _ in seen}
    has = lambda pre, suf="": any(l.startswith(pre) and l.endswith(suf) for l in labels)
    assert has(CE.HALO + "8, 32, 128,"), "no halo 128-wide instance"
    assert has(CE.HALO + "8, 32, 64, 8, 1, 1, 4,") or has(CE.HALO + "16, 16, 64, 8, 1, 1, 4,"), "no halo 64-wide instance"
    assert has(CE.HALO + "8, 32,") and has(CE.HALO + "16, 16,"), "a halo tile shape is missing"
    assert has(CE.HALO, "false, 1, false>"), "no halo thin head"
    assert has(CE.FLAT, "true>") and has(CE.FLAT, "false>"), "flat-M FAST / non-FAST missing"
    assert sum(1 for _, splits in seen if splits >= 2) >= 2, "fewer than two split-K launches"


# ================================================================================================================ B: the first layer
@pytest.mark.parametrize("nhw", IE.FIRST_SHAPES)
def test_first_layer_limbs_equal_the_float64_reference(nhw, dev):
    from dan_amd import _lib
    N, H, W = nhw
    inp = IE.first_inputs(nhw)
    IE.check_first_inputs(inp)
    api = IE.Api(dev)
    x, w, b = api.f32(inp["x"]), api.f32(inp["w"]), api.f32(inp["b"])
    for bias in (True, False):
        for relu in (True, False):
            y3 = torch.full((N, H, W, 192), float("nan"), dtype=torch.float16, device=dev)
            _lib.call("danhip_conv3x3_c3_f32_split3", _lib.ptr(x), _lib.ptr(w), _lib.ptr(b) if bias else None, _lib.ptr(y3), N, H, W, 64, int(relu), -IE.LIMB_EXP,
                      _lib.stream())
            IE.assert_same_halves(y3, IE.first_expected(inp, bias, relu), "first layer %s bias=%d relu=%d" % (nhw, bias, relu))
    api.range_ok()


def test_ops_conv2d_takes_the_first_layer_fast_path(dev):
    from dan_amd import ops
    api = IE.Api(dev)
    inp = IE.first_inputs((2, 3, 5))
    before = api.last_label()
    with ops.use_context(ops.OpsContext(SPLIT_EVAL=True)), torch.no_grad():
        y = ops.conv2d(api.f32(inp["x"]), api.f32(inp["w"]), api.f32(inp["b"]), relu=True)
    assert ops._is_limbs(y) and y._dh_exp == 2 and tuple(y.shape) == (2, 3, 5, 64)
    assert api.last_label() == before, "a danhip_conv2d_fwd_split kernel ran for the first layer"
    IE.assert_same_halves(y._dh_split3, IE.first_expected(inp, True, True), "first layer through ops.conv2d")


# ================================================================================================================ C: max-pool on the limb layout
@pytest.mark.parametrize("shape", IE.POOL_SHAPES)
def test_maxpool_on_limbs_equals_the_resplit_fp32_maximum(shape, dev):
    from dan_amd import _lib
    N, H, W, C = shape
    inp = IE.pool_inputs(shape)
    IE.check_pool_inputs(inp)
    want, loose, _ = IE.pool_expected(inp)
    x3 = inp["x3"].to(dev)
    y3 = torch.full((N, (H + 1) // 2, (W + 1) // 2, 3 * C), float("nan"), dtype=torch.float16, device=dev)
    _lib.call("danhip_maxpool2x2_split3", _lib.ptr(x3), _lib.ptr(y3), N, H, W, C, _lib.stream())
    assert torch.equal(y3[..., :C].view(torch.int16), y3[..., 2 * C:].view(torch.int16)), "sections 0 and 2 differ"
    IE.assert_same_halves(y3, want, "maxpool2x2_split3 %s" % (shape,), loose=torch.cat([loose, loose, loose], -1))


def test_maxpool_of_a_four_channel_limb_view_takes_the_fp32_fallback(dev):
    from dan_amd import ops
    g = CE.gen(5)
    x = CE.small((2, 7, 5, 4), g, -2 ** 19, 2 ** 19) / 64          # 20 significant bits: the limbs of x / 4 carry x exactly
    hi, lo = IE.limbs(x * 2.0 ** -IE.LIMB_EXP)
    assert torch.equal((hi + lo) * 2.0 ** IE.LIMB_EXP, x) and int((lo != 0).sum()) > x.numel() // 2
    xd = x.float().to(dev)
    xv = ops._limb_view(ops.split3(xd, IE.LIMB_EXP), 4, IE.LIMB_EXP)
    assert xv._dh_split3.shape[-1] == 16
    y = ops.max_pool_2x2(xv)
    assert y.dtype == torch.float32 and not ops._is_limbs(y)
    CE.assert_equal(y, CE.pool_ref(x)[0], "max_pool_2x2 of a C = 4 limb view")


# ================================================================================================================ D: l2norm
def _l2_case(dev, M, C, in_exp, limbs_in):
    from dan_amd import _lib
    inp = IE.l2_inputs(M, C, in_exp)
    IE.check_l2_inputs(inp)
    gamma = inp["gamma"].float().to(dev)
    if limbs_in:
        v = inp["carried"]
        x3 = torch.cat([inp["hi"], inp["lo"], inp["hi"]], -1).to(torch.float16).to(dev)
        y3 = torch.full((M, 3 * C), float("nan"), dtype=torch.float16, device=dev)
        _lib.call("danhip_l2norm_split3", _lib.ptr(x3), _lib.ptr(gamma), _lib.ptr(y3), M, C, in_exp, 0, _lib.stream())
        y3 = y3.cpu()
        assert torch.equal(y3[:, :C].view(torch.int16), y3[:, 2 * C:].view(torch.int16))
        got = y3[:, :C].double() + y3[:, C:2 * C].double()
    else:
        v = inp["x"]
        y = torch.full((M, C), float("nan"), dtype=torch.float32, device=dev)
        _lib.call("danhip_l2norm_fwd_f32", _lib.ptr(v.float().to(dev)), _lib.ptr(gamma), _lib.ptr(y), M, C, _lib.stream())
        got = y.cpu().double()
    ref = IE.l2_ref(v, inp["gamma"])
    rel, floor = IE.l2_bound(C, limbs_in)
    ratio = ((got - ref).abs() / (rel * ref.abs() + floor + 1e-300)).max().item()
    print("l2norm %s M=%d C=%d in_exp=%d: worst error / bound = %.3f" % ("limbs" if limbs_in else "fp32", M, C, in_exp, ratio))
    assert torch.isfinite(got).all() and ratio <= 1.0, ratio
    return ratio


@pytest.mark.parametrize("in_exp", [0, 2])
@pytest.mark.parametrize("C", IE.L2_CS)
def test_l2norm_on_limbs_within_the_composed_bound(C, in_exp, dev):
    """Per element |got - ref| <= rel |ref| + 2^-25 with rel = min(((ceil(C / 64) + 6) / 2 + 8) 2^-24, 2^-20) (infer_exact.l2_bound derives
    it), against float64 on the carried values.  Worst measured error / bound on an MI355X: 0.68 (C = 8) to 0.99 (C = 512); the worst elements
    are those whose lo limb is subnormal, where half's rounding step alone reaches the 2^-25 floor."""
    _l2_case(dev, 5, C, in_exp, True)


@pytest.mark.parametrize("C", IE.L2_CS)
def test_l2norm_fp32_within_the_composed_bound(C, dev):
    """Per element |got - ref| <= ((ceil(C / 64) + 6) / 2 + 4) 2^-24 |ref|.  Worst measured error / bound on an MI355X: 0.38 (C = 72)."""
    _l2_case(dev, 5, C, 0, False)


def test_l2norm_kernels_past_their_grid_loop_caps(dev):
    """The limb kernel launches at most 65536 blocks of four waves, the fp32 kernel 16384: a second trip from 262145 / 65537 rows.  Worst
    measured error / bound on an MI355X: 0.998 (limbs, 2.1 million elements: the subnormal-lo floor again) and 0.50 (fp32)."""
    _l2_case(dev, 65536 * 4 + 37, 8, 2, True)
    _l2_case(dev, 16384 * 4 + 37, 64, 0, False)


# ================================================================================================================ E: the fp32 path
@pytest.mark.parametrize("case", IE.F32_CONV_CASES, ids=[c[0] for c in IE.F32_CONV_CASES])
def test_fp32_convolution_equals_float64_on_integers(case, dev):
    from dan_amd import _lib, ops
    cid, shp, padding = case
    N, H, W, Cin, Cout, kh, kw, s = shp
    inp = IE.f32_conv_inputs(shp, padding)
    IE.check_f32_conv_inputs(inp)
    d = ops._desc(N, H, W, Cin, Cout, kh, kw, s, padding == "valid")
    assert (d.Ho, d.Wo) == IE.out_hw(H, W, kh, kw, s, padding)
    f = lambda t: t.float().to(dev).contiguous()
    x, w, b, res = f(inp["x"]), f(inp["w"]), f(inp["b"]), f(inp["res"])
    for bias, relu, residual in IE.F32_CONV_VARIANTS:
        y = torch.full((N, d.Ho, d.Wo, Cout), float("nan"), dtype=torch.float32, device=dev)
        _lib.call("danhip_conv2d_fwd_f32", ctypes.byref(d), _lib.ptr(x), _lib.ptr(w), _lib.ptr(b) if bias else None, _lib.ptr(y), int(relu),
                  _lib.ptr(res) if residual else None, _lib.stream())
        CE.assert_equal(y, IE.f32_conv_expected(inp, bias, relu, residual), "%s bias=%d relu=%d residual=%d" % (cid, bias, relu, residual))


def _layer_call(name, dev, x, out_shape, *dims):
    from dan_amd import _lib
    y = torch.full(out_shape, float("nan"), dtype=torch.float32, device=dev)
    _lib.call(name, _lib.ptr(x.to(dev).contiguous()), _lib.ptr(y), *dims, _lib.stream())
    return y.cpu()


@pytest.mark.parametrize("shape", IE.LAYER_SHAPES + [IE.MAXPOOL_LOOP])
def test_fp32_maxpool_equals_the_first_max_reference(shape, dev):
    N, H, W, C = shape
    x = IE.maxpool_inputs(shape)
    want = CE.pool_ref(x)[0]
    assert (want[..., 0] < 0).all()
    got = _layer_call("danhip_maxpool2x2_fwd_f32", dev, x, tuple(want.shape), N, H, W, C)
    assert torch.equal(got, want), int((got != want).sum())


@pytest.mark.parametrize("shape", IE.LAYER_SHAPES + [IE.AVGPOOL_LOOP])
def test_fp32_avgpool_equals_the_valid_tap_average(shape, dev):
    N, H, W, C = shape
    x = IE.avgpool_inputs(shape)
    want = IE.avgpool_ref(x)          # quarters: exact in fp32 (pinned for the small shapes in the CPU file)
    got = _layer_call("danhip_avgpool2x2s1_same_fwd_f32", dev, x, shape, N, H, W, C)
    assert torch.equal(got, want), int((got != want).sum())


def _resize(dev, up, lat, Ho, Wo):
    from dan_amd import _lib
    N, Hi, Wi, C = up.shape
    out = torch.full((N, Ho, Wo, C), float("nan"), dtype=torch.float32, device=dev)
    upd, latd = up.to(dev).contiguous(), None if lat is None else lat.to(dev).contiguous()
    _lib.call("danhip_resize_bilinear_add_fwd_f32", _lib.ptr(upd), _lib.ptr(latd), _lib.ptr(out), N, Hi, Wi, Ho, Wo, C, _lib.stream())
    return out.cpu()


@pytest.mark.parametrize("ratio", [2, 4])
@pytest.mark.parametrize("shape", IE.LAYER_SHAPES)
def test_fp32_resize_add_is_exact_on_dyadic_inputs(shape, ratio, dev):
    N, H, W, C = shape
    up = IE.resize_inputs(shape)
    Ho, Wo = H * ratio, W * ratio
    lat = IE.resize_inputs((N, Ho, Wo, C), seed=83)
    for l in (None, lat):
        want, _ = IE.resize_ref(up, Ho, Wo, l)
        assert IE.is_f32(want)
        got = _resize(dev, up, l, Ho, Wo)
        assert torch.equal(got.double(), want), (l is not None, int((got.double() != want).sum()))


def test_fp32_resize_add_past_its_grid_loop_cap(dev):
    shape, ratio = IE.RESIZE_LOOP
    N, H, W, C = shape
    up = IE.resize_inputs(shape)
    lat = IE.resize_inputs((N, H * ratio, W * ratio, C), seed=83)
    want, _ = IE.resize_ref(up.float(), H * ratio, W * ratio, lat)
    got = _resize(dev, up, lat, H * ratio, W * ratio)
    assert torch.equal(got, want.float()) and IE.is_f32(want[:, :4])


@pytest.mark.parametrize("sizes", [((10, 10), (19, 19)), ((5, 7), (9, 13))])
def test_fp32_resize_at_a_ratio_that_is_no_integer(sizes, dev):
    """Against the float64 blend at the kernel's own fp32 source coordinates (f = (float)i * ((float)in / (float)out) restated in fp32).  Bound:
    4 fp32 roundings per element - top, bottom and the final blend are one fused multiply-add each after one rounded difference, and the two
    row blends enter the result with weights (1 - ly) and ly - of quantities no larger than 2 max|corner| (a difference of two corners):
    4 * 2^-24 * 2 max|corner|.  Worst measured error / bound on an MI355X: 0.26 and 0.22."""
    (Hi, Wi), (Ho, Wo) = sizes
    g = CE.gen(Hi + Wo)
    up = torch.randn((2, Hi, Wi, 5), generator=g)
    want, scale = IE.resize_ref(up, Ho, Wo)
    got = _resize(dev, up, None, Ho, Wo).double()
    ratio = ((got - want).abs() / (4 * 2.0 ** -24 * 2 * scale)).max().item()
    print("resize %s -> %s: worst error / bound = %.3f" % (sizes[0], sizes[1], ratio))
    assert ratio <= 1.0, ratio
