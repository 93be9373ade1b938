"""Pins tests/hbm_layers.py itself (no GPU): the float64 references against the float32 oracle, the once-rounding helper, the exactness
of the exact-case inputs, and the loop-trip conditions of the committed shape lists."""
import os
import re
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import hbm_layers as HL  # noqa: E402
from oracle import tf_ops as T  # noqa: E402

CPU = torch.device("cpu")


def _close(a64, b32, tol=1e-6):
    assert a64.dtype == torch.float64 and b32.dtype == torch.float32
    return (a64 - b32.double()).abs().max().item() <= tol * max(b32.abs().max().item(), 1.0)


def test_oracle_ops_are_dtype_agnostic_and_float64_equals_float32():
    g = torch.Generator().manual_seed(0)
    x = torch.randn((2, 7, 9, 16), generator=g)
    gamma, beta = torch.rand(16, generator=g) + 0.5, torch.randn(16, generator=g)
    assert _close(T.l2_normalize(x.double(), gamma.double()), T.l2_normalize(x, gamma))
    assert _close(T.max_pool_2x2_same(x.double()), T.max_pool_2x2_same(x), 0)
    assert _close(T.max_pool_3x3_s2_same(x.double()), T.max_pool_3x3_s2_same(x), 0)
    assert _close(T.avg_pool_2x2_s1_same(x.double()), T.avg_pool_2x2_s1_same(x))
    assert _close(T.resize_bilinear_legacy(x.double(), 13, 20), T.resize_bilinear_legacy(x, 13, 20))
    for a, b in zip(T.batch_norm_train(x.double(), gamma.double(), beta.double(), 1e-5), T.batch_norm_train(x, gamma, beta, 1e-5)):
        assert _close(a, b, 1e-5)


def test_l2_terms_are_the_autograd_gradient():
    g = torch.Generator().manual_seed(1)
    M, C = 37, 64
    x = HL.l2_input(M, C, g, torch.bfloat16).double()
    gamma = HL.gamma_input(C, g).double()
    dy = torch.randn((M, C), generator=g).double()
    t1, t2, inv, addend = HL.l2_terms(x, gamma, dy)
    dx, dg = HL.l2_grads(x, gamma, dy)
    assert (t1 - t2 - dx).abs().max().item() <= 1e-12 * dx.abs().max().item()
    assert (addend.sum(0) - dg).abs().max().item() <= 1e-12 * dg.abs().max().item()
    assert abs(inv[0].item() - 1e5) < 1e-6 and t2[0].abs().max().item() == 0 and t2[1].abs().max().item() == 0       # the clamp: no second term
    xr, gr = x.float().requires_grad_(True), gamma.float().requires_grad_(True)
    T.l2_normalize(xr.view(1, 1, M, C), gr).backward(dy.float().view(1, 1, M, C))
    assert _close(dx, xr.grad) and _close(dg, gr.grad, 1e-5)


def test_max_pool_references_follow_the_first_maximum_rule():
    x = torch.zeros((1, 5, 5, 8))                                # every window is a tie
    am = HL.maxpool2_argmax(x)
    assert int(am.max()) == 0
    dy = torch.arange(1.0, 1 + 9 * 8).view(1, 3, 3, 8)
    dx = HL.maxpool2_scatter(am, dy, 5, 5)
    assert torch.equal(dx[:, 0::2, 0::2], dy) and dx.sum().item() == dy.sum().item()
    assert HL.maxpool2_codes(torch.tensor([[[[0, 1, 2, 3, 3, 2, 1, 0]]]])).tolist() == [[0xE4, 0x1B]]
    # without ties: the scatter is autograd's gradient of the oracle pool
    g = torch.Generator().manual_seed(2)
    x = torch.randn((2, 7, 9, 8), generator=g)
    xr = x.clone().requires_grad_(True)
    y = T.max_pool_2x2_same(xr)
    dy = torch.randn(y.shape, generator=g)
    y.backward(dy)
    assert torch.equal(HL.maxpool2_scatter(HL.maxpool2_argmax(x), dy, 7, 9), xr.grad)
    # 3 x 3 / 2: autograd sends a tie to the first element in window scan order (the rule of maxpool3x3s2_bwd_kernel)
    x = torch.zeros((1, 4, 4, 1), dtype=torch.float64)
    dx = HL.maxpool3_grad(x, torch.ones((1, 2, 2, 1), dtype=torch.float64))[0, :, :, 0]
    # even size: pad (0, 1), windows start at 0, 2 -> first elements (0,0), (0,2), (2,0), (2,2)
    assert dx.tolist() == [[1, 0, 1, 0], [0, 0, 0, 0], [1, 0, 1, 0], [0, 0, 0, 0]]


@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float16])
def test_round_once_is_the_storage_rounding(dt):
    g = torch.Generator().manual_seed(3)
    v = torch.cat([torch.randn(20000, generator=g) * 3, torch.randn(2000, generator=g) * 1e-6, torch.tensor([0.0, -0.0, 1.0, 255 - 103.94])])
    assert torch.equal(HL.round_once(v.double(), dt), v.to(dt).double())          # float32 values: .to(dtype) rounds once
    p = HL.SIG_BITS[dt]
    ties = torch.tensor([1 + 2.0 ** -p, 1 + 3 * 2.0 ** -p, -(2 + 2.0 ** (1 - p))], dtype=torch.float64)
    assert HL.round_once(ties, dt).tolist() == [1.0, 1 + 4 * 2.0 ** -p, -2.0]     # to even
    # a value that two roundings (float32 first) move and one does not
    v = torch.tensor([1 + 2.0 ** -p + 2.0 ** -40], dtype=torch.float64)
    assert HL.round_once(v, dt).item() == 1 + 2.0 ** (1 - p) and v.float().to(dt).item() == 1.0


# byte values whose exact difference to the channel mean rounds differently once than twice (fp32 subtraction, then storage): there
# danhip_preprocess_u8 is allowed one storage ulp, everywhere else it must equal the once-rounded reference
PREPROCESS_DOUBLE_ROUNDED = {torch.bfloat16: [], torch.float16: []}


@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float16])
def test_preprocess_reference_is_exact_after_one_rounding(dt):
    img = torch.arange(256, dtype=torch.uint8)[:, None].expand(256, 3).contiguous()
    v, once, dbl = HL.preprocess_reference(img, dt)
    assert torch.equal(v.float().double()[:232], v[:232])        # |b - mean| < 128: the fp32 subtraction is exact
    assert sorted(set(dbl.nonzero()[:, 0].tolist())) == PREPROCESS_DOUBLE_ROUNDED[dt]


def _exact_rows(c):
    cid, fn, _, kw, _ = c
    if fn is HL.case_l2norm and kw["exact"]:
        g = HL.gen(CPU, 1)
        x = HL.l2_input(kw["M"], kw["C"], g, torch.bfloat16, True).double()
        gamma = HL.gamma_input(kw["C"], g).double()
        dy = HL.quarters((kw["M"], kw["C"]), g, torch.bfloat16).double()
        return [torch.cat([torch.full((1, kw["C"]), 8.0, dtype=torch.float64), HL.l2_terms(x, gamma, dy)[3]], 0)]
    if fn is HL.case_relu_bias and kw["exact"]:
        g = HL.gen(CPU, 1)
        return [torch.cat([torch.full((1, kw["C"]), 8.0, dtype=torch.float64), HL.quarters((kw["M"], kw["C"]), g, torch.bfloat16).double()], 0)]
    if fn is HL.case_batchnorm and kw["kind"] == "exact":
        g = HL.gen(CPU, 1)
        x = HL.bn_input(kw["M"], kw["C"], "exact", g, torch.bfloat16).double()
        return [x, x * x, HL.quarters((kw["M"], kw["C"]), g, torch.bfloat16).double()]
    return []


def test_exact_case_inputs_are_exact():
    n = 0
    for c in HL.CASES:
        for rows in _exact_rows(c):
            assert HL.exact_precondition(rows), c[0]
            n += 1
    assert n >= 9
    assert not HL.exact_precondition(torch.tensor([[0.1], [0.2]], dtype=torch.float64))
    assert not HL.exact_precondition(torch.full((2 ** 22, 1), 4.25, dtype=torch.float64))           # 17 units of 1/4 each: the sum passes 2^24


def test_float32_floor_measures_plain_float32_sums():
    g = torch.Generator().manual_seed(4)
    a = torch.randn((5000, 3), generator=g).double()
    S, A, f = HL.float32_floor(a)
    assert torch.equal(S, a.sum(0)) and 0 < f < 2.0 ** -22
    s = torch.zeros(3)
    for row in a.float():
        s = s + row
    assert ((s.double() - S).abs() / A).max().item() <= f        # the strictly sequential order is one of the three


def test_shape_lists_meet_their_loop_trip_conditions():
    ids = [c[0] for c in HL.CASES]
    assert len(set(ids)) == len(ids) and set(HL.FP16_IDS) <= set(ids)
    loops, partial, small = {}, {}, {}
    for cid, fn, trips, kw, large in HL.CASES:
        t = trips(**kw)
        if large:
            assert any(items > per for _, items, per in t), cid
        else:
            assert all(items <= per for _, items, per in t), cid
            small[fn] = True
        for name, items, per in t:
            loops[name] = loops.get(name, False) or items > per
            partial[name] = partial.get(name, False) or (items > per and items % per != 0)
    assert all(loops.values()) and all(partial.values()), (loops, partial)
    fns = {c[1] for c in HL.CASES}
    assert fns == set(small)                                     # every family has a small shape too
    assert len(loops) == 18
    # the fp16 child: one looping shape per kernel
    fl = {}
    for cid, fn, trips, kw, large in HL.CASES:
        if cid in HL.FP16_IDS:
            for name, items, per in trips(**kw):
                fl[name] = fl.get(name, False) or items > per
    assert all(fl.values()) and set(fl) == set(loops), fl
    # every l2norm instantiation at a looping M that is not a multiple of PPW, and ragged small shapes
    for C in (64, 128, 256, 512, 1024):
        ms = [kw["M"] for _, fn, _, kw, large in HL.CASES if fn is HL.case_l2norm and kw["C"] == C and large and not kw["exact"]]
        assert ms and all(m % HL.l2_ppw(C) != 0 or HL.l2_ppw(C) == 1 for m in ms), C
    assert HL.l2_ppw(64) == 8 and HL.l2_ppw(512) == 1 and HL.l2_ppw(1024) == 1 and HL.rows_per_block(72) == 28 and HL.rows_per_block(2048) == 1


def test_constants_mirror_the_sources():
    """The launch caps are read back from the kernel sources, so a changed cap fails here and not silently in the shape conditions."""
    root = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "dan_amd", "csrc")
    ew = open(os.path.join(root, "elementwise.hip")).read()
    l2 = open(os.path.join(root, "layers2.hip")).read()
    for src in (ew, l2):                                         # dh_grid_for (common.h) has no default cap: every launch states its own
        caps = re.findall(r"dh_grid_for\(.*?, 256, (\d+)\)\), dim3\(256\)", src)
        assert caps and len(caps) == src.count("grid_for(") and set(caps) == {str(HL.GRID_FOR_CAP)}, caps
    assert l2.count("if (blocks > %d) blocks = %d;" % (HL.POOL3_CAP, HL.POOL3_CAP)) == 2
    assert l2.count("if (grid > %d) grid = %d;" % (HL.BN_REDUCE_BLOCKS, HL.BN_REDUCE_BLOCKS)) == 2
    for cap in (HL.L2_FWD_BLOCKS, HL.L2_BWD_BLOCKS, HL.RELU_BIAS_BLOCKS, HL.RELU_BITS_BLOCKS, HL.SLICE_BLOCKS):
        assert "if (blocks > %d) blocks = %d;" % (cap, cap) in ew, cap
    assert "long blocks = (M + 4 * ppw - 1) / (4 * ppw);" in ew and "long blocks = (M + 16 * ppw - 1) / (16 * ppw);" in ew
    assert "long blocks = (nwin + 8 * ppw - 1) / (8 * ppw);" in ew and "if (blocks > %d) {" % HL.JUNCTION_BLOCKS in ew


def test_check16_handles_the_range_of_the_storage_type():
    dt = torch.float16
    ref = torch.tensor([1505280.2, -1505280.2, 100.0], dtype=torch.float64)
    mag = ref.abs()
    inf = float("inf")
    HL.check16(torch.tensor([inf, -inf, 100.0], dtype=dt), ref, mag, dt, "overflow rounds to infinity")
    for wrong in ([65504.0, -inf, 100.0], [inf, inf, 100.0], [inf, -inf, inf], [inf, -inf, float("nan")], [inf, -inf, 100.25]):
        with pytest.raises(AssertionError):
            HL.check16(torch.tensor(wrong, dtype=dt), ref, mag, dt, "must fail")
    edge = torch.tensor([65519.0], dtype=torch.float64)             # within the bound of the rounding boundary 65520: either side
    HL.check16(torch.tensor([inf], dtype=dt), edge, edge, dt, "edge")
    HL.check16(torch.tensor([65504.0], dtype=dt), edge, edge, dt, "edge")
