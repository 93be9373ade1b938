"""Pins tests/conv_exact.py itself (no GPU): the float64 reference against the float32 oracle convolution and its autograd gradients, the
pool / arg-code / bit-mask restatements against the oracle pool and hand-written windows, the conditions every listed case must meet on its
reference (16-bit exact range, exact zeros, late ties, the cut a case is there for) and the launch-plan restatements against descriptors
worked out by hand from the .hip sources and against the library's own workspace queries."""
import ctypes
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import conv_exact as CE  # noqa: E402
from oracle import tf_ops as T  # noqa: E402

F64 = torch.float64


@pytest.mark.parametrize("shape", [(2, 9, 7, 5, 6, 3, 3, 1), (1, 10, 8, 4, 3, 3, 3, 2), (1, 11, 7, 4, 3, 3, 3, 2), (2, 6, 9, 8, 5, 3, 1, 1), (1, 7, 12, 8, 5, 1, 3, 1),
                                   (3, 5, 5, 16, 7, 1, 1, 1), (1, 5, 1, 3, 4, 3, 3, 1), (1, 9, 9, 8, 8, 3, 3, 3)])
def test_reference_is_the_oracle_convolution_and_its_gradients(shape):
    N, H, W, Cin, Cout, kh, kw, s = shape
    g = torch.Generator().manual_seed(sum(shape))
    x, w, b = torch.randn((N, H, W, Cin), generator=g), torch.randn((kh, kw, Cin, Cout), generator=g), torch.randn((Cout,), generator=g)
    xr, wr, br = x.clone().requires_grad_(True), w.clone().requires_grad_(True), b.clone().requires_grad_(True)
    want = T.conv2d_same(xr, wr, br, stride=s)
    got = CE.conv_ref(x.double(), w.double(), b.double(), s)
    assert got.dtype == F64 and got.shape == want.shape
    assert (got - want.detach().double()).abs().max().item() <= 1e-5 * max(1.0, want.abs().max().item())          # test_oracle_cpu.py's tolerance
    dy = torch.randn(want.shape, generator=g)
    want.backward(dy)
    dx = CE.dgrad_ref(dy.double(), w.double(), H, W, s)
    dw, db = CE.wgrad_ref(x.double(), dy.double(), kh, kw, s)
    for a, r in ((dx, xr.grad), (dw, wr.grad), (db, br.grad)):
        assert a.shape == r.shape and (a - r.double()).abs().max().item() <= 1e-5 * max(1.0, r.abs().max().item())


def test_stride_two_puts_the_odd_pad_pixel_at_the_bottom_right():
    assert CE.same_pad(10, 3, 2) == (0, 1, 5) and CE.same_pad(11, 3, 2) == (1, 1, 6) and CE.same_pad(7, 3, 1) == (1, 1, 7) and CE.same_pad(7, 1, 1) == (0, 0, 7)
    # 4 x 4 map, 3 x 3 window, stride 2: pad (0, 1) -> windows cover rows 0..2 and 2..4, their centres are the pixels (1,1), (1,3), (3,1), (3,3);
    # with the pad on the top / left the centres would be (0,0), (0,2), (2,0), (2,2)
    x = torch.zeros((1, 4, 4, 1), dtype=F64)
    x[0, 3, 3, 0] = 1.0
    w = torch.zeros((3, 3, 1, 1), dtype=F64)
    w[1, 1] = 1.0
    y = CE.conv_ref(x, w, None, 2)
    assert y.shape == (1, 2, 2, 1) and y[0, :, :, 0].tolist() == [[0, 0], [0, 1]]
    x[0, 3, 3, 0], x[0, 2, 2, 0] = 0.0, 1.0
    assert CE.conv_ref(x, w, None, 2).abs().sum().item() == 0


@pytest.mark.parametrize("shape", [(2, 29, 35, 3, 8, 7, 7, 2), (1, 9, 11, 6, 5, 3, 3, 1), (1, 10, 12, 4, 3, 3, 3, 2), (2, 8, 7, 4, 3, 5, 2, 3)])
def test_valid_reference_is_the_oracle_convolution_and_its_gradients(shape):
    """padding='valid': floor((in - k) / s) + 1 windows, no padding; (10, 12) at stride 2 and (8, 7) at stride 3 leave rows / columns behind the
    last window that no output reads (their data gradient is 0)."""
    N, H, W, Cin, Cout, kh, kw, s = shape
    g = torch.Generator().manual_seed(sum(shape))
    x, w, b = torch.randn((N, H, W, Cin), generator=g), torch.randn((kh, kw, Cin, Cout), generator=g), torch.randn((Cout,), generator=g)
    xr, wr, br = x.clone().requires_grad_(True), w.clone().requires_grad_(True), b.clone().requires_grad_(True)
    want = T.conv2d_valid(xr, wr, br, stride=s)
    got = CE.conv_ref(x.double(), w.double(), b.double(), s, valid=True)
    assert tuple(got.shape) == (N, CE.out_size(H, kh, s, True), CE.out_size(W, kw, s, True), Cout) == tuple(want.shape)
    assert (got - want.detach().double()).abs().max().item() <= 1e-5 * max(1.0, want.abs().max().item())
    dy = torch.randn(want.shape, generator=g)
    want.backward(dy)
    dx = CE.dgrad_ref(dy.double(), w.double(), H, W, s, valid=True)
    dw, db = CE.wgrad_ref(x.double(), dy.double(), kh, kw, s, valid=True)
    for a, r in ((dx, xr.grad), (dw, wr.grad), (db, br.grad)):
        assert a.shape == r.shape and (a - r.double()).abs().max().item() <= 1e-5 * max(1.0, r.abs().max().item())
    # by hand: output (i, j) reads the window whose top-left pixel is (i s, j s)
    i, j = got.shape[1] - 1, got.shape[2] - 1
    win = x[0, i * s:i * s + kh, j * s:j * s + kw].double()
    assert abs((win.unsqueeze(-1) * w.double()).sum((0, 1, 2))[0].item() + b[0].item() - got[0, i, j, 0].item()) <= 1e-9
    if (H - kh) % s:
        assert dx[:, (got.shape[1] - 1) * s + kh:].abs().sum().item() == 0


def test_view_selection_and_plus_kernel_restate_the_sources_by_hand():
    # conv_halo_c64.hip c64_eligible: 3x3 64 -> 64 with 30 x 62 of 32 x 64 tile pixels = 0.91 >= 0.78, and no partial ReLU; 37 x 40 of 40 x 64 = 0.58:
    # declined -> 4440 pixels >= 2048: the streaming GEMM's tap form, 64 wide
    S = CE.S
    assert CE.view_kernel(S(1, 30, 62, 64, 64), 0, 256, scratch=True) == "conv3x3_c64_kernel<false>"
    assert CE.view_kernel(S(1, 30, 62, 64, 64), 1, 256, scratch=True) == "conv3x3_c64_kernel<true>"
    assert CE.view_kernel(S(3, 37, 40, 64, 64), 0, 256) == "conv_pointwise_kernel<64, 4, false, true, true>"
    # ... with a partial ReLU the 1860 pixels are below the streaming GEMM's floor: flat-M, and with scratch its 8 tiles split K in 2
    assert CE.view_kernel(S(1, 30, 62, 64, 64), 0, 256, scratch=True, partial=True) == "conv_igemm_kernel<256, 64, 1, true>"
    assert CE.plan_splitk(S(1, 30, 62, 64, 64), 0, 256)[0] == 2 and CE.plan_splitk(S(2, 6, 6, 64, 64), 0, 256) == (2, 5, 72, 64)
    # 16 images of 3 x 3, 1024 -> 192: 144 pixels, 64-wide tiles: 1 x 3 tiles, 16 K tiles -> min(171, 16 / 4, 36) = 4 splits of 4
    assert CE.plan_splitk(S(16, 3, 3, 1024, 192, 1), 0, 256) == (4, 4, 144, 192)
    # its data gradient has K = 192: 3 K tiles < 8, no split; the residual conv's (K = 1024, 256 columns: 2 x 2 tiles of 128) splits in 4
    assert CE.plan_splitk(S(16, 3, 3, 1024, 192, 1), 1, 256)[0] == 1 and CE.plan_splitk(S(16, 3, 3, 256, 1024, 1), 1, 256) == (4, 4, 144, 256)
    # streaming GEMM: 256-wide tiles where Co % 256 == 0, except a data gradient with epilogue inputs (option pw_dgrad_ld_bn = 128)
    assert CE.view_kernel(S(1, 40, 56, 256, 192, 1), 1, 256, ld=True) == "conv_pointwise_kernel<128, 4, true, true, false>"
    assert CE.view_kernel(S(1, 40, 56, 256, 192, 1), 1, 256, ld=False) == "conv_pointwise_kernel<256, 3, true, false, false>"
    assert CE.view_kernel(S(1, 40, 56, 192, 256, 1), 0, 256) == "conv_pointwise_kernel<256, 3, false, true, false>"
    m = CE.plus_mask()
    assert m[:, :, 5, 7].tolist() == [[0, 1, 0], [0, 1, 0], [0, 1, 0]] and m[:, :, 5, 40].tolist() == [[0, 0, 0], [1, 1, 1], [0, 0, 0]]
    for dt in (torch.bfloat16, torch.float16):                     # the background pattern is a NaN in both 16-bit types
        assert bool(torch.tensor([CE.NAN16], dtype=torch.int16).view(dt).isnan().all())


def test_pool_codes_and_bit_masks_follow_their_rules():
    g = torch.Generator().manual_seed(2)
    x = torch.randn((2, 7, 9, 8), generator=g).double()
    p, code = CE.pool_ref(x)
    assert torch.equal(p, T.max_pool_2x2_same(x))
    xr = x.clone().requires_grad_(True)                           # without ties: the scatter is autograd's gradient of the oracle pool
    y = T.max_pool_2x2_same(xr)
    dy = torch.randn(y.shape, generator=g).double()
    y.backward(dy)
    assert torch.equal(CE.pool_scatter(code, dy, 7, 9), xr.grad)
    # hand-written windows, one channel each: [a b / c d] -> code of the first maximum in row-major order
    wins = [([0, 0, 0, 0], 0), ([1, 3, 3, 2], 1), ([0, 2, 1, 2], 1), ([0, 1, 5, 5], 2), ([0, 0, 0, 4], 3), ([2, 2, 1, 0], 0), ([0, 1, 1, 1], 1), ([0, 0, 7, 0], 2)]
    y = torch.tensor([[[w[0], w[1]] for w, _ in wins], [[w[2], w[3]] for w, _ in wins]], dtype=F64).permute(0, 2, 1).reshape(1, 2, 2, 8)
    p, code = CE.pool_ref(y)
    assert code[0, 0, 0].tolist() == [c for _, c in wins] and p[0, 0, 0].tolist() == [max(w) for w, _ in wins]
    assert CE.pack_codes(code).tolist() == [[0 | 1 << 2 | 1 << 4 | 2 << 6, 3 | 0 << 2 | 1 << 4 | 2 << 6]]
    assert CE.late_ties(y) == 4                                    # windows 1, 2, 3 and 6: a repeated maximum that does not start at code 0
    # odd sizes: the last window has one column / one row, and elements outside the map never win
    y = torch.tensor([[-1.0, -2.0, -3.0], [-4.0, -0.5, -6.0], [-7.0, -8.0, -9.0]], dtype=F64).reshape(1, 3, 3, 1)
    p, code = CE.pool_ref(y)
    assert p[0, :, :, 0].tolist() == [[-0.5, -3.0], [-7.0, -9.0]] and code[0, :, :, 0].tolist() == [[3, 0], [0, 0]]
    # bit mask: bit r of byte k = channel 8 k + r, set where y > 0 (not >= 0, and -0.0 is not positive)
    v = torch.tensor([[1, 0, -1, 2, -0.0, 0.5, 0, 3, 0, 0, 0, 0, 0, 0, 0, 9]], dtype=F64)
    assert CE.relu_bits(v).tolist() == [[0b10101001, 0b10000000]]


def test_generators_are_integer_valued_and_dense_where_stated():
    g = CE.gen(0)
    w = CE.signs((3, 3, 16, 8), g)
    assert set(w.unique().tolist()) == {-1.0, 1.0}
    t = CE.ternary((4000,), 0.25, g)
    assert set(t.unique().tolist()) == {-1.0, 0.0, 1.0} and 0.2 < (t != 0).double().mean().item() < 0.3
    s = CE.small((4000,), g)
    assert s.min().item() == -8 and s.max().item() == 8 and torch.equal(s, s.round())
    assert CE.density(9 * 512) == 1024 / 4608 and CE.density(27) == 1.0
    inp = CE.forward_inputs((2, 17, 45, 8, 64, 3, 3, 1))
    assert inp["cin_real"] == 3 and inp["x"][..., 3:].abs().sum().item() == 0 and tuple(inp["w"].shape) == (3, 3, 3, 64)
    inp = CE.dgrad_inputs((1, 12, 12, 64, 30, 3, 3, 1))
    assert inp["dy"].shape[-1] == 32 and inp["dy"][..., 30:].abs().sum().item() == 0
    for dt in (torch.bfloat16, torch.float16):                     # every integer up to the limit is a value of both 16-bit types
        v = torch.arange(-CE.LIMIT16, CE.LIMIT16 + 1, dtype=F64)
        assert torch.equal(v.to(dt).double(), v)


CASES = CE.all_cases()


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_case_meets_its_conditions_on_the_reference(case):
    """|value| <= 256 wherever the output is stored in 16 bits, an exact zero before every ReLU, a late tie in every pool case, the cut a
    weight-gradient / split-K case is there for (256 CUs: the MI355X, and what the library assumes without a device)."""
    figs = CE.check_case_inputs(case, cus=256)
    print(case[0], figs)


def test_resnet_rows_are_listed_under_the_families_the_label_functions_name():
    """The ResNet table's families are the host label functions' answers (256 CUs without a device), with and without scratch and for the
    plain and the masked data gradient; at least one forward row is the streaming GEMM's tap form with a 1x1 window, at least one data
    gradient the flat-M kernel at stride 2 (its fractionally strided gather: the streaming GEMM declines dstride != 1); 'valid' and 'same'
    of a 1x1 window are one descriptor and one reference; the unreached-pixel condition fails on a reference with a term there."""
    from dan_amd import build as B
    from dan_amd._lib import ConvDesc, bind
    B.build()
    L = bind(ctypes.CDLL(B.OUT))
    taps_1x1 = strided_gather = 0
    for n, shp, valid, ff, fe, df, de, wf in CE.RESNET_CASES:
        N, H, W, Cin, Cout, kh, kw, s = shp
        d = ConvDesc()
        d.N, d.H, d.W, d.Cin, d.Cout, d.kh, d.kw, d.stride = N, H, W, Cin, Cout, kh, kw, s
        d.Ho, d.Wo = CE.out_size(H, kh, s, valid), CE.out_size(W, kw, s, valid)
        p = ctypes.byref(d)
        assert (d.Ho, d.Wo) == (CE.out_size(H, kh, s, not valid), CE.out_size(W, kw, s, not valid)) or kh > 1
        for scratch in (0, 16):
            assert L.danhip_conv_kernel_label(p, 0 | scratch).decode() == ff, (n, scratch)
            for which in (1, 5):
                assert L.danhip_conv_kernel_label(p, which | scratch).decode() == df, (n, which, scratch)
        assert L.danhip_conv_wgrad_kernel_label(p).decode() == wf, n
        assert (fe == "splitk") == (CE.plan_splitk(shp, 0, 256, valid)[0] >= 2) and (de == "splitk") == (CE.plan_splitk(shp, 1, 256, valid)[0] >= 2), n
        taps_1x1 += ff.startswith(CE.PW) and ff.endswith("true>") and kh == kw == 1
        strided_gather += df.startswith(CE.FLAT) and s == 2
    assert taps_1x1 >= 1 and strided_gather >= 1
    shp = CE.S(2, 15, 17, 256, 512, 1, 2)
    for make, keys in ((CE.forward_inputs, ("pre",)), (CE.dgrad_inputs, ("dx",)), (CE.wgrad_inputs, ("dw", "db"))):
        a, b = make(shp, valid=True), make(shp, valid=False)
        assert all(torch.equal(a[k], b[k]) for k in keys)
    inp = dict(CE.dgrad_inputs(shp, valid=True))
    assert CE.check_dgrad_unreached(inp, shp) == 2 * (15 * 17 - 8 * 9)
    inp["dx"] = inp["dx"].clone()
    inp["dx"][0, 1, 0, 0] = 1.0
    with pytest.raises(AssertionError):
        CE.check_dgrad_unreached(inp, shp)
    inp = dict(CE.dgrad_inputs(shp, valid=True))
    inp["old"] = torch.zeros_like(inp["old"])
    with pytest.raises(AssertionError):
        CE.check_dgrad_unreached(inp, shp)


def test_average_pool_reference_is_the_oracle_pool():
    g = torch.Generator().manual_seed(4)
    x = torch.randn((2, 5, 7, 3), generator=g).double()
    assert (CE.avg_pool_ref(x) - T.avg_pool_2x2_s1_same(x)).abs().max().item() <= 1e-12
    for k in ((1, 1), (3, 3), (3, 1), (1, 3)):                     # the block's per-tap matrix products are the reference convolution
        w, b = torch.randn(k + (3, 4), generator=g).double(), torch.randn((4,), generator=g).double()
        assert (CE.conv_taps(x, w, b) - CE.conv_ref(x, w, b)).abs().max().item() <= 1e-12
    one = torch.ones((1, 3, 3, 1), dtype=F64)                     # the divisor counts the pixels inside the map: a constant map stays constant
    assert torch.equal(CE.avg_pool_ref(one), one)
    v = torch.arange(9, dtype=F64).reshape(1, 3, 3, 1)
    assert CE.avg_pool_ref(v)[0, :, :, 0].tolist() == [[2.0, 3.0, 3.5], [5.0, 6.0, 6.5], [6.5, 7.5, 8.0]]


@pytest.mark.parametrize("case", CE.BLOCK_CASES, ids=[c[0] for c in CE.BLOCK_CASES])
def test_block_case_meets_its_conditions_on_the_reference(case):
    """tests/test_conv_views_exact_gpu.py compares ops.context_block with this reference by equality.  That needs: the two orders of branch 2
    (pool-then-conv, conv-then-pool) equal in float64; every tensor either route stores in 16 bits - activations, the accumulated dT, dU and x's
    gradient buffer after each delivery - a multiple of 1/4 that survives bf16 and IEEE half; every fp32 sum below 2^24 quarters; and, so that
    the case cannot go trivial, every branch output non-zero, every ReLU with zeros and positives, every variable gradient non-zero."""
    figs = CE.check_block_case(case)
    print(case[0], figs)


def test_block_reference_is_the_oracle_block():
    """The float64 block against the oracle network's context block (fp32, its own convolutions and pool) on random weights: output, input
    gradient and every variable's gradient."""
    from oracle import nets as ON
    g = torch.Generator().manual_seed(9)
    C = 64
    P32 = {}
    for name, kh, kw, cin, cout in CE.BLOCK_LAYERS:
        cin, cout = cin or C, cout or C
        P32["blk/" + name + "/kernel"] = (torch.randn((kh, kw, cin, cout), generator=g) / (kh * kw * cin) ** 0.5).requires_grad_(True)
        P32["blk/" + name + "/bias"] = (0.1 * torch.randn((cout,), generator=g)).requires_grad_(True)
    x32 = torch.randn((2, 5, 7, C), generator=g).requires_grad_(True)
    dy = torch.randn((2, 5, 7, C), generator=g)
    ON.se_inception_block_v1(ON.Params(P32), x32, "blk").backward(dy)
    for commuted in (False, True):
        x = x32.detach().double().requires_grad_(True)
        P = {n[4:]: v.detach().double().requires_grad_(True) for n, v in P32.items()}
        out, _ = CE.block_ref(x, P, commuted)
        out.backward(dy.double())
        for got, want in [(x.grad, x32.grad)] + [(P[n[4:]].grad, v.grad) for n, v in P32.items()]:
            assert got.shape == want.shape and (got - want.double()).abs().max().item() <= 1e-4 * max(1.0, want.abs().max().item())


def test_tables_cover_every_dispatch_row_and_family():
    import test_conv_dispatch_gpu as D
    rows = [c for c in CASES if c[4].get("row")]
    assert len(D.CASES) == 30 and len(rows) == len(D.CASES)
    assert [c[0] for c in rows] == ["row_" + r[0] for r in D.CASES]
    assert {r[3] for r in D.CASES} == {c[3] for c in rows}          # (30 rows, 29 kernel instances: pointwise and pointwise_pool_not_fused share one)
    for (name, shp, call, family), c in zip(D.CASES, rows):
        assert c[2] == (shp[0], shp[1], shp[2], shp[3], shp[4], shp[5], shp[5], shp[6]) and c[4]["row"] == call
    ids = [c[0] for c in CASES]
    assert len(set(ids)) == len(ids)


def test_launch_plans_restate_the_sources_by_hand():
    # conv_wgrad_rows.hip: (3,37,40,256 -> 128): 128-wide co tile, 4 ci tiles x 1 co tile, 2 strips per image, 3 * 2 * 37 = 222 rows, 256 / 4 = 64
    # splits -> ceil(222 / 64) = 4 rows per split -> 56 splits; the slab holds one 9 x 4 x 512 float4 register tile per CU
    p = CE.plan_wg_rows((3, 37, 40, 256, 128, 3, 3, 1), 256)
    assert (p["cot"], p["pairs"], p["tiles_x"], p["total_rows"], p["rows_per_split"], p["splits"], p["slab"]) == (128, 4, 2, 222, 4, 56, True)
    assert p["slab_bytes"] == 256 * 9 * 4 * 512 * 16
    c = CE.wg_rows_cuts((3, 37, 40, 256, 128, 3, 3, 1), 256)
    # split 9 owns rows 36..39: row 36 of strip 0 and rows 0..2 of strip 1 (a second pair of warm-up steps); of the five strip changes at rows
    # 37, 74, 111, 148, 185 only 148 = 4 * 37 falls on a split boundary; the last split has 2 rows
    assert c["crossing"] == 4 and c["mid_strip"] >= 1 and c["last_rows"] == 2 and c["last_strip_width"] == 8
    # 72 output channels: padded to 128 -> one 128-wide tile; 8 channels: one 64-wide tile
    assert CE.plan_wg_rows((2, 32, 64, 256, 72, 3, 3, 1), 256)["cot"] == 128 and CE.plan_wg_rows((2, 16, 32, 256, 8, 3, 3, 1), 256)["cot"] == 64
    p = CE.plan_wg_rows((1, 33, 47, 64, 64, 3, 3, 1), 256)
    assert (p["pairs"], p["total_rows"], p["rows_per_split"], p["splits"]) == (1, 66, 1, 66)
    # (3,37,40,128 -> 64): 64-wide co tile, 2 ci tiles x 1 co tile, 222 rows on 256 / 2 = 128 splits -> 2 rows per split -> 111 splits; split 18 owns
    # rows 36 and 37: the last row of strip 0 and the first of strip 1
    p = CE.plan_wg_rows((3, 37, 40, 128, 64, 3, 3, 1), 256)
    assert (p["cot"], p["pairs"], p["total_rows"], p["rows_per_split"], p["splits"], p["slab"]) == (64, 2, 222, 2, 111, True)
    assert CE.wg_rows_cuts((3, 37, 40, 128, 64, 3, 3, 1), 256)["crossing"] == 3          # strip changes at the odd rows 37, 111, 185
    # a long launch keeps the atomic form: 16 images of 160 x 160, 256 -> 256: 8 pairs, 32 splits of 400 rows
    p = CE.plan_wg_rows((16, 160, 160, 256, 256, 3, 3, 1), 256)
    assert (p["pairs"], p["total_rows"], p["rows_per_split"], p["splits"], p["slab"]) == (8, 12800, 400, 32, False)
    assert not CE.wg_rows_eligible((1, 16, 16, 256, 256, 3, 3, 1)) and CE.wg_rows_eligible((1, 20, 20, 64, 64, 3, 3, 1))          # 16 / 32 < 0.6 <= 20 / 32
    # conv_wgrad_pw.hip: (1,64,72,2304 -> 256): 144 K-steps of 32 pixels, 9 x 1 tiles of 256 x 256, 28 splits -> 6 steps per split -> 24 splits
    p = CE.plan_wg_pw((1, 64, 72, 2304, 256, 1, 1, 1), 256)
    assert (p["ksteps"], p["pairs"], p["steps_per_split"], p["splits"], p["slab"], p["slab_bytes"]) == (144, 9, 6, 24, True, 256 * 32 * 512 * 16)
    assert not CE.wg_pw_eligible((1, 8, 8, 128, 64, 1, 1, 1)) and not CE.wg_pw_eligible((1, 64, 64, 64, 64, 1, 1, 1)) and CE.wg_pw_eligible((1, 64, 64, 128, 64, 1, 1, 1))
    # conv_igemm.hip plan_splitk: (1,10,10,512 -> 512) forward: 128 x 128 tiles: 1 x 4 tiles, 72 K tiles; target 512 -> 128 splits, capped at 72 / 4 = 18,
    # 4 K tiles each
    assert CE.plan_splitk((1, 10, 10, 512, 512, 3, 3, 1), 0, 256) == (18, 4, 100, 512)
    assert CE.conv_workspace_bytes((1, 10, 10, 512, 512, 3, 3, 1), 0, 256) == 18 * 100 * 512 * 4
    # stride 2, data gradient: M = 2 * 20 * 20 pixels of dx, Co = 256 input channels, K = 9 * 512: 7 x 2 tiles -> ceil(512 / 14) = 37 -> capped at 18
    assert CE.plan_splitk((2, 20, 20, 256, 512, 3, 3, 2), 1, 256) == (18, 4, 800, 256)
    # thin head: 16-wide tiles of 64 pixels, target 8 per CU: (2,16,32,256 -> 8): 16 tiles, 36 K tiles -> min(128, 9) = 9 splits of 4
    assert CE.plan_splitk((2, 16, 32, 256, 8, 3, 3, 1), 0, 256) == (9, 4, 1024, 8)
    # a stride that is no power of two has no split data gradient; a large map does not split
    assert CE.plan_splitk((1, 9, 9, 8, 8, 3, 3, 3), 1, 256)[0] == 1 and CE.plan_splitk((4, 136, 128, 64, 64, 3, 3, 1), 0, 256)[0] == 1


def test_launch_plans_equal_the_library_queries():
    """Without a device the library plans for 256 CUs (dh_cu_count), the MI355X's count: every listed shape, both directions."""
    from dan_amd import build as B
    from dan_amd._lib import ConvDesc, bind
    B.build()
    L = bind(ctypes.CDLL(B.OUT))
    shapes = sorted({c[2] for c in CASES} | {(16, 160, 160, 256, 256, 3, 3, 1), (2, 80, 80, 512, 64, 1, 1, 1), (4, 40, 40, 1024, 1024, 1, 1, 1)})
    for shp in shapes:
        N, H, W, Cin, Cout, kh, kw, s = shp
        d = ConvDesc()
        d.N, d.H, d.W, d.Cin, d.Cout, d.kh, d.kw, d.stride = N, H, W, Cin, Cout, kh, kw, s
        d.Ho, d.Wo = -(-H // s), -(-W // s)
        for which in (0, 1):
            assert L.danhip_conv2d_workspace_bytes(ctypes.byref(d), which) == CE.conv_workspace_bytes(shp, which, 256), (shp, which)
        assert L.danhip_conv2d_bwd_weight_workspace_bytes(ctypes.byref(d)) == CE.wgrad_workspace_bytes(shp, 256), shp
