"""Pins tests/infer_exact.py itself (no GPU): the limb arithmetic and the float64 identity the split-operand cases rest on, the conditions every
listed case must meet on its reference, the restated kernel selection of a split call against hand-worked plans and the fp16 library's own
workspace query, and the references of the pooling, normalisation and resize kernels against the oracle and hand-written values."""
import ctypes
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import conv_exact as CE  # noqa: E402
import infer_exact as IE  # noqa: E402
from oracle import tf_ops as T  # noqa: E402

F64 = torch.float64


def test_limbs_and_the_three_product_identity():
    """x = 16 a + 2^-8 b |a| as limbs of x / 4, w as limbs of w 2^9: normal halves, hi + lo exact; the float64 identity
    conv(x, w) == [conv(xh, wh) + conv(xl, wh) + conv(xh, wl)] 2^(E-e) + conv(xl, wl) 2^(E-e); and the three-product sum is exact in fp32."""
    inp = IE.split_inputs(CE.S(1, 8, 8, 64, 64), "C")
    xh, xl, wh, wl, we = inp["xh"], inp["xl"], inp["wh"], inp["wl"], inp["we"]
    assert we == 9 and set(xh.unique().tolist()) == {-4.0, 0.0, 4.0} and set(xl.unique().tolist()) == {-2.0 ** -10, 0.0, 2.0 ** -10}
    assert set(wh.unique().tolist()) == {-8192.0, 0.0, 8192.0} and set(wl.unique().tolist()) == {-2.0, 0.0, 2.0}
    assert not (xl != 0)[xh == 0].any() and not (wl != 0)[wh == 0].any()          # lo only where hi is
    sc = 2.0 ** (IE.LIMB_EXP - we)
    three = (CE.conv_ref(xh, wh) + CE.conv_ref(xl, wh) + CE.conv_ref(xh, wl)) * sc
    assert torch.equal(three + CE.conv_ref(xl, wl) * sc, inp["full"]) and torch.equal(three, inp["pre"])
    f32 = lambda t: t.to(torch.float32)
    acc = CE.conv_ref(f32(torch.cat([xh, xl, xh], -1)).double(), f32(torch.cat([wh, wh, wl], 2)).double())       # the kernel's 3C convolution
    assert torch.equal(acc * sc, inp["pre"]) and IE.is_f32(acc)
    x3 = f32(torch.cat([xh, xl, xh], -1)).permute(0, 3, 1, 2)
    w3 = f32(torch.cat([wh, wh, wl], 2)).permute(3, 2, 0, 1)
    got = torch.nn.functional.conv2d(torch.nn.functional.pad(x3, (1, 1, 1, 1)), w3).permute(0, 2, 3, 1)          # summed in fp32, in torch's order
    assert torch.equal(got.double() * sc, inp["pre"])
    assert IE.weight_exp(torch.tensor([16.0])) == 9 and IE.weight_exp(torch.tensor([2.0 ** -4])) == 17 and IE.weight_exp(torch.tensor([1.0])) == 13
    assert IE.quantum(torch.tensor([12.0, 0.0, -40.0], dtype=F64)) == 4.0 and IE.quantum(torch.tensor([0.375], dtype=F64)) == 0.125
    # the raw map: [hi | lo | hi]; a value that needs its lo limb
    m = IE.limb_map(torch.tensor([[2049.0, -0.0]], dtype=F64))
    assert m.tolist() == [[2048.0, -0.0, 1.0, 0.0, 2048.0, -0.0]] and m.view(torch.int16)[0, 1].item() == -32768


@pytest.mark.parametrize("case", IE.SPLIT_CASES, ids=[c[0] for c in IE.SPLIT_CASES])
def test_split_case_meets_its_conditions_on_the_reference(case):
    """Every class of the case: normal limbs, hi + lo exact, abs-sum below 2^24 quanta, fp32 values, >= 5 % lo limbs, a mostly non-zero lo.lo
    term in class C, a ReLU that clips some outputs; and the restated launch (256 CUs) is in the family the case is listed for."""
    print(case[0], IE.check_split_case(case, cus=256))


@pytest.mark.parametrize("cls", IE.CHAIN_CLASSES)
def test_chain_stages_stay_exact(cls):
    print(cls, IE.check_chain_inputs(IE.chain_inputs(cls)))


def test_split_table_covers_what_it_is_there_for():
    plans = {c[0]: IE.plan_split_call(c[1], not IE.case_opts(c)["f32"], IE.case_opts(c)["padding"], 256) for c in IE.SPLIT_CASES}
    labels = {p["label"] for p in plans.values()}
    assert any(l.startswith(CE.HALO + "8, 32, 128,") for l in labels) and any(l.startswith(CE.HALO + "16, 16, 64,") for l in labels)
    assert any(l.startswith(CE.HALO + "8, 32, 64, 8, 1, 1, 4") for l in labels) and any(l.endswith("false, 1, false>") for l in labels)
    assert any(l.startswith(CE.FLAT) and l.endswith("true>") for l in labels) and any(l.startswith(CE.FLAT) and l.endswith("false>") for l in labels)
    assert sum(1 for p in plans.values() if p["splits"] >= 2) >= 2
    assert len({c[0] for c in IE.SPLIT_CASES}) == len(IE.SPLIT_CASES)


def test_split_selection_restates_the_sources_by_hand():
    P = IE.plan_split_call
    # (1,16,32,64 -> 128) 3x3: 192 limb channels, 27 K tiles, M = 512: 4 x 1 tiles of 128 x 128, target 512 -> 128 splits, capped at 27 / 4 = 6 of
    # 5 K tiles; 4 tiles <= 160: ops hands the scratch over, 4 * 1 * 2 <= 256: select_conv prefers the split -> flat-M FAST, not the halo kernel
    p = P(CE.S(1, 16, 32, 64, 128), True)
    assert (p["ktiles"], p["splits"], p["ws_bytes"], p["label"]) == (27, 6, 6 * 512 * 128 * 4, "conv_igemm_kernel<128, 128, 2, true>")
    assert P(CE.S(1, 16, 32, 64, 128), True, use_splitk=False)["label"] == "conv3x3_halo_kernel<8, 32, 128, 4, 2, 1, 4, false, 0, false>"
    # (1,104,160): M = 16640 -> 130 tiles: scratch is handed over (4 splits of 7), but 130 * 2 > 256: no preference -> halo, 8 x 32 (utilisation 1)
    p = P(CE.S(1, 104, 160, 64, 128), True)
    assert (p["query_bytes"], p["splits"], p["label"]) == (4 * 16640 * 128 * 4, 1, "conv3x3_halo_kernel<8, 32, 128, 4, 2, 1, 4, false, 0, false>")
    # 130 x 130: 8 x 32 tiles cover 136 x 160 (0.777), 16 x 16 tiles 144 x 144 (0.815)
    assert P(CE.S(1, 130, 130, 64, 64), True)["label"] == "conv3x3_halo_kernel<16, 16, 64, 8, 1, 1, 4, false, 0, false>"
    # thin head: fp32 output takes the head instance, limb output never does
    assert P(CE.S(1, 104, 160, 64, 8), False)["label"] == "conv3x3_halo_kernel<8, 32, 64, 8, 1, 3, 3, false, 1, false>"
    assert P(CE.S(1, 104, 160, 64, 8), True)["label"] == "conv_igemm_kernel<64, 16, 1, true>"
    # (1,20,20,256 -> 256) 1x1: 768 limb channels = 12 K tiles, 4 x 2 tiles -> 64 splits, capped at 12 / 4 = 3
    p = P(CE.S(1, 20, 20, 256, 256, 1), True)
    assert (p["ktiles"], p["splits"], p["label"]) == (12, 3, "conv_igemm_kernel<128, 128, 2, true>")
    # (4,52,52,64 -> 256): 85 x 2 = 170 tiles of 128 x 128 > 160: no scratch asked for
    assert P(CE.S(4, 52, 52, 64, 256, 1), True)["ws_bytes"] == 0
    # the deformable GEMM: 5184 limb channels = 81 K tiles on one tile: 512 splits, capped at 81 / 4 = 20 -> 5 K tiles each -> 17 splits
    p = P(CE.S(1, 8, 8, 1728, 64, 1), True)
    assert (p["ktiles"], p["splits"]) == (81, 17)
    # thin head on a small map: 16-wide tiles of 64 pixels, target 8 * 256: 2 tiles -> 1024 splits, capped at 36 of 6 K tiles
    p = P(CE.S(1, 10, 10, 512, 6), False)
    assert (p["ktiles"], p["splits"], p["label"]) == (216, 36, "conv_igemm_kernel<64, 16, 1, true>")
    # stride 2, 33 x 31 -> 17 x 16, M = 544: 5 x 2 tiles, 54 K tiles -> 52 splits, capped at 13 -> 5 K tiles each -> 11 splits
    p = P(CE.S(2, 33, 31, 128, 256, 3, 2), True)
    assert (p["M"], p["ktiles"], p["splits"]) == (544, 54, 11)
    # 5 channels: 15 limb channels + one zero pad column, K = 144 -> 3 K tiles (< 8: no split); 72 channels: 216 limb channels, not FAST
    p = P(CE.S(2, 9, 11, 5, 16), True)
    assert (p["limb_shape"][3], p["ktiles"], p["splits"], p["label"]) == (16, 3, 1, "conv_igemm_kernel<64, 16, 1, false>")
    assert P(CE.S(1, 12, 12, 72, 64, 1), True)["label"] == "conv_igemm_kernel<256, 64, 1, false>"
    # 'valid': 9 x 10 -> 7 x 8
    assert P(CE.S(1, 9, 10, 64, 64), True, "valid")["M"] == 56


def test_split_plans_equal_the_fp16_library_query():
    """danhip_conv2d_workspace_bytes of the fp16 build on the limb descriptor (256 CUs without a device)."""
    from dan_amd import build as B
    from dan_amd._lib import ConvDesc, bind
    B.build()
    L = bind(ctypes.CDLL(os.path.join(os.path.dirname(B.OUT), "libdanhip_f16.so")), ["danhip_conv2d_workspace_bytes"])
    for c in IE.SPLIT_CASES:
        o = IE.case_opts(c)
        p = IE.plan_split_call(c[1], not o["f32"], o["padding"], 256)
        N, H, W, C3, Cout, kh, kw, s = p["limb_shape"]
        d = ConvDesc()
        d.N, d.H, d.W, d.Cin, d.Cout, d.kh, d.kw, d.stride = N, H, W, C3, Cout, kh, kw, s
        d.Ho, d.Wo = IE.out_hw(H, W, kh, kw, s, o["padding"])
        assert L.danhip_conv2d_workspace_bytes(ctypes.byref(d), 0) == p["query_bytes"], c[0]


@pytest.mark.parametrize("nhw", IE.FIRST_SHAPES)
def test_first_layer_case_meets_its_conditions(nhw):
    print(nhw, IE.check_first_inputs(IE.first_inputs(nhw)))
    N, H, W = nhw
    assert nhw != (1, 3, 45) or (N * H * -(-W // 4) * 8) % 256 != 0 and N * H * -(-W // 4) * 8 > 256


def test_pool_inputs_hold_the_windows_they_are_there_for():
    tot = dict(shared_pos=0, shared_neg=0, ties=0, negative=0, zeros=0)
    for shp in IE.POOL_SHAPES:
        inp = IE.pool_inputs(shp)
        for k, v in IE.check_pool_inputs(inp).items():
            tot[k] += v
        want, loose, s = IE.pool_expected(inp)
        C = shp[3]
        assert torch.equal(want[..., :C], want[..., 2 * C:])
        tot["mixed_zeros"] = tot.get("mixed_zeros", 0) + int(loose.sum())
        assert (want[..., 2].view(torch.int16) == -32768).all()                                     # the all -0 channel stays -0
        assert (want[..., :2].double() + want[..., C:C + 2].double() < 0).all()                     # the negative channels stay negative at every border
        # a pool that compared hi limbs only would differ
        hi_only = CE.pool_ref(inp["hi"])[0]
        if shp[1] > 1 and shp[2] > 1:
            assert not torch.equal(hi_only, (want[..., :C].double() + want[..., C:2 * C].double()))
    assert all(v >= 1 for v in tot.values()), tot
    # a hand-written window, one channel each: shared hi, lo decides; all negative; a tie
    hi = torch.tensor([[[[1.0, -3.0, 2.5]], [[1.0, -1.5, 2.5]]]], dtype=F64)           # [1, 2, 1, 3]
    lo = torch.tensor([[[[-2.0 ** -13, 2.0 ** -13, 0.0]], [[2.0 ** -13, 0.0, 0.0]]]], dtype=F64)
    want, _, _ = IE.pool_expected(dict(hi=hi, lo=lo))
    assert want.tolist() == [[[[1.0, -1.5, 2.5, 2.0 ** -13, 0.0, 0.0, 1.0, -1.5, 2.5]]]]


def test_l2_bound_and_reference():
    assert IE.l2_bound(8, False) == (7.5 * 2.0 ** -24, 0.0) and IE.l2_bound(512, True) == (15 * 2.0 ** -24, 2.0 ** -25)
    assert IE.l2_bound(1024, False)[0] == 15 * 2.0 ** -24 and IE.l2_bound(1024, True)[0] == 2.0 ** -20
    assert all(IE.l2_bound(C, lim)[0] <= 2.0 ** -20 for C in IE.L2_CS for lim in (False, True))
    for C in (8, 72):
        for e in (0, 2):
            inp = IE.l2_inputs(5, C, e)
            IE.check_l2_inputs(inp)
            want = T.l2_normalize(inp["carried"].float().view(1, 1, 5, C), inp["gamma"].float()).double().view(5, C)
            ref = IE.l2_ref(inp["carried"], inp["gamma"])
            assert (ref - want).abs().max().item() <= 1e-5 * want.abs().max().item()


def test_layer_references_are_the_oracle_ops():
    for shp in IE.LAYER_SHAPES:
        x = IE.avgpool_inputs(shp)
        assert torch.equal(IE.avgpool_ref(x.double()), T.avg_pool_2x2_s1_same(x).double())
        assert torch.equal(IE.avgpool_ref(x.double()).float().double(), IE.avgpool_ref(x.double()))           # exact in fp32
        m = IE.maxpool_inputs(shp)
        assert torch.equal(CE.pool_ref(m)[0], T.max_pool_2x2_same(m)) and (CE.pool_ref(m)[0][..., 0] < 0).all()
        for r in (2, 4):
            up = IE.resize_inputs(shp)
            ref, _ = IE.resize_ref(up, shp[1] * r, shp[2] * r)
            assert torch.equal(ref.float().double(), ref)
            want = T.resize_bilinear_legacy(up, shp[1] * r, shp[2] * r).double()
            assert (ref - want).abs().max().item() <= 1e-5 * max(1.0, want.abs().max().item())
    # hand-written: 2 -> 4 columns, legacy mapping src = dst / 2, the last column clamps
    up = torch.tensor([1.0, 3.0]).view(1, 1, 2, 1)
    assert IE.resize_ref(up, 1, 4)[0].view(-1).tolist() == [1.0, 2.0, 3.0, 3.0]
    x = torch.tensor([[1.0, 2.0], [4.0, 8.0]], dtype=F64).view(1, 2, 2, 1)
    assert IE.avgpool_ref(x).view(-1).tolist() == [3.75, 5.0, 6.0, 8.0]
    i0, i1, l = IE.resize_coords(10, 19)
    assert i0[18].item() == 9 and i1[18].item() == 9 and 0 < l[1].item() < 1


@pytest.mark.parametrize("case", IE.F32_CONV_CASES, ids=[c[0] for c in IE.F32_CONV_CASES])
def test_f32_conv_case_meets_its_conditions(case):
    cid, shp, padding = case
    inp = IE.f32_conv_inputs(shp, padding)
    print(cid, IE.check_f32_conv_inputs(inp))
    N, H, W, Cin, Cout, kh, kw, s = shp
    assert tuple(inp["pre"].shape) == (N,) + IE.out_hw(H, W, kh, kw, s, padding) + (Cout,)


def test_loop_sizes_pass_the_caps():
    N, H, W, C = IE.MAXPOOL_LOOP
    assert N * ((H + 1) // 2) * ((W + 1) // 2) * C > IE.LOOP_CAP
    N, H, W, C = IE.AVGPOOL_LOOP
    assert N * H * W * C > IE.LOOP_CAP
    (N, H, W, C), r = IE.RESIZE_LOOP
    assert N * H * r * W * r * C > IE.LOOP_CAP
