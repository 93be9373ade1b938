"""The transposed convolution 4x4 / stride 2 (csrc/conv_transpose.hip) through the C ABI against the float64 reference of
tests/conv_transpose_exact.py: forward, data gradient and weight / bias gradient as EQUALITIES on integer cases (a term dropped or counted
twice at a phase seam, a border tap, the crop or a tile edge is a whole-number difference), the error returns, and the fp32 entry within a
bound derived from its sum length."""
import ctypes
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import conv_transpose_exact as CT  # noqa: E402

pytestmark = pytest.mark.gpu

CASES = CT.all_cases()
IDS = [c["name"] for c in CASES]
EINVAL = -1


def _dims(c):
    return tuple(c[k] for k in ("N", "Hi", "Wi", "Ho", "Wo", "Cin", "Cout"))


def _act(t, dev):
    from dan_amd import _lib
    return t.to(_lib.ACT_DTYPE).to(dev).contiguous()


def _packed(c, dev):
    from dan_amd import _lib
    w = c["w"].to(torch.float32).to(dev).contiguous()
    wf = torch.empty((4, 4, c["Cout"], c["Cin"]), dtype=_lib.ACT_DTYPE, device=dev)
    wb = torch.empty((4, 4, c["Cin"], c["Cout"]), dtype=_lib.ACT_DTYPE, device=dev)
    _lib.call("danhip_conv_transpose4x4s2_pack_weight", _lib.ptr(w), _lib.ptr(wf), _lib.ptr(wb), c["Cin"], c["Cout"], _lib.stream())
    return wf, wb


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_forward_equals_the_reference(case, dev):
    from dan_amd import _lib
    c = CT.inputs(case)
    x, (wf, _) = _act(c["x"], dev), _packed(c, dev)
    b, lateral = c["b"].to(torch.float32).to(dev), _act(c["lateral"], dev)
    for with_lateral in (False, True):
        for with_bias in (False, True):
            out = torch.full((c["N"], c["Ho"], c["Wo"], c["Cout"]), 77.0, dtype=_lib.ACT_DTYPE, device=dev)
            _lib.call("danhip_conv_transpose4x4s2_add_fwd", _lib.ptr(x), _lib.ptr(wf), _lib.ptr(b) if with_bias else None,
                      _lib.ptr(lateral) if with_lateral else None, _lib.ptr(out), *_dims(c), _lib.stream())
            CT.assert_equal(out, CT.expected_forward(case, with_lateral, with_bias), "%s forward lateral=%s bias=%s" % (c["name"], with_lateral, with_bias))


@pytest.mark.parametrize("case", [c for c in CASES if c["kind"] == "taps"], ids=[n for n in IDS if n.startswith("taps")])
def test_tap_counts_on_the_device(case, dev):
    """All-ones x and W, no bias, no lateral: every output is Cin x (taps reaching its row) x (taps reaching its column) - 1, 2 or 4 times
    Cin at corner, edge and interior - counted by hand (CT.tap_counts), not by the reference."""
    from dan_amd import _lib
    c = CT.inputs(case)
    x, (wf, _) = _act(c["x"], dev), _packed(c, dev)
    out = torch.full((c["N"], c["Ho"], c["Wo"], c["Cout"]), 77.0, dtype=_lib.ACT_DTYPE, device=dev)
    _lib.call("danhip_conv_transpose4x4s2_add_fwd", _lib.ptr(x), _lib.ptr(wf), None, None, _lib.ptr(out), *_dims(c), _lib.stream())
    cy, cx = torch.tensor(CT.tap_counts(c["Hi"], c["Ho"])), torch.tensor(CT.tap_counts(c["Wi"], c["Wo"]))
    want = (c["Cin"] * cy[:, None] * cx[None, :]).to(CT.F64)[None, :, :, None].expand(c["N"], c["Ho"], c["Wo"], c["Cout"])
    assert set(want.unique().tolist()) <= {c["Cin"], 2 * c["Cin"], 4 * c["Cin"]}
    CT.assert_equal(out, want, c["name"] + " tap counts")


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_data_gradient_equals_the_reference(case, dev):
    """With the accumulate flag cleared (the slot's first delivery: the old content must not matter) and set (dx = old + gradient)."""
    from dan_amd import _lib
    c, e = CT.inputs(case), CT.expected(case)
    dout, (_, wb) = _act(c["dout"], dev), _packed(c, dev)
    for acc in (0, 1):
        dx = _act(c["dx0"], dev)
        _lib.call("danhip_conv_transpose4x4s2_dgrad", _lib.ptr(dout), _lib.ptr(wb), _lib.ptr(dx), *_dims(c), acc, _lib.stream())
        CT.assert_equal(dx, e["dx"] + c["dx0"] if acc else e["dx"], "%s data gradient accumulate=%d" % (c["name"], acc))


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_weight_gradient_equals_the_reference(case, dev):
    """dw and db are ADDED to what the buffers hold (gradient sinks): they start at an integer pattern.  The slab count comes from the
    workspace query; the 9 x 17 maps reduce more than one slab."""
    from dan_amd import _lib
    L = _lib.lib()
    c, e = CT.inputs(case), CT.expected(case)
    dims = _dims(c)
    x, dout = _act(c["x"], dev), _act(c["dout"], dev)
    nbytes, slabs = int(L.danhip_conv_transpose4x4s2_wgrad_workspace_bytes(*dims)), int(L.danhip_conv_transpose4x4s2_wgrad_slabs(*dims))
    pixels = c["N"] * c["Hi"] * c["Wi"]
    assert slabs >= 1 and nbytes >= slabs * 16 * c["Cin"] * c["Cout"] * 4 + c["Cout"] * 4
    if (c["Hi"], c["Wi"]) == (9, 17):
        assert slabs > 1 and pixels > CT.WGRAD_STEP * (slabs - 1), (slabs, pixels)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    dw = torch.full((4, 4, c["Cout"], c["Cin"]), 3.0, dtype=torch.float32, device=dev)
    db = torch.full((c["Cout"],), -5.0, dtype=torch.float32, device=dev)
    _lib.call("danhip_conv_transpose4x4s2_wgrad", _lib.ptr(x), _lib.ptr(dout), _lib.ptr(dw), _lib.ptr(db), *dims, _lib.ptr(ws), nbytes, _lib.stream())
    CT.assert_equal(dw, e["dw"] + 3.0, c["name"] + " weight gradient")
    CT.assert_equal(db, e["db"] - 5.0, c["name"] + " bias gradient")
    # a workspace one byte short is refused before any launch
    rc = L.danhip_conv_transpose4x4s2_wgrad(_lib.ptr(x), _lib.ptr(dout), _lib.ptr(dw), _lib.ptr(db), *dims, _lib.ptr(ws), nbytes - 1, _lib.stream())
    assert rc == -3 and b"workspace" in L.danhip_last_error()
    CT.assert_equal(dw, e["dw"] + 3.0, c["name"] + " weight gradient after the refused call")


@pytest.mark.parametrize("bad", ["cin72", "cout72", "ho_plus_one", "wo_minus_two"])
def test_unsupported_shapes_return_the_error_and_write_nothing(bad, dev):
    from dan_amd import _lib
    L = _lib.lib()
    N, Hi, Wi, Cin, Cout = 1, 3, 5, 64, 64
    Ho, Wo = 2 * Hi, 2 * Wi
    if bad == "cin72":
        Cin = 72
    elif bad == "cout72":
        Cout = 72
    elif bad == "ho_plus_one":
        Ho += 1
    else:
        Wo -= 2
    dims = (N, Hi, Wi, Ho, Wo, Cin, Cout)
    act = _lib.ACT_DTYPE
    x = torch.ones((N, Hi, Wi, Cin), dtype=act, device=dev)
    dout = torch.ones((N, Ho, Wo, Cout), dtype=act, device=dev)
    w16 = torch.ones((16 * Cin * Cout,), dtype=act, device=dev)
    out = torch.full((N, Ho + 2, Wo + 2, Cout + 8), 77.0, dtype=act, device=dev)       # (larger than any reading of the shape)
    dx = torch.full((N, Hi + 2, Wi + 2, Cin + 8), 77.0, dtype=act, device=dev)
    dw = torch.full((16 * (Cin + 8) * (Cout + 8),), 77.0, dtype=torch.float32, device=dev)
    db = torch.full((Cout + 8,), 77.0, dtype=torch.float32, device=dev)
    ws = torch.empty(1 << 20, dtype=torch.uint8, device=dev)
    st = _lib.stream()
    assert L.danhip_conv_transpose4x4s2_add_fwd(_lib.ptr(x), _lib.ptr(w16), None, None, _lib.ptr(out), *dims, st) == EINVAL
    assert L.danhip_last_error()
    assert L.danhip_conv_transpose4x4s2_dgrad(_lib.ptr(dout), _lib.ptr(w16), _lib.ptr(dx), *dims, 0, st) == EINVAL
    assert L.danhip_conv_transpose4x4s2_wgrad(_lib.ptr(x), _lib.ptr(dout), _lib.ptr(dw), _lib.ptr(db), *dims, _lib.ptr(ws), ws.numel(), st) == EINVAL
    xf, wf32, of = x.float(), torch.ones((16 * Cin * Cout,), dtype=torch.float32, device=dev), torch.full(out.shape, 77.0, dtype=torch.float32, device=dev)
    assert L.danhip_conv_transpose4x4s2_add_fwd_f32(_lib.ptr(xf), _lib.ptr(wf32), None, None, _lib.ptr(of), *dims, st) == EINVAL
    assert int(L.danhip_conv_transpose4x4s2_wgrad_workspace_bytes(*dims)) == 0
    torch.cuda.synchronize()
    for t in (out, dx, dw, db, of):
        assert bool((t == 77.0).all()), bad


@pytest.mark.parametrize("shape", [(1, 1, 1, False, 64, 64), (3, 5, 7, True, 128, 64), (1, 9, 17, False, 64, 128), (1, 3, 5, True, 512, 512),
                                   (2, 4, 9, False, 320, 64)], ids=lambda s: "n%d_%dx%d_%s_%dto%d" % (s[0], s[1], s[2], "crop" if s[3] else "full", s[4], s[5]))
def test_fp32_entry_within_the_roundoff_bound(shape, dev):
    """Random normal inputs against the float64 reference on the same fp32 values.  Each output is a sum of at most K = 4 Cin products plus
    bias plus lateral: K + 2 terms added one after the other in fp32 (FMA: one rounding per product-and-add), so the error is at most
    (K + 2) u sum |terms| with u = 2^-24 - the standard bound gamma_n <= n u for recursive summation, first order."""
    from dan_amd import _lib
    N, Hi, Wi, crop, Cin, Cout = shape
    Ho, Wo = 2 * Hi - int(crop), 2 * Wi - int(crop)
    g = torch.Generator().manual_seed(1234 + Hi * 31 + Wi)
    x = torch.randn((N, Hi, Wi, Cin), generator=g)
    w = torch.randn((4, 4, Cout, Cin), generator=g) * 0.1
    b = torch.randn((Cout,), generator=g)
    lateral = torch.randn((N, Ho, Wo, Cout), generator=g)
    want = CT.reference(x, w, b, lateral, Ho, Wo)["out"]
    terms = CT.reference(x.abs(), w.abs(), b.abs(), lateral.abs(), Ho, Wo)["out"]
    bound = (4 * Cin + 2) * 2.0 ** -24 * terms
    out = torch.full((N, Ho, Wo, Cout), 77.0, dtype=torch.float32, device=dev)
    xd, wd, bd, ld = x.to(dev), w.to(dev), b.to(dev), lateral.to(dev)          # (named: the call reads them after this line has run)
    _lib.call("danhip_conv_transpose4x4s2_add_fwd_f32", _lib.ptr(xd), _lib.ptr(wd), _lib.ptr(bd), _lib.ptr(ld), _lib.ptr(out), N, Hi, Wi, Ho, Wo, Cin, Cout,
              _lib.stream())
    err = (out.cpu().to(CT.F64) - want).abs()
    worst = (err / bound).max().item()
    print("fp32 entry %s: max error %.3e, worst error / bound %.3f" % (shape, err.max().item(), worst))
    assert bool((err <= bound).all()), (shape, worst)


def test_ops_conv_transpose_add_autograd_matches_the_reference(dev):
    """ops.conv_transpose_add as an autograd node without a trainer (gradients come back as tensors): one exact case end to end, and the
    packed operands follow an in-place change of the variable."""
    from dan_amd import _lib, ops
    case = [c for c in CASES if c["name"] == "random_n3_5x7_crop_128to64"][0]
    c, e = CT.inputs(case), CT.expected(case)
    up = _act(c["x"], dev).requires_grad_(True)
    lateral = _act(c["lateral"], dev).requires_grad_(True)
    w = torch.nn.Parameter(c["w"].to(torch.float32).to(dev))
    b = torch.nn.Parameter(c["b"].to(torch.float32).to(dev))
    out = ops.conv_transpose_add(up, w, b, lateral)
    CT.assert_equal(out, CT.expected_forward(case, True, True), "ops forward")
    dup, dlat, dw, db = torch.autograd.grad(out, (up, lateral, w, b), _act(c["dout"], dev))
    CT.assert_equal(dup, e["dx"], "ops dx")
    CT.assert_equal(dlat, c["dout"], "ops dlateral")
    CT.assert_equal(dw, e["dw"], "ops dw")
    CT.assert_equal(db, e["db"], "ops db")
    with torch.no_grad():
        w.mul_(2.0)
        out2 = ops.conv_transpose_add(up.detach(), w, None, None, size=(c["Ho"], c["Wo"]))
    CT.assert_equal(out2, 2.0 * CT.expected_forward(case, False, False), "ops forward after an in-place update of the variable")
    with pytest.raises(ValueError, match="split"):
        with ops.use_context(ops.OpsContext(SPLIT_EVAL=True)):
            ops.conv_transpose_add(up.detach().float(), w, b, None)
