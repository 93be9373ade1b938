"""The deformable sampling kernels (csrc/deform_conv.hip, csrc/deform_fused.hip, the fp32 sampling entry) against the float64 oracle on dyadic
inputs: every comparison is torch.equal on every element against the float64 reference cast to the output's type (tests/deform_exact.py says
why equality is the right check; tests/test_deform_exact_cpu.py asserts its preconditions and the census of knife-edge samples without a GPU).
The reference is always the oracle, never another kernel form."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import deform_exact as DE  # noqa: E402

pytestmark = pytest.mark.gpu

NAMES = [c.name for c in DE.CASES]
NAN = float("nan")


def _same(got, ref, what):
    """Equality on every element with the float64 reference cast to the output's type; the message names the first difference."""
    got = got.detach().cpu()
    want = ref.to(got.dtype).reshape(got.shape)
    if torch.equal(got, want):
        return
    bad = ~(got == want)
    first = bad.nonzero()[0].tolist()
    at = tuple(first)
    pytest.fail("%s: %d of %d elements differ; first at %s: got %r, reference %r" % (what, int(bad.sum().item()), bad.numel(), first,
                                                                                      got[at].item(), want[at].item()))


def _sample_bwd(dev, x, off, dS, dx_start, c, accumulate):
    """danhip_deform_sample_bwd on a NaN-filled workspace (the call zeroes what it reads) -> (dX, dOffset, workspace); outputs that the call
    must overwrite start as NaN."""
    from dan_amd import _lib
    dx = dx_start.clone() if accumulate else torch.full_like(x, NAN)
    doff = torch.full_like(off, NAN)
    ws = torch.full((x.numel() + 64,), NAN, dtype=torch.float32, device=dev)
    _lib.call("danhip_deform_sample_bwd", _lib.ptr(x), _lib.ptr(off), _lib.ptr(dS), _lib.ptr(dx), _lib.ptr(doff), c.N, c.H, c.W, c.C, 3, 3, 1, c.dil, c.dg,
              accumulate, _lib.ptr(ws), ws.numel() * 4, _lib.stream())
    torch.cuda.synchronize()
    return dx, doff, ws


def _stat(ws):
    return tuple(ws[-64:].view(torch.int32)[:2].tolist())


# ================================================================================================================ forward
@pytest.mark.parametrize("name", NAMES)
def test_sampling_forward_equals_the_reference(name, dev):
    """The stand-alone im2col kernel, the fp32 sampling entry, the column buffer the convolution's forward leaves (the fused kernel's for
    C / dg == 64) and y with gradients off and on."""
    from dan_amd import _lib, ops
    c = DE.CASE_BY_NAME[name]
    d = DE.check_case(c)
    fc = DE.fwd_conv_data(name)                                         # (asserts |16 y| <= 256 on the reference)
    xd, od = d.x.to(ops.ACT).to(dev), d.off.to(ops.ACT).to(dev)
    with torch.no_grad():
        S = ops.deform_sample(xd, od, 3, 3, dilation=c.dil, deformable_group=c.dg)
    torch.cuda.synchronize()
    _same(S, d.col, "deform_sample")
    x32, o32 = d.x.float().to(dev), d.off.float().to(dev)
    S32 = torch.full((c.N, c.H, c.W, 9 * c.C), NAN, dtype=torch.float32, device=dev)
    _lib.call("danhip_deform_sample_fwd_f32", _lib.ptr(x32), _lib.ptr(o32), _lib.ptr(S32), c.N, c.H, c.W, c.C, 3, 3, 1, c.dil, c.dg, _lib.stream())
    torch.cuda.synchronize()
    _same(S32, d.col, "deform_sample_fwd_f32")
    fused = _lib.lib().danhip_deform_conv_fused(c.N, c.H, c.W, c.C, c.C, 3, 3, 1, c.dg) == 1
    assert fused == (c.C // c.dg == 64)
    w1 = DE.filter_hwio(fc.w).float().to(dev)
    bd = fc.bias.float().to(dev)
    with torch.no_grad():
        y0 = ops.deform_conv(xd, w1, bd, od, 3, 3, dilation=c.dil, deformable_group=c.dg, relu=False)
    torch.cuda.synchronize()
    _same(y0, fc.y, "y, gradients off")
    y1 = ops.deform_conv(xd.clone().requires_grad_(True), w1.clone().requires_grad_(True), bd, od, 3, 3, dilation=c.dil, deformable_group=c.dg, relu=False)
    torch.cuda.synchronize()
    _same(y1, fc.y, "y, gradients on")
    col = y1.grad_fn.col
    assert col is not None
    _same(col[: S.numel() * 2].view(ops.ACT).view(S.shape), d.col, "column buffer of the convolution's forward")


# ================================================================================================================ backward
@pytest.mark.parametrize("name", NAMES)
def test_sampling_backward_equals_the_reference_in_every_form(name, dev):
    """danhip_deform_sample_bwd: deform_bwd_form {0, 1, 2, 3} x deform_dx_untiled {0, 1} x accumulate {0, 1} (the generic kernel of
    C / dg != 64 ignores the options and must not mind them); dX and dOffset equal the reference, the two counters behind the workspace
    equal the census."""
    from dan_amd import _lib, ops
    c = DE.CASE_BY_NAME[name]
    d = DE.check_case(c)
    cen = DE.census(c)
    xd, od, sd, x0 = (t.to(ops.ACT).to(dev) for t in (d.x, d.off, d.dS, d.dx0))
    gathered = c.C // c.dg == 64
    try:
        for form in (0, 1, 2, 3):
            for untiled in (0, 1):
                _lib.lib().danhip_set_option(b"deform_bwd_form", form)
                _lib.lib().danhip_set_option(b"deform_dx_untiled", untiled)
                for acc in (0, 1):
                    dx, doff, ws = _sample_bwd(dev, xd, od, sd, x0, c, acc)
                    what = "form %d, untiled %d, accumulate %d" % (form, untiled, acc)
                    _same(doff, d.doff, "dOffset, " + what)
                    _same(dx, d.dx + d.dx0 if acc else d.dx, "dX, " + what)
                    if gathered:
                        assert _stat(ws) == (cen["far2"], cen["far1"]), what
    finally:
        _lib.lib().danhip_set_option(b"deform_bwd_form", 0)
        _lib.lib().danhip_set_option(b"deform_dx_untiled", 0)


# ================================================================================================================ statistic
# 2 x 8 x 16 x 64, one group: 2304 offset pairs; scatter form when more than 2304 / 20 * 3 = 345 pairs leave [-2, 2) (`stat[0] > thresh2`),
# +-1 window while at most 2304 / 128 = 18 leave [-1, 1) (`stat[1] <= thresh1`), +-2 window between.
STAT_SHAPE = DE.Case("stat", 2, 8, 16, 64, 1, 1, 900, 0.25)
STAT_SETS = [(1.25, 17, "near"), (1.25, 18, "near"), (1.25, 19, "wide"), (2.25, 344, "wide"), (2.25, 345, "wide"), (2.25, 346, "scatter")]


@pytest.mark.parametrize("value,count,want", STAT_SETS)
def test_statistic_and_the_form_it_selects(value, count, want, dev):
    """Offsets just below, on and just above each threshold: the counters equal the census, the automatic form (option 0) returns the
    reference, and it is the form the thresholds name.  Which form ran shows in the fp32 side buffer the call leaves in its workspace: the
    scatter form accumulates all of dX there; the +-1 window only the corners two pixels from their tap's nominal position (the planted
    offsets of 1.25 px have one); the +-2 window nothing at all for offsets inside [-2, 2)."""
    from dan_amd import ops
    c = STAT_SHAPE
    pairs = c.N * c.H * c.W * c.dg * 9
    assert (pairs // 20 * 3, pairs // 128) == (345, 18)
    x = DE.gen_x(c.N, c.H, c.W, c.C, c.seed)
    dS = DE.gen_ternary((c.N * c.H * c.W, 9 * c.C), c.density, c.seed + 1)
    off = DE.planted_offsets(c.N, c.H, c.W, c.dg, c.seed + 2, count, value)
    far2, far1 = DE.far_counts(off)
    assert (far2, far1) == ((count, count) if value >= 2 else (0, count))
    assert want == ("scatter" if far2 > pairs // 20 * 3 else "near" if far1 <= pairs // 128 else "wide")
    dx_ref, doff_ref = DE.sample_bwd_ref(x, off, dS, c.dg, c.dil)
    DE.check_exact(DE.col_ref(x, off, c.dg, c.dil), 1.0 / 16, True)
    DE.check_exact(doff_ref, 0.25, True)
    DE.check_exact(dx_ref, 1.0 / 16, True)
    assert (dx_ref != 0).float().mean().item() > 0.3
    xd, od, sd = (t.to(ops.ACT).to(dev) for t in (x, off, dS))
    dx, doff, ws = _sample_bwd(dev, xd, od, sd, None, c, 0)            # options at their defaults: form by the statistic, tile kernels
    assert _stat(ws) == (far2, far1)
    _same(doff, doff_ref, "dOffset")
    _same(dx, dx_ref, "dX")
    side = ws[:-64].cpu()
    if want == "scatter":
        _same(side, dx_ref, "scatter form: the fp32 buffer holds all of dX")
    else:
        assert torch.isfinite(side).all()                               # (an offset left [-1, 1): the buffer was zeroed)
        assert not torch.equal(side, dx_ref.float().reshape(-1))
        if value < 2:                                                   # (2.25 px has a corner three pixels away: far for either window)
            assert bool((side != 0).any()) == (want == "near"), "far corners in the side buffer: %d" % int((side != 0).sum().item())


def test_no_offset_outside_the_narrow_window_leaves_the_workspace_alone(dev):
    """Bulk offsets only: both counters zero, the +-1 window runs, and the side buffer is neither zeroed nor read."""
    from dan_amd import ops
    c = STAT_SHAPE
    x = DE.gen_x(c.N, c.H, c.W, c.C, c.seed)
    dS = DE.gen_ternary((c.N * c.H * c.W, 9 * c.C), c.density, c.seed + 1)
    off = DE.bulk_offsets(c.N, c.H, c.W, c.dg, c.seed + 2)
    assert DE.far_counts(off) == (0, 0)
    dx_ref, doff_ref = DE.sample_bwd_ref(x, off, dS, c.dg, c.dil)
    DE.check_exact(doff_ref, 0.25, True)
    DE.check_exact(dx_ref, 1.0 / 16, True)
    xd, od, sd = (t.to(ops.ACT).to(dev) for t in (x, off, dS))
    dx, doff, ws = _sample_bwd(dev, xd, od, sd, None, c, 0)
    assert _stat(ws) == (0, 0)
    _same(doff, doff_ref, "dOffset")
    _same(dx, dx_ref, "dX")
    assert torch.isnan(ws[:-64]).all()


# ================================================================================================================ delivery, whole op
@pytest.mark.parametrize("name", DE.CONV_CASES)
def test_delivery_into_a_slot_equals_the_reference(name, dev):
    """danhip_deform_conv_bwd_deliver: dX times (x > 0), added into a slot that holds small integers; dOffset and dW as well."""
    from dan_amd import _lib, ops
    c = DE.CASE_BY_NAME[name]
    d = DE.check_case(c)
    cv = DE.check_conv(name)
    want_dx = DE.check_exact(cv.dx * (d.x > 0) + d.dx0, 1.0 / 16, True)
    cout = c.C
    xd, od, gd, dx = (t.to(ops.ACT).to(dev) for t in (d.x, d.off, cv.dy, d.dx0))
    w1 = DE.filter_hwio(cv.w).float().to(dev)
    desc = ops._desc(c.N, c.H, c.W, 9 * c.C, cout, 1, 1, 1)
    _, wb = ops.pack_conv_weight(desc, w1, need_bwd=True)
    doff = torch.full_like(od, NAN)
    dw = torch.zeros((1, 1, 9 * c.C, cout), dtype=torch.float32, device=dev)
    nws = _lib.lib().danhip_deform_conv_workspace_bytes(c.N, c.H, c.W, c.C, 3, 3, 1, 1)
    ws = torch.empty(nws, dtype=torch.uint8, device=dev)
    _lib.call("danhip_deform_conv_bwd_deliver", _lib.ptr(xd), _lib.ptr(wb), _lib.ptr(od), _lib.ptr(gd), None, _lib.ptr(dx), _lib.ptr(doff), _lib.ptr(dw), None,
              c.N, c.H, c.W, c.C, cout, 3, 3, 1, c.dil, c.dg, 1, 1, _lib.ptr(ws), nws, _lib.stream())
    torch.cuda.synchronize()
    _same(dx, want_dx, "delivered dX")
    _same(doff, cv.doff, "dOffset")
    _same(dw, DE.filter_hwio(cv.dw), "dW")


@pytest.mark.parametrize("name", DE.CONV_CASES)
def test_whole_op_forward_and_backward_equal_the_reference(name, dev):
    """custom_op.deform_conv_op: y, dX, dOffset (16 bits) and dW (fp32, |16 dW| < 2^24 asserted on the reference)."""
    from dan_amd import ops
    from dan_amd.utility import custom_op
    c = DE.CASE_BY_NAME[name]
    d = DE.check_case(c)
    cv = DE.check_conv(name)
    xd = d.x.to(ops.ACT).to(dev).requires_grad_(True)
    od = d.off.to(ops.ACT).to(dev).requires_grad_(True)
    wd = cv.w.float().to(dev).requires_grad_(True)
    y = custom_op.deform_conv_op(xd, wd, od, [1, 1, c.dil, c.dil], "SAME", [1, 1, 1, 1], 1, c.dg)
    y.backward(cv.dy.to(ops.ACT).to(dev))
    torch.cuda.synchronize()
    _same(y, DE.check_exact(cv.y - cv.bias, 1.0 / 16, True), "y")
    _same(xd.grad, cv.dx, "dX")
    _same(od.grad, cv.doff, "dOffset")
    assert wd.grad.dtype == torch.float32
    _same(wd.grad, cv.dw, "dW")
