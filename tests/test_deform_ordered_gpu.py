"""The deformable backward in deterministic mode (csrc/deform_far.hip; the order contract is in include/danhip.h): every term once (the dyadic
cases of tests/deform_exact.py, bit for bit against the float64 reference), the ORDER (sequential np.float32 sums in key order, bit for bit),
the kernels against the host emulation, and the mode's scope.  tests/deform_ordered_cases.py holds the cases and says why they decide."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import deform_exact as DE  # noqa: E402
import deform_ordered_cases as OC  # noqa: E402

pytestmark = pytest.mark.gpu
NAN = float("nan")


@pytest.fixture()
def mode():
    from dan_amd import _lib, ops
    with ops.use_context(ops.OpsContext(deterministic=True)):
        yield
    assert _lib.lib().danhip_get_option(b"deterministic") == 0


def _same(got, ref, what):
    got = got.detach().cpu()
    want = ref.to(got.dtype).reshape(got.shape)
    if torch.equal(got, want):
        return
    bad = ~(got == want)
    at = tuple(bad.nonzero()[0].tolist())
    pytest.fail("%s: %d of %d elements differ; first at %s: got %r, reference %r" % (what, int(bad.sum().item()), bad.numel(), list(at), got[at].item(),
                                                                                      want[at].item()))


def _ws(dev, N, H, W, C, dg):
    """The mode's workspace, NaN-filled (the call owns every word it reads)."""
    from dan_amd import _lib
    n = int(_lib.lib().danhip_deform_sample_bwd_ordered_workspace_bytes(N, H, W, C, dg))
    assert n > (N * H * W * C + 64) * 4 and n % 4 == 0
    return torch.full((n // 4,), NAN, dtype=torch.float32, device=dev)


def _sample_bwd(dev, x, off, dS, dx_start, N, H, W, C, dg, accumulate, ws=None):
    from dan_amd import _lib
    dx = dx_start.clone() if accumulate else torch.full_like(x, NAN)
    doff = torch.full_like(off, NAN)
    ws = _ws(dev, N, H, W, C, dg) if ws is None else ws
    _lib.call("danhip_deform_sample_bwd", _lib.ptr(x), _lib.ptr(off), _lib.ptr(dS), _lib.ptr(dx), _lib.ptr(doff), N, H, W, C, 3, 3, 1, 1, dg, accumulate,
              _lib.ptr(ws), ws.numel() * 4, _lib.stream())
    torch.cuda.synchronize()
    return dx, doff


def _far(dev, off, dS, N, H, W, C, dg, window=0):
    """danhip_deform_far_ordered -> far_dx float32 [N,H,W,C] on the host."""
    from dan_amd import _lib
    ws = _ws(dev, N, H, W, C, dg)
    _lib.call("danhip_deform_far_ordered", _lib.ptr(off), _lib.ptr(dS), N, H, W, C, dg, window, _lib.ptr(ws), ws.numel() * 4, _lib.stream())
    torch.cuda.synchronize()
    return ws[: N * H * W * C].cpu().numpy().reshape(N, H, W, C)


# ================================================================================================================ 1 every term once
@pytest.mark.parametrize("name", OC.EXACT_NAMES)
def test_every_term_once_on_the_dyadic_cases(name, mode, dev):
    """dX and dOffset equal the float64 reference bit for bit in the mode: window by the statistic and both pinned windows, = and +=."""
    from dan_amd import _lib, ops
    c = DE.CASE_BY_NAME[name]
    d = DE.check_case(c)
    xd, od, sd, x0 = (t.to(ops.ACT).to(dev) for t in (d.x, d.off, d.dS, d.dx0))
    try:
        for form in (0, 1, 3):
            _lib.lib().danhip_set_option(b"deform_bwd_form", form)
            for acc in (0, 1):
                dx, doff = _sample_bwd(dev, xd, od, sd, x0, c.N, c.H, c.W, c.C, c.dg, acc)
                what = "form %d, accumulate %d" % (form, acc)
                _same(doff, d.doff, "dOffset, " + what)
                _same(dx, d.dx + d.dx0 if acc else d.dx, "dX, " + what)
    finally:
        _lib.lib().danhip_set_option(b"deform_bwd_form", 0)


@pytest.mark.parametrize("name", DE.CONV_CASES)
def test_convolution_backward_through_ops_in_the_mode(name, mode, dev):
    """ops.deform_conv forward and backward inside the context: y, dX, dOffset and dW equal the float64 reference."""
    from dan_amd import ops
    c = DE.CASE_BY_NAME[name]
    d = DE.check_case(c)
    cv = DE.check_conv(name)
    x = d.x.to(ops.ACT).to(dev).requires_grad_(True)
    o = d.off.to(ops.ACT).to(dev).requires_grad_(True)
    w = DE.filter_hwio(cv.w).float().to(dev).requires_grad_(True)
    y = ops.deform_conv(x, w, cv.bias.float().to(dev), o, 3, 3, deformable_group=c.dg, relu=False)
    y.backward(cv.dy.to(ops.ACT).to(dev))
    torch.cuda.synchronize()
    _same(y, cv.y, "y")
    _same(x.grad, cv.dx, "dX")
    _same(o.grad, cv.doff, "dOffset")
    _same(w.grad, DE.filter_hwio(cv.dw), "dW")


# ================================================================================================================ 2 the order
@pytest.mark.parametrize("L", OC.ORDER_L)
def test_far_sums_are_formed_in_key_order(L, mode, dev):
    from dan_amd import ops
    case = OC.order_case(L)
    want = OC.order_expected(case, ops.ACT)
    assert case.shared, "no two destinations share a source pixel"
    assert len(case.records[OC.DESTS[0] + (0,)]) == L
    if L >= 7:          # (on the CPU, before the device is looked at: the case must tell the orders apart in the 16-bit output)
        assert not torch.equal(want.view(torch.int16), OC.order_expected(case, ops.ACT, descending=True).view(torch.int16))
    N, H, W, C, dg = 1, OC.OH, OC.OW, OC.OC, OC.ODG
    x = DE.gen_x(N, H, W, C, 31).to(ops.ACT).to(dev)
    od, sd = torch.from_numpy(case.off).to(ops.ACT).to(dev), torch.from_numpy(case.dS).to(ops.ACT).to(dev)
    for acc in (0, 1):
        dx0 = torch.zeros_like(x)
        dx, doff = _sample_bwd(dev, x, od, sd, dx0, N, H, W, C, dg, acc)
        assert torch.equal(dx.cpu().view(torch.int16), want.view(torch.int16).reshape(dx.shape)), "accumulate %d: %d elements differ" % (
            acc, int((dx.cpu().view(torch.int16) != want.view(torch.int16).reshape(dx.shape)).sum()))
        assert torch.isfinite(doff.float()).all()


# ================================================================================================================ 3 kernels = emulation
@pytest.mark.parametrize("name", OC.EXACT_NAMES)
def test_device_far_dx_equals_the_emulation_on_the_dyadic_cases(name, dev):
    from dan_amd import ops
    c = DE.CASE_BY_NAME[name]
    d = DE.data(name)
    o16, s16 = d.off.to(ops.ACT).contiguous(), d.dS.to(ops.ACT).contiguous()
    od, sd = o16.to(dev), s16.to(dev)
    for window in (0, 1, 2):
        want, records, errors = OC.emulate16(o16, s16, c.N, c.H, c.W, c.C, c.dg, window)
        assert errors == 0 and records > 0
        a = _far(dev, od, sd, c.N, c.H, c.W, c.C, c.dg, window)
        b = _far(dev, od, sd, c.N, c.H, c.W, c.C, c.dg, window)
        assert a.tobytes() == want.tobytes(), "window %d: %d elements differ" % (window, int((a != want).sum()))
        assert a.tobytes() == b.tobytes()


@pytest.mark.parametrize("L", OC.ORDER_L)
def test_device_far_dx_equals_the_emulation_on_the_order_cases(L, dev):
    from dan_amd import ops
    case = OC.order_case(L)
    N, H, W, C, dg = 1, OC.OH, OC.OW, OC.OC, OC.ODG
    o16, s16 = torch.from_numpy(case.off).to(ops.ACT).contiguous(), torch.from_numpy(case.dS).to(ops.ACT).contiguous()
    want, records, errors = OC.emulate16(o16, s16, N, H, W, C, dg)
    assert errors == 0 and records == sum(len(r) for r in case.records.values())
    assert want.tobytes() == OC.order_far_dx(case).tobytes()
    a = _far(dev, o16.to(dev), s16.to(dev), N, H, W, C, dg)
    b = _far(dev, o16.to(dev), s16.to(dev), N, H, W, C, dg)
    assert a.tobytes() == want.tobytes(), "%d elements differ" % int((a != want).sum())
    assert a.tobytes() == b.tobytes()


def test_prefix_sum_over_more_than_256_workgroups(dev):
    """730 x 730 destinations = 261 workgroups of the prefix sum: the single-workgroup scan of their sums takes its second round.  A few
    records at both ends and in the middle; far_dx equals the emulation everywhere."""
    from dan_amd import ops
    N, H, W, C, dg = 1, 730, 730, 64, 1
    assert (N * H * W * dg + 2047) // 2048 > 256
    rng = np.random.default_rng(5)
    o16 = torch.zeros((N, H, W, 18), dtype=ops.ACT)
    s16 = torch.zeros((N * H * W, 9 * C), dtype=ops.ACT)
    for (dh, dw) in ((0, 0), (3, 3), (365, 365), (729, 728), (728, 700)):
        for _ in range(9):
            sh, sw, t = int(rng.integers(max(0, dh - 100), min(H, dh + 100))), int(rng.integers(max(0, dw - 100), min(W, dw + 100))), int(rng.integers(0, 9))
            oh, ow = dh - (sh - 1 + t // 3), dw - (sw - 1 + t % 3)
            if max(abs(oh), abs(ow)) < 3:
                continue
            o16[0, sh, sw, 2 * t], o16[0, sh, sw, 2 * t + 1] = float(oh), float(ow)
            s16[sh * W + sw, t * C:(t + 1) * C] = torch.from_numpy(OC._values(rng, 1)[0]).to(ops.ACT)
    want, records, errors = OC.emulate16(o16, s16, N, H, W, C, dg)
    assert errors == 0 and records >= 20
    got = _far(dev, o16.to(dev), s16.to(dev), N, H, W, C, dg)
    assert got.tobytes() == want.tobytes(), "%d elements differ" % int((got != want).sum())
    assert np.count_nonzero(want) > 0


# ================================================================================================================ 4 scope
def test_other_shape_classes_are_refused_in_the_mode(mode, dev):
    from dan_amd import _lib, ops

    def call(N, H, W, C, dg, stride, dil):
        Ho, Wo = -(-H // stride), -(-W // stride)
        x = torch.zeros((N, H, W, C), dtype=ops.ACT, device=dev)
        off = torch.zeros((N, Ho, Wo, dg * 18), dtype=ops.ACT, device=dev)
        dS = torch.zeros((N * Ho * Wo, 9 * C), dtype=ops.ACT, device=dev)
        ws = torch.zeros(1 << 20, dtype=torch.float32, device=dev)
        _lib.call("danhip_deform_sample_bwd", _lib.ptr(x), _lib.ptr(off), _lib.ptr(dS), _lib.ptr(torch.empty_like(x)), _lib.ptr(torch.empty_like(off)), N, H, W, C,
                  3, 3, stride, dil, dg, 0, _lib.ptr(ws), ws.numel() * 4, _lib.stream())

    for args in ((1, 8, 16, 64, 1, 2, 1), (1, 8, 16, 64, 1, 1, 2), (1, 8, 16, 64, 2, 1, 1)):          # stride 2, dilation 2, C / dg = 32
        with pytest.raises(_lib.DanhipError, match="no ordered form"):
            call(*args)
    call(1, 8, 16, 64, 1, 1, 1)                                                                     # the shape class itself runs
    torch.cuda.synchronize()
    with pytest.raises(_lib.DanhipError, match="workspace"):                                        # ... and checks its workspace
        x = torch.zeros((1, 8, 16, 64), dtype=ops.ACT, device=dev)
        off = torch.zeros((1, 8, 16, 18), dtype=ops.ACT, device=dev)
        dS = torch.zeros((128, 576), dtype=ops.ACT, device=dev)
        ws = torch.zeros(x.numel() + 64, dtype=torch.float32, device=dev)
        _lib.call("danhip_deform_sample_bwd", _lib.ptr(x), _lib.ptr(off), _lib.ptr(dS), _lib.ptr(torch.empty_like(x)), _lib.ptr(torch.empty_like(off)), 1, 8, 16, 64,
                  3, 3, 1, 1, 1, 0, _lib.ptr(ws), ws.numel() * 4, _lib.stream())


@pytest.mark.parametrize("name", OC.EXACT_NAMES)
def test_default_mode_is_unchanged(name, dev):
    """Option off: the default workspace suffices and dX / dOffset equal the reference, as before."""
    from dan_amd import _lib, ops
    assert _lib.lib().danhip_get_option(b"deterministic") == 0
    c = DE.CASE_BY_NAME[name]
    d = DE.check_case(c)
    xd, od, sd, x0 = (t.to(ops.ACT).to(dev) for t in (d.x, d.off, d.dS, d.dx0))
    for acc in (0, 1):
        ws = torch.full((xd.numel() + 64,), NAN, dtype=torch.float32, device=dev)
        dx, doff = _sample_bwd(dev, xd, od, sd, x0, c.N, c.H, c.W, c.C, c.dg, acc, ws=ws)
        _same(doff, d.doff, "dOffset")
        _same(dx, d.dx + d.dx0 if acc else d.dx, "dX")
