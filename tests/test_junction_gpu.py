"""Gradient junction of a tapped backbone map (danhip_l2norm_bwd_pool_scatter): one launch against the two it replaces.

dx must be BIT-IDENTICAL to danhip_l2norm_bwd followed by danhip_maxpool2x2_bwd_arg(accumulate=1) (or, pool_first, the scatter followed by the
L2 norm with accumulate=1): the fused kernel reproduces the 16-bit rounding between the two deliveries.  dgamma is a sum of fp32 atomics
(LDS, then global) in both forms: the order of the adds is not fixed even between two launches of the SAME kernel, and the fused kernel
assigns pixels to lanes by pool window, not by linear pixel index, so block-level summation order cannot be kept.  dgamma is therefore compared
with the tolerance tests/test_ops_gpu.py::test_l2norm uses for it (2e-3 of the largest entry + 1e-4), not with torch.equal."""
import pytest
import torch

pytestmark = pytest.mark.gpu

BENCH_SHAPES = [(16, 160, 160, 256), (16, 80, 80, 512), (16, 40, 40, 512)]
ODD_SHAPE = (1, 37, 53, 64)


def _inputs(shape, dev, seed):
    from dan_amd._lib import call, ptr, stream
    N, H, W, C = shape
    g = torch.Generator(device=dev).manual_seed(seed)
    x = torch.relu(torch.randn(shape, generator=g, device=dev)).to(torch.bfloat16)
    x[0, 0, 0] = 0                                               # all-zero pixels: the ss <= 1e-10 clamp branch ...
    x[-1, H - 1, W - 1] = 0                                      # ... also in the last (for odd sizes: partial) window
    x[0, 2:4, 2:4] = 0                                           # an all-equal window: code 0
    gamma = (10.0 + torch.randn((C,), generator=g, device=dev)).float()
    dy = torch.randn(shape, generator=g, device=dev).to(torch.bfloat16)
    Ho, Wo = (H + 1) // 2, (W + 1) // 2
    pooled = torch.empty((N, Ho, Wo, C), dtype=torch.bfloat16, device=dev)
    arg = torch.empty((N * Ho * Wo, C // 4), dtype=torch.uint8, device=dev)
    call("danhip_maxpool2x2_fwd_arg", ptr(x), ptr(pooled), ptr(arg), N, H, W, C, stream())
    pdy = torch.randn(pooled.shape, generator=g, device=dev).to(torch.bfloat16)
    third = torch.randn(shape, generator=g, device=dev).to(torch.bfloat16)      # a contribution already in the slot (acc = 1)
    dg0 = torch.randn((C,), generator=g, device=dev).float()                     # dgamma is accumulated INTO
    return x, gamma, dy, arg, pdy, third, dg0


@pytest.mark.parametrize("pool_first", [0, 1])
@pytest.mark.parametrize("relu_mask", [0, 1])
@pytest.mark.parametrize("acc", [0, 1])
@pytest.mark.parametrize("shape", BENCH_SHAPES + [ODD_SHAPE])
def test_fused_equals_two_calls(shape, acc, relu_mask, pool_first, dev):
    from dan_amd._lib import call, ptr, stream
    N, H, W, C = shape
    x, gamma, dy, arg, pdy, third, dg0 = _inputs(shape, dev, 3)
    M = N * H * W
    # a fresh slot holds garbage: with acc = 0 neither form may read it (NaN patterns would show)
    fresh = torch.full(shape, float("nan"), dtype=torch.bfloat16, device=dev)
    want = (third if acc else fresh).clone()
    dg_want = dg0.clone()
    if pool_first:
        call("danhip_maxpool2x2_bwd_arg", ptr(arg), ptr(pdy), ptr(want), N, H, W, C, acc, stream())
        call("danhip_l2norm_bwd", ptr(x), ptr(gamma), ptr(dy), ptr(want), ptr(dg_want), M, C, 1, relu_mask, stream())
    else:
        call("danhip_l2norm_bwd", ptr(x), ptr(gamma), ptr(dy), ptr(want), ptr(dg_want), M, C, acc, relu_mask, stream())
        call("danhip_maxpool2x2_bwd_arg", ptr(arg), ptr(pdy), ptr(want), N, H, W, C, 1, stream())
    got = (third if acc else fresh).clone()
    dg_got = dg0.clone()
    call("danhip_l2norm_bwd_pool_scatter", ptr(x), ptr(gamma), ptr(dy), ptr(arg), ptr(pdy), ptr(got), ptr(dg_got), N, H, W, C, acc, relu_mask,
         pool_first, stream())
    torch.cuda.synchronize()
    assert not torch.isnan(want.float()).any()
    assert torch.equal(got.view(torch.int16), want.view(torch.int16)), (
        "dx differs in %d of %d elements" % ((got.view(torch.int16) != want.view(torch.int16)).sum().item(), got.numel()))
    ref = dg_want - dg0
    err = ((dg_got - dg0) - ref).abs().max().item()
    print("dgamma: max |fused - two calls| = %.3e, max |two calls| = %.3e" % (err, ref.abs().max().item()))
    assert err <= 2e-3 * ref.abs().max().item() + 1e-4


def test_unsupported_channels_are_refused(dev):
    from dan_amd import _lib
    t = torch.zeros((1, 2, 2, 1024), dtype=torch.bfloat16, device=dev)
    f = torch.zeros((1024,), device=dev)
    a = torch.zeros((1, 256), dtype=torch.uint8, device=dev)
    p = _lib.ptr
    rc = _lib.lib().danhip_l2norm_bwd_pool_scatter(p(t), p(f), p(t), p(a), p(t), p(t), p(f), 1, 2, 2, 1024, 0, 0, 0, _lib.stream())
    assert rc != 0 and b"unsupported" in _lib.lib().danhip_last_error()


def _graph(dev, l2_before_pool, use_junction, extra_consumer, monkeypatch, sink=False):
    """conv (ReLU) -> {L2 norm -> conv, 2 x 2 pool -> conv [, a third conv]}: every gradient of the tapped map travels through its slot."""
    from dan_amd import ops
    calls = []
    real = ops.call

    def spy(name, *a):
        calls.append(name)
        return real(name, *a)

    monkeypatch.setattr(ops, "call", spy)
    g = torch.Generator().manual_seed(11)
    x = torch.randn((2, 13, 18, 64), generator=g).to(torch.bfloat16).to(dev).requires_grad_(True)
    ws = [(torch.randn((3, 3, 64, 64), generator=g) * 0.05).to(dev).requires_grad_(True) for _ in range(4)]
    gamma = torch.nn.Parameter((10.0 + torch.randn((64,), generator=g)).to(dev))
    if sink:                                                     # a trainer's flat gradient buffer: dgamma is accumulated in place
        gamma._danhip_grad = torch.zeros((64,), device=dev)
    with ops.use_context(ops.OpsContext(USE_JUNCTION=use_junction, USE_SPLITK=False, WGRAD_STREAM=False)):
        y = ops.conv2d(x, ws[0], None, relu=True)
        if l2_before_pool:                                       # autograd runs the later-created node first
            a = ops.l2_normalize(y, gamma)
            b = ops.max_pool_2x2(y)
        else:
            b = ops.max_pool_2x2(y)
            a = ops.l2_normalize(y, gamma)
        outs = [ops.conv2d(a, ws[1], None, relu=False, out_f32=True), ops.conv2d(b, ws[2], None, relu=False, out_f32=True)]
        if extra_consumer:
            outs.append(ops.conv2d(y, ws[3], None, relu=False, out_f32=True))
        gens = [torch.randn(o.shape, generator=g).to(dev) for o in outs]
        torch.autograd.backward(outs, gens)
    torch.cuda.synchronize()
    monkeypatch.setattr(ops, "call", real)
    return x.grad, (gamma._danhip_grad if sink else gamma.grad), [w.grad for w in ws[:len(outs) + 1]], calls


@pytest.mark.parametrize("sink", [False, True])
@pytest.mark.parametrize("extra_consumer", [False, True])
@pytest.mark.parametrize("l2_before_pool", [False, True])
def test_graph_junction_equals_two_launches(l2_before_pool, extra_consumer, sink, dev, monkeypatch):
    """Whichever of the two backward nodes runs second issues the fused call; a third consumer of the map keeps its place in the order of
    the roundings, so the input gradient of the producing convolution is bit-identical.  The L2 norm may only wait for the pool when its
    dgamma goes to a gradient sink (a tensor returned to autograd must be complete): without one, that order keeps the two launches."""
    dx0, dg0, dw0, calls0 = _graph(dev, l2_before_pool, False, extra_consumer, monkeypatch, sink)
    dx1, dg1, dw1, calls1 = _graph(dev, l2_before_pool, True, extra_consumer, monkeypatch, sink)
    assert calls0.count("danhip_l2norm_bwd") == 1 and calls0.count("danhip_maxpool2x2_bwd_arg") == 1
    assert "danhip_l2norm_bwd_pool_scatter" not in calls0
    fused = calls1.count("danhip_l2norm_bwd_pool_scatter")
    alone = (calls1.count("danhip_l2norm_bwd"), calls1.count("danhip_maxpool2x2_bwd_arg"))
    l2_runs_first = not l2_before_pool                           # autograd runs the later-created node first
    assert (fused, alone) == ((0, (1, 1)) if (l2_runs_first and not sink) else (1, (0, 0))), (fused, alone)
    assert torch.equal(dx0.view(torch.int16), dx1.view(torch.int16))
    assert torch.equal(dw0[0], dw1[0])
    assert dg0.abs().max().item() > 0
    assert (dg0 - dg1).abs().max().item() <= 2e-3 * dg0.abs().max().item() + 1e-4


def test_single_contribution_runs_the_existing_call(dev, monkeypatch):
    """A map with an L2 norm but no pool (and the reverse) never waits for a partner."""
    from dan_amd import ops
    calls = []
    real = ops.call
    monkeypatch.setattr(ops, "call", lambda name, *a: (calls.append(name), real(name, *a))[1])
    g = torch.Generator().manual_seed(5)
    x = torch.randn((1, 8, 8, 64), generator=g).to(torch.bfloat16).to(dev).requires_grad_(True)
    w = [(torch.randn((3, 3, 64, 64), generator=g) * 0.05).to(dev).requires_grad_(True) for _ in range(2)]
    gamma = torch.full((64,), 10.0, device=dev, requires_grad=True)
    y = ops.conv2d(x, w[0], None, relu=True)
    out = ops.conv2d(ops.l2_normalize(y, gamma), w[1], None, relu=False, out_f32=True)
    out.backward(torch.ones_like(out))
    torch.cuda.synchronize()
    assert calls.count("danhip_l2norm_bwd") == 1 and "danhip_l2norm_bwd_pool_scatter" not in calls
    assert torch.isfinite(x.grad.float()).all() and x.grad.float().abs().max().item() > 0
