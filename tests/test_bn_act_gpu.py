"""The fused batch-norm tails (csrc/bn_act.hip) on the device against tests/bn_act_cases.py: the exact infer form and frozen backward bit for
bit, the training form against float64 by the neighbour rule, the fused bottleneck unit against the float64 oracle unit, and the refusal in
deterministic mode."""
import numpy as np
import pytest
import torch

import bn_act_cases as BC
import resnet_unit as RU

pytestmark = pytest.mark.gpu


def _act():
    from dan_amd import _lib
    return _lib.ACT_NAME, _lib.ACT_DTYPE


def _a16(a, dev):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(_act()[1]).to(dev)


def _f32(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dev)


def _np(t):
    return t.detach().double().cpu().numpy()


def _infer(c, relu, dev):
    from dan_amd._lib import call, ptr, stream
    M, C = c["x"].shape
    x, sc = _a16(c["x"], dev), _a16(c["shortcut"], dev)
    y = torch.full_like(x, float("nan"))
    gamma, beta, mean, rstd = (_f32(c[k], dev) for k in ("gamma", "beta", "mean", "rstd"))      # (named: alive until the call has been issued)
    call("danhip_bn_act_fwd_infer", ptr(x), ptr(sc), ptr(gamma), ptr(beta), ptr(mean), ptr(rstd), ptr(y), M, C, int(relu), stream())
    return y


def _bwd(c, y, mean, rstd, frozen, want_dsc, dev):
    from dan_amd._lib import call, ptr, stream
    M, C = c["x"].shape
    x, dy = _a16(c["x"], dev), _a16(c["dy"], dev)
    dx = torch.full_like(x, float("nan"))
    dsc = torch.full_like(x, float("nan")) if want_dsc else None
    dgamma, dbeta = torch.full((C,), float("nan"), device=dev), torch.full((C,), float("nan"), device=dev)
    gamma = _f32(c["gamma"], dev)
    call("danhip_bn_act_bwd", ptr(x), ptr(dy), ptr(y), ptr(gamma), ptr(mean), ptr(rstd), ptr(dx), ptr(dsc), ptr(dgamma), ptr(dbeta), M, C, int(frozen),
         stream())
    return dx, dsc, dgamma, dbeta


@pytest.mark.parametrize("shortcut", [False, True], ids=["plain", "shortcut"])
@pytest.mark.parametrize("C", BC.EXACT_C)
@pytest.mark.parametrize("M", BC.EXACT_M)
def test_exact_infer_and_frozen_backward(M, C, shortcut, dev):
    """bit for bit: y with and without ReLU (values land exactly on 0), then dx / dshortcut / dgamma / dbeta of the frozen form with the mask
    y > 0 and without one"""
    c = BC.exact_case(M, C, shortcut)
    args = [c[k] for k in ("x", "shortcut", "gamma", "beta", "mean", "rstd")]
    mean, rstd = _f32(c["mean"], dev), _f32(c["rstd"], dev)
    for relu in (False, True):
        y = _infer(c, relu, dev)
        want = BC.fwd(*args, relu)
        assert np.array_equal(_np(y), want), (relu, np.abs(_np(y) - want).max())
        dx, dsc, dgamma, dbeta = _bwd(c, y if relu else None, mean, rstd, True, shortcut, dev)
        wdx, wdsc, wdgamma, wdbeta = BC.bwd(c["x"], c["dy"], want if relu else None, c["gamma"], c["mean"], c["rstd"], True)
        assert np.array_equal(_np(dx), wdx) and (dsc is None or np.array_equal(_np(dsc), wdsc))
        assert np.array_equal(_np(dgamma), wdgamma) and np.array_equal(_np(dbeta), wdbeta)
    # dgamma / dbeta side by side (one clear inside the call) give the same sums
    from dan_amd._lib import call, ptr, stream
    sums = torch.full((2, C), float("nan"), device=dev)
    x, dy, gamma = _a16(c["x"], dev), _a16(c["dy"], dev), _f32(c["gamma"], dev)
    dx = torch.empty_like(x)
    call("danhip_bn_act_bwd", ptr(x), ptr(dy), ptr(y), ptr(gamma), ptr(mean), ptr(rstd), ptr(dx), None, ptr(sums[0]), ptr(sums[1]), M, C, 1, stream())
    assert np.array_equal(_np(sums[0]), wdgamma) and np.array_equal(_np(sums[1]), wdbeta)


@pytest.mark.parametrize("relu,shortcut", [(False, False), (True, False), (False, True), (True, True)], ids=["bn", "bn-relu", "bn-add", "bn-add-relu"])
@pytest.mark.parametrize("M,C", BC.TRAIN_SHAPES)
def test_training_form_against_float64(M, C, relu, shortcut, dev):
    """Statistics against danhip_batchnorm_fwd_train on the same input (atol 1e-6: the tighter of the two absolute tolerances
    tests/test_layers2_gpu.py::test_batch_norm holds the statistics to; they are the same kernels, up to the order of the double atomics),
    moving statistics updated once by the reference's rule (the same test's atol: 1e-5 mean, 1e-6 variance), y and dx against float64 from
    the device's own saved statistics by the neighbour rule (tests/bn_act_cases.py)."""
    from dan_amd._lib import call, ptr, stream
    act = _act()[0]
    c = BC.train_case(M, C, shortcut, act)
    x, sc = _a16(c["x"], dev), _a16(c["shortcut"], dev)
    gamma, beta = _f32(c["gamma"], dev), _f32(c["beta"], dev)
    mm, mv = _f32(c["moving_mean"], dev), _f32(c["moving_var"], dev)
    y = torch.full_like(x, float("nan"))
    mean, rstd = torch.empty(C, device=dev), torch.empty(C, device=dev)
    ws = torch.empty(2 * C, dtype=torch.float64, device=dev)
    call("danhip_bn_act_fwd_train", ptr(x), ptr(sc), ptr(gamma), ptr(beta), ptr(y), ptr(mean), ptr(rstd), ptr(mm), ptr(mv), M, C, BC.EPS, BC.MOMENTUM,
         int(relu), ptr(ws), stream())
    y0, mean0, rstd0 = torch.empty_like(x), torch.empty(C, device=dev), torch.empty(C, device=dev)
    call("danhip_batchnorm_fwd_train", ptr(x), ptr(gamma), ptr(beta), ptr(y0), ptr(mean0), ptr(rstd0), None, None, M, C, BC.EPS, BC.MOMENTUM, 0, ptr(ws),
         stream())
    print("statistics: max |mean - mean0| %.3g, max |rstd - rstd0| %.3g" % ((mean - mean0).abs().max().item(), (rstd - rstd0).abs().max().item()))
    assert torch.allclose(mean, mean0, rtol=0, atol=1e-6) and torch.allclose(rstd, rstd0, rtol=0, atol=1e-6)
    m64, v64, _ = BC.stats(c["x"])
    wmm, wmv = BC.moving(c["moving_mean"], c["moving_var"], m64, v64, M)
    assert np.allclose(_np(mm), wmm, rtol=0, atol=1e-5) and np.allclose(_np(mv), wmv, rtol=0, atol=1e-6)
    dm, dr = _np(mean), _np(rstd)
    want = BC.fwd(c["x"], c["shortcut"], c["gamma"], c["beta"], dm, dr, relu)
    ok = BC.within(_np(y), want, BC.fwd_slack(c["x"], c["shortcut"], c["gamma"], c["beta"], dm, dr), act)
    print("y: %d of %d elements off the rule" % ((~ok).sum(), ok.size))
    assert ok.all()
    dx, dsc, dgamma, dbeta = _bwd(c, y if relu else None, mean, rstd, False, shortcut, dev)
    yn = _np(y) if relu else None
    wdx, wdsc, wdgamma, wdbeta = BC.bwd(c["x"], c["dy"], yn, c["gamma"], dm, dr, False)
    ok = BC.within(_np(dx), wdx, BC.bwd_slack(c["x"], c["dy"], yn, c["gamma"], dm, dr), act)
    print("dx: %d of %d elements off the rule" % ((~ok).sum(), ok.size))
    assert ok.all()
    assert dsc is None or np.array_equal(_np(dsc), wdsc)
    # fp32 sums of M addends in any order: within (M - 1) 2^-24 of the sum of magnitudes
    g = wdsc
    xhat = (c["x"] - dm) * dr
    assert np.all(np.abs(_np(dbeta) - wdbeta) <= (M - 1) * 2.0 ** -24 * np.abs(g).sum(axis=0) + 1e-30)
    assert np.all(np.abs(_np(dgamma) - wdgamma) <= (M + 2) * 2.0 ** -24 * np.abs(g * xhat).sum(axis=0) + 1e-30)


def test_ops_are_one_node_with_the_shortcut_gradient(dev):
    """ops.batch_norm_act_train / _infer: one autograd node, the shortcut receives g = dy [y > 0] from it, the moving statistics move in
    training and stay under no_grad."""
    from dan_amd import ops
    act, dt = _act()
    c = BC.train_case(33, 8, True, act)
    mk = lambda k, grad: _a16(c[k], dev).reshape(1, 3, 11, 8).requires_grad_(grad)
    x, sc = mk("x", True), mk("shortcut", True)
    gamma, beta = _f32(c["gamma"], dev).requires_grad_(True), _f32(c["beta"], dev).requires_grad_(True)
    mm, mv = _f32(c["moving_mean"], dev), _f32(c["moving_var"], dev)
    y = ops.batch_norm_act_train(x, gamma, beta, mm, mv, BC.EPS, BC.MOMENTUM, True, shortcut=sc)
    assert type(y.grad_fn).__name__ == "_BatchNormActBackward"
    dy = _a16(c["dy"], dev).reshape(1, 3, 11, 8)
    y.backward(dy)
    m, _, r = BC.stats(c["x"])
    want = BC.fwd(c["x"], c["shortcut"], c["gamma"], c["beta"], m, r, True)
    assert np.abs(_np(y).reshape(33, 8) - want).max() <= 2.0 ** -7 * np.abs(want).max() + 1e-3            # (tests/test_layers2_gpu.py's forward tolerance)
    assert np.array_equal(_np(sc.grad).reshape(33, 8), np.where(_np(y).reshape(33, 8) > 0, c["dy"], 0.0))
    assert x.grad is not None and gamma.grad.shape == (8,) and beta.grad.shape == (8,)
    assert not torch.equal(mm, _f32(c["moving_mean"], dev))
    mm1 = mm.clone()
    with torch.no_grad():
        yi = ops.batch_norm_act_infer(x, gamma, beta, mm, mv, BC.EPS, True, shortcut=sc)
    assert torch.equal(mm, mm1) and yi.shape == x.shape
    wi = BC.fwd(c["x"], c["shortcut"], c["gamma"], c["beta"], _np(mm), 1.0 / np.sqrt(_np(mv) + BC.EPS), True)
    assert np.abs(_np(yi).reshape(33, 8) - wi).max() <= 2.0 ** -7 * np.abs(wi).max()


UNIT_CASES = [("root", False), ("root", True), ("identity", False), ("identity", True)]       # with a projection shortcut, and without


@pytest.mark.parametrize("kind,training", UNIT_CASES, ids=["%s-%s" % (k, "train" if t else "infer") for k, t in UNIT_CASES])
def test_fused_unit_matches_the_oracle(kind, training, dev):
    """ResNetBackbone(50, fused_tail=True).bottleneck_block against the float64 oracle unit at tests/resnet_unit.py's sizes and bound
    (BOUND = 2 r0), as tests/test_resnet_gpu.py holds the unfused unit; variable names and creation order equal the unfused backbone's."""
    from dan_amd.net import resnet_danet
    from dan_amd.net.variables import VariableStore
    cin, filters, need_reduce, is_root = RU.UNITS[kind]
    P, x, dy = RU.make_case(kind, 0)
    ref = RU.oracle_unit(kind, training, P, x, dy)
    names = {}
    for fused in (False, True):
        vs = VariableStore(device=dev)
        net = resnet_danet.ResNetBackbone(50, variables=vs, fused_tail=fused)
        xd = x.to(torch.bfloat16).to(dev).requires_grad_(True)
        with torch.no_grad():
            net.bottleneck_block(xd, filters, RU.SCOPE, training, need_reduce, is_root)
        names[fused] = ([n for n, _ in vs.named()], list(vs.bufs))
    assert names[True] == names[False]
    vs = VariableStore(device=dev)
    vs.load_tf_named({n: P[n] for n in RU.trainable(P)})
    for n, t in P.items():
        if "/moving_" in n:
            vs.buffer(n, t.shape, 0.0).copy_(t.to(dev))
    net = resnet_danet.ResNetBackbone(50, variables=vs, fused_tail=True)
    xd = x.to(torch.bfloat16).to(dev).requires_grad_(True)
    out = net.bottleneck_block(xd, filters, RU.SCOPE, training, need_reduce, is_root)
    assert type(out.grad_fn).__name__ == "_BatchNormActBackward"
    assert set(n for n, _ in vs.named()) | set(vs.bufs) == set(P)
    out.backward(dy.to(torch.bfloat16).to(dev))
    got = {"out": out.detach(), "dx": xd.grad}
    for n, p in vs.named():
        assert p.grad is not None, (n, "received no gradient")
        got[n] = p.grad
    got = {n: v.detach().double().cpu() for n, v in got.items()}
    err = RU.errors(got, ref)
    bound = RU.bound(kind, training)
    print(kind, training, "bound %.4f worst %.4f" % (bound, max(err.values())), {n: round(e, 4) for n, e in err.items()})
    bad = {n: e for n, e in err.items() if not e <= bound}
    assert not bad, (bound, bad)


def test_deterministic_option_refuses(dev):
    from dan_amd import _lib
    L = _lib.lib()
    c = BC.exact_case(7, 8, True)
    x, sc, dy = _a16(c["x"], dev), _a16(c["shortcut"], dev), _a16(c["dy"], dev)
    f = {k: _f32(c[k], dev) for k in ("gamma", "beta", "mean", "rstd")}
    y, dx = torch.empty_like(x), torch.empty_like(x)
    s1, s2 = torch.empty(8, device=dev), torch.empty(8, device=dev)
    ws = torch.empty(16, dtype=torch.float64, device=dev)
    p, st = _lib.ptr, _lib.stream()
    assert L.danhip_set_option(b"deterministic", 1) == 0
    try:
        rcs = [L.danhip_bn_act_fwd_train(p(x), p(sc), p(f["gamma"]), p(f["beta"]), p(y), p(s1), p(s2), None, None, 7, 8, 1e-5, 0.997, 1, p(ws), st),
               L.danhip_bn_act_fwd_infer(p(x), p(sc), p(f["gamma"]), p(f["beta"]), p(f["mean"]), p(f["rstd"]), p(y), 7, 8, 1, st),
               L.danhip_bn_act_bwd(p(x), p(dy), None, p(f["gamma"]), p(f["mean"]), p(f["rstd"]), p(dx), None, p(s1), p(s2), 7, 8, 0, st)]
        msg = L.danhip_last_error().decode()
    finally:
        assert L.danhip_set_option(b"deterministic", 0) == 0
    assert rcs == [-1, -1, -1] and "no deterministic form" in msg and "float atomics" in msg
