"""Deterministic mode (option "deterministic", OpsContext.deterministic, SFDTrainer(deterministic=True)) on the device.

(a) danhip_ordered_reduce_f32 against a numpy float32 loop in the documented order (include/danhip.h), on partials built so that the
    order changes the answer: exact equality.
(b)-(d) every site that ends in float atomics by default: bit-equal over 8 runs with another stream keeping the chip busy, += semantics,
    agreement with default mode and with a float64 reference at the tolerances the existing tests of those kernels use:
      tests/test_conv_gpu.py:560   (dw_s - dw_a).abs().max() <= 1e-4 * scale + 1e-5           slab form against atomic form (db: :561)
      tests/test_conv_gpu.py:106   err <= 2.0 ** -6 * scale + 2e-3                             weight gradient against the reference
      tests/test_conv_gpu.py:844   err <= 1e-3 * scale + 2e-6 * N * H * W ** 0.5               the first layer's kernel
      tests/test_ops_gpu.py:57     err <= 2e-3 * max + 1e-4                                    dgamma
(e) the whole step: two trainers from one seed hold the same bits after 3 steps - S3FD, and PyramidBox and DAN at the sizes of
    tests/test_train_models_gpu.py (the check that lets those two trainers accept the flag)."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

SEQ_MAX = 64          # DANHIP_ORDERED_REDUCE_SEQ_MAX


@pytest.fixture
def det(dev):
    from dan_amd import _lib
    L = _lib.lib()
    assert L.danhip_set_option(b"deterministic", 1) == 0
    yield L
    L.danhip_set_option(b"deterministic", 0)
    torch.cuda.synchronize()


def _ordered_ref(part, out0):
    """The order contract in numpy float32: sequential for P <= 64, else four contiguous groups of ceil(P / 4) rows, added in group order."""
    P = part.shape[0]

    def seq(rows):
        s = rows[0].copy()
        for r in rows[1:]:
            s = (s + r).astype(np.float32)
        return s

    if P <= SEQ_MAX:
        s = seq(part)
    else:
        G = -(-P // 4)
        gs = [seq(part[k * G:min(P, (k + 1) * G)]) for k in range(4)]
        s = (((gs[0] + gs[1]).astype(np.float32) + gs[2]).astype(np.float32) + gs[3]).astype(np.float32)
    return s if out0 is None else (out0 + s).astype(np.float32)


_PARTS = {}


def _partials(P, C):
    if (P, C) not in _PARTS:
        rng = np.random.RandomState(P * 131 + C)
        a = (rng.standard_normal((P, C)) * np.exp2(rng.uniform(-20, 20, (P, C)))).astype(np.float32)
        cyc = np.array([1e8, 1.0, -1e8, 1.0, 3e-1], dtype=np.float32)
        a[:, ::3] = cyc[(np.arange(P)[:, None] + np.arange(a[:, ::3].shape[1])[None, :]) % 5]      # cancellation: any other order shows
        _PARTS[(P, C)] = a
    return _PARTS[(P, C)]


@pytest.mark.parametrize("accumulate", [0, 1])
@pytest.mark.parametrize("C", [4, 68, 9 * 64 * 64, 7])
@pytest.mark.parametrize("P", [1, 2, 5, SEQ_MAX - 1, SEQ_MAX, SEQ_MAX + 1, 1000])
def test_ordered_reduce_keeps_the_documented_order(P, C, accumulate, dev):
    from dan_amd._lib import call, ptr, stream
    part = _partials(P, C)
    out0 = np.linspace(-3, 3, C).astype(np.float32)
    out = torch.from_numpy(out0.copy()).to(dev)
    call("danhip_ordered_reduce_f32", ptr(torch.from_numpy(part).to(dev)), P, C, ptr(out), accumulate, stream())
    want = _ordered_ref(part, out0 if accumulate else None)
    assert np.array_equal(out.cpu().numpy(), want)
    if P > 2:                                                  # the partials do tell orders apart
        assert not np.array_equal(_ordered_ref(part[::-1], None), _ordered_ref(part, None))


# ---- (b) weight gradient, per kernel family.  Shapes: the smallest at which >= 2 workgroups add into one element and an edge is ragged.
WGRAD = [
    ((2, 48, 40, 64, 128, 3, 3, 1), 64, b"conv_wgrad_rows_kernel<128>"),          # 40 wide: a strip of 32 columns + a ragged one of 8
    ((2, 48, 48, 128, 64, 1, 1, 1), 128, b"conv_wgrad_pw_kernel"),                # (the pointwise kernel takes Cin >= 128)
    # generic tiles: 18 wide is below the row-streaming kernel's 0.6 strip use.  A split takes at least 8 K tiles of 64 output pixels and two
    # addends commute, so the order shows from three splits on: 17 tiles (1044 and 1058 pixels here, the last tile ragged)
    ((2, 29, 18, 256, 16, 3, 3, 1), 256, b"conv_wgrad_kernel<128, 64, 2>"),
    ((2, 46, 46, 256, 512, 3, 3, 2), 256, b"conv_wgrad_kernel<128, 128, 2>"),
    ((2, 64, 128, 8, 64, 3, 3, 1), 3, b"conv_wgrad_c8_kernel"),
]


def _wgrad_case(shape, cin_real, dev):
    from dan_amd import ops
    N, H, W, Cin, Cout, kh, kw, s = shape
    g = torch.Generator().manual_seed(31)
    x = torch.zeros((N, H, W, Cin))
    x[..., :cin_real] = torch.randn((N, H, W, cin_real), generator=g)
    x = x.to(ops.ACT)
    d = ops._desc(*shape)
    dy = torch.randn((N, d.Ho, d.Wo, Cout), generator=g).to(ops.ACT)
    w = torch.zeros((kh, kw, cin_real, Cout), dtype=torch.float64, requires_grad=True)
    b = torch.zeros((Cout,), dtype=torch.float64, requires_grad=True)
    from oracle import tf_ops as T
    y = T.conv2d_same(x[..., :cin_real].double(), w, b, stride=s)
    (y * dy.double()).sum().backward()
    return d, x.to(dev), dy.to(dev), w.grad, b.grad


@pytest.mark.parametrize("shape,cin_real,label", WGRAD, ids=["rows", "pointwise", "generic", "generic_s2", "c8"])
def test_weight_gradient_sites(shape, cin_real, label, det, dev):
    from dan_amd import ops
    from dan_amd._lib import call, ptr, stream
    L = det
    N, H, W, Cin, Cout, kh, kw, s = shape
    d, x, dy, dw64, db64 = _wgrad_case(shape, cin_real, dev)
    assert L.danhip_conv_wgrad_kernel_label(ctypes.byref(d)) == label
    nws = L.danhip_conv2d_bwd_weight_workspace_bytes(ctypes.byref(d))
    assert nws > 0
    dshape = (kh, kw, cin_real, Cout)
    # noise on a side stream: forward convolutions of another layer (tests/test_conv_gpu.py:629-647)
    nd = ops._desc(2, 64, 64, 64, 64, 3, 3, 1)
    nx = torch.randn((2, 64, 64, 64), device=dev).to(ops.ACT)
    nwf, _ = ops.pack_conv_weight(nd, torch.randn((3, 3, 64, 64), device=dev) / 24, need_bwd=False)
    nb, ny = torch.zeros(64, device=dev), torch.empty((2, 64, 64, 64), dtype=ops.ACT, device=dev)
    side = torch.cuda.Stream()

    def run(dw0=None, db0=None):
        dw = torch.zeros(dshape, device=dev) if dw0 is None else dw0.clone()
        db = torch.zeros(Cout, device=dev) if db0 is None else db0.clone()
        ws = torch.full((nws,), 0x7f, dtype=torch.uint8, device=dev)      # garbage in the scratch must not matter
        with torch.cuda.stream(side):
            call("danhip_conv2d_fwd", ctypes.byref(nd), ptr(nx), ptr(nwf), ptr(nb), ptr(ny), 1, 1, None, stream())
        call("danhip_conv2d_bwd_weight_ws", ctypes.byref(d), ptr(x), ptr(dy), ptr(dw), ptr(db), cin_real, ptr(ws), nws, stream())
        torch.cuda.synchronize()
        return dw, db

    S, Sb = run()
    for _ in range(7):
        dw, db = run()
        assert torch.equal(dw, S) and torch.equal(db, Sb)
    g = torch.Generator().manual_seed(5)
    dw0, db0 = torch.randn(dshape, generator=g).to(dev), torch.randn(Cout, generator=g).to(dev)
    dw1, db1 = run(dw0, db0)
    assert torch.equal(dw1, dw0 + S) and torch.equal(db1, db0 + Sb)
    # the plain entry must not fall back to atomics
    dwp, dbp = torch.zeros(dshape, device=dev), torch.zeros(Cout, device=dev)
    assert L.danhip_conv2d_bwd_weight(ctypes.byref(d), ptr(x), ptr(dy), ptr(dwp), ptr(dbp), cin_real, stream()) == -1
    assert b"workspace" in L.danhip_last_error()
    torch.cuda.synchronize()
    assert not dwp.any() and not dbp.any()
    # default mode, same call
    L.danhip_set_option(b"deterministic", 0)
    dwa, dba = torch.zeros(dshape, device=dev), torch.zeros(Cout, device=dev)
    call("danhip_conv2d_bwd_weight", ctypes.byref(d), ptr(x), ptr(dy), ptr(dwa), ptr(dba), cin_real, stream())
    torch.cuda.synchronize()
    L.danhip_set_option(b"deterministic", 1)
    scale, sb = dw64.abs().max().item(), db64.abs().max().item()
    err_a, err_ab = (S - dwa).abs().max().item(), (Sb - dba).abs().max().item()
    err_r, err_rb = (S.cpu().double() - dw64).abs().max().item(), (Sb.cpu().double() - db64).abs().max().item()
    print("dW: |det - default| %.3e, |det - f64| %.3e, scale %.3e; db: %.3e, %.3e, scale %.3e" % (err_a, err_r, scale, err_ab, err_rb, sb))
    assert err_a <= 1e-4 * scale + 1e-5 and err_ab <= 1e-4 * dba.abs().max().item() + 1e-5
    if label == b"conv_wgrad_c8_kernel":
        assert err_r <= 1e-3 * scale + 2e-6 * N * H * W ** 0.5 and err_rb <= 1e-3 * sb + 2e-6 * N * H * W ** 0.5
    else:
        assert err_r <= 2.0 ** -6 * scale + 2e-3 and err_rb <= 2.0 ** -6 * sb + 2e-3


# ---- (c) the L2-norm backward pair and relu_bwd_bias_grad
def _l2_inputs(shape, dev):
    from dan_amd._lib import call, ptr, stream
    N, H, W, C = shape
    g = torch.Generator(device=dev).manual_seed(3)
    x = torch.relu(torch.randn(shape, generator=g, device=dev)).to(torch.bfloat16)
    x[0, 0, 0] = 0
    gamma = (10.0 + torch.randn((C,), generator=g, device=dev)).float()
    dy = torch.randn(shape, generator=g, device=dev).to(torch.bfloat16)
    Ho, Wo = (H + 1) // 2, (W + 1) // 2
    pooled = torch.empty((N, Ho, Wo, C), dtype=torch.bfloat16, device=dev)
    arg = torch.empty((N * Ho * Wo, C // 4), dtype=torch.uint8, device=dev)
    call("danhip_maxpool2x2_fwd_arg", ptr(x), ptr(pooled), ptr(arg), N, H, W, C, stream())
    pdy = torch.randn(pooled.shape, generator=g, device=dev).to(torch.bfloat16)
    third = torch.randn(shape, generator=g, device=dev).to(torch.bfloat16)
    dg0 = torch.randn((C,), generator=g, device=dev).float()
    return x, gamma, dy, arg, pdy, third, dg0


@pytest.mark.parametrize("fused,pool_first", [(0, 0), (1, 0), (1, 1)], ids=["l2norm_bwd", "junction", "junction_pool_first"])
@pytest.mark.parametrize("acc,relu_mask", [(0, 0), (1, 1)])
@pytest.mark.parametrize("shape", [(2, 24, 24, 256), (3, 10, 14, 512)])
def test_l2norm_backward_sites(shape, acc, relu_mask, fused, pool_first, det, dev):
    from dan_amd._lib import call, ptr, stream
    L = det
    N, H, W, C = shape
    M = N * H * W
    x, gamma, dy, arg, pdy, third, dg0 = _l2_inputs(shape, dev)
    nws = L.danhip_reduce_workspace_bytes(M, C)

    def run(ws_form):
        dx = (third if acc else torch.full(shape, float("nan"), dtype=torch.bfloat16, device=dev)).clone()
        dg = dg0.clone()
        ws = torch.full((nws,), 0x7f, dtype=torch.uint8, device=dev)
        tail = (ptr(ws), nws, stream()) if ws_form else (stream(),)
        if fused:
            call("danhip_l2norm_bwd_pool_scatter" + ("_ws" if ws_form else ""), ptr(x), ptr(gamma), ptr(dy), ptr(arg), ptr(pdy), ptr(dx), ptr(dg), N, H, W, C,
                 acc, relu_mask, pool_first, *tail)
        else:
            call("danhip_l2norm_bwd" + ("_ws" if ws_form else ""), ptr(x), ptr(gamma), ptr(dy), ptr(dx), ptr(dg), M, C, acc, relu_mask, *tail)
        torch.cuda.synchronize()
        return dx, dg

    dx, dg = run(True)
    for _ in range(7):
        dx1, dg1 = run(True)
        assert torch.equal(dg1, dg) and torch.equal(dx1.view(torch.int16), dx.view(torch.int16))
    # the plain entry is refused; default mode gives the same dx bits and dgamma within the bound of tests/test_ops_gpu.py:57
    dgp, dxp = dg0.clone(), third.clone()
    if fused:
        rc = L.danhip_l2norm_bwd_pool_scatter(ptr(x), ptr(gamma), ptr(dy), ptr(arg), ptr(pdy), ptr(dxp), ptr(dgp), N, H, W, C, acc, relu_mask, pool_first, stream())
    else:
        rc = L.danhip_l2norm_bwd(ptr(x), ptr(gamma), ptr(dy), ptr(dxp), ptr(dgp), M, C, acc, relu_mask, stream())
    assert rc == -1 and b"_ws" in L.danhip_last_error()
    L.danhip_set_option(b"deterministic", 0)
    dxa, dga = run(False)
    L.danhip_set_option(b"deterministic", 1)
    assert torch.equal(dx.view(torch.int16), dxa.view(torch.int16))
    ref = dga - dg0
    err = ((dg - dg0) - ref).abs().max().item()
    print("dgamma: |det - default| %.3e of %.3e" % (err, ref.abs().max().item()))
    assert err <= 2e-3 * ref.abs().max().item() + 1e-4


def test_relu_bwd_bias_grad_site(det, dev):
    from dan_amd._lib import call, ptr, stream
    L = det
    M, C = 5000, 72
    g = torch.Generator(device=dev).manual_seed(9)
    dy0 = torch.randn((M, C), generator=g, device=dev).to(torch.bfloat16)
    y = torch.randn((M, C), generator=g, device=dev).to(torch.bfloat16)
    db0 = torch.randn((C,), generator=g, device=dev)
    nws = L.danhip_reduce_workspace_bytes(M, C)

    def run(ws_form):
        dy, db = dy0.clone(), db0.clone()
        ws = torch.full((nws,), 0x7f, dtype=torch.uint8, device=dev)
        if ws_form:
            call("danhip_relu_bwd_bias_grad_ws", ptr(dy), ptr(y), ptr(db), M, C, ptr(ws), nws, stream())
        else:
            call("danhip_relu_bwd_bias_grad", ptr(dy), ptr(y), ptr(db), M, C, stream())
        torch.cuda.synchronize()
        return dy, db

    dy, db = run(True)
    for _ in range(7):
        dy1, db1 = run(True)
        assert torch.equal(db1, db) and torch.equal(dy1.view(torch.int16), dy.view(torch.int16))
    assert L.danhip_relu_bwd_bias_grad(ptr(dy0.clone()), ptr(y), ptr(db0.clone()), M, C, stream()) == -1
    assert L.danhip_relu_bwd_bias_grad(ptr(dy0.clone()), ptr(y), None, M, C, stream()) == 0      # no sum, nothing to order
    L.danhip_set_option(b"deterministic", 0)
    dya, dba = run(False)
    L.danhip_set_option(b"deterministic", 1)
    assert torch.equal(dy.view(torch.int16), dya.view(torch.int16))
    want = (dy0.float() * (y.float() > 0)).double().sum(0)
    assert ((db - db0).double() - want).abs().max().item() <= 2e-3 * want.abs().max().item() + 1e-4
    assert (db - dba).abs().max().item() <= 2e-3 * want.abs().max().item() + 1e-4


# ---- (d) loss sums and the optimizer's L2 term
def test_detection_loss_sums(det, dev):
    from dan_amd._lib import call, ptr, stream
    L = det
    B, A = 2, 4000
    g = torch.Generator(device=dev).manual_seed(4)
    cls = torch.randn((B, A, 2), generator=g, device=dev)
    loc, loc_t = torch.randn((B, A, 4), generator=g, device=dev), torch.randn((B, A, 4), generator=g, device=dev)
    labels = torch.zeros((B, A), dtype=torch.int32, device=dev)
    labels.view(-1)[torch.randperm(B * A, generator=g, device=dev)[:30]] = 1
    labels.view(-1)[torch.randperm(B * A, generator=g, device=dev)[:200]] -= 1          # some ignored anchors (and a few positives back to 0)
    score = torch.empty((B, A), device=dev)
    counts, k = torch.empty((B, 2), dtype=torch.int32, device=dev), torch.empty((B,), dtype=torch.int32, device=dev)
    thr = torch.empty((B,), device=dev)
    call("danhip_hard_neg_select", ptr(cls), ptr(labels), ptr(score), ptr(counts), ptr(thr), ptr(k), B, A, 3.0, 0, stream())
    ws = torch.full((2048,), 0x7f, dtype=torch.uint8, device=dev)

    def run(ws_form):
        sel, acc = torch.empty((B, A), dtype=torch.uint8, device=dev), torch.full((4,), float("nan"), device=dev)
        if ws_form:
            call("danhip_detection_loss_fwd_ws", ptr(cls), ptr(loc), ptr(labels), ptr(loc_t), ptr(score), ptr(thr), ptr(sel), ptr(acc), B, A, ptr(ws), 2048, stream())
        else:
            call("danhip_detection_loss_fwd", ptr(cls), ptr(loc), ptr(labels), ptr(loc_t), ptr(score), ptr(thr), ptr(sel), ptr(acc), B, A, stream())
        torch.cuda.synchronize()
        return acc

    acc = run(True)
    assert 10 <= acc[3].item() <= 30
    for _ in range(7):
        assert torch.equal(run(True), acc)
    sel = torch.empty((B, A), dtype=torch.uint8, device=dev)
    assert L.danhip_detection_loss_fwd(ptr(cls), ptr(loc), ptr(labels), ptr(loc_t), ptr(score), ptr(thr), ptr(sel), ptr(acc.clone()), B, A, stream()) == -1
    L.danhip_set_option(b"deterministic", 0)
    acca = run(False)
    L.danhip_set_option(b"deterministic", 1)
    assert ((acc - acca).abs() <= 1e-6 * acca.abs()).all(), (acc, acca)


def test_optimizer_l2_term(det, dev):
    from dan_amd._lib import call, ptr, stream
    L = det
    total = 100032                                             # three segments on 64-element boundaries
    seg = torch.tensor([0, 40000, 40064, total], dtype=torch.int64, device=dev)
    g = torch.Generator(device=dev).manual_seed(6)
    w0, gr, v0 = (torch.randn((total,), generator=g, device=dev) for _ in range(3))
    gm, wd = torch.tensor([1.0, 2.0, 1.0], device=dev), torch.tensor([5e-4, 0.0, 1e-4], device=dev)
    ws = torch.full((16640,), 0x7f, dtype=torch.uint8, device=dev)

    def run(ws_form):
        w, v, l2 = w0.clone(), v0.clone(), torch.full((1,), 0.25, device=dev)
        args = (ptr(w), ptr(gr), ptr(v), ptr(seg), ptr(gm), ptr(wd), 3, total, 1e-3, 0.9, 1.0, ptr(l2))
        if ws_form:
            call("danhip_sgd_momentum_flat_ws", *args, ptr(ws), 16640, stream())
        else:
            call("danhip_sgd_momentum_flat", *args, stream())
        torch.cuda.synchronize()
        return w, v, l2

    w, v, l2 = run(True)
    for _ in range(7):
        w1, v1, l21 = run(True)
        assert torch.equal(l21, l2) and torch.equal(w1, w) and torch.equal(v1, v)
    assert L.danhip_sgd_momentum_flat(ptr(w0.clone()), ptr(gr), ptr(v0.clone()), ptr(seg), ptr(gm), ptr(wd), 3, total, 1e-3, 0.9, 1.0, ptr(l2.clone()), stream()) == -1
    L.danhip_set_option(b"deterministic", 0)
    wa, va, l2a = run(False)
    L.danhip_set_option(b"deterministic", 1)
    assert torch.equal(w, wa) and torch.equal(v, va)           # elementwise: the mode does not touch them
    want = 0.25 + (0.5 * 5e-4 * w0[:40000].double().pow(2).sum() + 0.5 * 1e-4 * w0[40064:].double().pow(2).sum()).item()
    assert abs(l2.item() - want) <= 1e-5 * want and abs(l2a.item() - want) <= 1e-5 * want


# ---- (e) the whole step
def _sfd_run(dev, steps, deterministic):
    from dan_amd import synthetic
    from dan_amd.train_sfd import AnchorConfig, SFDModel, SFDTrainer
    B, S = 2, 128
    model = SFDModel(device=dev, seed=11)
    tr = SFDTrainer(model, deterministic=deterministic)
    imgs = synthetic.make_images(B, S, S, dev, seed=17)
    loc_t, cls_t, _ = AnchorConfig(S, S, dev).encode_batch(synthetic.make_gt_boxes(B, S, S, seed=5, max_faces=6))
    w0, w1 = tr.flat.w.clone(), None
    accs = []
    for _ in range(steps):
        terms = tr.train_step(imgs, loc_t, cls_t)
        accs.append(torch.cat([terms[0][2].clone(), tr.flat.l2.clone()]))
        w1 = tr.flat.w.clone() if w1 is None else w1
    torch.cuda.synchronize()
    return tr, w0, w1, accs


def test_sfd_step_is_bit_reproducible(dev):
    from dan_amd import _lib, ops
    a, w0, w1, la = _sfd_run(dev, 3, True)
    b, _, _, lb = _sfd_run(dev, 3, True)
    assert a.ops_ctx.deterministic and not ops.context().deterministic and _lib.lib().danhip_get_option(b"deterministic") == 0
    assert torch.equal(a.flat.w, b.flat.w) and torch.equal(a.flat.v, b.flat.v)
    for x, y in zip(la, lb):
        assert torch.equal(x, y)
    assert not torch.equal(a.flat.w, w0)
    # one step against default mode: the movement of every variable agrees within the 20-step trajectory test's bound
    # (tests/test_parity_hardening_gpu.py:130: |d_hip - d_ref| <= 0.25 |d_ref|), and so does the whole model's
    d0, _, _, _ = _sfd_run(dev, 1, False)
    md, m0 = w1 - w0, d0.flat.w - w0
    assert (md - m0).norm().item() <= 0.25 * m0.norm().item()
    starts = d0.flat.starts + [d0.flat.total]
    for n, s, e in zip(d0.flat.names, starts[:-1], starts[1:]):
        assert (md[s:e] - m0[s:e]).norm().item() <= 0.25 * m0[s:e].norm().item() + 1e-12, n


def _two_trainers(make, steps=3):
    """-> the two trainers after `steps` deterministic steps each, with their loss terms per step"""
    out = []
    for _ in range(2):
        tr, step = make()
        accs = []
        for _ in range(steps):
            terms = step(tr)
            accs.append(torch.cat([t[2].clone() for t in terms] + [tr.flat.l2.clone()]))
        torch.cuda.synchronize()
        out.append((tr, accs))
    return out


def _assert_same_bits(runs):
    (a, la), (b, lb) = runs
    assert a.ops_ctx.deterministic
    assert torch.equal(a.flat.w, b.flat.w), "%d weights differ" % (a.flat.w != b.flat.w).sum().item()
    assert torch.equal(a.flat.v, b.flat.v)
    for k, (x, y) in enumerate(zip(la, lb)):
        assert torch.equal(x, y), (k, x, y)
    assert torch.isfinite(a.flat.w).all() and a.flat.v.abs().max().item() > 0


def test_pyramidbox_step_is_bit_reproducible(dev):
    from dan_amd import synthetic
    from dan_amd.train_pb import PBAnchorTargets, PBModel, PBTrainer
    H = W = 64
    imgs = synthetic.make_images(2, H, W, dev, seed=1)
    targets = PBAnchorTargets(H, W, dev).encode_batch(synthetic.make_gt_boxes(2, H, W, seed=2, max_faces=3))

    def make():
        return PBTrainer(PBModel(device=dev, seed=3), deterministic=True), lambda tr: tr.train_step(imgs, targets)

    _assert_same_bits(_two_trainers(make))


def test_dan_step_is_bit_reproducible(dev):
    from dan_amd import synthetic
    from dan_amd.train_dan import DANModel, DANTrainer, dan_anchor_config, encode_batch_dan
    H, W = 64, 96
    anchors = dan_anchor_config(H, W, dev)
    imgs = synthetic.make_images(2, H, W, dev, seed=1)
    loc_t, cls_t, mgt = encode_batch_dan(anchors, synthetic.make_gt_boxes(2, H, W, seed=5, max_faces=3))

    def make():
        return DANTrainer(DANModel(device=dev, seed=4), anchors, deterministic=True), lambda tr: tr.train_step(imgs, loc_t, cls_t, mgt)

    _assert_same_bits(_two_trainers(make))


def test_trainers_outside_the_modes_scope_refuse(dev):
    from dan_amd.train_dan import DANModel, DANTrainer
    with pytest.raises(NotImplementedError, match="deterministic"):
        DANTrainer(DANModel(device=dev, deform=True), None, deterministic=True)
