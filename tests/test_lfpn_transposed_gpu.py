"""PyramidBox with lfpn_upsample="transposed" (net/pb_net.py build_lfpn, ops.conv_transpose_add): gradients for the new variables, a
bit-reproducible deterministic step, checkpoints with and without the new variables, the fp32 inference path, and the refusal of the
split-operand precision.  Inputs of 64 x 64 and 72 x 56: the second gives odd lateral maps (18 x 14 -> 9 x 7 -> 5 x 4), so the crop runs."""
import pytest
import torch

pytestmark = pytest.mark.gpu
SIZES = [(64, 64), (72, 56)]
LEVELS = ("lfpn/fpn_0", "lfpn/fpn_1", "lfpn/fpn_2")
# 16-bit path against the fp32 path: tests/test_eval_f32_gpu.py puts the 16-bit build's PyramidBox outputs at "4-6 % of scale" of an fp32
# reference on the same graph and holds the 16-bit logits to logits16_tol = 0.06 of the reference's scale where it compares them; the LFPN
# maps are held to the same fraction here.
TOL16 = 0.06


def _new_names(model):
    return [n for n, _ in model.vs.named() if "upsample_deconv" in n]


def _batch(H, W, dev, B=2):
    from dan_amd import synthetic
    from dan_amd.train_pb import PBAnchorTargets
    imgs = synthetic.make_images(B, H, W, dev, seed=1)
    targets = PBAnchorTargets(H, W, dev).encode_batch(synthetic.make_gt_boxes(B, H, W, seed=2, max_faces=3))
    return imgs, targets


def test_default_model_has_no_new_variable(dev):
    from dan_amd.train_pb import PBModel
    model = PBModel(device=dev, seed=3)
    with torch.no_grad():
        model.forward(torch.zeros((1, 64, 64, 3), dtype=torch.uint8, device=dev))
    assert not _new_names(model)
    t = PBModel(device=dev, seed=3, lfpn_upsample="transposed")
    with torch.no_grad():
        t.forward(torch.zeros((1, 64, 64, 3), dtype=torch.uint8, device=dev))
    assert sorted(_new_names(t)) == sorted(lv + "/upsample_deconv/" + k for lv in LEVELS for k in ("kernel", "bias"))
    order = [n for n, _ in t.vs.named()]
    for lv in LEVELS:                                    # created between the lateral and the fused convolution: backward meets them in reverse
        assert order.index(lv + "/lateral/bias") < order.index(lv + "/upsample_deconv/kernel") < order.index(lv + "/upsample_deconv/bias") \
            < order.index(lv + "/fused_conv/kernel")
    assert [n for n in order if "upsample_deconv" not in n] == [n for n, _ in model.vs.named()]
    shapes = dict((n, tuple(p.shape)) for n, p in t.vs.named())
    assert shapes["lfpn/fpn_2/upsample_deconv/kernel"] == (4, 4, 512, 512) and shapes["lfpn/fpn_0/upsample_deconv/kernel"] == (4, 4, 256, 256)


@pytest.mark.parametrize("H,W", SIZES)
def test_forward_backward_gives_finite_gradients_for_the_new_variables(H, W, dev):
    from dan_amd.train_pb import PBModel, PBTrainer
    imgs, targets = _batch(H, W, dev)
    tr = PBTrainer(PBModel(device=dev, seed=3, lfpn_upsample="transposed"))
    w0 = tr.flat.w.clone()
    tr.train_step(imgs, targets)
    torch.cuda.synchronize()
    names = _new_names(tr.model)
    assert len(names) == 6
    for n, p in tr.model.vs.named():
        if n in names:
            g = p._danhip_grad
            assert torch.isfinite(g).all() and g.abs().max().item() > 0, n
    assert torch.isfinite(tr.flat.w).all() and not torch.equal(tr.flat.w, w0)
    assert all(v == v for v in tr.loss_values()["face"])
    tr.close()


@pytest.mark.parametrize("H,W", SIZES)
def test_deterministic_step_twice_from_one_seed_gives_identical_bits(H, W, dev):
    from dan_amd.train_pb import PBModel, PBTrainer
    imgs, targets = _batch(H, W, dev)
    runs = []
    for _ in range(2):
        tr = PBTrainer(PBModel(device=dev, seed=3, lfpn_upsample="transposed"), deterministic=True)
        tr.train_step(imgs, targets)
        torch.cuda.synchronize()
        runs.append(tr)
    a, b = runs
    assert a.ops_ctx.deterministic
    assert torch.equal(a.flat.w, b.flat.w), "%d weights differ" % (a.flat.w != b.flat.w).sum().item()
    assert torch.equal(a.flat.v, b.flat.v)
    assert torch.isfinite(a.flat.w).all() and a.flat.v.abs().max().item() > 0
    for n, p in a.model.vs.named():                      # the new variables moved: their momenta are not zero
        if "upsample_deconv/kernel" in n:
            assert (a.flat.v[a.flat.start_of_member[n]:a.flat.start_of_member[n] + p.numel()] != 0).any(), n
    a.close()
    b.close()


def test_checkpoint_round_trip_and_restore_from_the_default_model(tmp_path, dev):
    from dan_amd.train_pb import PBModel, PBTrainer
    H, W = 72, 56
    imgs, targets = _batch(H, W, dev)
    tr = PBTrainer(PBModel(device=dev, seed=3, lfpn_upsample="transposed"))
    tr.train_step(imgs, targets)
    torch.cuda.synchronize()
    prefix = str(tmp_path / "model.ckpt-1")
    tr.save(prefix, "pyramid_box", checksums=True)
    want_w, want_v = tr.flat.w.clone(), tr.flat.v.clone()
    names = _new_names(tr.model)
    tr2 = PBTrainer(PBModel(device=dev, seed=11, lfpn_upsample="transposed"))
    assert not torch.equal(tr2.flat.w, want_w)
    restored = tr2.restore(prefix, "pyramid_box", verify=True)
    assert all("pyramid_box/" + n in restored and "pyramid_box/" + n + "/Momentum" in restored for n in names)
    assert torch.equal(tr2.flat.w, want_w) and torch.equal(tr2.flat.v, want_v) and tr2.step_no == 1
    tr2.train_step(imgs, targets)                         # and it trains on from there
    torch.cuda.synchronize()
    assert torch.isfinite(tr2.flat.w).all()
    # a checkpoint written by the default model: everything it holds is restored, the new variables keep their initialiser
    base = PBTrainer(PBModel(device=dev, seed=5))
    base.train_step(imgs, targets)
    torch.cuda.synchronize()
    prefix0 = str(tmp_path / "default.ckpt-1")
    base.save(prefix0, "pyramid_box", checksums=True)
    tr3 = PBTrainer(PBModel(device=dev, seed=11, lfpn_upsample="transposed"))
    init = {n: p.detach().clone() for n, p in tr3.model.vs.named()}
    restored = tr3.restore(prefix0, "pyramid_box", verify=True)
    assert not [r for r in restored if "upsample_deconv" in r]
    theirs = dict(base.model.vs.named())
    for n, p in tr3.model.vs.named():
        if "upsample_deconv" in n:
            assert torch.equal(p.detach(), init[n]), n
        else:
            assert torch.equal(p.detach(), theirs[n].detach()), n
    import sys, os
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    import conv_transpose_exact as CT
    k = dict(tr3.model.vs.named())["lfpn/fpn_1/upsample_deconv/kernel"].detach().cpu()
    assert torch.equal(k.to(CT.F64), CT.deconv_initializer(512, 512))
    # a warm start that asks for every variable (ignore_missing_vars=False) still treats the new ones as optional
    from dan_amd.utility import checkpoint
    warm = PBModel(device=dev, seed=13, lfpn_upsample="transposed")
    with torch.no_grad():
        warm.forward(torch.zeros((1, 64, 64, 3), dtype=torch.uint8, device=dev))
    got = checkpoint.init_from_checkpoint(warm.vs, prefix0, "pyramid_box", None, None, ignore_missing_vars=False, verify=True)
    assert len(got) == len(theirs) and not [n for n in got if "upsample_deconv" in n]
    for t in (tr, tr2, base, tr3):
        t.close()


@pytest.mark.parametrize("H,W", SIZES)
def test_fp32_detector_runs_and_its_lfpn_agrees_with_the_16_bit_path(H, W, dev):
    from dan_amd import synthetic
    from dan_amd.eval_dan import Detector
    from dan_amd.net import sfd_net
    from dan_amd.train_pb import PBModel
    from dan_amd.train_sfd import AnchorConfig
    model = PBModel(device=dev, seed=3, lfpn_upsample="transposed")
    imgs = synthetic.make_images(1, H, W, dev, seed=H + W)
    with torch.no_grad():
        model.forward(imgs)                               # creates the variables
        g = torch.Generator().manual_seed(5)
        for n, p in model.vs.named():                     # away from the initialiser: every tap and channel pair carries weight
            if "upsample_deconv/kernel" in n:
                p.add_((0.02 * torch.randn(p.shape, generator=g)).to(dev))
            if "upsample_deconv/bias" in n:
                p.add_((0.05 * torch.randn(p.shape, generator=g)).to(dev))
    from dan_amd import ops
    ops.WEIGHT_EPOCH += 1

    def lfpn(precision):
        b = model.backbone
        with torch.no_grad(), sfd_net.precision_scope(precision):
            feats = b.get_featmaps(sfd_net.prepare_input(imgs, precision), training=False)
            return [f.float() for f in b.build_lfpn(feats, skip_last=3, upsample="transposed")[:3]]

    ref, got = lfpn("fp32"), lfpn("act")
    for k, (r, a) in enumerate(zip(ref, got)):
        assert r.shape == a.shape and torch.isfinite(r).all()
        err, scale = (r - a).abs().max().item(), r.abs().max().item()
        print("lfpn level %d %s: 16-bit against fp32 %.4f of scale" % (k, tuple(r.shape), err / scale))
        assert err <= TOL16 * scale, (k, err, scale)
    det = Detector(model, lambda h, w, d: AnchorConfig(h, w, d), precision="fp32")
    boxes, scores = det(imgs[0])
    assert boxes.dtype == torch.float32 and torch.isfinite(boxes).all() and torch.isfinite(scores).all()
    det16 = Detector(model, lambda h, w, d: AnchorConfig(h, w, d), precision="act")
    assert torch.isfinite(det16(imgs[0])[0]).all()


def test_split_precision_raises_a_value_error_that_names_the_option(dev):
    from dan_amd import synthetic
    from dan_amd.eval_dan import Detector
    from dan_amd.train_pb import PBModel
    from dan_amd.train_sfd import AnchorConfig
    model = PBModel(device=dev, seed=3, lfpn_upsample="transposed")
    det = Detector(model, lambda h, w, d: AnchorConfig(h, w, d), precision="split")
    with pytest.raises(ValueError, match="lfpn_upsample"):
        det(synthetic.make_images(1, 64, 64, dev, seed=4)[0])
    from dan_amd import ops
    assert ops.context().SPLIT_EVAL is False               # the scope was left
    # and the default graph still runs in that precision
    ok = Detector(PBModel(device=dev, seed=3), lambda h, w, d: AnchorConfig(h, w, d), precision="split")
    assert torch.isfinite(ok(synthetic.make_images(1, 64, 64, dev, seed=4)[0])[0]).all()
