"""DAN-Deform in deterministic mode, end to end: two trainers built through ops_ctx=ops.deterministic_context() hold the same bits, one step
agrees with default mode within the bound tests/test_deterministic_gpu.py uses for S3FD, and two runs of `train_dan_deform --deterministic`
write byte-identical checkpoints.  The offset convolutions' biases are set to {-2.5, 0.25, 3.25} px, so every step has far corners."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_deterministic_gpu import _assert_same_bits, _two_trainers  # noqa: E402
from test_train_cli_gpu import COMMON, data_dir  # noqa: E402,F401

pytestmark = pytest.mark.gpu

H, W = 64, 96
BIASES = (-2.5, 0.25, 3.25)


def _make(dev, ctx):
    from dan_amd import synthetic
    from dan_amd.train_dan import DANModel, DANTrainer, dan_anchor_config, encode_batch_dan
    anchors = dan_anchor_config(H, W, dev)
    imgs = synthetic.make_images(2, H, W, dev, seed=1)
    loc_t, cls_t, mgt = encode_batch_dan(anchors, synthetic.make_gt_boxes(2, H, W, seed=5, max_faces=3))

    def make():
        tr = DANTrainer(DANModel(device=dev, seed=4, deform=True), anchors, ops_ctx=ctx())
        names = [n for n, _ in tr.model.vs.named() if n.endswith("/conv2d/bias")]
        assert names, "no offset convolution found"
        for n in names:
            p = dict(tr.model.vs.named())[n]
            vals = torch.tensor([BIASES[i % 3] for i in range(p.numel())], dtype=torch.float32)
            tr.model.vs.load_tf_named({n: vals})
        return tr, lambda tr: tr.train_step(imgs, loc_t, cls_t, mgt)

    return make


def test_dan_deform_step_is_bit_reproducible(dev):
    from dan_amd import _lib, ops
    runs = _two_trainers(_make(dev, ops.deterministic_context))
    _assert_same_bits(runs)
    assert not runs[0][0].deterministic and not ops.context().deterministic and _lib.lib().danhip_get_option(b"deterministic") == 0
    # one step against default mode, from the same start: ||d - d0|| <= 0.25 ||d0|| over the whole model
    a = _one_step(_make(dev, ops.deterministic_context))
    b = _one_step(_make(dev, lambda: ops.OpsContext(deterministic=False)))
    start, _ = _make(dev, lambda: ops.OpsContext(deterministic=False))()
    w0 = start.flat.w.clone()
    md, m0 = a.flat.w - w0, b.flat.w - w0
    assert m0.norm().item() > 0
    assert (md - m0).norm().item() <= 0.25 * m0.norm().item()


def _one_step(make):
    tr, step = make()
    step(tr)
    torch.cuda.synchronize()
    return tr


def test_dynamic_loss_scale_is_refused_under_a_deterministic_context(dev):
    from dan_amd import ops
    from dan_amd.train_dan import DANModel, DANTrainer, dan_anchor_config
    with pytest.raises(NotImplementedError, match="dynamic loss scale"):
        DANTrainer(DANModel(device=dev, seed=4, deform=True), dan_anchor_config(H, W, dev), ops_ctx=ops.deterministic_context(), dynamic_loss_scale=True)


def test_deterministic_command_runs_write_identical_checkpoints(data_dir, tmp_path):  # noqa: F811
    from dan_amd import train_dan_deform
    blobs = []
    for name in ("a", "b"):
        d = str(tmp_path / name)
        assert train_dan_deform.main(COMMON + ["--data_dir", data_dir, "--model_dir", d, "--max_number_of_steps", "3", "--save_checkpoints_steps", "2",
                                               "--deterministic", "--tf_random_seed", "7", "--checkpoint_path", str(tmp_path / "none")]) == 0
        blobs.append(open(os.path.join(d, "model.ckpt-3.data-00000-of-00001"), "rb").read())
    assert len(blobs[0]) > 1 << 20 and blobs[0] == blobs[1]
