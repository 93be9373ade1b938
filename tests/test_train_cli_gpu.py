"""The training driver end to end on the GPU (dan_amd/train_cli.py): 12 small JPEG records -> main([...]) in-process -> log lines and
TF-V2 checkpoints; resume, bit-reproducibility, the opt-in metric's launches, and the prefetching loader against the plain generator."""
import io
import os
import re

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

SIZE, BATCH = 64, 2
COMMON = ["--train_image_size", str(SIZE), "--batch_size", str(BATCH), "--log_every_n_steps", "1"]


@pytest.fixture(scope="module")
def data_dir(tmp_path_factory):
    Image = pytest.importorskip("PIL.Image")
    from dan_amd.dataset import dataset_common as DC
    d = tmp_path_factory.mktemp("records")
    recs = []
    for i in range(12):
        h, w = 96 + (i % 3) * 8, 128 - (i % 2) * 8
        rng = np.random.RandomState(i)
        img = (rng.rand(h // 8 + 1, w // 8 + 1, 3) * 255).astype(np.uint8).repeat(8, 0).repeat(8, 1)[:h, :w]
        buf = io.BytesIO()
        Image.fromarray(img).save(buf, format="JPEG", quality=90)                 # Pillow's default: a baseline stream
        boxes = [[0.10, 0.15, 0.60, 0.55], [0.35, 0.40, 0.95, 0.90], [0.05, 0.50, 0.45, 0.95]][: 1 + i % 3]
        k = len(boxes)
        recs.append(DC.convert_to_example("img%d.jpg" % i, buf.getvalue(), boxes, [0] * k, [0] * k, [0] * k, [0] * k, [0] * k, [0] * k, h, w))
    DC.write_tfrecord(str(d / "train-00000-of-00001"), recs)
    return str(d)


def _lines(model_dir):
    out = []
    for line in open(os.path.join(model_dir, "train.log")).read().splitlines():
        m = re.match(r"step (\d+): (.*)$", line)
        assert m, line
        out.append((int(m.group(1)), {k: float(v) for k, v in (kv.split("=") for kv in m.group(2).split(", "))}, m.group(2)))
    return out


def _state(model_dir):
    return open(os.path.join(model_dir, "checkpoint")).read().splitlines()[0]


@pytest.fixture(scope="module")
def first_run(data_dir, tmp_path_factory):
    from dan_amd import train_sfd
    model_dir = str(tmp_path_factory.mktemp("sfd_logs"))
    assert train_sfd.main(COMMON + ["--data_dir", data_dir, "--model_dir", model_dir, "--max_number_of_steps", "3", "--save_checkpoints_steps", "2",
                                    "--checkpoint_path", os.path.join(model_dir, "no_such_model")]) == 0
    return model_dir


def test_run_to_a_checkpoint(first_run):
    from dan_amd import train_cli
    from dan_amd.trainer import lr_schedule
    from dan_amd.utility.checkpoint import CheckpointReader, latest_checkpoint
    for step in (2, 3):
        r = CheckpointReader(os.path.join(first_run, "model.ckpt-%d" % step))
        assert int(r.get_tensor("global_step")) == step
        names = r.get_variable_to_shape_map()
        assert any(n.startswith("sfd/") and n.endswith("/Momentum") for n in names)
    assert not os.path.exists(os.path.join(first_run, "model.ckpt-1.index"))
    assert _state(first_run) == 'model_checkpoint_path: "model.ckpt-3"'
    assert latest_checkpoint(first_run) == os.path.join(first_run, "model.ckpt-3")
    lines = _lines(first_run)
    assert [s for s, _, _ in lines] == [1, 2, 3]
    for step, vals, text in lines:
        assert list(vals) == ["lr", "ce", "loc", "loss", "l2", "acc"]
        assert 0.0 <= vals["acc"] <= 1.0
        assert vals["lr"] == float("%.6f" % lr_schedule(step)), (step, vals["lr"])
        assert all(np.isfinite(v) for v in vals.values()) and vals["ce"] > 0 and vals["loss"] > vals["l2"] > 0
        assert text == train_cli.format_log(vals)                                # six decimals survive the round trip through float


def test_resume_continues_from_the_stored_step(first_run, data_dir):
    from dan_amd import train_sfd
    from dan_amd.utility.checkpoint import CheckpointReader
    before = len(_lines(first_run))
    assert before == 3
    assert train_sfd.main(COMMON + ["--data_dir", data_dir, "--model_dir", first_run, "--max_number_of_steps", "5"]) == 0
    lines = _lines(first_run)
    assert [s for s, _, _ in lines[before:]] == [4, 5]
    assert _state(first_run) == 'model_checkpoint_path: "model.ckpt-5"'
    assert int(CheckpointReader(os.path.join(first_run, "model.ckpt-5")).get_tensor("global_step")) == 5
    assert os.path.exists(os.path.join(first_run, "model.ckpt-2.index"))          # five are kept: nothing rotated out yet


def test_deterministic_runs_write_identical_checkpoints(data_dir, tmp_path):
    from dan_amd import train_sfd
    blobs = []
    for name in ("a", "b"):
        d = str(tmp_path / name)
        assert train_sfd.main(COMMON + ["--data_dir", data_dir, "--model_dir", d, "--max_number_of_steps", "3", "--save_checkpoints_steps", "2",
                                        "--deterministic", "--tf_random_seed", "7", "--checkpoint_path", str(tmp_path / "none")]) == 0
        blobs.append(open(os.path.join(d, "model.ckpt-3.data-00000-of-00001"), "rb").read())
    assert len(blobs[0]) > 1 << 20 and blobs[0] == blobs[1]


def _sfd_trainer(dev, metrics, seed=9):
    from dan_amd import synthetic
    from dan_amd.train_sfd import AnchorConfig, SFDModel, SFDTrainer
    tr = SFDTrainer(SFDModel(device=dev, seed=seed), deterministic=True, metrics=metrics)
    imgs = synthetic.make_images(BATCH, SIZE, SIZE, dev, seed=3)
    loc_t, cls_t, _ = AnchorConfig(SIZE, SIZE, dev).encode_batch(synthetic.make_gt_boxes(BATCH, SIZE, SIZE, seed=2, max_faces=3))
    return tr, (imgs, loc_t, cls_t)


def test_metric_is_read_only(dev):
    """Two steps from one seed, deterministic: the trainer that counts the metric and the one that does not hold the same weight and momentum bits."""
    states = []
    for metrics in (False, True):
        tr, args = _sfd_trainer(dev, metrics)
        for _ in range(2):
            tr.train_step(*args)
        states.append((tr.flat.w.clone(), tr.flat.v.clone(), tr.loss_values()))
        if metrics:
            m = tr.metric_values()
            correct, total = tr.metric_counts.tolist()
            assert 0 < total and 0 <= correct <= total and m == {"cls_accuracy": correct / total}
        else:
            assert tr.metric_counts is None
            with pytest.raises(RuntimeError):
                tr.metric_values()
        tr.close()
    assert torch.equal(states[0][0], states[1][0]) and torch.equal(states[0][1], states[1][1]) and states[0][2] == states[1][2]


def _step_launches(dev, build):
    """Every library call of one eager step, by name (ops.call and _lib.call are the two doors; recorded, then passed on)."""
    import gc
    from dan_amd import _lib, ops, trainer as T
    from dan_amd.utility import anchor_manipulator, custom_op
    # Earlier trainers' parameters die NOW, not when the collector happens to run: a packed parameter that dies between the two steps below
    # clears ops' packing tables, and the recorded step would carry the danhip_pack_entry_init calls of their rebuild.
    gc.collect()
    tr, args = build()
    tr.train_step(*args)                                                          # (first step: packings, scratch, lazy initialisation)
    names = []
    real = _lib.call

    def spy(name, *a):
        names.append(name)
        return real(name, *a)
    mods = [m for m in (ops, T, anchor_manipulator, custom_op) if getattr(m, "call", None) is real]
    for m in mods:
        m.call = spy
    try:
        tr.train_step(*args)
    finally:
        for m in mods:
            m.call = real
    tr.close()
    return names


def test_metric_adds_exactly_one_launch_per_measured_term(dev):
    """metrics=False: the step's library calls are exactly those of a trainer built without the argument (the parent commit's step) - no
    danhip_cls_accuracy among them; metrics=True: the same sequence plus ONE danhip_cls_accuracy, right behind the measured term's loss."""
    from dan_amd import synthetic
    from dan_amd.train_sfd import AnchorConfig, SFDModel, SFDTrainer

    def build(**kw):
        def make():
            tr = SFDTrainer(SFDModel(device=dev, seed=9), **kw)
            imgs = synthetic.make_images(BATCH, SIZE, SIZE, dev, seed=3)
            loc_t, cls_t, _ = AnchorConfig(SIZE, SIZE, dev).encode_batch(synthetic.make_gt_boxes(BATCH, SIZE, SIZE, seed=2, max_faces=3))
            return tr, (imgs, loc_t, cls_t)
        return make
    default, off, on = _step_launches(dev, build()), _step_launches(dev, build(metrics=False)), _step_launches(dev, build(metrics=True))
    assert len(default) > 50 and "danhip_cls_accuracy" not in default
    assert off == default
    assert on.count("danhip_cls_accuracy") == 1
    i = on.index("danhip_cls_accuracy")
    assert on[i - 1] == "danhip_detection_loss_fwd" and on[:i] + on[i + 1:] == default
    # PyramidBox (three loss terms) and DAN (two): the reference measures ONE of them - the face term / stage 1
    from dan_amd.train_dan import DANModel, DANTrainer, dan_anchor_config, encode_batch_dan
    from dan_amd.train_pb import PBAnchorTargets, PBModel, PBTrainer
    gts = synthetic.make_gt_boxes(BATCH, SIZE, SIZE, seed=2, max_faces=3)
    imgs = synthetic.make_images(BATCH, SIZE, SIZE, dev, seed=3)

    def pb(**kw):
        return lambda: (PBTrainer(PBModel(device=dev, seed=3), **kw), (imgs, PBAnchorTargets(SIZE, SIZE, dev).encode_batch(gts)))

    def dan(**kw):
        def make():
            anchors = dan_anchor_config(SIZE, SIZE, dev)
            return DANTrainer(DANModel(device=dev, seed=4), anchors, **kw), (imgs,) + tuple(encode_batch_dan(anchors, gts))
        return make
    for make, terms in ((pb, 3), (dan, 2)):
        off, on = _step_launches(dev, make()), _step_launches(dev, make(metrics=True))
        assert off.count("danhip_detection_loss_fwd") == terms and "danhip_cls_accuracy" not in off
        i = on.index("danhip_cls_accuracy")
        assert on.count("danhip_cls_accuracy") == 1 and on[:i] + on[i + 1:] == off
        assert on[:i].count("danhip_detection_loss_fwd") == 1                     # behind the FIRST term's loss: face / stage 1


def _flat(batch):
    from dan_amd.train_cli import _tensors
    return list(_tensors(batch))


def test_prefetching_loader_yields_the_plain_generators_batches(dev, data_dir):
    from dan_amd import train_cli
    args = train_cli.build_parser("sfd").parse_args(COMMON + ["--data_dir", data_dir, "--tf_random_seed", "5"])
    setup = train_cli._Setup("sfd", args, dev, dict(metrics=True))
    plain = []
    for batch in train_cli.batches(setup, args, dev):
        plain.append([t.clone() for t in _flat(batch)])
        if len(plain) == 4:
            break
    loader = train_cli.Prefetcher(lambda: train_cli.batches(setup, args, dev), dev)
    try:
        got = []
        for batch in loader:
            got.append([t.clone() for t in _flat(batch)])
            if len(got) == 4:
                break
    finally:
        loader.close()
        setup.trainer.close()
    assert not loader._thread.is_alive()
    assert len(plain) == len(got) == 4
    for a, b in zip(plain, got):
        assert len(a) == len(b) == 3
        assert tuple(a[0].shape) == (BATCH, SIZE, SIZE, 8) and a[2].dtype == torch.int32
        for x, y in zip(a, b):
            assert x.dtype == y.dtype and torch.equal(x, y)
    assert not all(torch.equal(plain[0][0], p[0]) for p in plain[1:])            # (four different batches, not one repeated)


@pytest.mark.parametrize("model", ["pb", "dan", "dan_deform"])
def test_other_entry_points_take_a_step(model, data_dir, tmp_path):
    import importlib
    from dan_amd import train_cli
    mod = importlib.import_module("dan_amd.train_" + model)
    d = str(tmp_path / model)
    assert mod.main(COMMON + ["--data_dir", data_dir, "--model_dir", d, "--max_number_of_steps", "1", "--checkpoint_path", str(tmp_path / "none")]) == 0
    (step, vals, _), = _lines(d)
    assert step == 1 and list(vals) == list(train_cli.LOG_KEYS[model]) and 0.0 <= vals["acc"] <= 1.0
    assert os.path.exists(os.path.join(d, "model.ckpt-1.index"))
