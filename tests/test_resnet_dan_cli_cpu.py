"""--backbone of train_dan / eval_dan without a device: --help lists it, it is not a reference flag, and the refusals (--deterministic, a warm
start, a precision without batch-norm kernels) are raised before the device is touched."""
import json
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BACKBONES = ("vgg16", "resnet50", "resnet101", "resnet152")


@pytest.fixture
def no_device(monkeypatch):
    """any use of the device from here on fails the test"""
    import torch

    def touched(*a, **k):
        raise AssertionError("the device was touched")
    for name in ("set_device", "init", "current_stream", "synchronize"):
        monkeypatch.setattr(torch.cuda, name, touched)
    from dan_amd import _lib
    monkeypatch.setattr(_lib, "lib", touched)


def test_help_lists_the_flag_and_the_reference_flags_do_not():
    from dan_amd import eval_cli, train_cli
    from dan_amd.train_dan import BACKBONES as MODEL_BACKBONES
    assert train_cli.BACKBONES == eval_cli.BACKBONES == MODEL_BACKBONES == BACKBONES
    for cli in (train_cli, eval_cli):
        text = cli.build_parser("dan").format_help()
        assert "--backbone" in text and all(b in text for b in BACKBONES)
        assert cli.build_parser("dan").parse_args([]).backbone == "vgg16"
        assert cli.build_parser("dan").parse_args(["--backbone", "resnet101"]).backbone == "resnet101"
        for other in ("sfd", "pb", "dan_deform"):                           # S3FD / PyramidBox: VGG scripts; the reference has no deformable ResNet
            assert "--backbone" not in cli.build_parser(other).format_help()
        with pytest.raises(SystemExit):
            cli.build_parser("dan").parse_args(["--backbone", "resnet18"])
    for name in ("train_flags.json", "eval_flags.json"):
        path = os.path.join(ROOT, "tests", "golden", name)
        if os.path.exists(path):
            assert "backbone" not in json.dumps(json.load(open(path)))


def test_deterministic_is_refused_before_the_device(no_device, tmp_path):
    from dan_amd import train_dan
    with pytest.raises(SystemExit, match="batch norm"):
        train_dan.main(["--backbone", "resnet50", "--deterministic", "--data_dir", str(tmp_path), "--model_dir", str(tmp_path / "logs")])
    assert not (tmp_path / "logs").exists()


def test_warm_start_is_refused_before_the_device(no_device, tmp_path):
    from dan_amd import train_dan
    init = tmp_path / "init"
    init.mkdir()
    (init / "vgg16.ckpt.index").write_bytes(b"x")                          # a checkpoint by its index file, as the driver looks for one
    for path in (str(init / "vgg16.ckpt"),):
        with pytest.raises(SystemExit, match="warm-start"):
            train_dan.main(["--backbone", "resnet50", "--data_dir", str(tmp_path), "--model_dir", str(tmp_path / "logs"), "--checkpoint_path", path])
    (init / "checkpoint").write_text('model_checkpoint_path: "vgg16.ckpt"\n')
    with pytest.raises(SystemExit, match="warm-start"):                      # a directory with a state file
        train_dan.main(["--backbone", "resnet152", "--data_dir", str(tmp_path), "--model_dir", str(tmp_path / "logs"), "--checkpoint_path", str(init)])
    assert not (tmp_path / "logs").exists()


@pytest.mark.parametrize("precision", ["fp32", "split"])
def test_eval_precisions_without_batch_norm_kernels_are_refused(precision, no_device, tmp_path):
    from dan_amd import eval_dan
    with pytest.raises(SystemExit, match="--precision act only"):
        eval_dan.main(["--backbone", "resnet50", "--precision", precision, "--data_dir", str(tmp_path), "--det_dir", str(tmp_path / "det")])


def test_model_and_trainer_refusals_need_no_device():
    import types
    from dan_amd.train_dan import DANModel, DANTrainer
    with pytest.raises(ValueError, match="deformable"):
        DANModel(device="cpu", backbone="resnet50", deform=True)
    with pytest.raises(ValueError, match="backbone must be one of"):
        DANModel(device="cpu", backbone="resnet18")
    with pytest.raises(NotImplementedError, match="batch norm"):
        DANTrainer(types.SimpleNamespace(batch_norm=True, backbone_name="resnet50"), None, deterministic=True)
