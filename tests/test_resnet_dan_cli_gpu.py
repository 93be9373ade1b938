"""train_dan --backbone resnet50 for two steps on tiny synthetic records (as tests/test_train_cli_gpu.py builds them, at its size), resumed for
a third, then eval_dan --backbone resnet50 on its checkpoint over two images: prediction files are written."""
import io
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SIZE, BATCH = 64, 2


def _jpeg(Image, i, h, w):
    rng = np.random.RandomState(i)
    img = (rng.rand(h // 8 + 1, w // 8 + 1, 3) * 255).astype(np.uint8).repeat(8, 0).repeat(8, 1)[:h, :w]
    buf = io.BytesIO()
    Image.fromarray(img).save(buf, format="JPEG", quality=90)
    return buf.getvalue()


def test_train_resume_and_evaluate(dev, tmp_path):
    Image = pytest.importorskip("PIL.Image")
    from dan_amd import eval_dan, train_dan
    from dan_amd.dataset import dataset_common as DC
    from dan_amd.utility.checkpoint import CheckpointReader
    recs = []
    for i in range(8):
        h, w = 96 + (i % 3) * 8, 128 - (i % 2) * 8
        boxes = [[0.10, 0.15, 0.60, 0.55], [0.35, 0.40, 0.95, 0.90], [0.05, 0.50, 0.45, 0.95]][: 1 + i % 3]
        k = len(boxes)
        recs.append(DC.convert_to_example("img%d.jpg" % i, _jpeg(Image, i, h, w), boxes, [0] * k, [0] * k, [0] * k, [0] * k, [0] * k, [0] * k, h, w))
    data = tmp_path / "records"
    data.mkdir()
    DC.write_tfrecord(str(data / "train-00000-of-00001"), recs)
    logs = str(tmp_path / "logs")
    common = ["--train_image_size", str(SIZE), "--batch_size", str(BATCH), "--log_every_n_steps", "1", "--backbone", "resnet50", "--data_dir", str(data),
              "--model_dir", logs, "--checkpoint_path", str(tmp_path / "none")]
    assert train_dan.main(common + ["--max_number_of_steps", "2"]) == 0
    r = CheckpointReader(os.path.join(logs, "model.ckpt-2"))
    names = r.get_variable_to_shape_map()
    assert int(r.get_tensor("global_step")) == 2
    mean = "dan/block_1/conv_1/increase/bn/moving_mean"
    assert mean in names and "dan/block_4/conv_3/increase/bn/gamma/Momentum" in names and not any("conv1_1" in n for n in names)
    assert np.abs(r.get_tensor(mean)).max() > 0                              # the moving statistics moved and were saved
    assert train_dan.main(common + ["--max_number_of_steps", "3"]) == 0      # resumes from model_dir
    lines = open(os.path.join(logs, "train.log")).read().splitlines()
    assert [l.split(":")[0] for l in lines] == ["step 1", "step 2", "step 3"]
    assert not np.array_equal(CheckpointReader(os.path.join(logs, "model.ckpt-3")).get_tensor(mean), r.get_tensor(mean))
    root = tmp_path / "wider"
    (root / "WIDER_val" / "images" / "0--Parade").mkdir(parents=True)
    for k, name in enumerate(("a", "b")):
        (root / "WIDER_val" / "images" / "0--Parade" / (name + ".jpg")).write_bytes(_jpeg(Image, 20 + k, 96, 120 + 8 * k))
    (root / "list.txt").write_text("0--Parade/a\n0--Parade/b\n")
    out = io.StringIO()
    res = eval_dan.main(["--backbone", "resnet50", "--data_dir", str(root), "--image_list", str(root / "list.txt"), "--det_dir", str(root / "det"),
                         "--debug_dir", "", "--checkpoint_path", logs, "--batch_images", "2"], out=out)
    assert res["images"] == 2 and "restored" in out.getvalue()
    for name in ("a", "b"):
        text = (root / "det" / "val" / "0--Parade" / (name + ".txt")).read_text().splitlines()
        assert text[0] in (name, "0--Parade/" + name, name + ".jpg") or name in text[0]
        assert int(text[1]) == len(text) - 2
    with pytest.raises(Exception):                                           # the VGG graph does not find its variables in this checkpoint
        eval_dan.main(["--data_dir", str(root), "--image_list", str(root / "list.txt"), "--det_dir", str(root / "det_vgg"), "--debug_dir", "",
                       "--checkpoint_path", logs, "--batch_images", "2"], out=io.StringIO())
