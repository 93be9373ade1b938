"""`python -m dan_amd.eval_sfd --redact_dir` end to end on the GPU (dan_amd/eval_cli.py) on a tiny synthetic WIDER tree in the style of
tests/test_eval_cli_chips_gpu.py: one event of two JPEGs, seeded initialisers saved as a checkpoint.  One file per image under its event,
each equal to JpegEncoder.encode_batch of redact.apply of the decoded image with the detections the run itself saw; without the flag no
directory is made and the "debug" and "chips" outputs are the same bytes."""
import io
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import jpeg_encode_cases as C  # noqa: E402
import redact_rule as R  # noqa: E402

pytestmark = pytest.mark.gpu

SIZES = [(120, 160), (97, 131)]
EVENT, NAMES = "0--Parade", ["0_Parade_a", "0_Parade_b"]
SEED, MAX_PER_IMAGE = 7, 40
FLAGS = ["--redact_mode", "mosaic", "--redact_shape", "ellipse", "--redact_strength", "0.2", "--redact_margin", "0.1"]


@pytest.fixture(scope="module")
def run(dev, tmp_path_factory):
    from dan_amd import eval_cli, eval_dan, eval_sfd
    from dan_amd.dataset.jpeg import JpegDecoder
    from dan_amd.utility import checkpoint
    root = tmp_path_factory.mktemp("wider_redact")
    L = C.host_lib()
    d = root / "WIDER_val" / "images" / EVENT
    d.mkdir(parents=True)
    datas = []
    for k, name in enumerate(NAMES):
        h, w = SIZES[k]
        rng = np.random.RandomState(60 + k)
        img = (rng.rand(h // 8 + 1, w // 8 + 1, 3) * 255).astype(np.uint8).repeat(8, 0).repeat(8, 1)[:h, :w]
        datas.append(C.encode_host(L, np.ascontiguousarray(img), 92, 3))
        (d / (name + ".jpg")).write_bytes(datas[-1])
    (root / "list.txt").write_text("".join("%s/%s\n" % (EVENT, n) for n in NAMES))
    net = eval_cli.build_detector("sfd", dev, "act", seed=SEED)
    os.makedirs(str(root / "logs"))
    checkpoint.save_checkpoint(net.model.vs, str(root / "logs" / "model.ckpt-5"), "sfd", checksums=True)
    (root / "logs" / "checkpoint").write_text('model_checkpoint_path: "model.ckpt-5"\nall_model_checkpoint_paths: "model.ckpt-5"\n')
    images = JpegDecoder(dev).decode_batch(datas)
    probe, probe_num = eval_dan.detect_image_list(net, images, False, 0.3, MAX_PER_IMAGE, 577.0)
    scores = np.concatenate([probe[b, :int(probe_num[b]), 4].cpu().numpy() for b in range(len(NAMES))])
    threshold = float(np.sort(scores)[len(scores) // 2])          # rows on both sides of it and at it
    seen, real = [], eval_dan.detect_image_list

    def recording(*a, **k):                                       # the detections the command itself sees, group by group
        dets, num = real(*a, **k)
        seen.append((dets.clone(), num.clone()))
        return dets, num
    common = ["--data_dir", str(root), "--image_list", str(root / "list.txt"), "--checkpoint_path", str(root / "logs"), "--batch_images", "2",
              "--max_per_image", str(MAX_PER_IMAGE), "--log_every_n_steps", "1", "--chips_size", "16"]
    eval_dan.detect_image_list = recording
    try:
        with_redact = eval_sfd.main(common + ["--det_dir", str(root / "det"), "--debug_dir", str(root / "debug"), "--chips_dir", str(root / "chips"),
                                              "--redact_dir", str(root / "redacted"), "--redact_threshold", repr(threshold)] + FLAGS, out=io.StringIO())
    finally:
        eval_dan.detect_image_list = real
    without = eval_sfd.main(common + ["--det_dir", str(root / "det_plain"), "--debug_dir", str(root / "debug_plain"),
                                      "--chips_dir", str(root / "chips_plain")], out=io.StringIO())
    return dict(root=root, images=images, seen=seen, threshold=threshold, with_redact=with_redact, without=without)


def test_one_file_per_image_holding_the_encoded_redaction_of_the_runs_detections(run):
    from dan_amd.dataset.jpeg import JpegEncoder
    from dan_amd.utility import redact
    root = run["root"]
    assert os.listdir(str(root / "redacted")) == [EVENT]
    assert sorted(os.listdir(str(root / "redacted" / EVENT))) == [n + ".jpg" for n in NAMES]
    assert run["with_redact"]["redacted"] == [str(root / "redacted" / EVENT / (n + ".jpg")) for n in NAMES]
    assert len(run["seen"]) == 1                                  # one group of two images
    dets, num = run["seen"][0]
    pictures, count = redact.apply(run["images"], dets, num, mode="mosaic", shape="ellipse", strength=0.2, margin=0.1, score_threshold=run["threshold"])
    host = [im.cpu().numpy() for im in run["images"]]
    want, want_count = R.reference(host, dets.cpu().numpy(), num.cpu().tolist(), mode="mosaic", shape="ellipse", strength_pm=200, margin_pm=100,
                                   threshold=run["threshold"])
    assert 0 < want_count == int(count.item()) < int(num.sum().item())       # rows on both sides of the threshold
    for p, w, h in zip(pictures, want, host):
        assert np.array_equal(p.cpu().numpy(), w) and not np.array_equal(w, h)
    for name, data in zip(NAMES, JpegEncoder(quality=75).encode_batch(pictures)):
        assert (root / "redacted" / EVENT / (name + ".jpg")).read_bytes() == data, name


def test_without_the_flag_nothing_changes(run):
    root = run["root"]
    assert run["without"]["redacted"] == [] and "redacted" in run["without"]
    assert sorted(os.listdir(str(root))) == ["WIDER_val", "chips", "chips_plain", "debug", "debug_plain", "det", "det_plain", "list.txt", "logs",
                                             "redacted"]
    for kind, plain in (("debug", "debug_plain"), ("chips", "chips_plain")):
        a, b = run["with_redact"][kind], run["without"][kind]
        assert len(a) == len(b) > 0
        for pa, pb in zip(a, b):
            assert os.path.relpath(pa, str(root / kind)) == os.path.relpath(pb, str(root / plain))
            with open(pa, "rb") as fa, open(pb, "rb") as fb:
                assert fa.read() == fb.read(), pa
    for n in NAMES:
        assert (root / "det" / "val" / EVENT / (n + ".txt")).read_bytes() == (root / "det_plain" / "val" / EVENT / (n + ".txt")).read_bytes()
