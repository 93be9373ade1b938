"""`python -m dan_amd.eval_sfd --chips_dir` end to end on the GPU (dan_amd/eval_cli.py) on a tiny synthetic WIDER tree in the style of
tests/test_eval_cli_gpu.py: one event of three JPEGs, seeded initialisers saved as a checkpoint.  The chip files are exactly the rows the
rule keeps, each decodes to size x size and each equals JpegEncoder applied to tests/face_chips_rule.py's chip of that row; without the
flag the prediction files are the same bytes and no directory is made."""
import io
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import face_chips_rule as R  # noqa: E402
import jpeg_encode_cases as C  # noqa: E402
from dan_amd.utility.face_chips import rule  # noqa: E402

pytestmark = pytest.mark.gpu

SIZES = [(120, 160), (97, 131), (150, 111)]
EVENT, NAMES = "0--Parade", ["0_Parade_a", "0_Parade_b", "0_Parade_c"]
SEED = 7
SIZE, MARGIN, MAX_PER_IMAGE = 24, 0.25, 40


@pytest.fixture(scope="module")
def run(dev, tmp_path_factory):
    from dan_amd import eval_cli, eval_dan, eval_sfd
    from dan_amd.dataset.jpeg import JpegDecoder
    from dan_amd.utility import checkpoint
    root = tmp_path_factory.mktemp("wider_chips")
    L = C.host_lib()
    d = root / "WIDER_val" / "images" / EVENT
    d.mkdir(parents=True)
    datas = []
    for k, name in enumerate(NAMES):
        h, w = SIZES[k]
        rng = np.random.RandomState(50 + k)
        img = (rng.rand(h // 8 + 1, w // 8 + 1, 3) * 255).astype(np.uint8).repeat(8, 0).repeat(8, 1)[:h, :w]
        datas.append(C.encode_host(L, np.ascontiguousarray(img), 92, 3))
        (d / (name + ".jpg")).write_bytes(datas[-1])
    (root / "list.txt").write_text("".join("%s/%s\n" % (EVENT, n) for n in NAMES))
    net = eval_cli.build_detector("sfd", dev, "act", seed=SEED)
    os.makedirs(str(root / "logs"))
    checkpoint.save_checkpoint(net.model.vs, str(root / "logs" / "model.ckpt-5"), "sfd", checksums=True)
    (root / "logs" / "checkpoint").write_text('model_checkpoint_path: "model.ckpt-5"\nall_model_checkpoint_paths: "model.ckpt-5"\n')
    images = JpegDecoder(dev).decode_batch(datas)
    # the threshold is an input of the run: the median score of a first pass, so that rows lie on both sides of it and at it
    probe, probe_num = eval_dan.detect_image_list(net, images, False, 0.3, MAX_PER_IMAGE, 577.0)
    scores = np.concatenate([probe[b, :int(probe_num[b]), 4].cpu().numpy() for b in range(len(NAMES))])
    threshold = float(np.sort(scores)[len(scores) // 2])
    rows, real = [], eval_dan.detect_image_list

    def recording(*a, **k):                                       # the detections the command itself sees, group by group
        dets, num = real(*a, **k)
        rows.extend(dets[b, :int(num[b])].cpu().numpy() for b in range(dets.shape[0]))
        return dets, num
    common = ["--data_dir", str(root), "--image_list", str(root / "list.txt"), "--checkpoint_path", str(root / "logs"), "--debug_dir", "",
              "--batch_images", "2", "--max_per_image", str(MAX_PER_IMAGE)]
    eval_dan.detect_image_list = recording
    try:
        with_chips = eval_sfd.main(common + ["--det_dir", str(root / "det"), "--chips_dir", str(root / "chips"), "--chips_size", str(SIZE),
                                             "--chips_margin", str(MARGIN), "--chips_threshold", repr(threshold)], out=io.StringIO())
    finally:
        eval_dan.detect_image_list = real
    without = eval_sfd.main(common + ["--det_dir", str(root / "det_plain")], out=io.StringIO())
    return dict(root=root, images=[im.cpu().numpy() for im in images], rows=rows, threshold=threshold, with_chips=with_chips,
                without=without)


def test_chip_files_are_the_rows_the_rule_keeps_and_hold_the_reference_chips(run):
    from PIL import Image
    from dan_amd.dataset.jpeg import JpegEncoder
    encoder = JpegEncoder(quality=75)
    want, dropped, THRESHOLD = {}, 0, run["threshold"]
    for b, name in enumerate(NAMES):
        det, (h, w) = run["rows"][b], run["images"][b].shape[:2]
        chips, src, count = R.reference([run["images"][b]], det[None], [det.shape[0]], SIZE, 250, True, THRESHOLD)
        assert count == len(chips)
        dropped += sum(1 for r in det if r[4] >= np.float32(THRESHOLD) and rule(r, h, w, 250, True) is None)
        for chip, s in zip(chips, src):
            want["%s_%d.jpg" % (name, int(s[1]))] = chip
    above = sum(int((det[:, 4] >= np.float32(THRESHOLD)).sum()) for det in run["rows"])
    total = sum(det.shape[0] for det in run["rows"])
    assert 0 < above < total, "the seeded network's scores lie on both sides of the threshold: %d of %d" % (above, total)
    files = sorted(os.listdir(str(run["root"] / "chips" / EVENT)))
    assert os.listdir(str(run["root"] / "chips")) == [EVENT]
    assert len(files) == len(want) == above - dropped and files == sorted(want)     # (a row above the threshold is dropped only for an empty rectangle)
    assert sorted(os.path.basename(p) for p in run["with_chips"]["chips"]) == files
    for name, chip in want.items():
        data = (run["root"] / "chips" / EVENT / name).read_bytes()
        with Image.open(io.BytesIO(data)) as im:
            assert im.size == (SIZE, SIZE) and im.mode == "RGB"
        assert data == encoder.encode(chip), name


def test_without_the_flag_nothing_changes(run):
    root = run["root"]
    assert run["without"]["chips"] == [] and sorted(os.listdir(str(root))) == ["WIDER_val", "chips", "det", "det_plain", "list.txt", "logs"]
    for n in NAMES:
        a = (root / "det" / "val" / EVENT / (n + ".txt")).read_bytes()
        assert a == (root / "det_plain" / "val" / EVENT / (n + ".txt")).read_bytes() and len(a.splitlines()) > 2
