"""`python -m dan_amd.eval_sfd` end to end on the GPU (dan_amd/eval_cli.py) on a synthetic WIDER tree in tmp_path: two events of three JPEGs
(the sizes tests/test_evalpipe_ragged_gpu.py uses), seeded initialisers saved as a checkpoint, --image_list.  Every prediction file is
byte for byte the per-image detect_image + write_to_txt; the printed AP equals a WiderEvaluator fed directly; the debug files exist
exactly for indices 0, n, 2n, ... of each event and each equals draw + danhip_jpeg_encode_host of the decoded image."""
import io
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import jpeg_encode_cases as C  # noqa: E402

pytestmark = pytest.mark.gpu

SIZES = [(120, 160), (97, 131), (150, 111)]
EVENTS = [("0--Parade", ["0_Parade_a", "0_Parade_b", "0_Parade_c"]), ("1--Handshaking", ["1_Hand_a", "1_Hand_b", "1_Hand_c"])]
SEED = 7


def _tree(root):
    """The JPEG files (made by the project's own host encoder, so that no test here needs Pillow) -> {event/name: bytes}."""
    L = C.host_lib()
    datas = {}
    for e, (event, names) in enumerate(EVENTS):
        d = root / "WIDER_val" / "images" / event
        d.mkdir(parents=True)
        for k, name in enumerate(names):
            h, w = SIZES[k]
            rng = np.random.RandomState(50 + 3 * e + k)
            img = (rng.rand(h // 8 + 1, w // 8 + 1, 3) * 255).astype(np.uint8).repeat(8, 0).repeat(8, 1)[:h, :w]
            data = C.encode_host(L, np.ascontiguousarray(img), 92, 3)
            (d / (name + ".jpg")).write_bytes(data)
            datas[event + "/" + name] = data
    (root / "list.txt").write_text("".join("%s/%s\n" % (event, n) for event, names in EVENTS for n in names))
    return datas


@pytest.fixture(scope="module")
def run(dev, tmp_path_factory):
    from dan_amd import eval_cli, eval_dan, eval_sfd
    from dan_amd.dataset.jpeg import JpegDecoder
    from dan_amd.utility import checkpoint
    from dan_amd.wider_eval import WiderEvaluator, WiderGroundTruth
    root = tmp_path_factory.mktemp("wider")
    datas = _tree(root)
    net = eval_cli.build_detector("sfd", dev, "act", seed=SEED)
    os.makedirs(str(root / "logs"))
    checkpoint.save_checkpoint(net.model.vs, str(root / "logs" / "model.ckpt-5"), "sfd", checksums=True)
    (root / "logs" / "checkpoint").write_text('model_checkpoint_path: "model.ckpt-5"\nall_model_checkpoint_paths: "model.ckpt-5"\n')
    # the reference results, image by image, with the same weights
    names = list(datas)
    images = {n: JpegDecoder(dev).decode(datas[n]) for n in names}
    dets = {n: eval_sfd.detect_image(net, images[n]) for n in names}
    rng = np.random.RandomState(1)
    gt_boxes = [np.concatenate([rng.rand(3, 2) * 60, 12 + rng.rand(3, 2) * 40], 1) for _ in names]
    gt = WiderGroundTruth(gt_boxes, [np.ones((3, 3), np.uint8)] * len(names), names=names)
    direct = WiderEvaluator(gt, device=dev)
    for n in names:
        direct.add_rows(gt.index_of(n), dets[n])
    want_ap = direct.result()
    out = io.StringIO()
    assert len(net.model.vs.named()) > 20                                      # the checkpoint holds the graph's variables; the command's own seed differs
    res = eval_sfd.main(["--data_dir", str(root), "--image_list", str(root / "list.txt"), "--det_dir", str(root / "det"),
                         "--debug_dir", str(root / "debug"), "--checkpoint_path", str(root / "logs"), "--log_every_n_steps", "2",
                         "--batch_images", "2"], gt=gt, out=out)
    return dict(root=root, datas=datas, images=images, dets=dets, gt=gt, want_ap=want_ap, res=res, text=out.getvalue(), net=net)


def test_prediction_files_equal_the_per_image_pipeline(run):
    from dan_amd import eval_sfd
    assert run["res"]["images"] == 6
    for event, names in EVENTS:
        for n in names:
            f = io.StringIO()
            eval_sfd.write_to_txt(f, run["dets"][event + "/" + n], event, n)
            got = (run["root"] / "det" / "val" / event / (n + ".txt")).read_text()
            assert got == f.getvalue(), n
            assert int(got.splitlines()[1]) > 0, "the seeded network writes rows: the comparison is not of empty files"


def test_printed_ap_equals_an_evaluator_fed_directly(run):
    lines = run["text"].splitlines()
    for s in ("easy", "medium", "hard"):
        assert run["res"]["ap"][s] == run["want_ap"][s]
        assert "%s AP: %.6f" % (s, run["want_ap"][s]) in lines
    assert ">> Predicting event:2/2 num:3/3" in run["text"] and "restored" in lines[0] and "model.ckpt-5" in lines[0]


def test_debug_images_are_drawn_and_encoded_where_expected(run):
    from dan_amd.utility import draw_toolbox
    want_names = sorted(names[i] + ".jpg" for _, names in EVENTS for i in (0, 2))       # indices 0, n, 2n, ... with n = 2
    assert sorted(os.listdir(str(run["root"] / "debug"))) == want_names
    assert sorted(os.path.basename(p) for p in run["res"]["debug"]) == want_names
    L = C.host_lib()
    drawn_pixels = 0
    for event, names in EVENTS:
        for i in (0, 2):
            key = event + "/" + names[i]
            det = run["dets"][key].cpu().numpy()
            image = run["images"][key].cpu().numpy()
            picture = draw_toolbox.draw_reference(image, (det[:, 4] > 0.2).astype(np.int32), det[:, :4], thickness=2)
            drawn_pixels += int((picture != image).any(axis=2).sum())
            assert (run["root"] / "debug" / (names[i] + ".jpg")).read_bytes() == C.encode_host(L, picture, 75, 3), key
    assert drawn_pixels > 0, "the seeded network scores some box above 0.2: the rectangles are in the files"
    assert run["res"]["encoder"]["device"] == 4 and run["res"]["encoder"]["host"] == 0


def test_empty_debug_dir_never_touches_the_encoder(run, monkeypatch):
    from dan_amd import eval_sfd
    from dan_amd.dataset import jpeg
    root = run["root"]

    def refuse(*a, **k):
        raise AssertionError("the encoder was constructed")
    monkeypatch.setattr(jpeg, "JpegEncoder", refuse)
    (root / "one.txt").write_text("0--Parade/0_Parade_b\n")
    res = eval_sfd.main(["--data_dir", str(root), "--image_list", str(root / "one.txt"), "--det_dir", str(root / "det2"), "--debug_dir", "",
                         "--checkpoint_path", str(root / "logs" / "model.ckpt-5")], out=io.StringIO())
    assert res["encoder"] is None and res["debug"] == [] and res["ap"] is None
    assert (root / "det2" / "val" / "0--Parade" / "0_Parade_b.txt").read_text() == (root / "det" / "val" / "0--Parade" / "0_Parade_b.txt").read_text()
