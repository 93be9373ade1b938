"""`python -m dan_amd.eval_sfd --encode_entropy device` on the GPU (dan_amd/eval_cli.py): two events, four 64 x 48 JPEGs, seeded
initialisers saved as the checkpoint, a debug image for every input.  The debug files written with the encoder's Huffman stage on the
device are byte for byte those written with it on the host, and none took the encoder's retry route."""
import io
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import jpeg_encode_cases as C  # noqa: E402

pytestmark = pytest.mark.gpu

EVENTS = [("0--Parade", ["0_Parade_a", "0_Parade_b"]), ("1--Handshaking", ["1_Hand_a", "1_Hand_b"])]


def test_debug_files_of_both_routes_are_byte_equal(dev, tmp_path):
    from dan_amd import eval_cli, eval_sfd
    from dan_amd.utility import checkpoint
    L = C.host_lib()
    root = tmp_path
    k = 0
    for event, names in EVENTS:
        d = root / "WIDER_val" / "images" / event
        d.mkdir(parents=True)
        for name in names:
            rng = np.random.RandomState(70 + k)
            img = (rng.rand(48 // 8, 64 // 8, 3) * 255).astype(np.uint8).repeat(8, 0).repeat(8, 1)
            (d / (name + ".jpg")).write_bytes(C.encode_host(L, np.ascontiguousarray(img), 92, 3))
            k += 1
    (root / "list.txt").write_text("".join("%s/%s\n" % (event, n) for event, names in EVENTS for n in names))
    net = eval_cli.build_detector("sfd", dev, "act", seed=7)
    os.makedirs(str(root / "logs"))
    checkpoint.save_checkpoint(net.model.vs, str(root / "logs" / "model.ckpt-5"), "sfd", checksums=True)
    results = {}
    for route in ("host", "device"):
        res = eval_sfd.main(["--data_dir", str(root), "--image_list", str(root / "list.txt"), "--det_dir", str(root / ("det_" + route)),
                             "--debug_dir", str(root / ("debug_" + route)), "--checkpoint_path", str(root / "logs" / "model.ckpt-5"),
                             "--log_every_n_steps", "1", "--batch_images", "2", "--encode_entropy", route], out=io.StringIO())
        results[route] = res
    names = sorted(os.listdir(str(root / "debug_host")))
    assert names == sorted(n + ".jpg" for _, ns in EVENTS for n in ns) == sorted(os.listdir(str(root / "debug_device")))
    for n in names:
        host = (root / "debug_host" / n).read_bytes()
        assert host[:2] == b"\xff\xd8" and host[-2:] == b"\xff\xd9" and len(host) > 700
        assert (root / "debug_device" / n).read_bytes() == host, n
    stats = results["device"]["encoder"]
    assert stats["entropy_retry"] == 0 and stats["entropy_device"] == 4 and stats["device"] == 4 and stats["entropy_launches"] > 0
    assert results["host"]["encoder"]["entropy_device"] == 0 and results["host"]["encoder"]["entropy_launches"] == 0
