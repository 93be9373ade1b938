"""JPEG decode on the device (dan_amd/dataset/jpeg.py over csrc/jpeg_entropy.cpp + csrc/jpeg_exact.hip) against the recorded Pillow pixels of
tests/golden/jpeg_golden.npz, bit for bit.  Every stream that reaches a kernel here has passed the host validator; the refused ones are shown
not to reach one.  Launches are counted by the library's launcher itself (danhip_jpeg_reconstruct_batch reports how many kernels it
launched - it is the only place that launches them - and JpegDecoder sums that in stats['launches']): the tree has no event counter that
covers non-convolution kernels."""
import io
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

GOLDEN = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "jpeg_golden.npz"))
ACCEPTED = [(str(n), GOLDEN["a%d_jpeg" % i].tobytes(), GOLDEN["a%d_rgb" % i]) for i, n in enumerate(GOLDEN["a_names"])]
REFUSED = [(str(n), GOLDEN["r%d_jpeg" % i].tobytes(), int(GOLDEN["r_reasons"][i])) for i, n in enumerate(GOLDEN["r_names"])]
ANCHOR_SCALES = [16., 32., 64., 128., 256., 512.]


def test_decode_equals_recorded_pillow_for_every_accepted_fixture(dev):
    from dan_amd.dataset.jpeg import JpegDecoder
    dec = JpegDecoder(dev)
    for name, data, want in ACCEPTED:
        got = dec.decode(data)
        assert got.dtype == torch.uint8 and got.is_cuda and tuple(got.shape) == want.shape, name
        assert torch.equal(got.cpu(), torch.from_numpy(want)), name
    assert dec.stats["fallback"] == {} and dec.stats["device"] == len(ACCEPTED)


def test_one_batch_of_mixed_sizes_and_modes_equals_the_single_decodes_in_the_same_two_launches(dev):
    from dan_amd.dataset.jpeg import JpegDecoder
    one = JpegDecoder(dev)
    single = one.decode(ACCEPTED[0][1])
    assert one.stats["launches"] == 2
    dec = JpegDecoder(dev, threads=4)
    batch = dec.decode_batch([d for _, d, _ in ACCEPTED])
    assert dec.stats["launches"] == 2 and dec.stats["device"] == len(ACCEPTED) and dec.stats["fallback"] == {}
    storage = {t.untyped_storage().data_ptr() for t in batch}
    assert len(storage) == 1                                              # views of one allocation
    assert torch.equal(batch[0], single)
    for (name, _, want), got in zip(ACCEPTED, batch):
        assert torch.equal(got.cpu(), torch.from_numpy(want)), name
    again = dec.decode_batch([d for _, d, _ in ACCEPTED[::-1]])           # the pinned staging buffer is reused: order must not matter
    for (name, _, want), got in zip(ACCEPTED[::-1], again):
        assert torch.equal(got.cpu(), torch.from_numpy(want)), name
    for (name, _, want), got in zip(ACCEPTED, batch):                     # ... and the first batch's images are still intact
        assert torch.equal(got.cpu(), torch.from_numpy(want)), name


def test_refused_streams_take_no_device_work_and_fall_back_to_pillow(dev):
    Image = pytest.importorskip("PIL.Image")
    from dan_amd.dataset.jpeg import REASONS, JpegDecoder
    for name, data, reason in REFUSED:
        dec = JpegDecoder(dev)
        try:
            with Image.open(io.BytesIO(data)) as im:
                want = np.asarray(im.convert("RGB"), dtype=np.uint8)
        except Exception:
            want = None                                                   # Pillow refuses it too (the hostile headers, the cut scan)
        if want is None:
            with pytest.raises(Exception):
                dec.decode(data)
        else:
            got = dec.decode(data)
            assert torch.equal(got.cpu(), torch.from_numpy(want)), name
        assert name not in ("noise_after_soi", "header_65535x65535") or want is None
        assert dec.stats["launches"] == 0 and dec.stats["device"] == 0, name
        assert dec.stats["fallback"] == {REASONS[reason]: 1}, name
    # in a batch: the neighbours are decoded on the device, the refused one comes from Pillow
    dec = JpegDecoder(dev)
    name, data, reason = [r for r in REFUSED if r[0] == "progressive"][0]
    got = dec.decode_batch([ACCEPTED[3][1], data, ACCEPTED[20][1]])
    with Image.open(io.BytesIO(data)) as im:
        want = np.asarray(im.convert("RGB"), dtype=np.uint8)
    assert torch.equal(got[1].cpu(), torch.from_numpy(want))
    assert torch.equal(got[0].cpu(), torch.from_numpy(ACCEPTED[3][2])) and torch.equal(got[2].cpu(), torch.from_numpy(ACCEPTED[20][2]))
    assert dec.stats["launches"] == 2 and dec.stats["device"] == 2 and dec.stats["fallback"] == {"progressive": 1}


def test_slim_get_batch_on_the_device_equals_the_host_path(dev, tmp_path):
    Image = pytest.importorskip("PIL.Image")
    from dan_amd.dataset import dataset_common as DC
    from dan_amd.preprocessing import dan_preprocessing as P
    recs = []
    for i in range(10):                                                   # the records of tests/test_dataset_cpu.py
        h, w = 40 + i, 56
        rng = np.random.RandomState(i)
        img = (rng.rand(h // 8 + 1, w // 8 + 1, 3) * 255).astype(np.uint8).repeat(8, 0).repeat(8, 1)[:h, :w]
        b = io.BytesIO()
        Image.fromarray(img).save(b, format="JPEG", quality=95)
        boxes = [] if i == 3 else [[0.1, 0.2, 0.5, 0.6], [0.3, 0.3, 0.9, 0.8]][: 1 + i % 2]
        k = len(boxes)
        recs.append(DC.convert_to_example("img%d.jpg" % i, b.getvalue(), boxes, [0] * k, [0] * k, [0] * k, [0] * k, [0] * k, [0] * k, h, w))
    DC.write_tfrecord(str(tmp_path / "wider_train-00000-of-00001"), recs)
    pattern = str(tmp_path / "wider_{}-*")

    def run(decode_device):
        draws, images = P.Draws(11), []

        def prep(image, bboxes):
            on_device = torch.is_tensor(image)
            assert on_device == (decode_device is not None)
            image = image if on_device else torch.from_numpy(image).to(dev)
            images.append(image.cpu())
            if len(bboxes) == 0:
                return None, []                                           # the face-less record: skipped by keep_input on both paths
            h, w = image.shape[:2]
            px = np.asarray(bboxes, np.float32).reshape(-1, 4) * np.asarray([h, w, h, w], np.float32)
            return P.preprocess_for_train(image, px, (128, 128), ANCHOR_SCALES, draws=draws)

        def encoder(b):
            return [np.zeros((5, 4), np.float32)], [np.ones((5,), np.int64)], [np.zeros((5,), np.float32)], [b]

        names, inputs = [], []
        for batch in DC.slim_get_batch(2, 3, "train", pattern, 2, 2, prep, encoder, num_epochs=2, is_training=True, seed=1,
                                       decode_device=decode_device):
            for e in batch:
                names.append(e[1])
                inputs.append(e[0].cpu())
        return names, inputs, images

    names_h, inputs_h, images_h = run(None)
    names_d, inputs_d, images_d = run(dev)
    assert names_h == names_d and len(names_h) >= 6
    assert len(images_h) == len(images_d) and all(torch.equal(a, b) for a, b in zip(images_h, images_d))
    assert len(inputs_h) == len(inputs_d) and all(torch.equal(a, b) for a, b in zip(inputs_h, inputs_d))
