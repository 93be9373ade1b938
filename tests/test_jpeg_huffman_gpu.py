"""JpegDecoder(dev, entropy="device"): the Huffman stage on the device (csrc/jpeg_huffman_exact.hip) against the default decoder, whose entropy
stage runs on the host - images with torch.equal, the coefficient buffers themselves, the launch count, the retry rule.  Every corrupted stream
that reaches a kernel here is one the CPU emulation of the same routines has decoded with checked indexing (tests/test_jpeg_huffman_cpu.py)."""
import ctypes
import io
import os

import numpy as np
import pytest
import torch

import jpeg_entropy_fixtures as F

pytestmark = pytest.mark.gpu

GOLDEN = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "jpeg_golden.npz"))
ACCEPTED = [(str(n), GOLDEN["a%d_jpeg" % i].tobytes(), GOLDEN["a%d_rgb" % i]) for i, n in enumerate(GOLDEN["a_names"])]
REFUSED = [(str(n), GOLDEN["r%d_jpeg" % i].tobytes(), int(GOLDEN["r_reasons"][i])) for i, n in enumerate(GOLDEN["r_names"])]
GOOD, BAD = F.load()
ANCHOR_SCALES = [16., 32., 64., 128., 256., 512.]
K = F.header_constants()
LAUNCHES = 5 + K["DANHIP_JPEG_SYNC_ROUNDS"] + 2                                # the Huffman launches and the reconstruct pair


def test_entropy_argument():
    from dan_amd.dataset.jpeg import JpegDecoder
    with pytest.raises(ValueError):
        JpegDecoder("cuda:0", entropy="gpu")
    assert JpegDecoder("cuda:0").entropy == "host" and JpegDecoder("cuda:0").stats["entropy_device"] == 0


def test_every_accepted_stream_equals_the_default_decoder_and_recorded_pillow(dev):
    from dan_amd.dataset.jpeg import JpegDecoder
    ref, dec = JpegDecoder(dev), JpegDecoder(dev, entropy="device")
    for name, data, want in ACCEPTED:
        got = dec.decode(data)
        assert got.dtype == torch.uint8 and got.is_cuda and tuple(got.shape) == want.shape, name
        assert torch.equal(got, ref.decode(data)), name
        assert torch.equal(got.cpu(), torch.from_numpy(want)), name
    for name, data in GOOD:
        assert torch.equal(dec.decode(data), ref.decode(data)), name
    n = len(ACCEPTED) + len(GOOD)
    assert dec.stats["fallback"] == {} and dec.stats["device"] == n and dec.stats["entropy_device"] == n and dec.stats["entropy_retry"] == 0
    assert dec.stats["launches"] == n * LAUNCHES
    assert ref.stats["entropy_device"] == 0 and ref.stats["entropy_retry"] == 0 and ref.stats["launches"] == 2 * n


def test_coefficient_buffer_of_one_mixed_batch_equals_the_host_entry_point(dev):
    from dan_amd import _lib
    from dan_amd.dataset.jpeg import JpegDecoder
    datas = [d for _, d, _ in ACCEPTED] + [d for _, d in GOOD]
    want, _, status = F.host_decode(_lib.lib(), _lib.JpegDesc, _lib.JpegInfo, datas)
    assert status == [0] * len(datas)
    dec = JpegDecoder(dev, entropy="device")
    dec.decode_batch(datas)
    assert dec.stats["entropy_retry"] == 0
    got = dec.coef.cpu().numpy()
    assert got.shape == want.shape and np.array_equal(got, want)


def test_one_batch_of_mixed_sizes_and_modes_equals_the_single_decodes_in_the_same_launches(dev):
    from dan_amd.dataset.jpeg import JpegDecoder
    one = JpegDecoder(dev, entropy="device")
    single = one.decode(ACCEPTED[0][1])
    assert one.stats["launches"] == LAUNCHES
    datas = [d for _, d, _ in ACCEPTED] + [d for _, d in GOOD]
    ref = JpegDecoder(dev).decode_batch(datas)
    dec = JpegDecoder(dev, entropy="device")
    batch = dec.decode_batch(datas)
    assert dec.stats["launches"] == LAUNCHES                                   # the same number for a batch of 1 and a batch of all fixtures
    assert dec.stats["entropy_retry"] == 0 and dec.stats["entropy_device"] == len(datas) and dec.stats["fallback"] == {}
    assert len({t.untyped_storage().data_ptr() for t in batch}) == 1           # views of one allocation
    assert torch.equal(batch[0], single)
    for got, want in zip(batch, ref):
        assert torch.equal(got, want)
    again = dec.decode_batch(datas[::-1])                                      # the pinned staging buffer is reused
    for got, want in zip(again, ref[::-1]):
        assert torch.equal(got, want)
    for got, want in zip(batch, ref):                                          # ... and the first batch's images are still intact
        assert torch.equal(got, want)


def test_refused_headers_take_no_device_work_and_fall_back_as_today(dev):
    Image = pytest.importorskip("PIL.Image")
    from dan_amd.dataset.jpeg import REASONS, JpegDecoder
    for name, data, reason in REFUSED:
        if name == "cut_mid_scan":
            continue                                                           # its header is fine: see the corrupted scans below
        dec = JpegDecoder(dev, entropy="device")
        try:
            with Image.open(io.BytesIO(data)) as im:
                want = np.asarray(im.convert("RGB"), dtype=np.uint8)
        except Exception:
            want = None
        if want is None:
            with pytest.raises(Exception):
                dec.decode(data)
        else:
            assert torch.equal(dec.decode(data).cpu(), torch.from_numpy(want)), name
        assert dec.stats["launches"] == 0 and dec.stats["device"] == 0 and dec.stats["entropy_device"] == 0 and dec.stats["entropy_retry"] == 0, name
        assert dec.stats["fallback"] == {REASONS[reason]: 1}, name


def test_corrupted_scans_between_good_neighbours_end_as_the_host_stage_says(dev):
    from dan_amd.dataset.jpeg import REASONS, JpegDecoder
    bad = BAD + [("cut_mid_scan", [d for n, d, _ in REFUSED if n == "cut_mid_scan"][0], 2)]
    left, right = ACCEPTED[7], ACCEPTED[22]
    for name, data, outcome in bad:
        dec, ref = JpegDecoder(dev, entropy="device"), JpegDecoder(dev)
        want = None
        try:
            got = dec.decode_batch([left[1], data, right[1]])
        except Exception:
            got = None                                                         # Pillow refuses the stream too: the fallback raises, as today
        try:
            want = ref.decode_batch([left[1], data, right[1]])
        except Exception:
            pass
        assert (got is None) == (want is None), name
        assert dec.stats["fallback"] == ref.stats["fallback"] == ({REASONS[outcome]: 1} if outcome else {}), name
        assert dec.stats["entropy_retry"] == 1, name                           # the device stage handed it back; the host stage named the reason
        if got is not None:
            assert torch.equal(got[0].cpu(), torch.from_numpy(left[2])) and torch.equal(got[2].cpu(), torch.from_numpy(right[2])), name
            assert torch.equal(got[1], want[1]), name
        # the neighbours alone in the next batch of the same decoder are exact
        after = dec.decode_batch([left[1], right[1]])
        assert torch.equal(after[0].cpu(), torch.from_numpy(left[2])) and torch.equal(after[1].cpu(), torch.from_numpy(right[2])), name


def test_slim_get_batch_with_the_device_entropy_stage_equals_the_host_one(dev, tmp_path):
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

    def run(entropy):
        draws, images = P.Draws(11), []

        def prep(image, bboxes):
            assert torch.is_tensor(image)
            images.append(image.cpu())
            if len(bboxes) == 0:
                return None, []
            h, w = image.shape[:2]
            px = np.asarray(bboxes, np.float32).reshape(-1, 4) * np.asarray([h, w, h, w], np.float32)
            return P.preprocess_for_train(image, px, (128, 128), ANCHOR_SCALES, draws=draws)

        def encoder(b):
            return [np.zeros((5, 4), np.float32)], [np.ones((5,), np.int64)], [np.zeros((5,), np.float32)], [b]

        names, inputs = [], []
        for batch in DC.slim_get_batch(2, 3, "train", pattern, 2, 2, prep, encoder, num_epochs=2, is_training=True, seed=1, decode_device=dev,
                                       decode_entropy=entropy):
            for e in batch:
                names.append(e[1])
                inputs.append(e[0].cpu())
        return names, inputs, images

    names_h, inputs_h, images_h = run("host")
    names_d, inputs_d, images_d = run("device")
    assert names_h == names_d and len(names_h) >= 6
    assert len(images_h) == len(images_d) and all(torch.equal(a, b) for a, b in zip(images_h, images_d))
    assert len(inputs_h) == len(inputs_d) and all(torch.equal(a, b) for a, b in zip(inputs_h, inputs_d))
