"""Progressive JPEG records on the device (JpegDecoder(progressive=True): the host entropy stage of csrc/jpeg_entropy.cpp for SOF2, then the
two unchanged launches of csrc/jpeg_exact.hip) against the recorded Pillow pixels of tests/golden/jpeg_progressive_golden.npz, bit for bit.
Every fixture and the refused set run once each; a stream the validator does not take - an incomplete progression among them - is shown
to take the Pillow fallback under its reason, and a default decoder to treat every progressive stream as before."""
import ctypes
import io
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = np.load(os.path.join(HERE, "golden", "jpeg_progressive_golden.npz"))
ACCEPTED = [(str(n), GOLDEN["a%d_jpeg" % i].tobytes(), GOLDEN["a%d_rgb" % i]) for i, n in enumerate(GOLDEN["a_names"])]
REFUSED = [(str(n), GOLDEN["r%d_jpeg" % i].tobytes(), int(GOLDEN["r_reasons"][i]), GOLDEN["r%d_rgb" % i] if "r%d_rgb" % i in GOLDEN.files else None)
           for i, n in enumerate(GOLDEN["r_names"])]
BASE = np.load(os.path.join(HERE, "golden", "jpeg_golden.npz"))
BASELINE = [(str(n), BASE["a%d_jpeg" % i].tobytes(), BASE["a%d_rgb" % i]) for i, n in enumerate(BASE["a_names"])]
MIXED = [x for pair in zip(BASELINE[3::4] + BASELINE[:5], ACCEPTED) for x in pair]       # baseline, progressive, baseline, ...: every mode of both
ANCHOR_SCALES = [16., 32., 64., 128., 256., 512.]


def test_mixed_batch_with_the_host_entropy_stage_is_two_launches_and_no_fallback(dev):
    from dan_amd.dataset.jpeg import JpegDecoder
    assert len(MIXED) == 2 * len(ACCEPTED)
    dec = JpegDecoder(dev, progressive=True)
    got = dec.decode_batch([d for _, d, _ in MIXED])
    for (name, _, want), image in zip(MIXED, got):
        assert image.dtype == torch.uint8 and image.is_cuda and torch.equal(image.cpu(), torch.from_numpy(want)), name
    assert dec.stats["launches"] == 2 and dec.stats["fallback"] == {}
    assert dec.stats["progressive"] == len(ACCEPTED) and dec.stats["device"] == len(MIXED)


def test_mixed_batch_with_the_device_entropy_stage_retries_the_progressive_ones_on_the_host(dev):
    from dan_amd.dataset.jpeg import JpegDecoder
    dec = JpegDecoder(dev, entropy="device", progressive=True)
    got = dec.decode_batch([d for _, d, _ in MIXED])
    for (name, _, want), image in zip(MIXED, got):
        assert torch.equal(image.cpu(), torch.from_numpy(want)), name
    assert dec.stats["entropy_retry"] == len(ACCEPTED) and dec.stats["entropy_device"] == len(MIXED) - len(ACCEPTED)
    assert dec.stats["fallback"] == {} and dec.stats["progressive"] == len(ACCEPTED)


def test_refused_progressive_streams_fall_back_under_their_reason(dev):
    Image = pytest.importorskip("PIL.Image")
    from dan_amd import _lib
    from dan_amd.dataset.jpeg import REASONS, JpegDecoder
    assert REASONS[18] == "progression"
    seen = 0
    for name, data, reason, want in REFUSED:
        dec = JpegDecoder(dev, progressive=True)
        info = _lib.JpegInfo()
        assert _lib.lib().danhip_jpeg_inspect_ex(data, len(data), 1, ctypes.byref(info)) == reason, name
        if want is None:                                                      # Pillow's verdict on the other three is not this test's business:
            try:                                                              # only its own refusal of the stream may end the call
                with Image.open(io.BytesIO(data)) as im:
                    im.convert("RGB")
                pillow_error = None
            except Exception as e:
                pillow_error = type(e)
            if pillow_error is None:
                dec.decode(data)
            else:
                with pytest.raises(pillow_error):
                    dec.decode(data)
        else:                                                                 # the incomplete progressions: exactly Pillow's pixels for the cut file
            got = dec.decode(data)
            assert torch.equal(got.cpu(), torch.from_numpy(want)), name
            assert reason == 18
            seen += 1
        assert dec.stats["fallback"] == {REASONS[reason]: 1}, name
        assert dec.stats["launches"] == 0 and dec.stats["device"] == 0 and dec.stats["progressive"] == 0, name
    assert seen == 2


def test_a_default_decoder_still_sends_a_progressive_stream_to_the_fallback(dev):
    pytest.importorskip("PIL.Image")
    from dan_amd.dataset.jpeg import JpegDecoder
    name, data, want = ACCEPTED[9]
    for entropy in ("host", "device"):
        dec = JpegDecoder(dev, entropy=entropy)
        got = dec.decode(data)
        assert torch.equal(got.cpu(), torch.from_numpy(want))
        assert dec.stats["fallback"] == {"progressive": 1} and dec.stats["launches"] == 0 and dec.stats["progressive"] == 0


def test_slim_get_batch_with_progressive_records_on_the_device_equals_the_host_path(dev, tmp_path):
    Image = pytest.importorskip("PIL.Image")
    from dan_amd.dataset import dataset_common as DC
    from dan_amd.dataset import jpeg as J
    from dan_amd.preprocessing import dan_preprocessing as P
    recs = []
    for i in range(8):
        h, w = 40 + i, 56
        rng = np.random.RandomState(i)
        img = (rng.rand(h // 8 + 1, w // 8 + 1, 3) * 255).astype(np.uint8).repeat(8, 0).repeat(8, 1)[:h, :w]
        b = io.BytesIO()
        Image.fromarray(img).save(b, format="JPEG", quality=95, progressive=i % 4 != 3)           # three progressive records in four
        boxes = [[0.1, 0.2, 0.5, 0.6], [0.3, 0.3, 0.9, 0.8]][: 1 + i % 2]
        k = len(boxes)
        recs.append(DC.convert_to_example("img%d.jpg" % i, b.getvalue(), boxes, [0] * k, [0] * k, [0] * k, [0] * k, [0] * k, [0] * k, h, w))
    DC.write_tfrecord(str(tmp_path / "wider_train-00000-of-00001"), recs)
    pattern = str(tmp_path / "wider_{}-*")
    decoders = []
    init = J.JpegDecoder.__init__

    def spy(self, *a, **kw):
        init(self, *a, **kw)
        decoders.append(self)

    def run(decode_device, **kw):
        draws, images = P.Draws(11), []

        def prep(image, bboxes):
            image = image if torch.is_tensor(image) else torch.from_numpy(image).to(dev)
            images.append(image.cpu())
            h, w = image.shape[:2]
            px = np.asarray(bboxes, np.float32).reshape(-1, 4) * np.asarray([h, w, h, w], np.float32)
            return P.preprocess_for_train(image, px, (128, 128), ANCHOR_SCALES, draws=draws)

        def encoder(b):
            return [np.zeros((5, 4), np.float32)], [np.ones((5,), np.int64)], [np.zeros((5,), np.float32)], [b]

        names, inputs = [], []
        for batch in DC.slim_get_batch(2, 4, "train", pattern, 2, 2, prep, encoder, num_epochs=1, is_training=True, seed=1,
                                       decode_device=decode_device, **kw):
            for e in batch:
                names.append(e[1])
                inputs.append(e[0].cpu())
        return names, inputs, images

    names_h, inputs_h, images_h = run(None)
    J.JpegDecoder.__init__ = spy
    try:
        names_d, inputs_d, images_d = run(dev, decode_progressive=True)
    finally:
        J.JpegDecoder.__init__ = init
    assert names_h == names_d and len(names_h) >= 4
    assert len(images_h) == len(images_d) and all(torch.equal(a, b) for a, b in zip(images_h, images_d))
    assert len(inputs_h) == len(inputs_d) and all(torch.equal(a, b) for a, b in zip(inputs_h, inputs_d))
    assert len(decoders) == 1 and decoders[0].stats["fallback"] == {} and decoders[0].stats["progressive"] == 6
